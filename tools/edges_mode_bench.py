"""attention="edges" against "nodes" and "graphs", in one process on the same batches and initial weights:

  * C4: the synthetic batches bench.py times (COLLAB-like, batch_size 64, num_neighbors 16, T 4, ff 1024, fwdh);
  * a molecule-like setting: MUTAG from dataset/, batch_size 64, the same model shape;
  * per setting, the fused trainer step (SupTrainer.step, dropout on) under each mode: a warm-up, then blocks of
    steps in rotating order, every step timed by device events; the median per mode;
  * the per-launch device time of u2gnn_csr_attn_fwd / _bwd alone at each batch's layer shape (REPS launches
    captured in one HIP graph), with nnz and sum_g n_g^2 of the batch, against the bytes the gather must move:
    every entry reads one K and one V row forward (nnz * dp * 4 * 2 B) and K, V, Qs, dO rows backward (twice that),
    beside the dense QKV / O / dO / dQKV traffic and the entries' indices and (backward) Pd, dS values.

--hops 1,2,3 adds, per H, the step of attention="edges" with hops=H (the H-hop pattern and the learned hop bias)
beside the three modes in the same rotation, and per batch and H: nnz, the CSR forward / backward on that pattern
without a bias and with a zero bias (the BIAS instantiations at equal arithmetic), and the u2gnn_bias_expand and
u2gnn_bias_table_grad launches for the step's T tables.  --settings picks the settings to run.

--pipeline times something else (and nothing of the above): edges-mode steps on fresh batches from a BatchLoader over
a GraphStore, with the adjacency resident, built on the host per batch, or assembled on the GPU per batch from the
store's DeviceGraphs, and the assemble kernel alone (pipeline() below); with --hops also per H.

Prints one JSON line.  Usage: python tools/edges_mode_bench.py [--steps 24] [--warmup 5] [--batches 4] [--hops 1,2]
[--settings c4,mutag] [--pipeline]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graph-transformer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from u2gnn_hip import kernels as K  # noqa: E402

REPS = 20
MODES = ("nodes", "graphs", "edges")


def graph_time_us(fn):
    """Device microseconds per call: REPS calls captured in one HIP graph, the second replay timed."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(REPS):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def bias_figures(adj, d, T, QKV, dO, O, stats, dQKV, N, Np, dp):
    """The kernels of the hop bias on one batch's H-hop pattern: the CSR forward / backward without and with a (zero)
    bias, and the two table kernels for T tables."""
    nnz, ld = adj.nnz, (adj.nnz + 3) // 4 * 4
    bias, dbias = torch.zeros(nnz, device="cuda"), torch.empty(nnz, device="cuda")
    qs = 1 / math.sqrt(d)
    out = {"nnz": nnz, "n_types": adj.n_types,
           "fwd_us": graph_time_us(lambda: K.csr_attn_fwd(QKV, dp, adj, O, stats, 0.5, 7, N, Np)),
           "fwd_bias_us": graph_time_us(lambda: K.csr_attn_fwd_bias(QKV, dp, adj, bias, O, stats, 0.5, 7, N, Np)),
           "bwd_us": graph_time_us(lambda: K.csr_attn_bwd(QKV, dp, adj, O, dO, stats, 0.5, 7, qs, dQKV, N, Np)),
           "bwd_bias_us": graph_time_us(lambda: K.csr_attn_bwd_bias(QKV, dp, adj, bias, O, dO, stats, 0.5, 7, qs, dQKV,
                                                                   dbias, N, Np))}
    tables, dtables = torch.zeros(T, adj.n_types, device="cuda"), torch.empty(T, adj.n_types, device="cuda")
    all_b = torch.empty(T, ld, device="cuda")
    out["bias_expand_us"] = graph_time_us(lambda: K.bias_expand(tables, adj.etype, all_b))
    out["bias_table_grad_us"] = graph_time_us(lambda: K.bias_table_grad(all_b, adj.etype, dtables))
    return {k: round(v, 2) if isinstance(v, float) else v for k, v in out.items()}


def kernel_figures(offsets, adj, d, hop_adjs=None, T=4):
    from u2gnn_hip.engine import row_pad, rup
    N, dp, nnz = int(offsets[-1]), rup(d, 64), adj.nnz
    Np = row_pad(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    QKV = torch.randn(Np, 3 * dp, device="cuda", generator=g)
    QKV[:, :dp] *= 1 / math.sqrt(dp)
    QKV[N:] = 0
    dO = torch.randn(Np, dp, device="cuda", generator=g)
    O, stats = torch.empty(Np, dp, device="cuda"), torch.empty(Np, 2, device="cuda")
    dQKV = torch.empty(Np, 3 * dp, device="cuda")
    fwd = graph_time_us(lambda: K.csr_attn_fwd(QKV, dp, adj, O, stats, 0.5, 7, N, Np))
    bwd = graph_time_us(lambda: K.csr_attn_bwd(QKV, dp, adj, O, dO, stats, 0.5, 7, 1 / math.sqrt(d), dQKV, N, Np))
    sq = float((np.diff(np.asarray(offsets)).astype(np.float64) ** 2).sum())
    f_gather, b_gather = nnz * dp * 4 * 2, nnz * dp * 4 * 4
    f_flop, b_flop = 2 * 2 * nnz * dp, 5 * 2 * nnz * dp
    return {"N": N, "graphs": len(offsets) - 1, "nnz": nnz, "mean_degree": round(nnz / N - 1, 2), "sum_ng2": sq,
            "fwd_us": round(fwd, 2), "fwd_gather_mb": round(f_gather / 1e6, 2),
            "fwd_gather_gbs": round(f_gather / fwd / 1e3, 1), "fwd_gflops": round(f_flop / fwd / 1e3, 1),
            "bwd_us": round(bwd, 2), "bwd_gather_mb": round(b_gather / 1e6, 2),
            "bwd_gather_gbs": round(b_gather / bwd / 1e3, 1), "bwd_gflops": round(b_flop / bwd / 1e3, 1),
            "hops": {str(h): bias_figures(a, d, T, QKV, dO, O, stats, dQKV, N, Np, dp)
                     for h, a in (hop_adjs or {}).items()}}


def time_steps(batches, d, C, T, ff, precision, args, hop_batches=None):
    """hop_batches: {H: the batches with the H-hop adjacency}; each adds the variant "edges_hH" (hops=H) to the
    rotation."""
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.train import SupTrainer
    variants = [(m, m, None, batches) for m in MODES]
    variants += [(f"edges_h{h}", "edges", h, bs) for h, bs in (hop_batches or {}).items()]
    names = tuple(v[0] for v in variants)
    trainers, feed = {}, {}
    for name, mode, hops, bs in variants:
        torch.manual_seed(123)
        m = TransformerU2GNN(d, ff, C, T, 0.5, 1, precision=precision, attention=mode, hops=hops).cuda().train()
        trainers[name], feed[name] = SupTrainer(m, lr=5e-4, max_norm=0.5, seed=123), bs
    nb = len(batches)
    for name, tr in trainers.items():
        for i in range(args.warmup):
            tr.step(feed[name][i % nb])
    torch.cuda.synchronize()
    times = {m: [] for m in names}
    done, blk = 0, 0
    while done < args.steps:
        r = blk % len(names)
        order = names[r:] + names[:r]
        n = min(args.block, args.steps - done)
        for mode in order:
            tr = trainers[mode]
            for i in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                tr.step(feed[mode][(done + i) % nb])
                e1.record()
                torch.cuda.synchronize()
                times[mode].append(e0.elapsed_time(e1))
        done += n
        blk += 1
    return ({k: round(statistics.median(v), 4) for k, v in times.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})


def setting(name, store, C, batch_size, k, args):
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import Adjacency, DeviceBatch
    T, ff = 4, 1024
    np.random.seed(123)
    loader = BatchLoader(store, batch_size, k)
    host = [loader() for _ in range(args.batches)]
    batches, hop_batches = [], {H: [] for H in args.hops}
    for h in host:
        b = DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device="cuda")
        b.adj = Adjacency.from_store(store, h.graph_ids, b.N, "cuda")
        batches.append(b)
        for H in args.hops:
            hb = DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device="cuda")
            hb.adj = Adjacency.from_store(store, h.graph_ids, hb.N, "cuda", hops=H)
            hop_batches[H].append(hb)
    d = host[0].X_concat.shape[1]
    med, rng = time_steps(batches, d, C, T, ff, args.precision, args, hop_batches)
    out = {"setting": f"{name}: bs {batch_size}, k {k}, d {d}, T {T}, ff {ff}, {args.precision}, {len(host)} batches, "
                      f"eager steps, median of {args.steps} per mode in rotating blocks of {args.block}",
           "step_ms": med, "step_ms_min_max": rng,
           "edges_over_nodes": round(med["edges"] / med["nodes"], 4),
           "edges_over_graphs": round(med["edges"] / med["graphs"], 4),
           "nnz": {"edges": [b.adj.nnz for b in batches],
                   **{f"edges_h{H}": [b.adj.nnz for b in bs] for H, bs in hop_batches.items()}},
           "kernels": [kernel_figures(h.offsets, b.adj, d, {H: bs[i].adj for H, bs in hop_batches.items()}, T)
                       for i, (h, b) in enumerate(list(zip(host, batches))[:2])]}
    return out


def assemble_figures(dg, ids):
    """u2gnn_adjacency_assemble alone on one batch: device time per launch (REPS launches in one HIP graph, events
    around its replay) and the bytes it moves -- per entry three int32 and, with hops, one byte read, three int64 and
    one int32 written; per row two int64 read and two written."""
    ids, row_off, ent_off, N, nnz, n_types = dg.plan(ids)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    gid, ro, eo = dev(ids), dev(row_off), dev(ent_off)
    out = [torch.empty(n, device="cuda", dtype=torch.int64) for n in (N + 1, nnz, N + 1, nnz, nnz)]
    et = torch.empty(nnz, device="cuda", dtype=torch.int32) if dg.hops else None
    us = graph_time_us(lambda: K.adjacency_assemble(dg.c_struct(), gid, ro, eo, N, nnz, *out, et, dg.err))
    moved = nnz * ((13 + 28) if dg.hops else (12 + 24)) + (N + 1) * 32
    return {"N": N, "nnz": nnz, "assemble_us": round(us, 2), "moved_mb": round(moved / 1e6, 3),
            "gbs": round(moved / us / 1e3, 1)}


def pipeline(name, store, C, batch_size, k, args, hops=None):
    """attention="edges" steps on FRESH batches from a BatchLoader over a GraphStore (native assembly into page-locked
    slots, DeviceBatch.from_store), three variants in rotating blocks of one process, one trainer:

      resident: --batches batches built up front and replayed (what the step figures above time);
      host:     every step draws a batch and builds its adjacency on the host (Adjacency.from_store) -- the CLIs'
                --adjacency host;
      device:   every step draws a batch and DeviceBatch.from_store(..., graphs=) assembles its adjacency on the GPU
                from the store's DeviceGraphs -- the CLIs' --adjacency device.

    A block is --block steps between two synchronisations, timed on the host clock (the host work is the subject);
    per variant the median of its blocks' per-step times.  pass: device no slower than host by more than the spread
    (max - min) of host's own blocks.  The structure's one-off build is timed apart."""
    import time
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import Adjacency, DeviceBatch
    from u2gnn_hip.pattern import DeviceGraphs
    from u2gnn_hip.train import SupTrainer
    T, ff = 4, 1024
    t0 = time.perf_counter()
    dg = DeviceGraphs.from_store(store, "cuda", hops=hops)
    build_s = time.perf_counter() - t0
    X_dev = torch.from_numpy(store.X).cuda()
    np.random.seed(123)
    loader = BatchLoader(store, batch_size, k, gather_x=False)
    resident = [DeviceBatch.from_store(loader(), X_dev, "cuda", graphs=dg) for _ in range(args.batches)]
    torch.manual_seed(123)
    m = TransformerU2GNN(store.d, ff, C, T, 0.5, 1, precision=args.precision, attention="edges", hops=hops).cuda().train()
    tr = SupTrainer(m, lr=5e-4, max_norm=0.5, seed=123)
    count = [0]

    def feed_resident():
        count[0] += 1
        return resident[count[0] % len(resident)]

    def feed_host():
        hb = loader()
        b = DeviceBatch.from_store(hb, X_dev, "cuda")
        b.adj = Adjacency.from_store(store, hb.graph_ids, b.N, "cuda", hops)
        return b

    def feed_device():
        return DeviceBatch.from_store(loader(), X_dev, "cuda", graphs=dg)
    feeds = {"resident": feed_resident, "host": feed_host, "device": feed_device}
    names = tuple(feeds)
    for f in feeds.values():
        for _ in range(args.warmup):
            tr.step(f())
    torch.cuda.synchronize()
    blocks = {n: [] for n in names}
    done, blk = 0, 0
    while done < args.steps:
        r = blk % len(names)
        n = min(args.block, args.steps - done)
        for v in names[r:] + names[:r]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step(feeds[v]())
            torch.cuda.synchronize()
            blocks[v].append((time.perf_counter() - t0) * 1e3 / n)
        done += n
        blk += 1
    med = {v: statistics.median(t) for v, t in blocks.items()}
    spread = max(blocks["host"]) - min(blocks["host"])
    dg.check_indices()
    return {"setting": f"{name}: bs {batch_size}, k {k}, d {store.d}, T {T}, ff {ff}, {args.precision}, hops {hops}, "
                       f"fresh batches, {args.steps} steps per variant in rotating blocks of {args.block}, host clock",
            "structure": {"graphs": dg.G, "nodes": dg.V, "entries": dg.E, "mb": round(dg.nbytes(dg.G, dg.V, dg.E, hops) / 1e6, 2),
                          "build_s": round(build_s, 3)},
            "step_ms": {v: round(t, 4) for v, t in med.items()},
            "block_ms_min_max": {v: [round(min(t), 4), round(max(t), 4)] for v, t in blocks.items()},
            "device_over_resident": round(med["device"] / med["resident"], 4),
            "host_over_resident": round(med["host"] / med["resident"], 4),
            "host_block_spread_ms": round(spread, 4),
            "pass": bool(med["device"] <= med["host"] + spread),
            "assemble": assemble_figures(dg, loader.rng.permutation(dg.G)[:batch_size])}


def main_pipeline(args, which):
    import util
    from u2gnn_hip.batching import GraphStore
    from u2gnn_hip.synthetic import as_graph_store, collab_like
    stores = {}
    if "mutag" in which:
        graphs, C = util.load_data("MUTAG", False)
        stores["mutag"] = ("MUTAG", GraphStore(graphs), C)
    if "c4" in which:
        stores["c4"] = ("C4 synthetic as a GraphStore", as_graph_store(collab_like(seed=0)), 3)
    out = {}
    for H in [None] + args.hops:
        res = out["pipeline" if H is None else f"pipeline_h{H}"] = {}
        for key, (name, store, C) in stores.items():
            res[key] = pipeline(name, store, C, 64, 16, args, H)
            print(f"{key} hops {H}: {res[key]['step_ms']}", file=sys.stderr, flush=True)   # progress; the JSON is the result
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pipeline", action="store_true",
                    help="instead: time edges-mode steps on fresh batches -- resident, host-built and device-built "
                         "adjacency -- and the assemble kernel alone (see pipeline())")
    ap.add_argument("--steps", type=int, default=24, help="timed steps per mode (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--block", type=int, default=4, help="steps per rotation block")
    ap.add_argument("--precision", default="fwdh")
    ap.add_argument("--hops", default="", help="comma-separated H values: also time attention='edges' with hops=H")
    ap.add_argument("--settings", default="c4,mutag", help="which of c4, mutag to run")
    args = ap.parse_args()
    args.hops = [int(h) for h in args.hops.split(",") if h]
    which = args.settings.split(",")
    assert torch.cuda.is_available(), "needs an MI355X: a timing without one would mean nothing"
    if args.pipeline:
        return main_pipeline(args, which)
    import util
    from u2gnn_hip.batching import GraphStore
    from u2gnn_hip.synthetic import collab_like
    graphs, C = util.load_data("MUTAG", False)
    out = {}
    if "c4" in which:
        out["c4"] = setting("C4 synthetic", collab_like(seed=0), 3, 64, 16, args)
    if "mutag" in which:
        out["mutag"] = setting("MUTAG", GraphStore(graphs), C, 64, 16, args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
