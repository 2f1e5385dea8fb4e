"""attention="graphs" against attention="nodes" on the C4 synthetic batches bench.py times (COLLAB-like, batch_size
64, num_neighbors 16, T 4, ff 1024, fwdh), in one process on the same batches and initial weights:

  * the fused trainer step (SupTrainer.step, dropout on) under each mode: a warm-up, then blocks of steps in
    alternating order (nodes, graphs / graphs, nodes / ...), every step timed by device events; the median per mode;
  * the per-launch device time of u2gnn_segment_attn_fwd / _bwd at each batch's layer shape (REPS launches captured
    in one HIP graph) against their algorithmic work: 2 * sum_g n_g^2 * dp FLOP per product (2 products forward, 5
    backward: P is recomputed) and the QKV / O / dO / dQKV bytes.

With --distances H (attention="graphs" with a learned bias per shortest-path distance) it measures that mode instead,
per setting (c4: the same synthetic graphs as a GraphStore; mutag: MUTAG from dataset/ at batch_size 64):

  * the segment kernels alone, without bias and as the BIAS instantiation at a zero table (equal arithmetic), beside the
    CSR kernels over the --csr_hops adjacency of the same batch with a zero bias (on C4 two hops reach every node: the
    same pairs), u2gnn_bias_expand and u2gnn_bias_table_grad for the step's T tables;
  * the eager step under graphs, graphs + distances=H and edges + hops, median over rotating blocks in one process;
  * the host cost of PairTypes.from_store per batch with cached blocks (host clock to the return of the call, and to a
    device synchronise after it).

With --distances H --pipeline it times distances steps on FRESH batches instead (``pair_pipeline``): the pair types
resident, built on the host per batch (PairTypes.from_store) or searched on the GPU per batch (DeviceGraphs.pair_types
through DeviceBatch.from_store), and u2gnn_pair_distances alone.  With --build it gives the wall time of
DeviceGraphs.from_store(hops=H) built on the host against build="device" (``structure_builds``).

Prints one JSON line.  Usage: python tools/graphs_mode_bench.py [--steps 24] [--warmup 5] [--batches 4]
       python tools/graphs_mode_bench.py --distances 3 [--settings c4,mutag] [--csr_hops 2]
       python tools/graphs_mode_bench.py --distances 3 --pipeline [--steps 32] [--settings c4,mutag]
       python tools/graphs_mode_bench.py --build c4:2,c4:3,ptc:3,ptc:31"""
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


def kernel_figures(offsets, d):
    from u2gnn_hip.engine import row_pad, rup
    N, dp = int(offsets[-1]), rup(d, 64)
    Np = row_pad(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    QKV = torch.randn(Np, 3 * dp, device="cuda", generator=g)
    QKV[:, :dp] *= 1 / math.sqrt(dp)
    QKV[N:] = 0
    dO = torch.randn(Np, dp, device="cuda", generator=g)
    O, stats = torch.empty(Np, dp, device="cuda"), torch.empty(Np, 2, device="cuda")
    dQKV = torch.empty(Np, 3 * dp, device="cuda")
    off = torch.as_tensor(np.asarray(offsets), dtype=torch.int64).cuda()
    fwd = graph_time_us(lambda: K.segment_attn_fwd(QKV, dp, off, O, stats, 0.5, 7, N, Np))
    bwd = graph_time_us(lambda: K.segment_attn_bwd(QKV, dp, off, O, dO, stats, 0.5, 7, 1 / math.sqrt(d), dQKV, N, Np))
    sq = float((np.diff(np.asarray(offsets)).astype(np.float64) ** 2).sum())
    f_flop, b_flop = 2 * 2 * sq * dp, 5 * 2 * sq * dp
    f_bytes = (Np * 3 * dp + Np * dp + 2 * Np) * 4
    b_bytes = (Np * 3 * dp + 2 * Np * dp + 2 * Np + Np * 3 * dp) * 4
    return {"N": N, "graphs": len(offsets) - 1, "sum_ng2": sq, "dense_N2": float(N) ** 2,
            "fwd_us": round(fwd, 2), "fwd_gflop": round(f_flop / 1e9, 4), "fwd_tflops": round(f_flop / fwd / 1e6, 3),
            "fwd_mb": round(f_bytes / 1e6, 2), "fwd_gbs": round(f_bytes / fwd / 1e3, 1),
            "bwd_us": round(bwd, 2), "bwd_gflop": round(b_flop / 1e9, 4), "bwd_tflops": round(b_flop / bwd / 1e6, 3),
            "bwd_mb": round(b_bytes / 1e6, 2), "bwd_gbs": round(b_bytes / bwd / 1e3, 1)}


def distance_kernel_figures(offsets, pairs, adj, d, T):
    """The segment kernels on one batch's layer shape without bias and with a zero bias, the CSR kernels over ``adj``
    with a zero bias, and the two table kernels over the pair types."""
    from u2gnn_hip.engine import row_pad, rup
    N, dp = int(offsets[-1]), rup(d, 64)
    Np = row_pad(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    QKV = torch.randn(Np, 3 * dp, device="cuda", generator=g)
    QKV[:, :dp] *= 1 / math.sqrt(dp)
    QKV[N:] = 0
    dO = torch.randn(Np, dp, device="cuda", generator=g)
    O, stats = torch.empty(Np, dp, device="cuda"), torch.empty(Np, 2, device="cuda")
    dQKV = torch.empty(Np, 3 * dp, device="cuda")
    off = torch.as_tensor(np.asarray(offsets), dtype=torch.int64).cuda()
    qs = 1 / math.sqrt(d)
    po, n = pairs.pair_off, pairs.n_pairs
    zero, db = torch.zeros(n, device="cuda"), torch.empty(n, device="cuda")
    zc, dbc = torch.zeros(adj.nnz, device="cuda"), torch.empty(adj.nnz, device="cuda")
    tables = torch.zeros(T, pairs.n_types, device="cuda")
    rows = torch.empty(T, rup(n, 4), device="cuda")
    dt = torch.empty(T, pairs.n_types, device="cuda")
    t = {
        "fwd_us": graph_time_us(lambda: K.segment_attn_fwd(QKV, dp, off, O, stats, 0.5, 7, N, Np)),
        "fwd_zero_bias_us": graph_time_us(lambda: K.segment_attn_fwd_bias(QKV, dp, off, po, zero, O, stats, 0.5, 7, N,
                                                                          Np)),
        "bwd_us": graph_time_us(lambda: K.segment_attn_bwd(QKV, dp, off, O, dO, stats, 0.5, 7, qs, dQKV, N, Np)),
        "bwd_zero_bias_us": graph_time_us(lambda: K.segment_attn_bwd_bias(QKV, dp, off, po, zero, O, dO, stats, 0.5, 7,
                                                                          qs, dQKV, db, N, Np)),
        "bwd_zero_bias_no_dbias_us": graph_time_us(lambda: K.segment_attn_bwd_bias(QKV, dp, off, po, zero, O, dO, stats,
                                                                                   0.5, 7, qs, dQKV, None, N, Np)),
        "csr_fwd_zero_bias_us": graph_time_us(lambda: K.csr_attn_fwd_bias(QKV, dp, adj, zc, O, stats, 0.5, 7, N, Np)),
        "csr_bwd_zero_bias_us": graph_time_us(lambda: K.csr_attn_bwd_bias(QKV, dp, adj, zc, O, dO, stats, 0.5, 7, qs,
                                                                          dQKV, dbc, N, Np)),
        "expand_us": graph_time_us(lambda: K.bias_expand(tables, pairs.etype, rows)),
        "table_grad_us": graph_time_us(lambda: K.bias_table_grad(rows, pairs.etype, dt)),
    }
    out = {"N": N, "dp": dp, "graphs": len(offsets) - 1, "pairs": n, "csr_nnz": adj.nnz,
           "bias_mb": round(4 * n / 1e6, 3)}
    out.update({k: round(v, 2) for k, v in t.items()})
    out["fwd_bias_over_plain"] = round(t["fwd_zero_bias_us"] / t["fwd_us"], 4)
    out["bwd_bias_over_plain"] = round(t["bwd_zero_bias_us"] / t["bwd_us"], 4)
    out["csr_over_segment_fwd"] = round(t["csr_fwd_zero_bias_us"] / t["fwd_zero_bias_us"], 4)
    out["csr_over_segment_bwd"] = round(t["csr_bwd_zero_bias_us"] / t["bwd_zero_bias_us"], 4)
    return out


def distance_setting(name, store, C, batch_size, k, args):
    import time

    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import Adjacency, DeviceBatch, PairTypes
    from u2gnn_hip.train import SupTrainer
    T, ff, H = 4, 1024, args.distances
    np.random.seed(123)
    loader = BatchLoader(store, batch_size, k)
    host = [loader() for _ in range(args.batches)]
    batches = []
    for h in host:
        b = DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device="cuda")
        b.pairs = PairTypes.from_store(store, h.graph_ids, b.N, "cuda", H)
        b.adj = Adjacency.from_store(store, h.graph_ids, b.N, "cuda", hops=args.csr_hops)
        batches.append(b)
    d = host[0].X_concat.shape[1]
    # the host cost per batch, blocks cached (the loop above computed them)
    ret, synced = [], []
    for i in range(5 * len(host)):
        h = host[i % len(host)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pt = PairTypes.from_store(store, h.graph_ids, int(h.offsets[-1]), "cuda", H)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ret.append((t1 - t0) * 1e3), synced.append((t2 - t0) * 1e3)
        del pt
    variants = [("graphs", dict(attention="graphs")), (f"graphs_d{H}", dict(attention="graphs", distances=H)),
                (f"edges_h{args.csr_hops}", dict(attention="edges", hops=args.csr_hops))]
    names = tuple(v[0] for v in variants)
    trainers = {}
    for vname, kw in variants:
        torch.manual_seed(123)
        m = TransformerU2GNN(d, ff, C, T, 0.5, 1, precision=args.precision, **kw).cuda().train()
        trainers[vname] = SupTrainer(m, lr=5e-4, max_norm=0.5, seed=123)
    nb = len(batches)
    for tr in trainers.values():
        for i in range(args.warmup):
            tr.step(batches[i % nb])
    torch.cuda.synchronize()
    times = {v: [] for v in names}
    done, blk = 0, 0
    while done < args.steps:
        r = blk % len(names)
        n = min(args.block, args.steps - done)
        for vname in names[r:] + names[:r]:
            for i in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                trainers[vname].step(batches[(done + i) % nb])
                e1.record()
                torch.cuda.synchronize()
                times[vname].append(e0.elapsed_time(e1))
        done += n
        blk += 1
    med = {v: round(statistics.median(x), 4) for v, x in times.items()}
    return {"setting": f"{name}: bs {batch_size}, k {k}, d {d}, T {T}, ff {ff}, {args.precision}, {nb} batches, eager "
                       f"steps, median of {args.steps} per variant in rotating blocks of {args.block}",
            "step_ms": med, "step_ms_min_max": {v: [round(min(x), 4), round(max(x), 4)] for v, x in times.items()},
            "distances_over_graphs": round(med[names[1]] / med[names[0]], 4),
            "distances_over_edges_hops": round(med[names[1]] / med[names[2]], 4),
            "pairs": [b.pairs.n_pairs for b in batches], "csr_nnz": [b.adj.nnz for b in batches],
            "pair_types_from_store_ms": {"to_return_median": round(statistics.median(ret), 4),
                                         "to_device_sync_median": round(statistics.median(synced), 4),
                                         "min_max_to_sync": [round(min(synced), 4), round(max(synced), 4)],
                                         "calls": len(ret)},
            "kernels": [distance_kernel_figures(h.offsets, b.pairs, b.adj, d, T)
                        for h, b in list(zip(host, batches))[:2]]}


def pair_pipeline(name, store, C, batch_size, k, args):
    """attention="graphs" with distances=H steps on FRESH batches from a BatchLoader over a GraphStore, three variants
    in rotating blocks of one process, one trainer:

      resident: --batches batches built up front and replayed;
      host:     every step draws a batch and builds its pair types on the host (PairTypes.from_store, blocks cached
                after the warm-up passes) -- the CLIs' --adjacency host;
      device:   every step draws a batch and DeviceBatch.from_store(..., graphs=, distances=H) searches its pair types
                on the GPU -- the CLIs' --adjacency device.

    A block is --block steps between two synchronisations, timed on the host clock; per variant the median of its
    blocks' per-step times.  pass: device no slower than host by more than the spread (max - min) of host's own
    blocks.  The one-hop structure's build and its extents are timed apart; u2gnn_pair_distances alone is timed as
    REPS launches in one HIP graph."""
    import time
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch, PairTypes
    from u2gnn_hip.pattern import DeviceGraphs
    from u2gnn_hip.train import SupTrainer
    T, ff, H = 4, 1024, args.distances
    t0 = time.perf_counter()
    dg = DeviceGraphs.from_store(store, "cuda")
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    dg.extents()
    extents_s = time.perf_counter() - t0
    X_dev = torch.from_numpy(store.X).cuda()
    np.random.seed(123)
    loader = BatchLoader(store, batch_size, k, gather_x=False)
    resident = [DeviceBatch.from_store(loader(), X_dev, "cuda", graphs=dg, distances=H) for _ in range(args.batches)]
    torch.manual_seed(123)
    m = TransformerU2GNN(store.d, ff, C, T, 0.5, 1, precision=args.precision, attention="graphs", distances=H)
    tr = SupTrainer(m.cuda().train(), lr=5e-4, max_norm=0.5, seed=123)
    count = [0]

    def feed_resident():
        count[0] += 1
        return resident[count[0] % len(resident)]

    def feed_host():
        hb = loader()
        b = DeviceBatch.from_store(hb, X_dev, "cuda")
        b.pairs = PairTypes.from_store(store, hb.graph_ids, b.N, "cuda", H)
        return b

    def feed_device():
        return DeviceBatch.from_store(loader(), X_dev, "cuda", graphs=dg, distances=H)
    feeds = {"resident": feed_resident, "host": feed_host, "device": feed_device}
    names = tuple(feeds)
    t0 = time.perf_counter()
    store.distances(np.arange(dg.G), H)                        # the host path's blocks, all cached before the timing
    host_cache_s = time.perf_counter() - t0
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
    ids, row_off, pair_off, N, n_pairs, max_n = dg.plan_pairs(loader.rng.permutation(dg.G)[:batch_size], H)
    to = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    gid, ro, po = to(ids), to(row_off), to(pair_off)
    et = torch.empty(n_pairs, device="cuda", dtype=torch.int32)
    us = graph_time_us(lambda: K.pair_distances(dg.c_struct(), gid, ro, po, N, n_pairs, max_n, H, et, dg.err))
    return {"setting": f"{name}: bs {batch_size}, k {k}, d {store.d}, T {T}, ff {ff}, {args.precision}, distances {H}, "
                       f"fresh batches, {args.steps} steps per variant in rotating blocks of {args.block}, host clock",
            "structure": {"graphs": dg.G, "nodes": dg.V, "entries": dg.E, "one_hop_build_s": round(build_s, 3),
                          "extents_s": round(extents_s, 3), "host_blocks_all_graphs_s": round(host_cache_s, 3)},
            "step_ms": {v: round(t, 4) for v, t in med.items()},
            "block_ms_min_max": {v: [round(min(t), 4), round(max(t), 4)] for v, t in blocks.items()},
            "device_over_resident": round(med["device"] / med["resident"], 4),
            "host_over_resident": round(med["host"] / med["resident"], 4),
            "host_block_spread_ms": round(spread, 4),
            "pass": bool(med["device"] <= med["host"] + spread),
            "pair_distances": {"rows": N, "pairs": n_pairs, "max_nodes": max_n, "us": round(us, 2)}}


def structure_builds(args):
    """The wall time of DeviceGraphs.from_store(hops=H), built on the host and with build="device", one run each in
    this process after a warm-up build of MUTAG; the results compared integer for integer."""
    import time
    import util
    from u2gnn_hip.batching import GraphStore
    from u2gnn_hip.pattern import DeviceGraphs
    from u2gnn_hip.synthetic import as_graph_store, collab_like
    stores = {"mutag": lambda: GraphStore(util.load_data("MUTAG", False)[0]),
              "ptc": lambda: GraphStore(util.load_data("PTC", False)[0]),
              "c4": lambda: as_graph_store(collab_like(seed=0))}
    for b in ("host", "device"):
        DeviceGraphs.from_store(stores["mutag"](), "cuda", hops=2, build=b)
    torch.cuda.synchronize()
    out = []
    for item in args.build.split(","):
        name, H = item.split(":")
        H = int(H)
        row = {"store": name, "hops": H}
        built = {}
        for b in ("device", "host"):
            store = stores[name]()                              # a fresh store: no cached hop lists
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            built[b] = DeviceGraphs.from_store(store, "cuda", hops=H, build=b, scratch_bytes=args.scratch_mb << 20)
            torch.cuda.synchronize()
            row[f"{b}_s"] = round(time.perf_counter() - t0, 3)
        dv, hs = built["device"], built["host"]
        row.update(graphs=dv.G, nodes=dv.V, entries=dv.E, chunks=dv.last_expand[0],
                   scratch_mb=round(dv.last_expand[1] / 2 ** 20, 1), host_over_device=round(row["host_s"] / row["device_s"], 2),
                   equal=bool(all(np.array_equal(dv.host[k], hs.host[k]) for k in dv.ARRAYS)
                              and np.array_equal(dv.max_dist, hs.max_dist) and np.array_equal(dv.n_entries, hs.n_entries)))
        out.append(row)
        del built, dv, hs
    print(json.dumps({"structure_builds": out}), flush=True)


def distances_main(args):
    import util
    from u2gnn_hip.batching import GraphStore
    from u2gnn_hip.synthetic import as_graph_store, collab_like
    out = {"distances": args.distances, "csr_hops": args.csr_hops}
    run = pair_pipeline if args.pipeline else distance_setting
    for which in args.settings.split(","):
        if which == "c4":
            out["c4"] = run("C4 synthetic as a GraphStore", as_graph_store(collab_like(seed=0)), 3, 64, 16, args)
        elif which == "mutag":
            graphs, C = util.load_data("MUTAG", False)
            out["mutag"] = run("MUTAG", GraphStore(graphs), C, 64, 16, args)
        else:
            raise SystemExit(f"unknown setting {which!r}")
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24, help="timed steps per mode (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--block", type=int, default=4, help="steps per alternation block")
    ap.add_argument("--precision", default="fwdh")
    ap.add_argument("--distances", type=int, default=0, help="H: measure attention='graphs' with distances=H instead")
    ap.add_argument("--settings", default="c4,mutag", help="with --distances: which of c4, mutag to run")
    ap.add_argument("--csr_hops", type=int, default=2, help="with --distances: the edges + hops route beside it")
    ap.add_argument("--pipeline", action="store_true", help="with --distances: fresh batches, host against device")
    ap.add_argument("--build", default="", help="instead: time DeviceGraphs.from_store(hops=H) on the host and on the "
                                                "device for store:H items of c4, ptc, mutag")
    ap.add_argument("--scratch_mb", type=int, default=256, help="with --build: the device build's dense scratch")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a timing without one would mean nothing"
    if args.build:
        return structure_builds(args)
    if args.distances:
        return distances_main(args)
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.synthetic import collab_like
    from u2gnn_hip.train import SupTrainer
    d, C, T, ff = 367, 3, 4, 1024
    np.random.seed(123)
    loader = BatchLoader(collab_like(seed=0), 64, 16)
    host = [loader() for _ in range(args.batches)]
    batches = [DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device="cuda") for h in host]
    trainers = {}
    for mode in ("nodes", "graphs"):
        torch.manual_seed(123)
        m = TransformerU2GNN(d, ff, C, T, 0.5, 1, precision=args.precision, attention=mode).cuda().train()
        trainers[mode] = SupTrainer(m, lr=5e-4, max_norm=0.5, seed=123)
    nb = len(batches)
    for mode, tr in trainers.items():
        for i in range(args.warmup):
            tr.step(batches[i % nb])
    torch.cuda.synchronize()
    times = {"nodes": [], "graphs": []}
    done, blk = 0, 0
    while done < args.steps:
        order = ("nodes", "graphs") if blk % 2 == 0 else ("graphs", "nodes")
        n = min(args.block, args.steps - done)
        for mode in order:
            tr = trainers[mode]
            for i in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                tr.step(batches[(done + i) % nb])
                e1.record()
                torch.cuda.synchronize()
                times[mode].append(e0.elapsed_time(e1))
        done += n
        blk += 1
    out = {"config": f"C4 synthetic: bs 64, k 16, T {T}, ff {ff}, {args.precision}, {nb} batches, eager steps, "
                     f"median of {args.steps} per mode in alternating blocks of {args.block}",
           "step_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "step_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "kernels": [kernel_figures(h.offsets, d) for h in host[:2]]}
    out["graphs_over_nodes"] = round(out["step_ms"]["graphs"] / out["step_ms"]["nodes"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
