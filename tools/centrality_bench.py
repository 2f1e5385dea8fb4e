"""What ``centrality`` costs, in one process on the same batches and initial weights:

  * C4: the synthetic batches bench.py times (COLLAB-like, batch_size 64, num_neighbors 16, T 4, ff 1024, fwdh) and
    MUTAG from dataset/ at batch_size 64 with the same model shape;
  * per setting, the fused trainer step (SupTrainer.step, dropout on) of attention="nodes" and "edges", each without
    and with centrality=16: a warm-up, then blocks of steps in rotating order, every step timed by device events; the
    median per variant;
  * the two new launches alone at each batch's shape (REPS launches captured in one HIP graph): u2gnn_gather_rows
    beside u2gnn_gather_rows_emb, and u2gnn_class_rows_grad (both of its launches);
  * layer (0, 0)'s backward (native executor, attention="nodes", no side stream) with and without its input gradient.

--off-step times something else (and nothing of the above): only the centrality-off steps of "nodes" and "edges", through
nothing this feature added, so that the same file runs against another build of the package (--pkg PATH: the
directory that holds u2gnn_hip/ and its lib/) -- this build and the parent commit's as alternating processes.

Prints one JSON line.  Usage: python tools/centrality_bench.py [--steps 24] [--warmup 5] [--batches 4]
[--settings c4,mutag] [--off-step] [--pkg DIR] [--label NAME]"""
import argparse
import json
import os
import statistics
import sys

_ap = argparse.ArgumentParser()
_ap.add_argument("--off-step", action="store_true", help="only the centrality-off steps (runs against any build)")
_ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "graph-transformer_amd"), help="the package directory to time")
_ap.add_argument("--label", default="this build", help="--off-step: the build's name in the result")
_ap.add_argument("--steps", type=int, default=24, help="timed steps per variant (>= 20)")
_ap.add_argument("--warmup", type=int, default=5)
_ap.add_argument("--batches", type=int, default=4)
_ap.add_argument("--block", type=int, default=4, help="steps per rotation block")
_ap.add_argument("--precision", default="fwdh")
_ap.add_argument("--depth", type=int, default=16, help="the centrality keyword's D")
_ap.add_argument("--settings", default="c4,mutag", help="which of c4, mutag to run")
ARGS = _ap.parse_args()
sys.path[:0] = [os.path.abspath(ARGS.pkg)]
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


def time_steps(variants, args):
    """variants: {name: (trainer, batches)}; -> (median ms, [min, max]) per name, steps in rotating blocks."""
    names = tuple(variants)
    nb = len(next(iter(variants.values()))[1])
    for tr, bs in variants.values():
        for i in range(args.warmup):
            tr.step(bs[i % nb])
    torch.cuda.synchronize()
    times = {m: [] for m in names}
    done, blk = 0, 0
    while done < args.steps:
        r = blk % len(names)
        n = min(args.block, args.steps - done)
        for name in names[r:] + names[:r]:
            tr, bs = variants[name]
            for i in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                tr.step(bs[(done + i) % nb])
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        done += n
        blk += 1
    return ({k: round(statistics.median(v), 4) for k, v in times.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})


def kernel_figures(b, d, depth):
    """The two new launches at one batch's shape (slot-0 rows: "nodes" / "edges"), and the bytes they move."""
    from u2gnn_hip.engine import row_pad, rup
    N, dp = b.N, rup(d, 64)
    Np = row_pad(N)
    X = torch.empty(Np, dp, device="cuda")
    table = torch.randn(depth + 1, d, device="cuda")
    dX = torch.randn(Np, dp, device="cuda")
    demb = torch.empty(depth + 1, d, device="cuda")
    stride = b.idx_stride
    plain = graph_time_us(lambda: K.gather_rows(b.X_concat, b.input_x, stride, X, N, Np, d, dp, b.err))
    emb = graph_time_us(lambda: K.gather_rows_emb(b.X_concat, b.input_x, stride, X, N, Np, d, dp, b.deg, table, b.err))
    grad = graph_time_us(lambda: K.class_rows_grad(dX, b.input_x, stride, b.deg, N, N, d, demb))
    moved = N * d * 4 + Np * dp * 4
    return {"N": N, "d": d, "classes": depth + 1, "gather_rows_us": round(plain, 2), "gather_rows_emb_us": round(emb, 2),
            "gather_mb": round(moved / 1e6, 2), "gather_rows_emb_gbs": round(moved / emb / 1e3, 1),
            "class_rows_grad_us": round(grad, 2), "class_rows_grad_read_mb": round(N * d * 4 / 1e6, 2),
            "class_rows_grad_gbs": round(N * d * 4 / grad / 1e3, 1)}


def layer00_figures(b, d, C, T, ff, precision):
    """Layer (0, 0)'s backward through the native executor on one batch, with and without its input gradient."""
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip import native
    from u2gnn_hip.core import LAYER_KEYS
    from u2gnn_hip.engine import LayerParams
    from u2gnn_hip.engine import deep_wgrad as engine_deep_wgrad
    torch.manual_seed(123)
    m = TransformerU2GNN(d, ff, C, T, 0.5, 1, precision=precision).cuda().train()
    flat = m.flatten_parameters()
    stack = m.core.stack
    _, ctx = stack.forward(b, True, True, 7)
    lc, ldims = ctx["layers"][0][0], ctx["ldims"]
    g = LayerParams(*[flat.grads["u2gnn_layers.0.layers.0." + k] for k in LAYER_KEYS])
    dX2 = torch.randn(ldims.Np, ldims.dp, device="cuda")
    dX2[ldims.N:] = 0
    out = {}
    for need_dx in (False, True):
        out["need_dx" if need_dx else "no_dx"] = round(graph_time_us(
            lambda: native.layer_backward(dX2, lc, stack.packed[0][0], stack.layer_params(0, 0), g, ldims, precision,
                                          side=None, deep_wgrad=engine_deep_wgrad(), need_dx=need_dx)), 2)
    out["extra_us"] = round(out["need_dx"] - out["no_dx"], 2)
    return out


def setting(name, store, C, batch_size, k, args):
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import Adjacency, DeviceBatch
    from u2gnn_hip.train import SupTrainer
    T, ff = 4, 1024
    np.random.seed(123)
    loader = BatchLoader(store, batch_size, k)
    host = [loader() for _ in range(args.batches)]
    batches = []
    for h in host:
        kw = {} if args.off_step else {"degrees": store.degrees_of(h.graph_ids)}
        b = DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device="cuda", **kw)
        b.adj = Adjacency.from_store(store, h.graph_ids, b.N, "cuda")
        batches.append(b)
    d = host[0].X_concat.shape[1]
    variants = {}
    for mode in ("nodes", "edges"):
        for depth in (None,) if args.off_step else (None, args.depth):
            torch.manual_seed(123)
            mkw = {} if depth is None else {"centrality": depth}
            m = TransformerU2GNN(d, ff, C, T, 0.5, 1, precision=args.precision, attention=mode, **mkw).cuda().train()
            variants[mode if depth is None else f"{mode}_c{depth}"] = (SupTrainer(m, lr=5e-4, max_norm=0.5, seed=123),
                                                                      batches)
    med, rng = time_steps(variants, args)
    out = {"setting": f"{name}: bs {batch_size}, k {k}, d {d}, T {T}, ff {ff}, {args.precision}, {len(host)} batches, "
                      f"eager steps, median of {args.steps} per variant in rotating blocks of {args.block}",
           "step_ms": med, "step_ms_min_max": rng}
    if not args.off_step:
        D = args.depth
        out["centrality_over_off"] = {mode: round(med[f"{mode}_c{D}"] / med[mode], 4) for mode in ("nodes", "edges")}
        out["kernels"] = [kernel_figures(b, d, D) for b in batches[:2]]
        out["layer00_bwd_us"] = [layer00_figures(b, d, C, T, ff, args.precision) for b in batches[:2]]
    return out


def main():
    args = ARGS
    assert torch.cuda.is_available(), "needs an MI355X: a timing without one would mean nothing"
    import util
    from u2gnn_hip.batching import GraphStore
    from u2gnn_hip.synthetic import collab_like
    which = args.settings.split(",")
    out = {"build": args.label} if args.off_step else {}
    if "c4" in which:
        out["c4"] = setting("C4 synthetic", collab_like(seed=0), 3, 64, 16, args)
    if "mutag" in which:
        graphs, C = util.load_data("MUTAG", False)
        out["mutag"] = setting("MUTAG", GraphStore(graphs), C, 64, 16, args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
