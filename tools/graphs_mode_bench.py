"""attention="graphs" against attention="nodes" on the C4 synthetic batches bench.py times (COLLAB-like, batch_size
64, num_neighbors 16, T 4, ff 1024, fwdh), in one process on the same batches and initial weights:

  * the fused trainer step (SupTrainer.step, dropout on) under each mode: a warm-up, then blocks of steps in
    alternating order (nodes, graphs / graphs, nodes / ...), every step timed by device events; the median per mode;
  * the per-launch device time of u2gnn_segment_attn_fwd / _bwd at each batch's layer shape (REPS launches captured
    in one HIP graph) against their algorithmic work: 2 * sum_g n_g^2 * dp FLOP per product (2 products forward, 5
    backward: P is recomputed) and the QKV / O / dO / dQKV bytes.

Prints one JSON line.  Usage: python tools/graphs_mode_bench.py [--steps 24] [--warmup 5] [--batches 4]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24, help="timed steps per mode (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--block", type=int, default=4, help="steps per alternation block")
    ap.add_argument("--precision", default="fwdh")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a timing without one would mean nothing"
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
