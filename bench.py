#!/usr/bin/env python
"""U2GNN-Sup training throughput on MI355X — BASELINE.json metric
"graphs/sec (fwd+bwd) U2GNN-Sup COLLAB k=16 T=4 at 1/2/4/8 MI355X".

Workload: COLLAB supervised, batch_size=64 graphs per GPU, num_neighbors=16,
num_timesteps=4, ff_hidden_size=1024, d=367 (degree-as-tag one-hot), 3 classes, dropout 0.5,
Adam lr 5e-4 + clip_grad_norm_(0.5).  COLLAB itself is not in the image, so the graphs are the
synthetic COLLAB-like set of u2gnn_hip.synthetic (published statistics); weights random-init.

A step = forward + smoothed-CE loss + backward + (DP: gradient all-reduce over RCCL) + clip + Adam
over one 64-graph batch per rank; batches are pre-assembled and resident in HBM before timing.
Data-parallel: one process per GPU, each rank trains its own 64-graph batch (weak scaling; the
attention couples all graphs of a batch, so a batch never splits across GPUs).

Usage: python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
  A plain run sets up, warms up, times the K steps and prints the result line.  --full adds everything else the
  line can carry (CPU baseline, the other precision policies, the on-the-fly pipeline, the other BASELINE configs,
  the neighbour-attention line, the live roofline probes and the gather roofline); the switches below
  (--cpu-baseline, --fp32-steps, --pipeline-steps, --configs, --neighbors-line, --no-roofline) select among them.
  N > 1: run under `torch.distributed.run --nproc-per-node N` (the driver's form), or let bench.py
  start that launcher itself when WORLD_SIZE is unset (the parent never touches the GPU).
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REPO, "graph-transformer_amd"), REPO]

if int(os.environ.get("WORLD_SIZE", "1")) > 1 or "--force-dist" in sys.argv:
    # a process-group rank: 16 HIP hardware queues, so that RCCL's streams do not share the main / side streams'
    # queues (C4 at one rank, overlapped all-reduce: +2.2 % over no process group with 16, +2.6-3.4 % with 8;
    # profiles/r06/dp_overhead_ab.txt).  Before the HIP runtime starts.
    _q = os.environ.get("GPU_MAX_HW_QUEUES", "")
    if not _q.isdigit() or int(_q) < 16:
        os.environ["GPU_MAX_HW_QUEUES"] = "16"

import u2gnn_hip  # noqa: E402,F401  (before the HIP runtime starts: GPU_MAX_HW_QUEUES, see ensure_hw_queues)
import numpy as np  # noqa: E402
import torch  # noqa: E402

METRIC = "graphs/sec (fwd+bwd) U2GNN-Sup COLLAB k=16 T=4 at 1/2/4/8 MI355X"
PEAK = {"fp32": 157.3,     # TFLOP/s dense f32-input MFMA peak (MI355X_MICROARCH.md)
        "bf16x3": 2500.0 / 3,  # 2.5 PF dense bf16 MFMA / 3 MFMAs per fp32-accurate product
        "bf16": 2500.0,
        "bf16x6": 2500.0 / 6,   # 6 MFMAs per fp32-accurate product
        # policy-level rate of a whole fwd6 step: its forward products (1/3 of the step's FLOPs) at 6 MFMAs each, the
        # backward (2/3) at 3: 1 / (1/(3 * 2500/6) + 2/(3 * 2500/3))
        "fwd6": 1.0 / (1.0 / (3 * 2500.0 / 6) + 2.0 / (3 * 2500.0 / 3)),
        "f16x3": 2500.0 / 3,    # 3 fp16 MFMAs per product (the fp16 and bf16 dense peaks are equal)
        "fwdh": 2500.0 / 3}
DTYPE = {"fp32": "fp32", "bf16x3": "bf16x3", "bf16": "bf16",
         "mixed": "bf16x3 (dS/dQ/dK: bf16)", "fwd32": "fp32 forward, bf16x3 backward",
         "fwd6": "bf16x6 forward, bf16x3 backward", "fwdh": "f16x3 forward, bf16x3 backward"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--allreduce", default="overlap", choices=["overlap", "after", "none"],
                    help="gradient all-reduce per layer under the backward (overlap) or after it")
    ap.add_argument("--force-dist", action="store_true",
                    help="init the RCCL process group even at one rank (exercises the DP path on one GPU)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline value does not need: CPU baseline, other precision policies, "
                         "the on-the-fly pipeline, the other configs, the neighbour-attention line and the rooflines "
                         "(each has its own switch below); off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step left its caller -- loss, flat parameters "
                         "and flat gradients -- as DIR/<name>.npy (float32; a fixed seeded sample of each array "
                         "when they exceed 64 MB in all, as for --workload c5)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--num-neighbors", type=int, default=16)
    ap.add_argument("--num-timesteps", type=int, default=4)
    ap.add_argument("--ff-hidden-size", type=int, default=1024)
    ap.add_argument("--num-hidden-layers", type=int, default=1)
    ap.add_argument("--precision", default="fwdh", choices=["fp32", "bf16x3", "mixed", "bf16", "fwd32", "fwd6", "fwdh"],
                    help="fwdh (default, round 6) = forward products on the two-plane fp16 split f16x3 (22-bit "
                         "pre-scaled operands), backward bf16x3: the train-mode ReLU decisions carry fp32-class rounding "
                         "at +2 %% over bf16x3 (DESIGN.md section 7.1); fwd6 = forward products on the three-plane "
                         "bf16x6 split (fp32-accurate, +16 %%); "
                         "bf16x3 = every product split-bf16; mixed = bf16x3 with the attention-backward dS/dQ/dK "
                         "products on plain bf16 (experiment: +4 %% at C4, outside the 1e-3 bound on the MUTAG L2T2 golden)")
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--distinct-batches", type=int, default=8)
    ap.add_argument("--cpu-baseline", type=int, default=1, help="1 = time the CPU oracle on rank 0 at N=1")
    ap.add_argument("--cpu-steps", type=int, default=3, help="CPU baseline steps (median reported)")
    ap.add_argument("--pipeline-steps", type=int, default=20,
                    help="C4 at N=1: steps of the on-the-fly pipeline line (native assembly + copy-stream H2D + "
                         "GPU feature gather per step); 0 = skip")
    ap.add_argument("--fp32-steps", type=int, default=10,
                    help="C4 at N=1: timed steps of the same step in exact fp32 beside the headline (0 = skip)")
    ap.add_argument("--launch-check", action="store_true",
                    help="ranks report (rank, world) and exit before touching the GPU (tests the --gpus launcher)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--probe", default="ds", choices=["qk", "pv", "ds", "dv", "dq", "dk"],
                    help="attention product timed live (HIP events on its own stream) inside the timed "
                         "region for the roofline object; ds = the step's dominant kernel")
    ap.add_argument("--graph", type=int, default=-1,
                    help="1 = replay each training step as one captured HIP graph (u2gnn_hip.train.StepGraphs, "
                         "one graph per distinct batch, captured before the warmup); default: on for c5 "
                         "(host-bound), off for c4 (the host runs ahead of the GPU)")
    ap.add_argument("--gemm-family", action="store_true",
                    help="extra untimed pass: every GEMM of the same steps serialised with per-launch events "
                         "(per-template-instance table); off by default so that a rocprofv3 trace of the "
                         "default command holds only the timed region's launches")
    ap.add_argument("--attention", default="nodes", choices=["nodes", "neighbors"],
                    help="nodes = the fork's semantics (the headline metric); neighbors = paper semantics")
    ap.add_argument("--configs", type=int, default=1,
                    help="C4 at N=1: also run the other BASELINE configs (c5, c2, c3) in the same process and "
                         "report each as an object of the C4 line (0 = skip)")
    ap.add_argument("--config-steps", type=int, default=30, help="timed steps of each embedded config line")
    ap.add_argument("--neighbors-line", type=int, default=1,
                    help="C4 at N=1: also time the paper-semantics neighbour attention (--attention neighbors) in a "
                         "child process and report it as the 'neighbors' object (0 = skip)")
    ap.add_argument("--workload", default="c4", choices=["c4", "c5", "c2", "c3"],
                    help="c4 = U2GNN-Sup COLLAB (the headline metric); c5 = U2GNN-UnSup REDDIT-M5K (HBM-bound); "
                         "c2 = U2GNN-Sup IMDBBINARY, c3 = U2GNN-UnSup PTC (BASELINE configs[1], [2]: real data, "
                         "latency-bound steps, replayed as HIP graphs)")
    return ap.parse_args()


def pmc_traffic(symbol):
    """HBM bytes per launch of `symbol` from a committed PMC pass (profiles/<round>/pmc_traffic.json,
    written by tools/pmc_traffic.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs with
    the gfx950 FETCH_SIZE x2 correction) OF THIS BUILD: the table's build_id must equal the hash of
    the native sources (u2gnn_hip._lib.source_build_id).  Returns (bytes or None, source or note)."""
    import glob
    from u2gnn_hip._lib import source_build_id
    bid = source_build_id()
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "*", "*pmc_traffic.json")), reverse=True):
        try:
            table = json.load(open(path))
        except (OSError, ValueError):
            continue
        if table.get("build_id") == bid and symbol in table.get("kernels", {}):
            return table["kernels"][symbol]["hbm_bytes_per_launch"], os.path.relpath(path, REPO)
    return None, f"no PMC pass of build {bid} covers this kernel"


def rocprof_stats(symbol, largest_grid=False):
    """(average launch us, calls, source) of `symbol` from a committed rocprofv3 kernel-trace summary
    (profiles/<round>/*_kstats.json, written by tools/kstats.py) OF THIS BUILD, or (None, None, note).
    largest_grid: the kernel's launches at its largest grid size only."""
    import glob
    from u2gnn_hip._lib import source_build_id
    bid = source_build_id()
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "*", "*kstats.json")), reverse=True):
        try:
            table = json.load(open(path))
        except (OSError, ValueError):
            continue
        if table.get("build_id") != bid:
            continue
        if largest_grid:
            rows = [r for r in table.get("by_grid", []) if r["kernel"] == symbol]
            if rows:
                r = max(rows, key=lambda r: r["grid"])
                return r["avg_us"], r["calls"], os.path.relpath(path, REPO)
        elif symbol in table.get("kernels", {}):
            k = table["kernels"][symbol]
            return k["avg_us"], k["calls"], os.path.relpath(path, REPO)
    return None, None, f"no kernel-trace summary of build {bid} under profiles/"


def host_cpu():
    """(model name, logical CPUs) of the host, from /proc/cpuinfo (lscpu's source)."""
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return model, os.cpu_count()


def cgroup_cpus():
    """CPUs this process's cgroup may use (cpu.max quota / period, cgroup v2; v1 cfs files), or None."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, int(int(q) // int(per)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, q // per)
    except (OSError, ValueError):
        return None


def cpu_threads():
    """Host threads for the CPU baseline: every CPU of the process's affinity mask
    (os.sched_getaffinity, not os.cpu_count(), which counts the whole machine), capped by the cgroup's
    CPU quota when one is set (threads beyond it only time-slice).  Returns (threads, how)."""
    aff = len(os.sched_getaffinity(0))
    quota = cgroup_cpus()
    threads = min(aff, quota) if quota else aff
    how = f"{threads} threads = sched_getaffinity ({aff} CPUs)" + (f" capped by the cgroup CPU quota ({quota})"
                                                                       if quota and quota < aff else "")
    return max(1, threads), how


def launch_ranks(args) -> int:
    """--gpus N > 1 without a launcher: run `torch.distributed.run --nproc-per-node N bench.py ...` as a
    CHILD process (this process has not initialised the GPU and never does; no exec) and relay the
    ranks' JSON lines.  Returns the launcher's exit code.  --standalone: the launcher's own rendezvous on a port
    it binds itself (no probe-then-close port race; the CLIs' launcher, u2gnn_hip/cli.py, does the same)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr=127.0.0.1",
           f"--nproc-per-node={args.gpus}", os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        line = line.strip()
        if line.startswith("{"):
            try:
                json.loads(line)
            except ValueError:
                continue
            print(line, flush=True)
    return proc.wait()


def model_step_flops(N, d, ff, T, L):
    """Algorithmic FLOPs of one fwd+bwd step, slot 0 only."""
    return 3.0 * L * T * (8.0 * N * d * d + 4.0 * N * N * d + 4.0 * N * d * ff)


def gather_roofline(b, d, ff, K, dev, reps=20):
    """a2 (pytorch_U2GNN_Sup.py:32, F.embedding(input_x, X_concat)): the reference materialises all
    k+1 neighbour slots of every node; time u2gnn_gather_rows over the same [N, k+1] index of one
    C4 batch into the padded [R_pad, dp] token image the neighbour-attention path consumes.
    HBM-minimum bytes per launch = token image written + index read + the unique source rows
    (the N x d table, re-read k+1 times from L2/MALL)."""
    from u2gnn_hip.engine import Dims, rup
    W = b.input_x.shape[1]
    R = b.N * W
    Rp, dp = Dims(R, d, ff).Np, rup(d, 64)
    # the launches write to destinations rotating over > 512 MiB (twice the 256 MB MALL), so a timed launch's
    # writes cannot sit in the cache a previous launch warmed: each launch pays its write-back to HBM
    dst_bytes = Rp * dp * 4
    nbuf = max(2, -(-(512 << 20) // dst_bytes) + 1)
    pool = torch.empty(nbuf, Rp, dp, device=dev, dtype=torch.float32)
    for i in range(3):
        K.gather_rows(b.X_concat, b.input_x, 1, pool[i % nbuf], R, Rp, d, dp)
    reps = max(reps, nbuf)
    st = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for i in range(reps):
        K.gather_rows(b.X_concat, b.input_x, 1, pool[(i + 3) % nbuf], R, Rp, d, dp)
    e1.record(st)
    torch.cuda.synchronize()
    del pool
    us = e0.elapsed_time(e1) * 1e3 / reps
    # algorithmic bytes: the REAL gathered values written (R rows x d columns; the image's padding columns and rows
    # are layout, not work), the int64 index and the unique source rows
    nbytes = R * d * 4 + R * 8 + b.N * d * 4
    ach = nbytes / (us * 1e-6) / 1e9
    sym = "gather_rows_multi_kernel<1, true, true>"
    traffic, tsrc = pmc_traffic(sym + "@maxgrid")
    rp_us, rp_calls, rsrc = rocprof_stats(sym, largest_grid=True)
    out = {"bound": "hbm", "kernel": sym + " (a2, all k+1 slots)", "achieved": round(ach, 1),
           "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4), "avg_launch_us": round(us, 2),
           "algorithmic_bytes_per_launch": nbytes, "image_bytes_written": Rp * dp * 4, "rows": R, "rows_pad": Rp,
           "d": d, "d_pad": dp, "timing": "HIP events around the launches",
           "destinations": f"{reps} launches rotating over {nbuf} destination images ({nbuf * dst_bytes / 2**20:.0f} MiB)",
           "traffic": traffic, "traffic_source": tsrc,
           "traffic_note": "PMC (2 * FETCH_SIZE + WRITE_SIZE) of these launches (the kernel's largest grid); the "
                           "writes are 16-B stores (exact), the reads 4-B-per-lane loads (the x2 FETCH_SIZE "
                           "correction is calibrated for 16-B reads)",
           "rocprof_avg_launch_us": round(rp_us, 2) if rp_us else None, "rocprof_source": rsrc}
    if rp_us:
        out["rocprof_frac"] = round(nbytes / (rp_us * 1e-6) / 1e9 / 8000.0, 4)
    return out


PROBE_STEPS = 10
ROLES = {}


def probe_precision(precision, role):
    """The matrix-core precision the probed product runs at under a precision policy."""
    fwd = role in ("qk", "pv")
    if precision == "mixed":
        return "bf16" if role in ("ds", "dq", "dk") else "bf16x3"
    if precision == "fwd32":
        return "fp32" if fwd else "bf16x3"
    if precision == "fwd6":
        return "bf16x6" if fwd else "bf16x3"
    if precision == "fwdh":
        return "f16x3" if fwd else "bf16x3"
    return precision


def attn_kernel_roofline(args, role, ms, n, used, d, per_step, K, LIB):
    """The roofline entry of one probed attention product: algorithmic FLOPs (2 N^2 d per product, real dims; the
    grouped dQ + dK launch carries two products) over the summed live event time, against the dense MFMA peak of
    the precision the product runs at; the kernel's PMC bytes per launch when the committed table is of this
    build, and its rocprof average when a committed kernel-trace summary is."""
    from u2gnn_hip.engine import row_pad, rup
    Np0, dp = row_pad(used[0].N), rup(d, 64)
    pk = probe_precision(args.precision, role)
    fused = pk in ("bf16x3", "bf16", "f16x3") and dp <= 384 and Np0 >= 1024   # encoder_layer.cpp fused_attn (fwd6: three-pass)
    prods = 2.0 if role == "dq" else 1.0   # the grouped dQ + dK launch
    fl = float(sum(per_step * prods * 2.0 * b.N * b.N * d for b in used))
    if role == "ds":
        sym = K.gemm_symbol(pk, Np0, Np0, 1, 0, False, True, LIB.EPI_ATTN_DS_SIGNED)
    elif role == "dv":
        sym = K.gemm_symbol(pk, Np0, dp, 4, 256, True, False, LIB.EPI_STORE, clamp_a=True)
    elif role == "dq":
        sym = "gemm_bf16_group_kernel<256, 128, 4, 2, 32, true>" if pk == "bf16x3" else "grouped dQ + dK"
    elif role == "qk":
        sym = K.gemm_symbol(pk, Np0, Np0, 1, 256, False, True, LIB.EPI_STORE_ROWSTAT if fused else LIB.EPI_STORE)
    else:
        sym = f"attn_softmax_pv_kernel<{dp}, {dict(bf16x3=2, f16x3=4).get(pk, 1)}>" if fused else \
            K.gemm_symbol(pk, Np0, dp, 4, 256, False, False, LIB.EPI_STORE, clamp_a=True)
    ach = fl / (ms * 1e-3) / 1e12
    peak = PEAK[pk]
    traffic, traffic_src = pmc_traffic(sym)
    rp_us, rp_calls, rp_src = rocprof_stats(sym)
    e = {"bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
         "frac": round(ach / peak, 4), "traffic": traffic, "traffic_source": traffic_src,
         "kernel": sym, "kernel_precision": pk, "role": "dq+dk (one grouped launch)" if role == "dq" else role,
         "launches": n, "avg_launch_us": round(1e3 * ms / n, 1), "algorithmic_flop_per_launch": round(fl / n),
         "rocprof_avg_launch_us": round(rp_us, 1) if rp_us else None, "rocprof_source": rp_src}
    if rp_us:
        e["rocprof_frac"] = round(fl / n / (rp_us * 1e-6) / 1e12 / peak, 4)
    return e


def cpu_baseline(hb, sd, args, d, C):
    """The oracle restatement (reference semantics incl. all k+1 slots and p=0.5 dropout,
    i.e. the reference's cost) timed on the host cores: forward + loss + backward + clip + Adam;
    median of --cpu-steps (>= 3) steps on one batch."""
    from oracle import u2gnn_oracle as O
    threads, how = cpu_threads()
    torch.set_num_threads(threads)
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in sd.items()}
    plist = list(params.values())
    opt = torch.optim.Adam(plist, lr=args.lr)
    ix = torch.from_numpy(hb.input_x)
    X = torch.from_numpy(hb.X_concat)
    lab = torch.from_numpy(hb.labels)
    times = []
    for _ in range(args.cpu_steps):
        t0 = time.perf_counter()
        opt.zero_grad()
        scores = O.sup_forward(params, ix, hb.offsets, X, args.num_hidden_layers, args.num_timesteps,
                               train=True, dropout=0.5)
        loss = O.soft_cross_entropy(scores, O.label_smoothing(lab, C))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(plist, 0.5)
        opt.step()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    model, ncpu = host_cpu()
    return {"value": hb.labels.shape[0] / t, "unit": "graphs/s", "cores": threads, "kind": "port",
            "cpu_model": model, "host_cpus": ncpu, "threads": how, "step_s": [round(x, 2) for x in times],
            "sample": f"median of {args.cpu_steps} full training steps of one {hb.labels.shape[0]}-graph batch "
                      f"(N={hb.N} nodes, all {args.num_neighbors + 1} neighbour slots, dropout on) "
                      f"= {t:.1f} s/step, oracle/u2gnn_oracle.py on torch CPU, {threads} threads"}


def pipeline_rate(store, trainer, args, dev, resident_value):
    """The same C4 training step with each batch built on the fly (SURVEY §8(d)'s timed region
    with the H2D inside; train_pytorch_U2GNN_Sup.py:114,117,153): native assembly of the next
    batch from the reference numpy stream into page-locked buffers, its H2D on the copy stream and
    the feature gather on the GPU (DeviceBatch.from_store), then the step.  Reported beside the
    resident-batch value, never as it (PCIe-inclusive rate)."""
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.synthetic import as_graph_store
    gs = as_graph_store(store)
    X_dev = torch.from_numpy(gs.X).to(dev)
    np.random.seed(321)
    loader = BatchLoader(gs, args.batch_size, args.num_neighbors, gather_x=False)
    for _ in range(2):
        trainer.step(DeviceBatch.from_store(loader(), X_dev, device=dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.pipeline_steps):
        trainer.step(DeviceBatch.from_store(loader(), X_dev, device=dev))
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    v = args.pipeline_steps * args.batch_size / el
    return {"value": round(v, 2), "unit": "graphs/s", "ms_per_step": round(1e3 * el / args.pipeline_steps, 3),
            "steps": args.pipeline_steps, "ratio_to_resident": round(v / resident_value, 4),
            "what": "per step: native batch assembly (numpy MT19937 stream continued in C++) into page-locked "
                    "buffers, H2D on a copy stream, GPU feature gather, training step"}


WHAT_PREC = {"fp32": "the same training step with every matrix-core product in exact fp32 (v_mfma_f32_32x32x2_f32)",
             "fwd32": "the same training step with the forward products in exact fp32 and the backward in bf16x3: "
                      "the forward's ReLU decisions then carry fp32 rounding only (DESIGN.md section 7)",
             "bf16x3": "the same training step with every product on the two-plane split (bf16x3, ~2^-16 per product): "
                       "the round-5 headline policy; 6-18 ReLU decisions per C4 step differ from the fp32 oracle's "
                       "(DESIGN.md section 7)",
             "fwd6": "the same training step with the forward products on the three-plane bf16x6 split (fp32-accurate) "
                     "and the backward in bf16x3",
             "fwdh": "the same training step with the forward products on the two-plane fp16 split f16x3 (~2^-21 per "
                     "product at the bf16x3 rate, fused softmax.P.V) and the backward in bf16x3"}


def exact_line(args, batches, sd0, dev, d, C, precision="fp32"):
    """The same C4 training step in another precision policy -- "fp32" (every product exact fp32,
    v_mfma_f32_32x32x2_f32) or "fwd32" (exact fp32 forward, bf16x3 backward) -- on the same batches and initial
    weights, beside the bf16x3 headline (the price of each policy on record).
    args.fp32_steps timed steps after 2 warmup steps; not the headline value."""
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.train import SupTrainer
    m = TransformerU2GNN(feature_dim_size=d, ff_hidden_size=args.ff_hidden_size, num_classes=C,
                         num_self_att_layers=args.num_timesteps, dropout=0.5,
                         num_U2GNN_layers=args.num_hidden_layers, precision=precision)
    m.load_state_dict(sd0)
    m = m.to(dev).train()
    tr = SupTrainer(m, lr=args.lr, max_norm=0.5, seed=123)
    nb = len(batches)
    for i in range(2):
        tr.step(batches[i % nb])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.fp32_steps):
        tr.step(batches[(2 + i) % nb])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"precision": precision, "value": round(args.fp32_steps * args.batch_size / el, 2), "unit": "graphs/s",
           "ms_per_step": round(1e3 * el / args.fp32_steps, 3), "steps": args.fp32_steps,
           "final_loss": round(float(tr.loss.item()), 5), "what": WHAT_PREC[precision]}
    del tr, m
    torch.cuda.empty_cache()
    return out


METRIC_C5 = "graphs/sec (fwd+bwd) U2GNN-UnSup REDDIT-M5K k=16 T=4 S=512 MI355X"


def init_dist(args, dev):
    """RCCL process group when the job has more than one rank (or --force-dist)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        if "MASTER_ADDR" not in os.environ:   # --force-dist without a launcher: a 1-rank group
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29533"))
        dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
        return dist, world, rank
    return None, world, rank


def unsup_cpu_baseline(hbs, sids, sd, V, T, lr, steps):
    """C5 CPU baseline: the oracle's UnSup composite with the reference's cost (all k+1 slots,
    dropout on) on the same batches and sample ids: forward + summed loss + backward + clip + Adam
    over the encoders and the dense [V, D] table; median of `steps` steps."""
    from oracle import u2gnn_oracle as O
    threads, how = cpu_threads()
    torch.set_num_threads(threads)
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in sd.items()}
    plist = list(params.values())
    opt = torch.optim.Adam(plist, lr=lr)
    enc = {k: v for k, v in params.items() if k != "ss.weight"}
    times = []
    for r in range(steps):
        h, sid = hbs[r % len(hbs)], sids[r % len(sids)]
        t0 = time.perf_counter()
        opt.zero_grad()
        lo = O.unsup_forward(enc, params["ss.weight"], torch.from_numpy(h.input_x), torch.from_numpy(h.X_concat),
                             torch.from_numpy(h.input_y), torch.from_numpy(sid), 1, T, train=True).sum()
        lo.backward()
        torch.nn.utils.clip_grad_norm_(plist, 0.5)
        opt.step()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    model, ncpu = host_cpu()
    return {"value": hbs[0].labels.shape[0] / t, "unit": "graphs/s", "cores": threads, "kind": "port",
            "cpu_model": model, "host_cpus": ncpu, "threads": how, "step_s": [round(x, 2) for x in times],
            "sample": f"median of {steps} training steps on the first {min(steps, len(hbs))} bench batches "
                      f"(all {hbs[0].input_x.shape[1]} neighbour slots, dropout on, V = {V}), "
                      f"median {t:.2f} s/step, oracle/u2gnn_oracle.py on torch CPU, {threads} threads"}


def c5_attn_kernel(args, trainer, batches):
    """C5's attention backward: the small-width layer backward (u2gnn_layer_small_bwd, csrc/small_layer.hip: the
    tail backward fused with the dQ walk, which also writes the compact query records, then the dK/dV walk over
    them with the in-projection's dX; the probe's time includes the tail backward, the FLOPs credited do not) that replaced the padded matrix-core products at d = 4 (round 5).  Timed live
    by the executor's probe (HIP events around each layer's backward attention call on its stream) over
    args.steps EAGER steps after the timed graph-replay region.  Algorithmic FLOPs 8 N^2 d per launch (dO.V^T,
    dS K, dS^T Q, Pd^T dO; the recomputed Q K^T not credited) against the fp32 vector peak: the kernels run on
    the vector ALUs (exp2, the dropout hash and d-wide dot products per (query, key) pair)."""
    from u2gnn_hip import _lib as LIB
    from u2gnn_hip import native
    if not native.enabled():
        return None
    per_step = args.num_hidden_layers * args.num_timesteps
    nb = len(batches)
    steps = max(4, args.steps)
    torch.cuda.synchronize()
    native.probe_arm(LIB.ROLE_DS, steps * per_step)
    for i in range(steps):
        trainer.step(*batches[i % nb])
    torch.cuda.synchronize()
    ms, n = native.probe_collect()
    if n != steps * per_step or ms <= 0.0:
        return None
    d = 4   # REDDIT-M5K features (X = 0.01 * ones[n, 4])
    fl = float(sum(per_step * 8.0 * batches[i % nb][0].N ** 2 * d for i in range(steps)))
    ach = fl / (ms * 1e-3) / 1e12
    return {"bound": "valu", "achieved": round(ach, 3), "peak": PEAK["fp32"], "unit": "TFLOP/s",
            "frac": round(ach / PEAK["fp32"], 4),
            "kernel": "u2gnn_layer_small_bwd (sa_bwd_q_kernel<4, tail> + sa_bwd_kv_kernel<4>)",
            "launches": n, "avg_launch_us": round(1e3 * ms / n, 1), "algorithmic_flop_per_launch": round(fl / n),
            "timing": "live: HIP events around each layer's attention backward, eager steps after the timed region"}


def main_c5(args):
    out = run_c5(args)
    if out is not None:
        emit(out)


def run_c5(args):
    """synthetic REDDIT-MULTI-5K (4999 graphs, mean 508.5 nodes, V = sum of
    nodes ~2.54M), batch 4, k=16, T=4, ff=1024, 512 sampled classes, D = 4.  HBM-bound: the
    roofline kernel is the optimizer sweep (clip-norm + Adam over the dense embedding table,
    32 algorithmic bytes per parameter: sqnorm reads g; Adam reads p, g, m, v and writes p, m, v).
    Data-parallel (world > 1): rank r trains batch r of each group of `world` with the r-th sample
    draw of the group; encoder gradients all-reduced, ss.weight's touched rows all-gathered
    (dp.UnSupGradSync)."""
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    dist, world, rank = init_dist(args, dev)
    from pytorch_U2GNN_UnSup import TransformerU2GNN as UnSupModel
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.dp import UnSupGradSync, broadcast_params, max_batch_nodes, rank_batches
    from u2gnn_hip.synthetic import reddit5k_like
    from u2gnn_hip.unsup import UnSupTrainer
    bs = 4
    store = reddit5k_like(seed=0)
    V = int(store.node_start[-1])
    np.random.seed(123)
    loader = BatchLoader(store, bs, args.num_neighbors, with_input_y=True)
    host = rank_batches(loader, world, rank, args.distinct_batches)
    torch.manual_seed(123)
    model = UnSupModel(feature_dim_size=4, ff_hidden_size=args.ff_hidden_size, dropout=0.5,
                       num_self_att_layers=args.num_timesteps, vocab_size=V, sampled_num=512,
                       num_U2GNN_layers=args.num_hidden_layers, device=dev, precision=args.precision)
    sd0 = {k: v.clone() for k, v in model.state_dict().items() if k in set(model.trainable_names())}
    model = model.to(dev)
    trainer = UnSupTrainer(model, lr=args.lr, max_norm=0.5, seed=123 + rank)
    if dist is not None:
        broadcast_params(trainer.flat)
        sync = UnSupGradSync(trainer.flat, max_batch_nodes(store.node_start, bs))
        trainer.grad_sync = trainer.row_sync = sync
    dbs = [DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, None, device=dev, input_y=h.input_y)
           for h in host]
    nb = len(dbs)
    S = 512
    # sample ids: drawn on the host EVERY step, as the reference does (sampled_softmax.py:31-42: the C++
    # log-uniform sampler, then H2D) -- one draw per batch of the stream, rank r keeps draw r of each group;
    # the ids go through a ring of page-locked buffers into the step's device buffer (stream-ordered H2D, so
    # a captured graph reads the fresh ids at replay)
    # (round 6 A/B: issuing step j + 1's H2D on a copy stream right after step j's launch, the compute stream
    # waiting on its event, ran 0.540 / 0.545 ms against 0.514 for the stream-ordered copy below: not kept)
    sid_dev = [torch.zeros(S, dtype=torch.int64, device=dev) for _ in range(nb)]
    ring = [(torch.empty(S, dtype=torch.int64, pin_memory=True), [None]) for _ in range(8)]
    draws_log = []
    counter = [0]
    t_draw = [0.0]

    def draw_into(i):
        td = time.perf_counter()
        draws = [model.ss.draw_samples() for _ in range(world)]
        ids = np.asarray(draws[rank], dtype=np.int64)
        if len(draws_log) < nb:
            draws_log.append(ids)
        buf, ev = ring[counter[0] % len(ring)]
        counter[0] += 1
        if ev[0] is not None:
            ev[0].synchronize()   # the H2D of this pinned slot 8 draws ago is done
        buf.numpy()[:] = ids
        sid_dev[i].copy_(buf, non_blocking=True)
        ev[0] = torch.cuda.Event()
        ev[0].record()
        t_draw[0] += time.perf_counter() - td

    batches = [(dbs[i], sid_dev[i]) for i in range(nb)]
    for i in range(nb):   # first ids of every distinct batch (also what the captures run with)
        draw_into(i)
    torch.cuda.synchronize()
    # HIP-graph replay of the step, also data parallel (the encoder all-reduce and the ss.weight row
    # all-gather captured with it; RCCL communicators are set up by one eager step first)
    graph = args.graph != 0
    runner = None
    try:
        if graph:   # one captured HIP graph per distinct batch, captured (not run) before the warmup
            from u2gnn_hip.train import StepGraphs
            if dist is not None:
                trainer.step(*batches[0])
                torch.cuda.synchronize()
                dist.barrier()
            runner = StepGraphs(trainer)
            for bt in batches:
                runner.capture(*bt)
        step = runner.step if runner is not None else trainer.step

        def one(i):
            draw_into(i % nb)
            step(*batches[i % nb])
        for i in range(args.warmup):
            one(i)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t_draw[0] = 0.0
        t0 = time.perf_counter()
        for i in range(args.steps):
            one(args.warmup + i)
        t_issue = time.perf_counter() - t0          # host time to enqueue the K steps (sampler draws included)
        t_draw_steps = t_draw[0]
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        loss = float(trainer.loss.item())
        if args.dump_outputs and rank == 0:   # before the optimizer roofline steps the parameters again
            dump_outputs(args.dump_outputs, trainer_outputs(trainer))
    finally:
        if runner is not None:
            runner.close()
    sids_host = draws_log
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    opt_roof = attn = None
    if args.full and not args.no_roofline:
        n = trainer.flat.n
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            trainer.opt.step()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        byts = 32.0 * n
        ach = byts / (us * 1e-6) / 1e9
        opt_roof = {"bound": "hbm", "achieved": round(ach, 1), "peak": 8000.0, "unit": "GB/s",
                    "frac": round(ach / 8000.0, 4), "traffic": None,
                    "kernel": "sqnorm + adam_kernel (clip-norm + Adam over the flat parameters)",
                    "params": n, "algorithmic_bytes_per_step": byts, "optimizer_us": round(us, 1),
                    "optimizer_share_of_step": round(us * 1e-3 / (1e3 * elapsed / args.steps), 3)}
        if dist is None:
            attn = c5_attn_kernel(args, trainer, batches)
    mean_N = float(np.mean([b.N for b, _ in batches]))
    # step-level HBM roofline: algorithmic bytes of the whole step = the dense Adam sweep
    # over ss.weight (p, g, m, v read; p, m, v written), the row gathers / scatters of the sampled softmax
    # and the encoder's parameter sweep, over the measured step time
    n_enc = trainer.flat.n - V * 4
    step_bytes = 4.0 * 6 * V * 4 + 4.0 * 3 * (mean_N + S) * 4 + 4.0 * 3 * n_enc * 7 / 3
    step_ach = step_bytes / (elapsed / args.steps) / 1e9
    step_roof = {"bound": "hbm", "achieved": round(step_ach, 1), "peak": 8000.0, "unit": "GB/s", "traffic": None,
                 "frac": round(step_ach / 8000.0, 4), "algorithmic_bytes_per_step": round(step_bytes),
                 "what": "SURVEY.md §8(d) C5 bytes per step (4*6*V*D + 4*3*(N+S)*D + 4*3*P_enc*7/3) / ms_per_step"}
    out = {"metric": METRIC_C5, "value": round(args.steps * bs * world / elapsed, 2), "unit": "graphs/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": args.precision,
           "data": f"synthetic REDDIT-M5K-like graphs (4999 graphs, V={V} nodes, X = 0.01*ones[n,4]); "
                   "random-init weights",
           "config": {"workload": "U2GNN-UnSup REDDIT-M5K (C5): batch_size=4/GPU, num_neighbors=16, num_timesteps=4, "
                                  "ff_hidden_size=1024, sampled_num=512, D=4",
                      "global_batch": bs * world, "mean_nodes_per_batch": round(mean_N, 1),
                      "parallelism": f"dp{world}" + (" (encoder all-reduce + ss.weight row all-gather)" if world > 1
                                                     else ""),
                      "precision": args.precision, "hip_graph": graph},
           "final_loss": round(loss, 4), "host_issue_ms_per_step": round(1e3 * t_issue / args.steps, 3),
           "host_sampler_ms_per_step": round(1e3 * t_draw_steps / args.steps, 3),
           "roofline": step_roof, "optimizer": opt_roof, "step_hbm": step_roof, "attention_kernel": attn,
           "cpu_baseline": None,
           "samples": "512 log-uniform ids drawn on the host every step (C++ sampler) and copied to HBM"}
    if args.full and rank == 0 and world == 1 and args.cpu_baseline:
        out["cpu_baseline"] = unsup_cpu_baseline(host, sids_host, sd0, V, args.num_timesteps, args.lr,
                                                 max(3, args.cpu_steps))
    if dist is not None:
        dist.destroy_process_group()
    return out if rank == 0 else None


METRIC_SMALL = {"c2": "graphs/sec (fwd+bwd) U2GNN-Sup IMDBBINARY k=8 T=4 MI355X",
                "c3": "graphs/sec (fwd+bwd) U2GNN-UnSup PTC k=4 T=2 S=512 MI355X"}


def main_small(args):
    emit(run_small(args))


def run_small(args):
    """BASELINE.json configs[1] (IMDBBINARY supervised, bs 4, k 8, T 4, ff 1024) and configs[2] (PTC
    unsupervised + SampledSoftmax 512, bs 4, k 4, T 2, ff 1024) on the real datasets of the image:
    N ~ 80-100 nodes per batch, so a step is latency-bound; it is replayed as one HIP graph per
    distinct batch (the side stream is off for layers this small).  cpu_baseline: the oracle (all
    k+1 slots, dropout on) on the same batches, host cores."""
    import util
    from oracle import u2gnn_oracle as O
    from u2gnn_hip.batching import BatchLoader, GraphStore
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.train import StepGraphs, SupTrainer
    if int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload c2/c3 runs on one GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sup = args.workload == "c2"
    name, k, T = ("IMDBBINARY", 8, 4) if sup else ("PTC", 4, 2)
    graphs, C = util.load_data(name, sup)
    np.random.seed(123)
    torch.manual_seed(123)
    store = GraphStore(graphs)
    d = store.X.shape[1]
    loader = BatchLoader(store, 4, k, with_input_y=not sup)
    host = [loader() for _ in range(args.distinct_batches)]
    if sup:
        from pytorch_U2GNN_Sup import TransformerU2GNN
        model = TransformerU2GNN(d, args.ff_hidden_size, C, T, 0.5, 1, precision=args.precision)
        sd0 = {kk: v.clone() for kk, v in model.state_dict().items()}
        model = model.to(dev).train()
        trainer = SupTrainer(model, lr=args.lr, max_norm=0.5)
        batches = [(DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device=dev),) for h in host]
    else:
        from pytorch_U2GNN_UnSup import TransformerU2GNN
        from u2gnn_hip.unsup import UnSupTrainer
        V = int(store.node_start[-1])
        model = TransformerU2GNN(feature_dim_size=d, ff_hidden_size=args.ff_hidden_size, dropout=0.5,
                                 num_self_att_layers=T, vocab_size=V, sampled_num=512, num_U2GNN_layers=1,
                                 device=dev, precision=args.precision)
        sd0 = {kk: v.clone() for kk, v in model.state_dict().items()}
        model = model.to(dev)
        trainer = UnSupTrainer(model, lr=5e-3, max_norm=0.5)
        batches = [(DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, None, device=dev, input_y=h.input_y),
                    torch.from_numpy(model.ss.draw_samples()).to(dev)) for h in host]
    graph = args.graph != 0
    runner = None
    if graph:
        runner = StepGraphs(trainer)
        for bt in batches:
            runner.capture(*bt)
    step = runner.step if runner is not None else trainer.step
    nb = len(batches)
    for i in range(args.warmup):
        step(*batches[i % nb])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(*batches[(args.warmup + i) % nb])
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    loss = float(trainer.loss.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, trainer_outputs(trainer))
    if runner is not None:
        runner.close()
    cpu = None
    if args.full and args.cpu_baseline:
        threads, how = cpu_threads()
        torch.set_num_threads(threads)
        params = {kk: v.detach().cpu().clone().requires_grad_(True) for kk, v in sd0.items()}
        plist = list(params.values())
        opt = torch.optim.Adam(plist, lr=args.lr if sup else 5e-3)
        sids = [model.ss.draw_samples() for _ in host] if not sup else None
        times = []
        reps = 40
        for r in range(reps):
            h = host[r % nb]
            t1 = time.perf_counter()
            opt.zero_grad()
            ix, X = torch.from_numpy(h.input_x), torch.from_numpy(h.X_concat)
            if sup:
                s = O.sup_forward(params, ix, h.offsets, X, 1, T, train=True, dropout=0.5)
                lo = O.soft_cross_entropy(s, O.label_smoothing(torch.from_numpy(h.labels), C))
            else:
                enc = {kk: v for kk, v in params.items() if kk != "ss.weight"}
                lo = O.unsup_forward(enc, params["ss.weight"], ix, X, torch.from_numpy(h.input_y),
                                     torch.from_numpy(sids[r % nb]), 1, T, train=True).sum()
            lo.backward()
            torch.nn.utils.clip_grad_norm_(plist, 0.5)
            opt.step()
            times.append(time.perf_counter() - t1)
        t = float(np.median(times[5:]))
        cpu = {"value": 4 / t, "unit": "graphs/s", "cores": threads, "kind": "port", "threads": how,
               "sample": f"{reps - 5} timed training steps of 4-graph {name} batches (all {k + 1} neighbour slots, "
                         f"dropout on), median {1e3 * t:.1f} ms/step, oracle/u2gnn_oracle.py on torch CPU"}
    mean_N = float(np.mean([bt[0].N for bt in batches]))
    ms_step = elapsed / args.steps
    largest = largest_kernel(args.workload)
    if sup:
        # C2 is MFMA-bound by its algorithmic FLOPs (slot 0 only), against the policy's dense rate
        fl = float(np.mean([model_step_flops(bt[0].N, d, args.ff_hidden_size, T, 1) for bt in batches]))
        ach = fl / ms_step / 1e12
        peak = PEAK[args.precision]
        roof = {"bound": "mfma", "achieved": round(ach, 3), "peak": round(peak, 1), "unit": "TFLOP/s",
                "frac": round(ach / peak, 5), "traffic": None, "algorithmic_flop_per_step": round(fl),
                "what": "SURVEY.md §8(d) step FLOPs 3*L*T*(8*N*d^2 + 4*N^2*d + 4*N*d*ff) / ms_per_step",
                "largest_kernel": largest}
    else:
        # C3 is HBM-bound by the bytes of its step: the dense Adam sweep over ss.weight [V, D]
        # (p, g, m, v read; p, m, v written), the sampled softmax's row gathers / scatters, the encoder's sweep
        D = d   # num_U2GNN_layers = 1
        n_enc = sum(v.numel() for kk, v in sd0.items() if kk != "ss.weight")
        byts = 4.0 * 6 * V * D + 4.0 * 3 * (mean_N + 512) * D + 4.0 * 3 * n_enc * 7 / 3
        ach = byts / ms_step / 1e9
        roof = {"bound": "hbm", "achieved": round(ach, 2), "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 5),
                "traffic": None, "algorithmic_bytes_per_step": round(byts),
                "what": "SURVEY.md §8(d) bytes per step (4*6*V*D + 4*3*(N+S)*D + 4*3*P_enc*7/3) / ms_per_step",
                "largest_kernel": largest}
    out = {"metric": METRIC_SMALL[args.workload], "value": round(args.steps * 4 / elapsed, 2), "unit": "graphs/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": DTYPE[args.precision],
           "data": f"{name} (the reference's dataset file), seed-123 batches; random-init weights",
           "config": {"workload": f"U2GNN-{'Sup' if sup else 'UnSup'} {name}: batch_size=4, num_neighbors={k}, "
                                  f"num_timesteps={T}, ff_hidden_size={args.ff_hidden_size}"
                                  + ("" if sup else ", sampled_num=512"),
                      "global_batch": 4, "mean_nodes_per_batch": round(mean_N, 1), "parallelism": "dp1",
                      "precision": args.precision, "hip_graph": graph},
           "final_loss": round(loss, 5), "host_issue_ms_per_step": round(1e3 * t_issue / args.steps, 3),
           "roofline": roof, "cpu_baseline": cpu}
    return out


def neighbors_line(args):
    """The paper-semantics neighbour attention (--attention neighbors: every node attends
    over its own k+1 sampled neighbours, csrc/window_attn.hip) on the same C4 batches, timed by this script in a
    child process (its own HIP context; this process has released its cached memory) -- the line that process
    prints, reduced to its timing fields."""
    import subprocess
    torch.cuda.empty_cache()
    cmd = [sys.executable, os.path.abspath(__file__), "--attention", "neighbors", "--steps", "10", "--warmup", "3",
           "--configs", "0", "--neighbors-line", "0", "--cpu-baseline", "0", "--fp32-steps", "0", "--pipeline-steps",
           "0", "--no-roofline", "--precision", args.precision]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = json.loads(r.stdout.strip().splitlines()[-1])
    except (subprocess.TimeoutExpired, ValueError, IndexError) as e:
        return {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    keep = ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "config", "host_issue_ms_per_step")
    out = {k: line[k] for k in keep if k in line}
    out["run_s"] = round(time.perf_counter() - t0, 1)
    out["command"] = " ".join(["python", "bench.py"] + cmd[2:])
    return out


def largest_kernel(workload):
    """The largest kernel (device time) of a workload's step from the committed kernel-trace summary of THIS build
    (profiles/<round>/*_<workload>_kstats.json, tools/wl_trace.sh), or a note."""
    import glob
    from u2gnn_hip._lib import source_build_id
    bid = source_build_id()
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "*", f"*{workload}_kstats.json")), reverse=True):
        try:
            t = json.load(open(path))
        except (OSError, ValueError):
            continue
        if t.get("build_id") != bid or not t.get("kernels"):
            continue
        name, k = max(t["kernels"].items(), key=lambda kv: kv[1]["total_ms"])
        return {"kernel": name, "avg_launch_us": round(k["avg_us"], 2), "calls": k["calls"],
                "share_of_kernel_time": round(k["total_ms"] / t["total_kernel_ms"], 3),
                "source": os.path.relpath(path, REPO)}
    return {"note": f"no kernel-trace summary of build {bid} for {workload} under profiles/"}


DUMP_BUDGET = 64 * 10 ** 6   # bytes of --dump-outputs, all arrays together


def dump_outputs(path, arrays):
    """--dump-outputs: `arrays` (name -> device tensor) as path/<name>.npy in float32.  At most DUMP_BUDGET bytes of
    array data in all: when the arrays exceed it, each is cut to the same fraction of its elements (rounded down, at
    least one; the budget keeps one element per array aside for that), at sorted positions drawn by a generator
    seeded with a constant, so two runs with the same arguments keep the same positions."""
    os.makedirs(path, exist_ok=True)
    total = sum(4 * t.numel() for t in arrays.values())
    frac = 1.0 if total <= DUMP_BUDGET else (DUMP_BUDGET - 4 * len(arrays)) / total
    for i, (name, t) in enumerate(arrays.items()):
        a = t.detach().reshape(-1).to(torch.float32).cpu().numpy()
        if frac < 1.0:
            rng = np.random.default_rng(20240 + i)
            keep = np.sort(rng.choice(a.size, size=max(1, int(a.size * frac)), replace=False))
            a = a[keep]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def trainer_outputs(trainer):
    """What a caller of trainer.step() holds after it: the returned loss and the state the step wrote (the flat
    parameter buffer after clip + Adam, the flat gradient buffer of that step)."""
    return {"loss": trainer.loss, "params": trainer.flat.flat, "grads": trainer.flat.gflat}


_JSON_OUT = None


def emit(out: dict) -> None:
    """The ONE result line, on the original stdout (libraries' stdout chatter -- e.g. RCCL's
    version banner at communicator init -- is redirected to stderr in main())."""
    f = _JSON_OUT if _JSON_OUT is not None else sys.stdout
    f.write(json.dumps(out) + "\n")
    f.flush()


def main():
    global _JSON_OUT
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher around us: start one as a child; nothing here has touched the GPU
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}: one rank per GPU")
    if args.launch_check:   # test hook: the launcher reached every rank (no GPU work)
        print(json.dumps({"launch_check": True, "rank": int(os.environ.get("RANK", "0")), "world": world}),
              flush=True)
        return
    sys.stdout.flush()
    _JSON_OUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)   # fd 1 -> stderr for everything else (native libraries write to fd 1 directly)
    if args.workload == "c5":
        return main_c5(args)
    if args.workload in ("c2", "c3"):
        if world != 1:
            raise SystemExit("--workload c2/c3 runs on one GPU")
        return main_small(args)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    from u2gnn_hip.engine import side_stream
    side_stream(dev)   # before RCCL creates its streams (own hardware queue, see side_stream)
    dist, world, rank = init_dist(args, dev)

    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.dp import GradAllReduce, OverlappedGradAllReduce, broadcast_params, rank_batches
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip import kernels as K
    from u2gnn_hip.synthetic import collab_like
    from u2gnn_hip.train import SupTrainer

    d, C = 367, 3
    store = collab_like(seed=0)
    np.random.seed(123)
    loader = BatchLoader(store, args.batch_size, args.num_neighbors)
    # rank r keeps batch r of every group of `world` consecutive batches of the single
    # reference numpy stream (the others are replayed to keep the stream aligned)
    host = rank_batches(loader, world, rank, args.distinct_batches)
    batches = [DeviceBatch.from_offsets(h.input_x, h.offsets, h.X_concat, h.labels, device=dev) for h in host]
    torch.manual_seed(123)
    model = TransformerU2GNN(feature_dim_size=d, ff_hidden_size=args.ff_hidden_size, num_classes=C,
                             num_self_att_layers=args.num_timesteps, dropout=0.5,
                             num_U2GNN_layers=args.num_hidden_layers, precision=args.precision,
                             attention=args.attention)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev).train()
    trainer = SupTrainer(model, lr=args.lr, max_norm=0.5, seed=123 + rank)
    if dist is not None:
        broadcast_params(trainer.flat)
        if args.allreduce == "none":   # diagnostics only: no gradient exchange
            pass
        elif args.allreduce == "overlap":   # per-layer buckets under the backward
            ar = OverlappedGradAllReduce(trainer.flat)
            model.core.stack.grad_ready = ar.layer_done
            trainer.grad_sync = ar
        else:
            trainer.grad_sync = GradAllReduce(bucket_mb=8.0)

    nb = len(batches)
    # HIP-graph replay, also data parallel: the gradient all-reduce (per-layer buckets issued from the
    # parameter-gradient side stream, or the buckets after the backward) is captured with the step, as in
    # run_unsup; RCCL's communicator is set up by one eager step first
    graph = args.graph == 1
    runner = None
    from u2gnn_hip import native
    from u2gnn_hip import _lib as LIB
    global ROLES
    ROLES = {"qk": LIB.ROLE_QK, "pv": LIB.ROLE_PV, "ds": LIB.ROLE_DS, "dv": LIB.ROLE_DV, "dq": LIB.ROLE_DQ,
             "dk": LIB.ROLE_DK}
    role = ROLES[args.probe]
    # (graph replay: the probe's events would belong to the capture, so no live probe)
    probing = args.full and not args.no_roofline and args.attention == "nodes" and native.enabled() and not graph
    per_step = args.num_hidden_layers * args.num_timesteps
    try:
        if graph:   # one captured HIP graph per distinct batch, captured (not run) before the warmup
            from u2gnn_hip.train import StepGraphs
            if dist is not None:
                trainer.step(batches[0])
                torch.cuda.synchronize()
                dist.barrier()
            runner = StepGraphs(trainer)
            for bt in batches:
                runner.capture(bt)
        step = runner.step if runner is not None else trainer.step
        for i in range(args.warmup):
            step(batches[i % nb])
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        if probing:   # live: HIP events around every launch of that product, on its stream
            native.probe_arm(role, args.steps * per_step)
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(batches[(args.warmup + i) % nb])
        t_issue = time.perf_counter() - t0          # host time to enqueue the K steps
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        probe_ms, probe_n = native.probe_collect() if probing else (0.0, 0)
    finally:
        if runner is not None:
            runner.close()
    loss = float(trainer.loss.item())
    if args.dump_outputs and rank == 0:   # before any further pass steps the trainer again
        dump_outputs(args.dump_outputs, trainer_outputs(trainer))
    # optional per-GEMM family pass: the same K steps again, serialised, with per-GEMM HIP events
    K.REC.records.clear()
    rec_elapsed = None
    if args.gemm_family and args.attention == "nodes":   # per-GEMM events: Python orchestration
        from u2gnn_hip.engine import set_overlap
        from u2gnn_hip import native
        set_overlap(False)   # serial: each GEMM's events time that kernel alone
        native.set_enabled(False)   # the same kernel sequence, launched from the evented wrappers
        K.REC.enabled = True
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.steps):
            trainer.step(batches[(args.warmup + i) % nb])
        torch.cuda.synchronize()
        rec_elapsed = time.perf_counter() - t1
        K.REC.enabled = False
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    graphs = args.steps * args.batch_size * world
    value = graphs / elapsed
    used = [batches[(args.warmup + i) % nb] for i in range(args.steps)]
    mean_N = float(np.mean([b.N for b in used]))
    step_flops = float(np.mean([model_step_flops(b.N, d, args.ff_hidden_size, args.num_timesteps,
                                                 args.num_hidden_layers) for b in used]))

    roof = None
    if probe_n:
        # the dominant kernel (the attention dS GEMM by default: the largest device time of a C4
        # step's critical path, rocprof profiles/) timed live in the timed region: achieved = its launches'
        # algorithmic FLOPs (2 N^2 d per product, real unpadded dims) / their summed event time
        if probe_n != args.steps * per_step:
            raise SystemExit(f"probe recorded {probe_n} launches, expected {args.steps * per_step}")
        roof = attn_kernel_roofline(args, args.probe, probe_ms, probe_n, used, d, per_step, K, LIB)
        roof.update({"timing": "live: HIP events around each launch on its own stream inside the timed region",
                     "dominance": "largest per-product device time on the critical path (DESIGN.md section 8)",
                     "step_tflops_per_gpu": round(step_flops / (elapsed / args.steps) / 1e12, 2),
                     "step_frac": round(step_flops / (elapsed / args.steps) / 1e12 / PEAK[args.precision], 4)})
        # the step's other large attention products, each timed live the same way in an untimed pass of
        # PROBE_STEPS steps of the same schedule after the timed region (one role armed per pass)
        others = {}
        for r in [x for x in ("dv", "dq", "qk", "pv") if x != args.probe]:
            native.probe_arm(ROLES[r], PROBE_STEPS * per_step)
            for i in range(PROBE_STEPS):
                step(batches[(args.warmup + i) % nb])
            torch.cuda.synchronize()
            ms, n = native.probe_collect()
            if n == PROBE_STEPS * per_step and ms > 0:
                others[r] = attn_kernel_roofline(args, r, ms, n, used[:PROBE_STEPS], d, per_step, K, LIB)
                others[r]["timing"] = f"live HIP events, untimed pass of {PROBE_STEPS} steps after the timed region"
        roof["other_kernels"] = others
    summ = K.REC.summary()
    if summ:
        fam = sorted(summ.items(), key=lambda kv: -kv[1][2])
        roof = roof or {}
        roof["gemm_share_of_serialised_step"] = round(sum(v[2] for v in summ.values()) / (1e3 * rec_elapsed), 3)
        roof["gemm_family_serialised"] = {k: {"launches": v[0], "ms": round(v[2], 2),
                                             "tflops": round(v[1] / (v[2] * 1e-3) / 1e12, 1)} for k, v in fam[:8]}
    out = {"metric": METRIC, "value": round(value, 2), "unit": "graphs/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": DTYPE[args.precision],
           "data": "synthetic COLLAB-like graphs (5000 graphs, mean 74.49 nodes, degree-tag one-hot d=367, "
                   "3 classes); random-init weights",
           "config": {"workload": "U2GNN-Sup COLLAB (C4): batch_size=64/GPU, num_neighbors=16, num_timesteps=4, "
                                  "ff_hidden_size=1024, num_hidden_layers=1, d=367",
                      "global_batch": args.batch_size * world, "mean_nodes_per_batch": round(mean_N, 1),
                      "parallelism": f"dp{world}", "precision": args.precision, "attention": args.attention,
                      "hip_graph": graph},
           "final_loss": round(loss, 5), "host_issue_ms_per_step": round(1e3 * t_issue / args.steps, 3),
           "roofline": roof, "gather": None, "cpu_baseline": None,
           "parity": {"tolerance": "max|ours - reference| / max(1, max|reference|) <= 1e-3 (north_star)",
                      "fwdh_train_c4": "the headline policy (round 6, late): forward products on the two-plane fp16 split "
                                       "f16x3 (22-bit operands, pre-scaled out of fp16's subnormals) with the fused "
                                       "softmax.P.V, backward bf16x3.  Train mode at the test seed "
                                       "(tests/test_train_parity_gpu.py): every output, gradient and post-Adam parameter "
                                       "within 1e-3 of the PLAIN oracle (4.1e-5, no flips).  Over 8 dropout seeds "
                                       "(profiles/r06/h3g_prec_fused.jsonl): 0-2 ReLU decisions per step differ from the "
                                       "fp32 oracle's (total 5; fwd32 6, fwd6 9, bf16x3 100); 5 of 8 seeds hold every "
                                       "gradient within 1e-3 (fwd32 4, fwd6 2); over 16 seeds "
                                       "(profiles/r06/prec_train_16seeds.jsonl) fwdh 7, fwd32 6, fwd6 4, the oracle's "
                                       "own fp32 vs float64 9",
                      "fwd6_train_c4": "(the 'fwd6' object) forward products on the three-plane bf16x6 split "
                                       "(fp32-accurate), backward bf16x3.  Train mode at the test seed "
                                       "(tests/test_train_parity_gpu.py): every output, gradient and post-Adam parameter "
                                       "within 1e-3 of the PLAIN oracle (no injected decisions, no flips).  Over 8 "
                                       "dropout seeds (profiles/r06/prec_train_8seeds.jsonl): 0-3 ReLU decisions per "
                                       "step differ from the fp32 oracle's (bf16x3: 6-18; the fp32 path 0-2); 2 of 8 "
                                       "seeds hold every gradient within 1e-3 (fp32 path 4, the reference's own fp32 vs "
                                       "float64 6): a single switched boundary unit moves its dW1 row by ~1e-2 for ANY "
                                       "implementation not bit-identical to torch-CPU's summation order",
                      "bf16x3_eval": "every output, loss, gradient and post-Adam parameter within 1e-3 of the "
                                     "reference goldens (MUTAG, MUTAG L2T2, IMDBBINARY) and of the oracle on a full "
                                     "C4 batch (tests/test_sup_parity_gpu.py)",
                      "bf16x3_train_c4": "(the round-5 headline policy, the 'bf16x3' object) train mode, the kernels' dropout masks in the oracle, no per-quantity "
                                         "exception (tests/test_train_parity_gpu.py, DESIGN section 7): with the GPU's "
                                         "own ReLU decisions every output, gradient and post-Adam parameter within "
                                         "1.03e-5 / 2.1e-5; the 11 decisions that differ from the plain oracle's are "
                                         "units with |z| <= 6.2e-6 (forward disagreement 2.2e-5); against the plain "
                                         "oracle the linear1 gradients are NOT held to 1e-3 (up to 1.7e-2: a switched "
                                         "boundary unit moves its dW1 row; the reference's own fp32 misses its fp64 "
                                         "run by up to 2e-2); outputs and loss within 1e-3 of it",
                      "fp32": "within 4.1e-6 in every case and mode; its C4 rate is the 'fp32' object"}}
    if rank == 0 and args.full:   # (--no-roofline is the live probes' switch, not the gather's)
        out["gather"] = gather_roofline(used[0], d, args.ff_hidden_size, K, dev)
    extras = args.full and rank == 0 and world == 1   # what only --full measures (see parse())
    if extras and args.fp32_steps > 0 and args.precision != "fp32" and args.attention == "nodes":
        # the other precision policies' price on the same batches: every product exact fp32,
        # the exact-fp32 forward, and the policies of bf16x3 / fwd6 / fwdh that are not the headline
        out["fp32"] = exact_line(args, batches, sd0, dev, d, C, "fp32")
        if args.precision in ("bf16x3", "fwd6", "fwdh"):
            out["fwd32"] = exact_line(args, batches, sd0, dev, d, C, "fwd32")
            for other in ("bf16x3", "fwd6", "fwdh"):
                if other != args.precision:
                    out[other] = exact_line(args, batches, sd0, dev, d, C, other)
    if extras and args.pipeline_steps > 0 and args.attention == "nodes":
        out["pipeline"] = pipeline_rate(store, trainer, args, dev, value)
    if extras and args.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(host[args.warmup % nb], sd0, args, d, C)
    if extras and args.configs and args.attention == "nodes" and not args.force_dist:
        # BASELINE configs[4], [1], [2] timed in this run too (driver-timed C5 / C2 / C3): each
        # object is the line its own --workload run prints
        import copy
        del trainer, model, batches
        torch.cuda.empty_cache()
        for wl in ("c5", "c2", "c3"):
            a = copy.copy(args)
            a.workload, a.steps, a.warmup, a.graph, a.dump_outputs = wl, args.config_steps, 5, -1, None
            t0 = time.perf_counter()
            sub = run_c5(a) if wl == "c5" else run_small(a)
            sub["run_s"] = round(time.perf_counter() - t0, 1)
            out[wl] = sub
            torch.cuda.empty_cache()
    if extras and args.neighbors_line and args.attention == "nodes" and not args.force_dist:
        out["neighbors"] = neighbors_line(args)
    if rank == 0:
        emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
