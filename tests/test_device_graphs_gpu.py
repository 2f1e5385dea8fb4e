"""pattern.DeviceGraphs on the GPU: a batch's adjacency assembled by u2gnn_adjacency_assemble from the device-resident
structure equals the host path (Adjacency.from_csr of the store's CSR) integer for integer -- the kernel alone, its
exact extent, a bad slot (the memory-safety contract), the DeviceBatch.from_store pipeline, a model step and both
CLIs.  Nothing here has a tolerance."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from device_graphs_ref import (HOPS_GPU, assert_adjacency_equal, batches_of, host_adjacency, odd_batches,  # noqa: E402
                               store_named, structure_of)

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
SENTINEL = -7777


@pytest.mark.parametrize("H", HOPS_GPU)
@pytest.mark.parametrize("name", ["MUTAG", "PTC", "synthetic", "odd"])
def test_kernel_equals_the_host_path(name, H):
    store = store_named(name)
    dg = structure_of(name, H, DEV)
    batches = odd_batches() if name == "odd" else batches_of(len(store.n_nodes))
    for ids in batches:
        assert_adjacency_equal(dg.adjacency(ids), host_adjacency(store, ids, H, DEV), (name, H, list(ids)[:8]))
    dg.check_indices()


def test_many_blocks_ptc_bs128_three_hops():
    """About 35 K entries: tens of 1024-entry blocks, chunk boundaries inside graphs and, somewhere among the 40
    seeded batches' 5 K graph boundaries, also at or next to one."""
    store = store_named("PTC")
    dg = structure_of("PTC", 3, DEV)
    rs = np.random.RandomState(5)
    nnzs = []
    for _ in range(3):
        ids = rs.permutation(len(store.n_nodes))[:128]
        got = dg.adjacency(ids)
        assert_adjacency_equal(got, host_adjacency(store, ids, 3, DEV), "PTC bs 128")
        nnzs.append(got.nnz)
    assert min(nnzs) > 8 * 1024, nnzs
    # a chunk that starts exactly at a graph's first entry: graphs (repeats allowed) whose entry counts add up to the
    # 1024 entries of a block, then two more graphs
    per = dg.n_entries
    last = {0: None}                                         # entry total -> the graph that completed it
    for t in range(1, 1025):
        for g in np.unique(per, return_index=True)[1]:
            if t - per[g] in last:
                last[t] = int(g)
                break
    assert 1024 in last
    ids, t = [], 1024
    while t:
        ids.append(last[t])
        t -= int(per[last[t]])
    assert int(per[ids].sum()) == 1024
    ids += [int(np.argmax(per)), int(np.argmin(per))]
    assert_adjacency_equal(dg.adjacency(ids), host_adjacency(store, ids, 3, DEV), "boundary")
    dg.check_indices()


def _raw_call(dg, ids, pad=37, gid_override=None):
    """The kernel wrapper on outputs carved from larger sentinel-filled buffers: (views, whole buffers, err, plan)."""
    from u2gnn_hip import kernels as K
    ids, row_off, ent_off, N, nnz, n_types = dg.plan(ids)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    gid = to(ids if gid_override is None else gid_override)
    sizes = {"rowptr": N + 1, "colidx": nnz, "t_rowptr": N + 1, "t_src": nnz, "t_eid": nnz}
    whole = {k: torch.full((n + 2 * pad + 1,), SENTINEL, device=DEV, dtype=torch.int64) for k, n in sizes.items()}
    view = {k: whole[k][pad + 1:pad + 1 + sizes[k]] for k in sizes}           # an odd element offset: 8-byte aligned only
    whole["etype"] = torch.full((nnz + 2 * pad,), SENTINEL, device=DEV, dtype=torch.int32) if dg.hops else None
    view["etype"] = whole["etype"][pad:pad + nnz] if dg.hops else None
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    K.adjacency_assemble(dg.c_struct(), gid, to(row_off), to(ent_off), N, nnz, view["rowptr"], view["colidx"],
                         view["t_rowptr"], view["t_src"], view["t_eid"], view["etype"], err)
    torch.cuda.synchronize()
    return view, whole, err, (ids, row_off, ent_off, N, nnz, n_types)


@pytest.mark.parametrize("H", [None, 3])
def test_nothing_is_written_outside_the_outputs(H):
    from u2gnn_hip.pattern import Adjacency
    store = store_named("PTC")
    dg = structure_of("PTC", H, DEV)
    ids = np.random.RandomState(3).permutation(len(store.n_nodes))[:40]
    view, whole, err, (_, _, _, N, nnz, n_types) = _raw_call(dg, ids)
    assert int(err.item()) == 0
    got = Adjacency(N, view["rowptr"], view["colidx"], view["t_rowptr"], view["t_src"], view["t_eid"], view["etype"],
                    n_types)
    assert_adjacency_equal(got, host_adjacency(store, ids, H, DEV), "carved")
    for k, w in whole.items():
        if w is None:
            continue
        n = view[k].numel()
        lo = 38 if w.dtype == torch.int64 else 37
        assert (w[:lo] == SENTINEL).all() and (w[lo + n:] == SENTINEL).all(), k
        assert w[lo:lo + n].data_ptr() == view[k].data_ptr()


@pytest.mark.parametrize("H", [None, 2])
def test_a_bad_slot_is_flagged_and_written_as_skipped_entries(H):
    """The memory-safety contract: a graph id outside [0, G) that reaches the kernel (the host check bypassed) sets the
    err flag, its slot's entries become -1, every other slot equals the host path, the row pointers stay inside
    [0, nnz], and the attention forward over the result runs and leaves finite output."""
    import math
    from u2gnn_hip import kernels as K
    from u2gnn_hip.engine import row_pad
    from u2gnn_hip.pattern import Adjacency
    store = store_named("MUTAG")
    dg = structure_of("MUTAG", H, DEV)
    ids = np.array([4, 60, 17, 99, 120, 33])
    bad = 3
    gid = ids.copy()
    gid[bad] = dg.G
    view, _, err, (_, row_off, ent_off, N, nnz, n_types) = _raw_call(dg, ids, gid_override=gid)
    assert int(err.item()) == 1
    ref = host_adjacency(store, ids, H, DEV)
    e0, e1, r0, r1 = int(ent_off[bad]), int(ent_off[bad + 1]), int(row_off[bad]), int(row_off[bad + 1])
    keep = torch.ones(nnz, dtype=torch.bool, device=DEV)
    keep[e0:e1] = False
    for k in ("colidx", "t_src", "t_eid"):
        assert (view[k][e0:e1] == -1).all(), k
        assert torch.equal(view[k][keep], getattr(ref, k)[keep]), k
    rows = torch.ones(N + 1, dtype=torch.bool, device=DEV)
    rows[r0:r1] = False
    for k in ("rowptr", "t_rowptr"):
        assert torch.equal(view[k][rows], getattr(ref, k)[rows]), k
        assert int(view[k].min()) >= 0 and int(view[k].max()) <= nnz, k
    if H:
        assert torch.equal(view["etype"][keep], ref.etype[keep]) and (view["etype"][e0:e1] == 0).all()
    A = Adjacency(N, view["rowptr"], view["colidx"], view["t_rowptr"], view["t_src"], view["t_eid"], view["etype"],
                  n_types)
    dp, Np = 64, row_pad(N)
    QKV = torch.randn(Np, 3 * dp, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    QKV[:, :dp] *= 1 / math.sqrt(dp)
    O = torch.full((Np, dp), float("nan"), device=DEV)
    stats = torch.full((Np, 2), float("nan"), device=DEV)
    K.csr_attn_fwd(QKV, dp, A, O, stats, 0.0, 11, N, Np)
    torch.cuda.synchronize()
    assert torch.isfinite(O).all()
    Oref = torch.empty_like(O)
    K.csr_attn_fwd(QKV, dp, ref, Oref, torch.empty_like(stats), 0.0, 11, N, Np)
    good = torch.ones(Np, dtype=torch.bool, device=DEV)
    good[r0:r1] = False
    assert torch.equal(O[good], Oref[good])                  # the other graphs' rows: untouched by the bad slot


@pytest.mark.parametrize("H", [None, 2])
def test_from_store_pipeline_builds_the_adjacency(H):
    """Six consecutive batches through the loader's ring of three page-locked slots."""
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    store = store_named("MUTAG")
    dg = structure_of("MUTAG", H, DEV)
    X_dev = torch.from_numpy(store.X).to(DEV)
    rng = np.random.RandomState(21)
    loader = BatchLoader(store, 32, 4, rng=rng, gather_x=False)
    assert loader.ring is not None and len(loader.ring) == 3
    made = []
    for _ in range(6):
        hb = loader()
        made.append((hb.graph_ids.copy(), DeviceBatch.from_store(hb, X_dev, DEV, graphs=dg)))
    for ids, b in made:
        assert b.adj is not None and b.adj.N == b.N
        assert_adjacency_equal(b.adj, host_adjacency(store, ids, H, DEV), "pipeline")
    plain = DeviceBatch.from_store(loader(), X_dev, DEV)
    assert plain.adj is None
    loose = store.assemble(made[0][0], 4, rng=rng, gather_x=False)           # no page-locked slot
    assert_adjacency_equal(DeviceBatch.from_store(loose, X_dev, DEV, graphs=dg).adj,
                           host_adjacency(store, made[0][0], H, DEV), "no slot")
    dg.check_indices()


def test_model_step_is_identical_under_both_adjacencies():
    """MUTAG, L 2, T 2, attention="edges", hops 2, train mode, one seed: the loss and every gradient, hop_bias included,
    bit for bit."""
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip import kernels as K
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    store = store_named("MUTAG")
    dg = structure_of("MUTAG", 2, DEV)
    X_dev = torch.from_numpy(store.X).to(DEV)
    hb = BatchLoader(store, 16, 4, rng=np.random.RandomState(8), gather_x=False)()
    ids = hb.graph_ids.copy()
    b_dev = DeviceBatch.from_store(hb, X_dev, DEV, graphs=dg)
    b_host = DeviceBatch.from_store(store.assemble(ids, 4, rng=np.random.RandomState(9), gather_x=False), X_dev, DEV)
    b_host.input_x = b_dev.input_x
    b_host.adj = host_adjacency(store, ids, 2, DEV)
    out = []
    for b in (b_dev, b_host):
        torch.manual_seed(3)
        m = TransformerU2GNN(store.d, 32, 2, 2, 0.5, 2, attention="edges", hops=2)
        with torch.no_grad():
            m.hop_bias.copy_(torch.randn(2, 2, 3, generator=torch.Generator().manual_seed(12)))
        m = m.to(DEV).train()
        flat = m.flatten_parameters()
        scores, ctx = m.core.forward(b, train=True, need_ctx=True, seed=424242)
        dsc, loss = torch.empty_like(scores), torch.zeros(1, device=DEV)
        K.smoothed_ce(scores, b.labels, b.B, 2, 0.1, loss, dsc)
        m.core.backward(ctx, dsc, flat.grads)
        torch.cuda.synchronize()
        out.append((loss.clone(), {k: v.clone() for k, v in flat.grads.items()}))
    (l0, g0), (l1, g1) = out
    assert torch.isfinite(l0).all() and torch.equal(l0, l1)
    assert set(g0) == set(g1) and "hop_bias" in g0 and g0["hop_bias"].abs().max().item() > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def _cli(script, extra, mode, tmp_path):
    run = tmp_path / mode / "run" / "x"
    run.mkdir(parents=True)
    cmd = [sys.executable, os.path.join(PKG, script), "--run_folder", str(run), "--num_epochs", "1", "--batch_size", "4",
           "--num_neighbors", "4", "--ff_hidden_size", "128", "--num_timesteps", "2", "--attention", "edges",
           "--max_steps", "3", "--adjacency", mode] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, U2GNN_PARAM_CHECKSUM="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"adjacency='{mode}'" in r.stdout                 # the argument namespace the CLI prints first
    lines = [re.sub(r"time:\s*\S+", "time: -", x) for x in r.stdout.splitlines() if x.startswith("| epoch")]
    sums = [x for x in r.stderr.splitlines() if x.startswith("param_checksum rank ")]
    assert len(lines) == 1 and len(sums) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return lines, sums


@pytest.mark.parametrize("script,extra", [
    ("train_pytorch_U2GNN_Sup.py", ["--dataset", "MUTAG", "--model_name", "MUTAG", "--hops", "2"]),
    ("train_pytorch_U2GNN_UnSup.py", ["--dataset", "MUTAG", "--model_name", "MUTAG"])])
def test_cli_prints_the_same_under_both_adjacencies(tmp_path, script, extra):
    """Fresh child processes: the epoch line (loss, accuracy; the wall time masked) and the final parameters'
    checksums are the same text with --adjacency device and --adjacency host."""
    dev = _cli(script, extra, "device", tmp_path)
    host = _cli(script, extra, "host", tmp_path)
    assert "loss" in dev[0][0]
    assert dev == host
