"""The shortest-path search on the GPU: a batch's pair types (DeviceGraphs.pair_types, u2gnn_pair_distances) equal
PairTypes.from_store of the store's distances, and the H-hop structure expanded on the GPU
(DeviceGraphs.from_store(..., build="device")) equals the host build -- the kernels alone, their exact extent, a bad
slot (the memory-safety contract), the DeviceBatch.from_store pipeline, a model step and both CLIs.  Integers only:
nothing here has a tolerance."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from device_distances_ref import assert_structures_equal, batches, dist_store, structure  # noqa: E402

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
SENTINEL = -7777


def _host_pairs(store, ids, H):
    from u2gnn_hip.pattern import PairTypes
    ids = np.asarray(ids, dtype=np.int64)
    return PairTypes.from_store(store, ids, int(store.n_nodes[ids].sum()), DEV, H)


def assert_pairs_equal(got, ref, what=""):
    assert got.pair_off.dtype == ref.pair_off.dtype == torch.int64 and torch.equal(got.pair_off, ref.pair_off), what
    assert got.etype.dtype == ref.etype.dtype == torch.int32 and torch.equal(got.etype, ref.etype), what
    assert (got.n_types, got.n_pairs, got.N) == (ref.n_types, ref.n_pairs, ref.N), what


@pytest.mark.parametrize("H", [1, 2, 3, 31])
@pytest.mark.parametrize("name", ["MUTAG", "PTC", "synthetic", "odd", "directed", "paths"])
def test_pair_types_equal_the_host_path(name, H):
    store, dg = dist_store(name), structure(name, None, DEV)
    for ids in batches(name):
        assert_pairs_equal(dg.pair_types(ids, H), _host_pairs(store, ids, H), (name, H, list(ids)[:8]))
    dg.check_indices()


def test_pair_types_of_mixed_graphs_and_given_row_offsets():
    """Directed graphs between long paths, one of them twice; the row offsets already on the device."""
    from u2gnn_hip.batching import GraphStore
    a, b = dist_store("directed"), dist_store("paths")
    store = GraphStore(a.graphs + b.graphs)
    from u2gnn_hip.pattern import DeviceGraphs
    dg = DeviceGraphs.from_store(store, DEV)
    ids = np.array([5, 0, 9, 3, 5, 1, 2, 7])
    row_off = torch.from_numpy(np.concatenate([[0], np.cumsum(store.n_nodes[ids])])).to(DEV)
    for H in (3, 31):
        ref = _host_pairs(store, ids, H)
        assert_pairs_equal(dg.pair_types(ids, H), ref, H)
        assert_pairs_equal(dg.pair_types(ids, H, row_off), ref, H)
    dg.check_indices()


def test_the_largest_graph_is_searched_and_a_larger_one_refused():
    from u2gnn_hip._lib import DIST_NODES_MAX
    store, dg = dist_store("bound"), structure("bound", None, DEV)
    assert store.n_nodes.tolist() == [DIST_NODES_MAX, DIST_NODES_MAX + 1]
    assert_pairs_equal(dg.pair_types([0], 3), _host_pairs(store, [0], 3), "bound")
    with pytest.raises(ValueError, match="searches at most"):
        dg.pair_types([1], 3)
    dg.check_indices()


def _raw_call(dg, ids, H, pad=37, gid_override=None):
    """The kernel wrapper on an output carved from a larger sentinel-filled buffer at an odd element offset."""
    from u2gnn_hip import kernels as K
    ids, row_off, pair_off, N, n_pairs, max_n = dg.plan_pairs(ids, H)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    whole = torch.full((n_pairs + 2 * pad,), SENTINEL, device=DEV, dtype=torch.int32)
    view = whole[pad:pad + n_pairs]
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    po = to(pair_off)
    K.pair_distances(dg.c_struct(), to(ids if gid_override is None else gid_override), to(row_off), po, N, n_pairs,
                     max_n, H, view, err)
    torch.cuda.synchronize()
    return view, whole, err, (row_off, pair_off, po, N, n_pairs)


@pytest.mark.parametrize("H", [2, 31])
def test_nothing_is_written_outside_the_pair_types(H):
    store, dg = dist_store("PTC"), structure("PTC", None, DEV)
    ids = np.random.RandomState(3).permutation(len(store.n_nodes))[:40]
    view, whole, err, _ = _raw_call(dg, ids, H)
    assert int(err.item()) == 0
    assert torch.equal(view, _host_pairs(store, ids, H).etype)
    assert (whole[:37] == SENTINEL).all() and (whole[37 + view.numel():] == SENTINEL).all()
    # the byte form, as the expansion takes it
    from u2gnn_hip import kernels as K
    _, row_off, pair_off, N, n_pairs, max_n = dg.plan_pairs(ids, H)
    to = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    w8 = torch.full((n_pairs + 74,), 201, device=DEV, dtype=torch.uint8)
    K.pair_distances(dg.c_struct(), to(ids), to(row_off), to(pair_off), N, n_pairs, max_n, H + 1, w8[37:37 + n_pairs], err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and (w8[:37] == 201).all() and (w8[37 + n_pairs:] == 201).all()
    ref = _host_pairs(store, ids, min(H + 1, 31)).etype if H < 31 else None
    if ref is not None:
        assert torch.equal(w8[37:37 + n_pairs].int(), ref)


def test_a_bad_slot_is_flagged_and_written_as_type_0():
    """The memory-safety contract: a graph id outside [0, G) that reaches the kernel (the host check bypassed) sets the
    err flag, its slot's pairs become 0, every other slot equals the host path, and the biased attention forward over
    the result leaves finite output."""
    from u2gnn_hip import kernels as K
    from u2gnn_hip.engine import row_pad
    store, dg = dist_store("MUTAG"), structure("MUTAG", None, DEV)
    ids = np.array([4, 60, 17, 99, 120, 33])
    bad, H = 3, 2
    for wrong in (dg.G, -1, 1 << 40):
        gid = ids.copy()
        gid[bad] = wrong
        view, _, err, (row_off, pair_off, po, N, n_pairs) = _raw_call(dg, ids, H, gid_override=gid)
        assert int(err.item()) == 1
        ref = _host_pairs(store, ids, H).etype
        p0, p1 = int(pair_off[bad]), int(pair_off[bad + 1])
        keep = torch.ones(n_pairs, dtype=torch.bool, device=DEV)
        keep[p0:p1] = False
        assert (view[p0:p1] == 0).all() and torch.equal(view[keep], ref[keep])
    dp, Np = 64, row_pad(N)
    QKV = torch.randn(Np, 3 * dp, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    QKV[:, :dp] *= 1 / math.sqrt(dp)
    tables = torch.randn(1, H + 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    bias = torch.empty(1, n_pairs + (-n_pairs) % 4, device=DEV)
    K.bias_expand(tables, view.clone(), bias)
    O = torch.full((Np, dp), float("nan"), device=DEV)
    stats = torch.full((Np, 2), float("nan"), device=DEV)
    off = torch.from_numpy(row_off).to(DEV)
    K.segment_attn_fwd_bias(QKV, dp, off, po, bias[0, :n_pairs], O, stats, 0.0, 11, N, Np)
    torch.cuda.synchronize()
    assert torch.isfinite(O[:N]).all()


@pytest.mark.parametrize("name,H", [(n, h) for n in ("MUTAG", "PTC", "synthetic", "odd", "directed") for h in (2, 3)]
                         + [("MUTAG", 31), ("paths", 3)])
def test_device_build_equals_the_host_build(name, H):
    from u2gnn_hip.pattern import DeviceGraphs
    ref = structure(name, H, "cpu")
    got = DeviceGraphs.from_store(dist_store(name), DEV, hops=H, build="device")
    assert got.last_expand[0] == 1
    for k in got.ARRAYS:
        assert got.dev[k].is_cuda and got.dev[k].dtype == torch.from_numpy(ref.host[k]).dtype, k
    assert_structures_equal(got, ref, (name, H))
    ids = batches(name)[-1]
    for a, b in zip(got.assemble_numpy(ids), ref.assemble_numpy(ids)):    # the arrays copied back on first use
        assert np.array_equal(a, b)


def test_device_build_in_several_chunks_gives_the_same_arrays():
    from u2gnn_hip.pattern import DeviceGraphs
    store = dist_store("PTC")
    scratch = 3 * int(store.n_nodes.max()) ** 2 + 4000
    got = DeviceGraphs.from_store(store, DEV, hops=3, build="device", scratch_bytes=scratch)
    assert got.last_expand[0] > 4 and got.last_expand[1] <= scratch + 16
    assert_structures_equal(got, structure("PTC", 3, "cpu"), "chunks")
    with pytest.raises(ValueError, match="scratch_bytes"):
        DeviceGraphs.from_store(store, DEV, hops=3, build="device", scratch_bytes=3 * int(store.n_nodes.max()) ** 2 - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        DeviceGraphs.from_store(store, DEV, hops=3, build="device", max_bytes=got.nbytes(got.G, got.V, got.E, 3) - 1)


def test_batch_adjacency_of_a_device_built_structure():
    from device_graphs_ref import assert_adjacency_equal, host_adjacency
    from u2gnn_hip.pattern import DeviceGraphs
    store = dist_store("MUTAG")
    dg = DeviceGraphs.from_store(store, DEV, hops=3, build="device")
    for ids in batches("MUTAG")[:4]:
        assert_adjacency_equal(dg.adjacency(ids), host_adjacency(store, ids, 3, DEV), "device-built")
    dg.check_indices()


def test_from_store_pipeline_builds_the_pair_types():
    """Six consecutive batches through the loader's ring of three page-locked slots."""
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    store, dg = dist_store("MUTAG"), structure("MUTAG", None, DEV)
    X_dev = torch.from_numpy(store.X).to(DEV)
    rng = np.random.RandomState(21)
    loader = BatchLoader(store, 32, 4, rng=rng, gather_x=False)
    assert loader.ring is not None and len(loader.ring) == 3
    made = []
    for _ in range(6):
        hb = loader()
        made.append((hb.graph_ids.copy(), DeviceBatch.from_store(hb, X_dev, DEV, graphs=dg, distances=2)))
    for ids, b in made:
        assert b.adj is None and b.pairs is not None and b.pairs.N == b.N
        assert_pairs_equal(b.pairs, _host_pairs(store, ids, 2), "pipeline")
    plain = DeviceBatch.from_store(loader(), X_dev, DEV, graphs=dg)
    assert plain.pairs is None and plain.adj is not None
    loose = store.assemble(made[0][0], 4, rng=rng, gather_x=False)           # no page-locked slot
    assert_pairs_equal(DeviceBatch.from_store(loose, X_dev, DEV, graphs=dg, distances=2).pairs,
                       _host_pairs(store, made[0][0], 2), "no slot")
    dg.check_indices()


def test_model_step_is_identical_under_both_pair_types():
    """MUTAG, L 2, T 2, attention="graphs", distances 2, train mode, one seed: the loss and every gradient, hop_bias
    included, bit for bit."""
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip import kernels as K
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    store, dg = dist_store("MUTAG"), structure("MUTAG", None, DEV)
    X_dev = torch.from_numpy(store.X).to(DEV)
    hb = BatchLoader(store, 16, 4, rng=np.random.RandomState(8), gather_x=False)()
    ids = hb.graph_ids.copy()
    b_dev = DeviceBatch.from_store(hb, X_dev, DEV, graphs=dg, distances=2)
    b_host = DeviceBatch.from_store(store.assemble(ids, 4, rng=np.random.RandomState(9), gather_x=False), X_dev, DEV)
    b_host.input_x = b_dev.input_x
    b_host.pairs = _host_pairs(store, ids, 2)
    out = []
    for b in (b_dev, b_host):
        torch.manual_seed(3)
        m = TransformerU2GNN(store.d, 32, 2, 2, 0.5, 2, attention="graphs", distances=2)
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
           "--num_neighbors", "4", "--ff_hidden_size", "128", "--num_timesteps", "2", "--max_steps", "3",
           "--dataset", "MUTAG", "--model_name", "MUTAG", "--adjacency", mode] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, U2GNN_PARAM_CHECKSUM="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"adjacency='{mode}'" in r.stdout                 # the argument namespace the CLI prints first
    assert "on the host" not in r.stdout                     # the device route served the run
    lines = [re.sub(r"time:\s*\S+", "time: -", x) for x in r.stdout.splitlines() if x.startswith("| epoch")]
    sums = [x for x in r.stderr.splitlines() if x.startswith("param_checksum rank ")]
    assert len(lines) == 1 and len(sums) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return lines, sums


@pytest.mark.parametrize("script,extra", [
    ("train_pytorch_U2GNN_Sup.py", ["--attention", "graphs", "--distances", "2"]),
    ("train_pytorch_U2GNN_UnSup.py", ["--attention", "graphs", "--distances", "2"]),
    ("train_pytorch_U2GNN_Sup.py", ["--attention", "edges", "--hops", "3"])])
def test_cli_prints_the_same_under_both_adjacencies(tmp_path, script, extra):
    """Fresh child processes: the epoch line (loss, accuracy; the wall time masked) and the final parameters'
    checksums are the same text with --adjacency device and --adjacency host."""
    dev = _cli(script, extra, "device", tmp_path)
    host = _cli(script, extra, "host", tmp_path)
    assert "loss" in dev[0][0]
    assert dev == host
