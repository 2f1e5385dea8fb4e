"""The shortest-path search of pattern.DeviceGraphs without a GPU: the numpy statements of the kernels
(pair_types_numpy, expand_numpy) equal the host builders, the host tables' formulas, the planning errors, and the C
entry points' argument checks.  Integers only: nothing here has a tolerance."""
import ctypes
import os

import numpy as np
import pytest

from device_distances_ref import assert_structures_equal, batches, bound_store, dist_store, structure

E_ARG, E_ALIGN, E_SHAPE = -1, -2, -3
STORES = ("MUTAG", "PTC", "synthetic", "odd", "directed", "paths")
HS = (1, 2, 3, 31)
SYMBOLS = ("u2gnn_pair_distances", "u2gnn_pair_distances_u8", "u2gnn_distance_extents", "u2gnn_hop_expand_count",
           "u2gnn_hop_expand_fill")


@pytest.mark.parametrize("name", STORES)
def test_pair_types_numpy_equals_the_stores_distances(name):
    store, dg = dist_store(name), structure(name)
    every = np.arange(dg.G)
    for H in HS:
        for ids in (every, batches(name)[-1]):
            po, et = store.distances(ids, H)
            got_po, got_et = dg.pair_types_numpy(ids, H)
            assert got_et.dtype == np.int32 and np.array_equal(got_po, po) and np.array_equal(got_et, et), (name, H)


@pytest.mark.parametrize("name", STORES)
def test_expand_numpy_equals_the_host_build(name):
    dg = structure(name)
    for H in HS:
        ref, got = structure(name, H).host, dg.expand_numpy(H)
        for k in dg.ARRAYS:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (name, H, k)


def _extents_numpy(dg):
    """(ecc31, fin31) from the numpy sweep at cap 32, as DeviceGraphs.extents defines them."""
    ecc, fin = np.zeros(dg.G, dtype=np.int64), np.zeros(dg.G, dtype=np.int64)
    for g in range(dg.G):
        D = dg._dense_numpy(g, 32)
        if D.size:
            ecc[g], fin[g] = np.minimum(D, 31).max(), D[D < 32].max()
    return ecc, fin


@pytest.mark.parametrize("name", STORES)
def test_n_types_and_max_dist_come_from_two_numbers_per_graph(name):
    store, dg = dist_store(name), structure(name)
    ecc, fin = _extents_numpy(dg)
    for H in HS:
        assert np.array_equal(np.minimum(fin, H), structure(name, H).max_dist), (name, H)
        for ids in batches(name)[:6] + batches(name)[-2:]:
            ids = np.asarray(ids, dtype=np.int64)
            want = int(store.distances(ids, H)[1].max()) + 1
            assert int(np.minimum(ecc[ids], H).max()) + 1 == want, (name, H, ids[:8])


def test_library_exports_the_entry_points_under_abi_19():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    listed = _lib.header_symbols("u2gnn_hip.h")
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in listed, s
    assert lib.u2gnn_abi_version() == _lib.ABI_VERSION == 19
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "u2gnn_hip.h")) as f:
        assert f"#define U2GNN_DIST_NODES_MAX {_lib.DIST_NODES_MAX}" in f.read()
    assert _lib.DIST_NODES_MAX >= 4096


def test_entry_points_refuse_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_* shows that nothing was launched
    (the method of tests/test_hops_cpu.py)."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    f = 1 << 40                                               # never dereferenced on the host
    members = ("node_start", "ent_start", "rowptr", "t_rowptr", "col", "t_src", "t_eid", "etype")
    P = lambda v: None if v is None else ctypes.c_void_p(v)   # noqa: E731

    def dist(fn=lib.u2gnn_pair_distances, S="ok", null=(), G=5, V=50, E=200, B=2, N=10, n_pairs=52, max_n=6, H=3,
             **ptr):
        s = None
        if S is not None:
            s = ctypes.byref(_lib.GraphStructure(*[None if k in null else f for k in members], G, V, E))
        p = {k: P(ptr.get(k, f)) for k in ("gid", "row_off", "pair_off", "out", "err")}
        return fn(s, p["gid"], p["row_off"], p["pair_off"], B, N, n_pairs, max_n, H, p["out"], p["err"], None)
    for fn in (lib.u2gnn_pair_distances, lib.u2gnn_pair_distances_u8):
        assert dist(fn, S=None) == E_ARG
        for k in ("node_start", "t_rowptr", "t_src"):
            assert dist(fn, null=(k,)) == E_ARG, k
        for k in ("gid", "row_off", "pair_off", "out", "err"):
            assert dist(fn, **{k: None}) == E_ARG, k
        for k in ("G", "V", "E", "B", "N", "n_pairs", "max_n"):
            assert dist(fn, **{k: 0}) == E_ARG, k
        assert dist(fn, B=-2) == E_ARG and dist(fn, n_pairs=-1) == E_ARG
        assert dist(fn, H=0) == E_SHAPE and dist(fn, H=33) == E_SHAPE
        assert dist(fn, max_n=_lib.DIST_NODES_MAX + 1) == E_SHAPE       # a graph above the bound: nothing launched
        for k in ("gid", "row_off", "pair_off"):
            assert dist(fn, **{k: f + 4}) == E_ALIGN, k
        assert dist(fn, err=f + 2) == E_ALIGN
    assert dist(H=32) == E_SHAPE and dist(out=f + 2) == E_ALIGN            # int32 pair types: H <= 31
    assert dist(lib.u2gnn_pair_distances_u8, out=f + 1, H=32) > 0          # bytes, cap 32: it launches

    def rest(fn, extra, B=2, N=10, n_pairs=52, max_n=6, H=3, D=f, row_off=f, pair_off=f, err=f):
        return fn(P(D), *extra[:1 if fn is lib.u2gnn_hop_expand_fill else 0], P(row_off), P(pair_off), B, N, n_pairs,
                  max_n, H, *extra[1 if fn is lib.u2gnn_hop_expand_fill else 0:], P(err), None)
    ok = [(lib.u2gnn_distance_extents, [P(f), P(f)]), (lib.u2gnn_hop_expand_count, [P(f), P(f)]),
          (lib.u2gnn_hop_expand_fill, [P(f), P(f), P(f), 77, P(f), P(f), P(f), P(f)])]
    for fn, extra in ok:
        assert rest(fn, extra) > 0                                         # the arguments are fine: a launch is tried
        for k in ("D", "row_off", "pair_off", "err"):
            assert rest(fn, extra, **{k: None}) == E_ARG, k
        for k in ("B", "N", "n_pairs", "max_n"):
            assert rest(fn, extra, **{k: 0}) == E_ARG, k
        assert rest(fn, extra, H=0) == E_SHAPE and rest(fn, extra, H=33) == E_SHAPE
        assert rest(fn, extra, max_n=_lib.DIST_NODES_MAX + 1) == E_SHAPE
        assert rest(fn, extra, row_off=f + 4) == E_ALIGN and rest(fn, extra, err=f + 1) == E_ALIGN
        for i, v in enumerate(extra):
            if isinstance(v, int):
                assert rest(fn, extra[:i] + [0] + extra[i + 1:]) == E_ARG   # E < 1
            else:
                assert rest(fn, extra[:i] + [None] + extra[i + 1:]) == E_ARG, i
    assert rest(lib.u2gnn_hop_expand_count, [P(f + 4), P(f)]) == E_ALIGN
    assert rest(lib.u2gnn_hop_expand_count, ok[1][1], H=32) == E_SHAPE       # hops end at 31


def test_kernel_wrappers_refuse_host_tensors():
    import torch
    from u2gnn_hip import _lib, kernels as K
    dg = structure("odd")
    i64 = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.U2GNNNativeError):
        K.pair_distances(dg.c_struct(), i64[:2], i64, i64, 2, 2, 1, 2, torch.zeros(2, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32))


def test_planning_errors():
    from u2gnn_hip._lib import DIST_NODES_MAX
    from u2gnn_hip.pattern import DeviceGraphs
    import u2gnn_hip.pattern as P
    dg = structure("MUTAG")
    for bad in ([dg.G], [-1], [0, 3, dg.G + 5], []):
        with pytest.raises(ValueError, match="graph id"):
            dg.plan_pairs(bad, 2)
        with pytest.raises(ValueError):
            dg.pair_types_numpy(bad, 2)
    for H in (0, 32, 1.5):
        with pytest.raises(ValueError, match="hops"):
            dg.plan_pairs([0], H)
    with pytest.raises(ValueError, match="without hops"):
        structure("MUTAG", 2).plan_pairs([0], 2)
    with pytest.raises(ValueError, match="without hops"):
        structure("MUTAG", 2).expand_numpy(2)
    big = DeviceGraphs.from_store(bound_store(), "cpu")
    assert big.plan_pairs([0], 3)[3:] == (DIST_NODES_MAX, DIST_NODES_MAX ** 2, DIST_NODES_MAX)
    with pytest.raises(ValueError, match="searches at most"):
        big.plan_pairs([0, 1], 3)
    with pytest.raises(ValueError, match="searches at most"):
        DeviceGraphs._chunks(big.n_nodes, 3, 1 << 40)
    with pytest.raises(ValueError, match="pairs"):            # more pairs than the bias reduction takes in one call
        big.plan_pairs([0] * (P.BIAS_ENTRIES_MAX // DIST_NODES_MAX ** 2 + 1), 3)
    n = dg.n_nodes
    with pytest.raises(ValueError, match="scratch_bytes"):
        DeviceGraphs._chunks(n, 3, 3 * int(n.max()) ** 2 - 1)
    chunks = DeviceGraphs._chunks(n, 3, 3 * int(n.max()) ** 2)
    assert chunks[0][0] == 0 and chunks[-1][1] == dg.G and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert len(chunks) > 1 and all(3 * int((n[a:b] ** 2).sum()) <= 3 * int(n.max()) ** 2 for a, b in chunks)
    assert DeviceGraphs._chunks(n, 3, 1 << 30) == [(0, dg.G)]
    with pytest.raises(ValueError, match="build"):
        DeviceGraphs.from_store(dist_store("odd"), "cpu", hops=2, build="gpu")


@pytest.mark.parametrize("H", [None, 2, 31])
def test_device_build_on_a_cpu_device_is_the_host_build(H):
    from u2gnn_hip.pattern import DeviceGraphs
    got = DeviceGraphs.from_store(dist_store("odd"), "cpu", hops=H, build="device", scratch_bytes=1)
    assert got.last_expand is None
    assert_structures_equal(got, structure("odd", H), H)


def test_from_store_asks_for_a_structure_with_distances():
    from u2gnn_hip.core import DeviceBatch
    with pytest.raises(ValueError, match="graphs=DeviceGraphs"):
        DeviceBatch.from_store(None, None, "cpu", graphs=None, distances=2)
