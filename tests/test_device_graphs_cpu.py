"""pattern.DeviceGraphs without a GPU: the numpy statement of the batch assembly (assemble_numpy, and the host tables'
N / nnz / n_types) equals the host path Adjacency.from_csr(*store.adjacency(ids, hops)) integer for integer, on the
datasets, a synthetic store and hand-made odd graphs; what it refuses; and the new entry point under ABI 19."""
import ctypes

import numpy as np
import pytest

from device_graphs_ref import (HOPS_CPU, batches_of, host_adjacency, odd_batches, odd_store, store_named,
                               structure_of)

E_ARG = -1
FIELDS = ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid")


def _check(dg, store, ids, H):
    ref = host_adjacency(store, ids, H)
    got = dg.assemble_numpy(ids)
    for name, g in zip(FIELDS, got):
        r = getattr(ref, name).numpy()
        assert g.dtype == np.int64 and np.array_equal(g, r), (name, list(ids)[:8], H)
    if H is None:
        assert got[5] is None and ref.etype is None
    else:
        assert got[5].dtype == np.int32 and np.array_equal(got[5], ref.etype.numpy()), ("etype", list(ids)[:8], H)
    _, row_off, ent_off, N, nnz, n_types = dg.plan(ids)
    assert (N, nnz, n_types) == (ref.N, ref.nnz, ref.n_types), (list(ids)[:8], H)
    assert row_off[-1] == N and ent_off[-1] == nnz and len(row_off) == len(ent_off) == len(ids) + 1


@pytest.mark.parametrize("H", HOPS_CPU)
@pytest.mark.parametrize("name", ["MUTAG", "PTC", "synthetic"])
def test_assemble_numpy_equals_the_host_path(name, H):
    store = store_named(name)
    dg = structure_of(name, H)
    G = len(store.n_nodes)
    assert (dg.G, dg.V, dg.hops) == (G, int(store.n_nodes.sum()), H)
    for ids in batches_of(G):
        _check(dg, store, ids, H)


@pytest.mark.parametrize("H", HOPS_CPU)
def test_odd_graphs(H):
    store = odd_store()
    dg = structure_of("odd", H)
    for ids in odd_batches():
        _check(dg, store, ids, H)


def test_structure_arrays_have_the_documented_types():
    dg = structure_of("MUTAG", 2)
    h = dg.host
    for k in ("node_start", "ent_start", "rowptr", "t_rowptr"):
        assert h[k].dtype == np.int64
    for k in ("col", "t_src", "t_eid"):
        assert h[k].dtype == np.int32 and h[k].shape == (dg.E,)
    assert h["etype"].dtype == np.uint8 and h["etype"].shape == (dg.E,)
    assert h["node_start"].shape == h["ent_start"].shape == (dg.G + 1,)
    assert h["rowptr"].shape == h["t_rowptr"].shape == (dg.V + 1,)
    assert structure_of("MUTAG", None).host["etype"] is None
    assert sum(a.nbytes for a in h.values()) == dg.nbytes(dg.G, dg.V, dg.E, 2)
    assert int(dg.max_dist.max()) == 2 and dg.max_dist.shape == (dg.G,)


def test_too_large_a_structure_is_refused_before_anything_is_allocated(monkeypatch):
    import torch
    from u2gnn_hip.pattern import DeviceGraphs
    store = store_named("MUTAG")

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the size check")
    monkeypatch.setattr(torch, "from_numpy", no_alloc)
    monkeypatch.setattr(torch, "zeros", no_alloc)
    monkeypatch.setattr(torch, "empty", no_alloc)
    with pytest.raises(ValueError, match="max_bytes"):
        DeviceGraphs.from_store(store, "cpu", max_bytes=1)
    dg = structure_of("MUTAG", None)
    need = dg.nbytes(dg.G, dg.V, dg.E, None)
    with pytest.raises(ValueError, match="max_bytes"):      # the exact size, known only from the entry count
        DeviceGraphs.from_store(store, "cpu", max_bytes=need - 1)
    monkeypatch.undo()
    assert DeviceGraphs.from_store(store, "cpu", max_bytes=need).E == dg.E


def test_bad_hops_and_bad_ids_are_refused():
    from u2gnn_hip.pattern import DeviceGraphs
    store = store_named("MUTAG")
    for bad in (-1, 32, 1.5):
        with pytest.raises(ValueError):
            DeviceGraphs.from_store(store, "cpu", hops=bad)
    dg = structure_of("MUTAG", None)
    for bad in ([dg.G], [-1], [0, 3, dg.G + 5], []):
        with pytest.raises(ValueError):
            dg.adjacency(bad)
        with pytest.raises(ValueError):
            dg.assemble_numpy(bad)


def test_library_exports_the_entry_point_under_abi_19():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    assert hasattr(lib, "u2gnn_adjacency_assemble")
    assert "u2gnn_adjacency_assemble" in _lib.header_symbols("u2gnn_hip.h")
    assert lib.u2gnn_abi_version() == _lib.ABI_VERSION == 19


def test_entry_point_refuses_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_ARG shows that nothing was
    launched (the method of tests/test_edges_mode_cpu.py)."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    f = 1 << 40                                               # never dereferenced on the host
    members = ("node_start", "ent_start", "rowptr", "t_rowptr", "col", "t_src", "t_eid", "etype")

    def call(S="ok", null=(), G=5, V=50, E=200, B=2, N=10, nnz=40, **ptr):
        s = None
        if S is not None:
            s = ctypes.byref(_lib.GraphStructure(*[None if k in null else f for k in members], G, V, E))
        names = ("gid", "row_off", "ent_off", "rowptr", "colidx", "t_rowptr", "t_src", "t_eid", "etype", "err")
        p = {k: ptr.get(k, ctypes.c_void_p(f)) for k in names}
        return lib.u2gnn_adjacency_assemble(s, p["gid"], p["row_off"], p["ent_off"], B, N, nnz, p["rowptr"], p["colidx"],
                                            p["t_rowptr"], p["t_src"], p["t_eid"], p["etype"], p["err"], None)
    assert call(S=None) == E_ARG
    for k in members[:-1]:
        assert call(null=(k,)) == E_ARG, k
    assert call(null=("etype",)) == E_ARG                     # etype asked of a structure without one
    for k in ("gid", "row_off", "ent_off", "rowptr", "colidx", "t_rowptr", "t_src", "t_eid", "err"):
        assert call(**{k: None}) == E_ARG, k
    for k in ("G", "V", "E", "B", "N", "nnz"):
        assert call(**{k: 0}) == E_ARG, k
    assert call(B=-3) == E_ARG and call(N=-1) == E_ARG and call(nnz=-1) == E_ARG
