"""Helpers of the pattern.DeviceGraphs tests (CPU and GPU).  Test infrastructure only.

The stores (MUTAG, PTC, a small SyntheticStore, hand-made odd graphs), the batch forms every comparison runs over,
and the host path the device path must equal: Adjacency.from_csr(*store.adjacency(ids, hops)).  Stores and
structures are built once and shared; nothing here is modified by a test."""
import numpy as np

from edges_ref import store_of

HOPS_CPU = (None, 1, 2, 3, 31)
HOPS_GPU = (None, 2, 3)
_CACHE = {}


def odd_store():
    """A 1-node graph, a 2-node graph with one edge, an edgeless 3-node graph, a 5-node path and a 40-node star."""
    if "odd" not in _CACHE:
        from u2gnn_hip.batching import GraphStore
        from u2gnn_hip.synthetic import _Graph

        def graph(n, edges):
            e = np.array(edges, dtype=np.int64).reshape(-1, 2)
            src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])   # forward, then reversed
            return _Graph(n, 0, np.eye(n, 3, dtype=np.float32), src, dst)
        _CACHE["odd"] = GraphStore([graph(1, []), graph(2, [(0, 1)]), graph(3, []),
                                    graph(5, [(i, i + 1) for i in range(4)]), graph(40, [(0, i) for i in range(1, 40)])])
    return _CACHE["odd"]


def odd_batches():
    """Every single graph, all together, and one graph three times."""
    return [[i] for i in range(5)] + [list(range(5)), [2, 2, 2]]


def store_named(name):
    if name == "odd":
        return odd_store()
    if name == "synthetic":
        if name not in _CACHE:
            from u2gnn_hip.synthetic import SyntheticStore
            _CACHE[name] = SyntheticStore(40, 20, 4, 60, 50, 2, 8)
        return _CACHE[name]
    return store_of(name, False)[0]


def structure_of(name, hops, device="cpu"):
    key = (name, hops, str(device))
    if key not in _CACHE:
        from u2gnn_hip.pattern import DeviceGraphs
        _CACHE[key] = DeviceGraphs.from_store(store_named(name), device, hops=hops)
    return _CACHE[key]


def batches_of(G, per_size=20, sizes=(1, 4, 64)):
    """per_size seeded random batches of each size (a permutation's head, as BatchLoader draws them), a batch with a
    repeated id, one in descending id order, the first graph alone and the last graph alone."""
    rs = np.random.RandomState(2024)
    out = [rs.permutation(G)[:bs] for bs in sizes for _ in range(per_size)]
    out += [np.array([3, 7, 3, 1]), np.arange(G - 1, max(G - 12, -1), -1), np.array([0]), np.array([G - 1])]
    return out


def host_adjacency(store, ids, hops, device="cpu"):
    """Today's host path for the batch ``ids``."""
    from u2gnn_hip.pattern import Adjacency
    ids = np.asarray(ids, dtype=np.int64)
    csr = store.adjacency(ids, hops=hops)                   # (rowptr, colidx), with hops also etype
    return Adjacency.from_csr(csr[0], csr[1], int(store.n_nodes[ids].sum()), device, *csr[2:])


def assert_adjacency_equal(got, ref, what=""):
    import torch
    for f in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid"):
        a, b = getattr(got, f), getattr(ref, f)
        assert a.dtype == b.dtype == torch.int64 and torch.equal(a, b), (f, what)
    if ref.etype is None:
        assert got.etype is None, what
    else:
        assert got.etype.dtype == torch.int32 and torch.equal(got.etype, ref.etype), ("etype", what)
    assert (got.N, got.nnz, got.n_types) == (ref.N, ref.nnz, ref.n_types), what
