"""Helpers of the device shortest-path tests (CPU and GPU).  Test infrastructure only.

The stores of device_graphs_ref plus hand-made graphs with one-way edges, components and long paths, the one-hop
structures the device searches from, and the host paths every result must equal: ``store.distances`` /
``PairTypes.from_store`` and the host-built ``DeviceGraphs``.  Everything is built once and shared; nothing here is
modified by a test."""
import numpy as np

from device_graphs_ref import batches_of, odd_batches, store_named

_CACHE = {}
PATHS = (63, 64, 65, 255, 256, 257)     # diameters above 31; a row crosses every lane and block boundary


def _store(graphs):
    from u2gnn_hip.batching import GraphStore
    from u2gnn_hip.synthetic import _Graph
    out = []
    for n, edges in graphs:
        e = np.array(edges, dtype=np.int64).reshape(-1, 2)
        out.append(_Graph(n, 0, np.eye(n, 3, dtype=np.float32), e[:, 0], e[:, 1]))     # one-way: exactly as listed
    return GraphStore(out)


def path(n, lo=0):
    """The two-way path lo, lo + 1, ..., lo + n - 1."""
    fwd = [(lo + i, lo + i + 1) for i in range(n - 1)]
    return fwd + [(b, a) for a, b in fwd]


def directed_store():
    """A 4-node one-way chain, a 6-node one-way ring with a self loop, a graph with a repeated edge, and two 5-node
    paths as one 10-node graph."""
    if "directed" not in _CACHE:
        _CACHE["directed"] = _store([
            (4, [(0, 1), (1, 2), (2, 3)]),
            (6, [(i, (i + 1) % 6) for i in range(6)] + [(2, 2)]),
            (5, [(0, 1), (0, 1), (1, 0), (1, 2), (2, 3), (3, 1), (0, 1)]),
            (10, path(5) + path(5, 5))])
    return _CACHE["directed"]


def paths_store():
    if "paths" not in _CACHE:
        _CACHE["paths"] = _store([(n, path(n)) for n in PATHS])
    return _CACHE["paths"]


def bound_store():
    """A path of exactly DIST_NODES_MAX nodes, and one of a node more."""
    if "bound" not in _CACHE:
        from u2gnn_hip._lib import DIST_NODES_MAX
        _CACHE["bound"] = _store([(DIST_NODES_MAX, path(DIST_NODES_MAX)), (DIST_NODES_MAX + 1, path(DIST_NODES_MAX + 1))])
    return _CACHE["bound"]


def dist_store(name):
    """A store with both ``adjacency`` and ``distances`` (the synthetic one as a GraphStore)."""
    if name == "directed":
        return directed_store()
    if name == "paths":
        return paths_store()
    if name == "bound":
        return bound_store()
    if name == "synthetic":
        if "synthetic" not in _CACHE:
            from u2gnn_hip.synthetic import as_graph_store
            _CACHE["synthetic"] = as_graph_store(store_named("synthetic"))
        return _CACHE["synthetic"]
    return store_named(name)


def batches(name):
    G = len(dist_store(name).n_nodes)
    if name == "odd":
        return odd_batches()
    if name in ("directed", "paths"):
        return [[g] for g in range(G)] + [list(range(G)), [1, 1, 0]]
    return batches_of(G, per_size=3)


def structure(name, hops=None, device="cpu", **kw):
    """DeviceGraphs.from_store of the named store, kept (the host build unless ``kw`` says otherwise)."""
    key = ("dg", name, hops, str(device), tuple(sorted(kw.items())))
    if key not in _CACHE:
        from u2gnn_hip.pattern import DeviceGraphs
        _CACHE[key] = DeviceGraphs.from_store(dist_store(name), device, hops=hops, **kw)
    return _CACHE[key]


def assert_structures_equal(got, ref, what=""):
    """Two DeviceGraphs: the eight arrays (dtype and value), n_entries and max_dist."""
    for k in got.ARRAYS:
        a, b = got.host[k], ref.host[k]
        assert (a is None) == (b is None), (k, what)
        if a is not None:
            assert a.dtype == b.dtype and np.array_equal(a, b), (k, what)
    assert np.array_equal(got.n_entries, ref.n_entries) and np.array_equal(got.max_dist, ref.max_dist), what
    assert (got.G, got.V, got.E, got.hops) == (ref.G, ref.V, ref.E, ref.hops), what
