"""Host batch assembly, vectorised and bit-exact with the reference's per-node Python loop.

Reference: get_batch_data / Batch_Loader (train_pytorch_U2GNN_Sup.py:58-126,
train_pytorch_U2GNN_UnSup.py:59-134).  The reference builds a dict of neighbour lists over
the concatenated edge_mat (forward edges then reversed, in file order) and draws
``np.random.choice(nbrs, k, replace=True)`` node by node from the global numpy stream.
``np.random.randint(0, deg[:, None], size=(n, k))`` consumes that stream identically (one
bounded draw per element, row-major; deg == 1 draws nothing in both), so the vectorised
version below yields the same ``input_x`` and leaves the stream in the same state.

``GraphStore`` precomputes, once per dataset, each graph's neighbour CSR in reference order,
so a batch costs O(N*k) work instead of a Python loop over every directed edge.  The production
path (``assemble``) runs that O(N*k) loop natively (csrc/batch_assembly.cpp, u2gnn_batch_assemble):
it continues numpy's MT19937 state in C++ exactly as the randint call below does, ~10x faster than
numpy's broadcast randint (which alone costs ~2 ms per 64-graph COLLAB batch, more than a GPU
step); ``assemble_numpy`` is the numpy form, kept as the readable statement and the test reference.
"""
from __future__ import annotations

import ctypes

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class HostBatch:
    input_x: np.ndarray      # int64 [N, k+1]
    offsets: np.ndarray      # int64 [B+1]
    X_concat: np.ndarray     # f32 [N, d]
    labels: np.ndarray       # int64 [B]
    graph_ids: np.ndarray    # int64 [B] (indices into the store's graph list)
    input_y: Optional[np.ndarray] = None   # int64 [N] global node ids (UnSup)
    gnode: Optional[np.ndarray] = None     # int64 [N] dataset node id of each row (native assembly)
    pinned: Optional["PinnedSlot"] = None  # page-locked buffers the arrays above live in

    @property
    def N(self):
        return int(self.offsets[-1])


def csr_with_self(N: int, rows: np.ndarray, cols: np.ndarray):
    """(rowptr [N+1], colidx [nnz]), int64: the entries (rows[e], cols[e]) plus the diagonal, every row sorted by
    column and without repeats."""
    diag = np.arange(N, dtype=np.int64)
    keys = np.unique(np.concatenate([np.asarray(rows, dtype=np.int64), diag]) * max(N, 1)
                     + np.concatenate([np.asarray(cols, dtype=np.int64), diag]))
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // max(N, 1), minlength=N), out=rowptr[1:])
    return rowptr, np.ascontiguousarray(keys % max(N, 1))


def hop_lists(n: int, deg: np.ndarray, start: np.ndarray, nbr: np.ndarray, hops: int):
    """One graph's ``hops``-hop lists in its local numbering: (counts int32 [n], cols int32 [nnz], dist uint8 [nnz]) --
    row i lists every node within shortest-path distance <= hops of i (itself at distance 0), columns ascending.
    Node i's neighbours are nbr[start[i] .. start[i] + deg[i]) (local ids; repeats are harmless).  A breadth-first
    sweep from all sources at once over (source, node) pairs: the frontier of distance h is every neighbour of the
    frontier of h - 1 that no earlier frontier reached.  numpy only."""
    n1 = max(n, 1)
    seen = np.arange(n, dtype=np.int64) * (n + 1)                  # keys source * n + node, sorted: the diagonal
    keys, dist = [seen], [np.zeros(n, dtype=np.uint8)]
    frontier = seen
    for h in range(1, hops + 1):
        src, node = frontier // n1, frontier % n1
        d = deg[node]
        total = int(d.sum())
        if total == 0:
            break
        pos = np.repeat(start[node] - (np.cumsum(d) - d), d) + np.arange(total, dtype=np.int64)
        frontier = np.setdiff1d(np.repeat(src, d) * n + nbr[pos], seen)
        if frontier.size == 0:
            break
        seen = np.union1d(seen, frontier)
        keys.append(frontier)
        dist.append(np.full(frontier.size, h, dtype=np.uint8))
    keys, dist = np.concatenate(keys), np.concatenate(dist)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    return np.bincount(keys // n1, minlength=n).astype(np.int32), (keys % n1).astype(np.int32), dist[order]


def batch_hop_lists(lists, sizes: np.ndarray):
    """(rowptr int64 [N+1], colidx int64 [nnz], etype int32 [nnz]) of a batch from its graphs' ``hop_lists`` (in batch
    order) and node counts: the lists concatenated, the columns moved to the batch's row numbering."""
    offsets = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    rowptr = np.zeros(int(offsets[-1]) + 1, dtype=np.int64)
    if not lists:
        return rowptr, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    np.cumsum(np.concatenate([c for c, _, _ in lists]), out=rowptr[1:])
    per_graph = np.array([len(c) for _, c, _ in lists], dtype=np.int64)
    colidx = np.concatenate([c for _, c, _ in lists]).astype(np.int64) + np.repeat(offsets[:-1], per_graph)
    return rowptr, colidx, np.concatenate([d for _, _, d in lists]).astype(np.int32)


def pair_block(lists, n: int, H: int) -> np.ndarray:
    """One graph's pair types from its ``hop_lists(…, H)``: uint8 [n * n], row-major [node][node], entry (i, j) =
    min(distance(i, j), H), and H where no path joins i and j -- filled with H, then the listed distances scattered."""
    counts, cols, dist = lists
    block = np.full(n * n, H, dtype=np.uint8)
    block[np.repeat(np.arange(n, dtype=np.int64), counts) * n + cols] = dist
    return block


def check_hops_range(hops) -> int:
    if int(hops) != hops or not 1 <= int(hops) <= 31:
        raise ValueError(f"adjacency: hops must be an integer in [1, 31], got {hops!r}")
    return int(hops)


class GraphStore:
    """Per-dataset arrays: node features, labels, neighbour CSR in the reference's order."""

    def __init__(self, graphs: Sequence, reddit_tile: int = 0):
        self.graphs = list(graphs)
        n = np.array([g.n if hasattr(g, "n") else len(g.g) for g in self.graphs], dtype=np.int64)
        self.n_nodes = n
        self.node_start = np.zeros(len(n) + 1, dtype=np.int64)
        np.cumsum(n, out=self.node_start[1:])
        self.labels = np.array([g.label for g in self.graphs], dtype=np.int64)
        feats = np.concatenate([g.node_features for g in self.graphs], 0).astype(np.float32)
        if reddit_tile:
            # train_pytorch_U2GNN_Sup.py:93-95 (REDDIT*): tile to 4 columns, scale 0.01
            feats = (np.tile(feats, reddit_tile) * 0.01).astype(np.float32)
        self.X = feats
        # neighbour lists: stable sort of each graph's edge_mat by source keeps file order
        deg_all = np.zeros(int(self.node_start[-1]), dtype=np.int64)
        nbr_chunks = []
        for gi, g in enumerate(self.graphs):
            em = np.asarray(g.edge_mat, dtype=np.int64).reshape(2, -1)
            if em.shape[1] == 0:
                nbr_chunks.append(np.zeros(0, dtype=np.int64))
                continue
            order = np.argsort(em[0], kind="stable")
            nbr_chunks.append(em[1][order])
            deg_all[self.node_start[gi]:self.node_start[gi + 1]] = np.bincount(em[0], minlength=int(n[gi]))
        self.deg = deg_all
        self.nbr = np.ascontiguousarray(np.concatenate(nbr_chunks) if nbr_chunks else np.zeros(0, dtype=np.int64),
                                        dtype=np.int64)   # local ids
        self.nbr_start = np.zeros(len(deg_all) + 1, dtype=np.int64)
        np.cumsum(deg_all, out=self.nbr_start[1:])
        self.d = self.X.shape[1]

    def degrees_of(self, ids) -> np.ndarray:
        return np.concatenate([self.deg[self.node_start[i]:self.node_start[i + 1]] for i in ids])

    def _hop_lists(self, gi: int, hops: int):
        """Graph ``gi``'s lists (``hop_lists``), computed on first use and kept in the store."""
        cache = self.__dict__.setdefault("_hop_cache", {}).setdefault(hops, {})
        hit = cache.get(gi)
        if hit is None:
            n, lo = int(self.n_nodes[gi]), int(self.node_start[gi])
            hit = cache[gi] = hop_lists(n, self.deg[lo:lo + n], self.nbr_start[lo:lo + n], self.nbr, hops)
        return hit

    def adjacency(self, graph_ids: Sequence[int], hops: Optional[int] = None):
        """(rowptr [N+1], colidx [nnz]), int64, of the batch ``graph_ids`` in the batch's row numbering (graph
        ``graph_ids[g]`` = rows offsets[g] .. offsets[g+1]-1, as ``assemble`` lays them out): row i lists itself and
        its graph neighbours, sorted and without repeats -- what attention="edges" attends over
        (``core.Adjacency.from_csr``).  Deterministic: nothing is drawn from any RNG.

        hops = H (1 <= H <= 31): (rowptr, colidx, etype) instead -- row i lists every node of its graph within
        shortest-path distance <= H, itself included (unreachable nodes never), sorted and without repeats, and
        etype[e] (int32) is that distance, 0 on the diagonal.  H = 1 gives the rowptr / colidx above.  A graph's
        lists do not depend on the batch: they are computed on first use and kept in the store (``_hop_lists``), a
        batch concatenates them."""
        if hops is not None:
            hops = check_hops_range(hops)
            ids = np.asarray(graph_ids, dtype=np.int64)
            return batch_hop_lists([self._hop_lists(int(g), hops) for g in ids], self.n_nodes[ids])
        ids = np.asarray(graph_ids, dtype=np.int64)
        sizes = self.n_nodes[ids]
        offsets = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        N = int(offsets[-1])
        rowbase = np.repeat(offsets[:-1], sizes)                     # first batch row of each row's graph
        gnode = np.repeat(self.node_start[ids], sizes) + (np.arange(N, dtype=np.int64) - rowbase)
        deg = self.deg[gnode]
        first = np.cumsum(deg) - deg                                 # each row's first entry in the batch's list
        pos = np.repeat(self.nbr_start[gnode] - first, deg) + np.arange(int(deg.sum()), dtype=np.int64)
        return csr_with_self(N, np.repeat(np.arange(N, dtype=np.int64), deg), self.nbr[pos] + np.repeat(rowbase, deg))

    def _pair_block(self, gi: int, H: int) -> np.ndarray:
        """Graph ``gi``'s pair types (``pair_block``), computed on first use and kept in the store as uint8."""
        cache = self.__dict__.setdefault("_pair_cache", {}).setdefault(H, {})
        hit = cache.get(gi)
        if hit is None:
            hit = cache[gi] = pair_block(self._hop_lists(gi, H), int(self.n_nodes[gi]), H)
        return hit

    def distances(self, graph_ids: Sequence[int], H: int, out=None):
        """(pair_off int64 [B+1], etype int32 [sum n_b^2]): the pair types of the batch ``graph_ids`` in packed order --
        what attention="graphs" with ``distances=H`` (1 <= H <= 31) indexes its hop_bias tables with.  Graph b of the
        batch owns the entries pair_off[b] .. pair_off[b+1]-1, row-major [n_b][n_b]: entry pair_off[b] + (i - lo) *
        n_b + (j - lo) is min(shortest-path distance of rows i and j, H), and H when no path joins them (0 on the
        diagonal).  A graph's block does not depend on the batch: it is computed on first use and kept in the store
        (uint8), a batch concatenates the blocks.  Deterministic: nothing is drawn from any RNG.
        out: an int32 array of at least sum n_b^2 entries that receives etype (a page-locked buffer)."""
        H = check_hops_range(H)
        ids = np.asarray(graph_ids, dtype=np.int64).reshape(-1)
        n = self.n_nodes[ids]
        pair_off = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(n * n, out=pair_off[1:])
        total = int(pair_off[-1])
        etype = np.empty(total, dtype=np.int32) if out is None else out[:total]
        for b, g in enumerate(ids):
            etype[pair_off[b]:pair_off[b + 1]] = self._pair_block(int(g), H)
        return pair_off, etype

    def assemble(self, graph_ids: Sequence[int], num_neighbors: int, rng=np.random,
                 with_input_y: bool = False, gather_x: bool = True, out=None) -> HostBatch:
        """get_batch_data for the graphs ``graph_ids`` (in that order), natively (see module doc).
        gather_x=False leaves X_concat None and returns the rows' dataset node ids in ``gnode`` (the
        caller gathers the features on the GPU from a device-resident copy of ``X``).  out: a
        PinnedSlot whose page-locked buffers receive input_x / offsets / gnode / labels (no copy
        before the asynchronous H2D of DeviceBatch.from_store)."""
        from ._lib import lus_lib
        ids = np.ascontiguousarray(graph_ids, dtype=np.int64)
        st = rng.get_state()
        if st[0] != "MT19937":
            raise ValueError("the reference stream is numpy's legacy MT19937 RandomState")
        key = np.array(st[1], dtype=np.uint32)
        pos = ctypes.c_int32(int(st[2]))
        k = int(num_neighbors)
        N = int(self.n_nodes[ids].sum())
        if out is not None:
            out.wait()   # the slot's previous H2D copies are done
            offsets, input_x, gnode = out.views(len(ids), N, k)
            labels = out.labels_view(len(ids))
            np.take(self.labels, ids, out=labels)
        else:
            offsets = np.empty(len(ids) + 1, dtype=np.int64)
            input_x = np.empty((N, k + 1), dtype=np.int64)
            gnode = np.empty(N, dtype=np.int64)
            labels = self.labels[ids]
        p = lambda a: a.ctypes.data  # noqa: E731
        rc = lus_lib().u2gnn_batch_assemble(p(key), ctypes.byref(pos), p(ids), len(ids), p(self.n_nodes),
                                            p(self.node_start), p(self.deg), p(self.nbr_start), p(self.nbr), k, N,
                                            p(offsets), p(input_x), p(gnode))
        if rc != 0:
            raise ValueError(f"u2gnn_batch_assemble failed ({rc})")
        rng.set_state((st[0], key, pos.value, st[3], st[4]))
        X = self.X[gnode] if gather_x else None
        iy = (gnode if out is not None else gnode.copy()) if with_input_y else None
        hb = HostBatch(input_x, offsets, X, labels, ids, iy, gnode)
        hb.pinned = out
        return hb

    def assemble_numpy(self, graph_ids: Sequence[int], num_neighbors: int, rng=np.random,
                       with_input_y: bool = False) -> HostBatch:
        """get_batch_data for the graphs ``graph_ids`` (in that order), numpy form."""
        ids = np.asarray(graph_ids, dtype=np.int64)
        sizes = self.n_nodes[ids]
        offsets = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        N = int(offsets[-1])
        # global node ids of the batch nodes (contiguous per graph)
        gnode = np.concatenate([np.arange(self.node_start[i], self.node_start[i + 1]) for i in ids]) if N else \
            np.zeros(0, dtype=np.int64)
        X = self.X[gnode]
        deg = self.deg[gnode]
        k = num_neighbors
        input_x = np.repeat(np.arange(N, dtype=np.int64)[:, None], k + 1, axis=1)
        live = np.nonzero(deg > 0)[0]
        if len(live):
            draws = rng.randint(0, deg[live][:, None], size=(len(live), k))
            base = self.nbr_start[gnode[live]]
            local = self.nbr[base[:, None] + draws]                 # neighbour id within its graph
            gpos = np.repeat(np.arange(len(ids)), sizes)[live]      # batch graph index of each node
            input_x[live, 1:] = local + offsets[gpos][:, None]
        iy = gnode.copy() if with_input_y else None
        return HostBatch(input_x, offsets, X, self.labels[ids], ids, iy)


class PinnedSlot:
    """Page-locked host buffers for one in-flight batch (input_x, offsets, gnode, labels) and the
    event recorded after their H2D copies; a ring of these lets the host assemble batch i+1 while
    the copies of batch i are still queued, without a synchronous pageable copy."""

    def __init__(self, max_rows: int, max_graphs: int, k: int):
        import torch
        self.ix = torch.empty(max_rows * (k + 1), dtype=torch.int64, pin_memory=True)
        self.gnode = torch.empty(max_rows, dtype=torch.int64, pin_memory=True)
        self.offsets = torch.empty(max_graphs + 1, dtype=torch.int64, pin_memory=True)
        self.labels = torch.empty(max_graphs, dtype=torch.int64, pin_memory=True)
        # DeviceBatch.from_store(..., graphs=): the batch's graph ids and entry offsets (pattern.DeviceGraphs.plan)
        self.gid = torch.empty(max_graphs, dtype=torch.int64, pin_memory=True)
        self.ent_off = torch.empty(max_graphs + 1, dtype=torch.int64, pin_memory=True)
        self.event = None

    def wait(self):
        if self.event is not None:
            self.event.synchronize()
            self.event = None

    def views(self, n_graphs: int, N: int, k: int):
        return (self.offsets.numpy()[:n_graphs + 1], self.ix.numpy()[:N * (k + 1)].reshape(N, k + 1),
                self.gnode.numpy()[:N])

    def labels_view(self, n_graphs: int):
        return self.labels.numpy()[:n_graphs]


class BatchLoader:
    """Batch_Loader of train_pytorch_U2GNN_Sup.py:120-126: a permutation of the (train) graph
    list from the global numpy stream, first batch_size of it, then get_batch_data."""

    def __init__(self, store: GraphStore, batch_size: int, num_neighbors: int, rng=np.random,
                 with_input_y: bool = False, gather_x: bool = True, native: bool = True):
        """gather_x=False: X_concat is left to the GPU (DeviceBatch.from_store); native=False: the
        numpy form of the assembly (measurements and tests)."""
        self.store, self.bs, self.k, self.rng, self.iy = store, batch_size, num_neighbors, rng, with_input_y
        self.gather_x, self.native = gather_x, native
        self.ring, self.slot = None, 0
        if not gather_x and native and isinstance(store, GraphStore):
            # batches bound for DeviceBatch.from_store are written straight into page-locked buffers
            max_rows = int(np.sort(store.n_nodes)[::-1][:batch_size].sum())
            self.ring = [PinnedSlot(max_rows, batch_size, num_neighbors) for _ in range(3)]

    def __call__(self) -> HostBatch:
        sel = self.rng.permutation(len(self.store.graphs))[:self.bs]
        if isinstance(self.store, GraphStore):
            if not self.native:
                return self.store.assemble_numpy(sel, self.k, self.rng, self.iy)
            out = None
            if self.ring is not None:
                out = self.ring[self.slot]
                self.slot = (self.slot + 1) % len(self.ring)
            return self.store.assemble(sel, self.k, self.rng, self.iy, gather_x=self.gather_x, out=out)
        return self.store.assemble(sel, self.k, self.rng, self.iy)

    def replay(self) -> None:
        """Consume exactly the numpy draws of one batch without building it (data-parallel
        ranks skip the batches of other ranks this way)."""
        sel = self.rng.permutation(len(self.store.graphs))[:self.bs]
        deg = self.store.degrees_of(sel)
        live = deg[deg > 0]
        if len(live):
            self.rng.randint(0, live[:, None], size=(len(live), self.k))
