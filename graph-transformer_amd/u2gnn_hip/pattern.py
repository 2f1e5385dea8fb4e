"""Which rows a row attends over, said once: the model's ``attention`` / ``hops`` / ``distances`` keywords
(check_attention, check_hops, check_distances), the batch's device-resident adjacency (Adjacency) or pair types
(PairTypes) and the value every layer call takes (AttnPattern), which alone turns a pattern into the arguments of the
C ABI (u2gnn_layer_*_csrb, u2gnn_layer_*_segb, u2gnn_csr_attn_*)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from ._lib import BIAS_TYPES_MAX, U2GNNNativeError

ATTENTION_MODES = ("nodes", "neighbors", "graphs", "edges")
BIAS_ENTRIES_MAX = 4096 * 112 * 256   # the entries u2gnn_bias_table_grad reduces in one call (u2gnn_hip.h)


def check_attention(name: str) -> str:
    """The ``attention`` keyword of the models and of EncoderStack."""
    if name not in ATTENTION_MODES:
        raise ValueError(f"attention must be 'nodes', 'neighbors', 'graphs' or 'edges', got {name!r}")
    return name


def check_hops(hops, attention: str) -> Optional[int]:
    """The ``hops`` keyword of the models: None (off) or an H in [1, 31], and only with attention="edges"."""
    if hops is None:
        return None
    if attention != "edges":
        raise ValueError(f"hops needs attention='edges', got attention={attention!r}")
    if int(hops) != hops or not 1 <= int(hops) <= BIAS_TYPES_MAX - 1:
        raise ValueError(f"hops must be an integer in [1, {BIAS_TYPES_MAX - 1}], got {hops!r}")
    return int(hops)


def check_distances(distances, attention: str, hops=None) -> Optional[int]:
    """The ``distances`` keyword of the models: None (off) or an H in [1, 31], only with attention="graphs" and never
    together with ``hops``."""
    if distances is None:
        return None
    if attention != "graphs":
        raise ValueError(f"distances needs attention='graphs', got attention={attention!r}")
    if hops is not None:
        raise ValueError("distances and hops exclude each other (hops is attention='edges', distances 'graphs')")
    if int(distances) != distances or not 1 <= int(distances) <= BIAS_TYPES_MAX - 1:
        raise ValueError(f"distances must be an integer in [1, {BIAS_TYPES_MAX - 1}], got {distances!r}")
    return int(distances)


class PairTypes:
    """The pair types of attention="graphs" with ``distances`` on the device: graph b of the batch owns the entries
    pair_off[b] .. pair_off[b+1]-1 of etype, its [n_b, n_b] block row-major (GraphStore.distances): etype[pair_off[b] +
    (i - lo) n_b + (j - lo)] is the clipped shortest-path distance of rows i and j, the index into the model's hop_bias
    tables.  pair_off int64 [B+1], etype int32 [n_pairs], n_types = max(etype) + 1; N: the batch's rows."""
    __slots__ = ("N", "n_pairs", "pair_off", "etype", "n_types")

    def __init__(self, N, pair_off, etype, n_types):
        self.N, self.n_pairs, self.n_types = int(N), int(etype.numel()), int(n_types)
        self.pair_off, self.etype = pair_off, etype

    @staticmethod
    def _check(pair_off, etype, N):
        po = np.ascontiguousarray(np.asarray(pair_off), dtype=np.int64).reshape(-1)
        et = np.asarray(etype).reshape(-1)
        if int(N) < 1 or po.shape[0] < 2:
            raise ValueError("pair types: at least one row and one graph")
        if po[0] != 0 or po[-1] != et.shape[0] or (np.diff(po) < 0).any():
            raise ValueError("pair types: pair_off must start at 0, never decrease and end at len(etype)")
        if not 1 <= et.shape[0] <= BIAS_ENTRIES_MAX:
            raise ValueError(f"pair types: between 1 and {BIAS_ENTRIES_MAX} pairs, got {et.shape[0]}")
        lo, hi = int(et.min()), int(et.max())
        if lo < 0 or hi >= BIAS_TYPES_MAX:
            raise ValueError(f"pair types: a type outside [0, {BIAS_TYPES_MAX})")
        return po, et, hi + 1

    @staticmethod
    def _send(po, et, N, n_types, device, staged=None) -> "PairTypes":
        """Both arrays leave from page-locked memory without blocking (staged: etype is already a view of ``staged``,
        a page-locked int32 tensor)."""
        dev = torch.device(device)
        pin = dev.type == "cuda"
        if staged is None:
            staged = torch.empty(et.shape[0], dtype=torch.int32, pin_memory=pin)   # the caching host allocator keeps a
            staged.numpy()[:] = et                                                 # block until its copy is done
        hp = torch.empty(po.shape[0], dtype=torch.int64, pin_memory=pin)
        hp.numpy()[:] = po
        return PairTypes(N, hp.to(dev, non_blocking=True), staged[:et.shape[0]].to(dev, non_blocking=True), n_types)

    @staticmethod
    def from_arrays(pair_off, etype, N: int, device="cuda") -> "PairTypes":
        """Validates on the host (ValueError: pair_off not starting at 0, decreasing or not ending at len(etype); a type
        outside [0, 32); no pair, or more than u2gnn_bias_table_grad reduces) and moves both arrays to ``device``
        (etype as int32)."""
        po, et, n_types = PairTypes._check(pair_off, etype, N)
        return PairTypes._send(po, et, N, n_types, device)

    @staticmethod
    def from_store(store, graph_ids, N: int, device="cuda", H: int = 1) -> "PairTypes":
        """The pair types of a batch of ``store``'s graphs (``store.distances(graph_ids, H)``: cached per-graph blocks,
        concatenated straight into a page-locked buffer), validated as ``from_arrays``."""
        ids = np.asarray(graph_ids, dtype=np.int64).reshape(-1)
        n = np.asarray(store.n_nodes, dtype=np.int64)[ids]
        total = int((n * n).sum())
        if int(n.sum()) != int(N):
            raise ValueError(f"pair types: the store gives the batch {int(n.sum())} rows, the batch has {int(N)}")
        if not 1 <= total <= BIAS_ENTRIES_MAX:
            raise ValueError(f"pair types: between 1 and {BIAS_ENTRIES_MAX} pairs, got {total}")
        staged = torch.empty(total, dtype=torch.int32, pin_memory=torch.device(device).type == "cuda")
        po, et = store.distances(ids, H, out=staged.numpy())
        po, et, n_types = PairTypes._check(po, et, N)
        return PairTypes._send(po, et, N, n_types, device, staged)


class Adjacency:
    """The attention pattern of attention="edges" on the device: row i attends over colidx[rowptr[i] .. rowptr[i+1])
    (GraphStore.adjacency: the node itself and its graph neighbours), with the transpose the backward walks: for
    column j the entries e = t_eid[t] (indices into colidx) and their rows t_src[t], t in t_rowptr[j] ..
    t_rowptr[j+1].  Five int64 tensors and nnz; the kernels never hand them back to the host.  With ``hops``
    (GraphStore.adjacency(ids, hops=H)) also etype, int32 [nnz]: the shortest-path distance of each entry, the index
    into the model's hop_bias tables, and n_types = max(etype) + 1."""
    __slots__ = ("N", "nnz", "rowptr", "colidx", "t_rowptr", "t_src", "t_eid", "etype", "n_types", "_c")

    def __init__(self, N, rowptr, colidx, t_rowptr, t_src, t_eid, etype=None, n_types=0):
        self.N, self.nnz = int(N), int(colidx.numel())
        self.rowptr, self.colidx, self.t_rowptr, self.t_src, self.t_eid = rowptr, colidx, t_rowptr, t_src, t_eid
        self.etype, self.n_types = etype, int(n_types)
        self._c = None

    @staticmethod
    def from_csr(rowptr, colidx, N: int, device="cuda", etype=None) -> "Adjacency":
        """Validates the CSR on the host (ValueError: rowptr not [N+1], not starting at 0, decreasing or not ending
        at len(colidx); a column outside [0, N); etype not one value per entry or outside [0, 32)), builds the
        transpose by a stable argsort of the columns (the entries of a column keep their row order) and moves the
        five arrays (and etype, as int32) to ``device``."""
        rp = np.ascontiguousarray(np.asarray(rowptr), dtype=np.int64).reshape(-1)
        ci = np.ascontiguousarray(np.asarray(colidx), dtype=np.int64).reshape(-1)
        N = int(N)
        if N < 1 or rp.shape[0] != N + 1:
            raise ValueError(f"adjacency: rowptr must hold N + 1 = {N + 1} entries, got {rp.shape[0]}")
        if rp[0] != 0 or rp[-1] != ci.shape[0] or (np.diff(rp) < 0).any():
            raise ValueError("adjacency: rowptr must start at 0, never decrease and end at len(colidx)")
        if ci.shape[0] and (ci.min() < 0 or ci.max() >= N):
            raise ValueError(f"adjacency: a column index outside [0, {N})")
        et, n_types = None, 0
        if etype is not None:
            et = np.ascontiguousarray(np.asarray(etype), dtype=np.int64).reshape(-1)
            if et.shape[0] != ci.shape[0]:
                raise ValueError(f"adjacency: etype must hold one value per entry ({ci.shape[0]}), got {et.shape[0]}")
            if et.shape[0] and (et.min() < 0 or et.max() >= BIAS_TYPES_MAX):
                raise ValueError(f"adjacency: an entry type outside [0, {BIAS_TYPES_MAX})")
            n_types = int(et.max()) + 1 if et.shape[0] else 0
        order = np.argsort(ci, kind="stable")                       # entry ids grouped by column, rows ascending
        t_rowptr = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(np.bincount(ci, minlength=N), out=t_rowptr[1:])
        rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
        dev = torch.device(device)
        h2d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)  # noqa: E731
        et_dev = None if et is None else torch.from_numpy(et.astype(np.int32)).to(dev)
        return Adjacency(N, h2d(rp), h2d(ci), h2d(t_rowptr), h2d(rows[order]), h2d(order), et_dev, n_types)

    @staticmethod
    def from_store(store, graph_ids, N: int, device="cuda", hops=None) -> "Adjacency":
        """The adjacency of a batch of ``store``'s graphs (plus the diagonal), built on the host from the store; with
        ``hops`` = H the H-hop lists and each entry's distance (hop_bias's index).  hops None or 0: off."""
        csr = store.adjacency(graph_ids, hops=hops or None)   # (rowptr, colidx), with hops also etype
        return Adjacency.from_csr(csr[0], csr[1], N, device, *csr[2:])

    def c_struct(self):
        """The u2gnn_csr_attn of these arrays (kept alive with them)."""
        if self._c is None:
            from ._lib import CsrAttn
            self._c = CsrAttn(*[t.data_ptr() or None for t in (self.rowptr, self.colidx, self.t_rowptr, self.t_src,
                                                               self.t_eid)], self.nnz)
        return self._c


class DeviceGraphs:
    """A dataset's adjacency, kept on the device as per-graph pieces, so that a batch's Adjacency is assembled there
    (u2gnn_adjacency_assemble) instead of being built on the host and copied for every batch.

    A batch's adjacency is block-diagonal: graph g's columns lie in its own row range and its entries are contiguous
    in entry order, so the stable sort by column that gives the transpose groups by graph first and keeps the entry
    order inside each graph.  Everything ``Adjacency.from_csr`` computes for a batch is therefore the concatenation
    of its graphs' pieces plus two offsets per graph (the graph's first row and first entry in the batch).  The
    pieces, computed once for all G graphs (V nodes, E entries):

    * ``node_start``, ``ent_start`` int64 [G+1]: graph g's nodes and entries in the dataset's numbering;
    * ``rowptr``, ``t_rowptr`` int64 [V+1]: the first entry of each node's list / transposed list;
    * ``col``, ``t_src``, ``t_eid`` int32 [E]: column, source row and entry id inside the graph;
    * ``etype`` uint8 [E], only with ``hops``: the entry's distance.

    The host keeps each graph's node count, entry count and largest distance: a batch's N, nnz and n_types come from
    them, never from the device.  ``adjacency(ids)`` equals ``Adjacency.from_csr(*store.adjacency(ids, hops), N,
    device)`` integer for integer; ``assemble_numpy(ids)`` is the numpy statement of the same assembly."""
    ARRAYS = ("node_start", "ent_start", "rowptr", "t_rowptr", "col", "t_src", "t_eid", "etype")

    def __init__(self, host: dict, hops, device):
        self.hops, self.device = hops, torch.device(device)
        self.host = host                                           # the numpy arrays (etype None without hops)
        self.G, self.V, self.E = len(host["node_start"]) - 1, int(host["node_start"][-1]), int(host["ent_start"][-1])
        self.n_nodes = np.diff(host["node_start"])
        self.n_entries = np.diff(host["ent_start"])
        et = host["etype"]
        if et is None or not self.E:
            self.max_dist = np.zeros(self.G, dtype=np.int64)
        else:   # per graph; a graph without entries (no nodes) keeps 0
            self.max_dist = np.maximum.reduceat(et, np.minimum(host["ent_start"][:-1], self.E - 1)).astype(np.int64)
            self.max_dist[self.n_entries == 0] = 0
        self.dev = {k: None if host[k] is None else torch.from_numpy(host[k]).to(self.device) for k in self.ARRAYS}
        self.err = torch.zeros(1, device=self.device, dtype=torch.int32)   # set by the kernel, never on checked ids
        if self.device.type == "cuda":   # built once; batches are assembled on other streams (DeviceBatch.from_store)
            torch.cuda.current_stream(self.device).synchronize()
        self._c = None

    @staticmethod
    def nbytes(G: int, V: int, E: int, hops) -> int:
        """The size of the dataset-wide arrays."""
        return 16 * (G + 1) + 16 * (V + 1) + (13 if hops else 12) * E

    @staticmethod
    def from_store(store, device="cuda", hops=None, max_bytes=8 << 30) -> "DeviceGraphs":
        """The structure of all of ``store``'s graphs (any store with ``n_nodes`` and ``adjacency(ids, hops=)``), built
        once on the host from one ``store.adjacency(range(G), hops)`` and its transpose (as ``Adjacency.from_csr``
        takes it), rewritten into each graph's own numbering, then moved to ``device``.  hops None or 0: off.
        ValueError: ``hops`` outside [1, 31]; a graph with 2^31 or more nodes or entries; arrays larger than
        ``max_bytes`` (known from the counts, before anything is allocated on or copied to the device)."""
        from .batching import check_hops_range
        hops = check_hops_range(hops) if hops else None
        n = np.asarray(store.n_nodes, dtype=np.int64)
        G, V = len(n), int(n.sum())
        if G < 1 or V < 1:
            raise ValueError("device graphs: the store holds no nodes")
        limit = lambda E: DeviceGraphs._check_size(G, V, E, hops, max_bytes)  # noqa: E731
        limit(V)                                                   # every node lists itself: E >= V
        if n.max() >= 1 << 31:
            raise ValueError("device graphs: a graph with 2^31 or more nodes")
        csr = store.adjacency(np.arange(G, dtype=np.int64), hops=hops)
        rp = np.ascontiguousarray(csr[0], dtype=np.int64)
        ci = np.ascontiguousarray(csr[1], dtype=np.int64)
        E = int(ci.shape[0])
        limit(E)
        node_start = np.zeros(G + 1, dtype=np.int64)
        np.cumsum(n, out=node_start[1:])
        ent_start = np.ascontiguousarray(rp[node_start])
        if (np.diff(ent_start) >= 1 << 31).any():
            raise ValueError("device graphs: a graph with 2^31 or more entries")
        # the whole dataset's transpose, exactly as Adjacency.from_csr takes a batch's
        order = np.argsort(ci, kind="stable")
        t_rowptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(ci, minlength=V), out=t_rowptr[1:])
        rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
        # into each graph's numbering: entry p and transposed entry p both belong to the graph that owns position p
        # (checked: a column inside its graph's nodes, a transposed entry's id inside its graph's entries)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        seg = np.diff(ent_start)
        first = np.repeat(node_start[:-1], seg)
        col, t_src = ci - first, i32(rows[order] - first)
        ok = not E or (col.min() >= 0 and bool((col < np.repeat(n, seg)).all()))
        del first, rows
        col = i32(col)
        t_eid = order - np.repeat(ent_start[:-1], seg)
        if not ok or (E and (t_eid.min() < 0 or bool((t_eid >= np.repeat(seg, seg)).any()))):
            raise ValueError("device graphs: the store's adjacency is not block-diagonal by graph")
        host = {"node_start": node_start, "ent_start": ent_start, "rowptr": rp, "t_rowptr": t_rowptr, "col": col,
                "t_src": t_src, "t_eid": i32(t_eid),
                "etype": np.ascontiguousarray(csr[2], dtype=np.uint8) if hops else None}
        return DeviceGraphs(host, hops, device)

    @staticmethod
    def _check_size(G, V, E, hops, max_bytes):
        need = DeviceGraphs.nbytes(G, V, E, hops)
        if need > max_bytes:
            raise ValueError(f"device graphs: the arrays need at least {need} bytes, more than max_bytes = {max_bytes}")

    def c_struct(self):
        """The u2gnn_graph_structure of the device arrays (kept alive with them)."""
        if self._c is None:
            from ._lib import GraphStructure
            self._c = GraphStructure(*[None if self.dev[k] is None else self.dev[k].data_ptr() for k in self.ARRAYS],
                                     self.G, self.V, self.E)
        return self._c

    def plan(self, graph_ids):
        """(ids, row_off, ent_off, N, nnz, n_types) of the batch ``graph_ids``, from the host tables alone: int64
        arrays [B], [B+1], [B+1].  ValueError for an empty batch or an id outside [0, G)."""
        ids = np.ascontiguousarray(graph_ids, dtype=np.int64).reshape(-1)
        if ids.shape[0] < 1 or ids.min() < 0 or ids.max() >= self.G:
            raise ValueError(f"device graphs: a batch of at least one graph id in [0, {self.G})")
        row_off, ent_off = np.zeros(len(ids) + 1, dtype=np.int64), np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(self.n_nodes[ids], out=row_off[1:])
        np.cumsum(self.n_entries[ids], out=ent_off[1:])
        n_types = int(self.max_dist[ids].max()) + 1 if self.hops and ent_off[-1] else 0
        return ids, row_off, ent_off, int(row_off[-1]), int(ent_off[-1]), n_types

    def assemble_numpy(self, graph_ids):
        """(rowptr, colidx, t_rowptr, t_src, t_eid, etype) of the batch as host numpy arrays (int64; etype int32, None
        without hops): what the kernel writes, and what ``Adjacency.from_csr`` builds from the batch's CSR."""
        h = self.host
        ids, row_off, ent_off, N, nnz, _ = self.plan(graph_ids)
        slot_r = np.repeat(np.arange(len(ids)), self.n_nodes[ids])            # the slot of each batch row / entry
        slot_e = np.repeat(np.arange(len(ids)), self.n_entries[ids])
        v = h["node_start"][ids][slot_r] + np.arange(N, dtype=np.int64) - row_off[slot_r]
        s = h["ent_start"][ids][slot_e] + np.arange(nnz, dtype=np.int64) - ent_off[slot_e]
        shift = (ent_off[:-1] - h["ent_start"][ids])[slot_r]
        rowptr, t_rowptr = np.full(N + 1, nnz, dtype=np.int64), np.full(N + 1, nnz, dtype=np.int64)
        rowptr[:N], t_rowptr[:N] = h["rowptr"][v] + shift, h["t_rowptr"][v] + shift
        ro, eo = row_off[slot_e], ent_off[slot_e]
        etype = None if h["etype"] is None else h["etype"][s].astype(np.int32)
        return rowptr, h["col"][s] + ro, t_rowptr, h["t_src"][s] + ro, h["t_eid"][s] + eo, etype

    def launch(self, gid, row_off, ent_off, N: int, nnz: int, n_types: int) -> Adjacency:
        """The batch's Adjacency from device int64 ``gid`` [B], ``row_off`` / ``ent_off`` [B+1] (``plan``'s arrays):
        allocates the outputs and launches u2gnn_adjacency_assemble on the current stream."""
        from . import kernels as K
        if nnz < 1:
            raise ValueError("device graphs: a batch without entries")
        np1 = N + 2 - N % 2                                        # N + 1 row pointers, the next array 16-byte aligned
        buf = torch.empty(2 * np1 + 3 * nnz, device=gid.device, dtype=torch.int64)
        rowptr, t_rowptr = buf[:N + 1], buf[np1:np1 + N + 1]
        colidx, t_src, t_eid = (buf[2 * np1 + i * nnz:2 * np1 + (i + 1) * nnz] for i in range(3))
        etype = torch.empty(nnz, device=gid.device, dtype=torch.int32) if self.hops else None
        K.adjacency_assemble(self.c_struct(), gid, row_off, ent_off, N, nnz, rowptr, colidx, t_rowptr, t_src, t_eid,
                             etype, self.err)
        return Adjacency(N, rowptr, colidx, t_rowptr, t_src, t_eid, etype, n_types)

    def adjacency(self, graph_ids, row_off_dev=None) -> Adjacency:
        """The Adjacency of the batch ``graph_ids`` (in that order), assembled on the device: the ids are checked on
        the host (ValueError outside [0, G)), ids and offsets leave from page-locked memory without blocking, the
        kernel runs on the current stream.  row_off_dev: the batch's row offsets when they are on the device already
        (DeviceBatch.rowptr of a batch built from offsets)."""
        ids, row_off, ent_off, N, nnz, n_types = self.plan(graph_ids)
        B = len(ids)
        pin = self.device.type == "cuda"
        stage = torch.empty(3 * B + 2, dtype=torch.int64, pin_memory=pin)   # the caching host allocator keeps a block
        h = stage.numpy()                                                  # until the copy that reads it is done
        h[:B], h[B:2 * B + 1], h[2 * B + 1:] = ids, ent_off, row_off
        n_send = 2 * B + 1 if row_off_dev is not None else 3 * B + 2
        d = stage[:n_send].to(self.device, non_blocking=True)
        return self.launch(d[:B], d[2 * B + 1:] if row_off_dev is None else row_off_dev, d[B:2 * B + 1], N, nnz, n_types)

    def check_indices(self):
        """IndexError if a launch met a slot or an index out of range (host sync)."""
        if int(self.err.item()):
            raise IndexError("device graphs: a graph id or an index out of range reached the kernel")


class AttnPattern:
    """The rows one encoder layer's rows attend over; an immutable value of exactly one kind:

    * ``NODES``: every row over all rows of the layer;
    * ``window(W)``: within each node's window of W token rows (the layer has nodes * W rows);
    * ``segments(offsets, pairs=None)``: over the rows of its own segment (per-graph attention); offsets: int64 device
      [n_seg + 1] row offsets; pairs: the segments' PairTypes, for layers that add a per-pair bias to their scores;
    * ``csr(adjacency)``: over the columns of its row of an Adjacency (neighbour attention).

    One payload per kind, so no two can be combined.  ``W`` and ``nnz`` are 0 for the kinds without them; ``key`` is
    what the layer's buffer sizes depend on (hashable: native.sizes caches by it) -- never on ``pairs``: nothing of a
    bias lives in the layer's buffers, and the pair count travels on its own (``pair_args``)."""
    __slots__ = ("kind", "what", "W", "nnz", "key", "pairs", "_c")

    def __init__(self, kind: str, what=None, pairs=None):
        W, nnz = what if kind == "window" else 0, getattr(what, "nnz", 0) if kind == "csr" else 0
        if pairs is not None and kind != "segments":
            raise ValueError("pair types go with a segments pattern")
        for name, v in (("kind", kind), ("what", what), ("W", W), ("nnz", nnz), ("key", (W, kind == "segments", nnz)),
                        ("pairs", pairs), ("_c", None)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("AttnPattern is immutable")

    @staticmethod
    def window(W: int) -> "AttnPattern":
        return AttnPattern("window", int(W))

    @staticmethod
    def segments(offsets: torch.Tensor, pairs: Optional[PairTypes] = None) -> "AttnPattern":
        return AttnPattern("segments", offsets, pairs)

    @staticmethod
    def csr(adjacency: Adjacency) -> "AttnPattern":
        return AttnPattern("csr", adjacency)

    def c_args(self, device):
        """(segment offsets pointer, segment count, u2gnn_csr_attn reference) as u2gnn_layer_fwd_csrb / _bwd_csrb and
        u2gnn_csr_attn_* take them -- (None, 0, None) for NODES and a window, which travels in u2gnn_layer_dims.
        U2GNNNativeError unless the arrays live on ``device`` in the kernels' type and layout (checked once, kept)."""
        c = self._c
        if c is None or c[0] != device:
            c = (device, self._c_args(device))
            object.__setattr__(self, "_c", c)
        return c[1]

    def pair_args(self, device):
        """(pair offsets pointer, pair count) as u2gnn_layer_fwd_segb / _bwd_segb take them.  U2GNNNativeError unless
        this is a segments pattern with PairTypes on ``device``, one offset per segment bound."""
        pt = self.pairs
        self.c_args(device)
        if (self.kind != "segments" or not isinstance(pt, PairTypes) or pt.n_pairs < 1 or not pt.pair_off.is_cuda
                or pt.pair_off.device != device or pt.pair_off.dtype != torch.int64 or not pt.pair_off.is_contiguous()
                or pt.pair_off.numel() != self.what.numel()):
            raise U2GNNNativeError("pairs: a segments pattern with PairTypes on the layer's device, pair_off int64 "
                                   "[n_seg + 1]")
        return ctypes.c_void_p(pt.pair_off.data_ptr()), pt.n_pairs

    def _c_args(self, device):
        t = self.what
        if self.kind == "segments":
            if (not t.is_cuda or t.device != device or t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 2
                    or not t.is_contiguous()):
                raise U2GNNNativeError("segments: a contiguous int64 tensor [n_seg + 1] on the layer's device")
            return ctypes.c_void_p(t.data_ptr()), t.numel() - 1, None
        if self.kind == "csr":
            if not isinstance(t, Adjacency) or t.nnz < 1 or not t.rowptr.is_cuda or t.rowptr.device != device:
                raise U2GNNNativeError("adjacency: an Adjacency with at least one entry on the layer's device")
            return None, 0, ctypes.byref(t.c_struct())
        return None, 0, None


NODES = AttnPattern("nodes")
