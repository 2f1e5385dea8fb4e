"""Which rows a row attends over, said once: the model's ``attention`` / ``hops`` / ``distances`` keywords
(check_attention, check_hops, check_distances), the batch's device-resident adjacency (Adjacency) or pair types
(PairTypes) and the value every layer call takes (AttnPattern), which alone turns a pattern into the arguments of the
C ABI (u2gnn_layer_*_csrb, u2gnn_layer_*_segb, u2gnn_csr_attn_*).

Where ``adj`` and ``pairs`` come from: the host builds them per batch from the store (Adjacency.from_store,
PairTypes.from_store), or the GPU does from a dataset's DeviceGraphs -- ``adjacency(ids)`` assembles a batch's adjacency
from the resident pieces (which ``from_store(..., hops=H, build="device")`` expands on the GPU from the one-hop lists),
``pair_types(ids, H)`` searches a batch's shortest-path distances from the one-hop structure.  Both routes give the
same integers."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from ._lib import BIAS_TYPES_MAX, DIST_NODES_MAX, U2GNNNativeError

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


CENTRALITY_MAX = 63   # degree classes 0 .. D of a centrality table: D + 1 <= U2GNN_CLASS_ROWS_MAX (u2gnn_hip.h)


def check_centrality(centrality) -> Optional[int]:
    """The ``centrality`` keyword of the models: None or 0 (off), or a D in [1, 63] -- a learned vector per node degree
    0 .. D (larger degrees take D's) added to the stack's input.  Any attention mode."""
    import numbers
    if centrality is None:
        return None
    if isinstance(centrality, bool) or not isinstance(centrality, numbers.Integral) or \
            not 0 <= int(centrality) <= CENTRALITY_MAX:
        raise ValueError(f"centrality must be None, 0 or an integer in [1, {CENTRALITY_MAX}], got {centrality!r}")
    return int(centrality) or None


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
    device)`` integer for integer; ``assemble_numpy(ids)`` is the numpy statement of the same assembly.

    A structure built without ``hops`` is also where the shortest-path search starts (csrc/distances.hip; graphs of up
    to DIST_NODES_MAX nodes): ``pair_types(ids, H)`` equals ``PairTypes.from_store(store, ids, N, device, H)``, and
    ``expand(H)`` -- what ``from_store(..., hops=H, build="device")`` returns -- equals the host-built H-hop structure;
    ``pair_types_numpy`` and ``expand_numpy`` are their numpy statements."""
    ARRAYS = ("node_start", "ent_start", "rowptr", "t_rowptr", "col", "t_src", "t_eid", "etype")

    def __init__(self, host, hops, device, dev=None, tables=None):
        """host: the numpy arrays (etype None without hops).  A structure expanded on the device (``expand``) comes
        with its device arrays ``dev`` and the host tables (n_nodes, n_entries, max_dist) instead, host None: the
        arrays are copied back on first use of ``host``."""
        self.hops, self.device = hops, torch.device(device)
        self._host = host
        if dev is None:
            self.n_nodes = np.diff(host["node_start"])
            self.n_entries = np.diff(host["ent_start"])
            self.E = int(host["ent_start"][-1])
            et = host["etype"]
            if et is None or not self.E:
                self.max_dist = np.zeros(len(self.n_nodes), dtype=np.int64)
            else:   # per graph; a graph without entries (no nodes) keeps 0
                self.max_dist = np.maximum.reduceat(et, np.minimum(host["ent_start"][:-1], self.E - 1)).astype(np.int64)
                self.max_dist[self.n_entries == 0] = 0
            self.dev = {k: None if host[k] is None else torch.from_numpy(host[k]).to(self.device) for k in self.ARRAYS}
        else:
            self.n_nodes, self.n_entries, self.max_dist = tables
            self.E = int(self.n_entries.sum())
            self.dev = dev
        self.G, self.V = len(self.n_nodes), int(self.n_nodes.sum())
        self.err = torch.zeros(1, device=self.device, dtype=torch.int32)   # set by the kernel, never on checked ids
        if self.device.type == "cuda":   # built once; batches are assembled on other streams (DeviceBatch.from_store)
            torch.cuda.current_stream(self.device).synchronize()
        self._c = None
        self._extents = None
        self.last_expand = None                                    # (chunks, scratch bytes) of ``expand``

    @property
    def host(self) -> dict:
        """The numpy arrays; of a structure expanded on the device, copied back on first use."""
        if self._host is None:
            self._host = {k: None if self.dev[k] is None else self.dev[k].cpu().numpy() for k in self.ARRAYS}
        return self._host

    @staticmethod
    def nbytes(G: int, V: int, E: int, hops) -> int:
        """The size of the dataset-wide arrays."""
        return 16 * (G + 1) + 16 * (V + 1) + (13 if hops else 12) * E

    @staticmethod
    def from_store(store, device="cuda", hops=None, max_bytes=8 << 30, build="host",
                   scratch_bytes=256 << 20) -> "DeviceGraphs":
        """The structure of all of ``store``'s graphs (any store with ``n_nodes`` and ``adjacency(ids, hops=)``), built
        once on the host from one ``store.adjacency(range(G), hops)`` and its transpose (as ``Adjacency.from_csr``
        takes it), rewritten into each graph's own numbering, then moved to ``device``.  hops None or 0: off.
        ValueError: ``hops`` outside [1, 31]; a graph with 2^31 or more nodes or entries; arrays larger than
        ``max_bytes`` (known from the counts, before anything is allocated on or copied to the device).

        build="device" with ``hops`` on a GPU: only the one-hop structure is built on the host; the shortest-path
        search and the H-hop lists are the GPU's (``expand``), in chunks of graphs whose dense scratch fits
        ``scratch_bytes``.  The arrays, ``n_entries`` and ``max_dist`` equal the host build's integer for integer.
        ValueError also for a graph above DIST_NODES_MAX nodes or one whose scratch exceeds ``scratch_bytes``.  A CPU
        device, or no ``hops``, builds on the host whatever ``build`` says."""
        from .batching import check_hops_range
        hops = check_hops_range(hops) if hops else None
        if build not in ("host", "device"):
            raise ValueError(f"device graphs: build must be 'host' or 'device', got {build!r}")
        if build == "device" and hops and torch.device(device).type == "cuda":
            DeviceGraphs._chunks(np.asarray(store.n_nodes, dtype=np.int64), DeviceGraphs.EXPAND_BYTES, scratch_bytes)
            one = DeviceGraphs.from_store(store, device, None, max_bytes)
            return one.expand(hops, scratch_bytes, max_bytes)
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

    # ---- shortest-path distances from the one-hop structure (u2gnn_pair_distances, u2gnn_hop_expand_*) ----
    EXPAND_BYTES = 3      # dense scratch per pair of the expansion: the distance (uint8) and the pair's rank (uint16)

    def _one_hop(self, what):
        if self.hops:
            raise ValueError(f"device graphs: {what} starts from a structure built without hops")

    @staticmethod
    def _chunks(n_nodes, per_pair: int, scratch_bytes: int):
        """The graph ranges [g0, g1) the dataset is searched in: consecutive graphs whose dense blocks (``per_pair``
        bytes for each of a graph's n^2 pairs) fit ``scratch_bytes`` together.  ValueError for a graph above
        DIST_NODES_MAX nodes or one that alone needs more than ``scratch_bytes``."""
        n = np.asarray(n_nodes, dtype=np.int64)
        if len(n) and int(n.max()) > DIST_NODES_MAX:
            raise ValueError(f"device graphs: a graph of {int(n.max())} nodes, the device searches at most "
                             f"{DIST_NODES_MAX} (the host path serves it)")
        need = per_pair * n * n
        if len(n) and int(need.max()) > scratch_bytes:
            raise ValueError(f"device graphs: one graph needs {int(need.max())} bytes of scratch, more than "
                             f"scratch_bytes = {scratch_bytes}")
        ends = np.cumsum(need)
        out, g0 = [], 0
        while g0 < len(n):
            g1 = int(np.searchsorted(ends, (ends[g0 - 1] if g0 else 0) + scratch_bytes, side="right"))
            out.append((g0, g1))
            g0 = g1
        return out

    def _chunk_slots(self, g0: int, g1: int, n_nodes=None):
        """(gid, row_off, pair_off) on the device, N, n_pairs, max_nodes of the chunk of graphs [g0, g1): sent from
        page-locked memory without blocking.  n_nodes: the node counts to plan with (a graph counted as 0 is left
        out of the chunk)."""
        C = g1 - g0
        n = (self.n_nodes if n_nodes is None else n_nodes)[g0:g1]
        stage = torch.empty(3 * C + 2, dtype=torch.int64, pin_memory=self.device.type == "cuda")
        h = stage.numpy()
        h[:C] = np.arange(g0, g1)
        h[C], h[2 * C + 1] = 0, 0
        np.cumsum(n, out=h[C + 1:2 * C + 1])
        np.cumsum(n * n, out=h[2 * C + 2:])
        N, n_pairs = int(h[2 * C]), int(h[3 * C + 1])
        d = stage.to(self.device, non_blocking=True)
        return (d[:C], d[C:2 * C + 1], d[2 * C + 1:]), N, n_pairs, int(n.max())

    def extents(self, scratch_bytes=256 << 20):
        """(ecc31, fin31), int64 [G] on the host: per graph the largest min(distance, 31) over all pairs, an unreachable
        pair counting as 31, and the same over the reachable pairs only.  Computed once on the device at cap 32, in
        chunks whose dense blocks fit ``scratch_bytes``, and kept: a batch's ``n_types`` is max min(ecc31, H) + 1 and
        an H-hop structure's ``max_dist`` is min(fin31, H), without reading the device again.  A graph the device does
        not search (above DIST_NODES_MAX nodes) keeps 0: ``pair_types`` refuses it."""
        from . import kernels as K
        self._one_hop("extents")
        if self._extents is None:
            small = self.n_nodes <= DIST_NODES_MAX
            n_small = np.where(small, self.n_nodes, 0)
            ecc = torch.zeros(self.G, device=self.device, dtype=torch.int32)
            fin = torch.zeros(self.G, device=self.device, dtype=torch.int32)
            plans = [(g0, g1) + self._chunk_slots(g0, g1, n_small) for g0, g1 in self._chunks(n_small, 1, scratch_bytes)]
            size = max([p[4] for p in plans] + [1])
            D = torch.empty(size, device=self.device, dtype=torch.uint8)
            for g0, g1, (gid, row_off, pair_off), N, n_pairs, max_n in plans:
                if n_pairs < 1:
                    continue
                K.pair_distances(self.c_struct(), gid, row_off, pair_off, N, n_pairs, max_n, BIAS_TYPES_MAX, D, self.err)
                K.distance_extents(D, row_off, pair_off, N, n_pairs, max_n, BIAS_TYPES_MAX, ecc[g0:g1], fin[g0:g1],
                                   self.err)
            self._extents = (ecc.cpu().numpy().astype(np.int64), fin.cpu().numpy().astype(np.int64))
            self.check_indices()
        return self._extents

    def plan_pairs(self, graph_ids, H: int):
        """(ids, row_off, pair_off, N, n_pairs, max_nodes) of the batch's pair types, from the host tables alone.
        ValueError: H outside [1, 31], an empty batch, an id outside [0, G), a graph above DIST_NODES_MAX nodes, no pair
        or more than BIAS_ENTRIES_MAX."""
        from .batching import check_hops_range
        self._one_hop("pair_types")
        check_hops_range(H)
        ids = np.ascontiguousarray(graph_ids, dtype=np.int64).reshape(-1)
        if ids.shape[0] < 1 or ids.min() < 0 or ids.max() >= self.G:
            raise ValueError(f"device graphs: a batch of at least one graph id in [0, {self.G})")
        n = self.n_nodes[ids]
        if int(n.max()) > DIST_NODES_MAX:
            raise ValueError(f"device graphs: a graph of {int(n.max())} nodes, the device searches at most "
                             f"{DIST_NODES_MAX} (the host path serves it)")
        row_off, pair_off = np.zeros(len(ids) + 1, dtype=np.int64), np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(n, out=row_off[1:])
        np.cumsum(n * n, out=pair_off[1:])
        if not 1 <= int(pair_off[-1]) <= BIAS_ENTRIES_MAX:
            raise ValueError(f"pair types: between 1 and {BIAS_ENTRIES_MAX} pairs, got {int(pair_off[-1])}")
        return ids, row_off, pair_off, int(row_off[-1]), int(pair_off[-1]), int(n.max())

    def _dense_numpy(self, g: int, cap: int) -> np.ndarray:
        """Graph g's [n, n] block min(distance, cap) as the kernel sweeps it: filled with cap, 0 on the diagonal; in
        sweep h = 1 .. cap - 1 an unset node takes h if one of its in-neighbours (t_src of its transposed list) holds
        h - 1; stop when a sweep sets nothing."""
        h_ = self.host
        n, v0 = int(self.n_nodes[g]), int(h_["node_start"][g])
        D = np.full((n, n), cap, dtype=np.uint8)
        D[np.arange(n), np.arange(n)] = 0
        tr = h_["t_rowptr"][v0:v0 + n + 1]
        into = np.zeros((n, n), dtype=np.float32)                   # into[s][u] = 1: s is an in-neighbour of u
        into[h_["t_src"][tr[0]:tr[-1]], np.repeat(np.arange(n), np.diff(tr))] = 1
        for h in range(1, cap):
            new = (D == cap) & (((D == h - 1).astype(np.float32) @ into) > 0)
            if not new.any():
                break
            D[new] = h
        return D

    def pair_types_numpy(self, graph_ids, H: int):
        """(pair_off int64 [B+1], etype int32 [n_pairs]) of the batch as host numpy arrays: what u2gnn_pair_distances
        writes, and what ``store.distances(ids, H)`` returns."""
        ids, _, pair_off, _, n_pairs, _ = self.plan_pairs(graph_ids, H)
        etype = np.empty(n_pairs, dtype=np.int32)
        for b, g in enumerate(ids):
            etype[pair_off[b]:pair_off[b + 1]] = self._dense_numpy(int(g), H).reshape(-1)
        return pair_off, etype

    def pair_types(self, graph_ids, H: int, row_off_dev=None) -> PairTypes:
        """The PairTypes of the batch ``graph_ids`` (in that order) with distances clipped at H, searched on the device
        from this one-hop structure: planned on the host (``plan_pairs``; n_types from ``extents``), ids and offsets
        leave from page-locked memory without blocking, one launch of u2gnn_pair_distances on the current stream.
        Equals ``PairTypes.from_store(store, ids, N, device, H)``.  row_off_dev: the batch's row offsets when they
        are on the device already."""
        ids, row_off, pair_off, N, n_pairs, max_n = self.plan_pairs(graph_ids, H)
        B = len(ids)
        stage = torch.empty(3 * B + 2, dtype=torch.int64, pin_memory=self.device.type == "cuda")
        h = stage.numpy()
        h[:B], h[B:2 * B + 1], h[2 * B + 1:] = ids, pair_off, row_off
        n_send = 2 * B + 1 if row_off_dev is not None else 3 * B + 2
        d = stage[:n_send].to(self.device, non_blocking=True)
        return self.launch_pairs(d[:B], d[2 * B + 1:] if row_off_dev is None else row_off_dev, d[B:2 * B + 1], N,
                                 n_pairs, max_n, H, self.n_pair_types(ids, H))

    def n_pair_types(self, ids, H: int) -> int:
        """max(etype) + 1 of the batch's pair types, from ``extents`` alone."""
        return int(np.minimum(self.extents()[0][ids], H).max()) + 1

    def launch_pairs(self, gid, row_off, pair_off, N: int, n_pairs: int, max_nodes: int, H: int, n_types: int) -> PairTypes:
        """The batch's PairTypes from device int64 ``gid`` [B], ``row_off`` / ``pair_off`` [B+1] (``plan_pairs``'s
        arrays): allocates etype and launches u2gnn_pair_distances on the current stream."""
        from . import kernels as K
        etype = torch.empty(n_pairs, device=gid.device, dtype=torch.int32)
        K.pair_distances(self.c_struct(), gid, row_off, pair_off, N, n_pairs, max_nodes, H, etype, self.err)
        return PairTypes(N, pair_off, etype, n_types)

    def expand_numpy(self, H: int) -> dict:
        """The eight host arrays of the H-hop structure, from the dense blocks of ``_dense_numpy`` (cap H + 1) as the
        expansion kernels build them: a row keeps the columns with D <= H in ascending order, a column the rows; a
        transposed entry's id is its row's first entry inside the graph plus the rank of the column in that row."""
        from .batching import check_hops_range
        self._one_hop("expand")
        H = check_hops_range(H)
        cnt, tcnt, col, et, t_src, t_eid = [], [], [], [], [], []
        for g in range(self.G):
            D = self._dense_numpy(g, H + 1)
            keep = D <= H
            c = keep.sum(1)
            first = np.cumsum(c) - c                                # each row's first entry inside the graph
            rank = np.cumsum(keep, 1) - 1
            ti, tj = np.nonzero(keep.T)[::-1]                       # grouped by column j, rows i ascending
            cnt.append(c), tcnt.append(keep.sum(0)), col.append(np.nonzero(keep)[1]), et.append(D[keep])
            t_src.append(ti), t_eid.append(first[ti] + rank[ti, tj])
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dtype=dt)   # noqa: E731
        rowptr, t_rowptr = np.zeros(self.V + 1, dtype=np.int64), np.zeros(self.V + 1, dtype=np.int64)
        np.cumsum(cat(cnt, np.int64), out=rowptr[1:])
        np.cumsum(cat(tcnt, np.int64), out=t_rowptr[1:])
        node_start = self.host["node_start"]
        return {"node_start": node_start, "ent_start": np.ascontiguousarray(rowptr[node_start]), "rowptr": rowptr,
                "t_rowptr": t_rowptr, "col": cat(col, np.int32), "t_src": cat(t_src, np.int32),
                "t_eid": cat(t_eid, np.int32), "etype": cat(et, np.uint8)}

    def expand(self, H: int, scratch_bytes=256 << 20, max_bytes=8 << 30) -> "DeviceGraphs":
        """The H-hop structure of the same graphs, expanded on the device from this one-hop structure: per chunk of
        graphs (``_chunks``) the dense distances at cap H + 1 (u2gnn_pair_distances_u8), the row and column counts and
        each graph's largest distance; one prefix sum over the dataset's nodes (torch.cumsum) gives rowptr and
        t_rowptr, the total is read back once and checked against ``max_bytes`` before the entry arrays are
        allocated; then per chunk the fill (the distances are searched again unless one chunk holds everything).
        Equals the host build integer for integer; ``last_expand`` keeps (chunks, scratch bytes)."""
        from . import kernels as K
        from .batching import check_hops_range
        self._one_hop("expand")
        H = check_hops_range(H)
        if self.device.type != "cuda":
            raise ValueError("device graphs: expand runs on a GPU")
        plans = [(g0, g1) + self._chunk_slots(g0, g1)
                 for g0, g1 in self._chunks(self.n_nodes, self.EXPAND_BYTES, scratch_bytes)]
        plans = [p for p in plans if p[4] >= 1]
        ns = self.host["node_start"]
        size = max(p[4] for p in plans)
        l_at = size + (-size) % 16                                  # the ranks follow the distances, 16-byte aligned
        scratch = torch.empty(l_at + 2 * size, device=self.device, dtype=torch.uint8)
        D, L = scratch[:size], scratch[l_at:].view(torch.int16)
        dev, i64 = self.device, torch.int64
        rowptr, t_rowptr = torch.zeros(self.V + 1, device=dev, dtype=i64), torch.zeros(self.V + 1, device=dev, dtype=i64)
        cnt, t_cnt = torch.empty(self.V, device=dev, dtype=i64), torch.empty(self.V, device=dev, dtype=i64)
        ecc, fin = (torch.zeros(self.G, device=dev, dtype=torch.int32) for _ in range(2))
        search = lambda p: K.pair_distances(self.c_struct(), *p[2], p[3], p[4], p[5], H + 1, D, self.err)  # noqa: E731
        for p in plans:
            g0, g1, (_, row_off, pair_off), N, n_pairs, max_n = p
            v0 = int(ns[g0])
            search(p)
            K.hop_expand_count(D, row_off, pair_off, N, n_pairs, max_n, H, cnt[v0:v0 + N], t_cnt[v0:v0 + N], self.err)
            K.distance_extents(D, row_off, pair_off, N, n_pairs, max_n, H + 1, ecc[g0:g1], fin[g0:g1], self.err)
        torch.cumsum(cnt, 0, out=rowptr[1:])
        torch.cumsum(t_cnt, 0, out=t_rowptr[1:])
        del cnt, t_cnt
        ent_start = rowptr[self.dev["node_start"]].contiguous()
        n_entries = np.diff(ent_start.cpu().numpy())                # the one read-back of the counts
        E = int(n_entries.sum())
        self._check_size(self.G, self.V, E, H, max_bytes)
        col, t_src, t_eid = (torch.empty(E, device=dev, dtype=torch.int32) for _ in range(3))
        etype = torch.empty(E, device=dev, dtype=torch.uint8)
        for p in plans:
            g0, g1, (_, row_off, pair_off), N, n_pairs, max_n = p
            v0 = int(ns[g0])
            if len(plans) > 1:
                search(p)
            K.hop_expand_fill(D, L, row_off, pair_off, N, n_pairs, max_n, H, rowptr[v0:v0 + N], t_rowptr[v0:v0 + N],
                              col, etype, t_src, t_eid, self.err)
        max_dist = fin.cpu().numpy().astype(np.int64)
        self.check_indices()
        out = DeviceGraphs(None, H, dev, dev={"node_start": self.dev["node_start"], "ent_start": ent_start,
                                              "rowptr": rowptr, "t_rowptr": t_rowptr, "col": col, "t_src": t_src,
                                              "t_eid": t_eid, "etype": etype},
                           tables=(self.n_nodes, n_entries, max_dist))
        out.last_expand = (len(plans), int(scratch.numel()))
        return out


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
