"""Which rows a row attends over, said once: the model's ``attention`` / ``hops`` keywords (check_attention,
check_hops), the batch's device-resident adjacency (Adjacency) and the value every layer call takes (AttnPattern),
which alone turns a pattern into the arguments of the C ABI (u2gnn_layer_*_csrb, u2gnn_csr_attn_*)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from ._lib import BIAS_TYPES_MAX, U2GNNNativeError

ATTENTION_MODES = ("nodes", "neighbors", "graphs", "edges")


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


class AttnPattern:
    """The rows one encoder layer's rows attend over; an immutable value of exactly one kind:

    * ``NODES``: every row over all rows of the layer;
    * ``window(W)``: within each node's window of W token rows (the layer has nodes * W rows);
    * ``segments(offsets)``: over the rows of its own segment (per-graph attention); offsets: int64 device
      [n_seg + 1] row offsets;
    * ``csr(adjacency)``: over the columns of its row of an Adjacency (neighbour attention).

    One payload per kind, so no two can be combined.  ``W`` and ``nnz`` are 0 for the kinds without them; ``key`` is
    what the layer's buffer sizes depend on (hashable: native.sizes caches by it)."""
    __slots__ = ("kind", "what", "W", "nnz", "key", "_c")

    def __init__(self, kind: str, what=None):
        W, nnz = what if kind == "window" else 0, getattr(what, "nnz", 0) if kind == "csr" else 0
        for name, v in (("kind", kind), ("what", what), ("W", W), ("nnz", nnz), ("key", (W, kind == "segments", nnz)),
                        ("_c", None)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("AttnPattern is immutable")

    @staticmethod
    def window(W: int) -> "AttnPattern":
        return AttnPattern("window", int(W))

    @staticmethod
    def segments(offsets: torch.Tensor) -> "AttnPattern":
        return AttnPattern("segments", offsets)

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
