"""Model-level orchestration of the U2GNN hot path on the gfx950 kernels.

* ``DeviceBatch``   — one mini-batch resident in HBM (input_x, X_concat, pooling CSR, labels).
* ``EncoderStack``  — the L x T encoder layers under one attention pattern per batch (pattern.AttnPattern, chosen by
                      ``_pattern`` from the model's ``attention``): one forward and one backward loop for every mode.
* ``SupCore``       — forward / backward of pytorch_U2GNN_Sup.TransformerU2GNN (:30-46):
                      gather -> L x (T encoder layers -> sum-pool -> dropout -> Linear, summed).
* ``FlatParams``    — all parameters (and grads, Adam moments) in single flat fp32 buffers,
                      so clip_grad_norm_ + Adam are two sweeps (train_pytorch_U2GNN_Sup.py:160-161).
* ``FusedAdam``     — torch.optim.Adam semantics with the clip coefficient applied on device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import kernels as K
from . import native
from .engine import deep_wgrad as engine_deep_wgrad
from .engine import (SITE_ATTN, SITE_DROP1, SITE_DROP2, SITE_DROPFF, SITE_HEAD, Dims, LayerParams, PackedLayer,
                     OffPath, encoder_layer_backward, encoder_layer_forward, rup, side_stream_pays, site_seed)
# (Adjacency, check_hops, ATTENTION_MODES: re-exported, the models, tools and tests import them from here)
from .pattern import (ATTENTION_MODES, NODES, Adjacency, AttnPattern, DeviceGraphs, PairTypes,  # noqa: F401
                      check_attention, check_centrality, check_distances, check_hops)


_IOTA = {}


_COPY: dict = {}


def _copy_stream(dev: torch.device) -> "torch.cuda.Stream":
    s = _COPY.get(dev.index)
    if s is None:
        s = _COPY[dev.index] = torch.cuda.Stream(device=dev)
    return s


def _pool_iota(N: int, dev: torch.device):
    """graph_pool's column indices (0..N-1) and values (ones) as views of cached device buffers."""
    key = (dev.type, dev.index)
    c = _IOTA.get(key)
    if c is None or c[0].numel() < N:
        n = max(N, 1 << 14, 2 * (c[0].numel() if c is not None else 0))
        c = _IOTA[key] = (torch.arange(n, device=dev, dtype=torch.int64), torch.ones(n, device=dev, dtype=torch.float32))
    return c[0][:N], c[1][:N]


@dataclass
class DeviceBatch:
    N: int
    B: int
    input_x: torch.Tensor           # int64 [N, k+1] (only column 0 is read: the slot-0 gather)
    X_concat: torch.Tensor          # f32 [N, d]
    rowptr: torch.Tensor            # int64 [B+1]   pooling CSR (graph_pool rows)
    colidx: torch.Tensor            # int64 [nnz]
    vals: torch.Tensor              # f32 [nnz]
    labels: Optional[torch.Tensor] = None   # int64 [B]
    input_y: Optional[torch.Tensor] = None  # int64 [N] (UnSup softmax labels)
    # int32[1] device flag the gather / scatter kernels set on an out-of-range input_x entry (they
    # read and write nothing there); the constructors validate input_x up front, so it stays 0
    err: Optional[torch.Tensor] = None
    # True when colidx is 0..N-1 in order (batches built from offsets, _pool_iota): the pool backward
    # then stores every row of its output (u2gnn_pool_bwd_rows) instead of accumulating into zeros
    block_rows: bool = False
    # True when graph g's nodes are the consecutive rows rowptr[g] .. rowptr[g+1]-1 (colidx is 0..N-1 in order):
    # what attention="graphs" needs, since its segments are rowptr.  from_offsets / from_store build such batches;
    # from_reference_inputs checks its graph_pool
    rows_contiguous: bool = False
    # the rows' attention pattern (attention="edges"): Adjacency.from_csr(*store.adjacency(graph_ids), N, device), or
    # the same arrays assembled on the GPU (from_store(..., graphs=DeviceGraphs)); the other modes never read it
    adj: Optional[Adjacency] = None
    # the pair types of attention="graphs" with ``distances``: PairTypes.from_store(store, graph_ids, N, device, H), or
    # the same integers searched on the GPU (from_store(..., graphs=DeviceGraphs, distances=H)); the other modes never
    # read it
    pairs: Optional[PairTypes] = None
    # the rows' node degrees, int32 [N], raw (the kernels clip): what ``centrality`` indexes the model's degree_emb with
    # -- from_offsets(..., degrees=store.degrees_of(graph_ids)) or from_store(..., degrees=the store's on the device);
    # without ``centrality`` nothing reads it
    deg: Optional[torch.Tensor] = None

    def __post_init__(self):
        if self.err is None:
            self.err = torch.zeros(1, device=self.X_concat.device, dtype=torch.int32)

    def check_indices(self):
        """IndexError if a kernel met an out-of-range input_x entry (host sync; F.embedding raises)."""
        if int(self.err.item()):
            raise IndexError("index out of range in self (input_x entry outside [0, N))")

    @property
    def idx_stride(self):
        return self.input_x.stride(0)

    @staticmethod
    def from_offsets(input_x, offsets, X_concat, labels=None, device="cuda", input_y=None, degrees=None):
        """Host arrays (numpy / torch CPU) -> HBM.  Block-diagonal graph_pool of ones given by
        node offsets (train_pytorch_U2GNN_Sup.py:73-89).  degrees: the rows' node degrees (a host array of N integers,
        GraphStore.degrees_of(graph_ids)) -> ``deg``."""
        dev = torch.device(device)
        _check_range_host(input_x, int(np.asarray(offsets)[-1]))
        ix = torch.as_tensor(input_x, dtype=torch.int64).to(dev, non_blocking=True).contiguous()
        X = torch.as_tensor(X_concat, dtype=torch.float32).to(dev, non_blocking=True).contiguous()
        off = torch.as_tensor(np.asarray(offsets), dtype=torch.int64)
        N = int(off[-1])
        B = off.numel() - 1
        lab = None if labels is None else torch.as_tensor(labels, dtype=torch.int64).to(dev, non_blocking=True)
        iy = None if input_y is None else torch.as_tensor(input_y, dtype=torch.int64).to(dev, non_blocking=True)
        deg = None
        if degrees is not None:
            deg = torch.as_tensor(np.asarray(degrees).astype(np.int32)).to(dev, non_blocking=True).contiguous()
            if deg.shape != (N,):
                raise ValueError(f"degrees: one per row, {N}, got {tuple(deg.shape)}")
        return DeviceBatch(N, B, ix, X, off.to(dev), torch.arange(N, device=dev, dtype=torch.int64),
                           torch.ones(N, device=dev, dtype=torch.float32), lab, iy, block_rows=True,
                           rows_contiguous=True, deg=deg)

    @staticmethod
    def from_store(hb, X_dev: torch.Tensor, device="cuda", graphs=None, distances=None, degrees=None):
        """A natively assembled batch (GraphStore.assemble(..., gather_x=False)) -> HBM: input_x, offsets
        and the rows' dataset node ids cross PCIe asynchronously from page-locked buffers (~0.7 MB at
        C4 instead of the 7 MB X_concat; BatchLoader assembles straight into a ring of them);
        X_concat is gathered on the GPU from the dataset's device-resident features X_dev [V, d]
        (u2gnn_gather_rows).  No host synchronisation.
        graphs: the store's pattern.DeviceGraphs -- the batch also gets its adjacency (``adj``, attention="edges"),
        assembled on the GPU from the device-resident structure: the graph ids and entry offsets travel with the
        arrays above, the row offsets are the batch's own, and the kernel runs beside the feature gather.
        distances = H (with ``graphs`` a structure built without hops): the batch gets its pair types instead (``pairs``,
        attention="graphs" with distances=H, no ``adj``), searched on the GPU from the one-hop structure
        (DeviceGraphs.launch_pairs) in the same place: ids and pair offsets travel with the arrays above.
        degrees: the store's node degrees resident on the device (int32 [V], uploaded once per dataset from store.deg):
        the batch's rows of it are gathered beside the features -> ``deg`` (``centrality``)."""
        from . import kernels as K
        if distances and graphs is None:
            raise ValueError("distances: the pair types are searched from graphs=DeviceGraphs (built without hops)")
        dev = torch.device(device)
        if degrees is not None and (degrees.dtype != torch.int32 or degrees.shape != (X_dev.shape[0],)
                                    or degrees.device != X_dev.device):
            raise ValueError("degrees: int32 [V] beside X_dev (torch.from_numpy(store.deg.astype(np.int32)).to(device))")
        N, B = int(hb.offsets[-1]), len(hb.offsets) - 1
        slot = getattr(hb, "pinned", None)
        _check_range_host(hb.input_x, N)
        plan = None
        if graphs is not None:   # host tables only: the ids checked, the entry (pair) offsets, nnz (pairs) and n_types
            plan = graphs.plan_pairs(hb.graph_ids, distances) if distances else graphs.plan(hb.graph_ids)
            if plan[3] != N or len(plan[0]) != B:
                raise ValueError(f"graphs: the structure gives the batch {plan[3]} rows, the batch has {N}")
            if distances:
                n_types = graphs.n_pair_types(plan[0], distances)
        if slot is not None and dev.type == "cuda":
            # the batch's transfers and its feature gather run on a copy stream, so the next batch
            # crosses PCIe while the current step computes; the compute stream waits on one event
            main = torch.cuda.current_stream(dev)
            cs = _copy_stream(dev)
            k1 = hb.input_x.shape[1]
            with torch.cuda.stream(cs):
                h2d = lambda t: t.to(dev, non_blocking=True)  # noqa: E731
                ix = h2d(slot.ix[:N * k1]).view(N, k1)
                gnode, off, lab = h2d(slot.gnode[:N]), h2d(slot.offsets[:B + 1]), h2d(slot.labels[:B])
                if plan is not None:
                    slot.gid.numpy()[:B], slot.ent_off.numpy()[:B + 1] = plan[0], plan[2]
                    gid, ent_off = h2d(slot.gid[:B]), h2d(slot.ent_off[:B + 1])
                slot.event = torch.cuda.Event()
                slot.event.record()
                d = X_dev.shape[1]
                X = torch.empty(N, d, device=dev, dtype=torch.float32)
                if N:
                    K.gather_rows(X_dev, gnode, 1, X, N, N, d, d)
                deg = degrees[gnode] if degrees is not None else None
                err = torch.zeros(1, device=dev, dtype=torch.int32)
                adj = pairs = None
                if distances:
                    pairs = graphs.launch_pairs(gid, off, ent_off, *plan[3:], distances, n_types)
                elif plan is not None:
                    adj = graphs.launch(gid, off, ent_off, *plan[3:])
            ready = torch.cuda.Event()
            ready.record(cs)
            main.wait_event(ready)
            used = [ix, gnode, off, lab, X, err]   # allocated on the copy stream, used on the compute one
            if deg is not None:
                used.append(deg)
            if adj is not None:   # (the adjacency's five arrays are views of one buffer, rowptr its start)
                used += [gid, ent_off, adj.rowptr] + ([adj.etype] if adj.etype is not None else [])
            if pairs is not None:   # (pair_off is ent_off)
                used += [gid, ent_off, pairs.etype]
            for t in used:
                t.record_stream(main)
            iy = gnode if hb.input_y is not None else None
            colidx, vals = _pool_iota(N, dev)
            return DeviceBatch(N, B, ix, X, off, colidx, vals, lab, iy, err, block_rows=True, rows_contiguous=True,
                               adj=adj, pairs=pairs, deg=deg)
        if slot is not None:
            k1 = hb.input_x.shape[1]
            h2d = lambda t: t.to(dev, non_blocking=True)  # noqa: E731
            ix = h2d(slot.ix[:N * k1]).view(N, k1)
            gnode, off, lab = h2d(slot.gnode[:N]), h2d(slot.offsets[:B + 1]), h2d(slot.labels[:B])
            slot.event = torch.cuda.Event()
            slot.event.record()
            iy = gnode if hb.input_y is not None else None   # UnSup labels = dataset node ids
        else:
            pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)  # noqa: E731
            ix, gnode, off = pin(hb.input_x), pin(hb.gnode), pin(np.asarray(hb.offsets, dtype=np.int64))
            lab = None if hb.labels is None else pin(np.asarray(hb.labels, dtype=np.int64))
            iy = None if hb.input_y is None else pin(np.asarray(hb.input_y, dtype=np.int64))
        d = X_dev.shape[1]
        X = torch.empty(N, d, device=dev, dtype=torch.float32)
        if N:
            K.gather_rows(X_dev, gnode, 1, X, N, N, d, d)
        colidx, vals = _pool_iota(N, dev)
        adj = pairs = None
        if distances:
            pairs = graphs.pair_types(hb.graph_ids, distances, off)
        elif graphs is not None:
            adj = graphs.adjacency(hb.graph_ids, off)
        return DeviceBatch(N, B, ix, X, off, colidx, vals, lab, iy, block_rows=True, rows_contiguous=True, adj=adj,
                           pairs=pairs, deg=degrees[gnode] if degrees is not None else None)

    @staticmethod
    def from_reference_inputs(input_x, graph_pool, X_concat, labels=None):
        """The reference forward() inputs: input_x int64 [N,k+1], graph_pool sparse COO [B,N],
        X_concat f32 [N,d] (pytorch_U2GNN_Sup.py:30)."""
        dev = X_concat.device
        gp = graph_pool.coalesce()
        B, N = gp.shape
        if input_x.numel() and (int(input_x.min()) < 0 or int(input_x.max()) >= int(N)):
            raise IndexError("index out of range in self (input_x entry outside [0, N))")
        rows, cols = gp.indices()
        vals = gp.values().to(torch.float32)
        rowptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=B), 0)
        # graph g's nodes as consecutive rows (attention="graphs"): the coalesced pool lists every column once, in
        # order (this constructor synchronises already)
        contiguous = cols.numel() == int(N) and bool(
            torch.equal(cols, torch.arange(int(N), device=cols.device, dtype=cols.dtype)))
        return DeviceBatch(int(N), int(B), input_x.to(dev).contiguous(), X_concat.to(torch.float32).contiguous(),
                           rowptr, cols.contiguous(), vals.contiguous(), labels, rows_contiguous=contiguous)


def _check_range_host(input_x, N: int):
    """F.embedding(input_x, X_concat) raises IndexError for an entry outside [0, N) (pytorch_U2GNN_Sup.py:32)."""
    a = input_x.numpy() if isinstance(input_x, torch.Tensor) else np.asarray(input_x)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= N):
        raise IndexError("index out of range in self (input_x entry outside [0, N))")


TRAILING = ("degree_emb", "hop_bias")   # the models' own trailing parameters, in flat-buffer order


def hop_bias_last(named, prefix: str = ""):
    """A model's named_parameters() with its own trailing parameters moved to the end: ..., ``degree_emb``, ``hop_bias``
    (TRAILING; whichever exist).  torch lists a module's own parameters before its children's, which would put them
    first; last, every other parameter keeps its place in the flat buffer (FlatParams) and the region after the last
    encoder layer ends where the first of them begins (dp.OverlappedGradAllReduce)."""
    keys = {(prefix + "." if prefix else "") + k: i for i, k in enumerate(TRAILING)}
    held = {}
    for n, p in named:
        if n in keys:
            held[keys[n]] = (n, p)
        else:
            yield n, p
    for i in sorted(held):
        yield held[i]


class EncoderStack:
    """L U2GNN layers x T post-LN encoder layers on slot-0 rows, with the re-gather between
    U2GNN layers (pytorch_U2GNN_Sup.py:33-39; pytorch_U2GNN_UnSup.py:55-64)."""

    def __init__(self, u2gnn_layers, d: int, ff: int, T: int, L: int, prec: str = "fp32", p_enc: float = 0.5,
                 attention: str = "nodes", hops: Optional[int] = None, hop_bias=None,
                 distances: Optional[int] = None, centrality: Optional[int] = None, degree_emb=None):
        """hops = H with attention="edges", or distances = H with attention="graphs": every layer adds
        hop_bias()[l][t][type] to its attention scores, type = the distance of an adjacency entry (hops) or the clipped
        distance of a pair of the graph (distances); hop_bias: a callable that returns the model's [L, T, H + 1]
        parameter (read where it lies at each forward).
        centrality = D (any attention): the stack's input is X_concat[n] + degree_emb()[min(deg[n], D)] (the batch's
        ``deg``), added inside the first gather; degree_emb: a callable that returns the model's [D + 1, d] parameter
        (read where it lies); the backward then takes layer (0, 0)'s input gradient and reduces it per degree class
        into grads["degree_emb"]."""
        self.layers, self.d, self.ff, self.T, self.L, self.prec, self.p_enc = u2gnn_layers, d, ff, T, L, prec, p_enc
        self.attention = check_attention(attention)
        self.hops, self.hop_bias = check_hops(hops, attention), hop_bias
        self.distances = check_distances(distances, attention, hops)
        self.n_types = (self.hops or self.distances or 0) + 1   # the width of a hop_bias table (1: no tables)
        self.centrality, self.degree_emb = check_centrality(centrality), degree_emb
        self.packed = None
        # Python orchestration only: the three-pass attention forward where the fused kernel would run
        # (tools/prec_train_probe.py)
        self.three_pass = False
        # optional callable(prefix, stream): called once a layer's parameter gradients are
        # enqueued (on `stream`), e.g. dp.OverlappedGradAllReduce.layer_done
        self.grad_ready = None

    @classmethod
    def for_module(cls, module, precision: str = "fp32") -> "EncoderStack":
        """The stack of a model module; encoder dropout is hard-coded to 0.5 (pytorch_U2GNN_Sup.py:20)."""
        return cls(module.u2gnn_layers, module.feature_dim_size, module.ff_hidden_size, module.num_self_att_layers,
                   module.num_U2GNN_layers, precision, 0.5, getattr(module, "attention", "nodes"),
                   getattr(module, "hops", None), lambda: module.hop_bias, getattr(module, "distances", None),
                   getattr(module, "centrality", None), lambda: module.degree_emb)

    def layer_params(self, l, t) -> LayerParams:
        return LayerParams.from_encoder_layer(self.layers[l].layers[t])

    def _pack(self, device):
        if self.packed is None:
            self.packed = [[PackedLayer(self.d, self.ff, device) for _ in range(self.T)] for _ in range(self.L)]
        jobs = []
        for l in range(self.L):
            for t in range(self.T):
                jobs += self.packed[l][t].jobs(self.layer_params(l, t))
        K.pack_padded_multi(jobs)      # one launch per 32 tensors

    def _pattern(self, b: "DeviceBatch"):
        """-> (pattern, W, stride): what a row of this batch's layers attends over (the one AttnPattern every layer
        call of a forward takes), and the layers' row layout: W rows per node (row n * W + s = slot s of node n;
        slot 0 is the node's output) gathered from input_x with ``stride``.  Validates the batch for the mode."""
        mode = self.attention
        if mode != "nodes" and not native.enabled():
            raise NotImplementedError(f"attention={mode!r} runs on the native layer executor (U2GNN_NATIVE_LAYER=1)")
        if mode == "neighbors":
            # paper semantics (U2GNN_tf/model_U2GNN_Sup_multi.py:14-45): every node attends
            # over its own k+1 gathered neighbour tokens; each layer runs on all N*W tokens (the executor's window mode)
            if not b.input_x.is_contiguous():
                raise ValueError("input_x must be contiguous [N, k+1]")
            W = b.input_x.shape[1]
            return AttnPattern.window(W), W, 1
        if mode == "graphs":
            # the "nodes" path with every layer's attention cut into the batch's graphs (b.rowptr, on the device)
            if not b.rows_contiguous:
                raise ValueError("attention='graphs' needs every graph's nodes as consecutive rows: graph_pool row g "
                                 "must hold the columns rowptr[g] .. rowptr[g+1]-1 and colidx must be 0..N-1 in order "
                                 "(DeviceBatch.from_offsets / from_store build such batches)")
            pairs = None
            if self.distances:
                pairs = b.pairs
                if pairs is None:
                    raise ValueError("distances needs the batch's pair types: set DeviceBatch.pairs = "
                                     "PairTypes.from_store(store, graph_ids, N, device, H) (reference-style tensor "
                                     "inputs carry no edges)")
                if pairs.N != b.N or pairs.pair_off.numel() != b.B + 1:
                    raise ValueError(f"distances: the pair types are over {pairs.N} rows in "
                                     f"{pairs.pair_off.numel() - 1} graphs, the batch has {b.N} in {b.B}")
                if pairs.n_types > self.distances + 1:
                    raise ValueError(f"distances={self.distances}: the pair types go up to {pairs.n_types - 1}")
            return AttnPattern.segments(b.rowptr[:b.B + 1].contiguous(), pairs), 1, b.idx_stride
        if mode == "edges":
            # the "nodes" path with every row attending over its row of the batch's adjacency (b.adj, on the device)
            if b.adj is None:
                raise ValueError("attention='edges' needs the batch's adjacency: set DeviceBatch.adj = "
                                 "Adjacency.from_csr(*store.adjacency(graph_ids), N, device) (reference-style tensor "
                                 "inputs carry no edges)")
            if b.adj.N != b.N:
                raise ValueError(f"attention='edges': the adjacency is over {b.adj.N} rows, the batch has {b.N}")
            if self.hops and b.adj.etype is None:
                raise ValueError("hops needs the entries' distances: Adjacency.from_csr(rowptr, colidx, N, device, "
                                 "etype=etype) with (rowptr, colidx, etype) = store.adjacency(graph_ids, hops=H)")
            if self.hops and b.adj.n_types > self.hops + 1:
                raise ValueError(f"hops={self.hops}: the adjacency holds distances up to {b.adj.n_types - 1}")
            return AttnPattern.csr(b.adj), 1, b.idx_stride
        return NODES, 1, b.idx_stride

    @staticmethod
    def _entry_types(pattern):
        """The pattern's entry types (int32, one per bias value): an adjacency's distances under ``hops``, the pair
        types under ``distances``."""
        return pattern.what.etype if pattern.kind == "csr" else pattern.pairs.etype

    def _degrees(self, b: "DeviceBatch"):
        """The batch's degrees for ``centrality`` (validated) and the table where it lies."""
        if b.deg is None:
            raise ValueError("centrality needs the batch's node degrees: DeviceBatch.from_offsets(..., degrees="
                             "store.degrees_of(graph_ids)) or from_store(..., degrees=the store's int32 degrees on the "
                             "device), or set DeviceBatch.deg (int32 [N]) (reference-style tensor inputs carry no "
                             "edges)")
        if b.deg.dtype != torch.int32 or b.deg.shape != (b.N,) or not b.deg.is_contiguous():
            raise ValueError(f"centrality: DeviceBatch.deg must be contiguous int32 [{b.N}]")
        table = self.degree_emb().detach()
        if table.shape != (self.centrality + 1, self.d):
            raise ValueError(f"centrality={self.centrality}: degree_emb must be [{self.centrality + 1}, {self.d}]")
        return b.deg, table

    def forward(self, b: "DeviceBatch", train: bool, need_ctx: bool, seed: int):
        """Returns (outs, ctx): outs[l] = padded [Np, dp] slot-0 output of U2GNN layer l."""
        pattern, W, stride = self._pattern(b)
        # hops / distances: the bias of all L * T layers per entry type, expanded from the tables in one launch.  The
        # tables are read where the parameter lies (the flat buffer under a trainer), so a replayed HIP graph sees
        # Adam's updates
        bias_all, n_bias = None, 0
        if self.n_types > 1:
            etype = self._entry_types(pattern)
            n_bias = etype.numel()
            tables = self.hop_bias().detach().view(self.L * self.T, self.n_types)
            bias_all = torch.empty(self.L * self.T, rup(n_bias, 4), device=tables.device, dtype=torch.float32)
            K.bias_expand(tables, etype, bias_all)
        dev = b.X_concat.device
        d, dp = self.d, rup(self.d, 64)
        dims = Dims(b.N, d, self.ff)                                  # the node rows: outs, the heads
        ldims = dims if W == 1 else Dims(b.N * W, d, self.ff)         # the layers' rows
        Np, R, Rp = dims.Np, ldims.N, ldims.Np
        self._pack(dev)
        slot0 = torch.arange(b.N, device=dev, dtype=torch.int64) * W if W > 1 else None
        X = torch.empty(Rp, dp, device=dev, dtype=torch.float32)
        if self.centrality:   # the table row of each gathered node's degree added on the way: still one launch
            K.gather_rows_emb(b.X_concat, b.input_x, stride, X, R, Rp, d, dp, *self._degrees(b), b.err)
        else:
            K.gather_rows(b.X_concat, b.input_x, stride, X, R, Rp, d, dp, b.err)
        outs, lctxs = [], []
        for l in range(self.L):
            lctx = []
            for t in range(self.T):
                seeds = {s: site_seed(seed, l, t, s) for s in (SITE_ATTN, SITE_DROP1, SITE_DROPFF, SITE_DROP2)}
                if native.enabled():
                    X, c = native.layer_forward(X, self.packed[l][t], self.layer_params(l, t), ldims, train, seeds,
                                                need_ctx, self.prec, self.p_enc, deep_wgrad=engine_deep_wgrad(),
                                                pattern=pattern, bias=None if bias_all is None else
                                                bias_all[l * self.T + t, :n_bias])
                else:
                    X, c = encoder_layer_forward(X, self.packed[l][t], self.layer_params(l, t), dims, train, seeds,
                                                 need_ctx, self.prec, self.p_enc, three_pass=self.three_pass)
                lctx.append(c)
            if slot0 is not None:   # slot 0 of every node's window is the node's output
                out = torch.empty(Np, dp, device=dev, dtype=torch.float32)
                K.gather_rows(X, slot0, 1, out, b.N, Np, d, dp)
                X = out
            outs.append(X)
            lctxs.append(lctx)
            if l + 1 < self.L:
                Xn = torch.empty(Rp, dp, device=dev, dtype=torch.float32)
                K.gather_rows(X, b.input_x, stride, Xn, R, Rp, d, dp, b.err)
                X = Xn
        return outs, {"dims": dims, "layers": lctxs, "batch": b, "ldims": ldims, "stride": stride, "slot0": slot0,
                      "pattern": pattern}

    def _layer_grads_done(self, pre: str, off: OffPath, need_dx: bool) -> None:
        """Hand a layer's finished parameter-gradient region to ``grad_ready`` with a stream ordered after
        EVERY write of that region.  A layer with an input gradient writes its parameter gradients on the
        side stream after a fork from this one (encoder_layer.cpp flush after sd.fork(); engine OffPath.run),
        so the side stream covers them.  The last layer of the backward (need_dx false) writes them on THIS
        stream (encoder_layer.cpp: flush on `st`; engine.py: in_proj_grads inline, the rest on the side
        stream), so the side stream first waits for this one -- nothing is queued behind it any more, so no
        overlap is lost.  Without the wait a collective issued on the side stream read the region before
        the main stream had written it (tests/test_grad_order_gpu.py)."""
        if self.grad_ready is None:
            return
        if not need_dx and off.side is not None:
            off.side.wait_stream(torch.cuda.current_stream())
        self.grad_ready(pre, off.side)

    def backward(self, ctx, ext_grad, grads: dict, prefix: str = "u2gnn_layers"):
        """ext_grad(l) -> fresh padded gradient of outs[l] from outside the stack (head / loss).
        Writes encoder parameter gradients into grads[<reference key>]; returns None (the stack
        input, rows of X_concat, takes no gradient) -- with ``centrality`` the gradient of the stack's input rows,
        after reducing it per degree class into grads["degree_emb"]."""
        b = ctx["batch"]
        ldims, stride, slot0 = ctx["ldims"], ctx["stride"], ctx["slot0"]
        dnext = None
        off = OffPath(b.input_x.device, enabled=side_stream_pays(ldims))
        # hops / distances: every layer leaves dL/dbias of its entries in its row; one reduction to the tables after
        # the last layer
        dbias_all, etype = None, None
        if self.n_types > 1:
            etype = self._entry_types(ctx["pattern"])
            dbias_all = torch.empty(self.L * self.T, rup(etype.numel(), 4), device=b.input_x.device,
                                    dtype=torch.float32)
        for l in reversed(range(self.L)):
            dX = ext_grad(l)                                     # [Np, dp] node rows
            if dnext is not None:                                # re-gather of the next U2GNN layer
                K.scatter_add_rows(dnext, b.input_x, stride, dX, ldims.N, self.d, b.err)
            if slot0 is not None:                                # the node's gradient enters at slot 0 of its window
                dOut, dX = dX, torch.zeros(ldims.Np, ldims.dp, device=dX.device, dtype=torch.float32)
                K.scatter_add_rows(dOut, slot0, 1, dX, b.N, self.d)
            for t in reversed(range(self.T)):
                pre = f"{prefix}.{l}.layers.{t}."
                g = LayerParams(*[grads[pre + k] for k in LAYER_KEYS])
                lc = ctx["layers"][l][t]
                # the stack's input (gathered X_concat rows) is not trainable: no dX out of layer (0, 0) -- unless
                # ``centrality`` adds its table to it.  (That layer then writes its parameter gradients on the side
                # stream after the fork, as every layer with an input gradient does: _layer_grads_done)
                need_dx = l > 0 or t > 0 or bool(self.centrality)
                if isinstance(lc, native.NativeCtx):
                    dX = native.layer_backward(dX, lc, self.packed[l][t], self.layer_params(l, t), g, ldims,
                                               self.prec, side=off.side, deep_wgrad=engine_deep_wgrad(),
                                               need_dx=need_dx,
                                               dbias=None if dbias_all is None else
                                               dbias_all[l * self.T + t, :etype.numel()])
                else:
                    dX = encoder_layer_backward(dX, lc, self.packed[l][t], self.layer_params(l, t), g, ldims,
                                                self.prec, off=off, need_dx=need_dx)
                self._layer_grads_done(pre, off, need_dx)
            dnext = dX
        if dbias_all is not None:
            K.bias_table_grad(dbias_all, etype, grads["hop_bias"].view(self.L * self.T, self.n_types))
        if self.centrality:   # d degree_emb[c] = the sum of layer (0, 0)'s input-gradient rows of class c (this stream)
            K.class_rows_grad(dnext, b.input_x, stride, b.deg, b.N, ldims.N, self.d, grads["degree_emb"])
        off.join()   # parameter gradients complete before the caller's optimizer reads them
        return dnext


class SupCore:
    """Forward/backward of the supervised TransformerU2GNN (pytorch_U2GNN_Sup.py:30-46)."""

    def __init__(self, module, precision: str = "fp32"):
        self.m = module
        self.d = module.feature_dim_size
        self.C = module.num_classes
        self.L = module.num_U2GNN_layers
        self.p_head = module.dropout_p        # args.dropout, pytorch_U2GNN_Sup.py:28
        self.stack = EncoderStack.for_module(module, precision)

    def forward(self, b: DeviceBatch, train: bool, need_ctx: bool, seed: int):
        dev = b.X_concat.device
        d, dp = self.d, rup(self.d, 64)
        outs, sctx = self.stack.forward(b, train, need_ctx, seed)
        scores = torch.empty(b.B, self.C, device=dev, dtype=torch.float32)
        ph = self.p_head if train else 0.0
        heads = []
        for l in range(self.L):
            G = torch.empty(b.B, dp, device=dev, dtype=torch.float32)
            hs = site_seed(seed, l, 0, SITE_HEAD)
            K.pool_fwd(outs[l], dp, b.rowptr, b.colidx, b.vals, G, dp, b.B, d, ph, hs)
            K.head_fwd(G, dp, self.m.predictions[l].weight, self.m.predictions[l].bias, scores, b.B, self.C, d,
                       accumulate=l > 0)
            heads.append((G, hs))
        return scores, {"stack": sctx, "heads": heads, "ph": ph, "batch": b}

    def backward(self, ctx, dscores: torch.Tensor, grads: dict):
        """grads: name -> real-shaped tensor (reference state_dict key names)."""
        b: DeviceBatch = ctx["batch"]
        dims: Dims = ctx["stack"]["dims"]
        dev = dscores.device
        d, dp, Np = self.d, dims.dp, dims.Np

        def ext(l):
            G, hs = ctx["heads"][l]
            dG = torch.empty(b.B, dp, device=dev, dtype=torch.float32)
            K.head_bwd(dscores, G, dp, self.m.predictions[l].weight, dG, dp, grads[f"predictions.{l}.weight"],
                       grads[f"predictions.{l}.bias"], b.B, self.C, d)
            if b.block_rows:   # every row stored: no zero fill, no atomics
                dX = torch.empty(Np, dp, device=dev, dtype=torch.float32)
                K.pool_bwd_rows(dG, dp, b.rowptr, b.colidx, b.vals, dX, dp, b.B, d, dp, b.N, Np, ctx["ph"], hs)
            else:
                dX = torch.zeros(Np, dp, device=dev, dtype=torch.float32)
                K.pool_bwd(dG, dp, b.rowptr, b.colidx, b.vals, dX, dp, b.B, d, ctx["ph"], hs)
            return dX
        return self.stack.backward(ctx["stack"], ext, grads)


LAYER_KEYS = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
              "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
              "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"]


class FlatParams:
    """Re-homes every parameter of ``module`` into one flat fp32 device buffer (params become
    views, keeping their reference shapes and state_dict keys) with a matching flat grad buffer."""

    def __init__(self, module: torch.nn.Module, names=None):
        sel = None if names is None else set(names)
        self.names, self.params = zip(*[(n, p) for n, p in module.named_parameters() if sel is None or n in sel])
        dev = self.params[0].device
        sizes = [p.numel() for p in self.params]
        # 16-byte aligned offsets for the float4 sweeps
        offs, o = [], 0
        for s in sizes:
            offs.append(o)
            o += rup(s, 4)
        self.n = o
        self.flat = torch.zeros(o, device=dev, dtype=torch.float32)
        self.gflat = torch.zeros(o, device=dev, dtype=torch.float32)
        self.grads = {}
        for name, p, off, s in zip(self.names, self.params, offs, sizes):
            self.flat[off:off + s].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + s].view(p.shape)
            gv = self.gflat[off:off + s].view(p.shape)
            p.grad = gv
            self.grads[name] = gv


class FusedAdam:
    """torch.optim.Adam (lr, betas=(0.9, 0.999), eps=1e-8, no weight decay) preceded by
    clip_grad_norm_(max_norm) — both on device over the flat buffers, no host sync."""

    def __init__(self, flat: FlatParams, lr: float, max_norm: Optional[float] = 0.5, betas=(0.9, 0.999),
                 eps: float = 1e-8):
        self.f = flat
        self.lr, self.max_norm, self.betas, self.eps = lr, max_norm, betas, eps
        dev = flat.flat.device
        self.m = torch.zeros_like(flat.flat)
        self.v = torch.zeros_like(flat.flat)
        self.ws = torch.empty(1024, device=dev, dtype=torch.float32)
        self.sq = torch.zeros(1, device=dev, dtype=torch.float32)
        self.step_count = 0
        # device-resident schedule (HIP-graph replay, train.StepGraphs): step count t and lr live in
        # HBM, u2gnn_step_advance bumps t inside the captured step, u2gnn_adam_dev forms the bias
        # corrections on the device
        self.t_dev: Optional[torch.Tensor] = None
        self.lr_dev: Optional[torch.Tensor] = None

    def use_device_schedule(self) -> None:
        dev = self.f.flat.device
        self.t_dev = torch.full((1,), self.step_count, device=dev, dtype=torch.int64)
        self.lr_dev = torch.full((1,), float(self.lr), device=dev, dtype=torch.float64)

    def use_host_schedule(self) -> None:
        if self.t_dev is not None:
            self.step_count = int(self.t_dev.item())
        self.t_dev = self.lr_dev = None

    def set_lr(self, lr: float) -> None:
        self.lr = lr
        if self.lr_dev is not None:
            self.lr_dev.fill_(float(lr))

    def step(self):
        b1, b2 = self.betas
        clip = self.max_norm is not None
        if clip:   # the partial sums of g^2; Adam's blocks fold them (u2gnn_adam(_dev)_sq): 2 launches, not 3
            K.sqnorm_partials(self.f.gflat, self.f.n, self.ws)
        if self.t_dev is not None:
            # inside a captured step the graph's first node (StepGraphs: u2gnn_step_advance) bumps t;
            # an eager step taken while the device schedule is live bumps it here, so every path
            # advances t exactly once per step (a fresh t of 0 gave lr / (1 - b1^0) = inf)
            if not torch.cuda.is_current_stream_capturing():
                K.step_advance(None, self.t_dev)
            if clip:
                K.adam_dev_sq(self.f.flat, self.f.gflat, self.m, self.v, self.f.n, self.ws, self.sq, self.max_norm,
                              b1, b2, self.eps, self.lr_dev, self.t_dev)
            else:
                K.adam_dev(self.f.flat, self.f.gflat, self.m, self.v, self.f.n, None, 0.0, b1, b2, self.eps,
                           self.lr_dev, self.t_dev)
            return
        self.step_count += 1
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        if clip:
            K.adam_sq(self.f.flat, self.f.gflat, self.m, self.v, self.f.n, self.ws, self.sq, self.max_norm, b1, b2,
                      self.eps, self.lr / bc1, math.sqrt(bc2))
        else:
            K.adam(self.f.flat, self.f.gflat, self.m, self.v, self.f.n, None, 0.0, b1, b2, self.eps, self.lr / bc1,
                   math.sqrt(bc2))

    def grad_norm(self) -> float:
        return float(self.sq.sqrt().item())
