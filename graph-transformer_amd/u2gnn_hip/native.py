"""Python handle on the native encoder-layer executor (csrc/encoder_layer.cpp,
include/u2gnn_hip.h u2gnn_layer_*): one C-ABI call per layer forward / backward.

engine.py issues the same kernel sequence launch by launch from Python (kept as the readable
reference orchestration and for per-GEMM event timing); this module is the production path.  Every tile, split
count and threshold of that sequence is decided in the executor alone: engine.py asks layer_plan / split_plan
below (u2gnn_layer_plan, u2gnn_gemm_split_plan; host-only calls, cached by their arguments).
The rows a layer's rows attend over are one argument, a pattern.AttnPattern (NODES, window, segments or csr).
Buffers come from the torch caching allocator: the forward's saved tensors live in one uint8
"ctx" tensor per layer, workspaces are allocated per call.  Memory read by the backward's
side stream is record_stream'ed so the allocator cannot recycle it early.
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import LayerDims, LayerGrads, LayerParamsC, LayerSeeds, check, hip_lib
from .kernels import PREC
from .pattern import NODES, AttnPattern

_SIZES: Dict[tuple, tuple] = {}
_LAYER_PLANS: Dict[tuple, _lib.LayerPlan] = {}
_SPLIT_PLANS: Dict[tuple, _lib.SplitPlan] = {}
# a product precision that is no layer precision, as the layer precision whose forward products run on it
_PRODUCT_PREC = {"bf16x6": "fwd6", "f16x3": "fwdh"}


_ENABLED = [os.environ.get("U2GNN_NATIVE_LAYER", "1") == "1"]


def enabled() -> bool:
    """U2GNN_NATIVE_LAYER=0 routes layers through the Python orchestration (engine.py)."""
    return _ENABLED[0]


def set_enabled(on: bool) -> bool:
    """bench.py's per-GEMM timing pass runs the Python orchestration (its wrappers carry the HIP
    events); returns the previous setting."""
    prev = _ENABLED[0]
    _ENABLED[0] = bool(on)
    return prev


def _dims(N: int, d: int, ff: int, prec: str, deep_wgrad: bool, window: int = 0) -> LayerDims:
    flags = _lib.LAYER_DEEP_WGRAD if deep_wgrad else 0
    if prec == "mixed":   # bf16x3 except the attention-backward products dS, dQ, dK (engine.MIXED_BF16_ROLES)
        prec, flags = "bf16x3", flags | _lib.LAYER_ATTN_BWD_BF16
    elif prec == "fwd32":  # exact fp32 forward products, bf16x3 backward (engine.FWD_ROLES)
        prec, flags = "bf16x3", flags | _lib.LAYER_FWD_F32
    elif prec == "fwd6":   # bf16x6 forward products, bf16x3 backward (engine.FWD_ROLES)
        prec, flags = "bf16x3", flags | _lib.LAYER_FWD_X6
    elif prec == "fwdh":   # f16x3 forward products, bf16x3 backward (engine.FWD_ROLES)
        prec, flags = "bf16x3", flags | _lib.LAYER_FWD_H3
    return LayerDims(int(N), int(d), int(ff), PREC[prec], flags, int(window), 0)


def sizes(N: int, d: int, ff: int, prec: str, p_drop: float, deep_wgrad: bool = True, pattern: AttnPattern = NODES):
    """(ctx, forward workspace, backward workspace) bytes of a layer under ``pattern``: they depend on its kind, window
    and nnz only (pattern.key), never on the offsets or the columns (the CSR backward workspace holds 2 nnz floats)."""
    key = (N, d, ff, prec, p_drop > 0, deep_wgrad) + pattern.key
    r = _SIZES.get(key)
    if r is None:
        c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        dims = _dims(N, d, ff, prec, deep_wgrad, pattern.W)
        check(hip_lib().u2gnn_layer_sizes_csr(ctypes.byref(dims), float(p_drop), 1 if pattern.kind == "segments" else 0,
                                              pattern.nnz, ctypes.byref(c), ctypes.byref(f), ctypes.byref(b)),
              "u2gnn_layer_sizes_csr")
        r = _SIZES[key] = (c.value, f.value, b.value)
    return r


def layer_plan(dims, prec: str, p_drop: float) -> _lib.LayerPlan:
    """The executor's shape rules (u2gnn_layer_plan) of the node-axis layer dims (N, d, ff) at dropout p_drop; prec: a
    layer precision, or the precision of the product the rule is asked for (engine._rp)."""
    key = (dims.N, dims.d, dims.ff, prec, float(p_drop))
    r = _LAYER_PLANS.get(key)
    if r is None:
        r = _lib.LayerPlan()
        dd = _dims(dims.N, dims.d, dims.ff, _PRODUCT_PREC.get(prec, prec), True)
        check(hip_lib().u2gnn_layer_plan(ctypes.byref(dd), float(p_drop), ctypes.byref(r)), "u2gnn_layer_plan")
        _LAYER_PLANS[key] = r
    return r


def split_plan(M: int, N: int, K: int, prec: str, accumulate=False, deep=False, mapped=False, grouped=False,
               deep_wgrad=True, held=False) -> _lib.SplitPlan:
    """How the executor's split-K runs the product C[M, N] (+)= op(A) op(B) of depth K in the product precision
    prec (u2gnn_gemm_split_plan; the flags: u2gnn_hip.h u2gnn_split_query)."""
    key = (M, N, K, prec, accumulate, deep, mapped, grouped, deep_wgrad, held)
    r = _SPLIT_PLANS.get(key)
    if r is None:
        r = _lib.SplitPlan()
        q = _lib.SplitQuery(int(M), int(N), int(K), PREC[prec], *(int(bool(f)) for f in key[4:]))
        check(hip_lib().u2gnn_gemm_split_plan(ctypes.byref(q), ctypes.byref(r)), "u2gnn_gemm_split_plan")
        _SPLIT_PLANS[key] = r
    return r


def _params(packed, p) -> LayerParamsC:
    return LayerParamsC(packed.W_in.data_ptr(), packed.b_in.data_ptr(), packed.W_o.data_ptr(), packed.b_o.data_ptr(),
                        packed.W1.data_ptr(), packed.b1.data_ptr(), packed.W2.data_ptr(), packed.b2.data_ptr(),
                        p.n1_w.data_ptr(), p.n1_b.data_ptr(), p.n2_w.data_ptr(), p.n2_b.data_ptr())


def _seeds(p_drop: float, seeds: Dict[int, int]) -> LayerSeeds:
    from .engine import SITE_ATTN, SITE_DROP1, SITE_DROP2, SITE_DROPFF
    return LayerSeeds(float(p_drop), seeds.get(SITE_ATTN, 0), seeds.get(SITE_DROP1, 0), seeds.get(SITE_DROPFF, 0),
                      seeds.get(SITE_DROP2, 0))


# what the backward needs from one layer's forward
NativeCtx = namedtuple("NativeCtx", "X buf p_drop seeds pattern bias")


def _stream(s=None):
    return ctypes.c_void_p((s or torch.cuda.current_stream()).cuda_stream)


def _entry_bias(t, pattern, dev, what):
    """The pointer of a layer's attention bias (or its gradient): contiguous float32 on the layer's device, one per
    entry of a csr pattern's adjacency (pattern.nnz) or per pair of a segments pattern's pair types
    (pattern.pairs.n_pairs); None: NULL."""
    if t is None:
        return None
    n = pattern.nnz if pattern.kind == "csr" else pattern.pairs.n_pairs if pattern.pairs is not None else -1
    if n < 1 or not t.is_cuda or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise _lib.U2GNNNativeError(f"{what}: a contiguous float32 tensor on the layer's device, one value per entry "
                                    "of the adjacency (csr) or per pair of the pair types (segments with pairs)")
    return ctypes.c_void_p(t.data_ptr())


def _pair_biased(pattern, bias) -> bool:
    """Whether the call goes through u2gnn_layer_*_segb: a segments pattern that carries pairs, with a bias."""
    return bias is not None and pattern.kind == "segments" and pattern.pairs is not None


def _shared_args(dims, packed, p, prec, deep_wgrad, pattern, p_drop, seeds, X):
    """(dims, params, seeds, X): what u2gnn_layer_fwd_csrb and u2gnn_layer_bwd_csrb take alike in front.  The attention
    pattern that goes before the streams is pattern.c_args -- NULL, 0, NULL for a layer with neither segments nor a
    CSR, which with a NULL bias is the plain u2gnn_layer_fwd / u2gnn_layer_bwd call."""
    dd, pp, ss = _dims(dims.N, dims.d, dims.ff, prec, deep_wgrad, pattern.W), _params(packed, p), _seeds(p_drop, seeds)
    return ctypes.byref(dd), ctypes.byref(pp), ctypes.byref(ss), X.data_ptr()


def layer_forward(X: torch.Tensor, packed, p, dims, train: bool, seeds: Dict[int, int], need_ctx: bool,
                  prec: str, p_enc: float, deep_wgrad: bool = True, pattern: AttnPattern = NODES, bias=None):
    """pattern (pattern.AttnPattern): the rows every row of X attends over -- NODES: all dims.N rows; window(W): its
    node's W token rows (dims.N = nodes * W); segments(offsets): the rows of its own segment (per-graph attention);
    csr(adjacency): the columns of its CSR row (neighbour attention).  bias (f32 device): added to the scores before
    the softmax -- [pattern.nnz] per entry of a csr pattern, or [pattern.pairs.n_pairs] per pair of a segments pattern
    that carries pairs (PairTypes' packed order)."""
    pd = p_enc if train else 0.0
    cb, fb, _ = sizes(dims.N, dims.d, dims.ff, prec, pd, deep_wgrad, pattern)
    dev = X.device
    X2 = torch.empty(dims.Np, dims.dp, device=dev, dtype=torch.float32)
    buf = torch.empty(cb, device=dev, dtype=torch.uint8) if need_ctx else None
    ws = torch.empty(max(256, fb + (0 if need_ctx else cb)), device=dev, dtype=torch.uint8)
    head = _shared_args(dims, packed, p, prec, deep_wgrad, pattern, pd, seeds, X)
    if _pair_biased(pattern, bias):
        check(hip_lib().u2gnn_layer_fwd_segb(*head, X2.data_ptr(), buf.data_ptr() if buf is not None else None, cb,
                                             ws.data_ptr(), ws.numel(), *pattern.c_args(dev)[:2],
                                             *pattern.pair_args(dev), _entry_bias(bias, pattern, dev, "bias"),
                                             _stream()), "u2gnn_layer_fwd_segb")
        return X2, NativeCtx(X, buf, pd, dict(seeds), pattern, bias) if need_ctx else None
    check(hip_lib().u2gnn_layer_fwd_csrb(*head, X2.data_ptr(), buf.data_ptr() if buf is not None else None, cb,
                                         ws.data_ptr(), ws.numel(), *pattern.c_args(dev),
                                         _entry_bias(bias, pattern, dev, "bias"), _stream()), "u2gnn_layer_fwd_csrb")
    return X2, NativeCtx(X, buf, pd, dict(seeds), pattern, bias) if need_ctx else None


def layer_backward(dX2: torch.Tensor, ctx: NativeCtx, packed, p, g, dims, prec: str,
                   side: Optional["torch.cuda.Stream"] = None, deep_wgrad: bool = True,
                   need_dx: bool = True, dbias=None) -> Optional[torch.Tensor]:
    """The forward's pattern and bias are taken from ctx; dbias (f32 device, the bias's length, only for a forward with
    a bias) receives the bias's gradient."""
    if dbias is not None and ctx.bias is None:
        raise _lib.U2GNNNativeError("layer_backward: dbias given for a forward that ran without a bias")
    pattern = ctx.pattern
    cb, _, bb = sizes(dims.N, dims.d, dims.ff, prec, ctx.p_drop, deep_wgrad, pattern)
    dev = dX2.device
    dX = torch.empty(dims.Np, dims.dp, device=dev, dtype=torch.float32) if need_dx else None
    ws = torch.empty(max(256, bb), device=dev, dtype=torch.uint8)
    head = _shared_args(dims, packed, p, prec, deep_wgrad, pattern, ctx.p_drop, ctx.seeds, ctx.X)
    gg = LayerGrads(*[getattr(g, k).data_ptr() for k in _lib._PKEYS])
    if _pair_biased(pattern, ctx.bias):
        check(hip_lib().u2gnn_layer_bwd_segb(*head, ctx.buf.data_ptr(), cb, dX2.data_ptr(),
                                             dX.data_ptr() if need_dx else None, ctypes.byref(gg), ws.data_ptr(),
                                             ws.numel(), *pattern.c_args(dev)[:2], *pattern.pair_args(dev),
                                             _entry_bias(ctx.bias, pattern, dev, "bias"),
                                             _entry_bias(dbias, pattern, dev, "dbias"), _stream(),
                                             _stream(side) if side is not None else None), "u2gnn_layer_bwd_segb")
    else:
        check(hip_lib().u2gnn_layer_bwd_csrb(*head, ctx.buf.data_ptr(), cb, dX2.data_ptr(),
                                             dX.data_ptr() if need_dx else None, ctypes.byref(gg), ws.data_ptr(),
                                             ws.numel(), *pattern.c_args(dev),
                                             _entry_bias(ctx.bias, pattern, dev, "bias"),
                                             _entry_bias(dbias, pattern, dev, "dbias"), _stream(),
                                             _stream(side) if side is not None else None), "u2gnn_layer_bwd_csrb")
    if side is not None:
        for t in (ws, ctx.buf, ctx.X, dX2):
            t.record_stream(side)
    return dX


def probe_arm(role: int, capacity: int) -> None:
    """Time the next `capacity` executor launches of one product (``_lib.ROLE_*``) with HIP events
    recorded on the stream each kernel runs on (u2gnn_probe_arm)."""
    check(hip_lib().u2gnn_probe_arm(int(role), int(capacity)), "u2gnn_probe_arm")


def probe_collect():
    """(summed device milliseconds, launches) of the armed probe; frees its events."""
    ms, n = ctypes.c_float(), ctypes.c_int32()
    check(hip_lib().u2gnn_probe_collect(ctypes.byref(ms), ctypes.byref(n)), "u2gnn_probe_collect")
    return float(ms.value), int(n.value)
