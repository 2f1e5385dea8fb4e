"""Per-graph attention kernels (csrc/segment_attn.hip) against a float64 dense restatement: Q K^T with -inf
outside the diagonal blocks, softmax, the kernels' own dropout mask (K.dropout_mask over the global indices),
gradients by autograd.  The offsets are chosen to break tiling: sizes 1, 17, an empty segment, 64, 1, 316 (several
key tiles) and 37 with padding rows; one segment equal to N; segments aligned to the tile height."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from u2gnn_hip import kernels as K  # noqa: E402

DEV = "cuda"
RAGGED = [0, 1, 2, 19, 19, 83, 84, 400, 437]
SEED = 4321
Q_SCALE = 1 / math.sqrt(7.0)


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def _pad(n):
    return (n + 127) // 128 * 128


def _inputs(N, rows_pad, dp, gen_seed=1):
    g = torch.Generator(device=DEV).manual_seed(gen_seed)
    QKV = torch.randn(rows_pad, 3 * dp, device=DEV, generator=g)
    QKV[:, :dp] *= 1 / math.sqrt(dp)      # scores of order 1, as the in-projection's 1/sqrt(d) leaves them
    QKV[N:] = 0
    dO = torch.randn(rows_pad, dp, device=DEV, generator=g)
    dO[N:] = 0
    return QKV, dO


def _run(QKV, dO, offsets, N, rows_pad, dp, p):
    off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    O = torch.full((rows_pad, dp), float("nan"), device=DEV)
    stats = torch.full((rows_pad, 2), float("nan"), device=DEV)
    K.segment_attn_fwd(QKV, dp, off, O, stats, p, SEED, N, rows_pad)
    dQKV = torch.full((rows_pad, 3 * dp), float("nan"), device=DEV)
    K.segment_attn_bwd(QKV, dp, off, O, dO, stats, p, SEED, Q_SCALE, dQKV, N, rows_pad)
    return O, stats, dQKV


def _reference(QKV, dO, offsets, N, dp, p):
    """float64, dense: (O, dQ, dK, dV) over the N real rows."""
    q = QKV[:N, :dp].double().clone().requires_grad_(True)
    k = QKV[:N, dp:2 * dp].double().clone().requires_grad_(True)
    v = QKV[:N, 2 * dp:3 * dp].double().clone().requires_grad_(True)
    seg = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    for g in range(len(offsets) - 1):
        seg[offsets[g]:offsets[g + 1]] = g
    same = (seg[:, None] == seg[None, :]) & (seg[:, None] >= 0)
    S = (q @ k.t()).masked_fill(~same, float("-inf"))
    P = torch.softmax(S, dim=-1)
    if p > 0:
        P = P * K.dropout_mask(SEED, N, N, p).double() / (1 - p)
    O = P @ v
    O.backward(dO[:N].double())
    return O.detach(), q.grad, k.grad, v.grad


def _check(offsets, rows_pad, dp, p):
    N = offsets[-1]
    QKV, dO = _inputs(N, rows_pad, dp)
    O, stats, dQKV = _run(QKV, dO, offsets, N, rows_pad, dp, p)
    assert torch.isfinite(O).all() and torch.isfinite(dQKV).all() and torch.isfinite(stats).all()
    Or, dq, dk, dv = _reference(QKV, dO, offsets, N, dp, p)
    figs = {"O": rel(O[:N].double(), Or), "dQ": rel(dQKV[:N, :dp].double(), dq * Q_SCALE),
            "dK": rel(dQKV[:N, dp:2 * dp].double(), dk), "dV": rel(dQKV[:N, 2 * dp:].double(), dv)}
    print(f"segment_attn offsets={offsets} dp={dp} p={p}: {figs}")
    for name, f in figs.items():
        assert f < 1e-5, (name, f)
    if N < rows_pad:
        assert O[N:].abs().max().item() == 0 and dQKV[N:].abs().max().item() == 0
    # bit-identical from run to run
    O2, stats2, dQKV2 = _run(QKV, dO, offsets, N, rows_pad, dp, p)
    assert torch.equal(O, O2) and torch.equal(stats, stats2) and torch.equal(dQKV, dQKV2)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384])
@pytest.mark.parametrize("offsets,rows_pad", [(RAGGED, 512), ([0, 437], 512), ([0, 16, 32, 48, 64], 128)],
                         ids=["ragged", "one", "aligned"])
def test_segment_attention_fwd_bwd(offsets, rows_pad, dp, p):
    _check(offsets, rows_pad, dp, p)


def test_segment_attention_widest():
    _check([0, 1, 2, 19, 19, 83], 128, 1024, 0.5)


def test_segments_do_not_mix():
    """A cross-segment entry of dK / dV cannot be non-zero by construction; through the result: perturbing V (and K)
    inside one segment leaves the O rows of every other segment bit-unchanged."""
    dp, N, rows_pad, p = 384, RAGGED[-1], 512, 0.5
    QKV, dO = _inputs(N, rows_pad, dp)
    O, _, _ = _run(QKV, dO, RAGGED, N, rows_pad, dp, p)
    a0, a1 = 84, 400                      # the 316-row segment
    QKV2 = QKV.clone()
    QKV2[a0:a1, dp:] += 1.0
    O2, _, _ = _run(QKV2, dO, RAGGED, N, rows_pad, dp, p)
    assert torch.equal(O[:a0], O2[:a0]) and torch.equal(O[a1:], O2[a1:])
    assert not torch.equal(O[a0:a1], O2[a0:a1])


def test_uncovered_rows_and_bad_arguments():
    """Rows before the first / after the last segment get zero output; offsets past N are clamped; argument errors
    are refused before a launch."""
    from u2gnn_hip._lib import U2GNNNativeError
    dp, N, rows_pad = 64, 100, 128
    QKV, dO = _inputs(N, rows_pad, dp)
    O, _, dQKV = _run(QKV, dO, [5, 40, 90], N, rows_pad, dp, 0.0)
    assert O[:5].abs().max().item() == 0 and O[90:].abs().max().item() == 0
    assert dQKV[:5].abs().max().item() == 0 and dQKV[90:].abs().max().item() == 0
    Or, _, _, _ = _reference(QKV, dO, [5, 40, 90], N, dp, 0.0)
    assert rel(O[5:90].double(), Or[5:90]) < 1e-5
    Oc, _, dc = _run(QKV, dO, [-7, 40, 10 ** 9], N, rows_pad, dp, 0.0)    # clamped to [0, N]
    Orc, _, _, _ = _reference(QKV, dO, [0, 40, N], N, dp, 0.0)
    assert rel(Oc[:N].double(), Orc) < 1e-5 and torch.isfinite(dc).all()
    off = torch.tensor([0, N], dtype=torch.int64, device=DEV)
    st = torch.empty(rows_pad, 2, device=DEV)
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_fwd(QKV, dp, off, O, st, 1.0, SEED, N, rows_pad)          # p outside [0, 1)
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_fwd(QKV, 32, off, O, st, 0.0, SEED, N, rows_pad)          # dp % 64
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_fwd(QKV, dp, off[:1], O, st, 0.0, SEED, N, rows_pad)      # n_seg < 1
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_fwd(QKV.cpu(), dp, off, O, st, 0.0, SEED, N, rows_pad)    # host tensor
