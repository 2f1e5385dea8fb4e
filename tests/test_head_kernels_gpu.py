"""The kernels of csrc/head_ops.hip against the float64 references of tests/head_ref.py, at the edges of their
loops: the 4-deep / 16-deep load batches and their remainders, the float4 paths and their scalar tails, the 64-column
chunks, the two-sample and eight-row unrolls of the sampled softmax, block boundaries of flat thread ranges.

Every launch is in bounds by construction: each buffer is sized from the kernel's own index expression, input
padding the kernel must not read holds NaN, output padding it must not write holds SENT and is compared bit for bit.

Tolerances (metric: head_ref.rel_err = max|got - ref| / max|ref|).  Each bound is the larger of 1e-5 -- the bar
tests/test_kernels_gpu.py sets for these kernels -- and 4 x the float32 error of the same formula on the same inputs,
measured on the CPU against the float64 reference two ways (torch's blocked float32 ops; one term at a time) by
tests/test_head_ref_cpu.py, which also asserts that those figures stay under a quarter of each constant.  The factor
4: the kernels sum in yet another order (per-thread runs, then a fixed tree), and the two CPU orders already differ
from each other by up to 10x on long sums.  No bound is taken from a kernel's output."""
import math

import pytest
import torch

import head_ref as R
from u2gnn_hip import _lib
from u2gnn_hip import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 12345.0          # output padding
NAN = float("nan")      # input padding
SEED = 20240611

# bound                  CPU float32 figure on the worst case of the family: blocked / one term at a time
TOL_POOL = 1e-5         # 1.2e-7 / 2.0e-7: pool_fwd at d = 130, graphs of up to 100 entries
TOL_HEAD = 1e-5         # 3.9e-7 / 3.5e-7: head_fwd at d = 200; head_bwd dW at B = 67: 2.0e-7 / 2.2e-7
TOL_CE = 1e-5           # 4.8e-8 / 5.0e-7: the loss at B = 600, C = 10; dscores 1.5e-7 (scores x 30)
TOL_ADAM = 1e-5         # 1.1e-7: p, m, v after three steps at n = 4099 (elementwise: one order only)
TOL_SS = 1e-5           # 4.0e-7 / 1.4e-6: dW_smp at n_rows = 4097; at S = 1025, D = 19: 1.1e-6 / 6.9e-7
TOL_SS_D1024 = 1.5e-5   # 8.7e-7 / 3.6e-6: prob at S = 513, D = 1024 (dW_smp 1.3e-6 / 3.3e-6); 4 x 3.6e-6
TOL_SUM = 1e-5          # 4.9e-8 / 1.6e-6: n = 4097
TOL_DROP = 1e-5         # 5.2e-8: concat_dropout / split_dropout_bwd (one product per element)
TOL_SQNORM = 2.0 ** -22  # double accumulation, one rounding to float: nothing measured
# every logit near 100 (S = 513, D = 9): one float32 ulp of a logit is 7.6e-6 of a probability, and column 0 of dX is
# 100 (sum_j p_j - 1), of which float32 keeps three digits.  CPU float32, both orders alike:
#                      loss 1.9e-6, prob 1.10e-5, dX 3.33e-4, dW 4.9e-7, dW_lab 2.3e-8, dW_smp 4.8e-6
TOL_SS_SHIFTED = dict(loss=1e-5, prob=4.6e-5, dX=1.4e-3, dW=1e-5, dW_lab=1e-5, dW_smp=2.0e-5)


def dev(t):
    return t.to(DEV)


def padded(t, ld, fill, rows=None):
    """t [r, c] as the leading columns of a [rows or r, ld] device buffer filled with ``fill``."""
    out = torch.full((t.shape[0] if rows is None else rows, ld), fill, dtype=t.dtype)
    out[:t.shape[0], :t.shape[1]] = t
    return out.to(DEV)


def guarded(n, fill=SENT, guard=8, dtype=torch.float32):
    """A device buffer of n + guard elements, all ``fill``: the kernel owns [:n]."""
    return torch.full((n + guard,), fill, dtype=dtype, device=DEV)


def untouched(region, fill=SENT):
    return torch.equal(region, torch.full_like(region, fill))


def close(got, ref, tol, what=""):
    e = R.rel_err(got, ref)
    print(f"{what} rel_err {e:.3g} (bound {tol:.3g})")
    return bool(torch.isfinite(torch.as_tensor(got)).all()) and e < tol


# ----------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------
POOL_D = [1, 63, 64, 65, 130]


def _mask(rows, cols, p):
    return K.dropout_mask(SEED, rows, cols, p).cpu().bool() if p > 0 else None


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("d", POOL_D)
def test_pool_fwd(d, p):
    c = R.pool_case(d)
    B, ld = c["B"], R.rup(d, 64) + 64
    X = padded(c["X"], ld, NAN)
    G = torch.full((B, ld), SENT, device=DEV)
    K.pool_fwd(X, ld, dev(c["rowptr"]), dev(c["colidx"]), dev(c["vals"]), G, ld, B, d, p, SEED)
    G = G.cpu()
    mask = _mask(B, d, p)
    ref = R.pool_fwd(c["X"], c["rowptr"], c["colidx"], c["vals"], d, mask, p)
    assert close(G[:, :d], ref, TOL_POOL, "G")
    assert untouched(G[:, d:])
    assert torch.equal(G[1, :d], torch.zeros(d))            # the empty graph
    if p > 0:
        assert (G[:, :d][~mask] == 0).all()


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("d", POOL_D)
def test_pool_bwd(d, p):
    c = R.pool_case(d)
    B, N, ld = c["B"], c["N"], R.rup(d, 64) + 64
    dG = padded(c["dG"], ld, NAN)
    dX = torch.zeros(N, ld, device=DEV)
    K.pool_bwd(dG, ld, dev(c["rowptr"]), dev(c["colidx"]), dev(c["vals"]), dX, ld, B, d, p, SEED)
    dX = dX.cpu()
    ref = R.pool_bwd(c["dG"], c["rowptr"], c["colidx"], c["vals"], N, d, _mask(B, d, p), p)
    assert close(dX[:, :d], ref, TOL_POOL, "dX")
    assert untouched(dX[:, d:], 0.0)
    assert (dX[:, :d][ref == 0] == 0).all()                  # rows no entry names, dropped columns


@pytest.mark.parametrize("d", [1, 65, 130])
def test_pool_bwd_uses_the_forward_mask(d):
    """dG = 1, vals = 1, identity colidx: a row's gradient is mask / (1 - p) of its graph, and the forward of X = 1
    under the same seed is zero exactly where the mask is."""
    p = 0.3
    c = R.pool_case(d)
    B, N, rowptr = c["B"], c["N"], c["rowptr"]
    ones, col = torch.ones(N, device=DEV), torch.arange(N, device=DEV)
    G = torch.full((B, d), NAN, device=DEV)
    K.pool_fwd(torch.ones(N, d, device=DEV), d, dev(rowptr), col, ones, G, d, B, d, p, SEED)
    dX = torch.zeros(N, d, device=DEV)
    K.pool_bwd(torch.ones(B, d, device=DEV), d, dev(rowptr), col, ones, dX, d, B, d, p, SEED)
    dXr = torch.full((N, d), NAN, device=DEV)
    K.pool_bwd_rows(torch.ones(B, d, device=DEV), d, dev(rowptr), col, ones, dXr, d, B, d, d, N, N, p, SEED)
    mask = _mask(B, d, p)
    lens = rowptr[1:] - rowptr[:-1]
    gid = torch.repeat_interleave(torch.arange(B), lens)
    want = torch.where(mask, 1.0 / (1.0 - p), 0.0).double()
    assert torch.equal(G.cpu()[lens > 0] != 0, mask[lens > 0])
    assert close(G.cpu(), want * lens[:, None], TOL_POOL, "G")
    for got in (dX.cpu(), dXr.cpu()):
        assert torch.equal(got != 0, mask[gid])
        assert close(got, want[gid], TOL_POOL, "dX")


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("d,d_pad,ldx", [(65, 65, 129), (10, 64, 128), (130, 192, 256)])
@pytest.mark.parametrize("pad_rows", [0, 1, 32, 33])       # 0, 1, 1 and 2 blocks of padding rows
def test_pool_bwd_rows(pad_rows, d, d_pad, ldx, p):
    c = R.pool_case(d, distinct=True)
    B, N = c["B"], c["N"]
    Np, ldg = N + pad_rows, d + 3
    dG = padded(c["dG"], ldg, NAN)
    args = (dev(c["rowptr"]), dev(c["colidx"]), dev(c["vals"]))
    dX = torch.full((Np, ldx), NAN, device=DEV)
    dX[:, d_pad:] = SENT
    K.pool_bwd_rows(dG, ldg, *args, dX, ldx, B, d, d_pad, N, Np, p, SEED)
    acc = torch.zeros(Np, ldx, device=DEV)
    K.pool_bwd(dG, ldg, *args, acc, ldx, B, d, p, SEED)
    dX, acc = dX.cpu(), acc.cpu()
    ref = R.pool_bwd(c["dG"], c["rowptr"], c["colidx"], c["vals"], N, d, _mask(B, d, p), p)
    assert close(dX[:N, :d], ref, TOL_POOL, "dX")
    assert untouched(dX[:, d_pad:])
    assert untouched(dX[:, d:d_pad], 0.0) and untouched(dX[N:, :d_pad], 0.0)
    assert torch.equal(dX[:, :d_pad], acc[:, :d_pad])


# ----------------------------------------------------------------------------------------------------------------
# head
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,C", [(1, 2), (3, 3), (5, 10), (64, 2)])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 200])
def test_head_fwd(d, B, C, accumulate):
    c = R.head_case(B, C, d)
    ldg = d + 3
    sc = guarded(B * C)
    sc[:B * C] = dev(c["old"]).flatten() if accumulate else NAN
    K.head_fwd(padded(c["G"], ldg, NAN), ldg, dev(c["W"]), dev(c["bias"]), sc, B, C, d, accumulate)
    sc = sc.cpu()
    ref = R.head_fwd(c["G"], c["W"], c["bias"], d, c["old"] if accumulate else None)
    assert close(sc[:B * C].view(B, C), ref, TOL_HEAD, "scores")
    assert untouched(sc[B * C:])


# the thread ranges [0, B d), [B d, B d + C d), [B d + C d, B d + C d + C): in one block (C = 3, d = 10, small B),
# across blocks (C = 7, d = 65), and with boundaries on multiples of 256 (C = 4, d = 64: B d = 256 at B = 4)
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("C,d", [(3, 10), (7, 65), (4, 64)])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 15, 16, 17, 20, 35, 67])
def test_head_bwd(B, C, d, accumulate):
    c = R.head_case(B, C, d)
    ldg, lddg = d + 5, d + 3
    dG = torch.full((B, lddg), SENT, device=DEV)
    dG[:, :d] = NAN
    dW, db = guarded(C * d), guarded(C)
    dW[:C * d] = dev(c["dW0"]).flatten() if accumulate else NAN
    db[:C] = dev(c["db0"]) if accumulate else NAN
    K.head_bwd(dev(c["dS"]), padded(c["G"], ldg, NAN), ldg, dev(c["W"]), dG, lddg, dW, db, B, C, d, accumulate)
    dG, dW, db = dG.cpu(), dW.cpu(), db.cpu()
    rG, rW, rb = R.head_bwd(c["dS"], c["G"], c["W"], d)
    if accumulate:
        rW, rb = rW + c["dW0"].double(), rb + c["db0"].double()
    assert close(dG[:, :d], rG, TOL_HEAD, "dG")
    assert close(dW[:C * d].view(C, d), rW, TOL_HEAD, "dW")
    assert close(db[:C], rb, TOL_HEAD, "db")
    assert untouched(dG[:, d:]) and untouched(dW[C * d:]) and untouched(db[C:])


# ----------------------------------------------------------------------------------------------------------------
# label-smoothed cross-entropy
# ----------------------------------------------------------------------------------------------------------------
def _check_ce(scores, labels, smoothing):
    B, C = scores.shape
    loss, ds = guarded(1), guarded(B * C)
    K.smoothed_ce(dev(scores), dev(labels), B, C, smoothing, loss, ds)
    loss, ds = loss.cpu(), ds.cpu()
    rl, rd = R.smoothed_ce(scores, labels, smoothing)
    assert close(loss[:1], rl.reshape(1), TOL_CE, "loss")
    assert close(ds[:B * C].view(B, C), rd, TOL_CE, "dscores")
    assert untouched(loss[1:]) and untouched(ds[B * C:])


@pytest.mark.parametrize("smoothing", [0.1, 0.0])
@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_smoothed_ce(B, C, smoothing):
    _check_ce(*R.ce_case(B, C), smoothing)


@pytest.mark.parametrize("B,C", [(257, 3), (600, 10)])
@pytest.mark.parametrize("kind", ["equal", "scaled", "spike"])
def test_smoothed_ce_hard_inputs(kind, B, C):
    _check_ce(*R.ce_case(B, C, kind), 0.1)


# ----------------------------------------------------------------------------------------------------------------
# sqnorm, Adam
# ----------------------------------------------------------------------------------------------------------------
def _sq_blocks(n):
    return max(1, min(512, -(-n // 4096)))   # sqnorm_blocks() of head_ops.hip; ws holds 512 doubles


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8197, 2_097_157, 3_000_001])
def test_sqnorm(n):
    g = R.sqnorm_case(n)
    ref = (g.double() ** 2).sum().item()
    gd = dev(g)
    for partials in (False, True):
        ws, out = guarded(1024, guard=0), guarded(1)
        if partials:
            K.sqnorm_partials(gd, n, ws)
        else:
            K.sqnorm(gd, n, ws, out)
        nb = _sq_blocks(n)
        got = ws.view(torch.float64)[:nb].sum().item() if partials else out[0].item()
        print(f"n={n} partials={partials} rel_err {abs(got - ref) / ref:.3g}")
        assert abs(got - ref) <= TOL_SQNORM * ref
        assert untouched(ws[2 * nb:]) and untouched(out[0 if partials else 1:])


def test_sqnorm_refuses_misaligned_g():
    n = 4097
    g = dev(R.sqnorm_case(n + 1))[1:]
    assert g.data_ptr() % 16 == 4
    for fn in (K.sqnorm, K.sqnorm_partials):
        ws, out = guarded(1024, guard=0), guarded(1)
        with pytest.raises(_lib.U2GNNNativeError):
            fn(g, n, ws, out) if fn is K.sqnorm else fn(g, n, ws)
        torch.cuda.synchronize()
        assert untouched(ws) and untouched(out)


B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 0.01
GUARD = 8


def _buf(x, offset):
    """x in a device allocation of offset + n + GUARD floats (the rest SENT); returns (allocation, the view)."""
    n = x.numel()
    full = torch.full((offset + n + GUARD,), SENT, device=DEV)
    full[offset:offset + n] = dev(x)
    view = full[offset:offset + n]
    assert full.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * offset
    return full, view


def _run_adam(param, grads, max_norm, offsets, clip=True):
    """Three steps of sqnorm + adam; offsets = (param, grad, m, v) offsets in floats.  Returns (p, m, v) on the CPU."""
    n = param.numel()
    zeros = torch.zeros(n)
    (fp, p), (fm, m), (fv, v) = _buf(param, offsets[0]), _buf(zeros, offsets[2]), _buf(zeros, offsets[3])
    ws, sq = torch.empty(1024, device=DEV), torch.empty(1, device=DEV)
    for t, g in enumerate(grads, 1):
        K.sqnorm(dev(g), n, ws, sq)
        fg, gv = _buf(g, offsets[1])
        K.adam(p, gv, m, v, n, sq if clip else None, max_norm, B1, B2, EPS, LR / (1 - B1 ** t),
               math.sqrt(1 - B2 ** t))
        assert torch.equal(fg.cpu(), _buf(g, offsets[1])[0].cpu())      # the gradient is read only
    for full, off in ((fp, offsets[0]), (fm, offsets[2]), (fv, offsets[3])):
        assert untouched(full[:off]) and untouched(full[off + n:])
    return p.cpu(), m.cpu(), v.cpu()


def _ref_adam(param, grads, max_norm):
    p, m, v = param, torch.zeros_like(param), torch.zeros_like(param)
    sq = None
    for t, g in enumerate(grads, 1):
        p, m, v, sq = R.clip_adam(p, g, m, v, max_norm, B1, B2, EPS, LR, t)
    return p, m, v, sq


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_adam(n, clipped):
    """The float4 path (all four buffers 16-byte aligned) against float64, and the scalar path (all four buffers
    offset by one float; only v offset) against the float4 path bit for bit: head_ops.hip promises the same
    per-element arithmetic on both."""
    param, grads, max_norm = R.adam_case(n, clipped)
    ref = _ref_adam(param, grads, max_norm)
    aligned = _run_adam(param, grads, max_norm, (0, 0, 0, 0))
    for got, want, what in zip(aligned, ref, "pmv"):
        assert close(got, want, TOL_ADAM, what)
    for offsets in ((1, 1, 1, 1), (0, 0, 0, 1)):
        other = _run_adam(param, grads, max_norm, offsets)
        for a, b, what in zip(aligned, other, "pmv"):
            assert torch.equal(a, b), f"{what}: offsets {offsets} differ from the float4 path"
    if not clipped:
        # |g| < max_norm: the coefficient is exactly 1, the same bits as without a norm
        for offsets in ((0, 0, 0, 0), (1, 1, 1, 1)):
            noclip = _run_adam(param, grads, max_norm, offsets, clip=False)
            for a, b in zip(aligned, noclip):
                assert torch.equal(a, b)
        unclipped_ref = _ref_adam(param, grads, None)
        assert torch.equal(ref[0], unclipped_ref[0])


@pytest.mark.parametrize("form", ["adam_sq", "adam_dev_sq", "adam_dev"])
@pytest.mark.parametrize("n", [5, 4097, 2_097_157])
def test_adam_fused_forms(n, form):
    """adam_sq / adam_dev_sq (the sqnorm partials folded in the Adam launch) and adam_dev (bias corrections from the
    device-resident lr and step) against float64 -- not against the unfused path -- at steps t = 1, 2, 3."""
    param, grads, max_norm = R.adam_case(n, True)
    (fp, p), (fm, m), (fv, v) = (_buf(x, 0) for x in (param, torch.zeros(n), torch.zeros(n)))
    lr_dev = torch.tensor([LR], dtype=torch.float64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    rp, rm, rv = param, torch.zeros(n), torch.zeros(n)
    for t, g in enumerate(grads, 1):
        gd = dev(g)
        ws, sq = guarded(1024, guard=0), guarded(1)
        step.fill_(t)                       # a _dev form is never called with t == 0
        if form == "adam_dev":
            K.sqnorm(gd, n, ws, sq)
            K.adam_dev(p, gd, m, v, n, sq, max_norm, B1, B2, EPS, lr_dev, step)
        else:
            K.sqnorm_partials(gd, n, ws)
            if form == "adam_sq":
                K.adam_sq(p, gd, m, v, n, ws, sq, max_norm, B1, B2, EPS, LR / (1 - B1 ** t), math.sqrt(1 - B2 ** t))
            else:
                K.adam_dev_sq(p, gd, m, v, n, ws, sq, max_norm, B1, B2, EPS, lr_dev, step)
        rp, rm, rv, rsq = R.clip_adam(rp, g, rm, rv, max_norm, B1, B2, EPS, LR, t)
        assert abs(sq[0].item() - rsq.item()) <= TOL_SQNORM * rsq.item()
        assert untouched(sq[1:]) and untouched(ws[2 * _sq_blocks(n):])
        for got, want, what in ((p, rp, "p"), (m, rm, "m"), (v, rv, "v")):
            assert close(got, want, TOL_ADAM, f"t={t} {what}")
    for full in (fp, fm, fv):
        assert untouched(full[n:])
    assert step.item() == 3 and lr_dev.item() == LR


# ----------------------------------------------------------------------------------------------------------------
# sampled softmax
# ----------------------------------------------------------------------------------------------------------------
SS_GRID = [(S, D, 37) for S in (1, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769, 1025) for D in (1, 7, 8, 9, 19)]
SS_WIDE = [(513, D, 37) for D in (16, 17, 100, 1024)]
SS_ROWS = [(5, 9, n) for n in (1, 255, 256, 257, 1792, 1793, 2048, 2049, 4097)]   # the eight-row unroll's edges


def _check_ss(S, D, n, shifted, tol):
    c = R.ss_case(S, D, n, shifted)
    tol = tol if isinstance(tol, dict) else dict.fromkeys(("loss", "prob", "dX", "dW", "dW_lab", "dW_smp"), tol)
    V, ldx, ldw, lddx, lddw, ldl, lds = R.SS_V, D + 3, D + 5, D + 2, D + 1, D + 4, D + 6
    X, W = padded(c["X"], ldx, NAN), padded(c["W"], ldw, NAN)
    labels, sids = dev(c["labels"]), dev(c["sids"])
    loss, prob = guarded(n), guarded(n * S)
    K.sampled_softmax_fwd(X, ldx, labels, sids, S, W, ldw, loss, prob, n, D)
    lo, pr = loss.cpu(), prob.cpu()
    assert untouched(lo[n:]) and untouched(pr[n * S:])
    pr = pr[:n * S].view(n, S)
    ref = R.sampled_softmax(c["X"], c["labels"], c["sids"], c["W"], None)
    assert close(lo[:n], ref["loss"], tol["loss"], "loss")
    assert close(pr, ref["prob"], tol["prob"], "prob")
    assert close(pr.double().sum(1), torch.ones(n), tol["prob"], "prob rows sum")
    touched = torch.zeros(V, dtype=torch.bool)
    touched[c["labels"]] = True
    touched[c["sids"]] = True
    for dloss in (None, c["dloss"]):
        if dloss is not None:
            ref = R.sampled_softmax(c["X"], c["labels"], c["sids"], c["W"], dloss)
        dl = None if dloss is None else dev(dloss)
        # dense: atomics onto a zero-filled dW
        dX = torch.full((n, lddx), SENT, device=DEV)
        dW = torch.full((V, lddw), SENT, device=DEV)
        dW[:, :D] = 0
        K.sampled_softmax_bwd(X, ldx, labels, sids, S, W, ldw, prob, dl, dX, lddx, dW, lddw, n, D)
        dX, dW = dX.cpu(), dW.cpu()
        assert close(dX[:, :D], ref["dX"], tol["dX"], "dX")
        assert close(dW[:, :D], ref["dW"], tol["dW"], "dW")
        assert untouched(dX[:, D:]) and untouched(dW[:, D:])
        assert untouched(dW[:, :D][~touched], 0.0)
        # compact rows: plain stores
        dX2 = torch.full((n, lddx), SENT, device=DEV)
        lab, smp = torch.full((n, ldl), SENT, device=DEV), torch.full((S, lds), SENT, device=DEV)
        K.sampled_softmax_bwd_rows(X, ldx, labels, sids, S, W, ldw, prob, dl, dX2, lddx, lab[:, :D], smp[:, :D], n, D)
        dX2, lab, smp = dX2.cpu(), lab.cpu(), smp.cpu()
        assert torch.equal(dX2, dX)
        assert close(lab[:, :D], ref["dW_lab"], tol["dW_lab"], "dW_lab")
        assert close(smp[:, :D], ref["dW_smp"], tol["dW_smp"], "dW_smp")
        assert untouched(lab[:, D:]) and untouched(smp[:, D:])


@pytest.mark.parametrize("S,D,n", SS_GRID + SS_WIDE + SS_ROWS)
def test_sampled_softmax(S, D, n):
    """S <= 192 leaves at least one wave of the forward without a sample (the -inf of the online max); S > 512 takes
    the sids[j] path; odd multiples of 256 leave the two-sample loop a remainder; D = 7, 9, 17, 19, 100: a partial
    last 8-column pass; n > 1792: the eight-row unroll."""
    _check_ss(S, D, n, False, TOL_SS_D1024 if D == 1024 else TOL_SS)


def test_sampled_softmax_shifted_logits():
    """X[:, 0] = 1, W[:, 0] = 100: every logit near 100, where exp overflows float32 without the max subtraction."""
    _check_ss(513, 9, 37, True, TOL_SS_SHIFTED)


# ----------------------------------------------------------------------------------------------------------------
# row helpers and small reductions
# ----------------------------------------------------------------------------------------------------------------
ROWS_D = [1, 63, 64, 65, 130]
DST_ROWS = 13


def _rows_case(D, n_rows, seed=0):
    g = torch.Generator().manual_seed(8000 + seed)
    return (torch.randn(n_rows, D, generator=g), torch.randn(DST_ROWS, D, generator=g),
            torch.randperm(DST_ROWS, generator=g)[:n_rows])


@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("D", ROWS_D)
def test_index_add_and_zero_rows(D, n_rows, alpha):
    src, dst0, idx = _rows_case(D, n_rows)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    dst = padded(dst0, D + 3, SENT)
    K.index_add_rows(padded(src, D + 2, NAN), dev(idx), dst[:, :D], alpha, err)
    ref = dst0.clone()
    ref[idx] += alpha * src                   # one product and one sum per element: float32 is the exact statement
    got = dst.cpu()
    assert torch.equal(got[:, :D], ref) and untouched(got[:, D:])
    K.index_zero_rows(dev(idx), dst[:, :D], err)
    ref[idx] = 0
    got = dst.cpu()
    assert torch.equal(got[:, :D], ref) and untouched(got[:, D:])
    assert err.item() == 0


@pytest.mark.parametrize("D", ROWS_D)
def test_index_rows_skip_bad_indices(D):
    """A negative index and one equal to dst_rows set err and are skipped; the other rows are done."""
    src, dst0, _ = _rows_case(D, 5, seed=1)
    idx = torch.tensor([-1, 2, DST_ROWS, 0, 7])
    ok = torch.tensor([1, 3, 4])
    dst = padded(dst0, D + 3, SENT)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.index_add_rows(padded(src, D + 2, NAN), dev(idx), dst[:, :D], -0.5, err)
    ref = dst0.clone()
    ref[idx[ok]] += -0.5 * src[ok]
    got = dst.cpu()
    assert err.item() == 1 and torch.equal(got[:, :D], ref) and untouched(got[:, D:])
    for fn in ("zero", "zero2"):
        dst = padded(dst0, D + 3, SENT)
        err.zero_()
        if fn == "zero":
            K.index_zero_rows(dev(idx), dst[:, :D], err)
        else:
            K.index_zero_rows2(dev(idx[:2]), dev(idx[2:]), dst[:, :D], err)
        ref = dst0.clone()
        ref[idx[ok]] = 0
        got = dst.cpu()
        assert err.item() == 1 and torch.equal(got[:, :D], ref) and untouched(got[:, D:])


@pytest.mark.parametrize("D", [1, 65])
@pytest.mark.parametrize("empty", ["first", "second", "both"])
def test_index_zero_rows2_with_an_empty_list(empty, D):
    _, dst0, idx = _rows_case(D, 9, seed=2)
    none = torch.empty(0, dtype=torch.int64)
    a, b = {"first": (none, idx), "second": (idx, none), "both": (none, none)}[empty]
    dst = padded(dst0, D + 3, SENT)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.index_zero_rows2(dev(a), dev(b), dst[:, :D], err)
    ref = dst0.clone()
    ref[torch.cat([a, b])] = 0
    got = dst.cpu()
    assert err.item() == 0 and torch.equal(got[:, :D], ref) and untouched(got[:, D:])


@pytest.mark.parametrize("n", [1023, 1024, 1025, 4095, 4096, 4097])
def test_sum_all(n):
    x = R.sum_case(n)
    xd = torch.full((n + GUARD,), NAN, device=DEV)
    xd[:n] = dev(x)
    out = guarded(1)
    K.sum_all(xd, n, out)
    out = out.cpu()
    assert close(out[:1], x.double().sum().reshape(1), TOL_SUM, "sum") and untouched(out[1:])


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("d", [4, 19])
@pytest.mark.parametrize("L", [1, 3, 8])
def test_concat_and_split_dropout(L, d, p):
    """Against dropout_mask and plain indexing (tests/test_kernels_gpu.py compares them with other kernels)."""
    N, Np, dp, D = 300, 320, 64, d * L
    g = torch.Generator().manual_seed(9000)
    srcs = [torch.randn(N, d, generator=g) for _ in range(L)]
    mask = K.dropout_mask(SEED, N, D, p).cpu().bool() if p > 0 else torch.ones(N, D, dtype=torch.bool)
    ldy = D + 3
    Y = torch.full((N, ldy), SENT, device=DEV)
    K.concat_dropout([padded(s, dp, NAN, rows=Np) for s in srcs], dp, N, d, Y, ldy, p, SEED)
    Y = Y.cpu()
    cat = torch.cat(srcs, 1)
    ref = torch.where(mask, cat.double() / (1.0 - p), 0.0)
    assert untouched(Y[:, D:]) and (Y[:, :D][~mask] == 0).all()
    assert torch.equal(Y[:, :D], cat) if p == 0 else close(Y[:, :D], ref, TOL_DROP, "Y")
    dY = torch.randn(N, D, generator=g)
    dsts = [torch.full((Np * dp + GUARD,), SENT, device=DEV) for _ in range(L)]
    dsts[0][:Np * dp] = NAN
    K.split_dropout_bwd(padded(dY, ldy, NAN), ldy, N, Np, d, dp, p, SEED, dsts)
    rd = torch.where(mask, dY.double() / (1.0 - p), 0.0)
    for l, t in enumerate(dsts):
        t = t.cpu()
        img = t[:Np * dp].view(Np, dp)
        assert untouched(t[Np * dp:]) and untouched(img[N:], 0.0) and untouched(img[:, d:], 0.0)
        assert (img[:N, :d][~mask[:, l * d:(l + 1) * d]] == 0).all()
        if p == 0:
            assert torch.equal(img[:N, :d], dY[:, l * d:(l + 1) * d])
        else:
            assert close(img[:N, :d], rd[:, l * d:(l + 1) * d], TOL_DROP, f"dst {l}")


def test_concat_and_split_dropout_refuse_nine_layers():
    N, d, dp = 10, 4, 64
    srcs = [torch.zeros(N, dp, device=DEV) for _ in range(9)]
    Y = torch.full((N, 9 * d), SENT, device=DEV)
    with pytest.raises(_lib.U2GNNNativeError):
        K.concat_dropout(srcs, dp, N, d, Y, 9 * d, 0.3, SEED)
    with pytest.raises(_lib.U2GNNNativeError):
        K.split_dropout_bwd(Y, 9 * d, N, N, d, dp, 0.3, SEED, srcs)
    torch.cuda.synchronize()
    assert untouched(Y) and all(untouched(s, 0.0) for s in srcs)
