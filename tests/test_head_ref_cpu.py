"""tests/head_ref.py checked without a GPU: each float64 reference against an independent statement of the same
operation (the oracle, torch.optim, torch.autograd, a dense pool matrix), and the tolerance table of
tests/test_head_kernels_gpu.py: the float32 error of each formula on the inputs the kernels see, computed here two
ways (torch's blocked float32 ops; one term at a time) against the float64 reference, must stay under a quarter of
the bound the GPU tests assert."""
import math

import pytest
import torch

import head_ref as R
import test_head_kernels_gpu as T
from oracle import u2gnn_oracle as O

F64 = torch.float64
EXACT = 1e-12     # two float64 statements of one formula


def _f64_default(fn):
    """Run fn with float64 as torch's default dtype (the oracle builds its targets in the default dtype)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(old)


# ----------------------------------------------------------------------------------------------------------------
# the references against independent statements
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_pool_against_a_dense_pool_matrix(p):
    d = 65
    c = R.pool_case(d)
    B, N = c["B"], c["N"]
    P = torch.zeros(B, N, dtype=F64)
    for b in range(B):
        for e in range(int(c["rowptr"][b]), int(c["rowptr"][b + 1])):
            P[b, c["colidx"][e]] += c["vals"][e].double()
    mask = torch.rand(B, d, generator=torch.Generator().manual_seed(1)) >= p
    keep = mask.double() / (1 - p) if p > 0 else torch.ones(B, d, dtype=F64)
    x = c["X"].double().requires_grad_(True)
    G = (P @ x) * keep
    assert R.rel_err(R.pool_fwd(c["X"], c["rowptr"], c["colidx"], c["vals"], d, mask, p), G.detach()) < EXACT
    (G * c["dG"].double()).sum().backward()
    assert R.rel_err(R.pool_bwd(c["dG"], c["rowptr"], c["colidx"], c["vals"], N, d, mask, p), x.grad) < EXACT
    assert R.rel_err(R.pool_fwd_seq(c["X"], c["rowptr"], c["colidx"], c["vals"], d, mask, p), G.detach()) < 1e-5
    lens = c["rowptr"][1:] - c["rowptr"][:-1]
    assert sorted(lens.tolist()) == [0, 1, 8, 24, 25, 32, 33, 57, 64, 75, 100]
    assert c["colidx"].unique().numel() < N                   # repeated rows: atomics on one address
    assert R.pool_case(d, distinct=True)["colidx"].unique().numel() == N


def test_head_against_autograd():
    B, C, d = 17, 7, 65
    c = R.head_case(B, C, d)
    G, W, b = (c[k].double().requires_grad_(True) for k in ("G", "W", "bias"))
    s = torch.nn.functional.linear(G, W, b) + c["old"].double()
    assert R.rel_err(R.head_fwd(c["G"], c["W"], c["bias"], d, c["old"]), s.detach()) < EXACT
    s.backward(c["dS"].double())
    for got, want in zip(R.head_bwd(c["dS"], c["G"], c["W"], d), (G.grad, W.grad, b.grad)):
        assert R.rel_err(got, want) < EXACT
    wide = torch.cat([c["G"], torch.full((B, 3), float("nan"))], 1)      # columns past d are not read
    assert torch.equal(R.head_fwd(wide, c["W"], c["bias"], d), R.head_fwd(c["G"], c["W"], c["bias"], d))


@pytest.mark.parametrize("smoothing", [0.1, 0.0])
@pytest.mark.parametrize("kind", ["plain", "equal", "scaled", "spike"])
def test_smoothed_ce_against_the_oracle(kind, smoothing):
    scores, labels = R.ce_case(257, 3, kind)
    loss, ds = R.smoothed_ce(scores, labels, smoothing)
    s = scores.double().requires_grad_(True)
    want = _f64_default(lambda: O.soft_cross_entropy(s, O.label_smoothing(labels, 3, smoothing)))
    want.backward()
    assert want.dtype == F64 and abs(loss.item() - want.item()) <= EXACT * abs(want.item())
    assert R.rel_err(ds, s.grad) < EXACT and bool(torch.isfinite(ds).all())


def test_clip_adam_against_torch_optim_and_the_oracle():
    """Betas that float32 holds exactly, so that the float32 rounding clip_adam applies to them changes nothing."""
    b1, b2, eps, lr, n = 0.875, 1 - 2.0 ** -8, 1e-8, 0.01, 1025
    for clipped in (True, False):
        param, grads, max_norm = R.adam_case(n, clipped)
        tp = param.double().requires_grad_(True)
        opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps)
        op, state = param.double(), {}
        p, m, v = param, torch.zeros(n), torch.zeros(n)
        for t, g in enumerate(grads, 1):
            p, m, v, sq = R.clip_adam(p, g, m, v, max_norm, b1, b2, eps, lr, t)
            tp.grad = g.double()
            total = torch.nn.utils.clip_grad_norm_([tp], max_norm)
            opt.step()
            O.clip_and_adam([op], [g.double()], state, lr, max_norm, (b1, b2), eps)
            assert abs(math.sqrt(sq.item()) - total.item()) <= EXACT * total.item()
            assert (math.sqrt(sq.item()) > 4 * max_norm) if clipped else (math.sqrt(sq.item()) < max_norm)
            assert R.rel_err(p, tp.detach()) < EXACT and R.rel_err(p, op) < EXACT
            st = opt.state[tp]
            assert R.rel_err(m, st["exp_avg"]) < EXACT and R.rel_err(v, st["exp_avg_sq"]) < EXACT
        if not clipped:
            q, m, v = param, torch.zeros(n), torch.zeros(n)
            for t, g in enumerate(grads, 1):
                q, m, v, _ = R.clip_adam(q, g, m, v, None, b1, b2, eps, lr, t)
            assert torch.equal(p, q)


def test_clip_adam_rounds_the_decay_betas_to_float32():
    """With the betas the models use, the decays are the float32 values the native entry points receive."""
    g = torch.ones(4)
    z = torch.zeros(4)
    _, m, v, _ = R.clip_adam(z, g, z, z, None, 0.9, 0.999, 1e-8, 0.01, 1)
    f1, f2 = torch.tensor(0.9).item(), torch.tensor(0.999).item()
    assert m[0].item() == 1 - f1 and v[0].item() == 1 - f2
    assert abs(v[0].item() - 0.001) / 0.001 > 1.2e-5


@pytest.mark.parametrize("use_dloss", [False, True])
def test_sampled_softmax_against_the_oracle(use_dloss):
    c = R.ss_case(65, 9, 37)
    dloss = c["dloss"] if use_dloss else None
    r = R.sampled_softmax(c["X"], c["labels"], c["sids"], c["W"], dloss)
    x, w = c["X"].double().requires_grad_(True), c["W"].double().requires_grad_(True)
    loss = O.sampled_softmax_logits(x, c["labels"], w, c["sids"])
    g = torch.ones(37, dtype=F64) if dloss is None else dloss.double()
    (g * loss).sum().backward()
    assert R.rel_err(r["loss"], loss.detach()) < EXACT
    assert R.rel_err(r["dX"], x.grad) < EXACT and R.rel_err(r["dW"], w.grad) < EXACT
    assert R.rel_err(r["prob"].sum(1), torch.ones(37)) < EXACT
    assert R.rel_err(r["prob"], torch.softmax(x.detach() @ w.detach()[c["sids"]].t(), 1)) < EXACT
    fold = torch.zeros_like(r["dW"])
    fold.index_add_(0, c["labels"], r["dW_lab"])
    fold.index_add_(0, c["sids"], r["dW_smp"])
    assert R.rel_err(fold, r["dW"]) < EXACT
    # the inputs hold what the GPU tests rely on
    assert c["sids"].unique().numel() == 65
    assert torch.isin(c["labels"], c["sids"]).any() and c["labels"].unique().numel() < 37
    assert (c["dloss"] == 0).any() and (c["dloss"] < 0).any()


def test_sampled_softmax_shifted_logits_overflow_a_naive_exp():
    c = R.ss_case(513, 9, 37, shifted=True)
    logits = c["X"] @ c["W"][c["sids"]].t()
    assert logits.min() > 90 and not torch.isfinite(logits.exp()).all()
    r = R.sampled_softmax(c["X"], c["labels"], c["sids"], c["W"], c["dloss"])
    assert all(bool(torch.isfinite(t).all()) for t in r.values())


def test_sqnorm_case_shows_a_dropped_tail_element():
    """Every element of the n % 4 tail moves the total by more than the bound of the GPU test."""
    for n in (1, 3, 5, 4097, 8197, 2_097_157, 3_000_001):
        sq = R.sqnorm_case(n).double() ** 2
        assert n % 4 and (sq[n - n % 4:] > 4 * T.TOL_SQNORM * sq.sum()).all()


# ----------------------------------------------------------------------------------------------------------------
# the tolerance table
# ----------------------------------------------------------------------------------------------------------------
def _both(name, what, blocked, seq, ref, bound, rows):
    eb, es = R.rel_err(blocked, ref), R.rel_err(seq, ref)
    rows.append((name, what, eb, es, bound))
    return max(eb, es)


def _ss_rows(name, label, c, dloss, bound, rows, per_quantity=False):
    ref = R.sampled_softmax(c["X"], c["labels"], c["sids"], c["W"], dloss)
    blk = R.sampled_softmax_f32(c["X"], c["labels"], c["sids"], c["W"], dloss)
    seq = R.sampled_softmax_f32(c["X"], c["labels"], c["sids"], c["W"], dloss, seq=True)
    for k in ref:
        if per_quantity:
            _both(f"{name}[{k}]", label, blk[k], seq[k], ref[k], bound[k], rows)
        else:
            _both(name, f"{label} {k}", blk[k], seq[k], ref[k], bound, rows)


def _adam_f32(param, grads, max_norm, b1, b2, eps, lr):
    p, m, v = param, torch.zeros_like(param), torch.zeros_like(param)
    for t, g in enumerate(grads, 1):
        p, m, v, _ = R.clip_adam(p, g, m, v, max_norm, b1, b2, eps, lr, t, dtype=torch.float32)
    return p, m, v


@pytest.fixture(scope="module")
def table():
    rows = []
    # pooling: the widest d, graphs of up to 100 entries
    c = R.pool_case(130)
    a = (c["X"], c["rowptr"], c["colidx"], c["vals"], 130)
    _both("TOL_POOL", "pool_fwd d=130", R.pool_fwd(*a, dtype=torch.float32), R.pool_fwd_seq(*a), R.pool_fwd(*a),
          T.TOL_POOL, rows)
    b = (c["dG"], c["rowptr"], c["colidx"], c["vals"], c["N"], 130)
    f = R.pool_bwd(*b, dtype=torch.float32)
    _both("TOL_POOL", "pool_bwd d=130", f, f, R.pool_bwd(*b), T.TOL_POOL, rows)
    # head: the longest dot product (d = 200) and the longest batch sums (B = 67)
    c = R.head_case(64, 2, 200)
    _both("TOL_HEAD", "head_fwd d=200", R.head_fwd(c["G"], c["W"], c["bias"], 200, c["old"], torch.float32),
          R.head_fwd_seq(c["G"], c["W"], c["bias"], 200) + c["old"], R.head_fwd(c["G"], c["W"], c["bias"], 200, c["old"]),
          T.TOL_HEAD, rows)
    c = R.head_case(67, 7, 65)
    ref = R.head_bwd(c["dS"], c["G"], c["W"], 65)
    blk, seq = R.head_bwd(c["dS"], c["G"], c["W"], 65, torch.float32), R.head_bwd_seq(c["dS"], c["G"], c["W"], 65)
    for k, what in enumerate(("dG", "dW", "db")):
        _both("TOL_HEAD", f"head_bwd B=67 {what}", blk[k], seq[k], ref[k], T.TOL_HEAD, rows)
    # cross-entropy: the longest batch, plain and hard inputs
    for kind in ("plain", "equal", "scaled", "spike"):
        s, y = R.ce_case(600, 10, kind)
        ref, blk, seq = R.smoothed_ce(s, y, 0.1), R.smoothed_ce_f32(s, y, 0.1), R.smoothed_ce_f32(s, y, 0.1, True)
        _both("TOL_CE", f"ce B=600 {kind} loss", blk[0], seq[0], ref[0], T.TOL_CE, rows)
        _both("TOL_CE", f"ce B=600 {kind} dscores", blk[1], seq[1], ref[1], T.TOL_CE, rows)
    # Adam: elementwise, one order
    for clipped in (True, False):
        param, grads, mn = R.adam_case(4099, clipped)
        hp = (T.B1, T.B2, T.EPS, T.LR)
        ref, f = T._ref_adam(param, grads, mn), _adam_f32(param, grads, mn, *hp)
        for k, what in enumerate("pmv"):
            _both("TOL_ADAM", f"adam n=4099 clipped={clipped} {what}", f[k], f[k], ref[k], T.TOL_ADAM, rows)
    # sampled softmax: the longest sums over S, D and n_rows
    for S, D, n in ((1025, 19, 37), (513, 100, 37), (5, 9, 4097), (513, 1024, 37)):
        c = R.ss_case(S, D, n)
        name = "TOL_SS_D1024" if D == 1024 else "TOL_SS"
        _ss_rows(name, f"ss S={S} D={D} n={n}", c, c["dloss"], getattr(T, name), rows)
    c = R.ss_case(513, 9, 37, shifted=True)
    _ss_rows("TOL_SS_SHIFTED", "ss shifted S=513 D=9 n=37", c, c["dloss"], T.TOL_SS_SHIFTED, rows, per_quantity=True)
    # sum_all
    x = R.sum_case(4097)
    _both("TOL_SUM", "sum n=4097", x.sum(), R.seq_sum(x), x.double().sum(), T.TOL_SUM, rows)
    # concat / split dropout: one product per element
    x = torch.randn(300, 152, generator=torch.Generator().manual_seed(9000))
    f = x * (1.0 / (1.0 - 0.3))
    _both("TOL_DROP", "x / (1 - p)", f, f, x.double() / (1.0 - 0.3), T.TOL_DROP, rows)
    return rows


def test_float32_baselines_stay_under_a_quarter_of_each_bound(table):
    worst, bounds = {}, {}
    for name, what, eb, es, bound in table:
        print(f"{name:24s} {what:36s} blocked {eb:.3e}  sequential {es:.3e}  bound {bound:.2e}")
        worst[name] = max(worst.get(name, 0.0), eb, es)
        bounds[name] = bound
    for name, e in worst.items():
        print(f"{name}: worst float32 figure {e:.3e}, bound {bounds[name]:.2e}")
        assert 4 * e <= bounds[name], name
        # a bound above the 1e-5 bar is what the measurement calls for and no more (rounded up by under a tenth)
        assert bounds[name] == 1e-5 or bounds[name] <= 4.4 * e, name
    assert {n.split("[")[0] for n in worst} == {n for n in dir(T) if n.startswith("TOL_")} - {"TOL_SQNORM"}
    assert {n for n in worst if "[" in n} == {f"TOL_SS_SHIFTED[{k}]" for k in T.TOL_SS_SHIFTED}


def test_f32_restatement_of_the_sampled_softmax_is_the_reference_formula():
    """sampled_softmax_f32 in float64 inputs' place: the explicit gradients agree with autograd to float32 accuracy."""
    c = R.ss_case(257, 8, 37)
    ref = R.sampled_softmax(c["X"], c["labels"], c["sids"], c["W"], c["dloss"])
    for seq in (False, True):
        got = R.sampled_softmax_f32(c["X"], c["labels"], c["sids"], c["W"], c["dloss"], seq)
        for k in ref:
            assert R.rel_err(got[k], ref[k]) < 1e-5, k
