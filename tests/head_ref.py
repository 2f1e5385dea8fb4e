"""Float64 references of the graph-level kernels (csrc/head_ops.hip): sum pooling with dropout, the linear head, the
label-smoothed cross-entropy, clip + Adam, the sampled-softmax loss -- and the inputs the tests of those kernels share.
Test infrastructure only.

Plain torch on the CPU, no project kernels.  Every reference takes float32 inputs and computes in float64; the
gradients of the two losses come from autograd of the float64 loss, not from a hand-written formula.  The ``*_f32``
functions are the same formulas in float32, once with torch's own (blocked) float32 ops and once accumulated one
term at a time: tests/test_head_ref_cpu.py measures both against the float64 reference, and the tolerances of
tests/test_head_kernels_gpu.py are taken from those figures.  The ``*_case`` functions build the inputs, so that the
figures are measured on the inputs the kernels then see.  Nothing here is modified by a test."""
import math

import torch

F64 = torch.float64


def rel_err(got, ref):
    """The project's metric (tests/test_kernels_gpu.py): max|got - ref| / max|ref|."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    if ref.numel() == 0:
        return 0.0
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def rup(x, m):
    return -(-x // m) * m


# ----------------------------------------------------------------------------------------------------------------
# pooling: G[b] = sum_e vals[e] X[colidx[e], :d] over e in [rowptr[b], rowptr[b + 1]), then dropout
# ----------------------------------------------------------------------------------------------------------------
def _drop(G, mask, p):
    if p > 0:
        return torch.where(mask.bool(), G / (1.0 - p), torch.zeros_like(G))
    return G


def pool_fwd(X, rowptr, colidx, vals, d, mask=None, p=0.0, dtype=F64):
    X, vals = X[:, :d].to(dtype), vals.to(dtype)
    B = rowptr.numel() - 1
    G = torch.zeros(B, d, dtype=dtype)
    for b in range(B):
        e0, e1 = int(rowptr[b]), int(rowptr[b + 1])
        if e1 > e0:
            G[b] = (vals[e0:e1, None] * X[colidx[e0:e1]]).sum(0)
    return _drop(G, None if mask is None else mask[:B, :d], p)


def pool_fwd_seq(X, rowptr, colidx, vals, d, mask=None, p=0.0):
    """float32, one entry at a time."""
    X = X[:, :d]
    B = rowptr.numel() - 1
    G = torch.zeros(B, d)
    for b in range(B):
        for e in range(int(rowptr[b]), int(rowptr[b + 1])):
            G[b] += vals[e] * X[colidx[e]]
    return _drop(G, None if mask is None else mask[:B, :d], p)


def pool_bwd(dG, rowptr, colidx, vals, n_rows, d, mask=None, p=0.0, dtype=F64):
    """The transpose: dX[colidx[e], :d] += vals[e] drop(dG)[b]; repeated colidx accumulate."""
    B = rowptr.numel() - 1
    g = _drop(dG[:B, :d].to(dtype), None if mask is None else mask[:B, :d], p)
    dX = torch.zeros(n_rows, d, dtype=dtype)
    for b in range(B):
        e0, e1 = int(rowptr[b]), int(rowptr[b + 1])
        if e1 > e0:
            dX.index_add_(0, colidx[e0:e1], vals[e0:e1, None].to(dtype) * g[b])
    return dX


def pool_case(d, seed=0, lengths=(33, 0, 100, 1, 25, 64, 8, 75, 24, 57, 32), distinct=False):
    """One batch of graphs of ``lengths`` entries (shuffled; an empty graph in the middle).  colidx: a random
    permutation of the rows with every seventh entry repeating an earlier row (``distinct``: a plain permutation,
    every row once: what pool_bwd_rows requires); vals in [0.5, 1.5).  X [n_rows, d]."""
    g = torch.Generator().manual_seed(1000 + seed)
    rowptr = torch.tensor([0] + list(lengths)).cumsum(0)
    N = int(rowptr[-1])
    colidx = torch.randperm(N, generator=g)
    if not distinct:
        rep = torch.arange(6, N, 7)
        colidx[rep] = colidx[rep - 5]
    vals = torch.rand(N, generator=g) + 0.5
    X = torch.randn(N, d, generator=g)
    dG = torch.randn(len(lengths), d, generator=g)
    return dict(rowptr=rowptr, colidx=colidx, vals=vals, X=X, dG=dG, N=N, B=len(lengths))


# ----------------------------------------------------------------------------------------------------------------
# head: scores = G[:, :d] W^T + bias (+ old)
# ----------------------------------------------------------------------------------------------------------------
def head_fwd(G, W, bias, d, old=None, dtype=F64):
    s = G[:, :d].to(dtype) @ W.to(dtype).t() + bias.to(dtype)
    return s if old is None else s + old.to(dtype)


def head_bwd(dS, G, W, d, dtype=F64):
    """(dG, dW, db) of head_fwd under the upstream gradient dS."""
    dS = dS.to(dtype)
    return dS @ W.to(dtype), dS.t() @ G[:, :d].to(dtype), dS.sum(0)


def head_fwd_seq(G, W, bias, d):
    s = torch.zeros(G.shape[0], W.shape[0])
    for j in range(d):
        s += G[:, j, None] * W[None, :, j]
    return s + bias


def head_bwd_seq(dS, G, W, d):
    B, C = dS.shape
    dG, dW, db = torch.zeros(B, d), torch.zeros(C, d), torch.zeros(C)
    for k in range(C):
        dG += dS[:, k, None] * W[None, k]
    for b in range(B):
        dW += dS[b, :, None] * G[b, None, :d]
        db += dS[b]
    return dG, dW, db


def head_case(B, C, d, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return dict(G=torch.randn(B, d, generator=g), W=torch.randn(C, d, generator=g), bias=torch.randn(C, generator=g),
                old=torch.randn(B, C, generator=g), dS=torch.randn(B, C, generator=g),
                dW0=torch.randn(C, d, generator=g), db0=torch.randn(C, generator=g))


# ----------------------------------------------------------------------------------------------------------------
# label-smoothed cross-entropy: mean_b (lse(s_b) - sum_k t_bk s_bk), t = 1 - smoothing at the label, else
# smoothing / (C - 1) (the targets sum to 1)
# ----------------------------------------------------------------------------------------------------------------
def smoothed_ce(scores, labels, smoothing, dtype=F64):
    """(loss, dscores); dscores by autograd of the loss."""
    s = scores.detach().to(dtype).requires_grad_(True)
    B, C = s.shape
    t = torch.full((B, C), smoothing / (C - 1), dtype=dtype)
    t[torch.arange(B), labels] = 1.0 - smoothing
    loss = (torch.logsumexp(s, 1) - (t * s).sum(1)).sum() / B
    loss.backward()
    return loss.detach(), s.grad


def smoothed_ce_f32(scores, labels, smoothing, seq=False):
    """float32 by the formula of the kernel: ls = log_softmax(s), loss = mean_b sum_k -t ls, dscores = (exp(ls) - t)
    / B; ``seq``: the row losses added one row at a time."""
    B, C = scores.shape
    t = torch.full((B, C), smoothing / (C - 1))
    t[torch.arange(B), labels] = 1.0 - smoothing
    ls = torch.log_softmax(scores, 1)
    rows = (-t * ls).sum(1)
    return (seq_sum(rows) if seq else rows.sum()) / B, (ls.exp() - t) / B


def ce_case(B, C, kind="plain", seed=0):
    """kind: "plain" randn scores; "equal" all labels the same; "scaled" scores times 30; "spike" row 0 holds +90 on
    one class and -90 on the others."""
    g = torch.Generator().manual_seed(3000 + seed)
    s = torch.randn(B, C, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    if kind == "equal":
        labels = torch.full((B,), C - 1)
    elif kind == "scaled":
        s = s * 30
    elif kind == "spike":
        s[0] = -90.0
        s[0, 1] = 90.0
    return s, labels


# ----------------------------------------------------------------------------------------------------------------
# clip_grad_norm_(max_norm) + one Adam step (no weight decay, no amsgrad)
# ----------------------------------------------------------------------------------------------------------------
def clip_adam(param, grad, m, v, max_norm, b1, b2, eps, lr, step, dtype=F64):
    """(param, m, v, sum g^2) after step number ``step`` (from 1); max_norm None: no clipping.

    The native entry points take beta1 and beta2 as float32 and the bias-corrected step size and sqrt(1 - b2^t) as
    values their caller forms in double from the exact betas.  The reference restates that contract: the decays
    use the float32 values of the betas (inputs like the tensors are), the bias corrections the betas as given.
    With the exact 0.999 in the decay, exp_avg_sq would differ by 1.3e-5 of itself: 1 - float32(0.999) against
    0.001."""
    p, g, m, v = (t.to(dtype) for t in (param, grad, m, v))
    sq = (g * g).sum()
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (math.sqrt(float(sq)) + 1e-6))
    f1, f2 = torch.tensor(b1, dtype=torch.float32).item(), torch.tensor(b2, dtype=torch.float32).item()
    g = g * coef
    m = f1 * m + (1 - f1) * g
    v = f2 * v + (1 - f2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - (lr / (1 - b1 ** step)) * (m / denom), m, v, sq


def adam_case(n, clipped, seed=0, steps=3):
    """param (the size of freshly initialised weights), one gradient per step and max_norm: ``clipped`` has
    |g| >> max_norm, otherwise |g| < max_norm so that the clip coefficient is exactly 1.  m and v start at zero."""
    g = torch.Generator().manual_seed(4000 + seed)
    param = 0.05 * torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (3.0 if clipped else 0.1) for _ in range(steps)]
    max_norm = 0.5 if clipped else 10.0 * (1.0 + math.sqrt(n))
    return param, grads, max_norm


def sqnorm_case(n, seed=0):
    """randn times magnitudes rising from 1e-3 to 1e3, with |randn| at least 0.5 and the last three magnitudes all
    1e3: the elements the scalar tail of the kernel reads are among the largest, so dropping any one of them moves
    the total by 2e-6 of itself or more at every n the tests use."""
    g = torch.Generator().manual_seed(5000 + seed)
    r = torch.randn(n, generator=g)
    mag = torch.logspace(-3, 3, n)
    mag[-3:] = 1e3
    return (r.abs() + 0.5) * torch.where(r < 0, -1.0, 1.0) * mag


# ----------------------------------------------------------------------------------------------------------------
# sampled softmax: logits = X W[sids]^T, loss_i = lse_i - x_i . W[y_i]
# ----------------------------------------------------------------------------------------------------------------
def sampled_softmax(X, labels, sids, W, dloss=None, dtype=F64):
    """dict(loss [n], prob [n, S], dX [n, D], dW [V, D] dense, dW_lab [n, D], dW_smp [S, D]); dX and dW by autograd of
    sum_i g_i loss_i (g = dloss, or ones), the compact rows dW_lab[i] = -g_i X_i, dW_smp[j] = sum_i g_i p_ij X_i."""
    x = X.detach().to(dtype).requires_grad_(True)
    w = W.detach().to(dtype).requires_grad_(True)
    g = torch.ones(x.shape[0], dtype=dtype) if dloss is None else dloss.to(dtype)
    logits = x @ w[sids].t()
    lse = torch.logsumexp(logits, 1)
    loss = lse - (x * w[labels]).sum(1)
    (g * loss).sum().backward()
    prob = (logits - lse[:, None]).exp().detach()
    xd = x.detach()
    return dict(loss=loss.detach(), prob=prob, dX=x.grad, dW=w.grad, dW_lab=-g[:, None] * xd,
                dW_smp=(g[:, None] * prob).t() @ xd)


def sampled_softmax_f32(X, labels, sids, W, dloss=None, seq=False):
    """The same quantities in float32 by the formulas of the kernels (max-subtracted softmax, explicit gradients);
    ``seq``: every reduction one term at a time instead of torch's blocked sums."""
    n, D = X.shape
    S = sids.numel()
    g = torch.ones(n) if dloss is None else dloss
    Ws, Wy = W[sids], W[labels]
    if seq:
        logits, tl = torch.zeros(n, S), torch.zeros(n)
        for c in range(D):
            logits += X[:, c, None] * Ws[None, :, c]
            tl += X[:, c] * Wy[:, c]
    else:
        logits, tl = X @ Ws.t(), (X * Wy).sum(1)
    mx = logits.max(1, keepdim=True).values
    e = (logits - mx).exp()
    if seq:
        z = torch.zeros(n)
        for j in range(S):
            z += e[:, j]
    else:
        z = e.sum(1)
    lse = mx[:, 0] + z.log()
    prob = (logits - lse[:, None]).exp()
    gp = g[:, None] * prob
    if seq:
        acc, smp = torch.zeros(n, D), torch.zeros(S, D)
        for j in range(S):
            acc += prob[:, j, None] * Ws[j]
        for i in range(n):
            smp += gp[i, :, None] * X[i]
    else:
        acc, smp = prob @ Ws, gp.t() @ X
    lab = -g[:, None] * X
    dW = torch.zeros_like(W)
    dW.index_add_(0, labels, lab)
    dW.index_add_(0, sids, smp)
    return dict(loss=lse - tl, prob=prob, dX=g[:, None] * (acc - Wy), dW=dW, dW_lab=lab, dW_smp=smp)


SS_V = 3001


def ss_case(S, D, n_rows, shifted=False, seed=0):
    """X [n_rows, D], W [V, D] (V = 3001), distinct sids [S], labels [n_rows] of which every fourth also is a sample
    and every row 3 mod 7 repeats the label of the row before, and a dloss with zeros and negative values.
    Logits are O(1): X ~ N(0, 1), W ~ N(0, 1 / D).  ``shifted``: X[:, 0] = 1, W[:, 0] = 100, every logit near 100."""
    g = torch.Generator().manual_seed(6000 + seed)
    X = torch.randn(n_rows, D, generator=g)
    W = torch.randn(SS_V, D, generator=g) / math.sqrt(D)
    if shifted:
        assert D >= 2
        X[:, 0] = 1.0
        W[:, 0] = 100.0
    sids = torch.randperm(SS_V, generator=g)[:S]
    labels = torch.randint(0, SS_V, (n_rows,), generator=g)
    i4 = torch.arange(n_rows)[::4]
    labels[i4] = sids[i4 % S]
    i7 = torch.arange(n_rows)[3::7]
    labels[i7] = labels[i7 - 1]
    dloss = torch.randn(n_rows, generator=g)
    dloss[::5] = 0.0
    return dict(X=X, W=W, sids=sids, labels=labels, dloss=dloss, S=S, D=D, n_rows=n_rows)


def sum_case(n, seed=0):
    """Values in [0.5, 1.5): the sum is well conditioned and one dropped element is 1e-4 of it or more."""
    return torch.rand(n, generator=torch.Generator().manual_seed(7000 + seed)) + 0.5


def seq_sum(x):
    acc = torch.zeros((), dtype=x.dtype)
    for i in range(x.numel()):
        acc = acc + x[i]
    return acc
