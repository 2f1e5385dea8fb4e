"""Neighbour attention kernels (csrc/csr_attn.hip) against the float64 dense restatement of
tests/test_segment_attn_gpu.py: Q K^T with -inf where the adjacency count is 0 and log(count) added where a column is
listed more than once, softmax, the kernels' own dropout mask (K.dropout_mask over the global indices), gradients by
autograd; rel < 1e-5, that file's gate for the same arithmetic class (exact fp32 products, expf).

The main pattern (N = 437, seeded, non-symmetric) holds an empty row, rows with only themselves, a row of degree 1,
a row of degree 130 (more than any unroll or group width), a wide row, a duplicated column, and a hub column that
every row of the random part lists.  "A row attending over all N" and "a column that no row lists" exclude each
other, so the pattern comes in two forms that differ in the wide row only: "full" (all N columns) and "hole" (all
but column HOLE, which then no row lists: an empty transpose list)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from edges_ref import block_csr, csr_to_dense  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip.core import Adjacency  # noqa: E402

DEV = "cuda"
RAGGED = [0, 1, 2, 19, 19, 83, 84, 400, 437]
SEED = 4321
Q_SCALE = 1 / math.sqrt(7.0)
N_MAIN, HUB, HOLE = 437, 50, 100
EMPTY, SELF_ONLY, DEG1, DEG130, WIDE, DUP = 0, (1, 2), 3, 4, 5, 6


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def main_pattern(form, N=N_MAIN):
    """Row lists (not sorted: the kernels do not need it) of the main case."""
    r = np.random.RandomState(5)
    legal = np.array([c for c in range(N) if c != HOLE])
    rows = [[] for _ in range(N)]
    for i in SELF_ONLY:
        rows[i] = [i]
    rows[DEG1] = [10]
    rows[DEG130] = list(r.choice(legal, 130, replace=False))
    rows[WIDE] = list(range(N)) if form == "full" else list(legal)
    rows[DUP] = [7, 7, 20, 33, HUB]
    for i in range(DUP + 1, N):
        cols = set(r.choice(legal, r.randint(1, 13), replace=False).tolist())
        rows[i] = list(r.permutation(sorted(cols | {HUB})))
    return rows


def to_csr(rows):
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    return rowptr, np.concatenate([np.asarray(c, dtype=np.int64) for c in rows])


def _inputs(N, rows_pad, dp, gen_seed=1):
    g = torch.Generator(device=DEV).manual_seed(gen_seed)
    QKV = torch.randn(rows_pad, 3 * dp, device=DEV, generator=g)
    QKV[:, :dp] *= 1 / math.sqrt(dp)      # scores of order 1, as the in-projection's 1/sqrt(d) leaves them
    QKV[N:] = 0
    dO = torch.randn(rows_pad, dp, device=DEV, generator=g)
    dO[N:] = 0
    return QKV, dO


def _run(QKV, dO, A, N, rows_pad, dp, p):
    O = torch.full((rows_pad, dp), float("nan"), device=DEV)
    stats = torch.full((rows_pad, 2), float("nan"), device=DEV)
    K.csr_attn_fwd(QKV, dp, A, O, stats, p, SEED, N, rows_pad)
    dQKV = torch.full((rows_pad, 3 * dp), float("nan"), device=DEV)
    K.csr_attn_bwd(QKV, dp, A, O, dO, stats, p, SEED, Q_SCALE, dQKV, N, rows_pad)
    return O, stats, dQKV


def _reference(QKV, dO, count, N, dp, p):
    """float64, dense: (O, dQ, dK, dV) over the N real rows; count [N, N]: how often row i lists column j."""
    q = QKV[:N, :dp].double().clone().requires_grad_(True)
    k = QKV[:N, dp:2 * dp].double().clone().requires_grad_(True)
    v = QKV[:N, 2 * dp:3 * dp].double().clone().requires_grad_(True)
    cnt = torch.as_tensor(count, device=DEV).double()
    S = q @ k.t() + torch.log(cnt)                    # log 0 = -inf: outside the pattern
    none = (cnt.sum(1) == 0)[:, None]
    P = torch.softmax(S.masked_fill(none, 0.0), dim=-1).masked_fill(none, 0.0)   # a row with no entries: zeros
    if p > 0:
        P = P * K.dropout_mask(SEED, N, N, p).double() / (1 - p)
    O = P @ v
    O.backward(dO[:N].double())
    return O.detach(), q.grad, k.grad, v.grad


def _check(rowptr, colidx, N, rows_pad, dp, p, what):
    A = Adjacency.from_csr(rowptr, colidx, N, device=DEV)
    QKV, dO = _inputs(N, rows_pad, dp)
    O, stats, dQKV = _run(QKV, dO, A, N, rows_pad, dp, p)
    assert torch.isfinite(O).all() and torch.isfinite(dQKV).all() and torch.isfinite(stats).all()
    Or, dq, dk, dv = _reference(QKV, dO, csr_to_dense(rowptr, colidx, N), N, dp, p)
    figs = {"O": rel(O[:N].double(), Or), "dQ": rel(dQKV[:N, :dp].double(), dq * Q_SCALE),
            "dK": rel(dQKV[:N, dp:2 * dp].double(), dk), "dV": rel(dQKV[:N, 2 * dp:].double(), dv)}
    print(f"csr_attn {what} N={N} nnz={len(colidx)} dp={dp} p={p}: {figs}")
    for name, f in figs.items():
        assert f < 1e-5, (name, f)
    if N < rows_pad:   # padding rows: exactly zero
        assert O[N:].abs().max().item() == 0 and dQKV[N:].abs().max().item() == 0
    # bit-identical from run to run
    O2, stats2, dQKV2 = _run(QKV, dO, A, N, rows_pad, dp, p)
    assert torch.equal(O, O2) and torch.equal(stats, stats2) and torch.equal(dQKV, dQKV2)
    return O, dQKV


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384])
@pytest.mark.parametrize("form", ["full", "hole"])
def test_csr_attention_fwd_bwd(form, dp, p):
    rows = main_pattern(form)
    assert len(rows[EMPTY]) == 0 and len(rows[DEG1]) == 1 and len(rows[DEG130]) == 130
    assert len(rows[WIDE]) == (N_MAIN if form == "full" else N_MAIN - 1)
    assert all(HUB in c for c in rows[DUP:]) and rows[DUP].count(7) == 2
    rowptr, colidx = to_csr(rows)
    count = csr_to_dense(rowptr, colidx, N_MAIN)
    assert (count != count.T).any() and count.max() == 2
    assert (count[:, HOLE].sum() == 0) == (form == "hole")
    O, dQKV = _check(rowptr, colidx, N_MAIN, 512, dp, p, form)
    # the empty row: exactly zero in O and dQ (its dK / dV rows are whatever lists it: the wide row does)
    assert O[EMPTY].abs().max().item() == 0 and dQKV[EMPTY, :dp].abs().max().item() == 0
    if form == "hole":   # a column no row lists: exactly zero dK and dV
        assert dQKV[HOLE, dp:].abs().max().item() == 0


def test_csr_attention_widest():
    N = 83
    r = np.random.RandomState(9)
    rows = [[]] + [[i] for i in (1, 2)] + [list(range(N))]
    rows += [list(r.choice(N, r.randint(1, 9), replace=False)) for _ in range(len(rows), N)]
    rowptr, colidx = to_csr(rows)
    _check(rowptr, colidx, N, 128, 1024, 0.5, "widest")


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_complete_blocks_match_the_segment_kernels(p):
    """The CSR of complete diagonal blocks over RAGGED is per-graph attention: O and dQKV within 1e-5 of
    K.segment_attn_fwd / _bwd."""
    dp, N, rows_pad = 384, RAGGED[-1], 512
    rowptr, colidx = block_csr(RAGGED)
    A = Adjacency.from_csr(rowptr, colidx, N, device=DEV)
    QKV, dO = _inputs(N, rows_pad, dp)
    O, _, dQKV = _run(QKV, dO, A, N, rows_pad, dp, p)
    off = torch.tensor(RAGGED, dtype=torch.int64, device=DEV)
    Os, st = torch.empty(rows_pad, dp, device=DEV), torch.empty(rows_pad, 2, device=DEV)
    K.segment_attn_fwd(QKV, dp, off, Os, st, p, SEED, N, rows_pad)
    dS = torch.empty(rows_pad, 3 * dp, device=DEV)
    K.segment_attn_bwd(QKV, dp, off, Os, dO, st, p, SEED, Q_SCALE, dS, N, rows_pad)
    figs = {"O": rel(O.double(), Os.double()), "dQ": rel(dQKV[:, :dp].double(), dS[:, :dp].double()),
            "dK": rel(dQKV[:, dp:2 * dp].double(), dS[:, dp:2 * dp].double()),
            "dV": rel(dQKV[:, 2 * dp:].double(), dS[:, 2 * dp:].double())}
    print(f"csr_attn vs segment_attn p={p}: {figs}")
    for name, f in figs.items():
        assert f < 1e-5, (name, f)


def test_full_pattern_matches_dense_attention():
    N = 100
    rowptr, colidx = block_csr([0, N])
    assert len(colidx) == N * N
    _check(rowptr, colidx, N, 128, 128, 0.5, "dense")


def test_a_key_row_reaches_exactly_the_rows_that_list_it():
    """Perturbing K and V of row j changes the O rows that list j; every other row is bit-unchanged."""
    dp, N, rows_pad, j = 384, N_MAIN, 512, 33
    rows = main_pattern("hole")
    A = Adjacency.from_csr(*to_csr(rows), N, device=DEV)
    QKV, dO = _inputs(N, rows_pad, dp)
    O, _, _ = _run(QKV, dO, A, N, rows_pad, dp, 0.0)
    QKV2 = QKV.clone()
    QKV2[j, dp:] += 1.0
    O2, _, _ = _run(QKV2, dO, A, N, rows_pad, dp, 0.0)
    lists = torch.tensor([j in c for c in rows] + [False] * (rows_pad - N), device=DEV)
    assert 2 <= int(lists.sum()) < N
    changed = (O != O2).any(1)
    assert torch.equal(changed, lists)


def test_bad_arguments():
    from u2gnn_hip._lib import U2GNNNativeError
    dp, N, rows_pad = 64, 100, 128
    QKV, dO = _inputs(N, rows_pad, dp)
    A = Adjacency.from_csr(*block_csr([0, 10, N]), N, device=DEV)
    O, st = torch.empty(rows_pad, dp, device=DEV), torch.empty(rows_pad, 2, device=DEV)
    K.csr_attn_fwd(QKV, dp, A, O, st, 0.0, SEED, N, rows_pad)
    dQKV = torch.empty(rows_pad, 3 * dp, device=DEV)
    empty = Adjacency.from_csr(np.zeros(N + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), N, device=DEV)
    for bad in (lambda: K.csr_attn_fwd(QKV, dp, empty, O, st, 0.0, SEED, N, rows_pad),          # nnz < 1
                lambda: K.csr_attn_fwd(QKV, 32, A, O, st, 0.0, SEED, N, rows_pad),              # dp % 64
                lambda: K.csr_attn_fwd(QKV, dp, A, O, st, 1.0, SEED, N, rows_pad),              # p outside [0, 1)
                lambda: K.csr_attn_fwd(QKV.cpu(), dp, A, O, st, 0.0, SEED, N, rows_pad),        # host tensor
                lambda: K.csr_attn_bwd(QKV, dp, empty, O, dO, st, 0.0, SEED, Q_SCALE, dQKV, N, rows_pad),
                lambda: K.csr_attn_bwd(QKV, 32, A, O, dO, st, 0.0, SEED, Q_SCALE, dQKV, N, rows_pad),
                lambda: K.csr_attn_bwd(QKV, dp, A, O, dO, st, 1.0, SEED, Q_SCALE, dQKV, N, rows_pad),
                lambda: K.csr_attn_bwd(QKV, dp, A, O, dO.cpu(), st, 0.0, SEED, Q_SCALE, dQKV, N, rows_pad)):
        with pytest.raises(U2GNNNativeError):
            bad()
