"""The per-entry additive attention bias of the neighbour attention kernels (csrc/csr_attn.hip, u2gnn_csr_attn_*_bias)
and the two table kernels around it (u2gnn_bias_expand, u2gnn_bias_table_grad).

Reference of the attention: float64 in ENTRY space -- s_e = q_i . k_j + b_e, a softmax over each row's own entries (so
a column listed twice counts twice, each entry with its own bias), the kernels' dropout mask at (i, j), gradients of q,
k, v and b by autograd; rel < 1e-5, tests/test_csr_attn_gpu.py's gate for the same arithmetic class."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_csr_attn_gpu import N_MAIN, Q_SCALE, SEED, _inputs, main_pattern, rel, to_csr  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip.core import Adjacency  # noqa: E402

DEV = "cuda"
ROWS_PAD = 512
_PATTERN = {}


def _pattern(form):
    """(rowptr, colidx, Adjacency) of the main pattern, built once per form."""
    if form not in _PATTERN:
        rowptr, colidx = to_csr(main_pattern(form))
        _PATTERN[form] = (rowptr, colidx, Adjacency.from_csr(rowptr, colidx, N_MAIN, device=DEV))
    return _PATTERN[form]


def _bias(nnz):
    g = torch.Generator(device=DEV).manual_seed(77)
    return 2.0 * torch.randn(nnz, device=DEV, generator=g)


def _run(QKV, dO, A, bias, dp, p, want_dbias=True):
    O = torch.full((ROWS_PAD, dp), float("nan"), device=DEV)
    stats = torch.full((ROWS_PAD, 2), float("nan"), device=DEV)
    K.csr_attn_fwd_bias(QKV, dp, A, bias, O, stats, p, SEED, N_MAIN, ROWS_PAD)
    dQKV = torch.full((ROWS_PAD, 3 * dp), float("nan"), device=DEV)
    db = torch.full((A.nnz,), float("nan"), device=DEV) if want_dbias else None
    K.csr_attn_bwd_bias(QKV, dp, A, bias, O, dO, stats, p, SEED, Q_SCALE, dQKV, db, N_MAIN, ROWS_PAD)
    return O, stats, dQKV, db


def _reference(QKV, dO, rowptr, colidx, bias, dp, p):
    N = N_MAIN
    q = QKV[:N, :dp].double().clone().requires_grad_(True)
    k = QKV[:N, dp:2 * dp].double().clone().requires_grad_(True)
    v = QKV[:N, 2 * dp:3 * dp].double().clone().requires_grad_(True)
    b = bias.double().clone().requires_grad_(True)
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rowptr))).to(DEV)
    cols = torch.from_numpy(colidx).to(DEV)
    s = (q[rows] * k[cols]).sum(1) + b
    m = torch.full((N,), float("-inf"), device=DEV, dtype=torch.float64).scatter_reduce(0, rows, s.detach(), "amax")
    ex = torch.exp(s - m[rows])
    P = ex / torch.zeros(N, device=DEV, dtype=torch.float64).index_add(0, rows, ex)[rows]
    if p > 0:
        P = P * K.dropout_mask(SEED, N, N, p)[rows, cols].double() / (1 - p)
    O = torch.zeros(N, dp, device=DEV, dtype=torch.float64).index_add(0, rows, P[:, None] * v[cols])
    O.backward(dO[:N].double())
    return O.detach(), q.grad, k.grad, v.grad, b.grad


def _check(form, dp, p):
    rowptr, colidx, A = _pattern(form)
    N = N_MAIN
    QKV, dO = _inputs(N, ROWS_PAD, dp)
    bias = _bias(A.nnz)
    O, stats, dQKV, db = _run(QKV, dO, A, bias, dp, p)
    for t in (O, stats, dQKV, db):
        assert torch.isfinite(t).all()
    Or, dq, dk, dv, dbr = _reference(QKV, dO, rowptr, colidx, bias, dp, p)
    figs = {"O": rel(O[:N].double(), Or), "dQ": rel(dQKV[:N, :dp].double(), dq * Q_SCALE),
            "dK": rel(dQKV[:N, dp:2 * dp].double(), dk), "dV": rel(dQKV[:N, 2 * dp:].double(), dv),
            "db": rel(db.double(), dbr)}
    print(f"csr_attn bias {form} nnz={A.nnz} dp={dp} p={p}: {figs}")
    for name, f in figs.items():
        assert f < 1e-5, (name, f)
    assert O[N:].abs().max().item() == 0 and dQKV[N:].abs().max().item() == 0     # padding rows: exactly zero
    O2, stats2, dQKV2, db2 = _run(QKV, dO, A, bias, dp, p)                          # bit-identical from run to run
    assert torch.equal(O, O2) and torch.equal(stats, stats2) and torch.equal(dQKV, dQKV2) and torch.equal(db, db2)
    # dbias = NULL: the same dQKV bits
    _, _, dQKV3, _ = _run(QKV, dO, A, bias, dp, p, want_dbias=False)
    assert torch.equal(dQKV, dQKV3)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384])
@pytest.mark.parametrize("form", ["full", "hole"])
def test_csr_attention_bias_fwd_bwd(form, dp, p):
    _check(form, dp, p)


def test_csr_attention_bias_widest():
    """dp = 1024: the U = 1 / MAXC = 16 instantiation."""
    _check("full", 1024, 0.5)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384, 1024])
def test_zero_bias_is_the_call_without_bias(dp, p):
    """bias = 0: O, the statistics and dQKV equal the calls without bias bit for bit (s + 0.0f is exact)."""
    _, _, A = _pattern("full")
    QKV, dO = _inputs(N_MAIN, ROWS_PAD, dp)
    O, stats, dQKV, _ = _run(QKV, dO, A, torch.zeros(A.nnz, device=DEV), dp, p)
    O0 = torch.full((ROWS_PAD, dp), float("nan"), device=DEV)
    stats0 = torch.full((ROWS_PAD, 2), float("nan"), device=DEV)
    K.csr_attn_fwd(QKV, dp, A, O0, stats0, p, SEED, N_MAIN, ROWS_PAD)
    dQKV0 = torch.full((ROWS_PAD, 3 * dp), float("nan"), device=DEV)
    K.csr_attn_bwd(QKV, dp, A, O0, dO, stats0, p, SEED, Q_SCALE, dQKV0, N_MAIN, ROWS_PAD)
    assert torch.equal(O, O0) and torch.equal(stats, stats0) and torch.equal(dQKV, dQKV0)


def _tables_case(R, n_types, nnz, lo=0, hi=None):
    g = torch.Generator(device=DEV).manual_seed(1000 * R + 10 * n_types + nnz % 7)
    hi = n_types if hi is None else hi
    etype = torch.randint(lo, hi, (nnz,), device=DEV, generator=g, dtype=torch.int64).to(torch.int32)
    tables = torch.randn(R, n_types, device=DEV, generator=g)
    ld = (nnz + 3) // 4 * 4
    return etype, tables, ld, g


GRID = [(R, T, nnz) for R in (1, 8) for T in (1, 2, 32) for nnz in (1, 1000, 65537)]


@pytest.mark.parametrize("R,n_types,nnz", GRID)
def test_bias_expand(R, n_types, nnz):
    etype, tables, ld, _ = _tables_case(R, n_types, nnz)
    out = torch.full((R, ld), float("nan"), device=DEV)
    K.bias_expand(tables, etype, out)
    assert torch.equal(out[:, :nnz], tables[:, etype.long()])
    assert torch.isnan(out[:, nnz:]).all()                      # nothing past the entries is written


def test_bias_expand_out_of_range_type_gives_zero():
    R, n_types, nnz = 3, 4, 1000
    etype, tables, ld, _ = _tables_case(R, n_types, nnz, lo=-2, hi=n_types + 3)
    bad = (etype < 0) | (etype >= n_types)
    assert bad.any() and (~bad).any()
    out = torch.full((R, ld), float("nan"), device=DEV)
    K.bias_expand(tables, etype, out)
    ref = torch.where(bad[None, :], torch.zeros((), device=DEV), tables[:, etype.long().clamp(0, n_types - 1)])
    assert torch.equal(out[:, :nnz], ref)


def _table_grad_check(R, n_types, etype, dbias, nnz):
    guard = torch.full((R + 1, n_types), 12345.0, device=DEV)
    got = guard[:R]
    K.bias_table_grad(dbias, etype, got)
    ok = (etype >= 0) & (etype < n_types)
    idx = etype.long()[ok]
    d64 = dbias[:, :nnz].double()[:, ok]
    ref = torch.zeros(R, n_types, device=DEV, dtype=torch.float64).index_add(1, idx, d64)
    mag = torch.zeros(R, n_types, device=DEV, dtype=torch.float64).index_add(1, idx, d64.abs())
    # the kernels' bound: 16 + 1 sequential adds and 16 tree levels here, within (128 + 32) * 2^-24 ~ 9.5e-6 of mag
    err = (got.double() - ref).abs()
    print(f"bias_table_grad R={R} types={n_types} nnz={nnz}: max err / mag "
          f"{(err / mag.clamp_min(1e-30)).max().item():.3g}")
    assert (err <= 1e-5 * mag).all()
    assert (got[mag == 0] == 0).all()                            # a type without entries: exactly zero
    assert (guard[R] == 12345.0).all()                           # nothing else is written
    again = torch.empty(R, n_types, device=DEV)
    K.bias_table_grad(dbias, etype, again)
    assert torch.equal(got, again)                               # bit-identical from run to run
    return got


@pytest.mark.parametrize("R,n_types,nnz", GRID)
def test_bias_table_grad(R, n_types, nnz):
    etype, _, ld, g = _tables_case(R, n_types, nnz)
    dbias = torch.randn(R, ld, device=DEV, generator=g)
    _table_grad_check(R, n_types, etype, dbias, nnz)


def test_bias_table_grad_type_without_entries():
    R, n_types, nnz = 2, 5, 4099
    etype, _, ld, g = _tables_case(R, n_types, nnz)
    etype[etype == 3] = 1
    dbias = torch.randn(R, ld, device=DEV, generator=g)
    got = _table_grad_check(R, n_types, etype, dbias, nnz)
    assert (got[:, 3] == 0).all() and (got[:, 1] != 0).all()


def test_bias_table_grad_skips_out_of_range_types():
    R, n_types, nnz = 2, 4, 5001
    etype, _, ld, g = _tables_case(R, n_types, nnz, lo=-2, hi=n_types + 3)
    assert ((etype < 0) | (etype >= n_types)).any()
    dbias = torch.randn(R, ld, device=DEV, generator=g)
    _table_grad_check(R, n_types, etype, dbias, nnz)
