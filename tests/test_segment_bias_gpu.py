"""The per-pair additive bias of the per-graph attention kernels (csrc/segment_attn.hip, u2gnn_segment_attn_*_bias) on
the shapes of tests/test_segment_attn_gpu.py, the ones chosen to break tiling.

Reference: float64, dense -- Q K^T plus a dense bias (segment g's [n_g, n_g] block at pair_off[g], row-major) with
-inf outside the diagonal blocks, softmax, the kernels' own dropout mask, gradients by autograd with the bias as a
leaf; rel < 1e-5, the gate of test_segment_attn_gpu.py and test_csr_bias_gpu.py for the same arithmetic class.  Against
the CSR kernels (every pair of every segment as an entry, the same bias per entry): 2e-5, the sum of the two gates."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from edges_ref import block_csr  # noqa: E402
from test_segment_attn_gpu import Q_SCALE, RAGGED, SEED, _inputs, rel  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip._lib import U2GNNNativeError  # noqa: E402
from u2gnn_hip.core import Adjacency  # noqa: E402

DEV = "cuda"
SHAPES = [(RAGGED, 512), ([0, 437], 512), ([0, 16, 32, 48, 64], 128)]
IDS = ["ragged", "one", "aligned"]
WIDEST = ([0, 1, 2, 19, 19, 83], 128, 1024, 0.5)


def _pairs(offsets):
    """(pair_off list, n_pairs, rows, cols): the entry pair_off[g] + (i - lo) n_g + (j - lo) of every pair, in entry
    order."""
    n = np.diff(np.asarray(offsets))
    pair_off = np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)
    rows = np.concatenate([np.repeat(np.arange(offsets[g], offsets[g + 1]), n[g]) for g in range(len(n))])
    cols = np.concatenate([np.tile(np.arange(offsets[g], offsets[g + 1]), n[g]) for g in range(len(n))])
    return pair_off, int(pair_off[-1]), rows.astype(np.int64), cols.astype(np.int64)


def _bias(n_pairs):
    g = torch.Generator(device=DEV).manual_seed(77)
    return 2.0 * torch.randn(n_pairs, device=DEV, generator=g)


def _run(QKV, dO, offsets, pair_off, bias, N, rows_pad, dp, p, want_dbias=True):
    off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    po = None if pair_off is None else torch.as_tensor(pair_off, dtype=torch.int64).to(DEV)
    O = torch.full((rows_pad, dp), float("nan"), device=DEV)
    stats = torch.full((rows_pad, 2), float("nan"), device=DEV)
    K.segment_attn_fwd_bias(QKV, dp, off, po, bias, O, stats, p, SEED, N, rows_pad)
    dQKV = torch.full((rows_pad, 3 * dp), float("nan"), device=DEV)
    db = torch.full_like(bias, float("nan")) if want_dbias and bias is not None else None
    K.segment_attn_bwd_bias(QKV, dp, off, po, bias, O, dO, stats, p, SEED, Q_SCALE, dQKV, db, N, rows_pad)
    return O, stats, dQKV, db


def _plain(QKV, dO, offsets, N, rows_pad, dp, p):
    off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    O = torch.full((rows_pad, dp), float("nan"), device=DEV)
    stats = torch.full((rows_pad, 2), float("nan"), device=DEV)
    K.segment_attn_fwd(QKV, dp, off, O, stats, p, SEED, N, rows_pad)
    dQKV = torch.full((rows_pad, 3 * dp), float("nan"), device=DEV)
    K.segment_attn_bwd(QKV, dp, off, O, dO, stats, p, SEED, Q_SCALE, dQKV, N, rows_pad)
    return O, stats, dQKV


def _reference(QKV, dO, rows, cols, bias, N, dp, p):
    """float64, dense: (O, dQ, dK, dV, dbias) over the N real rows."""
    q = QKV[:N, :dp].double().clone().requires_grad_(True)
    k = QKV[:N, dp:2 * dp].double().clone().requires_grad_(True)
    v = QKV[:N, 2 * dp:3 * dp].double().clone().requires_grad_(True)
    b = bias.double().clone().requires_grad_(True)
    r, c = torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)
    mask = torch.full((N, N), float("-inf"), device=DEV, dtype=torch.float64).index_put((r, c), b)   # block mask + bias
    P = torch.softmax(q @ k.t() + mask, dim=-1)
    if p > 0:
        P = P * K.dropout_mask(SEED, N, N, p).double() / (1 - p)
    O = P @ v
    O.backward(dO[:N].double())
    return O.detach(), q.grad, k.grad, v.grad, b.grad


def _check(offsets, rows_pad, dp, p):
    N = offsets[-1]
    pair_off, n_pairs, rows, cols = _pairs(offsets)
    QKV, dO = _inputs(N, rows_pad, dp)
    bias = _bias(n_pairs)
    O, stats, dQKV, db = _run(QKV, dO, offsets, pair_off, bias, N, rows_pad, dp, p)
    for t in (O, stats, dQKV, db):
        assert torch.isfinite(t).all()                           # (db: every pair was written)
    Or, dq, dk, dv, dbr = _reference(QKV, dO, rows, cols, bias, N, dp, p)
    figs = {"O": rel(O[:N].double(), Or), "dQ": rel(dQKV[:N, :dp].double(), dq * Q_SCALE),
            "dK": rel(dQKV[:N, dp:2 * dp].double(), dk), "dV": rel(dQKV[:N, 2 * dp:].double(), dv),
            "db": rel(db.double(), dbr)}
    print(f"segment_attn bias offsets={offsets} dp={dp} p={p}: {figs}")
    for name, f in figs.items():
        assert f < 1e-5, (name, f)
    if N < rows_pad:
        assert O[N:].abs().max().item() == 0 and dQKV[N:].abs().max().item() == 0     # padding rows: exactly zero
    O2, stats2, dQKV2, db2 = _run(QKV, dO, offsets, pair_off, bias, N, rows_pad, dp, p)   # bit-identical run to run
    assert torch.equal(O, O2) and torch.equal(stats, stats2) and torch.equal(dQKV, dQKV2) and torch.equal(db, db2)
    _, _, dQKV3, _ = _run(QKV, dO, offsets, pair_off, bias, N, rows_pad, dp, p, want_dbias=False)   # dbias = NULL
    assert torch.equal(dQKV, dQKV3)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384])
@pytest.mark.parametrize("offsets,rows_pad", SHAPES, ids=IDS)
def test_segment_attention_bias_fwd_bwd(offsets, rows_pad, dp, p):
    _check(offsets, rows_pad, dp, p)


def test_segment_attention_bias_widest():
    _check(*WIDEST)


def _zero_bias_case(offsets, rows_pad, dp, p):
    N = offsets[-1]
    pair_off, n_pairs, _, _ = _pairs(offsets)
    QKV, dO = _inputs(N, rows_pad, dp)
    O0, stats0, dQKV0 = _plain(QKV, dO, offsets, N, rows_pad, dp, p)
    O, stats, dQKV, db = _run(QKV, dO, offsets, pair_off, torch.zeros(n_pairs, device=DEV), N, rows_pad, dp, p)
    assert torch.equal(O, O0) and torch.equal(stats, stats0) and torch.equal(dQKV, dQKV0)   # s + 0.0f is exact
    assert torch.isfinite(db).all() and db.abs().max().item() > 0
    On, statsn, dQKVn, _ = _run(QKV, dO, offsets, None, None, N, rows_pad, dp, p)            # NULL bias: the plain call
    assert torch.equal(On, O0) and torch.equal(statsn, stats0) and torch.equal(dQKVn, dQKV0)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384])
@pytest.mark.parametrize("offsets,rows_pad", SHAPES, ids=IDS)
def test_zero_and_null_bias_are_the_plain_calls(offsets, rows_pad, dp, p):
    _zero_bias_case(offsets, rows_pad, dp, p)


def test_zero_and_null_bias_are_the_plain_calls_widest():
    _zero_bias_case(*WIDEST)


def _against_csr(offsets, rows_pad, dp, p):
    """Every pair of every segment as a CSR entry: block_csr lists segment g's rows in order, each with the columns
    lo .. hi-1 ascending, so entry e of the CSR is pair e of the packed order and takes bias[e]."""
    N = offsets[-1]
    pair_off, n_pairs, rows, cols = _pairs(offsets)
    rowptr, colidx = block_csr(offsets)
    assert len(colidx) == n_pairs and np.array_equal(colidx, cols)
    assert np.array_equal(np.repeat(np.arange(N), np.diff(rowptr)), rows)
    A = Adjacency.from_csr(rowptr, colidx, N, device=DEV)
    QKV, dO = _inputs(N, rows_pad, dp)
    bias = _bias(n_pairs)
    O, _, dQKV, db = _run(QKV, dO, offsets, pair_off, bias, N, rows_pad, dp, p)
    Oc = torch.full((rows_pad, dp), float("nan"), device=DEV)
    sc = torch.full((rows_pad, 2), float("nan"), device=DEV)
    K.csr_attn_fwd_bias(QKV, dp, A, bias, Oc, sc, p, SEED, N, rows_pad)
    dc = torch.full((rows_pad, 3 * dp), float("nan"), device=DEV)
    dbc = torch.full_like(bias, float("nan"))
    K.csr_attn_bwd_bias(QKV, dp, A, bias, Oc, dO, sc, p, SEED, Q_SCALE, dc, dbc, N, rows_pad)
    figs = {"O": rel(O[:N], Oc[:N]), "dQ": rel(dQKV[:N, :dp], dc[:N, :dp]),
            "dK": rel(dQKV[:N, dp:2 * dp], dc[:N, dp:2 * dp]), "dV": rel(dQKV[:N, 2 * dp:], dc[:N, 2 * dp:]),
            "db": rel(db, dbc)}
    print(f"segment bias vs csr bias offsets={offsets} dp={dp} p={p}: {figs}")
    for name, f in figs.items():
        assert f < 2e-5, (name, f)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dp", [64, 384])
@pytest.mark.parametrize("offsets,rows_pad", SHAPES, ids=IDS)
def test_segment_bias_against_the_csr_kernels(offsets, rows_pad, dp, p):
    _against_csr(offsets, rows_pad, dp, p)


def test_segment_bias_against_the_csr_kernels_widest():
    _against_csr(*WIDEST)


@pytest.mark.parametrize("dp,p", [(64, 0.0), (384, 0.5)])
def test_pair_base_out_of_range_reads_zero_and_writes_nothing(dp, p):
    """The last segment's pair_off set to n_pairs: every entry id of that segment is >= n_pairs, so it runs as under a
    zero bias and leaves its dbias entries alone; the other segments are unchanged bit for bit; all finite."""
    offsets, rows_pad = RAGGED, 512
    N = offsets[-1]
    pair_off, n_pairs, _, _ = _pairs(offsets)
    last = len(offsets) - 2
    lo, hi, e0 = offsets[last], offsets[last + 1], int(pair_off[last])
    QKV, dO = _inputs(N, rows_pad, dp)
    bias = _bias(n_pairs)
    good = _run(QKV, dO, offsets, pair_off, bias, N, rows_pad, dp, p)
    bad_off = pair_off.copy()
    bad_off[last] = n_pairs
    bad = _run(QKV, dO, offsets, bad_off, bias, N, rows_pad, dp, p)
    zeroed = bias.clone()
    zeroed[e0:] = 0
    zero = _run(QKV, dO, offsets, pair_off, zeroed, N, rows_pad, dp, p)
    for t in bad[:3]:
        assert torch.isfinite(t).all()
    for g, b, z in zip(good[:3], bad[:3], zero[:3]):
        assert torch.equal(b[:lo], g[:lo]) and torch.equal(b[hi:], g[hi:])     # the other segments
        assert torch.equal(b[lo:hi], z[lo:hi])                                 # this one: as under a zero bias
        assert not torch.equal(b[lo:hi], g[lo:hi])
    assert torch.equal(bad[3][:e0], good[3][:e0]) and torch.isnan(bad[3][e0:]).all()   # its pairs: not written


def test_wrappers_refuse_bad_arguments():
    dp, N, rows_pad = 64, 64, 128
    offsets = [0, 16, 32, 48, 64]
    pair_off, n_pairs, _, _ = _pairs(offsets)
    QKV, dO = _inputs(N, rows_pad, dp)
    off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    po = torch.from_numpy(pair_off).to(DEV)
    bias = _bias(n_pairs)
    O, st = torch.empty(rows_pad, dp, device=DEV), torch.empty(rows_pad, 2, device=DEV)
    dQKV = torch.empty(rows_pad, 3 * dp, device=DEV)
    def fwd(po=po, bias=bias, QKV=QKV):
        K.segment_attn_fwd_bias(QKV, dp, off, po, bias, O, st, 0.0, SEED, N, rows_pad)

    def bwd(po=po, bias=bias, db=None):
        K.segment_attn_bwd_bias(QKV, dp, off, po, bias, O, dO, st, 0.0, SEED, Q_SCALE, dQKV, db, N, rows_pad)
    fwd()
    bwd(db=torch.empty_like(bias))
    for call in (lambda: fwd(bias=bias.cpu()), lambda: fwd(po=po.cpu()), lambda: fwd(QKV=QKV.cpu()),   # host tensors
                 lambda: fwd(po=None),                                     # a bias without its pair offsets
                 lambda: fwd(po=po[:-1]), lambda: fwd(po=po.int()),        # one offset per segment bound, int64
                 lambda: fwd(bias=bias.double()), lambda: fwd(bias=bias.view(-1, 2)), lambda: fwd(bias=bias[:0]),
                 lambda: bwd(bias=None, po=None, db=torch.empty_like(bias)),   # dbias without a bias
                 lambda: bwd(db=torch.empty(n_pairs - 1, device=DEV)), lambda: bwd(db=torch.empty(n_pairs)),
                 lambda: bwd(db=torch.empty(n_pairs, device=DEV, dtype=torch.float64))):
        with pytest.raises(U2GNNNativeError):
            call()
