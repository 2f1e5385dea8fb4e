"""The two launches of ``centrality`` alone: u2gnn_gather_rows_emb against numpy bit for bit on every route of the
gather, u2gnn_class_rows_grad against a float64 sum under the bound of a fixed-order fp32 sum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from u2gnn_hip import U2GNNNativeError  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402

DEV = "cuda"
RB = K.CLASS_ROWS_CHUNK
SRC_ROWS = 23
# (d, ld_src, d_pad): the multi-row XCD kernel with wide stores, MODE 1, the multi-row kernel again (C4's width), MODE 2,
# MODE 0 -- and (6, 7, 6) with an 8-float destination row: the multi-row kernel's dword stores (d_pad % 4 != 0)
ROUTES = [(7, 7, 64), (64, 64, 64), (367, 367, 384), (600, 601, 640), (1100, 1100, 1152), (6, 7, 6)]


def _forward_case(d, ld_src, d_pad, n_rows, stride, n_classes, seed):
    rng = np.random.RandomState(seed)
    src = rng.randn(SRC_ROWS, ld_src).astype(np.float32)
    emb = rng.randn(n_classes, d).astype(np.float32)
    D = n_classes - 1
    deg = rng.randint(0, D + 4, size=SRC_ROWS).astype(np.int32)      # degrees above D take row D
    deg[0], deg[1], deg[2] = -3, D + 100, 0                           # a negative degree takes row 0
    idx = rng.randint(0, SRC_ROWS, size=(8, stride)).astype(np.int64)
    idx[0, 0] = 0
    if n_rows > 1:
        idx[1, 0], idx[2, 0] = 1, 2
    return src, emb, deg, idx


@pytest.mark.parametrize("n_classes", [1, 2, 64])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n_rows", [1, 5])
@pytest.mark.parametrize("d,ld_src,d_pad", ROUTES)
def test_gather_rows_emb_is_one_ieee_add_on_every_route(d, ld_src, d_pad, n_rows, stride, n_classes):
    src, emb, deg, idx = _forward_case(d, ld_src, d_pad, n_rows, stride, n_classes, 100 * d + 10 * n_rows + stride)
    n_pad, ld_dst = 8, (d_pad + 3) // 4 * 4
    dst = torch.full((n_pad, ld_dst), float("nan"), device=DEV)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    K.gather_rows_emb(t(src), t(idx), stride, dst, n_rows, n_pad, d, d_pad, t(deg), t(emb), err)
    want = np.zeros((n_pad, d_pad), dtype=np.float32)
    s = idx[:n_rows, 0]
    want[:n_rows, :d] = src[s, :d] + emb[np.clip(deg[s], 0, n_classes - 1)]      # fp32 + fp32, one rounding
    got = dst.cpu().numpy()[:, :d_pad]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert int(err.item()) == 0
    if ld_dst > d_pad:                                                # beyond d_pad nothing is written
        assert np.isnan(dst.cpu().numpy()[:, d_pad:]).all()


@pytest.mark.parametrize("d,ld_src,d_pad", ROUTES)
def test_gather_rows_emb_out_of_range_index_gives_a_zero_row_and_sets_err(d, ld_src, d_pad):
    src, emb, deg, idx = _forward_case(d, ld_src, d_pad, 5, 1, 4, d)
    idx[3, 0] = SRC_ROWS           # one past the end
    idx[4, 0] = -1
    ld_dst = (d_pad + 3) // 4 * 4
    dst = torch.full((8, ld_dst), float("nan"), device=DEV)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    K.gather_rows_emb(t(src), t(idx), 1, dst, 5, 8, d, d_pad, t(deg), t(emb), err)
    got = dst.cpu().numpy()[:, :d_pad]
    want = np.zeros((8, d_pad), dtype=np.float32)
    want[:3, :d] = src[idx[:3, 0], :d] + emb[np.clip(deg[idx[:3, 0]], 0, 3)]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and int(err.item()) == 1


def test_gather_rows_emb_with_an_unaligned_table_leaves_mode_1():
    """A table whose rows are not 16-byte aligned (a view one float into a buffer) takes the next route: same bits."""
    src, emb, deg, idx = _forward_case(64, 64, 64, 5, 1, 4, 9)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    buf = torch.zeros(4 * 64 + 1, device=DEV)
    table = buf[1:].view(4, 64)
    table.copy_(t(emb))
    out = []
    for e in (t(emb), table):
        dst = torch.empty(8, 64, device=DEV)
        K.gather_rows_emb(t(src), t(idx), 1, dst, 5, 8, 64, 64, t(deg), e)
        out.append(dst.cpu())
    assert torch.equal(out[0], out[1])


def _classes_of(idx, deg, n_classes, n_rows, src_rows):
    """Row i's class (its index is idx[i, 0] = the flat idx[i * stride]); -1: out of range, the row counts nowhere."""
    s = idx[:n_rows, 0]
    ok = (s >= 0) & (s < src_rows)
    return np.where(ok, np.clip(deg[np.clip(s, 0, src_rows - 1)], 0, n_classes - 1), -1)


def _grad_case(n_rows, d, n_classes, stride, kind, seed):
    """dX [n_rows, ld] N(0, 1), the index [n_rows, stride] and the degrees; kind: "mixed", "one" (all rows in one
    class), "repeat" (few distinct nodes, repeated), "oob" (some indices out of range)."""
    rng = np.random.RandomState(seed)
    src_rows = 37
    ld = d + 3
    dX = rng.randn(n_rows, ld).astype(np.float32)
    deg = rng.randint(-1, n_classes + 2, size=src_rows).astype(np.int32)
    idx = rng.randint(0, 3 if kind == "repeat" else src_rows, size=(n_rows, stride)).astype(np.int64)
    if kind == "one":
        deg[:] = min(1, n_classes - 1)
    if kind == "oob":
        idx[::3, 0] = src_rows
        idx[1::7, 0] = -5
    return dX, deg, idx, src_rows


def _run_grad(dX, deg, idx, src_rows, n_rows, d, n_classes, stride):
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    demb = torch.full((n_classes, d), float("nan"), device=DEV)
    K.class_rows_grad(t(dX), t(idx), stride, t(deg), src_rows, n_rows, d, demb)
    return demb.cpu().numpy()


def _check_grad(n_rows, d, n_classes, stride, kind, seed):
    dX, deg, idx, src_rows = _grad_case(n_rows, d, n_classes, stride, kind, seed)
    got = _run_grad(dX, deg, idx, src_rows, n_rows, d, n_classes, stride)
    cls = _classes_of(idx, deg, n_classes, n_rows, src_rows)
    x = dX[:, :d].astype(np.float64)
    # |ours - f64| <= K 2^-24 sum|terms| (1 + 1e-3): a value passes through at most K = class_rows_k(n_rows) additions
    # (chain adds and tree levels), each with relative error <= 2^-24; the factor covers the second-order terms
    bound_k = K.class_rows_k(n_rows) * 2.0 ** -24 * (1 + 1e-3)
    worst = 0.0
    for c in range(n_classes):
        rows = cls == c
        ref, mag = x[rows].sum(0), np.abs(x[rows]).sum(0)
        if not rows.any():
            assert np.array_equal(got[c].view(np.uint32), np.zeros(d, dtype=np.uint32)), c      # exactly +0.0
        assert (np.abs(got[c] - ref) <= bound_k * mag).all(), (c, np.abs(got[c] - ref).max(), (bound_k * mag).min())
        worst = max(worst, float((np.abs(got[c] - ref) / np.maximum(bound_k * mag, 1e-300)).max()) if rows.any() else 0)
    again = _run_grad(dX, deg, idx, src_rows, n_rows, d, n_classes, stride)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))                           # deterministic
    return worst


@pytest.mark.parametrize("n_classes", [1, 2, 64])
@pytest.mark.parametrize("d", [1, 7, 65, 367])
@pytest.mark.parametrize("n_rows", [1, RB - 1, RB, RB + 1, 3 * RB + 5])
def test_class_rows_grad_within_the_fixed_order_bound(n_rows, d, n_classes):
    worst = _check_grad(n_rows, d, n_classes, 1, "mixed", 1000 * n_rows + 10 * d + n_classes)
    print(f"class_rows_grad n_rows={n_rows} d={d} classes={n_classes}: worst |err| / bound {worst:.3g}")


@pytest.mark.parametrize("kind,stride", [("one", 1), ("mixed", 3), ("repeat", 1), ("oob", 1), ("oob", 3)])
@pytest.mark.parametrize("n_classes", [2, 64])
def test_class_rows_grad_cases(kind, stride, n_classes):
    """All rows in one class (every other class exactly 0.0), idx_stride 3, repeated indices, out-of-range indices
    (they contribute nothing)."""
    _check_grad(3 * RB + 5, 65, n_classes, stride, kind, 77 + n_classes + stride)


def test_class_rows_grad_reads_padded_rows_and_a_strided_table():
    """dX as the stack hands it over ([Np, dp] padded, only n_rows x d read) and demb as a view with a wider row."""
    n_rows, d, dp = RB + 9, 7, 64
    rng = np.random.RandomState(5)
    dX = np.full((RB * 2, dp), np.nan, dtype=np.float32)
    dX[:n_rows, :d] = rng.randn(n_rows, d)
    deg = rng.randint(0, 6, size=n_rows).astype(np.int32)
    idx = rng.permutation(n_rows).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    wide = torch.full((4, 12), 7.0, device=DEV)
    K.class_rows_grad(t(dX), t(idx), 1, t(deg), n_rows, n_rows, d, wide[:, :d])
    got = wide.cpu().numpy()
    assert (got[:, d:] == 7.0).all() and np.isfinite(got).all()
    cls = np.clip(deg[idx], 0, 3)
    for c in range(4):
        ref = dX[:n_rows, :d][cls == c].astype(np.float64).sum(0)
        assert np.allclose(got[c, :d], ref, rtol=0, atol=K.class_rows_k(n_rows) * 2.0 ** -24 * np.abs(dX[:n_rows, :d]).sum())


def test_bad_arguments_raise_through_the_wrappers():
    dX = torch.zeros(8, 64, device=DEV)
    ix = torch.zeros(8, dtype=torch.int64, device=DEV)
    deg = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(U2GNNNativeError):
        K.class_rows_grad(dX, ix, 1, deg, 8, 8, 7, torch.zeros(65, 7, device=DEV))          # 65 classes
    with pytest.raises(U2GNNNativeError):
        K.class_rows_grad(dX, ix, 1, deg, 8, 8, 65, torch.zeros(3, 65, device=DEV))         # ld < d
    with pytest.raises(U2GNNNativeError):
        K.class_rows_grad(dX, ix, 1, deg.long(), 8, 8, 7, torch.zeros(3, 7, device=DEV))    # degrees must be int32
    with pytest.raises(U2GNNNativeError):
        K.gather_rows_emb(dX, ix, 1, torch.zeros(8, 64, device=DEV), 8, 8, 64, 64, deg, torch.zeros(3, 7, device=DEV))
    with pytest.raises(U2GNNNativeError):
        K.gather_rows_emb(dX, ix, 1, torch.zeros(8, 64, device=DEV), 9, 8, 64, 64, deg, torch.zeros(3, 64, device=DEV))
