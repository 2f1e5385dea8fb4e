"""attention="edges" without a GPU: the adjacency builder and its transpose, the new entry points under the unchanged
ABI version and their refusal of bad arguments before any launch, the layer sizes, and the modules' and CLIs'
fourth mode."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from edges_ref import csr_to_dense, host_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
E_ARG = -1
IDS = [0, 5, 17, 23, 42, 77, 101, 150]
NEW_SYMBOLS = ("u2gnn_csr_attn_fwd", "u2gnn_csr_attn_bwd", "u2gnn_layer_sizes_csr", "u2gnn_layer_fwd_csr",
               "u2gnn_layer_bwd_csr")


def test_adjacency_equals_a_brute_force_set_from_edge_mat():
    store, _, hb, (rowptr, colidx) = host_batch("MUTAG", False, IDS)
    N = hb.N
    assert rowptr.dtype == np.int64 and colidx.dtype == np.int64 and rowptr.shape == (N + 1,)
    assert rowptr[0] == 0 and rowptr[-1] == len(colidx)
    for g, gid in enumerate(IDS):
        s, e = int(hb.offsets[g]), int(hb.offsets[g + 1])
        em = np.asarray(store.graphs[gid].edge_mat).reshape(2, -1)
        want = [{i} for i in range(s, e)]
        for a, b in zip(em[0], em[1]):
            want[int(a)].add(int(b) + s)
        for i in range(s, e):
            row = colidx[rowptr[i]:rowptr[i + 1]]
            assert list(row) == sorted(want[i - s]), (gid, i)     # itself + neighbours, sorted, unique
            assert i in row and row.min() >= s and row.max() < e  # no column leaves the graph's row range


def test_adjacency_draws_nothing_from_the_rng():
    store, _, _, _ = host_batch("MUTAG", False, IDS)
    np.random.seed(11)
    ref = store.assemble(IDS, 4).input_x.copy()
    np.random.seed(11)
    st = np.random.get_state()
    store.adjacency(IDS)
    st2 = np.random.get_state()
    assert st[2] == st2[2] and np.array_equal(st[1], st2[1])
    assert np.array_equal(store.assemble(IDS, 4).input_x, ref)


def test_synthetic_store_adjacency():
    from u2gnn_hip.synthetic import collab_like
    s = collab_like()
    ids = [3, 0, 9]
    rowptr, colidx = s.adjacency(ids)
    off = np.concatenate([[0], np.cumsum(s.n_nodes[ids])])
    A = csr_to_dense(rowptr, colidx, int(off[-1]))
    assert A.max() == 1 and (np.diag(A) == 1).all() and (A == A.T).all()
    for g, gid in enumerate(ids):
        start, nbr, deg, _ = s.graph(gid)
        blk = A[off[g]:off[g + 1], off[g]:off[g + 1]]
        assert np.array_equal(blk.sum(1) - 1, deg)            # simple graphs: degree + the diagonal
        assert A[off[g]:off[g + 1]].sum() == blk.sum()        # nothing outside the diagonal block
        assert all(blk[i, j] for i in range(len(deg)) for j in nbr[start[i]:start[i + 1]])


def test_transpose_round_trips_and_bad_csrs_are_refused():
    from u2gnn_hip.core import Adjacency
    _, _, hb, (rowptr, colidx) = host_batch("MUTAG", False, IDS)
    # a non-symmetric pattern with a duplicate: drop the last entry of row 3, list the first column of row 5 twice
    cols = [list(colidx[rowptr[i]:rowptr[i + 1]]) for i in range(hb.N)]
    cols[3] = cols[3][:-1]
    cols[5] = [cols[5][0]] + cols[5]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    ci = np.concatenate(cols).astype(np.int64)
    A = Adjacency.from_csr(rp, ci, hb.N, device="cpu")
    assert A.nnz == len(ci) and A.N == hb.N
    t_rowptr, t_src, t_eid = A.t_rowptr.numpy(), A.t_src.numpy(), A.t_eid.numpy()
    assert t_rowptr[0] == 0 and t_rowptr[-1] == A.nnz and sorted(t_eid) == list(range(A.nnz))
    for j in range(hb.N):
        for t in range(t_rowptr[j], t_rowptr[j + 1]):
            assert ci[t_eid[t]] == j
            assert rp[t_src[t]] <= t_eid[t] < rp[t_src[t] + 1]
    for bad_rp, bad_ci, n in ((rp[:-1], ci, hb.N),                                   # wrong length
                              (np.concatenate([rp[:-1], [rp[-1] - 1]]), ci, hb.N),   # does not end at nnz
                              (np.concatenate([[0, 5, 3], rp[3:]]), ci, hb.N),       # decreasing
                              (np.concatenate([[1], rp[1:]]), ci, hb.N),             # does not start at 0
                              (rp, np.concatenate([ci[:-1], [hb.N]]), hb.N),         # column == N
                              (rp, np.concatenate([[-1], ci[1:]]), hb.N)):           # negative column
        with pytest.raises(ValueError):
            Adjacency.from_csr(bad_rp, bad_ci, n, device="cpu")


def test_library_exports_csr_entry_points():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.header_symbols("u2gnn_hip.h"), name
    assert lib.u2gnn_abi_version() == _lib.ABI_VERSION == 19


def _layer_args(window=0):
    from u2gnn_hip import _lib
    dims = _lib.LayerDims(437, 100, 256, 1, 0, window, 0)
    fake = ctypes.c_void_p(1 << 40)   # never dereferenced on the host
    params = _lib.LayerParamsC(*([fake.value] * 12))
    seeds = _lib.LayerSeeds(0.5, 1, 2, 3, 4)
    grads = _lib.LayerGrads(*([fake.value] * len(_lib._PKEYS)))
    return dims, fake, params, seeds, grads


def _csr(nnz=1000, **null):
    from u2gnn_hip import _lib
    f = 1 << 40
    return _lib.CsrAttn(*[None if k in null else f for k in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid")], nnz)


def test_csr_layer_sizes():
    """NULL / 0 is u2gnn_layer_sizes; the statistics take the place of the [Np, Np] image; the backward workspace
    grows by exactly 8 bytes per entry."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    by = ctypes.byref
    dims = _layer_args()[0]

    def sizes(fn, *extra):
        c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        rc = fn(by(dims), 0.5, *extra, by(c), by(f), by(b))
        return rc, (c.value, f.value, b.value)
    rc, node = sizes(lib.u2gnn_layer_sizes)
    assert rc == 0
    assert sizes(lib.u2gnn_layer_sizes_csr, 0, 0) == (0, node)
    assert sizes(lib.u2gnn_layer_sizes_csr, 8, 0) == sizes(lib.u2gnn_layer_sizes_seg, 8)
    rc, a = sizes(lib.u2gnn_layer_sizes_csr, 0, 1000)
    rc2, b = sizes(lib.u2gnn_layer_sizes_csr, 0, 5000)
    assert rc == 0 and rc2 == 0
    assert 0 < a[0] == b[0] < node[0] and a[1] == b[1]
    assert b[2] - a[2] == 8 * 4000
    assert sizes(lib.u2gnn_layer_sizes_csr, 0, -1)[0] == E_ARG
    assert sizes(lib.u2gnn_layer_sizes_csr, 8, 1000)[0] == E_ARG      # segments and a CSR together
    wdims = _layer_args(window=19)[0]
    c = ctypes.c_int64()
    assert lib.u2gnn_layer_sizes_csr(by(wdims), 0.5, 0, 1000, by(c), by(c), by(c)) == E_ARG


def test_csr_layer_entry_points_refuse_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_ARG shows that nothing was
    launched."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    by = ctypes.byref
    dims, fake, params, seeds, grads = _layer_args()
    c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.u2gnn_layer_sizes_csr(by(dims), 0.5, 0, 1000, by(c), by(f), by(b)) == 0
    fwd = lambda d, X, A, seg=None, n=0, ws=None: lib.u2gnn_layer_fwd_csr(   # noqa: E731
        by(d), by(params), by(seeds), X, fake, fake, c.value, fake, f.value if ws is None else ws, seg, n,
        by(A) if A is not None else None, None)
    bwd = lambda d, X, A, seg=None, n=0, ws=None: lib.u2gnn_layer_bwd_csr(   # noqa: E731
        by(d), by(params), by(seeds), X, fake, c.value, fake, fake, by(grads), fake, b.value if ws is None else ws,
        seg, n, by(A) if A is not None else None, None, None)
    wdims = _layer_args(window=19)[0]
    for call in (fwd, bwd):
        assert call(dims, None, _csr()) == E_ARG                       # null pointer
        for member in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid"):
            assert call(dims, fake, _csr(**{member: True})) == E_ARG   # a NULL member
        assert call(dims, fake, _csr(nnz=0)) == E_ARG
        assert call(dims, fake, _csr(nnz=-4)) == E_ARG
        assert call(dims, fake, _csr(), fake, 8) == E_ARG              # a CSR together with segments
        assert call(wdims, fake, _csr()) == E_ARG                      # a CSR together with a window
        assert call(dims, fake, _csr(), ws=256) == E_ARG               # short workspace: refused by the planning pass
    # the backward workspace of a larger CSR does not fit the one sized for 1000 entries
    assert bwd(dims, fake, _csr(nnz=10 ** 6)) == E_ARG


def test_csr_kernels_refuse_bad_arguments_before_launching():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    p = ctypes.c_void_p(1 << 40)
    by = ctypes.byref
    fwd = lambda QKV=p, dp=64, A=_csr(), O=p, st=p, pr=0.5: lib.u2gnn_csr_attn_fwd(   # noqa: E731
        QKV, 192, dp, by(A) if A is not None else None, O, 64, st, pr, 1, 100, 128, None)
    bwd = lambda QKV=p, dp=64, A=_csr(), dO=p, dQ=p, ws=p, pr=0.5: lib.u2gnn_csr_attn_bwd(   # noqa: E731
        QKV, 192, dp, by(A) if A is not None else None, p, dO, 64, p, pr, 1, 0.1, dQ, 192, ws, 100, 128, None)
    assert fwd(QKV=None) == E_ARG and fwd(A=None) == E_ARG and fwd(O=None) == E_ARG and fwd(st=None) == E_ARG
    assert fwd(A=_csr(rowptr=True)) == E_ARG and fwd(A=_csr(colidx=True)) == E_ARG
    assert fwd(A=_csr(nnz=0)) == E_ARG and fwd(dp=96) == E_ARG and fwd(pr=1.0) == E_ARG and fwd(pr=-0.1) == E_ARG
    assert bwd(QKV=None) == E_ARG and bwd(dO=None) == E_ARG and bwd(dQ=None) == E_ARG and bwd(ws=None) == E_ARG
    for member in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid"):
        assert bwd(A=_csr(**{member: True})) == E_ARG
    assert bwd(A=None) == E_ARG and bwd(A=_csr(nnz=0)) == E_ARG and bwd(dp=96) == E_ARG and bwd(pr=1.0) == E_ARG
    assert fwd(dp=2048) == -3 and bwd(dp=2048) == -3       # U2GNN_E_SHAPE: wider than the executor's widest layer


def test_kernel_wrappers_refuse_host_tensors():
    import torch
    from u2gnn_hip import U2GNNNativeError
    from u2gnn_hip import kernels as K
    from u2gnn_hip.core import Adjacency
    A = Adjacency.from_csr([0, 1, 2], [0, 1], 2, device="cpu")
    x = torch.zeros(128, 192)
    with pytest.raises(U2GNNNativeError):
        K.csr_attn_fwd(x, 64, A, torch.zeros(128, 64), torch.zeros(128, 2), 0.0, 1, 2, 128)
    with pytest.raises(U2GNNNativeError):
        K.csr_attn_bwd(x, 64, A, torch.zeros(128, 64), torch.zeros(128, 64), torch.zeros(128, 2), 0.0, 1, 0.1,
                       torch.zeros(128, 192), 2, 128)


def test_modules_accept_edges_and_reject_unknown_modes():
    from pytorch_U2GNN_Sup import TransformerU2GNN as Sup
    from pytorch_U2GNN_UnSup import TransformerU2GNN as UnSup
    from u2gnn_hip.core import ATTENTION_MODES, DeviceBatch
    assert ATTENTION_MODES == ("nodes", "neighbors", "graphs", "edges")
    assert DeviceBatch.__dataclass_fields__["adj"].default is None
    for build in (lambda a: Sup(7, 32, 2, 1, 0.5, 1, attention=a),
                  lambda a: UnSup(50, 7, 32, 8, 1, 1, 0.5, "cpu", attention=a)):
        with pytest.raises(ValueError) as e:
            build("edge")
        for mode in ("'nodes'", "'neighbors'", "'graphs'", "'edges'"):
            assert mode in str(e.value)
        assert build("edges").attention == "edges"
        assert build("nodes").attention == "nodes"


@pytest.mark.parametrize("script", ["train_pytorch_U2GNN_Sup.py", "train_pytorch_U2GNN_UnSup.py"])
def test_cli_help_lists_edges(script):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    flat = r.stdout.replace("\n", "").replace(" ", "")
    assert "--attention{nodes,neighbors,graphs,edges}" in flat
    assert re.search(r"edges=eachnodeattendsoveritselfanditsgraphneighbours", flat)
