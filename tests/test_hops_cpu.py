"""``hops`` without a GPU: the H-hop adjacency builder against brute-force distances, the entry types of Adjacency,
the new entry points under the unchanged ABI version and their refusal of bad arguments before any launch, the
modules' one new parameter, the CLIs' flag, and the data-parallel all-reduce that sends hop_bias's region last."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from edges_ref import store_of
from hops_ref import UNREACHED, batch_distances, lists_from_distances

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
E_ARG = -1
IDS = [0, 5, 17, 23, 42, 77, 101, 150]
NEW_SYMBOLS = ("u2gnn_csr_attn_fwd_bias", "u2gnn_csr_attn_bwd_bias", "u2gnn_layer_fwd_csrb", "u2gnn_layer_bwd_csrb",
               "u2gnn_bias_expand", "u2gnn_bias_table_grad", "u2gnn_bias_table_grad_ws_floats")
_DIST = {}


def _mutag():
    store, _ = store_of("MUTAG", False)
    if "D" not in _DIST:
        _DIST["D"] = batch_distances(store, IDS)
    return store, _DIST["D"]


@pytest.mark.parametrize("H", [1, 2, 3])
def test_hop_adjacency_equals_brute_force_distances(H):
    store, D = _mutag()
    rowptr, colidx, etype = store.adjacency(IDS, hops=H)
    assert rowptr.dtype == np.int64 and colidx.dtype == np.int64 and etype.dtype == np.int32
    rp, ci, et = lists_from_distances(D, H)
    assert np.array_equal(rowptr, rp) and np.array_equal(colidx, ci) and np.array_equal(etype, et)
    if H == 1:
        rp1, ci1 = store.adjacency(IDS)
        assert np.array_equal(rowptr, rp1) and np.array_equal(colidx, ci1)
        rows = np.repeat(np.arange(len(rp1) - 1), np.diff(rp1))
        assert np.array_equal(etype, (rows != ci1).astype(np.int32))      # 0 on the diagonal, 1 elsewhere
    else:
        assert etype.max() == H


def test_without_hops_the_return_value_is_todays_pair():
    store, _ = _mutag()
    out = store.adjacency(IDS)
    assert isinstance(out, tuple) and len(out) == 2


def test_31_hops_list_exactly_the_connected_component():
    store, D = _mutag()
    rowptr, colidx, etype = store.adjacency(IDS, hops=31)
    rp, ci, et = lists_from_distances(D, UNREACHED - 1)
    assert np.array_equal(rowptr, rp) and np.array_equal(colidx, ci) and np.array_equal(etype, et)
    assert et.max() <= 31


def test_a_graph_does_not_depend_on_its_batch():
    store, _ = _mutag()
    rowptr, colidx, etype = store.adjacency(IDS, hops=3)
    g = 4
    off = np.concatenate([[0], np.cumsum(store.n_nodes[IDS])])
    rp1, ci1, et1 = store.adjacency([IDS[g]], hops=3)
    s, e = rowptr[off[g]], rowptr[off[g + 1]]
    assert np.array_equal(colidx[s:e] - off[g], ci1) and np.array_equal(etype[s:e], et1)
    assert np.array_equal(rowptr[off[g]:off[g + 1] + 1] - s, rp1)


class _G:
    def __init__(self, n, edges):
        self.n, self.g, self.label = n, list(range(n)), 0
        self.node_features = np.eye(n, 3, dtype=np.float32)
        e = np.array(edges, dtype=np.int64).reshape(-1, 2).T
        self.edge_mat = np.concatenate([e, e[::-1]], 1)     # forward edges, then reversed


def test_disconnected_graph_never_lists_the_other_component():
    from u2gnn_hip.batching import GraphStore
    # graph 0: a path 0-1-2-3 and a separate triangle 4-5-6, and an isolated node 7; graph 1: one edge
    store = GraphStore([_G(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 4)]), _G(2, [(0, 1)])])
    for H in (1, 2, 31):
        rowptr, colidx, etype = store.adjacency([0, 1], hops=H)
        rows = [list(colidx[rowptr[i]:rowptr[i + 1]]) for i in range(10)]
        for i in range(4):
            assert set(rows[i]) <= {0, 1, 2, 3}
        for i in range(4, 7):
            assert rows[i] == [4, 5, 6]
        assert rows[7] == [7] and rows[8] == [8, 9] and rows[9] == [8, 9]
    rowptr, colidx, etype = store.adjacency([0, 1], hops=2)
    assert list(colidx[rowptr[0]:rowptr[1]]) == [0, 1, 2] and list(etype[rowptr[0]:rowptr[1]]) == [0, 1, 2]
    rowptr, colidx, etype = store.adjacency([0, 1], hops=31)
    assert list(colidx[rowptr[0]:rowptr[1]]) == [0, 1, 2, 3] and list(etype[rowptr[0]:rowptr[1]]) == [0, 1, 2, 3]


def test_hops_range_is_validated():
    store, _ = _mutag()
    for bad in (0, -1, 32):
        with pytest.raises(ValueError):
            store.adjacency(IDS, hops=bad)


def test_hop_adjacency_draws_nothing_from_the_rng():
    store, _ = _mutag()
    store.__dict__.pop("_hop_cache", None)              # first use: the lists are computed here
    np.random.seed(11)
    ref = store.assemble(IDS, 4).input_x.copy()
    np.random.seed(11)
    st = np.random.get_state()
    store.adjacency(IDS, hops=3)
    st2 = np.random.get_state()
    assert st[2] == st2[2] and np.array_equal(st[1], st2[1])
    assert np.array_equal(store.assemble(IDS, 4).input_x, ref)


def test_adjacency_keeps_entry_types_and_refuses_bad_ones():
    from u2gnn_hip.core import Adjacency
    store, _ = _mutag()
    rowptr, colidx, etype = store.adjacency(IDS, hops=3)
    N = len(rowptr) - 1
    A = Adjacency.from_csr(rowptr, colidx, N, device="cpu", etype=etype)
    assert A.etype.dtype == torch.int32 and np.array_equal(A.etype.numpy(), etype) and A.n_types == 4
    plain = Adjacency.from_csr(rowptr, colidx, N, device="cpu")
    assert plain.etype is None and plain.n_types == 0
    bad_neg, bad_big = etype.copy(), etype.copy()
    bad_neg[3], bad_big[3] = -1, 32
    for bad in (etype[:-1], bad_neg, bad_big):
        with pytest.raises(ValueError):
            Adjacency.from_csr(rowptr, colidx, N, device="cpu", etype=bad)
    ok = etype.copy()
    ok[3] = 31
    assert Adjacency.from_csr(rowptr, colidx, N, device="cpu", etype=ok).n_types == 32


def test_library_exports_the_bias_entry_points_under_abi_19():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.header_symbols("u2gnn_hip.h"), name
    assert lib.u2gnn_abi_version() == _lib.ABI_VERSION == 19
    assert _lib.BIAS_TYPES_MAX == 32


def _csr(nnz=1000, **null):
    from u2gnn_hip import _lib
    f = 1 << 40
    return _lib.CsrAttn(*[None if k in null else f for k in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid")], nnz)


def test_bias_attention_kernels_refuse_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_ARG shows that nothing was
    launched (the method of tests/test_edges_mode_cpu.py)."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    p = ctypes.c_void_p(1 << 40)
    by = ctypes.byref
    fwd = lambda QKV=p, dp=64, A=_csr(), O=p, st=p, pr=0.5, bias=p: lib.u2gnn_csr_attn_fwd_bias(   # noqa: E731
        QKV, 192, dp, by(A) if A is not None else None, bias, O, 64, st, pr, 1, 100, 128, None)
    bwd = lambda QKV=p, dp=64, A=_csr(), dO=p, dQ=p, ws=p, pr=0.5, bias=p, db=p: lib.u2gnn_csr_attn_bwd_bias(  # noqa: E731
        QKV, 192, dp, by(A) if A is not None else None, bias, p, dO, 64, p, pr, 1, 0.1, dQ, 192, ws, db, 100, 128,
        None)
    assert fwd(QKV=None) == E_ARG and fwd(A=None) == E_ARG and fwd(O=None) == E_ARG and fwd(st=None) == E_ARG
    assert fwd(A=_csr(rowptr=True)) == E_ARG and fwd(A=_csr(colidx=True)) == E_ARG
    assert fwd(A=_csr(nnz=0)) == E_ARG and fwd(dp=96) == E_ARG and fwd(pr=1.0) == E_ARG
    assert bwd(QKV=None) == E_ARG and bwd(dO=None) == E_ARG and bwd(dQ=None) == E_ARG and bwd(ws=None) == E_ARG
    for member in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid"):
        assert bwd(A=_csr(**{member: True})) == E_ARG
    assert bwd(A=None) == E_ARG and bwd(A=_csr(nnz=0)) == E_ARG and bwd(dp=96) == E_ARG and bwd(pr=1.0) == E_ARG
    assert bwd(bias=None, db=p) == E_ARG                       # a bias gradient without a bias
    assert bwd(A=None, bias=p) == E_ARG                        # a bias without a CSR


def _layer_args(window=0):
    from u2gnn_hip import _lib
    dims = _lib.LayerDims(437, 100, 256, 1, 0, window, 0)
    fake = ctypes.c_void_p(1 << 40)   # never dereferenced on the host
    params = _lib.LayerParamsC(*([fake.value] * 12))
    seeds = _lib.LayerSeeds(0.5, 1, 2, 3, 4)
    grads = _lib.LayerGrads(*([fake.value] * len(_lib._PKEYS)))
    return dims, fake, params, seeds, grads


def test_bias_layer_entry_points_refuse_bad_arguments_before_launching():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    by = ctypes.byref
    dims, fake, params, seeds, grads = _layer_args()
    c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.u2gnn_layer_sizes_csr(by(dims), 0.5, 0, 1000, by(c), by(f), by(b)) == 0
    fwd = lambda d, X, A, bias, seg=None, n=0, ws=None: lib.u2gnn_layer_fwd_csrb(   # noqa: E731
        by(d), by(params), by(seeds), X, fake, fake, c.value, fake, f.value if ws is None else ws, seg, n,
        by(A) if A is not None else None, bias, None)
    bwd = lambda d, X, A, bias, seg=None, n=0, ws=None, db=fake: lib.u2gnn_layer_bwd_csrb(   # noqa: E731
        by(d), by(params), by(seeds), X, fake, c.value, fake, fake, by(grads), fake, b.value if ws is None else ws,
        seg, n, by(A) if A is not None else None, bias, db if bias is not None else None, None, None)
    wdims = _layer_args(window=19)[0]
    for call in (fwd, bwd):
        assert call(dims, None, _csr(), fake) == E_ARG                        # null pointer
        assert call(dims, fake, None, fake) == E_ARG                          # a bias without a CSR
        assert call(dims, fake, None, fake, fake, 8) == E_ARG                 # ... also with segments instead
        for member in ("rowptr", "colidx", "t_rowptr", "t_src", "t_eid"):
            assert call(dims, fake, _csr(**{member: True}), fake) == E_ARG    # a NULL member
        assert call(dims, fake, _csr(nnz=0), fake) == E_ARG
        assert call(wdims, fake, _csr(), fake) == E_ARG                       # a window
        assert call(dims, fake, _csr(), fake, ws=256) == E_ARG                # short workspace
    assert lib.u2gnn_layer_bwd_csrb(by(dims), by(params), by(seeds), fake, fake, c.value, fake, fake, by(grads), fake,
                                    b.value, None, 0, by(_csr()), None, fake, None, None) == E_ARG   # dbias, no bias


def test_bias_table_kernels_refuse_bad_arguments_before_launching():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    p = ctypes.c_void_p(1 << 40)
    ex = lambda tables=p, R=4, T=3, et=p, nnz=1000, out=p, ld=1000: lib.u2gnn_bias_expand(   # noqa: E731
        tables, R, T, et, nnz, out, ld, None)
    assert ex(tables=None) == E_ARG and ex(et=None) == E_ARG and ex(out=None) == E_ARG
    assert ex(R=0) == E_ARG and ex(T=0) == E_ARG and ex(T=33) == E_ARG and ex(nnz=0) == E_ARG and ex(ld=999) == E_ARG
    need = lib.u2gnn_bias_table_grad_ws_floats(4, 3, 10000)
    assert need == 4 * 3 * 3                                    # 3 blocks of 4096 entries
    for bad in ((0, 3, 10), (4, 0, 10), (4, 33, 10), (4, 3, 0)):
        assert lib.u2gnn_bias_table_grad_ws_floats(*bad) == -1
    tg = lambda db=p, ld=10000, R=4, T=3, et=p, nnz=10000, dt=p, ws=p, n=need: lib.u2gnn_bias_table_grad(  # noqa: E731
        db, ld, R, T, et, nnz, dt, ws, n, None)
    assert tg(db=None) == E_ARG and tg(et=None) == E_ARG and tg(dt=None) == E_ARG and tg(ws=None) == E_ARG
    assert tg(R=0) == E_ARG and tg(T=0) == E_ARG and tg(T=33) == E_ARG and tg(nnz=0) == E_ARG
    assert tg(ld=9996) == E_ARG and tg(ld=10001) == E_ARG       # shorter than a row; not a multiple of 4
    assert tg(n=need - 1) == E_ARG                              # a workspace that is too small


def test_kernel_wrappers_refuse_host_tensors():
    from u2gnn_hip import U2GNNNativeError
    from u2gnn_hip import kernels as K
    with pytest.raises(U2GNNNativeError):
        K.bias_expand(torch.zeros(2, 3), torch.zeros(8, dtype=torch.int32), torch.zeros(2, 8))
    with pytest.raises(U2GNNNativeError):
        K.bias_table_grad(torch.zeros(2, 8), torch.zeros(8, dtype=torch.int32), torch.zeros(2, 3))


def _models(**kw):
    from pytorch_U2GNN_Sup import TransformerU2GNN as Sup
    from pytorch_U2GNN_UnSup import TransformerU2GNN as UnSup
    return (lambda: Sup(7, 32, 2, 2, 0.5, 2, **kw)), (lambda: UnSup(50, 7, 32, 8, 2, 2, 0.5, "cpu", **kw))


@pytest.mark.parametrize("which", [0, 1])
def test_modules_gain_exactly_one_zero_parameter(which):
    torch.manual_seed(5)
    nodes = _models()[which]()
    torch.manual_seed(5)
    plain = _models(attention="edges")[which]()
    torch.manual_seed(5)
    hop = _models(attention="edges", hops=2)[which]()
    assert list(plain.state_dict()) == list(nodes.state_dict())                 # without hops: today's keys
    assert set(hop.state_dict()) - set(plain.state_dict()) == {"hop_bias"}
    assert set(plain.state_dict()) <= set(hop.state_dict())
    assert hop.hop_bias.shape == (2, 2, 3) and float(hop.hop_bias.abs().max()) == 0.0
    for k, v in plain.state_dict().items():
        assert torch.equal(v, hop.state_dict()[k]), k
    names = [n for n, _ in hop.named_parameters()]
    assert names[-1] == "hop_bias" and names[:-1] == [n for n, _ in plain.named_parameters()]
    assert len(list(hop.parameters())) == len(list(plain.parameters())) + 1
    assert not hasattr(plain, "hop_bias")


@pytest.mark.parametrize("which", [0, 1])
def test_hops_needs_edges_mode(which):
    for mode in ("nodes", "graphs", "neighbors"):
        with pytest.raises(ValueError, match="edges"):
            _models(attention=mode, hops=2)[which]()
    for bad in (0, 32, -1):
        with pytest.raises(ValueError):
            _models(attention="edges", hops=bad)[which]()


def test_unsup_trains_hop_bias():
    m = _models(attention="edges", hops=2)[1]()
    assert m.trainable_names()[-1] == "hop_bias" and "ss.weight" in m.trainable_names()
    assert "hop_bias" not in _models(attention="edges")[1]().trainable_names()


@pytest.mark.parametrize("script", ["train_pytorch_U2GNN_Sup.py", "train_pytorch_U2GNN_UnSup.py"])
def test_cli_lists_hops_and_refuses_it_without_edges(script):
    run = lambda *a: subprocess.run([sys.executable, os.path.join(PKG, script), *a], capture_output=True,  # noqa: E731
                                    text=True, timeout=300)
    r = run("--help")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--hops" in r.stdout
    r = run("--hops", "2", "--attention", "nodes")
    assert r.returncode == 2 and "--hops needs --attention edges" in r.stderr
    if "UnSup" in script:
        r = run("--hops", "2", "--attention", "edges", "--world_size", "2")
        assert r.returncode == 2 and "--world_size" in r.stderr


def _dp_worker(rank, world, port):
    sys.path[:0] = [os.path.join(REPO, "graph-transformer_amd"), REPO]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TORCHELASTIC_USE_AGENT_STORE="True")
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.core import FlatParams
    from u2gnn_hip.dp import GradAllReduce, OverlappedGradAllReduce
    torch.manual_seed(1)
    f2 = FlatParams(TransformerU2GNN(7, 32, 2, 2, 0.5, 2, attention="edges", hops=2))
    assert f2.names[-1] == "hop_bias"
    mine_g = torch.randn(f2.gflat.numel(), generator=torch.Generator().manual_seed(7 + rank))
    f2.gflat.copy_(mine_g)
    GradAllReduce(bucket_mb=0.001)(f2)
    g_after = f2.gflat.clone()
    for mb in (9.0, 1e-5, 0.02):
        ar = OverlappedGradAllReduce(f2, bucket_mb=mb)
        lo, hi = ar.span["hop_bias"]
        assert hi - lo == 2 * 2 * 3 and hi <= f2.gflat.numel()
        for rep in range(2):
            f2.gflat.copy_(mine_g)
            for l in reversed(range(2)):
                for t in reversed(range(2)):
                    ar.layer_done(f"u2gnn_layers.{l}.layers.{t}.")
            # hop_bias's gradient exists only after the last layer's backward: no collective issued so far covers it
            assert ar.launched and all(b <= lo or a >= hi for a, b in ar.launched), (mb, ar.launched, lo, hi)
            ar(f2)
            assert torch.equal(f2.gflat, g_after), mb
            assert not ar.pending and not ar.launched
    dist.destroy_process_group()


def test_gloo_world2_overlapped_allreduce_sends_hop_bias_last(rdzv_port):
    mp.spawn(_dp_worker, args=(2, rdzv_port), nprocs=2, join=True)
