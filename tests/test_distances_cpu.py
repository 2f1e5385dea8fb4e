"""``distances`` without a GPU: the host pair types against brute-force distances, a batch as the concatenation of its
graphs' blocks, PairTypes' validation, the modules' one new parameter and their refusals, the CLIs' flag, the four new
entry points under the unchanged ABI version and their refusal of bad arguments before any launch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from edges_ref import store_of
from hops_ref import UNREACHED, graph_distances

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
E_ARG = -1
NEW_SYMBOLS = ("u2gnn_segment_attn_fwd_bias", "u2gnn_segment_attn_bwd_bias", "u2gnn_layer_fwd_segb",
               "u2gnn_layer_bwd_segb")


def _expected(store, ids, H):
    """(pair_off, etype) from Floyd-Warshall: min(D, H), UNREACHED -> H, every graph's block row-major."""
    blocks = []
    for g in ids:
        D = graph_distances(store, int(g))
        assert D.max() <= UNREACHED
        blocks.append(np.minimum(D, H).reshape(-1))              # UNREACHED = 255 > H: clipped to H as well
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
    return off, np.concatenate(blocks).astype(np.int64)


@pytest.mark.parametrize("dataset,count,H", [("MUTAG", 188, 3), ("PTC", 200, 5)])
def test_store_distances_equal_brute_force(dataset, count, H):
    store, _ = store_of(dataset, False)
    ids = np.arange(count)
    pair_off, etype = store.distances(ids, H)
    assert pair_off.dtype == np.int64 and etype.dtype == np.int32
    off, ref = _expected(store, ids, H)
    assert np.array_equal(pair_off, off) and np.array_equal(etype, ref)
    assert etype.min() == 0 and etype.max() == H
    if dataset == "PTC":   # clipping is exercised: some pair of these graphs lies further apart than H
        assert max(int(np.where(D < UNREACHED, D, 0).max()) for D in
                   (graph_distances(store, g) for g in range(0, count, 10))) > H


class _G:
    def __init__(self, n, edges):
        self.n, self.g, self.label = n, list(range(n)), 0
        self.node_features = np.eye(n, 3, dtype=np.float32)
        e = np.array(edges, dtype=np.int64).reshape(-1, 2).T
        self.edge_mat = np.concatenate([e, e[::-1]], 1)     # forward edges, then reversed


def test_two_components_and_an_isolated_node():
    from u2gnn_hip.batching import GraphStore
    # a path 0-1-2-3, a separate triangle 4-5-6 and an isolated node 7
    store = GraphStore([_G(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 4)]), _G(2, [(0, 1)])])
    for H in (1, 2, 31):
        pair_off, etype = store.distances([0, 1], H)
        off, ref = _expected(store, [0, 1], H)
        assert np.array_equal(pair_off, off) and np.array_equal(etype, ref)
        B = etype[:64].reshape(8, 8)
        assert (B[:4, 4:] == H).all() and (B[4:7, :4] == H).all()          # no path: index H
        assert (B[7, :7] == H).all() and (B[:7, 7] == H).all() and B[7, 7] == 0
        assert list(B[0, :4]) == [0, 1, min(2, H), min(3, H)]
        assert list(etype[64:]) == [0, 1, 1, 0]


def test_a_batch_is_the_concatenation_of_its_graphs_blocks():
    store, _ = store_of("MUTAG", False)
    ids = [5, 0, 150, 5, 42]                                               # any order, a repeat
    pair_off, etype = store.distances(ids, 3)
    n = store.n_nodes[ids]
    assert np.array_equal(pair_off, np.concatenate([[0], np.cumsum(n * n)]))
    for b, g in enumerate(ids):
        po1, et1 = store.distances([g], 3)
        assert np.array_equal(po1, [0, n[b] * n[b]])
        assert np.array_equal(etype[pair_off[b]:pair_off[b + 1]], et1)
    assert store._pair_cache[3][5].dtype == np.uint8                       # kept per (H, graph) as uint8
    out = np.full(int(pair_off[-1]) + 7, -1, dtype=np.int32)               # into a caller's buffer
    po2, et2 = store.distances(ids, 3, out=out)
    assert np.array_equal(et2, etype) and et2.base is out and (out[int(pair_off[-1]):] == -1).all()


def test_distances_range_and_rng():
    store, _ = store_of("MUTAG", False)
    for bad in (0, -1, 32, 2.5):
        with pytest.raises(ValueError):
            store.distances([0, 1], bad)
    store.__dict__.pop("_pair_cache", None)
    store.__dict__.pop("_hop_cache", None)                                 # first use: the blocks are computed here
    np.random.seed(11)
    st = np.random.get_state()
    store.distances([0, 5, 17], 4)
    st2 = np.random.get_state()
    assert st[2] == st2[2] and np.array_equal(st[1], st2[1])


def test_pair_types_validate_on_the_host():
    from u2gnn_hip.core import PairTypes
    from u2gnn_hip.pattern import BIAS_ENTRIES_MAX
    store, _ = store_of("MUTAG", False)
    ids = [0, 5, 17]
    N = int(store.n_nodes[ids].sum())
    pt = PairTypes.from_store(store, ids, N, "cpu", 3)
    po, et = store.distances(ids, 3)
    assert pt.N == N and pt.n_pairs == len(et) and pt.n_types == 4
    assert pt.pair_off.dtype == torch.int64 and pt.etype.dtype == torch.int32
    assert np.array_equal(pt.pair_off.numpy(), po) and np.array_equal(pt.etype.numpy(), et)
    pa = PairTypes.from_arrays(po, et, N, "cpu")
    assert torch.equal(pa.etype, pt.etype) and torch.equal(pa.pair_off, pt.pair_off) and pa.n_types == 4
    bad_start, bad_end, bad_order = po.copy(), po.copy(), po.copy()
    bad_start[0], bad_end[-1] = 1, po[-1] - 1
    bad_order[1], bad_order[2] = po[2], po[1]
    for bad in (bad_start, bad_end, bad_order):
        with pytest.raises(ValueError):
            PairTypes.from_arrays(bad, et, N, "cpu")
    neg, big = et.copy(), et.copy()
    neg[3], big[3] = -1, 32
    for bad in (neg, big):
        with pytest.raises(ValueError):
            PairTypes.from_arrays(po, bad, N, "cpu")
    ok = et.copy()
    ok[3] = 31
    assert PairTypes.from_arrays(po, ok, N, "cpu").n_types == 32
    with pytest.raises(ValueError):
        PairTypes.from_arrays([0, 0], np.zeros(0, dtype=np.int32), N, "cpu")   # no pair
    with pytest.raises(ValueError):
        PairTypes.from_store(store, ids, N + 1, "cpu", 3)                      # not this batch's rows
    assert BIAS_ENTRIES_MAX == 4096 * 112 * 256


def test_segments_pattern_carries_pairs_and_keeps_its_key():
    from u2gnn_hip.core import AttnPattern, PairTypes
    store, _ = store_of("MUTAG", False)
    ids = [0, 5]
    N = int(store.n_nodes[ids].sum())
    pt = PairTypes.from_store(store, ids, N, "cpu", 2)
    off = torch.tensor([0, int(store.n_nodes[0]), N])
    plain, with_pairs = AttnPattern.segments(off), AttnPattern.segments(off, pt)
    assert plain.pairs is None and with_pairs.pairs is pt
    assert with_pairs.key == plain.key and with_pairs.nnz == 0            # the buffer sizes do not depend on the bias
    with pytest.raises(ValueError):
        AttnPattern("window", 5, pt)


def _models(**kw):
    from pytorch_U2GNN_Sup import TransformerU2GNN as Sup
    from pytorch_U2GNN_UnSup import TransformerU2GNN as UnSup
    return (lambda: Sup(7, 32, 2, 2, 0.5, 2, **kw)), (lambda: UnSup(50, 7, 32, 8, 2, 2, 0.5, "cpu", **kw))


@pytest.mark.parametrize("which", [0, 1])
def test_modules_gain_exactly_one_zero_parameter(which):
    torch.manual_seed(5)
    nodes = _models()[which]()
    torch.manual_seed(5)
    plain = _models(attention="graphs")[which]()
    torch.manual_seed(5)
    dist = _models(attention="graphs", distances=3)[which]()
    after = torch.rand(1)                                                  # torch's generator is not touched
    torch.manual_seed(5)
    _models(attention="graphs")[which]()
    assert torch.equal(after, torch.rand(1))
    assert list(plain.state_dict()) == list(nodes.state_dict())           # without distances: the reference's keys
    assert set(dist.state_dict()) - set(plain.state_dict()) == {"hop_bias"}
    assert dist.hop_bias.shape == (2, 2, 4) and float(dist.hop_bias.abs().max()) == 0.0
    for k, v in plain.state_dict().items():
        assert torch.equal(v, dist.state_dict()[k]), k
    names = [n for n, _ in dist.named_parameters()]
    assert names[-1] == "hop_bias" and names[:-1] == [n for n, _ in plain.named_parameters()]
    assert len(list(dist.parameters())) == len(list(plain.parameters())) + 1
    assert not hasattr(plain, "hop_bias") and dist.distances == 3 and dist.hops is None and plain.distances is None
    if which == 1:
        assert dist.trainable_names()[-1] == "hop_bias" and "hop_bias" not in plain.trainable_names()


@pytest.mark.parametrize("which", [0, 1])
def test_distances_misuse_raises(which):
    for mode in ("nodes", "neighbors", "edges"):
        with pytest.raises(ValueError, match="graphs"):
            _models(attention=mode, distances=2)[which]()
    with pytest.raises(ValueError):
        _models(attention="graphs", distances=2, hops=2)[which]()         # (hops itself refuses "graphs", naming edges)
    with pytest.raises(ValueError, match="exclude"):
        from u2gnn_hip.core import check_distances
        check_distances(2, "graphs", hops=2)
    for bad in (0, 32, -1, 2.5):
        with pytest.raises(ValueError):
            _models(attention="graphs", distances=bad)[which]()


def test_encoder_stack_checks_the_batchs_pair_types():
    """A batch without pair types, with those of another batch, or with types beyond H: ValueError before any launch
    (_pattern runs on the host)."""
    from u2gnn_hip.core import DeviceBatch, EncoderStack, PairTypes
    store, _ = store_of("MUTAG", False)
    ids = [0, 5, 17]
    n = store.n_nodes[ids]
    N = int(n.sum())
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]))
    z = torch.zeros(N, 7)
    b = DeviceBatch(N, 3, torch.zeros(N, 5, dtype=torch.int64), z, off, torch.arange(N), torch.ones(N),
                    rows_contiguous=True)
    stack = EncoderStack([], 7, 32, 2, 2, attention="graphs", distances=2)
    with pytest.raises(ValueError, match="pair types"):
        stack._pattern(b)
    b.pairs = PairTypes.from_store(store, ids, N, "cpu", 3)
    with pytest.raises(ValueError, match="go up to 3"):
        stack._pattern(b)
    b.pairs = PairTypes.from_store(store, ids[:2], int(n[:2].sum()), "cpu", 2)
    with pytest.raises(ValueError, match="rows"):
        stack._pattern(b)
    b.pairs = PairTypes.from_store(store, ids, N, "cpu", 2)
    pattern, W, _ = stack._pattern(b)
    assert pattern.kind == "segments" and pattern.pairs is b.pairs and W == 1
    b.pairs = PairTypes.from_store(store, ids, N, "cpu", 1)               # fewer types: fine
    assert stack._pattern(b)[0].pairs.n_types == 2
    plain = EncoderStack([], 7, 32, 2, 2, attention="graphs")
    assert plain._pattern(b)[0].pairs is None                             # the other modes never read it


@pytest.mark.parametrize("script", ["train_pytorch_U2GNN_Sup.py", "train_pytorch_U2GNN_UnSup.py"])
def test_cli_lists_distances_and_refuses_misuse(script):
    run = lambda *a: subprocess.run([sys.executable, os.path.join(PKG, script), *a], capture_output=True,  # noqa: E731
                                    text=True, timeout=300)
    r = run("--help")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--distances" in r.stdout and "--hops" in r.stdout
    for mode in ("nodes", "edges"):
        r = run("--distances", "2", "--attention", mode)
        assert r.returncode == 2 and "--distances needs --attention graphs" in r.stderr
    r = run("--distances", "2", "--attention", "graphs", "--hops", "2")
    assert r.returncode == 2                                              # (--hops needs edges, or the pair excludes)
    r = run("--distances", "32", "--attention", "graphs")
    assert r.returncode == 2 and "0..31" in r.stderr
    r = run("--hops", "2", "--attention", "graphs")
    assert r.returncode == 2 and "--hops needs --attention edges" in r.stderr
    if "UnSup" in script:
        r = run("--distances", "2", "--attention", "graphs", "--world_size", "2")
        assert r.returncode == 2 and "--world_size" in r.stderr


def test_library_exports_the_new_entry_points_under_abi_19():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.header_symbols("u2gnn_hip.h"), name
    assert lib.u2gnn_abi_version() == _lib.ABI_VERSION == 19


def test_segment_bias_kernels_refuse_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_ARG shows that nothing was
    launched (the method of tests/test_hops_cpu.py)."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    p = ctypes.c_void_p(1 << 40)
    fwd = lambda QKV=p, dp=64, off=p, n=3, po=p, npair=100, bias=p, O=p, st=p, pr=0.5: (   # noqa: E731
        lib.u2gnn_segment_attn_fwd_bias(QKV, 192, dp, off, n, po, npair, bias, O, 64, st, pr, 1, 100, 128, None))
    bwd = lambda QKV=p, dp=64, off=p, n=3, po=p, npair=100, bias=p, dO=p, dQ=p, ws=p, db=p, pr=0.5: (   # noqa: E731
        lib.u2gnn_segment_attn_bwd_bias(QKV, 192, dp, off, n, po, npair, bias, p, dO, 64, p, pr, 1, 0.1, dQ, 192, ws,
                                        db, 100, 128, None))
    assert fwd(QKV=None) == E_ARG and fwd(off=None) == E_ARG and fwd(O=None) == E_ARG and fwd(st=None) == E_ARG
    assert fwd(n=0) == E_ARG and fwd(dp=96) == E_ARG and fwd(pr=1.0) == E_ARG
    assert fwd(po=None) == E_ARG                                  # a bias without its pair offsets
    assert fwd(npair=0) == E_ARG and fwd(npair=-5) == E_ARG       # a bias without a pair
    assert bwd(QKV=None) == E_ARG and bwd(dO=None) == E_ARG and bwd(dQ=None) == E_ARG and bwd(ws=None) == E_ARG
    assert bwd(n=0) == E_ARG and bwd(dp=96) == E_ARG and bwd(pr=1.0) == E_ARG
    assert bwd(po=None) == E_ARG and bwd(npair=0) == E_ARG
    assert bwd(bias=None, db=p) == E_ARG                          # a bias gradient without a bias
    # the plain calls' own refusals are unchanged (they forward to the new ones)
    assert lib.u2gnn_segment_attn_fwd(p, 192, 64, p, 0, p, 64, p, 0.5, 1, 100, 128, None) == E_ARG
    assert lib.u2gnn_segment_attn_fwd(None, 192, 64, p, 3, p, 64, p, 0.5, 1, 100, 128, None) == E_ARG


def _layer_args(window=0):
    from u2gnn_hip import _lib
    dims = _lib.LayerDims(437, 100, 256, 1, 0, window, 0)
    fake = ctypes.c_void_p(1 << 40)   # never dereferenced on the host
    params = _lib.LayerParamsC(*([fake.value] * 12))
    seeds = _lib.LayerSeeds(0.5, 1, 2, 3, 4)
    grads = _lib.LayerGrads(*([fake.value] * len(_lib._PKEYS)))
    return dims, fake, params, seeds, grads


def test_segb_layer_entry_points_refuse_bad_arguments_before_launching():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    by = ctypes.byref
    dims, fake, params, seeds, grads = _layer_args()
    c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.u2gnn_layer_sizes_seg(by(dims), 0.5, 8, by(c), by(f), by(b)) == 0
    fwd = lambda d, X=fake, seg=fake, n=8, po=fake, npair=1000, bias=fake, ws=None, db=fake: (   # noqa: E731
        lib.u2gnn_layer_fwd_segb(by(d), by(params), by(seeds), X, fake, fake, c.value, fake,
                                 f.value if ws is None else ws, seg, n, po, npair, bias, None))
    bwd = lambda d, X=fake, seg=fake, n=8, po=fake, npair=1000, bias=fake, ws=None, db=fake: (   # noqa: E731
        lib.u2gnn_layer_bwd_segb(by(d), by(params), by(seeds), X, fake, c.value, fake, fake, by(grads), fake,
                                 b.value if ws is None else ws, seg, n, po, npair, bias, db, None, None))
    wdims = _layer_args(window=19)[0]
    for call in (fwd, bwd):
        assert call(dims, X=None) == E_ARG                                # null pointer
        assert call(dims, po=None) == E_ARG                               # a bias without its pair offsets
        assert call(dims, npair=0) == E_ARG                               # a bias without a pair
        assert call(dims, seg=None, n=0) == E_ARG                         # a bias without segments
        assert call(dims, seg=None) == E_ARG and call(dims, n=0) == E_ARG  # offsets and count: both or neither
        assert call(wdims) == E_ARG                                       # a window
        assert call(dims, ws=256) == E_ARG                                # short workspace
    assert bwd(dims, bias=None, db=fake) == E_ARG                         # a bias gradient without a bias
    # u2gnn_layer_*_csrb keep refusing a bias without a CSR, also with segments instead
    assert lib.u2gnn_layer_fwd_csrb(by(dims), by(params), by(seeds), fake, fake, fake, c.value, fake, f.value, fake, 8,
                                    None, fake, None) == E_ARG


def test_segment_bias_wrappers_refuse_host_tensors():
    from u2gnn_hip import U2GNNNativeError
    from u2gnn_hip import kernels as K
    QKV, O, st = torch.zeros(128, 192), torch.zeros(128, 64), torch.zeros(128, 2)
    off = torch.tensor([0, 100])
    po, bias = torch.tensor([0, 10000]), torch.zeros(10000)
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_fwd_bias(QKV, 64, off, po, bias, O, st, 0.0, 1, 100, 128)
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_bwd_bias(QKV, 64, off, po, bias, O, O, st, 0.0, 1, 0.1, QKV, bias, 100, 128)
