"""``centrality`` without a GPU: the keyword's check, the models' one more parameter and its place in the flat buffer,
the store's degrees, the new entry points and their refusal of bad arguments before any launch, the tail of the
overlapped all-reduce, and the CLIs' flag."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from edges_ref import store_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
E_ARG = -1
IDS = [0, 5, 17, 23, 42, 77, 101, 150]     # the fixed MUTAG graphs of tests/test_hops_mode_gpu.py
NEW_SYMBOLS = ("u2gnn_gather_rows_emb", "u2gnn_class_rows_grad", "u2gnn_class_rows_grad_ws_floats")


def test_check_centrality_accepts_and_rejects():
    from u2gnn_hip.core import check_centrality
    assert check_centrality(None) is None and check_centrality(0) is None
    for ok in (1, 16, 63, np.int64(5)):
        assert check_centrality(ok) == int(ok) and type(check_centrality(ok)) is int
    for bad in (64, -1, 2.5, "3", True):
        with pytest.raises(ValueError, match="centrality"):
            check_centrality(bad)


def _models(**kw):
    from pytorch_U2GNN_Sup import TransformerU2GNN as Sup
    from pytorch_U2GNN_UnSup import TransformerU2GNN as UnSup
    return (lambda: Sup(7, 32, 2, 2, 0.5, 2, **kw)), (lambda: UnSup(50, 7, 32, 8, 2, 2, 0.5, "cpu", **kw))


def _offsets(flat):
    base = flat.gflat.data_ptr()
    return {n: (flat.grads[n].data_ptr() - base) // 4 for n in flat.names}


@pytest.mark.parametrize("which", [0, 1])
def test_modules_gain_degree_emb_before_hop_bias_and_keep_every_offset(which):
    from u2gnn_hip.core import FlatParams
    torch.manual_seed(5)
    plain = _models()[which]()
    torch.manual_seed(5)
    both = _models(attention="edges", hops=2, centrality=4)[which]()
    torch.manual_seed(5)
    only = _models(centrality=4)[which]()
    ref_names = [n for n, _ in plain.named_parameters()]
    assert [n for n, _ in both.named_parameters()] == ref_names + ["degree_emb", "hop_bias"]
    assert [n for n, _ in only.named_parameters()] == ref_names + ["degree_emb"]
    assert list(_models(centrality=0)[which]().state_dict()) == list(plain.state_dict())      # off: today's keys
    assert not hasattr(plain, "degree_emb")
    for m in (both, only):
        assert m.degree_emb.shape == (5, 7) and float(m.degree_emb.abs().max()) == 0.0
        for k, v in plain.state_dict().items():                          # the seed's values: torch's generator untouched
            assert torch.equal(v, m.state_dict()[k]), k
    names = None if which == 0 else plain.trainable_names()
    o_plain = _offsets(FlatParams(plain, names))
    for m in (both, only):
        o = _offsets(FlatParams(m, None if which == 0 else m.trainable_names()))
        for n, off in o_plain.items():
            assert o[n] == off, n
        assert o["degree_emb"] >= max(o_plain.values())
        if "hop_bias" in o:
            assert o["hop_bias"] == o["degree_emb"] + 5 * 7 + 1          # 35 floats, padded to 36


def test_unsup_trains_degree_emb_next_to_hop_bias():
    m = _models(attention="edges", hops=2, centrality=3)[1]()
    assert m.trainable_names()[-2:] == ["degree_emb", "hop_bias"] and "ss.weight" in m.trainable_names()
    assert "degree_emb" not in _models()[1]().trainable_names()


def test_degrees_of_equals_the_neighbour_list_lengths():
    store, _ = store_of("MUTAG", False)
    want = np.concatenate([[len(nb) for nb in store.graphs[i].neighbors] for i in IDS])
    got = store.degrees_of(IDS)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got.min() == 1 and got.max() == 3        # these eight graphs: D = 3 uses every row but 0, D = 2 clips


def test_stack_names_how_to_set_deg_for_tensor_inputs():
    """The message is raised before any launch: reference-style inputs carry no edges, hence no degrees."""
    from u2gnn_hip.core import DeviceBatch, EncoderStack
    m = _models(centrality=3)[0]()
    b = DeviceBatch(3, 1, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, 7), None, None, None)
    with pytest.raises(ValueError, match="DeviceBatch.deg"):
        EncoderStack.for_module(m)._degrees(b)
    b.deg = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="int32"):
        EncoderStack.for_module(m)._degrees(b)
    b.deg = torch.zeros(3, dtype=torch.int32)
    deg, table = EncoderStack.for_module(m)._degrees(b)
    assert table.data_ptr() == m.degree_emb.data_ptr()                    # read where the parameter lies


def test_from_offsets_carries_the_degrees():
    from u2gnn_hip.core import DeviceBatch
    store, _ = store_of("MUTAG", False)
    hb = store.assemble_numpy(IDS, 4, rng=np.random.RandomState(7))
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, hb.labels, device="cpu",
                                 degrees=store.degrees_of(IDS))
    assert b.deg.dtype == torch.int32 and np.array_equal(b.deg.numpy(), store.degrees_of(IDS))
    assert DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, device="cpu").deg is None
    with pytest.raises(ValueError, match="degrees"):
        DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, device="cpu", degrees=np.zeros(3))


def test_library_exports_the_centrality_entry_points():
    from u2gnn_hip import _lib
    from u2gnn_hip import kernels as K
    lib = _lib.hip_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.header_symbols("u2gnn_hip.h"), name
    assert lib.u2gnn_abi_version() == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "u2gnn_hip.h")).read()
    for name, value in (("CHUNK", K.CLASS_ROWS_CHUNK), ("MAX", K.CLASS_ROWS_MAX)):      # the header's constants
        assert int(re.search(rf"#define U2GNN_CLASS_ROWS_{name} +(\d+)", header).group(1)) == value
    RB = K.CLASS_ROWS_CHUNK
    assert K.class_rows_k(1) == K.class_rows_k(16 * RB) == RB // 4 + 2 + 1 + 4 and K.class_rows_k(16 * RB + 1) == RB // 4 + 8


def test_centrality_kernels_refuse_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_ARG shows that nothing was
    launched (the method of tests/test_hops_cpu.py)."""
    from u2gnn_hip import _lib
    from u2gnn_hip import kernels as K
    lib = _lib.hip_lib()
    p = ctypes.c_void_p(1 << 40)
    RB = K.CLASS_ROWS_CHUNK
    need = lib.u2gnn_class_rows_grad_ws_floats(3 * RB + 5, 367, 17)
    assert need == 4 * 17 * 367                                           # 4 chunks
    assert lib.u2gnn_class_rows_grad_ws_floats(0, 7, 1) == 0
    for bad in ((-1, 7, 3), (10, 0, 3), (10, 7, 0), (10, 7, 65)):
        assert lib.u2gnn_class_rows_grad_ws_floats(*bad) == -1
    cg = lambda dX=p, ld=384, n=3 * RB + 5, d=367, idx=p, deg=p, C=17, de=p, ldd=367, ws=p, nws=need: \
        lib.u2gnn_class_rows_grad(dX, ld, n, d, idx, 1, deg, 1000, C, de, ldd, ws, nws, None)   # noqa: E731
    assert cg(dX=None) == E_ARG and cg(idx=None) == E_ARG and cg(deg=None) == E_ARG and cg(de=None) == E_ARG
    assert cg(ws=None) == E_ARG
    assert cg(C=0) == E_ARG and cg(C=65) == E_ARG and cg(d=0) == E_ARG and cg(ld=366) == E_ARG and cg(ldd=366) == E_ARG
    assert cg(nws=need - 1) == E_ARG                                      # a workspace that is too small
    ge = lambda src=p, idx=p, dst=p, deg=p, emb=p, lde=367, C=17, n=5, npad=8, d=367, dp=384: \
        lib.u2gnn_gather_rows_emb(src, 367, 100, idx, 1, dst, 384, n, npad, d, dp, deg, emb, lde, C, None, None)   # noqa: E731
    assert ge(src=None) == E_ARG and ge(idx=None) == E_ARG and ge(dst=None) == E_ARG and ge(deg=None) == E_ARG
    assert ge(emb=None) == E_ARG and ge(C=0) == E_ARG and ge(lde=366) == E_ARG
    assert ge(n=9) == E_ARG and ge(d=385) == E_ARG                        # the gather's own checks


def test_kernel_wrappers_refuse_host_tensors():
    from u2gnn_hip import U2GNNNativeError
    from u2gnn_hip import kernels as K
    ix, deg = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(U2GNNNativeError):
        K.gather_rows_emb(torch.zeros(4, 7), ix, 1, torch.zeros(8, 64), 4, 8, 7, 64, deg, torch.zeros(3, 7))
    with pytest.raises(U2GNNNativeError):
        K.class_rows_grad(torch.zeros(8, 64), ix, 1, deg, 4, 4, 7, torch.zeros(3, 7))


def _tail_worker(rank, world, port):
    sys.path[:0] = [os.path.join(REPO, "graph-transformer_amd"), REPO]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TORCHELASTIC_USE_AGENT_STORE="True")
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.core import FlatParams
    from u2gnn_hip.dp import OverlappedGradAllReduce
    for kw in (dict(attention="edges", hops=2, centrality=4), dict(centrality=4), dict(attention="edges", hops=2), {}):
        torch.manual_seed(1)
        flat = FlatParams(TransformerU2GNN(7, 32, 2, 2, 0.5, 2, **kw))
        ar = OverlappedGradAllReduce(flat)
        enc_hi = max(b for n, (a, b) in ar.span.items() if n.startswith("u2gnn_layers."))
        first = "degree_emb" if "centrality" in kw else "hop_bias" if "hops" in kw else None
        end = ar.span[first][0] if first else flat.gflat.numel()
        assert ar.tail == (ar._align_end(enc_hi), end), (kw, ar.tail)
        assert ar.tail[1] - ar.tail[0] == 2 * (16 + 4)                    # the two heads: [2, 7] and [2], padded to 4 floats
        if "centrality" in kw:
            lo, hi = ar.span["degree_emb"]
            assert hi - lo == 5 * 7
            if "hops" in kw:
                assert ar.span["hop_bias"][0] == ar._align_end(hi) and ar.span["hop_bias"][1] <= flat.gflat.numel()
            # the backward's calls: nothing issued before __call__ covers degree_emb (or hop_bias)
            g0 = torch.randn(flat.gflat.numel(), generator=torch.Generator().manual_seed(3))
            flat.gflat.copy_(g0)
            for l in reversed(range(2)):
                for t in reversed(range(2)):
                    ar.layer_done(f"u2gnn_layers.{l}.layers.{t}.")
            assert ar.launched and all(b <= lo for a, b in ar.launched), ar.launched
            ar(flat)
            assert torch.equal(flat.gflat, g0) and not ar.pending and not ar.launched      # one rank: the sum is g0
    dist.destroy_process_group()


def test_overlapped_allreduce_tail_ends_where_degree_emb_begins(rdzv_port):
    mp.spawn(_tail_worker, args=(1, rdzv_port), nprocs=1, join=True)


@pytest.mark.parametrize("script", ["train_pytorch_U2GNN_Sup.py", "train_pytorch_U2GNN_UnSup.py"])
def test_cli_lists_centrality_and_checks_its_range(script):
    run = lambda *a: subprocess.run([sys.executable, os.path.join(PKG, script), *a], capture_output=True,  # noqa: E731
                                    text=True, timeout=300)
    r = run("--help")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--centrality" in r.stdout
    r = run("--centrality", "64")
    assert r.returncode == 2 and "--centrality must be in 0..63" in r.stderr
    if "UnSup" in script:
        r = run("--centrality", "4", "--world_size", "2")
        assert r.returncode == 2 and "--centrality is not available with --world_size" in r.stderr
