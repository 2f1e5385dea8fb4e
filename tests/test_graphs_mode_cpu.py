"""attention="graphs" without a GPU: the library exports the new entry points under the unchanged ABI version, they
refuse bad arguments before launching anything, and the modules and CLIs know the third mode."""
import ctypes
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
E_ARG = -1


def test_library_exports_segment_entry_points():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    for name in ("u2gnn_segment_attn_fwd", "u2gnn_segment_attn_bwd", "u2gnn_layer_sizes_seg", "u2gnn_layer_fwd_seg",
                 "u2gnn_layer_bwd_seg"):
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


def test_segment_layer_entry_points_refuse_bad_arguments_before_launching():
    """On a GPU-less host a launch fails with a (positive) HIP error code, so U2GNN_E_ARG shows that nothing was
    launched."""
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    dims, fake, params, seeds, grads = _layer_args()
    c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    by = ctypes.byref
    assert lib.u2gnn_layer_sizes_seg(by(dims), 0.5, 8, by(c), by(f), by(b)) == 0
    cn, fn, bn = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.u2gnn_layer_sizes(by(dims), 0.5, by(cn), by(fn), by(bn)) == 0
    # the statistics take the place of the [Np, Np] image; the size does not depend on the segment count
    assert 0 < c.value < cn.value
    c2, f2, b2 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.u2gnn_layer_sizes_seg(by(dims), 0.5, 1, by(c2), by(f2), by(b2)) == 0
    assert (c2.value, f2.value, b2.value) == (c.value, f.value, b.value)
    assert lib.u2gnn_layer_sizes_seg(by(dims), 0.5, 0, by(c2), by(f2), by(b2)) == 0    # n_seg = 0: the node-axis layer
    assert (c2.value, f2.value, b2.value) == (cn.value, fn.value, bn.value)
    assert lib.u2gnn_layer_sizes_seg(by(dims), 0.5, -1, by(c2), by(f2), by(b2)) == E_ARG
    assert lib.u2gnn_layer_sizes_seg(None, 0.5, 8, by(c2), by(f2), by(b2)) == E_ARG
    fwd = lambda d, X, seg, n, ws=f.value: lib.u2gnn_layer_fwd_seg(   # noqa: E731
        by(d), by(params), by(seeds), X, fake, fake, c.value, fake, ws, seg, n, None)
    bwd = lambda d, X, seg, n, ws=b.value: lib.u2gnn_layer_bwd_seg(   # noqa: E731
        by(d), by(params), by(seeds), X, fake, c.value, fake, fake, by(grads), fake, ws, seg, n, None, None)
    for call in (fwd, bwd):
        assert call(dims, None, fake, 8) == E_ARG          # null pointer
        assert call(dims, fake, fake, 0) == E_ARG          # offsets without a count
        assert call(dims, fake, None, 8) == E_ARG          # a count without offsets
        assert call(dims, fake, fake, -3) == E_ARG
        assert call(dims, fake, fake, 8, 256) == E_ARG     # short workspace: refused by the planning pass
    wdims = _layer_args(window=19)[0]                      # 437 = 23 * 19 rows in windows of 19
    assert lib.u2gnn_layer_sizes_seg(by(wdims), 0.5, 8, by(c2), by(f2), by(b2)) == E_ARG
    for call in (fwd, bwd):
        assert call(wdims, fake, fake, 8) == E_ARG         # window and segments together


def test_segment_kernels_refuse_bad_arguments_before_launching():
    from u2gnn_hip import _lib
    lib = _lib.hip_lib()
    p = ctypes.c_void_p(1 << 40)
    fwd = lambda QKV=p, dp=64, off=p, n=3, O=p, st=p, pr=0.5: lib.u2gnn_segment_attn_fwd(   # noqa: E731
        QKV, 192, dp, off, n, O, 64, st, pr, 1, 100, 128, None)
    bwd = lambda QKV=p, dp=64, off=p, n=3, dO=p, dQ=p, ws=p, pr=0.5: lib.u2gnn_segment_attn_bwd(   # noqa: E731
        QKV, 192, dp, off, n, p, dO, 64, p, pr, 1, 0.1, dQ, 192, ws, 100, 128, None)
    assert fwd(QKV=None) == E_ARG and fwd(off=None) == E_ARG and fwd(O=None) == E_ARG and fwd(st=None) == E_ARG
    assert fwd(n=0) == E_ARG and fwd(dp=96) == E_ARG and fwd(pr=1.0) == E_ARG and fwd(pr=-0.1) == E_ARG
    assert bwd(QKV=None) == E_ARG and bwd(dO=None) == E_ARG and bwd(dQ=None) == E_ARG and bwd(ws=None) == E_ARG
    assert bwd(n=0) == E_ARG and bwd(dp=96) == E_ARG and bwd(pr=1.0) == E_ARG


def test_kernel_wrappers_refuse_host_tensors():
    import torch
    from u2gnn_hip import U2GNNNativeError
    from u2gnn_hip import kernels as K
    x = torch.zeros(128, 192)
    off = torch.tensor([0, 100])
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_fwd(x, 64, off, torch.zeros(128, 64), torch.zeros(128, 2), 0.0, 1, 100, 128)
    with pytest.raises(U2GNNNativeError):
        K.segment_attn_bwd(x, 64, off, torch.zeros(128, 64), torch.zeros(128, 64), torch.zeros(128, 2), 0.0, 1, 0.1,
                           torch.zeros(128, 192), 100, 128)


def test_modules_reject_an_unknown_attention_mode():
    from pytorch_U2GNN_Sup import TransformerU2GNN as Sup
    from pytorch_U2GNN_UnSup import TransformerU2GNN as UnSup
    for build in (lambda a: Sup(7, 32, 2, 1, 0.5, 1, attention=a),
                  lambda a: UnSup(50, 7, 32, 8, 1, 1, 0.5, "cpu", attention=a)):
        with pytest.raises(ValueError) as e:
            build("graph")
        for mode in ("'nodes'", "'neighbors'", "'graphs'"):
            assert mode in str(e.value)
        assert build("graphs").attention == "graphs"


@pytest.mark.parametrize("script", ["train_pytorch_U2GNN_Sup.py", "train_pytorch_U2GNN_UnSup.py"])
def test_cli_help_lists_graphs(script):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "{nodes,neighbors,graphs}" in r.stdout.replace("\n", "").replace(" ", "")
