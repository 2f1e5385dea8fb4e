"""The two trailing parameters in the data-parallel exchange: world 2 over gloo on ONE GPU (the set-up of
tests/test_dp_gloo_gpu.py), L = 1, T = 2, attention="edges", hops = 2, centrality = 3 on two MUTAG batches.
OverlappedGradAllReduce, wired into the backward, must leave the same flat gradient, bit for bit, as GradAllReduce over
the same per-rank gradients -- the degree_emb and hop_bias regions included, which go out after their reductions."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2
IDS = ([0, 5, 17, 23, 42, 77, 101, 150], [3, 15, 27, 39, 51, 63, 75, 87])


def _worker(rank, world, port, out_dir):
    sys.path[:0] = [os.path.join(REPO, "graph-transformer_amd"), REPO, os.path.join(REPO, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TORCHELASTIC_USE_AGENT_STORE="True")
    import u2gnn_hip  # noqa: F401  (hardware queues before HIP starts)
    import torch.distributed as dist
    dev = torch.device("cuda", 0)   # both ranks on the one GPU
    torch.cuda.set_device(dev)
    from u2gnn_hip.engine import side_stream
    side_stream(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from edges_ref import host_batch
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.core import Adjacency, DeviceBatch
    from u2gnn_hip.dp import GradAllReduce, OverlappedGradAllReduce, broadcast_params
    from u2gnn_hip.train import SupTrainer
    ids = IDS[rank]
    store, C, hb, _ = host_batch("MUTAG", False, ids)
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, hb.labels, device=dev,
                                 degrees=store.degrees_of(ids))
    csr = store.adjacency(ids, hops=2)
    b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=dev, etype=csr[2])
    torch.manual_seed(123)
    m = TransformerU2GNN(7, 32, C, 2, 0.5, 1, precision="fp32", attention="edges", hops=2, centrality=3)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        m.degree_emb.copy_(torch.randn(m.degree_emb.shape, generator=g))
        m.hop_bias.copy_(torch.randn(m.hop_bias.shape, generator=g))
    tr = SupTrainer(m.to(dev).eval(), lr=5e-4)
    broadcast_params(tr.flat)
    assert tr.flat.names[-2:] == ("degree_emb", "hop_bias")
    # the plain exchange of this rank's gradient
    tr.forward_backward(b, train=False, seed=7)
    local = tr.flat.gflat.detach().clone()
    GradAllReduce(bucket_mb=8.0)(tr.flat)
    plain = tr.flat.gflat.detach().cpu().clone()
    # the same backward with the overlapped exchange wired in
    ar = OverlappedGradAllReduce(tr.flat)
    m.core.stack.grad_ready = ar.layer_done
    tr.flat.gflat.zero_()
    tr.forward_backward(b, train=False, seed=7)
    lo = ar.span["degree_emb"][0]
    assert ar.launched and all(hi <= lo for _, hi in ar.launched), ar.launched     # the trailing regions wait for __call__
    ar(tr.flat)
    torch.cuda.synchronize()
    over = tr.flat.gflat.detach().cpu().clone()
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), local=local.cpu().numpy(), plain=plain.numpy(), over=over.numpy(),
             span=np.array([ar.span["degree_emb"], ar.span["hop_bias"]]))
    dist.destroy_process_group()


def test_overlapped_allreduce_equals_plain_allreduce_with_both_trailing_parameters(tmp_path, rdzv_port):
    mp.spawn(_worker, args=(WORLD, rdzv_port, str(tmp_path)), nprocs=WORLD, join=True)
    r = [dict(np.load(os.path.join(tmp_path, f"r{i}.npz"))) for i in range(WORLD)]
    for x in r:
        assert np.isfinite(x["over"]).all()
        assert np.array_equal(x["over"].view(np.uint32), x["plain"].view(np.uint32))
    assert np.array_equal(r[0]["over"], r[1]["over"]), "ranks hold different gradients"
    assert not np.array_equal(r[0]["local"], r[1]["local"])
    mean = (r[0]["local"] + r[1]["local"]) * np.float32(0.5)                      # gloo: sum, then one scaling
    assert np.array_equal(r[0]["over"], mean)
    for lo, hi in r[0]["span"]:
        assert hi > lo and np.abs(r[0]["over"][lo:hi]).max() > 0
