"""attention="graphs" with ``distances=H``: every node attends over all nodes of its graph and each encoder layer adds
hop_bias[l][t][min(shortest-path distance, H)] to its scores.  The small batches of tests/test_hops_mode_gpu.py: MUTAG
(dp = 64, 8 graphs) and IMDB-BINARY (degree tags, dp = 128, 4 graphs), L = 2, T = 2, ff 32.

The oracle is tests/hops_ref.py's float64 restatement, fed the full-block lists: every pair of every graph as an entry,
its type the clipped distance (GraphStore.distances lists them in exactly that order).  Gate 1e-3, the project's model
gate."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from edges_ref import block_csr, host_batch  # noqa: E402
from hops_ref import dense_bias, encode_hops, sup_forward_hops  # noqa: E402
from test_hops_mode_gpu import BATCHES, FF, L, T, TOL, _err, _err_own_max, _gpu_fwd_bwd  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip.core import Adjacency, DeviceBatch, PairTypes  # noqa: E402

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")
SIZES = {"mutag": 8, "imdbb": 4}
_BATCH, _ORACLE = {}, {}


def _batch(name, H):
    """(store, classes, HostBatch, ids, (rowptr, colidx, etype) of the full blocks with etype = min(D, H))."""
    key = (name, H)
    if key not in _BATCH:
        dataset, deg, ids = BATCHES[name]
        ids = ids[:SIZES[name]]
        store, C, hb, _ = host_batch(dataset, deg, ids)
        rowptr, colidx = block_csr(hb.offsets)
        pair_off, etype = store.distances(ids, H)
        assert len(etype) == len(colidx) and pair_off[-1] == rowptr[-1]
        _BATCH[key] = (store, C, hb, ids, (rowptr, colidx, etype))
    return _BATCH[key]


def _device_batch(hb, store, ids, H):
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, hb.labels, device=DEV)
    b.pairs = PairTypes.from_store(store, ids, hb.N, DEV, H)
    return b


def _model(d, C, precision="fp32", distances=None, seed=0, table_seed=None, attention="graphs", hops=None):
    from pytorch_U2GNN_Sup import TransformerU2GNN
    torch.manual_seed(seed)
    m = TransformerU2GNN(d, FF, C, T, 0.5, L, precision=precision, attention=attention, hops=hops, distances=distances)
    if table_seed is not None:
        with torch.no_grad():
            m.hop_bias.copy_(torch.randn(m.hop_bias.shape, generator=torch.Generator().manual_seed(table_seed)))
    return m


def _oracle(name, H, table_seed=11, train=False, masks=None):
    """(state dict, scores, loss, gradients) of the float64 restatement on the module's own state_dict; eval results
    are computed once per (batch, H, tables) and shared."""
    from oracle import u2gnn_oracle as O
    key = (name, H, table_seed)
    if not train and key in _ORACLE:
        return _ORACLE[key]
    _, C, hb, _, csr = _batch(name, H)
    m = _model(hb.X_concat.shape[1], C, distances=H, table_seed=table_seed)
    sd32 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd = {k: v.double().clone().requires_grad_(True) for k, v in sd32.items()}
    ref = sup_forward_hops(sd, hb.input_x, hb.offsets, torch.from_numpy(hb.X_concat).double(), csr, L, T, train, masks)
    loss = O.soft_cross_entropy(ref, O.label_smoothing(torch.from_numpy(hb.labels), C).double())
    loss.backward()
    out = (sd32, ref.detach(), loss.item(), {k: v.grad for k, v in sd.items()})
    if not train:
        _ORACLE[key] = out
    return out


def _figures(m, scores, loss, grads, ref, lref, gref):
    figs = {"scores": _err(scores, ref), "loss": abs(loss.item() - lref) / max(1.0, abs(lref))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], gref[n])
    assert "hop_bias" in figs and gref["hop_bias"].abs().max().item() > 0
    figs["hop_bias / own max"] = _err_own_max(grads["hop_bias"], gref["hop_bias"])
    return figs


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fwdh"])
@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_distances_eval_vs_float64_restatement(name, precision):
    """distances = 3, hop_bias = seeded randn: scores, loss and every parameter gradient, hop_bias included."""
    H = 3
    store, C, hb, ids, csr = _batch(name, H)
    sd, ref, lref, gref = _oracle(name, H)
    m = _model(hb.X_concat.shape[1], C, precision, distances=H)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    scores, loss, grads = _gpu_fwd_bwd(m, _device_batch(hb, store, ids, H), C)
    figs = _figures(m, scores, loss, grads, ref, lref, gref)
    print(f"distances eval parity {name} {precision} pairs={len(csr[1])}: max {max(figs.values()):.3g} "
          f"(scores {figs['scores']:.3g}, hop_bias {figs['hop_bias']:.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def test_distances_train_step_vs_float64_restatement_with_kernel_masks():
    """Train mode, fp32, MUTAG, distances = 3: the restatement fed the kernels' own dropout masks."""
    from train_parity_util import layer_masks
    from u2gnn_hip.engine import SITE_HEAD, rup, site_seed
    H, seed = 3, 987654321
    store, C, hb, ids, _ = _batch("mutag", H)
    d = hb.X_concat.shape[1]
    b = _device_batch(hb, store, ids, H)
    masks = {}
    for l in range(L):
        for t in range(T):
            masks[(l, t)] = layer_masks(seed, l, t, b.N, d, FF)
        masks[("head", l)] = K.dropout_mask(site_seed(seed, l, 0, SITE_HEAD), b.B, rup(d, 64), 0.5).float().cpu()[:, :d]
    sd, ref, lref, gref = _oracle("mutag", H, table_seed=12, train=True, masks=masks)
    m = _model(d, C, "fp32", distances=H)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    scores, loss, grads = _gpu_fwd_bwd(m, b, C, train=True, seed=seed)
    figs = _figures(m, scores, loss, grads, ref, lref, gref)
    print(f"distances train parity: max {max(figs.values()):.3g} "
          f"(hop_bias rel own max {figs['hop_bias / own max']:.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def test_unsup_distances_eval_vs_float64_restatement():
    """UnSup on PTC, distances = 2, eval: the summed loss and every trainable gradient, hop_bias included."""
    from oracle import u2gnn_oracle as O
    from pytorch_U2GNN_UnSup import TransformerU2GNN
    from u2gnn_hip.unsup import UnSupTrainer
    H = 2
    ids = [2, 9, 31, 44]
    store, _, hb, _ = host_batch("PTC", False, ids, with_input_y=True)
    csr = block_csr(hb.offsets) + (store.distances(ids, H)[1],)
    V = int(store.node_start[-1])
    torch.manual_seed(3)
    m = TransformerU2GNN(vocab_size=V, feature_dim_size=store.d, ff_hidden_size=FF, sampled_num=256,
                         num_self_att_layers=T, num_U2GNN_layers=L, dropout=0.5, device=DEV, attention="graphs",
                         distances=H)
    with torch.no_grad():
        m.hop_bias.copy_(torch.randn(L, T, H + 1, generator=torch.Generator().manual_seed(14)))
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()
          if k.startswith("u2gnn_layers.") or k in ("ss.weight", "hop_bias")}
    m = m.to(DEV).eval()
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, input_y=hb.input_y, device=DEV)
    b.pairs = PairTypes.from_store(store, ids, hb.N, DEV, H)
    tr = UnSupTrainer(m, lr=5e-4)
    sid = torch.from_numpy(m.ss.draw_samples()).to(DEV)
    loss = tr.forward_backward(b, sid, train=False)
    torch.cuda.synchronize()
    outs = encode_hops(sd, hb.input_x, torch.from_numpy(hb.X_concat).double(), csr, L, T, False)
    ref = O.sampled_softmax_logits(torch.cat(outs, 1), torch.from_numpy(hb.input_y), sd["ss.weight"], sid.cpu()).sum()
    ref.backward()
    figs = {"loss": abs(loss.item() - ref.item()) / max(1.0, abs(ref.item()))}
    for n in tr.flat.names:
        figs[n] = _err(tr.flat.grads[n], sd[n].grad)
    assert "hop_bias" in figs and sd["hop_bias"].grad.abs().max().item() > 0
    figs["hop_bias / own max"] = _err_own_max(tr.flat.grads["hop_bias"], sd["hop_bias"].grad)
    print(f"unsup distances eval parity: max {max(figs.values()):.3g}")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


@pytest.mark.parametrize("train", [False, True])
def test_a_zero_table_is_plain_graphs_mode(train):
    """A zero table adds 0.0f: loss, scores and every shared gradient are torch.equal to the attention="graphs" model
    of the same seed on the same batch; hop_bias's own gradient is finite and not zero."""
    H = 3
    store, C, hb, ids, _ = _batch("mutag", H)
    d = hb.X_concat.shape[1]
    out = []
    for distances in (None, H):
        m = _model(d, C, "fp32", distances=distances).to(DEV).train(train)
        scores, loss, grads = _gpu_fwd_bwd(m, _device_batch(hb, store, ids, H), C, train=train, seed=4242)
        torch.cuda.synchronize()
        out.append((scores, loss, grads))
    (s0, l0, g0), (s1, l1, g1) = out
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    assert set(g1) - set(g0) == {"hop_bias"}
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    hg = g1["hop_bias"]
    assert hg.shape == (L, T, H + 1) and torch.isfinite(hg).all() and hg.abs().max().item() > 0


@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_graph_scores_do_not_depend_on_the_batch(name):
    """fp32, eval, distances = 2, a random table: the logits of graph g inside the batch equal those of g alone, bit
    for bit."""
    H = 2
    dataset, deg, ids = BATCHES[name]
    store, C, hb, _ = host_batch(dataset, deg, ids)                       # the batch of 8
    m = _model(hb.X_concat.shape[1], C, "fp32", distances=H, table_seed=13).to(DEV).eval()

    def single(g):
        s, e = int(hb.offsets[g]), int(hb.offsets[g + 1])
        b = DeviceBatch.from_offsets(hb.input_x[s:e] - s, np.array([0, e - s]), hb.X_concat[s:e], hb.labels[g:g + 1],
                                     device=DEV)
        b.pairs = PairTypes.from_store(store, [ids[g]], e - s, DEV, H)
        return b
    with torch.no_grad():
        full = m(_device_batch(hb, store, ids, H), None, None).cpu()
        alone = torch.cat([m(single(g), None, None).cpu() for g in range(len(hb.labels))])
    assert torch.equal(full, alone)


def test_distances_16_equals_edges_with_16_hops_on_mutag():
    """Every MUTAG graph is connected with diameter <= 15, so attention="edges", hops=16 lists every pair of a graph
    with its exact distance -- the pattern and bias of distances=16.  The two dense masks are the same array; both
    models are within 1e-3 of the one oracle, and of each other within 2e-3."""
    H = 16
    store, C, hb, ids, full = _batch("mutag", H)
    edges = store.adjacency(ids, hops=H)
    table = torch.randn(H + 1, generator=torch.Generator().manual_seed(5)).double()
    assert torch.equal(dense_bias(*edges, hb.N, table), dense_bias(*full, hb.N, table))
    assert all(np.array_equal(a, b) for a, b in zip(edges, full))
    sd, ref, lref, gref = _oracle("mutag", H)
    d = hb.X_concat.shape[1]
    res = {}
    for mode in ("graphs", "edges"):
        kw = dict(attention="graphs", distances=H) if mode == "graphs" else dict(attention="edges", hops=H)
        m = _model(d, C, "fp32", **kw)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        b = _device_batch(hb, store, ids, H)
        b.adj = Adjacency.from_csr(edges[0], edges[1], hb.N, device=DEV, etype=edges[2])
        scores, loss, grads = _gpu_fwd_bwd(m, b, C)
        figs = _figures(m, scores, loss, grads, ref, lref, gref)
        print(f"distances=16 vs oracle, {mode}: max {max(figs.values()):.3g}")
        bad = {k: v for k, v in figs.items() if not v <= TOL}
        assert not bad, (mode, bad)
        res[mode] = (scores, loss, {k: v.clone() for k, v in grads.items()})
    (s0, l0, g0), (s1, l1, g1) = res["graphs"], res["edges"]
    direct = {"scores": _err(s0, s1), "loss": _err(l0, l1)}
    direct.update({n: _err(g0[n], g1[n]) for n in g0})
    print(f"distances=16 (segment kernels) vs edges hops=16 (CSR kernels): max {max(direct.values()):.3g} "
          f"(scores {direct['scores']:.3g}, hop_bias {direct['hop_bias']:.3g})")
    bad = {k: v for k, v in direct.items() if not v <= 2e-3}
    assert not bad, bad


def test_distances_steps_replay_as_a_hip_graph():
    """Three trainer steps under StepGraphs replay against three eagerly issued ones (eval mode: no dropout): loss,
    hop_bias and every parameter within 1e-6.  hop_bias changes between the replays, so a table copied at capture
    time would fail."""
    from u2gnn_hip.train import StepGraphs, SupTrainer
    H = 2
    store, C, hb, ids, _ = _batch("mutag", H)
    b = _device_batch(hb, store, ids, H)
    res = []
    for graphed in (False, True):
        m = _model(hb.X_concat.shape[1], C, "fwdh", distances=H).to(DEV).eval()
        tr = SupTrainer(m, lr=5e-3)
        losses, tables = [], []
        with StepGraphs(tr) as runner:
            for _ in range(3):
                loss = runner.step(b, False) if graphed else tr.step(b, False)
                torch.cuda.synchronize()
                losses.append(loss.detach().cpu().clone())
                tables.append(m.hop_bias.detach().cpu().clone())
            res.append((losses, tables, tr.flat.flat.detach().cpu().clone()))
    (l0, t0, p0), (l1, t1, p1) = res
    for t in (t0, t1):
        assert t[0].abs().max().item() > 0 and not torch.equal(t[0], t[1]) and not torch.equal(t[1], t[2])
    assert not torch.equal(l1[0], l1[1])
    for a, c in zip(l0 + t0 + [p0], l1 + t1 + [p1]):
        assert _err(c, a) <= 1e-6


def test_sup_cli_mutag_distances(tmp_path):
    run = tmp_path / "run" / "x"
    run.mkdir(parents=True)
    cmd = [sys.executable, os.path.join(PKG, "train_pytorch_U2GNN_Sup.py"), "--run_folder", str(run), "--num_epochs",
           "1", "--dataset", "MUTAG", "--model_name", "MUTAG", "--batch_size", "4", "--num_neighbors", "4",
           "--ff_hidden_size", "128", "--num_timesteps", "2", "--attention", "graphs", "--distances", "3",
           "--precision", "fwdh", "--max_steps", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "distances=3" in r.stdout                  # the argument namespace the CLI prints first
    m = re.search(r"\| epoch\s+1 \|.*\| loss\s+(\S+) \| test acc", r.stdout)
    assert m, r.stdout[-2000:]
    assert math.isfinite(float(m.group(1)))
