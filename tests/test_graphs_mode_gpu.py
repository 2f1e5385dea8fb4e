"""attention="graphs": every node attends over the nodes of its own graph.  That is the "nodes" model applied to
every graph on its own, so the reference is the existing oracle called once per graph
(oracle.u2gnn_oracle.sup_forward on the graph's rows, indices rebased), its rows stacked."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from u2gnn_hip import kernels as K  # noqa: E402

DEV = "cuda"
TOL = 1e-3


def _err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def _close(a, b, tol=TOL):
    return _err(a, b) <= tol


def _load(golden_dir, name):
    z = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    off = z["b0_offsets"]
    ix = z["b0_input_x"]
    for g in range(len(off) - 1):   # the neighbours of a graph's nodes are nodes of that graph
        s, e = int(off[g]), int(off[g + 1])
        assert ix[s:e].min() >= s and ix[s:e].max() < e
    return z


def _model(z, precision="fp32", attention="graphs"):
    from pytorch_U2GNN_Sup import TransformerU2GNN
    bs, k, T, ff, L, d, C, fold = [int(x) for x in z["meta"]]
    m = TransformerU2GNN(d, ff, C, T, 0.5, L, precision=precision, attention=attention)
    m.load_state_dict({kk[5:]: torch.from_numpy(v) for kk, v in z.items() if kk.startswith("init.")})
    return m, (T, ff, L, d, C)


def _oracle_per_graph(sd, z, L, T, train=False, masks=None):
    """Scores [B, C]: the oracle's nodes-mode model on every graph alone.  masks: whole-batch kernel masks, sliced
    per graph (attention [s:e, s:e], row sites [s:e], head [g:g+1])."""
    from oracle import u2gnn_oracle as O
    off = z["b0_offsets"]
    ix, X = torch.from_numpy(z["b0_input_x"]), torch.from_numpy(z["b0_X"])
    rows = []
    for g in range(len(off) - 1):
        s, e = int(off[g]), int(off[g + 1])
        mg = None
        if masks is not None:
            mg = {}
            for key, v in masks.items():
                if key[0] == "head":
                    mg[key] = v[g:g + 1]
                else:
                    mg[key] = {n: (t[s:e, s:e] if n == "attn" else t[s:e]) for n, t in v.items()}
        rows.append(O.sup_forward(sd, ix[s:e] - s, np.array([0, e - s]), X[s:e], L, T, train=train, slots=1, masks=mg))
    return torch.cat(rows, 0)


def _gpu_fwd_bwd(m, b, C, train=False, seed=0):
    flat = m.flatten_parameters()
    scores, ctx = m.core.forward(b, train=train, need_ctx=True, seed=seed)
    dsc = torch.empty_like(scores)
    loss = torch.zeros(1, device=DEV)
    K.smoothed_ce(scores, b.labels, b.B, C, 0.1, loss, dsc)
    m.core.backward(ctx, dsc, flat.grads)
    return scores, loss, flat.grads


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fwdh"])
@pytest.mark.parametrize("name", ["imdbb_sup", "mutag_sup_L2T2"])
def test_graphs_mode_eval_vs_oracle_per_graph(golden_dir, name, precision):
    """Scores, loss and every parameter gradient, max|ours - oracle| / max(1, max|oracle|) <= 1e-3: the project's
    bar, which the nodes-mode parity tests of these fixtures hold for every policy.  Measured maxima (IMDB-BINARY /
    MUTAG L2T2): fp32 1.4e-6 / 1.2e-6, bf16x3 1.0e-5 / 3.0e-5, fwdh 1.0e-5 / 2.0e-5."""
    from oracle import u2gnn_oracle as O
    from u2gnn_hip.core import DeviceBatch
    z = _load(golden_dir, name)
    m, (T, ff, L, d, C) = _model(z, precision)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    b = DeviceBatch.from_offsets(z["b0_input_x"], z["b0_offsets"], z["b0_X"], z["b0_labels"], device=DEV)
    scores, loss, grads = _gpu_fwd_bwd(m, b, C)
    ref = _oracle_per_graph(sd, z, L, T)
    lref = O.soft_cross_entropy(ref, O.label_smoothing(torch.from_numpy(z["b0_labels"]), C))
    lref.backward()
    figs = {"scores": _err(scores, ref.detach()), "loss": abs(loss.item() - lref.item()) / max(1.0, abs(lref.item()))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], sd[n].grad)
    print(f"graphs-mode eval parity {name} {precision}: max {max(figs.values()):.3g} "
          f"(scores {figs['scores']:.3g}, loss {figs['loss']:.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def test_graphs_mode_train_step_vs_oracle_with_kernel_masks(golden_dir):
    """Train mode, fp32: the per-graph oracle fed the kernels' own masks (the graph's block of every site's mask)."""
    from oracle import u2gnn_oracle as O
    from train_parity_util import layer_masks
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.engine import SITE_HEAD, rup, site_seed
    z = _load(golden_dir, "mutag_sup_L2T2")
    m, (T, ff, L, d, C) = _model(z, "fp32")
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    b = DeviceBatch.from_offsets(z["b0_input_x"], z["b0_offsets"], z["b0_X"], z["b0_labels"], device=DEV)
    seed = 987654321
    scores, loss, grads = _gpu_fwd_bwd(m, b, C, train=True, seed=seed)
    masks = {}
    for l in range(L):
        for t in range(T):
            masks[(l, t)] = layer_masks(seed, l, t, b.N, d, ff)
        masks[("head", l)] = K.dropout_mask(site_seed(seed, l, 0, SITE_HEAD), b.B, rup(d, 64), 0.5).float().cpu()[:, :d]
    ref = _oracle_per_graph(sd, z, L, T, train=True, masks=masks)
    lref = O.soft_cross_entropy(ref, O.label_smoothing(torch.from_numpy(z["b0_labels"]), C))
    lref.backward()
    figs = {"scores": _err(scores, ref.detach()), "loss": abs(loss.item() - lref.item()) / max(1.0, abs(lref.item()))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], sd[n].grad)
    print(f"graphs-mode train parity: max {max(figs.values()):.3g}")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def _single(z, g):
    off = z["b0_offsets"]
    s, e = int(off[g]), int(off[g + 1])
    return z["b0_input_x"][s:e] - s, np.array([0, e - s]), z["b0_X"][s:e], z["b0_labels"][g:g + 1]


def test_graph_scores_do_not_depend_on_the_batch(golden_dir):
    """fp32, eval: the logits of graph g in the batch equal those of a batch holding g alone (measured: of order
    1e-6 of max|scores|); the oracle's "nodes" mode, on the CPU, differs by more than the bound: the comparison
    discriminates."""
    from oracle import u2gnn_oracle as O
    from u2gnn_hip.core import DeviceBatch
    z = _load(golden_dir, "imdbb_sup")
    m, (T, ff, L, d, C) = _model(z, "fp32")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    B = min(8, len(z["b0_offsets"]) - 1)
    off = z["b0_offsets"][:B + 1]
    n = int(off[-1])
    b = DeviceBatch.from_offsets(z["b0_input_x"][:n], off, z["b0_X"][:n], z["b0_labels"][:B], device=DEV)
    with torch.no_grad():
        full = m(b, None, None).cpu()
        alone = torch.cat([m(DeviceBatch.from_offsets(*_single(z, g), device=DEV), None, None).cpu() for g in range(B)])
    scale = full.abs().max().item()
    diff = (full - alone).abs().max().item() / scale
    print(f"graphs-mode batch invariance: {diff:.3g} of max|scores|")
    assert diff <= TOL
    ix, X = torch.from_numpy(z["b0_input_x"][:n]), torch.from_numpy(z["b0_X"][:n])
    nodes_full = O.sup_forward(sd, ix, off, X, L, T, train=False, slots=1)
    nodes_alone = torch.cat([O.sup_forward(sd, torch.from_numpy(a), o, torch.from_numpy(x), L, T, train=False, slots=1)
                             for a, o, x, _ in (_single(z, g) for g in range(B))])
    ndiff = (nodes_full - nodes_alone).abs().max().item() / nodes_full.abs().max().item()
    print(f"nodes-mode (oracle) batch dependence: {ndiff:.3g}")
    assert ndiff > TOL


def test_single_graph_equals_nodes_mode(golden_dir):
    from u2gnn_hip.core import DeviceBatch
    z = _load(golden_dir, "imdbb_sup")
    outs = {}
    for mode in ("graphs", "nodes"):
        m, _ = _model(z, "fp32", mode)
        m = m.to(DEV).eval()
        with torch.no_grad():
            outs[mode] = m(DeviceBatch.from_offsets(*_single(z, 0), device=DEV), None, None).cpu()
    assert _close(outs["graphs"], outs["nodes"])


def test_graphs_mode_refuses_scattered_graphs(golden_dir):
    """from_reference_inputs with a column-permuted graph_pool: a ValueError in graphs mode that says what is
    required; nodes mode still runs."""
    z = _load(golden_dir, "imdbb_sup")
    off = z["b0_offsets"]
    B, N = len(off) - 1, int(off[-1])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
    idx = torch.tensor([[g, int(perm[j])] for g in range(B) for j in range(off[g], off[g + 1])]).t()
    pool = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1]), (B, N)).to(DEV)
    ix, X = torch.from_numpy(z["b0_input_x"]).to(DEV), torch.from_numpy(z["b0_X"]).to(DEV)
    mg, _ = _model(z, "fp32", "graphs")
    mn, _ = _model(z, "fp32", "nodes")
    with torch.no_grad():
        with pytest.raises(ValueError, match="consecutive rows"):
            mg.to(DEV).eval()(ix, pool, X)
        assert torch.isfinite(mn.to(DEV).eval()(ix, pool, X)).all()
        # the block-diagonal pool of the reference's get_graphpool is accepted
        idx = torch.tensor([[g, j] for g in range(B) for j in range(off[g], off[g + 1])]).t()
        pool = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1]), (B, N)).to(DEV)
        assert torch.isfinite(mg(ix, pool, X)).all()


def test_graphs_mode_step_replays_as_a_hip_graph(golden_dir):
    """One trainer step under StepGraphs replay equals the eagerly issued step bit for bit (both on the device-side
    Adam schedule that StepGraphs switches on): nothing in the path synchronises with the host or depends on it."""
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.train import StepGraphs, SupTrainer
    z = _load(golden_dir, "mutag_sup_L2T2")
    b = DeviceBatch.from_offsets(z["b0_input_x"], z["b0_offsets"], z["b0_X"], z["b0_labels"], device=DEV)
    res = []
    for graphed in (False, True):
        m, _ = _model(z, "fwdh")
        m = m.to(DEV).eval()
        tr = SupTrainer(m, lr=float(z["lr"]))
        with StepGraphs(tr) as runner:
            loss = runner.step(b, False) if graphed else tr.step(b, False)
            torch.cuda.synchronize()
            res.append((loss.detach().cpu().clone(), tr.flat.flat.detach().cpu().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_graphs_mode_training_smoke():
    """Ten fused training steps (dropout on) on one synthetic batch: finite losses, and the batch's eval loss falls."""
    from pytorch_U2GNN_Sup import TransformerU2GNN
    from u2gnn_hip.batching import BatchLoader
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.synthetic import collab_like
    from u2gnn_hip.train import SupTrainer
    np.random.seed(0)
    hb = BatchLoader(collab_like(), 8, 16)()
    torch.manual_seed(0)
    m = TransformerU2GNN(367, 512, 3, 2, 0.5, 1, precision="fwdh", attention="graphs").to(DEV).train()
    tr = SupTrainer(m, lr=1e-4, max_norm=0.5, seed=1)
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, hb.labels, device=DEV)

    def eval_loss():
        return float(tr.forward_backward(b, train=False).item())
    l0 = eval_loss()
    losses = [float(tr.step(b).item()) for _ in range(10)]
    assert all(np.isfinite(losses))
    assert eval_loss() < l0


def test_unsup_graphs_mode(golden_dir):
    """UnSup: a graph's stack outputs agree between a batch of 4 and the graph alone; one train step is finite."""
    from pytorch_U2GNN_UnSup import TransformerU2GNN
    from u2gnn_hip.core import DeviceBatch
    from u2gnn_hip.unsup import UnSupTrainer
    z = dict(np.load(os.path.join(golden_dir, "ptc_unsup.npz")))
    bs, k, T, ff, L, d, V = [int(x) for x in z["meta"]]
    torch.manual_seed(3)
    m = TransformerU2GNN(vocab_size=V, feature_dim_size=d, ff_hidden_size=ff, sampled_num=512, num_self_att_layers=T,
                         num_U2GNN_layers=L, dropout=0.5, device=DEV, attention="graphs").to(DEV).eval()
    off = z["offsets"][:5]
    n = int(off[-1])
    ix, X, iy = z["input_x"][:n], z["X"][:n], z["input_y"][:n]
    for g in range(4):
        s, e = int(off[g]), int(off[g + 1])
        assert ix[s:e].min() >= s and ix[s:e].max() < e
    b = DeviceBatch.from_offsets(ix, off, X, input_y=iy, device=DEV)
    full, _ = m.core.encode(b, False, False, 0)
    for g in range(4):
        s, e = int(off[g]), int(off[g + 1])
        one = DeviceBatch.from_offsets(ix[s:e] - s, np.array([0, e - s]), X[s:e], input_y=iy[s:e], device=DEV)
        alone, _ = m.core.encode(one, False, False, 0)
        assert _close(full[s:e], alone), g
    m.train()
    tr = UnSupTrainer(m, lr=float(z["lr"]))
    loss = tr.step(b, torch.from_numpy(z["sample_ids"]).to(DEV))
    assert np.isfinite(float(loss.item()))
