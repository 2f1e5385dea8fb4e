"""attention="edges": every node attends over itself and its graph neighbours (the batch's adjacency plus the
diagonal).  Batches: MUTAG (d = 7, dp = 64) and IMDB-BINARY (degree tags, the dp = 128 class) from dataset/, fixed
graph ids, 8 graphs, L = 2, T = 2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from edges_ref import block_csr, csr_to_dense, dense_to_csr, host_batch, rewire, sup_forward_edges  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip.core import Adjacency, DeviceBatch  # noqa: E402

DEV = "cuda"
TOL = 1e-3
L, T, FF = 2, 2, 128
BATCHES = {"mutag": ("MUTAG", False, [0, 5, 17, 23, 42, 77, 101, 150]),
           "imdbb": ("IMDBBINARY", True, [1, 40, 123, 250, 377, 512, 700, 901])}


def _err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def _batch(name):
    dataset, deg, ids = BATCHES[name]
    store, C, hb, csr = host_batch(dataset, deg, ids)
    return store, C, hb, csr


def _device_batch(hb, csr):
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, hb.labels, device=DEV)
    if csr is not None:
        b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=DEV)
    return b


def _model(d, C, precision="fp32", attention="edges", seed=0):
    from pytorch_U2GNN_Sup import TransformerU2GNN
    torch.manual_seed(seed)
    return TransformerU2GNN(d, FF, C, T, 0.5, L, precision=precision, attention=attention)


def _gpu_fwd_bwd(m, b, C, train=False, seed=0):
    flat = m.flatten_parameters()
    scores, ctx = m.core.forward(b, train=train, need_ctx=True, seed=seed)
    dsc = torch.empty_like(scores)
    loss = torch.zeros(1, device=DEV)
    K.smoothed_ce(scores, b.labels, b.B, C, 0.1, loss, dsc)
    m.core.backward(ctx, dsc, flat.grads)
    return scores, loss, flat.grads


_TORCH_REF = {}


def _torch_reference(name):
    """Scores, loss and parameter gradients (fp32, CPU) of torch.nn.TransformerEncoderLayer(d, 1, ff, 0.5) stacks
    in eval mode under the float -inf adjacency mask, on the module's own state_dict; pool, heads and loss as in
    oracle.u2gnn_oracle.  Computed once per batch and shared by the precisions."""
    if name in _TORCH_REF:
        return _TORCH_REF[name]
    from oracle import u2gnn_oracle as O
    from torch.nn import TransformerEncoder, TransformerEncoderLayer
    _, C, hb, csr = _batch(name)
    d = hb.X_concat.shape[1]
    sd = {k: v.detach().clone() for k, v in _model(d, C).state_dict().items()}
    stacks = torch.nn.ModuleList([TransformerEncoder(TransformerEncoderLayer(d, 1, FF, 0.5), T) for _ in range(L)])
    stacks.load_state_dict({k[len("u2gnn_layers."):]: v for k, v in sd.items() if k.startswith("u2gnn_layers.")})
    stacks.eval()
    heads = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("predictions.")}
    allowed = torch.from_numpy(csr_to_dense(csr[0], csr[1], hb.N) > 0)
    mask = torch.zeros(hb.N, hb.N).masked_fill(~allowed, float("-inf"))
    ix = torch.from_numpy(hb.input_x[:, 0])
    P = O.pool_matrix(hb.offsets)
    x = torch.from_numpy(hb.X_concat)[ix]
    scores = 0
    for l in range(L):
        out = stacks[l](x[:, None, :], mask=mask)[:, 0, :]
        x = out[ix]
        scores = scores + (P @ out) @ heads[f"predictions.{l}.weight"].t() + heads[f"predictions.{l}.bias"]
    loss = O.soft_cross_entropy(scores, O.label_smoothing(torch.from_numpy(hb.labels), C))
    loss.backward()
    grads = {"u2gnn_layers." + k: p.grad for k, p in stacks.named_parameters()}
    grads.update({k: v.grad for k, v in heads.items()})
    _TORCH_REF[name] = (sd, scores.detach(), loss.item(), grads)
    return _TORCH_REF[name]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fwdh"])
@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_edges_mode_eval_vs_torch_encoder_layers(name, precision):
    """Scores, loss and every parameter gradient, max|ours - ref| / max(1, max|ref|) <= 1e-3 (the project's bar)
    against an independent reference: torch's own TransformerEncoderLayer stacks with mask= the adjacency.
    Measured maxima (MUTAG / IMDB-BINARY): fp32 6.8e-7 / 2.1e-6, bf16x3 1.1e-5 / 7.3e-6, fwdh 5.3e-6 / 9.0e-6."""
    _, C, hb, csr = _batch(name)
    sd, ref, lref, gref = _torch_reference(name)
    m = _model(hb.X_concat.shape[1], C, precision)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    scores, loss, grads = _gpu_fwd_bwd(m, _device_batch(hb, csr), C)
    figs = {"scores": _err(scores, ref), "loss": abs(loss.item() - lref) / max(1.0, abs(lref))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], gref[n])
    print(f"edges-mode eval parity {name} {precision}: max {max(figs.values()):.3g} "
          f"(scores {figs['scores']:.3g}, loss {figs['loss']:.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def test_edges_mode_train_step_vs_float64_restatement_with_kernel_masks():
    """Train mode, fp32, MUTAG: the float64 restatement (tests/edges_ref.py) fed the kernels' own masks, the attention
    mask taken at [i, j]; gate 1e-3 (measured 2.7e-7)."""
    from oracle import u2gnn_oracle as O
    from train_parity_util import layer_masks
    from u2gnn_hip.engine import SITE_HEAD, rup, site_seed
    _, C, hb, csr = _batch("mutag")
    d = hb.X_concat.shape[1]
    m = _model(d, C, "fp32")
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    b = _device_batch(hb, csr)
    seed = 987654321
    scores, loss, grads = _gpu_fwd_bwd(m, b, C, train=True, seed=seed)
    masks = {}
    for l in range(L):
        for t in range(T):
            masks[(l, t)] = layer_masks(seed, l, t, b.N, d, FF)
        masks[("head", l)] = K.dropout_mask(site_seed(seed, l, 0, SITE_HEAD), b.B, rup(d, 64), 0.5).float().cpu()[:, :d]
    allowed = torch.from_numpy(csr_to_dense(csr[0], csr[1], hb.N) > 0)
    ref = sup_forward_edges(sd, hb.input_x, hb.offsets, torch.from_numpy(hb.X_concat).double(), allowed, L, T, True,
                            masks)
    lref = O.soft_cross_entropy(ref, O.label_smoothing(torch.from_numpy(hb.labels), C).double())
    lref.backward()
    figs = {"scores": _err(scores, ref.detach()), "loss": abs(loss.item() - lref.item()) / max(1.0, abs(lref.item()))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], sd[n].grad)
    print(f"edges-mode train parity: max {max(figs.values()):.3g}")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def _single(store, hb, csr, g):
    """Graph g of the batch as a batch of its own (rows, slots and adjacency rebased)."""
    s, e = int(hb.offsets[g]), int(hb.offsets[g + 1])
    A = csr_to_dense(csr[0], csr[1], hb.N)[s:e, s:e]
    b = DeviceBatch.from_offsets(hb.input_x[s:e] - s, np.array([0, e - s]), hb.X_concat[s:e], hb.labels[g:g + 1],
                                 device=DEV)
    b.adj = Adjacency.from_csr(*dense_to_csr(A), e - s, device=DEV)
    return b


@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_graph_scores_do_not_depend_on_the_batch(name):
    """fp32, eval: the logits of graph g in the batch of 8 equal those of a batch holding g alone, bit for bit."""
    store, C, hb, csr = _batch(name)
    m = _model(hb.X_concat.shape[1], C, "fp32").to(DEV).eval()
    with torch.no_grad():
        full = m(_device_batch(hb, csr), None, None).cpu()
        alone = torch.cat([m(_single(store, hb, csr, g), None, None).cpu() for g in range(len(hb.labels))])
    print(f"edges-mode batch invariance {name}: max |diff| {(full - alone).abs().max().item():.3g}")
    assert torch.equal(full, alone)


def test_scores_depend_on_the_edges_of_their_own_graph_only():
    """One degree-preserving edge swap inside graph 3 (same features, same degrees): that graph's logits change, no
    other graph's do; under attention="graphs" the same rewiring changes nothing."""
    _, C, hb, csr = _batch("mutag")
    g = 3
    s, e = int(hb.offsets[g]), int(hb.offsets[g + 1])
    A = csr_to_dense(csr[0], csr[1], hb.N)
    A2 = rewire(A, s, e)
    assert (A2 != A).sum() == 8 and np.array_equal(A2.sum(1), A.sum(1)) and np.array_equal(A2.sum(0), A.sum(0))
    csr2 = dense_to_csr(A2)
    out = {}
    for mode in ("edges", "graphs"):
        m = _model(hb.X_concat.shape[1], C, "fp32", attention=mode).to(DEV).eval()
        with torch.no_grad():
            out[mode] = (m(_device_batch(hb, csr), None, None).cpu(), m(_device_batch(hb, csr2), None, None).cpu())
    a, b = out["edges"]
    others = [i for i in range(len(hb.labels)) if i != g]
    assert not torch.equal(a[g], b[g])
    assert torch.equal(a[others], b[others])
    assert torch.equal(*out["graphs"])


@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_complete_graph_adjacency_equals_graphs_mode(name):
    _, C, hb, _ = _batch(name)
    outs = {}
    for mode, csr in (("edges", block_csr(hb.offsets)), ("graphs", None)):
        m = _model(hb.X_concat.shape[1], C, "fp32", attention=mode).to(DEV).eval()
        with torch.no_grad():
            outs[mode] = m(_device_batch(hb, csr), None, None).cpu()
    err = _err(outs["edges"], outs["graphs"])
    print(f"edges mode on complete graphs vs graphs mode {name}: {err:.3g}")
    assert err <= 1e-5


def test_edges_mode_needs_an_adjacency():
    """A DeviceBatch without adj, and reference-style tensor inputs (they carry no edges): a ValueError that names
    Adjacency.from_csr; nodes mode runs on the same inputs."""
    _, C, hb, _ = _batch("mutag")
    d = hb.X_concat.shape[1]
    m = _model(d, C).to(DEV).eval()
    off = hb.offsets
    idx = torch.tensor([[g, j] for g in range(len(off) - 1) for j in range(off[g], off[g + 1])]).t()
    pool = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1]), (len(off) - 1, hb.N)).to(DEV)
    ix, X = torch.from_numpy(hb.input_x).to(DEV), torch.from_numpy(hb.X_concat).to(DEV)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"Adjacency\.from_csr"):
            m(_device_batch(hb, None), None, None)
        with pytest.raises(ValueError, match=r"Adjacency\.from_csr"):
            m(ix, pool, X)
        assert torch.isfinite(_model(d, C, attention="nodes").to(DEV).eval()(ix, pool, X)).all()


def test_edges_mode_step_replays_as_a_hip_graph():
    """One trainer step under StepGraphs replay equals the eagerly issued step bit for bit (both on the device-side
    Adam schedule that StepGraphs switches on): nothing in the path synchronises with the host or depends on it."""
    from u2gnn_hip.train import StepGraphs, SupTrainer
    _, C, hb, csr = _batch("mutag")
    b = _device_batch(hb, csr)
    res = []
    for graphed in (False, True):
        m = _model(hb.X_concat.shape[1], C, "fwdh").to(DEV).eval()
        tr = SupTrainer(m, lr=5e-4)
        with StepGraphs(tr) as runner:
            loss = runner.step(b, False) if graphed else tr.step(b, False)
            torch.cuda.synchronize()
            res.append((loss.detach().cpu().clone(), tr.flat.flat.detach().cpu().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_edges_mode_training_smoke():
    """Twenty fused training steps (dropout on) on the MUTAG batch: finite losses, and the batch's eval loss falls."""
    from u2gnn_hip.train import SupTrainer
    _, C, hb, csr = _batch("mutag")
    m = _model(hb.X_concat.shape[1], C, "fwdh").to(DEV).train()
    tr = SupTrainer(m, lr=5e-4, max_norm=0.5, seed=1)
    b = _device_batch(hb, csr)

    def eval_loss():
        return float(tr.forward_backward(b, train=False).item())
    l0 = eval_loss()
    losses = [float(tr.step(b).item()) for _ in range(20)]
    assert all(np.isfinite(losses))
    l1 = eval_loss()
    print(f"edges-mode training smoke: eval loss {l0:.4f} -> {l1:.4f}")
    assert l1 < l0


def test_unsup_edges_mode():
    """UnSup on PTC: one train step has a finite loss and finite gradients, and they are not all zero."""
    from pytorch_U2GNN_UnSup import TransformerU2GNN
    from u2gnn_hip.unsup import UnSupTrainer
    ids = [2, 9, 31, 44]
    store, _, hb, csr = host_batch("PTC", False, ids, with_input_y=True)
    V = int(store.node_start[-1])
    torch.manual_seed(3)
    m = TransformerU2GNN(vocab_size=V, feature_dim_size=store.d, ff_hidden_size=FF, sampled_num=256,
                         num_self_att_layers=T, num_U2GNN_layers=L, dropout=0.5, device=DEV,
                         attention="edges").to(DEV).train()
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, input_y=hb.input_y, device=DEV)
    b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=DEV)
    tr = UnSupTrainer(m, lr=5e-4)
    sid = torch.from_numpy(m.ss.draw_samples()).to(DEV)
    loss = tr.forward_backward(b, sid, train=True)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.item()))
    g = tr.flat.gflat
    assert torch.isfinite(g).all() and g.abs().max().item() > 0
    assert np.isfinite(float(tr.step(b, sid).item()))
