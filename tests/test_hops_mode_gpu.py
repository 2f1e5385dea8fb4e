"""attention="edges" with ``hops=H``: every node attends over the nodes of its graph within H bonds and each encoder
layer adds hop_bias[l][t][distance] to its scores.  The small batches of tests/test_edges_mode_gpu.py: MUTAG (dp = 64)
and IMDB-BINARY (degree tags, dp = 128), 8 fixed graphs, L = 2, T = 2, ff 32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from edges_ref import host_batch  # noqa: E402
from hops_ref import dense_bias, encode_hops, sup_forward_hops  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip.core import Adjacency, DeviceBatch  # noqa: E402

DEV = "cuda"
TOL = 1e-3
L, T, FF = 2, 2, 32
BATCHES = {"mutag": ("MUTAG", False, [0, 5, 17, 23, 42, 77, 101, 150]),
           "imdbb": ("IMDBBINARY", True, [1, 40, 123, 250, 377, 512, 700, 901])}


def _err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def _err_own_max(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _batch(name, hops):
    """(store, classes, HostBatch, (rowptr, colidx, etype)); hops None: the plain adjacency, etype None."""
    dataset, deg, ids = BATCHES[name]
    store, C, hb, csr = host_batch(dataset, deg, ids)
    return store, C, hb, (store.adjacency(ids, hops=hops) if hops else csr + (None,))


def _device_batch(hb, csr):
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, hb.labels, device=DEV)
    b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=DEV, etype=csr[2])
    return b


def _model(d, C, precision="fp32", hops=None, seed=0, table_seed=None):
    from pytorch_U2GNN_Sup import TransformerU2GNN
    torch.manual_seed(seed)
    m = TransformerU2GNN(d, FF, C, T, 0.5, L, precision=precision, attention="edges", hops=hops)
    if table_seed is not None:
        with torch.no_grad():
            m.hop_bias.copy_(torch.randn(L, T, hops + 1, generator=torch.Generator().manual_seed(table_seed)))
    return m


def _gpu_fwd_bwd(m, b, C, train=False, seed=0):
    flat = m.flatten_parameters()
    scores, ctx = m.core.forward(b, train=train, need_ctx=True, seed=seed)
    dsc = torch.empty_like(scores)
    loss = torch.zeros(1, device=DEV)
    K.smoothed_ce(scores, b.labels, b.B, C, 0.1, loss, dsc)
    m.core.backward(ctx, dsc, flat.grads)
    return scores, loss, flat.grads


_TORCH_REF = {}


def _torch_reference(name, H):
    """Scores, loss and parameter gradients (fp32, CPU) of torch.nn.TransformerEncoderLayer(d, 1, ff, 0.5) layers in
    eval mode, each under its own float mask (-inf outside the H-hop pattern, hop_bias[l][t][distance] inside), on the
    module's own state_dict; pool, heads and loss as in oracle.u2gnn_oracle.  Once per batch, shared by the
    precisions."""
    if name in _TORCH_REF:
        return _TORCH_REF[name]
    from oracle import u2gnn_oracle as O
    from torch.nn import TransformerEncoder, TransformerEncoderLayer
    _, C, hb, csr = _batch(name, H)
    d = hb.X_concat.shape[1]
    sd = {k: v.detach().clone() for k, v in _model(d, C, hops=H, table_seed=11).state_dict().items()}
    stacks = torch.nn.ModuleList([TransformerEncoder(TransformerEncoderLayer(d, 1, FF, 0.5), T) for _ in range(L)])
    stacks.load_state_dict({k[len("u2gnn_layers."):]: v for k, v in sd.items() if k.startswith("u2gnn_layers.")})
    stacks.eval()
    heads = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("predictions.")}
    table = sd["hop_bias"].clone().requires_grad_(True)
    ix = torch.from_numpy(hb.input_x[:, 0])
    P = O.pool_matrix(hb.offsets)
    x = torch.from_numpy(hb.X_concat)[ix]
    scores = 0
    for l in range(L):
        out = x[:, None, :]
        for t in range(T):
            out = stacks[l].layers[t](out, src_mask=dense_bias(*csr, hb.N, table[l, t], torch.float32))
        out = out[:, 0, :]
        x = out[ix]
        scores = scores + (P @ out) @ heads[f"predictions.{l}.weight"].t() + heads[f"predictions.{l}.bias"]
    loss = O.soft_cross_entropy(scores, O.label_smoothing(torch.from_numpy(hb.labels), C))
    loss.backward()
    grads = {"u2gnn_layers." + k: p.grad for k, p in stacks.named_parameters()}
    grads.update({k: v.grad for k, v in heads.items()})
    grads["hop_bias"] = table.grad
    _TORCH_REF[name] = (sd, scores.detach(), loss.item(), grads)
    return _TORCH_REF[name]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fwdh"])
@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_hops_eval_vs_torch_encoder_layers(name, precision):
    """hops = 3, hop_bias = seeded randn: scores, loss and every parameter gradient (hop_bias included), max|ours -
    ref| / max(1, max|ref|) <= 1e-3 against torch's own encoder layers under the float mask."""
    H = 3
    _, C, hb, csr = _batch(name, H)
    sd, ref, lref, gref = _torch_reference(name, H)
    m = _model(hb.X_concat.shape[1], C, precision, hops=H)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    scores, loss, grads = _gpu_fwd_bwd(m, _device_batch(hb, csr), C)
    figs = {"scores": _err(scores, ref), "loss": abs(loss.item() - lref) / max(1.0, abs(lref))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], gref[n])
    assert "hop_bias" in figs and gref["hop_bias"].abs().max().item() > 0
    print(f"hops eval parity {name} {precision} nnz={len(csr[1])}: max {max(figs.values()):.3g} "
          f"(scores {figs['scores']:.3g}, hop_bias {figs['hop_bias']:.3g}, "
          f"hop_bias rel own max {_err_own_max(grads['hop_bias'], gref['hop_bias']):.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def test_hops_train_step_vs_float64_restatement_with_kernel_masks():
    """Train mode, fp32, MUTAG, hops = 3: the float64 restatement (tests/hops_ref.py) fed the kernels' own masks; the
    gate of the train-mode edges test (1e-3), hop_bias.grad relative to its own max."""
    from oracle import u2gnn_oracle as O
    from train_parity_util import layer_masks
    from u2gnn_hip.engine import SITE_HEAD, rup, site_seed
    H = 3
    _, C, hb, csr = _batch("mutag", H)
    d = hb.X_concat.shape[1]
    m = _model(d, C, "fp32", hops=H, table_seed=12)
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
    ref = sup_forward_hops(sd, hb.input_x, hb.offsets, torch.from_numpy(hb.X_concat).double(), csr, L, T, True, masks)
    lref = O.soft_cross_entropy(ref, O.label_smoothing(torch.from_numpy(hb.labels), C).double())
    lref.backward()
    figs = {"scores": _err(scores, ref.detach()), "loss": abs(loss.item() - lref.item()) / max(1.0, abs(lref.item()))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], sd[n].grad)
    figs["hop_bias / own max"] = _err_own_max(grads["hop_bias"], sd["hop_bias"].grad)
    print(f"hops train parity: max {max(figs.values()):.3g} (hop_bias rel own max {figs['hop_bias / own max']:.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


@pytest.mark.parametrize("train", [False, True])
def test_one_hop_with_a_zero_table_is_plain_edges_mode(train):
    """hops = 1 lists today's pattern and a zero table adds 0.0f: scores and every shared gradient are torch.equal to
    the attention="edges" model of the same seed; hop_bias's own gradient is finite and not zero."""
    _, C, hb, csr1 = _batch("mutag", 1)
    _, _, _, csr0 = _batch("mutag", None)
    assert np.array_equal(csr0[0], csr1[0]) and np.array_equal(csr0[1], csr1[1])
    d = hb.X_concat.shape[1]
    out = []
    for hops, csr in ((None, csr0), (1, csr1)):
        m = _model(d, C, "fp32", hops=hops).to(DEV).train(train)
        scores, loss, grads = _gpu_fwd_bwd(m, _device_batch(hb, csr), C, train=train, seed=4242)
        torch.cuda.synchronize()
        out.append((scores, loss, grads))
    (s0, l0, g0), (s1, l1, g1) = out
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    assert set(g1) - set(g0) == {"hop_bias"}
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    hg = g1["hop_bias"]
    assert hg.shape == (L, T, 2) and torch.isfinite(hg).all() and hg.abs().max().item() > 0


def _single(hb, csr, g, hops, store, ids):
    s, e = int(hb.offsets[g]), int(hb.offsets[g + 1])
    b = DeviceBatch.from_offsets(hb.input_x[s:e] - s, np.array([0, e - s]), hb.X_concat[s:e], hb.labels[g:g + 1],
                                 device=DEV)
    rp, ci, et = store.adjacency([ids[g]], hops=hops)
    b.adj = Adjacency.from_csr(rp, ci, e - s, device=DEV, etype=et)
    return b


@pytest.mark.parametrize("name", ["mutag", "imdbb"])
def test_graph_scores_do_not_depend_on_the_batch(name):
    """fp32, eval, hops = 2, a random table: the logits of graph g in the batch of 8 equal those of g alone, bit for
    bit."""
    H = 2
    store, C, hb, csr = _batch(name, H)
    ids = BATCHES[name][2]
    m = _model(hb.X_concat.shape[1], C, "fp32", hops=H, table_seed=13).to(DEV).eval()
    with torch.no_grad():
        full = m(_device_batch(hb, csr), None, None).cpu()
        alone = torch.cat([m(_single(hb, csr, g, H, store, ids), None, None).cpu() for g in range(len(hb.labels))])
    assert torch.equal(full, alone)


def test_hops_steps_replay_as_a_hip_graph():
    """Three trainer steps under StepGraphs replay equal three eagerly issued ones bit for bit -- loss, every
    parameter, hop_bias.  hop_bias changes between the steps, so a table copied at capture time would fail."""
    from u2gnn_hip.train import StepGraphs, SupTrainer
    H = 2
    _, C, hb, csr = _batch("mutag", H)
    b = _device_batch(hb, csr)
    res = []
    for graphed in (False, True):
        m = _model(hb.X_concat.shape[1], C, "fwdh", hops=H).to(DEV).eval()
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
    assert t0[0].abs().max().item() > 0 and not torch.equal(t0[0], t0[1]) and not torch.equal(t0[1], t0[2])
    assert not torch.equal(l0[0], l0[1])
    for a, c in zip(l0 + t0 + [p0], l1 + t1 + [p1]):
        assert torch.equal(a, c)


def test_hops_training_smoke():
    """Ten fused training steps (dropout on) on a MUTAG batch of 16 graphs, hops = 3: finite losses, and hop_bias
    leaves zero."""
    from u2gnn_hip.train import SupTrainer
    ids = list(range(3, 188, 12))[:16]
    store, C, hb, _ = host_batch("MUTAG", False, ids)
    assert len(ids) == 16
    m = _model(hb.X_concat.shape[1], C, "fwdh", hops=3).to(DEV).train()
    tr = SupTrainer(m, lr=5e-4, max_norm=0.5, seed=1)
    b = _device_batch(hb, store.adjacency(ids, hops=3))
    losses = [float(tr.step(b).item()) for _ in range(10)]
    assert all(np.isfinite(losses))
    assert torch.isfinite(m.hop_bias).all() and m.hop_bias.abs().max().item() > 0


def test_hops_needs_entry_types_that_fit_the_table():
    _, C, hb, csr3 = _batch("mutag", 3)
    m = _model(hb.X_concat.shape[1], C, "fp32", hops=2).to(DEV).eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="etype"):
            m(_device_batch(hb, (csr3[0], csr3[1], None)), None, None)
        with pytest.raises(ValueError, match="distances up to 3"):
            m(_device_batch(hb, csr3), None, None)
        assert torch.isfinite(m(_device_batch(hb, _batch("mutag", 1)[3]), None, None)).all()   # fewer types: fine


def test_unsup_hops_eval_vs_float64_restatement():
    """UnSup on PTC, hops = 2, eval: the summed loss and every trainable gradient (hop_bias included) against the
    float64 restatement; 1e-3, the bar of this file's other comparisons."""
    from oracle import u2gnn_oracle as O
    from pytorch_U2GNN_UnSup import TransformerU2GNN
    from u2gnn_hip.unsup import UnSupTrainer
    H = 2
    ids = [2, 9, 31, 44]
    store, _, hb, _ = host_batch("PTC", False, ids, with_input_y=True)
    csr = store.adjacency(ids, hops=H)
    V = int(store.node_start[-1])
    torch.manual_seed(3)
    m = TransformerU2GNN(vocab_size=V, feature_dim_size=store.d, ff_hidden_size=FF, sampled_num=256,
                         num_self_att_layers=T, num_U2GNN_layers=L, dropout=0.5, device=DEV, attention="edges", hops=H)
    with torch.no_grad():
        m.hop_bias.copy_(torch.randn(L, T, H + 1, generator=torch.Generator().manual_seed(14)))
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()
          if k.startswith("u2gnn_layers.") or k in ("ss.weight", "hop_bias")}
    m = m.to(DEV).eval()
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, input_y=hb.input_y, device=DEV)
    b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=DEV, etype=csr[2])
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
    print(f"unsup hops eval parity: max {max(figs.values()):.3g}")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad
