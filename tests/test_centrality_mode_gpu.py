"""``centrality=D``: the stack's input is X_concat[n] + degree_emb[min(deg[n], D)] in every attention mode.  The small
batches of tests/test_hops_mode_gpu.py: MUTAG (dp = 64; D = 3: these graphs' degrees are 1..3, so rows 1..D are used;
D = 2 clips) and IMDB-BINARY (degree tags, dp = 128; D = 8, most degrees clip), 8 fixed graphs, L = 2, T = 2, ff 32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from centrality_ref import (add_table, classes, encode_centrality, host_batch, pattern_csr,  # noqa: E402
                            sup_forward_centrality, sup_forward_centrality_neighbors)
from hops_ref import dense_bias  # noqa: E402
from test_hops_mode_gpu import BATCHES, FF, L, T, TOL, _err, _err_own_max, _gpu_fwd_bwd  # noqa: E402
from u2gnn_hip import kernels as K  # noqa: E402
from u2gnn_hip.core import Adjacency, DeviceBatch, PairTypes  # noqa: E402

DEV = "cuda"
DEPTH = {"mutag": 3, "imdbb": 8}
MODES = ["nodes", "graphs", "edges", "neighbors"]
_BATCH = {}


def _batch(name):
    """(store, classes, HostBatch, ids, degrees int64 [N])"""
    if name not in _BATCH:
        dataset, tag, ids = BATCHES[name]
        store, C, hb, _ = host_batch(dataset, tag, ids)
        _BATCH[name] = (store, C, hb, ids, store.degrees_of(ids))
    return _BATCH[name]


def _device_batch(name, mode, hops=None, distances=None, X=None, with_deg=True):
    store, _, hb, ids, deg = _batch(name)
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat if X is None else X, hb.labels, device=DEV,
                                 degrees=deg if with_deg else None)
    if mode == "edges":
        csr = store.adjacency(ids, hops=hops) if hops else store.adjacency(ids) + (None,)
        b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=DEV, etype=csr[2])
    if distances:
        b.pairs = PairTypes.from_store(store, ids, hb.N, DEV, distances)
    return b


def _model(name, precision="fp32", attention="nodes", centrality=None, hops=None, distances=None, seed=0,
           table_seed=None):
    from pytorch_U2GNN_Sup import TransformerU2GNN
    _, C, hb, _, _ = _batch(name)
    torch.manual_seed(seed)
    m = TransformerU2GNN(hb.X_concat.shape[1], FF, C, T, 0.5, L, precision=precision, attention=attention, hops=hops,
                         distances=distances, centrality=centrality)
    if table_seed is not None:
        g = torch.Generator().manual_seed(table_seed)
        with torch.no_grad():
            m.degree_emb.copy_(torch.randn(m.degree_emb.shape, generator=g))
            if hops or distances:
                m.hop_bias.copy_(torch.randn(m.hop_bias.shape, generator=g))
    return m


@pytest.mark.parametrize("mode", MODES)
def test_zero_table_is_the_model_without_centrality(mode):
    """fp32, MUTAG: X + 0.0f = X, so scores and loss are torch.equal to the same-seed model built without the keyword
    (eval and train mode); the table's own gradient is finite and not zero."""
    _, C, _, _, _ = _batch("mutag")
    for train in (False, True):
        out = []
        for D in (None, DEPTH["mutag"]):
            m = _model("mutag", "fp32", mode, centrality=D).to(DEV).train(train)
            out.append(_gpu_fwd_bwd(m, _device_batch("mutag", mode), C, train=train, seed=4242))
            torch.cuda.synchronize()
        (s0, l0, g0), (s1, l1, g1) = out
        assert torch.equal(s0, s1) and torch.equal(l0, l1), (mode, train)
        assert set(g1) - set(g0) == {"degree_emb"}
        same = [n for n in g0 if torch.equal(g0[n], g1[n])]
        print(f"zero table {mode} train={train}: {len(same)} of {len(g0)} shared gradients bit-equal")
        eg = g1["degree_emb"]
        assert eg.shape == (DEPTH["mutag"] + 1, 7) and torch.isfinite(eg).all() and eg.abs().max().item() > 0
        assert eg[0].abs().max().item() == 0.0              # no node of degree 0 in these graphs: stored, exactly 0


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fwdh"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,D", [("mutag", 3), ("imdbb", 8), ("mutag", 2)])
def test_forward_equals_the_model_fed_pre_added_features(name, D, mode, precision):
    """Eval forward, a seeded randn table E: the scores of model(centrality=D) on X equal those of the plain model on
    X + E[cls] added on the host in fp32, bit for bit -- the fused gather adds exactly that, in every mode (the
    neighbour tokens of "neighbors" included)."""
    _, _, hb, _, deg = _batch(name)
    m1 = _model(name, precision, mode, centrality=D, table_seed=21)
    E = m1.degree_emb.detach().clone()
    X2 = (torch.from_numpy(hb.X_concat) + E[torch.from_numpy(classes(deg, D))]).numpy()     # fp32 + fp32
    assert X2.dtype == np.float32
    m0 = _model(name, precision, mode)
    m1, m0 = m1.to(DEV).eval(), m0.to(DEV).eval()
    with torch.no_grad():
        s1 = m1(_device_batch(name, mode), None, None).cpu()
        s0 = m0(_device_batch(name, mode, X=X2, with_deg=False), None, None).cpu()
    assert torch.isfinite(s1).all() and torch.equal(s1, s0)
    with torch.no_grad():   # and the table matters: the plain features give other scores
        assert not torch.equal(s1, m0(_device_batch(name, mode, with_deg=False), None, None).cpu())


_TORCH_REF = {}
CONFIGS = {"nodes": ("nodes", None, None), "graphs": ("graphs", None, None), "edges": ("edges", None, None),
           "edges+hops2": ("edges", 2, None), "graphs+distances2": ("graphs", None, 2)}


def _torch_reference(name, config):
    """Scores, loss and parameter gradients (fp32, CPU) of torch.nn.TransformerEncoderLayer(d, 1, ff, 0.5) layers in
    eval mode on x = X + E[cls] (E requires grad), each layer under the mode's float mask (hops_ref.dense_bias: -inf
    outside the pattern, the layer's bias or 0 inside); pool, heads and loss as in oracle.u2gnn_oracle.  The method of
    test_hops_mode_gpu._torch_reference; once per (batch, config), shared by the precisions."""
    key = (name, config)
    if key in _TORCH_REF:
        return _TORCH_REF[key]
    from oracle import u2gnn_oracle as O
    from torch.nn import TransformerEncoder, TransformerEncoderLayer
    mode, hops, distances = CONFIGS[config]
    store, C, hb, ids, deg = _batch(name)
    d = hb.X_concat.shape[1]
    csr = pattern_csr(mode, store, ids, hb, hops, distances)
    m = _model(name, "fp32", mode, DEPTH[name], hops, distances, table_seed=11)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    stacks = torch.nn.ModuleList([TransformerEncoder(TransformerEncoderLayer(d, 1, FF, 0.5), T) for _ in range(L)])
    stacks.load_state_dict({k[len("u2gnn_layers."):]: v for k, v in sd.items() if k.startswith("u2gnn_layers.")})
    stacks.eval()
    heads = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("predictions.")}
    E = sd["degree_emb"].clone().requires_grad_(True)
    table = sd["hop_bias"].clone().requires_grad_(True) if "hop_bias" in sd else torch.zeros(L, T, 1)
    ix = torch.from_numpy(hb.input_x[:, 0])
    P = O.pool_matrix(hb.offsets)
    x = add_table(torch.from_numpy(hb.X_concat), E, deg)[ix]
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
    grads["degree_emb"] = E.grad
    if "hop_bias" in sd:
        grads["hop_bias"] = table.grad
    _TORCH_REF[key] = (sd, scores.detach(), loss.item(), grads)
    return _TORCH_REF[key]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fwdh"])
@pytest.mark.parametrize("name,config", [("mutag", c) for c in CONFIGS] + [("imdbb", c) for c in ("nodes", "graphs", "edges")])
def test_eval_vs_torch_encoder_layers(name, config, precision):
    """A seeded randn table: every score, the loss and every parameter gradient, degree_emb included, max|ours - ref| /
    max(1, max|ref|) <= 1e-3 against torch's own encoder layers on the pre-added features."""
    mode, hops, distances = CONFIGS[config]
    _, C, _, _, _ = _batch(name)
    sd, ref, lref, gref = _torch_reference(name, config)
    m = _model(name, precision, mode, DEPTH[name], hops, distances)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    scores, loss, grads = _gpu_fwd_bwd(m, _device_batch(name, mode, hops, distances), C)
    figs = {"scores": _err(scores, ref), "loss": abs(loss.item() - lref) / max(1.0, abs(lref))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], gref[n])
    assert "degree_emb" in figs and gref["degree_emb"].abs().max().item() > 0
    print(f"centrality eval parity {name} {config} {precision}: max {max(figs.values()):.3g} (scores "
          f"{figs['scores']:.3g}, degree_emb {figs['degree_emb']:.3g}, degree_emb rel own max "
          f"{_err_own_max(grads['degree_emb'], gref['degree_emb']):.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


def test_train_step_vs_float64_restatement_with_kernel_masks():
    """Train mode, fp32, MUTAG, attention="edges": the float64 restatement (tests/centrality_ref.py) fed the kernels'
    own dropout masks; the gate of the other train-mode comparisons (1e-3)."""
    from oracle import u2gnn_oracle as O
    from train_parity_util import layer_masks
    from u2gnn_hip.engine import SITE_HEAD, rup, site_seed
    store, C, hb, ids, deg = _batch("mutag")
    d = hb.X_concat.shape[1]
    m = _model("mutag", "fp32", "edges", DEPTH["mutag"], table_seed=12)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    b = _device_batch("mutag", "edges")
    seed = 987654321
    scores, loss, grads = _gpu_fwd_bwd(m, b, C, train=True, seed=seed)
    masks = {}
    for l in range(L):
        for t in range(T):
            masks[(l, t)] = layer_masks(seed, l, t, b.N, d, FF)
        masks[("head", l)] = K.dropout_mask(site_seed(seed, l, 0, SITE_HEAD), b.B, rup(d, 64), 0.5).float().cpu()[:, :d]
    ref = sup_forward_centrality(sd, hb, deg, pattern_csr("edges", store, ids, hb), L, T, True, masks)
    lref = O.soft_cross_entropy(ref, O.label_smoothing(torch.from_numpy(hb.labels), C).double())
    lref.backward()
    figs = {"scores": _err(scores, ref.detach()), "loss": abs(loss.item() - lref.item()) / max(1.0, abs(lref.item()))}
    for n, _ in m.named_parameters():
        figs[n] = _err(grads[n], sd[n].grad)
    assert sd["degree_emb"].grad.abs().max().item() > 0
    figs["degree_emb / own max"] = _err_own_max(grads["degree_emb"], sd["degree_emb"].grad)
    print(f"centrality train parity: max {max(figs.values()):.3g} (degree_emb rel own max "
          f"{figs['degree_emb / own max']:.3g})")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad


H_STEP = 2.0 ** -6


def _loss64(mode, sd, E, name):
    """The float64 restatement's eval loss with the table E."""
    from oracle import u2gnn_oracle as O
    store, C, hb, ids, deg = _batch(name)
    sd = dict(sd, degree_emb=E)
    if mode == "neighbors":
        s = sup_forward_centrality_neighbors(sd, hb, deg, L, T)
    else:
        s = sup_forward_centrality(sd, hb, deg, pattern_csr(mode, store, ids, hb), L, T)
    return O.soft_cross_entropy(s, O.label_smoothing(torch.from_numpy(hb.labels), C).double())


def _central(f, E, V, h):
    return (float(f(E + h * V)) - float(f(E - h * V))) / (2 * h)


H_SMALL = 2.0 ** -20


def test_neighbors_table_gradient_vs_central_difference():
    """attention="neighbors" has no torch-encoder or masked restatement of its backward here, so degree_emb.grad is
    checked against a central difference of the eval-mode fp32 loss, cd(h) = (L(E + hV) - L(E - hV)) / 2h formed in
    float64, along two seeded directions V (randn scaled to max|V| = 1), at h = 2^-6.

    The check itself first, on the float64 restatements of all four modes: cd(2^-20) must equal autograd's <dL/dE, V>
    within 1e-4 max(1, |<g, V>|).  (L is piecewise smooth -- ~14 000 ReLUs -- so cd's error is C h, not c h^2: C is the
    derivative's variation along V, kinks included.  The restatements give |cd(2^-6) - <g, V>| <= 0.033, i.e. C <= 2.1,
    so C h = 2e-6 at 2^-20 and the float64 rounding 1e-16 |L| / h = 1e-9: the gate leaves a factor 50.)

    Then the kernels, |cd_gpu(h) - <grad_gpu, V>| <= trunc + noise + gate at h = 2^-6, with
      trunc = |cd64(h) - <g64, V>| of the float64 neighbors restatement: the difference quotient's own error at this h
              along this direction (the reference's error, the same function at the same points);
      noise = delta / h: each of the two fp32 losses carries a rounding error of at most delta, and their difference is
              divided by 2h.  delta = 350 * 2^-24 * max(1, |L|): a score passes through about 5 d + ff + 2 (k + 1) + 10
              = 87 roundings per encoder layer at d = 7, ff = 32, k + 1 = 5 (five dot products of depth d, one of
              depth ff, the softmax and P V over the window, two LayerNorms), 4 layers, then the pool (<= 28 nodes),
              the head (d) and the cross-entropy: ~ 350 in all, each 2^-24 relative, accumulated linearly;
      gate  = 1e-3 * max(1, |<g64, V>|): the project's gate on a gradient, for <grad_gpu, V> itself.
    h = 2^-6 is where C h and delta / h meet: with |L| ~ 9 (an untrained model under a randn table) delta = 1.9e-4,
    noise = 1.2e-2, trunc ~ 1e-2 beside |<g, V>| of 3 to 8 -- a relative tolerance below 1e-2, printed per direction."""
    name = "mutag"
    _, C, hb, _, deg = _batch(name)
    D = DEPTH[name]
    base = _model(name, "fp32", "neighbors", D, table_seed=31)
    sd64 = {k: v.detach().double().clone() for k, v in base.state_dict().items()}
    E0 = sd64["degree_emb"]
    dirs = []
    for s in (41, 42):
        V = torch.randn(E0.shape, generator=torch.Generator().manual_seed(s), dtype=torch.float64)
        dirs.append(V / V.abs().max())
    trunc_nb, g64_nb = [], []
    for mode in ("nodes", "graphs", "edges", "neighbors"):           # the check on the float64 restatements
        E = E0.clone().requires_grad_(True)
        _loss64(mode, sd64, E, name).backward()
        for V in dirs:
            gv = float((E.grad * V).sum())
            with torch.no_grad():
                cd_small, cd = (_central(lambda e: _loss64(mode, sd64, e, name), E0, V, h) for h in (H_SMALL, H_STEP))
            print(f"float64 {mode}: <g, V> {gv:.6g}, |cd(2^-20) - <g, V>| {abs(cd_small - gv):.3g}, "
                  f"|cd(2^-6) - <g, V>| {abs(cd - gv):.3g}")
            assert abs(cd_small - gv) <= 1e-4 * max(1.0, abs(gv)), (mode, cd_small, gv)
            if mode == "neighbors":
                trunc_nb.append(abs(cd - gv))
                g64_nb.append(gv)
    m = _model(name, "fp32", "neighbors", D, table_seed=31).to(DEV).eval()
    b = _device_batch(name, "neighbors")
    _, loss0, grads = _gpu_fwd_bwd(m, b, C)
    g_gpu = grads["degree_emb"].detach().double().cpu().clone()
    E_dev = m.degree_emb.detach().clone()

    def gpu_loss(E):
        with torch.no_grad():
            m.degree_emb.copy_(E.float().to(DEV))
            scores = m(b, None, None)
            loss = torch.zeros(1, device=DEV)
            K.smoothed_ce(scores, b.labels, b.B, C, 0.1, loss, torch.empty_like(scores))
            m.degree_emb.copy_(E_dev)
        return loss.item()
    delta = 350 * 2.0 ** -24 * max(1.0, abs(loss0.item()))
    for V, trunc, g64 in zip(dirs, trunc_nb, g64_nb):
        gv = float((g_gpu * V).sum())
        cd = _central(gpu_loss, E_dev.double().cpu(), V, H_STEP)
        tol = trunc + delta / H_STEP + 1e-3 * max(1.0, abs(g64))
        print(f"neighbors fp32: <grad, V> {gv:.6g}, cd {cd:.6g}, float64 <g, V> {g64:.6g}; |cd - <grad, V>| "
              f"{abs(cd - gv):.3g} <= {tol:.3g} (trunc {trunc:.3g}, noise {delta / H_STEP:.3g}; relative "
              f"{tol / abs(g64):.3g})")
        assert abs(cd - gv) <= tol, (cd, gv, tol)
        assert abs(gv - g64) <= 1e-3 * max(1.0, abs(g64)), (gv, g64)     # and against the restatement's autograd


def test_centrality_steps_replay_as_a_hip_graph():
    """Three trainer steps under StepGraphs replay equal three eagerly issued ones bit for bit -- loss, every parameter,
    degree_emb.  degree_emb changes between the steps, so a table copied at capture time would fail."""
    from u2gnn_hip.train import StepGraphs, SupTrainer
    b = _device_batch("mutag", "edges", hops=2)
    res = []
    for graphed in (False, True):
        m = _model("mutag", "fwdh", "edges", DEPTH["mutag"], hops=2).to(DEV).eval()
        tr = SupTrainer(m, lr=5e-3)
        losses, tables = [], []
        with StepGraphs(tr) as runner:
            for _ in range(3):
                loss = runner.step(b, False) if graphed else tr.step(b, False)
                torch.cuda.synchronize()
                losses.append(loss.detach().cpu().clone())
                tables.append(m.degree_emb.detach().cpu().clone())
            res.append((losses, tables, tr.flat.flat.detach().cpu().clone()))
    (l0, t0, p0), (l1, t1, p1) = res
    assert t0[0].abs().max().item() > 0 and not torch.equal(t0[0], t0[1]) and not torch.equal(t0[1], t0[2])
    assert not torch.equal(l0[0], l0[1])
    for a, c in zip(l0 + t0 + [p0], l1 + t1 + [p1]):
        assert torch.equal(a, c)


def test_tensor_inputs_and_missing_degrees_raise():
    _, _, hb, _, _ = _batch("mutag")
    m = _model("mutag", "fp32", "nodes", 3).to(DEV).eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="DeviceBatch.deg"):
            m(_device_batch("mutag", "nodes", with_deg=False), None, None)
        N = hb.N
        pool = torch.sparse_coo_tensor(torch.stack([torch.zeros(N, dtype=torch.int64), torch.arange(N)]),
                                       torch.ones(N), (1, N)).to(DEV)
        with pytest.raises(ValueError, match="reference-style tensor inputs carry no edges"):
            m(torch.from_numpy(hb.input_x).to(DEV), pool, torch.from_numpy(hb.X_concat).to(DEV))


def test_from_store_gathers_the_degrees_on_the_device():
    """DeviceBatch.from_store(..., degrees=the store's on the device): the batch's rows of it, on both of its paths
    (a pinned slot through the copy stream, and plain arrays)."""
    from u2gnn_hip.batching import BatchLoader
    store, _, _, ids, deg = _batch("mutag")
    X_dev = torch.from_numpy(store.X).to(DEV)
    deg_dev = torch.from_numpy(store.deg.astype(np.int32)).to(DEV)
    hb = store.assemble(ids, 4, rng=np.random.RandomState(3), gather_x=False)
    b = DeviceBatch.from_store(hb, X_dev, device=DEV, degrees=deg_dev)
    assert b.deg.dtype == torch.int32 and np.array_equal(b.deg.cpu().numpy(), deg)
    loader = BatchLoader(store, 8, 4, rng=np.random.RandomState(3), gather_x=False)
    hb = loader()
    assert hb.pinned is not None
    b = DeviceBatch.from_store(hb, X_dev, device=DEV, degrees=deg_dev)
    torch.cuda.synchronize()
    assert np.array_equal(b.deg.cpu().numpy(), store.degrees_of(hb.graph_ids))
    assert DeviceBatch.from_store(loader(), X_dev, device=DEV).deg is None
    with pytest.raises(ValueError, match="degrees"):
        DeviceBatch.from_store(loader(), X_dev, device=DEV, degrees=deg_dev.long())


def test_unsup_eval_vs_float64_restatement():
    """UnSup on PTC, attention="edges", centrality = 3, eval: the summed loss and every trainable gradient (degree_emb
    included) against the float64 restatement; 1e-3, the bar of this file's other comparisons."""
    from oracle import u2gnn_oracle as O
    from pytorch_U2GNN_UnSup import TransformerU2GNN
    from u2gnn_hip.unsup import UnSupTrainer
    D = 3
    ids = [2, 9, 31, 44]
    store, _, hb, _ = host_batch("PTC", False, ids, with_input_y=True)
    deg = store.degrees_of(ids)
    V = int(store.node_start[-1])
    torch.manual_seed(3)
    m = TransformerU2GNN(vocab_size=V, feature_dim_size=store.d, ff_hidden_size=FF, sampled_num=256,
                         num_self_att_layers=T, num_U2GNN_layers=L, dropout=0.5, device=DEV, attention="edges",
                         centrality=D)
    with torch.no_grad():
        m.degree_emb.copy_(torch.randn(D + 1, store.d, generator=torch.Generator().manual_seed(14)))
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()
          if k.startswith("u2gnn_layers.") or k in ("ss.weight", "degree_emb")}
    m = m.to(DEV).eval()
    b = DeviceBatch.from_offsets(hb.input_x, hb.offsets, hb.X_concat, input_y=hb.input_y, device=DEV, degrees=deg)
    csr = store.adjacency(ids)
    b.adj = Adjacency.from_csr(csr[0], csr[1], hb.N, device=DEV)
    tr = UnSupTrainer(m, lr=5e-4)
    assert tr.flat.names[-1] == "degree_emb"
    sid = torch.from_numpy(m.ss.draw_samples()).to(DEV)
    loss = tr.forward_backward(b, sid, train=False)
    torch.cuda.synchronize()
    outs = encode_centrality(sd, hb, deg, pattern_csr("edges", store, ids, hb), L, T)
    ref = O.sampled_softmax_logits(torch.cat(outs, 1), torch.from_numpy(hb.input_y), sd["ss.weight"], sid.cpu()).sum()
    ref.backward()
    figs = {"loss": abs(loss.item() - ref.item()) / max(1.0, abs(ref.item()))}
    for n in tr.flat.names:
        figs[n] = _err(tr.flat.grads[n], sd[n].grad)
    assert "degree_emb" in figs and sd["degree_emb"].grad.abs().max().item() > 0
    figs["degree_emb / own max"] = _err_own_max(tr.flat.grads["degree_emb"], sd["degree_emb"].grad)
    print(f"unsup centrality eval parity: max {max(figs.values()):.3g}")
    bad = {k: v for k, v in figs.items() if not v <= TOL}
    assert not bad, bad
