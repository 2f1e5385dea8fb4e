"""Drop-in replacement of U2GNN_pytorch/pytorch_U2GNN_Sup.py on MI355X.

Same class name, constructor, ``forward(input_x, graph_pool, X_concat)`` signature,
parameter construction order (so ``torch.manual_seed`` gives identical initial weights) and
state_dict keys as the reference (pytorch_U2GNN_Sup.py:7-46).  The torch.nn encoder modules
are only parameter containers here: the computation runs on the gfx950 kernels of
libu2gnn_hip.so through ``u2gnn_hip.core.SupCore`` (no CPU fallback — the forward raises if
the HIP library or a GPU is missing).

Extra keywords (not in the reference): ``precision`` = "fp32" (exact fp32 matrix cores,
the parity path), "bf16x3" (split-bf16, ~2^-16 per product), "mixed" (bf16x3 with the
attention-backward products dS, dQ, dK on plain bf16; an experiment, see
u2gnn_hip.engine.MIXED_BF16_ROLES), "fwd32" (exact fp32 forward products, bf16x3 backward: the
forward's ReLU decisions carry fp32 rounding only), "fwd6" (the forward products on the
three-plane bf16x6 split -- fp32-accurate products on bf16 matrix cores -- bf16x3 backward) or "bf16" (experiments
only); ``attention`` = "nodes" (the fork's semantics: the encoder's sequence axis is
the node axis, pytorch_U2GNN_Sup.py:35), "neighbors" (the paper / TF semantics: each node
attends over its own k+1 sampled neighbours, U2GNN_tf/model_U2GNN_Sup_multi.py:14-45) or "graphs"
(the "nodes" encoder applied to every graph on its own: a node attends over the nodes of its graph,
so a graph's scores do not depend on the other graphs of the batch; it needs each graph's nodes as
consecutive rows, which ``forward`` checks on its graph_pool) or "edges" (a node attends over itself and its
graph neighbours: the batch's adjacency plus the diagonal, ``DeviceBatch.adj`` =
``Adjacency.from_csr(*store.adjacency(graph_ids), N, device)``, or -- the same integers without the per-batch host
work -- ``DeviceGraphs.from_store(store, device, hops)`` once per dataset and then ``graphs.adjacency(graph_ids)`` or
``DeviceBatch.from_store(hb, X_dev, graphs=graphs)`` per batch; structure-aware without sampling and, as "graphs",
independent of the batch; reference-style tensor inputs carry no edges, so ``forward`` raises a ValueError for them);
``hops`` = None, or H in [1, 31] with attention="edges": a node attends over every node of its graph within H bonds
(``Adjacency.from_csr(rowptr, colidx, N, device, etype=etype)`` of ``store.adjacency(graph_ids, hops=H)``) and each
encoder layer adds a learned scalar per shortest-path distance to its scores: ONE more parameter, ``hop_bias``
[L, T, H + 1], zero-initialised and registered after every other, so the rest of the model keeps its values under a
seed and, without ``hops``, the state_dict keys are the reference's;
``distances`` = None, or H in [1, 31] with attention="graphs" (and without ``hops``): every node still attends over ALL
nodes of its graph, and each encoder layer adds hop_bias[l][t][min(shortest-path distance, H)] to the score of a pair
(index H also for a pair no path joins) -- Graphormer's spatial encoding on the per-graph kernels.  The same ONE more
parameter ``hop_bias`` [L, T, H + 1] (zeros, registered last); the batch carries the pair types as
``DeviceBatch.pairs`` = ``PairTypes.from_store(store, graph_ids, N, device, H)``;
``centrality`` = None / 0, or D in [1, 63], with any ``attention``: Graphormer's centrality encoding -- the stack's input
is X_concat[n] + degree_emb[min(degree of n, D)], one more parameter ``degree_emb`` [D + 1, feature_dim_size]
(zeros, registered after every reference parameter and before ``hop_bias``), added inside the first gather, so every
gathered row (the neighbour tokens of "neighbors" too) carries the vector of the node it was gathered from; the
re-gather between U2GNN layers is untouched.  The batch carries the nodes' degrees as ``DeviceBatch.deg``
(``from_offsets(..., degrees=store.degrees_of(graph_ids))`` or ``from_store(..., degrees=...)``; reference-style tensor
inputs carry no edges, so ``forward`` raises a ValueError for them).
"""
import torch
import torch.nn as nn
from torch.nn import TransformerEncoder, TransformerEncoderLayer

from u2gnn_hip.core import (DeviceBatch, FlatParams, SupCore, check_attention, check_centrality, check_distances,
                            check_hops, hop_bias_last)


class _SupFunction(torch.autograd.Function):
    @staticmethod
    def forward(fctx, core, batch, train, seed, names, *params):
        scores, ctx = core.forward(batch, train, need_ctx=True, seed=seed)
        fctx.core, fctx.ctx, fctx.names, fctx.params = core, ctx, names, params
        return scores

    @staticmethod
    def backward(fctx, dscores):
        params = fctx.params
        grads = {n: torch.empty_like(p) for n, p in zip(fctx.names, params)}
        fctx.core.backward(fctx.ctx, dscores.contiguous(), grads)
        fctx.ctx = None
        return (None, None, None, None, None) + tuple(grads[n] for n in fctx.names)


class TransformerU2GNN(nn.Module):

    def __init__(self, feature_dim_size, ff_hidden_size, num_classes,
                 num_self_att_layers, dropout, num_U2GNN_layers, precision="fp32", attention="nodes", hops=None,
                 distances=None, centrality=None):
        super(TransformerU2GNN, self).__init__()
        self.feature_dim_size = feature_dim_size
        self.ff_hidden_size = ff_hidden_size
        self.num_classes = num_classes
        self.num_self_att_layers = num_self_att_layers
        self.num_U2GNN_layers = num_U2GNN_layers
        self.dropout_p = dropout
        self.precision = precision
        self.attention = check_attention(attention)
        self.hops = check_hops(hops, attention)
        self.distances = check_distances(distances, attention, hops)
        self.centrality = check_centrality(centrality)
        # parameter containers built in the reference's order (identical init under a seed)
        self.u2gnn_layers = torch.nn.ModuleList()
        for _ in range(self.num_U2GNN_layers):
            encoder_layers = TransformerEncoderLayer(d_model=self.feature_dim_size, nhead=1,
                                                     dim_feedforward=self.ff_hidden_size, dropout=0.5)
            self.u2gnn_layers.append(TransformerEncoder(encoder_layers, self.num_self_att_layers,
                                                        enable_nested_tensor=False))
        self.predictions = torch.nn.ModuleList()
        self.dropouts = torch.nn.ModuleList()
        for _ in range(self.num_U2GNN_layers):
            self.predictions.append(nn.Linear(self.feature_dim_size, self.num_classes))
            self.dropouts.append(nn.Dropout(dropout))
        if self.centrality:   # after every reference parameter; zeros: torch's generator is not touched
            self.degree_emb = nn.Parameter(torch.zeros(self.centrality + 1, self.feature_dim_size))
        if self.hops or self.distances:   # after every reference parameter; zeros: torch's generator is not touched
            self.hop_bias = nn.Parameter(torch.zeros(self.num_U2GNN_layers, self.num_self_att_layers,
                                                     (self.hops or self.distances) + 1))
        self._core = None

    def named_parameters(self, prefix='', recurse=True, remove_duplicate=True):
        """torch's, with degree_emb and hop_bias (registered last, but parameters of the model itself) listed last."""
        return hop_bias_last(super().named_parameters(prefix, recurse, remove_duplicate), prefix)

    @property
    def core(self) -> SupCore:
        if self._core is None:
            self._core = SupCore(self, self.precision)
        return self._core

    def flatten_parameters(self) -> FlatParams:
        """Move all parameters into one flat device buffer (for the fused clip+Adam)."""
        return FlatParams(self)

    def forward(self, input_x, graph_pool, X_concat):
        if isinstance(input_x, DeviceBatch):
            batch = input_x
        else:
            batch = DeviceBatch.from_reference_inputs(input_x, graph_pool, X_concat)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.training else 0
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            names, params = zip(*self.named_parameters())
            return _SupFunction.apply(self.core, batch, self.training, seed, names, *params)
        scores, _ = self.core.forward(batch, self.training, need_ctx=False, seed=seed)
        return scores


def label_smoothing(true_labels: torch.Tensor, classes: int, smoothing=0.1):
    """pytorch_U2GNN_Sup.py:48-60: confidence 1-smoothing on the true class,
    smoothing/(classes-1) elsewhere."""
    assert 0 <= smoothing < 1
    true_dist = torch.full((true_labels.size(0), classes), smoothing / (classes - 1), device=true_labels.device)
    true_dist.scatter_(1, true_labels.data.unsqueeze(1), 1.0 - smoothing)
    return true_dist
