"""Helpers of the ``hops`` tests (attention="edges" over the H-hop neighbourhood with a learned bias per shortest-path
distance).  Test infrastructure only.

* brute-force all-pairs shortest-path distances (Floyd-Warshall in numpy) and the H-hop lists cut from them;
* the dense additive mask of a batch: -inf outside the pattern, table[distance] inside;
* a float64 restatement of the supervised model with that mask: tests/edges_ref.py's encoder layer with the bias
  added to the scores before the softmax."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from edges_ref import csr_to_dense  # noqa: F401  (re-exported for the tests)

UNREACHED = 255


def graph_distances(store, gi):
    """[n, n] int64 shortest-path distances inside graph ``gi`` of a GraphStore (UNREACHED where there is no path),
    by Floyd-Warshall over its neighbour lists."""
    n = int(store.n_nodes[gi])
    lo = int(store.node_start[gi])
    D = np.full((n, n), UNREACHED, dtype=np.int64)
    np.fill_diagonal(D, 0)
    for i in range(n):
        s, e = int(store.nbr_start[lo + i]), int(store.nbr_start[lo + i + 1])
        for j in store.nbr[s:e]:
            if j != i:
                D[i, int(j)] = 1
    for k in range(n):
        D = np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :])
    return np.minimum(D, UNREACHED)


def batch_distances(store, ids):
    """[N, N] distances of the batch ``ids`` (block-diagonal; UNREACHED between graphs and between components)."""
    sizes = [int(store.n_nodes[g]) for g in ids]
    N = sum(sizes)
    D = np.full((N, N), UNREACHED, dtype=np.int64)
    o = 0
    for g, n in zip(ids, sizes):
        D[o:o + n, o:o + n] = graph_distances(store, int(g))
        o += n
    return D


def lists_from_distances(D, H):
    """(rowptr, colidx, etype) of the entries with distance <= H, columns ascending."""
    inside = D <= H
    rowptr = np.zeros(D.shape[0] + 1, dtype=np.int64)
    np.cumsum(inside.sum(1), out=rowptr[1:])
    rows, cols = np.nonzero(inside)
    return rowptr, cols.astype(np.int64), D[rows, cols].astype(np.int32)


def dense_bias(rowptr, colidx, etype, N, table, dtype=torch.float64):
    """[N, N] additive mask of one encoder layer: table[etype[e]] at the entries, -inf elsewhere.  ``table`` may
    require grad (the gather is differentiable)."""
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(np.asarray(rowptr))))
    cols = torch.from_numpy(np.asarray(colidx))
    m = torch.full((N, N), float("-inf"), dtype=dtype)
    return m.index_put((rows, cols), table.to(dtype)[torch.from_numpy(np.asarray(etype)).long()])


def encoder_layer_hops(x, prm, mask, train, p=0.5, masks=None):
    """edges_ref.encoder_layer_edges with the additive ``mask`` ([N, N]: -inf outside the pattern, the layer's bias
    inside) on the scores before the softmax."""
    d = x.shape[1]
    qkv = x @ prm["in_proj_weight"].t() + prm["in_proj_bias"]
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    attn = torch.softmax((q @ k.t()) / math.sqrt(d) + mask, dim=-1)
    drop = train and p > 0

    def dr(t, name):
        return t * masks[name].to(t.dtype) / (1 - p) if drop else t
    o = dr(attn, "attn") @ v
    sa = o @ prm["out_proj.weight"].t() + prm["out_proj.bias"]
    x = F.layer_norm(x + dr(sa, "drop1"), (d,), prm["norm1.weight"], prm["norm1.bias"], 1e-5)
    h = dr(torch.relu(x @ prm["linear1.weight"].t() + prm["linear1.bias"]), "drop_ff")
    ff = h @ prm["linear2.weight"].t() + prm["linear2.bias"]
    return F.layer_norm(x + dr(ff, "drop2"), (d,), prm["norm2.weight"], prm["norm2.bias"], 1e-5)


def encode_hops(sd, input_x, X, csr, L, T, train, masks=None):
    """The per-U2GNN-layer slot-0 outputs [out_0, ..., out_{L-1}] in the dtype of ``sd`` / ``X``; csr = (rowptr,
    colidx, etype); the tables are sd["hop_bias"] [L, T, H + 1]."""
    from oracle import u2gnn_oracle as O
    N = X.shape[0]
    ix = torch.as_tensor(input_x)[:, 0]
    x = X[ix]
    outs = []
    for l in range(L):
        for t in range(T):
            x = encoder_layer_hops(x, O.layer_params(sd, l, t), dense_bias(*csr, N, sd["hop_bias"][l, t], X.dtype),
                                   train, 0.5, None if masks is None else masks[(l, t)])
        outs.append(x)
        x = x[ix]
    return outs


def sup_forward_hops(sd, input_x, offsets, X, csr, L, T, train, masks=None):
    """edges_ref.sup_forward_edges with the hop bias: scores [B, C]."""
    from oracle import u2gnn_oracle as O
    P = O.pool_matrix(offsets).to(X.dtype)
    scores = 0
    for l, out in enumerate(encode_hops(sd, input_x, X, csr, L, T, train, masks)):
        ge = P @ out
        if train:
            ge = ge * masks[("head", l)].to(ge.dtype) / 0.5
        scores = scores + ge @ sd[f"predictions.{l}.weight"].t() + sd[f"predictions.{l}.bias"]
    return scores
