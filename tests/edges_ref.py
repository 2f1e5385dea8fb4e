"""Helpers of the attention="edges" tests.  Test infrastructure only.

* CSR <-> dense conversions and small batches built from the datasets of ``dataset/``;
* a float64 restatement of the supervised model with the adjacency mask: the oracle's encoder layer
  (oracle.u2gnn_oracle.encoder_layer, slot 0 only) with -inf outside the adjacency before the softmax and the
  attention dropout mask taken at [i, j]; pool, heads and loss as in the oracle."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def csr_to_dense(rowptr, colidx, N):
    """[N, N] int64 counts: how often row i lists column j."""
    rp, ci = np.asarray(rowptr), np.asarray(colidx)
    rows = np.repeat(np.arange(N), np.diff(rp))
    A = np.zeros((N, N), dtype=np.int64)
    np.add.at(A, (rows, ci), 1)
    return A


def dense_to_csr(A):
    """(rowptr, colidx) of the non-zero entries of a [N, N] 0/1 matrix, columns ascending."""
    A = np.asarray(A) != 0
    rowptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(A.sum(1), out=rowptr[1:])
    return rowptr, np.nonzero(A)[1].astype(np.int64)


def block_csr(offsets):
    """The complete-graph adjacency of every segment offsets[g] .. offsets[g+1]-1 (diagonal blocks of ones)."""
    N = int(offsets[-1])
    A = np.zeros((N, N), dtype=np.int64)
    for g in range(len(offsets) - 1):
        A[offsets[g]:offsets[g + 1], offsets[g]:offsets[g + 1]] = 1
    return dense_to_csr(A)


_STORES = {}


def store_of(dataset, degree_as_tag):
    import util
    from u2gnn_hip.batching import GraphStore
    key = (dataset, degree_as_tag)
    if key not in _STORES:
        graphs, C = util.load_data(dataset, degree_as_tag)
        _STORES[key] = (GraphStore(graphs), C)
    return _STORES[key]


def host_batch(dataset, degree_as_tag, ids, k=4, with_input_y=False):
    """(store, classes, HostBatch, (rowptr, colidx)) of the fixed graphs ``ids``; the sampled slots come from a
    private RandomState, so nothing depends on the global stream."""
    store, C = store_of(dataset, degree_as_tag)
    hb = store.assemble_numpy(ids, k, rng=np.random.RandomState(7), with_input_y=with_input_y)
    return store, C, hb, store.adjacency(ids)


def rewire(A, lo, hi):
    """A copy of the symmetric 0/1 adjacency A (with diagonal) with one double edge swap inside rows lo .. hi-1:
    edges (a, b), (c, d) become (a, d), (c, b); every degree stays.  The first legal swap in index order."""
    A = np.array(A)
    edges = [(a, b) for a in range(lo, hi) for b in range(a + 1, hi) if A[a, b]]
    for a, b in edges:
        for c, d in edges:
            if len({a, b, c, d}) == 4 and not A[a, d] and not A[c, b]:
                for x, y, v in ((a, b, 0), (c, d, 0), (a, d, 1), (c, b, 1)):
                    A[x, y] = A[y, x] = v
                return A
    raise AssertionError("no legal edge swap in this graph")


def encoder_layer_edges(x, prm, allowed, train, p=0.5, masks=None):
    """oracle.u2gnn_oracle.encoder_layer on slot 0 ([N, d]) with attention restricted to ``allowed`` ([N, N] bool)."""
    d = x.shape[1]
    qkv = x @ prm["in_proj_weight"].t() + prm["in_proj_bias"]
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    scores = (q @ k.t()) / math.sqrt(d)
    attn = torch.softmax(scores.masked_fill(~allowed, float("-inf")), dim=-1)
    drop = train and p > 0

    def dr(t, name):
        return t * masks[name].to(t.dtype) / (1 - p) if drop else t
    o = dr(attn, "attn") @ v
    sa = o @ prm["out_proj.weight"].t() + prm["out_proj.bias"]
    x = F.layer_norm(x + dr(sa, "drop1"), (d,), prm["norm1.weight"], prm["norm1.bias"], 1e-5)
    h = dr(torch.relu(x @ prm["linear1.weight"].t() + prm["linear1.bias"]), "drop_ff")
    ff = h @ prm["linear2.weight"].t() + prm["linear2.bias"]
    return F.layer_norm(x + dr(ff, "drop2"), (d,), prm["norm2.weight"], prm["norm2.bias"], 1e-5)


def sup_forward_edges(sd, input_x, offsets, X, allowed, L, T, train, masks=None):
    """oracle.u2gnn_oracle.sup_forward (slot 0) in the dtype of ``sd`` / ``X`` with the adjacency mask."""
    from oracle import u2gnn_oracle as O
    P = O.pool_matrix(offsets).to(X.dtype)
    ix = torch.as_tensor(input_x)[:, 0]
    scores = 0
    x = X[ix]
    for l in range(L):
        for t in range(T):
            x = encoder_layer_edges(x, O.layer_params(sd, l, t), allowed, train, 0.5,
                                    None if masks is None else masks[(l, t)])
        out = x
        x = out[ix]
        ge = P @ out
        if train:
            ge = ge * masks[("head", l)].to(ge.dtype) / 0.5
        scores = scores + ge @ sd[f"predictions.{l}.weight"].t() + sd[f"predictions.{l}.bias"]
    return scores
