"""Helpers of the ``centrality`` tests (a learned vector per node degree added to the stack's input).  Test
infrastructure only.

The restatement is one line, ``x = X + E[min(deg, D)]``, in front of the references the other modes already have:
tests/hops_ref.py's float64 model under an additive mask (every attention mode over node rows is such a mask: all
pairs for "nodes", the diagonal blocks for "graphs", the adjacency for "edges", each with or without a bias table) and
the oracle's ``sup_forward(attention="neighbors")``.  Nothing here is modified by a test."""
import numpy as np
import torch

from edges_ref import block_csr, host_batch  # noqa: F401  (host_batch: re-exported for the tests)
from hops_ref import dense_bias, encode_hops, sup_forward_hops  # noqa: F401


def classes(deg, D):
    """The table row of every node: its degree clipped to [0, D] (int64 numpy)."""
    return np.clip(np.asarray(deg, dtype=np.int64), 0, D)


def add_table(X, E, deg):
    """X + E[min(deg, D)] in the dtype of X and E (torch; differentiable in E); D = E.shape[0] - 1."""
    return X + E[torch.from_numpy(classes(deg, E.shape[0] - 1))]


def pattern_csr(mode, store, ids, hb, hops=None, distances=None):
    """(rowptr, colidx, etype) of the pairs the rows of batch ``ids`` attend over under ``mode``, etype the index into
    the layer's bias table (all zeros for a mode without one: ``tables`` then gives a single zero)."""
    if mode == "edges":
        if hops:
            return store.adjacency(ids, hops=hops)
        rowptr, colidx = store.adjacency(ids)
    elif mode == "graphs":
        rowptr, colidx = block_csr(hb.offsets)
        if distances:
            return rowptr, colidx, store.distances(ids, distances)[1]
    elif mode == "nodes":
        rowptr, colidx = block_csr(np.array([0, hb.N]))
    else:
        raise ValueError(mode)
    return rowptr, colidx, np.zeros(len(colidx), dtype=np.int32)


def with_tables(sd, L, T, dtype):
    """``sd`` with a zero ``hop_bias`` [L, T, 1] when the model has none (what hops_ref's model indexes)."""
    if "hop_bias" in sd:
        return sd
    return dict(sd, hop_bias=torch.zeros(L, T, 1, dtype=dtype))


def sup_forward_centrality(sd, hb, deg, csr, L, T, train=False, masks=None):
    """Scores [B, C] of the supervised model over node rows in the dtype of ``sd``: sd["degree_emb"] added to the
    features by degree class, then hops_ref.sup_forward_hops under the mode's mask ``csr`` (pattern_csr)."""
    E = sd["degree_emb"]
    x = add_table(torch.from_numpy(hb.X_concat).to(E.dtype), E, deg)
    return sup_forward_hops(with_tables(sd, L, T, E.dtype), hb.input_x, hb.offsets, x, csr, L, T, train, masks)


def sup_forward_centrality_neighbors(sd, hb, deg, L, T):
    """The same for attention="neighbors" (eval): the oracle's window model on the pre-added features, so every
    gathered token carries the vector of the node it was gathered from."""
    from oracle import u2gnn_oracle as O
    E = sd["degree_emb"]
    x = add_table(torch.from_numpy(hb.X_concat).to(E.dtype), E, deg)
    return O.sup_forward(sd, torch.from_numpy(hb.input_x), hb.offsets, x, L, T, train=False, attention="neighbors")


def encode_centrality(sd, hb, deg, csr, L, T):
    """The per-U2GNN-layer outputs of the stack (eval) on the pre-added features: hops_ref.encode_hops."""
    E = sd["degree_emb"]
    x = add_table(torch.from_numpy(hb.X_concat).to(E.dtype), E, deg)
    return encode_hops(with_tables(sd, L, T, E.dtype), hb.input_x, x, csr, L, T, False)
