"""The k-nearest selection rule of `build_graph(k=...)`, in plain numpy / torch on the CPU -- TEST INFRASTRUCTURE.

Applied to a DENSE cross-camera list (what `build_graph` without `k`, or oracle.graph_oracle.build, returns):
    key(i, j) = the cosine distance edge_attr[e, 1] of the directed edge e = (i, j)
    row i ranks its cross-camera nodes by (key, column index j) ascending; top_i = the first min(k, n_out(i)) of them
    edge (i, j) is kept iff j is in top_i or i is in top_j
"""
import numpy as np
import torch


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def ranks(attr_cos, edge_index):
    """Rank of every dense edge in its row's (key, column) order, 0 = nearest."""
    key, row, col = _np(attr_cos), _np(edge_index[0]), _np(edge_index[1])
    order = np.lexsort((col, key, row))                      # by row, then key, then column
    rs = row[order]
    first = np.searchsorted(rs, rs, side="left")             # where each row starts in the sorted order
    rank = np.empty(row.size, dtype=np.int64)
    rank[order] = np.arange(row.size) - first
    return rank


def reverse_positions(edge_index, n):
    """Position of (j, i) in the list for every edge (i, j); the cross-camera list holds both directions."""
    row, col = _np(edge_index[0]).astype(np.int64), _np(edge_index[1]).astype(np.int64)
    code = row * n + col
    sorter = np.argsort(code)
    rev = sorter[np.searchsorted(code[sorter], col * n + row)]
    assert np.array_equal(code[rev], col * n + row)
    return rev


def select(attr_cos, edge_index, cams, k):
    """Kept dense positions (ascending, int64 tensor) of the symmetric k-nearest list."""
    if _np(edge_index).shape[1] == 0:
        return torch.zeros(0, dtype=torch.int64)
    picked = ranks(attr_cos, edge_index) < k                 # j in top_i
    keep = picked | picked[reverse_positions(edge_index, len(cams))]
    return torch.from_numpy(np.nonzero(keep)[0].astype(np.int64))
