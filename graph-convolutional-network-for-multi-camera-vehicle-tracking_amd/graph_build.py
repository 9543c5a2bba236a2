"""`build_graph`: the callers' graph construction on the GPU (SURVEY.md 8(f)-1,2).

Replaces what reference inference.py:402-458 (and train.py:316-342) do around the MPN call -- stack + column
normalisation of the 2048-d tracklet features, the cross-camera cartesian edge list, the O(E*N) Python edge-label
loop, and the two 2048-d gathers per edge for `edge_attr` -- by one library call (`mtmc_build_graph`): a Gram matrix
on the matrix cores plus an 8-byte-per-edge epilogue.  Returns a `Data`-like namespace whose attributes feed
`MOTMPNet.forward` directly.
"""
from __future__ import annotations

import types

import numpy as np
import torch

from . import _call, _lib

MAX_NODES = 46000               # where the Gram matrix is formed whole: N^2 x 4 bytes
MAX_NODES_PANELED = 262144      # where it is formed in row panels (`mtmc_build_graph_paneled`)
MAX_K_PANELED = 4096


def camera_tables(cam_ids):
    """Small host-side index tables of the camera structure (O(N * cameras) ints)."""
    cams = np.asarray(cam_ids)
    n = cams.shape[0]
    nodes = np.arange(n, dtype=np.int32)
    uniq = np.unique(cams)
    in_list, out_list, in_off, out_off, block_off = [], [], [0], [0], [0]
    for c in uniq:
        inside, outside = nodes[cams == c], nodes[cams != c]
        in_list.append(inside)
        out_list.append(outside)
        in_off.append(in_off[-1] + inside.size)
        out_off.append(out_off[-1] + outside.size)
        block_off.append(block_off[-1] + inside.size * outside.size)
    return (np.concatenate(in_list).astype(np.int32), np.asarray(in_off, dtype=np.int32),
            np.concatenate(out_list).astype(np.int32) if out_list else np.zeros(0, np.int32),
            np.asarray(out_off, dtype=np.int64), np.asarray(block_off, dtype=np.int64), len(uniq))


FRAME_LIMIT = 1 << 62           # |start frame| at the most, so that no difference of two leaves int64
_GAP_LIMIT = (1 << 63) - 1


def _start_frames(start_frames, n):
    """N start frames as an int64 numpy array; RuntimeError for anything but N host integers within +-FRAME_LIMIT."""
    if isinstance(start_frames, torch.Tensor):
        if start_frames.is_cuda:
            raise RuntimeError("mtmc_mpn.build_graph: start_frames live on the host, like cam_ids")
        start_frames = start_frames.numpy()
    s = np.asarray(start_frames)
    if s.dtype.kind not in "iu" or s.ndim != 1:
        raise RuntimeError("mtmc_mpn.build_graph: start_frames must be a one-dimensional list / array / CPU tensor of integers")
    if s.shape[0] != n:
        raise RuntimeError("mtmc_mpn.build_graph: one start frame per node expected")
    if s.size and (int(s.max()) > FRAME_LIMIT or int(s.min()) < -FRAME_LIMIT):
        raise RuntimeError("mtmc_mpn.build_graph: start_frames must lie within +-2^62")
    return np.ascontiguousarray(s, dtype=np.int64)


def _max_gap(max_gap):
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 1 <= max_gap <= _GAP_LIMIT:
        raise RuntimeError("mtmc_mpn.build_graph: max_gap must be an integer >= 1")
    return int(max_gap)


def _pairs_inside(u, gap):
    """Unordered pairs {a, b} of entries of `u` (uint64) with |u_a - u_b| < gap: in sorted order, for every entry the later
    ones below it + gap.  The queries ascend with the array they search, and u + gap < 2^64."""
    u = np.sort(u)
    below = np.searchsorted(u, u + gap, side="left")          # > own index: gap >= 1
    return int(below.sum()) - u.size * (u.size + 1) // 2


def _gated_count(cams, starts, gap):
    u = starts.astype(np.uint64) + np.uint64(FRAME_LIMIT)     # order-preserving image in [0, 2^63] (the sum wraps back)
    gap = np.uint64(gap)
    pairs = _pairs_inside(u, gap)                             # all pairs inside the window ...
    for c in np.unique(cams):
        pairs -= _pairs_inside(u[cams == c], gap)             # ... less those of one camera
    return 2 * pairs                                          # both directions


def gated_edge_count(cam_ids, start_frames, max_gap) -> int:
    """The exact length of the list `build_graph(..., start_frames=, max_gap=)` returns without `k`: the directed pairs
    (i, j) in different cameras with |start_i - start_j| < max_gap.  Host only, O(N log N) per camera: sorted starts and
    `searchsorted` -- the pairs inside the window among all nodes, less those inside it within each camera."""
    cams = np.asarray(cam_ids)
    return _gated_count(cams, _start_frames(start_frames, cams.shape[0]), _max_gap(max_gap))


def _head(feats, l2norm, tables, n_cams, e):
    """The 12 arguments every entry of the family starts with (feats ... n_edges).  A call without edges (e == 0) passes
    no out_list: one camera has none, and the library asks for the tables only where n_edges > 0."""
    t_in, t_inoff, t_out, t_outoff, t_blk = tables
    return (feats.data_ptr(), feats.stride(0), feats.shape[0], feats.shape[1], 1 if l2norm else 0,
            t_in.data_ptr(), t_inoff.data_ptr(), t_out.data_ptr() if e else None, t_outoff.data_ptr(), t_blk.data_ptr(),
            n_cams, e)


def _build(node_feats: torch.Tensor, cam_ids, node_labels, l2norm: bool, k=None, starts=None, max_gap=None, panel_rows=None):
    """The raw library call; returns a namespace of `outputs` (x, edge_index, edge_attr, edge_labels, labels_dev, edge_pos)
    and what a backward needs again: `feats` as the library read them, the five camera `tables` on the device, `n_cams` and
    `e_dense`, the DENSE list's length in every form.  k=None: `mtmc_build_graph`, the reference's list (edge_pos None).
    k given: `mtmc_build_graph_knn`; the edge outputs are allocated at min(E_dense, 2 k N) and narrowed to the E_k the device
    reports -- one host read-back (the host builds the camera tables anyway).  starts (int64 array) / max_gap given:
    `mtmc_build_graph_gated`; the host counts the gated list (`_gated_count`), so without k the outputs are allocated at
    exactly E_g and nothing is read back, and with k at min(E_g, 2 k N) before the same read-back.  panel_rows given (0: the
    library chooses): `mtmc_build_graph_paneled` in place of either thinned entry -- same outputs, same allocation."""
    n, f = node_feats.shape
    dev = node_feats.device
    feats = node_feats if (node_feats.stride(1) == 1 and node_feats.stride(0) % 4 == 0) else node_feats.contiguous()
    in_list, in_off, out_list, out_off, block_off, n_cams = camera_tables(cam_ids)
    e = int(block_off[-1])
    thinned = k is not None or starts is not None
    cap = e if starts is None else _gated_count(np.asarray(cam_ids), starts, max_gap)
    if k is not None:
        cap = min(cap, 2 * min(k, n) * n)
    e_call = e if cap else 0                                  # an empty gate: x alone, as with one camera
    lib = _lib.load()
    up = lambda a: torch.from_numpy(a).to(dev)
    tables = (up(in_list), up(in_off), up(out_list), up(out_off), up(block_off))
    labels_dev = None
    if node_labels is not None:
        labels_dev = torch.as_tensor(np.asarray(node_labels), dtype=torch.int64).to(dev)
    x = torch.empty((n, f), dtype=torch.float32, device=dev)
    edge_pairs = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    edge_labels = torch.empty((cap,), dtype=torch.float32, device=dev) if labels_dev is not None else None
    kk = min(k, n) if k is not None else 0
    if panel_rows is not None:
        need = lib.mtmc_graph_paneled_workspace_bytes(n, f, kk, panel_rows)
    else:
        need = lib.mtmc_graph_knn_workspace_bytes(n, f) if thinned else lib.mtmc_graph_workspace_bytes(n, f)
    if need == 0:
        raise RuntimeError("mtmc_mpn.build_graph: unsupported size")
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    shared = (*_head(feats, l2norm, tables, n_cams, e_call), labels_dev.data_ptr() if labels_dev is not None else None,
              x.data_ptr(), edge_pairs.data_ptr() if e_call else None, edge_attr.data_ptr() if e_call else None,
              edge_labels.data_ptr() if edge_labels is not None else None)
    edge_pos = None
    if not thinned:
        _call.run(dev, lib.mtmc_build_graph, *shared, ws.data_ptr(), ws.numel(), _call.stream(dev))
    else:
        edge_pos = torch.empty((cap,), dtype=torch.int64, device=dev)
        n_kept = torch.zeros((1,), dtype=torch.int64, device=dev)
        tail = (cap, edge_pos.data_ptr() if e_call else None, n_kept.data_ptr(), ws.data_ptr(), ws.numel(), _call.stream(dev))
        t_start = up(starts) if starts is not None else None
        gate = (t_start.data_ptr() if starts is not None else None, max_gap or 0, kk)
        if panel_rows is not None:
            _call.run(dev, lib.mtmc_build_graph_paneled, *shared, *gate, panel_rows, *tail)
        elif starts is None:
            _call.run(dev, lib.mtmc_build_graph_knn, *shared, kk, *tail)
        else:
            _call.run(dev, lib.mtmc_build_graph_gated, *shared, *gate, *tail)
    if k is not None:
        e_k = int(n_kept.item())                              # the one host synchronisation of the k path
        if e_k > cap:
            raise RuntimeError(f"mtmc_mpn.build_graph: {e_k} edges kept, capacity {cap}")
        edge_pairs, edge_attr, edge_pos = edge_pairs[:e_k], edge_attr[:e_k], edge_pos[:e_k]
        edge_labels = edge_labels[:e_k] if edge_labels is not None else None
    return types.SimpleNamespace(outputs=(x, edge_pairs.t(), edge_attr, edge_labels, labels_dev, edge_pos), feats=feats,
                                 tables=tables, n_cams=n_cams, e_dense=e)


def _dense_scatter(edge_attr, g_attr, edge_pos, e):
    """The kept edges' attributes and gradients at their positions in dense-layout [e, 2] buffers.  Dropped edges: zero
    gradient, and an infinite distance so that the backward's near-duplicate pass (d^2 below 1e-3 (rho_r^2 + rho_c^2),
    which d = 0 would meet) does not visit them: a_e = 0 / inf = 0 all the same."""
    dense_attr = torch.zeros((e, 2), dtype=torch.float32, device=edge_attr.device)
    dense_attr[:, 0] = float("inf")
    dense_attr[edge_pos] = edge_attr
    dense_g = torch.zeros((e, 2), dtype=torch.float32, device=edge_attr.device)
    dense_g[edge_pos] = g_attr
    return dense_attr, dense_g


class _BuildGraph(torch.autograd.Function):
    """`build_graph` with its HIP backward to the node features (`mtmc_build_graph_backward`): the reference's fine-tuning
    chain (train.py:304-342) without its two [E, F] gathers -- one [N, N] x [N, F] product on the matrix cores.

    With `k` or a temporal gate the gradient flows through the kept edges only (neither selection has one).  A dropped
    edge adds exactly zero to every term of the backward (a_e = b_e = 0), so the kept edges' attributes and gradients are
    scattered through `edge_pos` into dense-layout buffers and the same backward runs: 16 bytes x E_dense of extra memory,
    sized for the few-hundred-node graphs that are fine-tuned."""

    @staticmethod
    def forward(ctx, node_feats, cam_ids, node_labels, l2norm, k, starts, max_gap, panel_rows):
        b = _build(node_feats.detach(), cam_ids, node_labels, l2norm, k, starts, max_gap, panel_rows)
        x, edge_index, edge_attr, edge_labels, labels_dev, edge_pos = b.outputs
        ctx.save_for_backward(b.feats, x, edge_attr, *b.tables, *([edge_pos] if edge_pos is not None else []))
        ctx.meta = (bool(l2norm), b.n_cams, b.e_dense)
        ctx.mark_non_differentiable(*[t for t in (edge_index, edge_labels, labels_dev, edge_pos) if t is not None])
        return b.outputs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, _g_index, g_attr, _g_labels, _g_y, _g_pos):
        feats, x, edge_attr, *tables = ctx.saved_tensors
        pos = tables.pop() if len(tables) > 5 else None
        l2norm, n_cams, e = ctx.meta
        n, f = x.shape
        dev = x.device
        if edge_attr.shape[0] == 0:                               # no edges, or none kept: the gradient of x alone
            e, g_attr = 0, None
        if g_x is None and g_attr is None:
            return torch.zeros((n, f), dtype=torch.float32, device=dev), None, None, None, None, None, None, None
        g_x = g_x.contiguous().float() if g_x is not None else None
        g_attr = g_attr.contiguous().float() if g_attr is not None else None
        if pos is not None and g_attr is not None:
            edge_attr, g_attr = _dense_scatter(edge_attr, g_attr, pos, e)
        lib = _lib.load()
        d_feats = torch.empty((n, f), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.mtmc_graph_backward_workspace_bytes(n, f) + 256, dtype=torch.uint8, device=dev)
        _call.run(dev, lib.mtmc_build_graph_backward, *_head(feats, l2norm, tables, n_cams, e),
                  x.data_ptr(), edge_attr.data_ptr() if e else None,
                  g_x.data_ptr() if g_x is not None else None, g_attr.data_ptr() if g_attr is not None else None,
                  d_feats.data_ptr(), ws.data_ptr(), ws.numel(), _call.stream(dev))
        return d_feats, None, None, None, None, None, None, None


def build_graph(node_feats: torch.Tensor, cam_ids, node_labels=None, l2norm: bool = True, k=None, start_frames=None,
                max_gap=None, panel_rows=None):
    """node_feats: [N, F] float32 on a ROCm GPU (the stacked per-tracklet ReID features); cam_ids: N camera ids
    (host list / array, as the reference keeps them); node_labels: optional N identities (edge labels for training).
    With grad mode on and `node_feats.requires_grad`, `x` and `edge_attr` carry the gradient back to `node_feats`.

    k=None: the reference's all-pairs cross-camera list (inference.py:407-413), E ~ N^2.
    k = int >= 1: that list thinned to a symmetric k-nearest list (`mtmc_build_graph_knn`), never forming the dense edge
    arrays.  Row i ranks its cross-camera nodes by (cosine distance edge_attr[e, 1], column index) ascending; top_i is the
    first min(k, n_out(i)) of them; edge (i, j) is kept iff j is in top_i or i is in top_j.  The kept edges are a
    subsequence of the dense list, with the dense call's `edge_attr` / `edge_labels` bits, E_k <= min(E_dense, 2 k N), and
    the extra field `edge_pos` (int64 [E_k]) holds each one's index in the dense list.  Costs one host read-back of E_k;
    the backward costs 16 bytes x E_dense (see `_BuildGraph`).  The encoders normalise over the edges of a call, so train
    a model on the kind of list it is run on: nothing is claimed about the accuracy of a dense-trained model on a k list.

    start_frames = N integers on the host (list, integer array or integer CPU tensor: each tracklet's first frame, within
    +-2^62) with max_gap = int >= 1: the temporal gate the reference leaves commented out (inference.py:420-441), through
    `mtmc_build_graph_gated`.  (i, j) is a candidate iff the cameras differ and |start_i - start_j| < max_gap -- strict:
    equal starts pass, a difference of max_gap does not.  Without `k` the kept edges are exactly the candidates, again a
    subsequence of the dense list with its bits and with `edge_pos`; the host counts them beforehand (`gated_edge_count`),
    so the outputs are allocated at exactly that length and nothing is read back.  With `k` every row ranks its candidates
    only, top_i is the first min(k, candidates of i) of them, and the union rule above applies: "gate, then k", which is
    not the k list filtered afterwards; outputs are allocated at min(E_gated, 2 k N) and E is read back once.  A node
    without candidates is isolated, and no candidates at all gives E = 0, as one camera does.  Both arguments or neither.
    The backward is the k path's: it scatters through `edge_pos` into dense-layout buffers, 16 bytes x E_dense.  And the
    same warning holds: the encoders normalise over the edges of a call, so train a model on the kind of list -- gated,
    k-nearest, both or neither -- it is run on.

    panel_rows = int >= 1, with `k` or a gate: the same list through `mtmc_build_graph_paneled`, which forms the Gram matrix
    in panels of that many node rows (clipped to N), twice, and keeps the picks as per-row lists: every output has the bits
    of the call without `panel_rows`, the workspace is panel_rows x N x 4 bytes plus 8 N min(k, N) instead of N^2 x 4.125, and
    min(k, N) <= 4096.  panel_rows=None takes that entry by itself, with a panel of its own choosing
    (`mtmc_graph_panel_rows`), above 46 000 nodes, where no other applies, up to 262 144 nodes; the all-pairs list stays at
    46 000.  The backward needs dense [E_dense, 2] buffers and an N x N matrix: above 46 000 nodes features that require a
    gradient are refused."""
    _call.require_gpu("build_graph", node_feats)
    if node_feats.dim() != 2 or node_feats.dtype != torch.float32 or node_feats.shape[1] % 32:
        raise RuntimeError("mtmc_mpn.build_graph: node_feats must be float32 [N, F] with F a multiple of 32")
    n, f = node_feats.shape
    if len(cam_ids) != n:
        raise RuntimeError("mtmc_mpn.build_graph: one camera id per node expected")
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise RuntimeError("mtmc_mpn.build_graph: k must be None or an integer >= 1")
        k = int(k)
    starts = None
    if start_frames is not None or max_gap is not None:
        if start_frames is None or max_gap is None:
            raise RuntimeError("mtmc_mpn.build_graph: start_frames and max_gap go together")
        starts, max_gap = _start_frames(start_frames, n), _max_gap(max_gap)
    thinned = k is not None or starts is not None
    if panel_rows is not None:
        if isinstance(panel_rows, bool) or not isinstance(panel_rows, (int, np.integer)) or panel_rows < 1:
            raise RuntimeError("mtmc_mpn.build_graph: panel_rows must be None or an integer >= 1")
        if not thinned:
            raise RuntimeError("mtmc_mpn.build_graph: panel_rows needs k or a temporal gate (the all-pairs list is N^2-sized anyway)")
        panel_rows = int(panel_rows)
    elif n > MAX_NODES and thinned:
        panel_rows = 0                                            # the library chooses
    grad = torch.is_grad_enabled() and node_feats.requires_grad
    if n > MAX_NODES_PANELED or (n > MAX_NODES and panel_rows is None):
        raise NotImplementedError(f"mtmc_mpn.build_graph: up to {MAX_NODES} nodes, and up to {MAX_NODES_PANELED} with k or a gate")
    if n > MAX_NODES and grad:
        raise NotImplementedError(f"mtmc_mpn.build_graph: the backward handles up to {MAX_NODES} nodes")
    if panel_rows is not None and k is not None and min(k, n) > MAX_K_PANELED:
        raise RuntimeError(f"mtmc_mpn.build_graph: min(k, N) must be <= {MAX_K_PANELED} with panel_rows or above {MAX_NODES} nodes")
    args = (node_feats, cam_ids, node_labels, l2norm, k, starts, max_gap, panel_rows)
    x, edge_index, edge_attr, edge_labels, labels_dev, edge_pos = _BuildGraph.apply(*args) if grad else _build(*args).outputs
    out = types.SimpleNamespace(x=x, edge_index=edge_index, edge_attr=edge_attr, edge_labels=edge_labels, y=labels_dev)
    if edge_pos is not None:
        out.edge_pos = edge_pos
    return out
