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

MAX_NODES = 46000


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


def _build(node_feats: torch.Tensor, cam_ids, node_labels, l2norm: bool, k=None):
    """The raw library call: (x, edge_pairs [E,2], edge_attr, edge_labels, labels_dev, edge_pos) and what a backward needs
    again.  k=None: `mtmc_build_graph`, the reference's list (edge_pos None).  k given: `mtmc_build_graph_knn`; the edge
    outputs are allocated at min(E_dense, 2 k N) and narrowed to the E_k the device reports -- one host read-back (the host
    builds the camera tables anyway).  `e` in the second tuple is the DENSE list's length either way: the backward's."""
    n, f = node_feats.shape
    dev = node_feats.device
    feats = node_feats if (node_feats.stride(1) == 1 and node_feats.stride(0) % 4 == 0) else node_feats.contiguous()
    in_list, in_off, out_list, out_off, block_off, n_cams = camera_tables(cam_ids)
    e = int(block_off[-1])
    cap = e if k is None else min(e, 2 * min(k, n) * n)
    lib = _lib.load()
    up = lambda a: torch.from_numpy(a).to(dev)
    t_in, t_inoff, t_out, t_outoff, t_blk = up(in_list), up(in_off), up(out_list), up(out_off), up(block_off)
    labels_dev = None
    if node_labels is not None:
        labels_dev = torch.as_tensor(np.asarray(node_labels), dtype=torch.int64).to(dev)
    x = torch.empty((n, f), dtype=torch.float32, device=dev)
    edge_pairs = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    edge_labels = torch.empty((cap,), dtype=torch.float32, device=dev) if labels_dev is not None else None
    need = lib.mtmc_graph_workspace_bytes(n, f) if k is None else lib.mtmc_graph_knn_workspace_bytes(n, f)
    if need == 0:
        raise RuntimeError("mtmc_mpn.build_graph: unsupported size")
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    shared = (feats.data_ptr(), feats.stride(0), n, f, 1 if l2norm else 0,
              t_in.data_ptr(), t_inoff.data_ptr(), t_out.data_ptr() if e else None, t_outoff.data_ptr(), t_blk.data_ptr(),
              n_cams, e, labels_dev.data_ptr() if labels_dev is not None else None,
              x.data_ptr(), edge_pairs.data_ptr() if e else None, edge_attr.data_ptr() if e else None,
              edge_labels.data_ptr() if edge_labels is not None else None)
    edge_pos = None
    if k is None:
        _call.run(dev, lib.mtmc_build_graph, *shared, ws.data_ptr(), ws.numel(), _call.stream(dev))
    else:
        edge_pos = torch.empty((cap,), dtype=torch.int64, device=dev)
        n_kept = torch.zeros((1,), dtype=torch.int64, device=dev)
        _call.run(dev, lib.mtmc_build_graph_knn, *shared, min(k, n), cap, edge_pos.data_ptr() if e else None,
                  n_kept.data_ptr(), ws.data_ptr(), ws.numel(), _call.stream(dev))
        e_k = int(n_kept.item())                              # the one host synchronisation of the k path
        if e_k > cap:
            raise RuntimeError(f"mtmc_mpn.build_graph: {e_k} edges kept, capacity {cap}")
        edge_pairs, edge_attr, edge_pos = edge_pairs[:e_k], edge_attr[:e_k], edge_pos[:e_k]
        edge_labels = edge_labels[:e_k] if edge_labels is not None else None
    return ((x, edge_pairs, edge_attr, edge_labels, labels_dev, edge_pos),
            (feats, (t_in, t_inoff, t_out, t_outoff, t_blk), n_cams, e))


class _BuildGraph(torch.autograd.Function):
    """`build_graph` with its HIP backward to the node features (`mtmc_build_graph_backward`): the reference's fine-tuning
    chain (train.py:304-342) without its two [E, F] gathers -- one [N, N] x [N, F] product on the matrix cores.

    With `k` the gradient flows through the kept edges only (the selection has none).  A dropped edge adds exactly zero to
    every term of the backward (a_e = b_e = 0), so the kept edges' attributes and gradients are scattered through
    `edge_pos` into dense-layout buffers and the same backward runs: 16 bytes x E_dense of extra memory, sized for the
    few-hundred-node graphs that are fine-tuned."""

    @staticmethod
    def forward(ctx, node_feats, cam_ids, node_labels, l2norm, k):
        (x, edge_pairs, edge_attr, edge_labels, labels_dev, edge_pos), (feats, tables, n_cams, e) = \
            _build(node_feats.detach(), cam_ids, node_labels, l2norm, k)
        edge_index = edge_pairs.t()
        ctx.save_for_backward(feats, x, edge_attr, *tables, *([edge_pos] if k is not None else []))
        ctx.meta = (bool(l2norm), n_cams, e)
        ctx.mark_non_differentiable(*[t for t in (edge_index, edge_labels, labels_dev, edge_pos) if t is not None])
        return x, edge_index, edge_attr, edge_labels, labels_dev, edge_pos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, _g_index, g_attr, _g_labels, _g_y, _g_pos):
        feats, x, edge_attr, t_in, t_inoff, t_out, t_outoff, t_blk, *pos = ctx.saved_tensors
        l2norm, n_cams, e = ctx.meta
        n, f = x.shape
        dev = x.device
        if e == 0:
            g_attr = None
        if g_x is None and g_attr is None:
            return torch.zeros((n, f), dtype=torch.float32, device=dev), None, None, None, None
        g_x = g_x.contiguous().float() if g_x is not None else None
        g_attr = g_attr.contiguous().float() if g_attr is not None else None
        if pos and g_attr is not None:
            # dropped edges: zero gradient, and an infinite distance so that the backward's near-duplicate pass (d^2 below
            # 1e-3 (rho_r^2 + rho_c^2), which d = 0 would meet) does not visit them: a_e = 0 / inf = 0 all the same
            dense_attr = torch.zeros((e, 2), dtype=torch.float32, device=dev)
            dense_attr[:, 0] = float("inf")
            dense_attr[pos[0]] = edge_attr
            dense_g = torch.zeros((e, 2), dtype=torch.float32, device=dev)
            dense_g[pos[0]] = g_attr
            edge_attr, g_attr = dense_attr, dense_g
        lib = _lib.load()
        d_feats = torch.empty((n, f), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.mtmc_graph_backward_workspace_bytes(n, f) + 256, dtype=torch.uint8, device=dev)
        _call.run(dev, lib.mtmc_build_graph_backward,
                  feats.data_ptr(), feats.stride(0), n, f, 1 if l2norm else 0,
                  t_in.data_ptr(), t_inoff.data_ptr(), t_out.data_ptr() if e else None, t_outoff.data_ptr(), t_blk.data_ptr(),
                  n_cams, e, x.data_ptr(), edge_attr.data_ptr() if e else None,
                  g_x.data_ptr() if g_x is not None else None, g_attr.data_ptr() if g_attr is not None else None,
                  d_feats.data_ptr(), ws.data_ptr(), ws.numel(), _call.stream(dev))
        return d_feats, None, None, None, None


def build_graph(node_feats: torch.Tensor, cam_ids, node_labels=None, l2norm: bool = True, k=None):
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
    a model on the kind of list it is run on: nothing is claimed about the accuracy of a dense-trained model on a k list."""
    _call.require_gpu("build_graph", node_feats)
    if node_feats.dim() != 2 or node_feats.dtype != torch.float32 or node_feats.shape[1] % 32:
        raise RuntimeError("mtmc_mpn.build_graph: node_feats must be float32 [N, F] with F a multiple of 32")
    n, f = node_feats.shape
    if len(cam_ids) != n:
        raise RuntimeError("mtmc_mpn.build_graph: one camera id per node expected")
    if n > MAX_NODES:
        raise NotImplementedError(f"mtmc_mpn.build_graph: the Gram-matrix builder handles up to {MAX_NODES} nodes")
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise RuntimeError("mtmc_mpn.build_graph: k must be None or an integer >= 1")
        k = int(k)
    if torch.is_grad_enabled() and node_feats.requires_grad:
        x, edge_index, edge_attr, edge_labels, labels_dev, edge_pos = \
            _BuildGraph.apply(node_feats, cam_ids, node_labels, l2norm, k)
    else:
        (x, edge_pairs, edge_attr, edge_labels, labels_dev, edge_pos), _ = _build(node_feats, cam_ids, node_labels, l2norm, k)
        edge_index = edge_pairs.t()
    out = types.SimpleNamespace(x=x, edge_index=edge_index, edge_attr=edge_attr, edge_labels=edge_labels, y=labels_dev)
    if k is not None:
        out.edge_pos = edge_pos
    return out
