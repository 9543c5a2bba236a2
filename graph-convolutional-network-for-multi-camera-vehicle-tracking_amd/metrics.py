"""How good a tracking result is, computed on the GPU: what the reference's inference / validation loop does with
`input_test == 'gt'` (inference.py:501-526) after `post_processing`.

  cluster_scores   adjusted Rand, adjusted mutual information, homogeneity, completeness and V-measure of two label
      vectors (the five scikit-learn calls at inference.py:509, :516-519), with the entropies, MI, EMI and the integer
      counts they are made of
  edge_prf         TP / FP / TN / FN, P, R, F and the two per-class figures of `compute_P_R_F` (inference.py:23-68) on the
      int64 predictions that `postprocess` returns
  evaluate         both, with ID_GT = the connected components of the label-1 edges (utils.py:30-52) from `postprocess`

All of them run HIP kernels through the C ABI, read nothing back to the host and leave their results on the device; CPU
tensors are refused.  Neither scikit-learn nor networkx is needed.
"""
from __future__ import annotations

import collections
import types

import torch

from . import _call, _lib
from .postprocess import postprocess

ClusterScores = collections.namedtuple("ClusterScores", ["ari", "ami", "homogeneity", "completeness", "v_measure",
                                                         "entropy_true", "entropy_pred", "mi", "emi", "counts"])
EdgePRF = collections.namedtuple("EdgePRF", ["confusion", "precision", "recall", "f_score", "class_precision"])

MAX_LABELS = _lib.CLUSTER_SCORES_MAX_N
_INT_TYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def cluster_scores(labels_true, labels_pred):
    """labels_true, labels_pred: [n] integer tensors on one ROCm device, any stride, any values (not compact, negative,
    INT64_MIN / INT64_MAX); they are read as int64 and not modified.  1 <= n <= 1 048 576.

    Returns the named tuple ClusterScores(ari, ami, homogeneity, completeness, v_measure, entropy_true, entropy_pred, mi,
    emi, counts): the scores are 0-d float64 device tensors (views of one buffer) with scikit-learn's definitions and
    special cases in natural logarithms, `counts` is int64 [7] = clusters of either side, non-empty contingency cells, and
    the pair confusion tp, fp, fn, tn behind the adjusted Rand index.  Nothing is read on the host."""
    t, p = labels_true, labels_pred
    if t.dim() != 1 or p.dim() != 1 or t.dtype not in _INT_TYPES or p.dtype not in _INT_TYPES:
        raise ValueError("mtmc_mpn.cluster_scores: labels must be [n] integer tensors")
    if t.shape != p.shape:
        raise ValueError(f"mtmc_mpn.cluster_scores: {t.shape[0]} true labels against {p.shape[0]} predicted ones")
    n = t.shape[0]
    if n < 1 or n > MAX_LABELS:
        raise ValueError(f"mtmc_mpn.cluster_scores: n = {n} is outside [1, {MAX_LABELS}]")
    _call.require_gpu("cluster_scores", t, p)
    dev = t.device
    t, p = t.long(), p.long()                                   # (no copy of an int64 tensor; its stride goes to the kernel)
    lib = _lib.load()
    need = lib.mtmc_cluster_scores_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    scores = torch.empty(_lib.CLUSTER_SCORES, dtype=torch.float64, device=dev)
    counts = torch.empty(_lib.CLUSTER_COUNTS, dtype=torch.int64, device=dev)
    _call.run(dev, lib.mtmc_cluster_scores, t.data_ptr(), t.stride(0), p.data_ptr(), p.stride(0), n, scores.data_ptr(),
              counts.data_ptr(), ws.data_ptr(), need, _call.stream(dev))
    return ClusterScores(*scores.unbind(0), counts)


def edge_prf(predictions, labels):
    """`compute_P_R_F` (reference inference.py:23-68) in one pass: predictions [E] integer (what `postprocess` returns),
    labels [E] int64 or the float 0/1 tensor the reference keeps, any stride.  Rows whose label (or prediction) is neither
    0 nor 1 count for nothing.  Returns the named tuple EdgePRF(confusion int64 [4] = TP FP TN FN, precision, recall,
    f_score (0-d float64, 0 on a zero denominator), class_precision float64 [2] = the reference's precision_class0,
    precision_class1: the share of the label-0 / label-1 edges predicted right, in percent).  E = 0 gives zeros."""
    y, x = predictions, labels
    if y.dim() != 1 or x.shape != y.shape or y.dtype not in _INT_TYPES:
        raise ValueError("mtmc_mpn.edge_prf: predictions must be an [E] integer tensor, labels [E]")
    _call.require_gpu("edge_prf", y, x)
    dev = y.device
    y, x = y.long(), x.long()
    e = y.shape[0]
    confusion = torch.empty(4, dtype=torch.int64, device=dev)
    out = torch.empty(_lib.EDGE_PRF, dtype=torch.float64, device=dev)
    _call.run(dev, _lib.load().mtmc_edge_prf, y.data_ptr() if e else None, y.stride(0) if e else 1,
              x.data_ptr() if e else None, x.stride(0) if e else 1, e, confusion.data_ptr(), out.data_ptr(), _call.stream(dev))
    return EdgePRF(confusion, out[0], out[1], out[2], out[3:5])


def evaluate(ID_pred, predictions, edge_index, edge_labels, num_nodes: int):
    """The `input_test == 'gt'` branch of reference inference.py:501-526 in one call, without a host read: ID_GT = the
    connected components of the label-1 edges (what `compute_SCC_and_Clusters` makes of `G_GT`; the scores do not depend
    on how the clusters are numbered), then `cluster_scores(ID_GT, ID_pred)` and `edge_prf(predictions, edge_labels)`.
    Returns a namespace with ID_GT [N] int64, clusters (ClusterScores) and edges (EdgePRF)."""
    _call.require_gpu("evaluate", edge_labels, ID_pred, predictions, edge_index)
    gt = postprocess(None, edge_index, num_nodes, 1, cutting=False, pruning=False, splitting=False,
                     preds_prob=edge_labels, predictions=edge_labels, check=False)
    return types.SimpleNamespace(ID_GT=gt.ID_pred, clusters=cluster_scores(gt.ID_pred, ID_pred),
                                 edges=edge_prf(predictions, edge_labels))
