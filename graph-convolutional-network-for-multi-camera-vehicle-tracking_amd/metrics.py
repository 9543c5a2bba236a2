"""How good a tracking result is, computed on the GPU: what the reference's inference / validation loop does with
`input_test == 'gt'` (inference.py:501-526) after `post_processing`.

  cluster_scores   adjusted Rand, adjusted mutual information, homogeneity, completeness and V-measure of two label
      vectors (the five scikit-learn calls at inference.py:509, :516-519), with the entropies, MI, EMI and the integer
      counts they are made of
  edge_prf         TP / FP / TN / FN, P, R, F and the two per-class figures of `compute_P_R_F` (inference.py:23-68) on the
      int64 predictions that `postprocess` returns
  evaluate         both, with ID_GT = the connected components of the label-1 edges (utils.py:30-52) from `postprocess`

  relabel_detections, idf1   what main.py:166-213 does with the clusters: the detections written back with the cluster
      number as identity (inference.py:538-551), then IDF1 / IDP / IDR / IDTP / IDFP / IDFN of eval/eval.py::eval

  mot_scores, tracking_summary   the CLEAR MOT columns of the same result row (eval/eval.py:409-411): MOTA, MOTP, recall,
      precision, switches, fragmentations, mostly tracked / lost, ...; `tracking_summary` returns both score sets

All of them run HIP kernels through the C ABI; CPU tensors are refused.  The first three read nothing back to the host
and leave their results on the device; `idf1` reads the non-zero overlap counts and solves the ID assignment on the host
(in the library, not in Python); `mot_scores` reads the candidate pairs and walks the frames on the host (in the library
too).  Neither scikit-learn, networkx, motmetrics nor pandas is needed.
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
IdScores = collections.namedtuple("IdScores", "idf1 idp idr idtp idfp idfn num_objects num_predictions matches kept")

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


# ---- IDF1 / IDP / IDR: the score the reference reports (main.py:166-213, eval/eval.py::eval) ----------
_TABLE_TYPES = (torch.int32, torch.int64, torch.float32, torch.float64)


def relabel_detections(table, index, ID_pred):
    """The reference's last step (inference.py:538-551): a copy of the [n, 7] detection table (camera, id, frame, x, y,
    width, height) whose id column is ID_pred[index], `index` [n] naming the node (tracklet) of each detection.  Plain
    torch, so it works on CPU tensors as on the device."""
    if table.dim() != 2 or table.shape[1] < 2 or index.dim() != 1 or index.shape[0] != table.shape[0]:
        raise ValueError("mtmc_mpn.relabel_detections: table must be [n, >= 2] and index [n]")
    out = table.clone()
    out[:, 1] = ID_pred[index.long()].to(table.dtype)
    return out


def _id_table(name, t, entry="idf1"):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 7 or t.dtype not in _TABLE_TYPES:
        raise ValueError(f"mtmc_mpn.{entry}: {name} must be an [n, 7] int32, int64, float32 or float64 tensor "
                         "(camera, id, frame, x, y, width, height)")
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"mtmc_mpn.{entry}: {name} has 2^31 rows or more")
    return t[:, :3].to(torch.int64), t[:, 3:7].to(torch.float64)


def _id_side(group_inv, ident_inv, cam_inv, boxes, n_ident, n_groups):
    """One table in grouped order: a stable sort by (group, identity), so repeats stay in input order."""
    dev = boxes.device
    _, perm = torch.sort(group_inv * max(n_ident, 1) + ident_inv, stable=True)
    group = group_inv[perm]
    return types.SimpleNamespace(
        perm=perm, n=boxes.shape[0], n_ident=n_ident, boxes=boxes[perm].contiguous(), group=group.to(torch.int32),
        cam=cam_inv[perm].to(torch.int32), ident=ident_inv[perm].to(torch.int32), keep=None,
        offsets=torch.searchsorted(group, torch.arange(n_groups + 1, dtype=torch.int64, device=dev)))


def _id_filter(side, n_cam, counter, band, roi, planes, min_cameras, drop_repeats):
    dev = side.boxes.device
    stage = torch.empty(side.n, dtype=torch.uint8, device=dev)
    side.keep = torch.empty(side.n, dtype=torch.uint8, device=dev)
    cameras = torch.empty(side.n_ident, dtype=torch.int64, device=dev)
    ptr = (lambda t: t.data_ptr()) if side.n else (lambda t: None)
    _call.run(dev, _lib.load().mtmc_id_filter, ptr(side.boxes), ptr(side.cam), ptr(side.ident), ptr(side.group), side.n,
              side.n_ident, n_cam, int(band is not None), *(band or (0.0, 0.0, 0.0, 0.0)),
              roi.data_ptr() if roi is not None else None, planes.data_ptr() if roi is not None else None,
              *((roi.shape[0], roi.shape[1], roi.shape[2]) if roi is not None else (0, 0, 0)), int(min_cameras),
              int(bool(drop_repeats)), ptr(stage), ptr(side.keep), ptr(cameras), counter.data_ptr(), _call.stream(dev))


def _id_passes(gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size, entry="idf1",
               overlap=True):
    """Grouping in torch on the device, then the filter and (overlap=True) overlap passes.  Returns a namespace: the two
    grouped sides, the identity values, the workspace whose first n_obj * n_hyp int32 words are C, and counters (int64 [3]
    on the device: ground-truth rows kept, prediction rows kept, non-zero cells -- the last written by `mtmc_id_cells`).
    `entry` is the public function the error texts name."""
    gkeys, gbox = _id_table("gt", gt, entry)
    pkeys, pbox = _id_table("pred", pred, entry)
    _call.require_gpu(entry, gt, pred)
    dev = gt.device
    n_gt, n_pr = gt.shape[0], pred.shape[0]
    cams, cam_inv = torch.unique(torch.cat([gkeys[:, 0], pkeys[:, 0]]), return_inverse=True)
    n_cam = cams.numel()
    if n_cam > _lib.ID_MAX_CAMERAS:
        raise ValueError(f"mtmc_mpn.{entry}: {n_cam} cameras, at most {_lib.ID_MAX_CAMERAS}")
    frames, frame_inv = torch.unique(torch.cat([gkeys[:, 2], pkeys[:, 2]]), return_inverse=True)
    groups, group_inv = torch.unique(cam_inv * max(frames.numel(), 1) + frame_inv, return_inverse=True)
    obj_ids, obj_inv = torch.unique(gkeys[:, 1], return_inverse=True)
    hyp_ids, hyp_inv = torch.unique(pkeys[:, 1], return_inverse=True)
    n_groups, n_obj, n_hyp = groups.numel(), obj_ids.numel(), hyp_ids.numel()
    lib = _lib.load()
    need = lib.mtmc_id_overlap_workspace_bytes(n_obj, n_hyp, n_groups) if overlap else 1     # (1: no table, no cell limit)
    if need == 0:
        raise ValueError(f"mtmc_mpn.{entry}: {n_obj} ground-truth x {n_hyp} predicted identities are more than "
                         f"{_lib.ID_MAX_CELLS} cells (or 2^31 groups)")
    band = planes = None
    if border is not None:
        if image_size is None:
            raise ValueError(f"mtmc_mpn.{entry}: border needs image_size=(W, H)")
        w, h, p = image_size[0], image_size[1], float(border)
        band = (float(w * p), float(w - w * p), float(h * p), float(h - h * p))
    if roi is not None:
        if roi.dim() != 3 or roi.dtype != torch.uint8 or roi_cameras is None or len(roi_cameras) != roi.shape[0]:
            raise ValueError(f"mtmc_mpn.{entry}: roi must be a [C, Hr, Wr] uint8 mask stack with roi_cameras = its C camera values")
        _call.require_gpu(entry, gt, roi)
        roi = roi.contiguous()
        hit = cams[:, None] == torch.as_tensor(roi_cameras, dtype=torch.int64, device=dev)[None, :]
        planes = torch.where(hit.any(1), hit.int().argmax(1), -1).to(torch.int32)
        if n_pr and bool((planes[cam_inv[n_gt:]] < 0).any()):
            raise ValueError(f"mtmc_mpn.{entry}: a prediction's camera has no plane in roi (roi_cameras)")
    g = _id_side(group_inv[:n_gt], obj_inv, cam_inv[:n_gt], gbox, n_obj, n_groups)
    q = _id_side(group_inv[n_gt:], hyp_inv, cam_inv[n_gt:], pbox, n_hyp, n_groups)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    if band is not None:
        _id_filter(g, n_cam, counters[0:1], band, None, None, 0, False)
    else:
        counters[0] = n_gt
    _id_filter(q, n_cam, counters[1:2], band, roi, planes, min_cameras, drop_repeats)
    r = types.SimpleNamespace(gt=g, pred=q, obj_ids=obj_ids, hyp_ids=hyp_ids, n_obj=n_obj, n_hyp=n_hyp, n_groups=n_groups,
                              n_cam=n_cam, ws=torch.empty(need, dtype=torch.uint8, device=dev), counters=counters, dev=dev)
    if overlap:
        _id_overlap(r, max_dist)
    return r


def _id_overlap(r, max_dist):
    g, q = r.gt, r.pred
    ptr = (lambda t: t.data_ptr()) if g.n > 0 and q.n > 0 else (lambda t: None)
    _call.run(r.dev, _lib.load().mtmc_id_overlap, ptr(g.boxes), ptr(g.offsets), ptr(g.ident),
              ptr(g.keep) if g.keep is not None else None, g.n, ptr(q.boxes), ptr(q.offsets), ptr(q.ident), ptr(q.keep), q.n,
              r.n_groups, r.n_obj, r.n_hyp, float(max_dist), r.ws.data_ptr(), r.ws.numel(), _call.stream(r.dev))


def _input_order(side):
    kept = torch.empty(side.n, dtype=torch.bool, device=side.boxes.device)
    kept[side.perm] = side.keep.bool() if side.keep is not None else True
    return kept


def id_overlap_counts(gt, pred, max_dist=0.75, *, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None,
                      border=None, image_size=None):
    """The table behind `idf1`, for inspection: (C, gt_ids, pred_ids, kept_gt, kept_pred) with C int32 [n_obj, n_hyp] on
    the device, C[o, h] = the frames in which ground-truth identity gt_ids[o] and predicted identity pred_ids[h] have
    boxes within max_dist, and the two bool row masks in input order."""
    r = _id_passes(gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size)
    c = r.ws[:r.n_obj * r.n_hyp * 4].view(torch.int32).view(r.n_obj, r.n_hyp).clone()
    return c, r.obj_ids, r.hyp_ids, _input_order(r.gt), _input_order(r.pred)


def idf1(gt, pred, max_dist=0.75, *, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None,
         image_size=None):
    """IDF1 / IDP / IDR of a tracking result as the reference scores it (main.py:166-213: the centre band, then
    eval/eval.py::eval with motmetrics' `compare_to_groundtruth(..., 'iou', max_dist)` and its global ID assignment);
    the definition is DESIGN.md 3.11.  gt, pred: [n, 7] tensors on one ROCm device in the reference's column order
    (camera, id, frame, x, y, width, height), int32 / int64 / float32 / float64; columns 0-2 are read as int64, the boxes
    as fp64.  Ground-truth rows must be unique per (camera, frame, id).  A frame group is one (camera, frame) pair.

    Filters on the predictions, in this order: border=p with image_size=(W, H) (the centre band, applied to the ground
    truth too; default off), roi= a [C, Hr, Wr] uint8 mask stack with roi_cameras= the camera value of each plane
    (`isROIOutlier`; default off; a prediction whose camera has no plane is refused), min_cameras (identities seen by
    fewer cameras go), drop_repeats (the first row of equal (camera, id, frame) stays).

    Returns IdScores(idf1, idp, idr, idtp, idfp, idfn, num_objects, num_predictions, matches, kept): three floats (NaN
    on 0 / 0), five ints, matches int64 [M, 2] on the device = (ground-truth id, predicted id) of the optimal matching,
    kept bool [n_pred] on the device in input order.  The overlap counts are made by HIP kernels, the assignment by the
    library on the host; the host reads the counters, then the non-zero cells."""
    return _id_scores(_id_passes(gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size))


def _id_scores(r):
    """IdScores from the passes: the non-zero cells read back, the assignment on the host."""
    import ctypes
    import numpy as np
    lib, dev = _lib.load(), r.dev
    n_all = r.n_obj * r.n_hyp
    cap = min(n_all, max(4096, 4 * (r.n_obj + r.n_hyp)))
    while True:
        triples = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        _call.run(dev, lib.mtmc_id_cells, r.ws.data_ptr(), r.n_obj, r.n_hyp, triples.data_ptr() if cap else None, cap,
                  r.counters[2:3].data_ptr(), _call.stream(dev))
        num_objects, num_predictions, n_cells = r.counters.tolist()
        if n_cells <= cap:
            break
        cap = n_cells
    cells = triples[:n_cells].cpu().numpy()
    cells = np.ascontiguousarray(cells[np.lexsort((cells[:, 1], cells[:, 0]))])      # (the device lists them in any order)
    idtp, match = ctypes.c_int64(0), np.full(max(r.n_obj, 1), -1, dtype=np.int32)
    _lib.check(lib.mtmc_id_assign(cells.ctypes.data if n_cells else None, n_cells, r.n_obj, r.n_hyp, ctypes.addressof(idtp),
                                  match.ctypes.data, None))
    idtp = int(idtp.value)
    o = np.nonzero(match[:r.n_obj] >= 0)[0]
    matches = torch.stack([r.obj_ids[torch.from_numpy(o).to(dev)],
                           r.hyp_ids[torch.from_numpy(match[o].astype(np.int64)).to(dev)]], dim=1)
    idfn, idfp = num_objects - idtp, num_predictions - idtp
    div = lambda a, b: a / b if b else float("nan")                                  # noqa: E731
    return IdScores(div(2 * idtp, num_objects + num_predictions), div(idtp, idtp + idfp), div(idtp, idtp + idfn), idtp, idfp,
                    idfn, num_objects, num_predictions, matches, _input_order(r.pred))


# ---- the CLEAR MOT columns of the same result row (eval/eval.py:409-411 with motmetrics) ---------------
MotScores = collections.namedtuple("MotScores", "mota motp recall precision num_matches num_switches num_false_positives "
                                                "num_misses num_fragmentations mostly_tracked partially_tracked mostly_lost "
                                                "num_unique_objects num_objects num_predictions num_frames matched kept")


def _mot_passes(entry, gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size, overlap):
    if not drop_repeats:
        raise ValueError(f"mtmc_mpn.{entry}: drop_repeats must be True (the correspondence walk needs predicted ids that "
                         "are unique within a (camera, frame) group, as eval() always makes them)")
    return _id_passes(gt, pred, max_dist, min_cameras, True, roi, roi_cameras, border, image_size, entry, overlap)


def _mot_pairs(r, max_dist):
    """The candidate pass on the grouped sides of `_id_passes`: (pairs int32 [k, 3] = group, ground-truth row, prediction
    row in grouped order; d float64 [k]) on the device, sorted by (group, ground-truth row, prediction row).  One host read
    of the counter per pass; the pass is repeated once when the first list was too short."""
    g, q, dev, lib = r.gt, r.pred, r.dev, _lib.load()
    need = lib.mtmc_mot_pairs_workspace_bytes(r.n_groups)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    ptr = (lambda t: t.data_ptr()) if g.n > 0 and q.n > 0 else (lambda t: None)
    cap = max(4096, 4 * (g.n + q.n))
    while True:
        pairs = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        dist = torch.empty(cap, dtype=torch.float64, device=dev)
        _call.run(dev, lib.mtmc_mot_pairs, ptr(g.boxes), ptr(g.offsets), ptr(g.keep) if g.keep is not None else None, g.n,
                  ptr(q.boxes), ptr(q.offsets), ptr(q.keep), q.n, r.n_groups, float(max_dist), pairs.data_ptr(),
                  dist.data_ptr(), cap, counter.data_ptr(), ws.data_ptr(), need, _call.stream(dev))
        n_pairs = int(counter)
        if n_pairs <= cap:
            break
        cap = n_pairs
    pairs, dist = pairs[:n_pairs], dist[:n_pairs]
    # (the device lists them in any order; the keys are distinct, so the sorted list is the same on every run)
    order = torch.argsort(pairs[:, 1].long() * max(q.n, 1) + pairs[:, 2].long())
    return pairs[order].contiguous(), dist[order].contiguous()


def _mot_scores(r, max_dist):
    """MotScores from the passes: the candidates and the row keys read back, the walk on the host (in the library)."""
    import ctypes
    import numpy as np
    g, q, dev, lib = r.gt, r.pred, r.dev, _lib.load()
    pairs, dist = _mot_pairs(r, max_dist)
    host = lambda t: np.ascontiguousarray(t.cpu().numpy())                            # noqa: E731
    at = lambda a: a.ctypes.data if a is not None and a.size else None                # noqa: E731
    pairs, dist = host(pairs), host(dist)
    g_group, g_ident, g_pos, g_keep = host(g.group), host(g.ident), host(g.perm), host(g.keep) if g.keep is not None else None
    q_group, q_ident, q_keep = host(q.group), host(q.ident), host(q.keep)
    counts, total = np.zeros(_lib.MOT_COUNTS, dtype=np.int64), ctypes.c_double(0.0)
    match = np.full(max(g.n, 1), -1, dtype=np.int32)
    _lib.check(lib.mtmc_mot_walk(at(pairs), at(dist), pairs.shape[0], at(g_group), at(g_ident), at(g_pos), at(g_keep), g.n,
                                 at(q_group), at(q_ident), at(q_keep), q.n, r.n_groups, r.n_obj, r.n_hyp, counts.ctypes.data,
                                 ctypes.addressof(total), match.ctypes.data, None))
    (matches, switches, misses, false_positives, fragmentations, mostly_tracked, partially_tracked, mostly_lost, unique_objects,
     num_objects, num_predictions, frames) = counts.tolist()
    # matched, in input order on either side: the input index of the prediction row, -1 a miss, -2 dropped by the border
    m = torch.from_numpy(match[:g.n].astype(np.int64)).to(dev)
    matched = torch.empty(g.n, dtype=torch.int64, device=dev)
    matched[g.perm] = torch.where(m >= 0, q.perm[m.clamp(min=0)], m) if q.n else m
    detections = matches + switches
    div = lambda a, b: a / b if b else float("nan")                                  # noqa: E731
    return MotScores(1.0 - div(misses + switches + false_positives, num_objects), div(total.value, detections), div(detections, num_objects), div(detections, detections + false_positives),
                     matches, switches, false_positives, misses, fragmentations, mostly_tracked, partially_tracked,
                     mostly_lost, unique_objects, num_objects, num_predictions, frames, matched, _input_order(q))


def mot_pairs(gt, pred, max_dist=0.75, *, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None,
              image_size=None):
    """The candidates behind `mot_scores`, for inspection: (gt_index int64 [k], pred_index int64 [k], d float64 [k]) on the
    device -- every pair of a ground-truth row and a kept prediction row of one (camera, frame) with d <= max_dist, as
    input indices, sorted by (camera, frame, ground-truth id, predicted id).  A pair is listed exactly when it counts in
    `id_overlap_counts`."""
    r = _mot_passes("mot_pairs", gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size, False)
    pairs, dist = _mot_pairs(r, max_dist)
    return r.gt.perm[pairs[:, 1].long()], r.pred.perm[pairs[:, 2].long()], dist


def mot_scores(gt, pred, max_dist=0.75, *, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None,
               image_size=None):
    """The CLEAR MOT columns of the reference's result row (eval/eval.py:409-411: motmetrics' `compare_to_groundtruth(...,
    'iou', max_dist)`, `MOTAccumulator.update` frame by frame, then the metric functions); the definition is DESIGN.md
    3.12.  Tables, filters, groups and the pair test are those of `idf1`; drop_repeats must be True.  The groups are
    visited in ascending (camera, frame), one state for all cameras: an identity keeps the predicted id it was last
    matched to while the two are candidates (in input order), the rows left are assigned (most pairs, then the smallest
    sum of d), and a pair whose identity was last matched to another predicted id is a switch.

    Returns MotScores(mota, motp, recall, precision: floats, NaN on 0 / 0; num_matches, num_switches, num_false_positives,
    num_misses, num_fragmentations, mostly_tracked, partially_tracked, mostly_lost, num_unique_objects, num_objects,
    num_predictions, num_frames: ints; matched int64 [n_gt] on the device in input order = the input index of the matched
    prediction row, -1 for a miss, -2 for a ground-truth row the border filter dropped; kept as in IdScores).  motp is the
    mean DISTANCE of the matched pairs (motmetrics' convention: 0 is perfect).  The candidate pairs are made by a HIP
    kernel, the walk by the library on the host; the host reads the candidate count, then the candidates and row keys.
    Not built: num_transfer / num_ascend / num_migrate, a finite max_switch_time, the MOT text files."""
    r = _mot_passes("mot_scores", gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size, False)
    return _mot_scores(r, max_dist)


def tracking_summary(gt, pred, max_dist=0.75, *, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None,
                     image_size=None):
    """(IdScores, MotScores): the reference's summary row (without num_transfer, num_ascend, num_migrate) from one
    grouping and one filter pass; either part is exactly what `idf1` / `mot_scores` return."""
    r = _mot_passes("tracking_summary", gt, pred, max_dist, min_cameras, drop_repeats, roi, roi_cameras, border, image_size,
                    True)
    return _id_scores(r), _mot_scores(r, max_dist)
