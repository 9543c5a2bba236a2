"""The yardstick of `mtmc_mpn.idf1`: numpy only, loops over the (camera, frame) groups, the fp64 overlap expression of
DESIGN.md 3.11 written out, and the ID assignment as motmetrics poses it -- a plain Hungarian on the full
(objects + hypotheses)^2 matrix fpmatrix + fnmatrix of `id_global_assignment` -- which is deliberately NOT the
per-component max-weight form the library solves.  Also the union-find component statistics of `mtmc_id_assign`."""
import collections

import numpy as np

Result = collections.namedtuple("Result", "idf1 idp idr idtp idfp idfn num_objects num_predictions C gt_ids pred_ids "
                                          "kept kept_gt matches")
FORBIDDEN = 1 << 40


def border_keep(table, border, image_size):
    w, h = image_size
    x, y, bw, bh = (table[:, k].astype(np.float64) for k in (3, 4, 5, 6))
    cx, by = x + bw / 2, y + bh
    return (w * border <= cx) & (cx <= w - w * border) & (h * border <= by) & (by <= h - h * border)


def roi_outlier(row, mask):
    """eval.py::isROIOutlier with the corners computed in fp64 and truncated to int64"""
    hr, wr = mask.shape
    x, y, bw, bh = (np.float64(v) for v in row[3:7])
    with np.errstate(invalid="ignore"):
        xs = [np.float64(x).astype(np.int64), np.float64(x + bw).astype(np.int64)]
        ys = [np.float64(y).astype(np.int64), np.float64(y + bh).astype(np.int64)]
    for xc in xs:
        if 0 <= xc < wr:
            for yc in ys:
                if 0 <= yc < hr and mask[yc, xc] < 255:
                    return True
    return False


def filter_predictions(pred, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None, image_size=None):
    """bool [n_pred] in input order: steps 1-4 of the definition"""
    n = pred.shape[0]
    keep = np.ones(n, dtype=bool)
    if border is not None:
        keep &= border_keep(pred, border, image_size)
    if roi is not None:
        plane = {int(c): k for k, c in enumerate(roi_cameras)}
        for i in range(n):
            if int(pred[i, 0]) not in plane:
                raise ValueError("a prediction's camera has no plane")
            if keep[i] and roi_outlier(pred[i], roi[plane[int(pred[i, 0])]]):
                keep[i] = False
    cams = collections.defaultdict(set)
    for i in np.nonzero(keep)[0]:
        cams[int(pred[i, 1])].add(int(pred[i, 0]))
    for i in np.nonzero(keep)[0]:
        if len(cams[int(pred[i, 1])]) < min_cameras:
            keep[i] = False
    if drop_repeats:
        seen = set()
        for i in np.nonzero(keep)[0]:
            key = (int(pred[i, 0]), int(pred[i, 1]), int(pred[i, 2]))
            if key in seen:
                keep[i] = False
            seen.add(key)
    return keep


def pair_counts(a, b, max_dist):
    """one ground-truth box against one predicted box, every operation a separate fp64 rounding"""
    ax, ay, aw, ah = (np.float64(v) for v in a)
    bx, by, bw, bh = (np.float64(v) for v in b)
    iw = max(np.float64(0), min(ax + aw, bx + bw) - max(ax, bx))
    ih = max(np.float64(0), min(ay + ah, by + bh) - max(ay, by))
    inter = iw * ih
    union = aw * ah + bw * bh - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.float64(1) - inter / union
    return bool(d <= max_dist)


def overlap_counts(gt, pred, max_dist):
    """C int32 [n_obj, n_hyp] over the sorted distinct id values of either table, by a loop over the groups"""
    gt_ids, pred_ids = np.unique(gt[:, 1].astype(np.int64)), np.unique(pred[:, 1].astype(np.int64))
    orow = {int(v): k for k, v in enumerate(gt_ids)}
    hcol = {int(v): k for k, v in enumerate(pred_ids)}
    groups = collections.defaultdict(lambda: ([], []))
    for i in range(gt.shape[0]):
        groups[(int(gt[i, 0]), int(gt[i, 2]))][0].append(i)
    for j in range(pred.shape[0]):
        groups[(int(pred[j, 0]), int(pred[j, 2]))][1].append(j)
    c = np.zeros((len(gt_ids), len(pred_ids)), dtype=np.int32)
    for rows, cols in groups.values():
        for i in rows:
            for j in cols:
                if pair_counts(gt[i, 3:7], pred[j, 3:7], max_dist):
                    c[orow[int(gt[i, 1])], hcol[int(pred[j, 1])]] += 1
    return c, gt_ids, pred_ids


def hungarian(cost):
    """Minimum-cost perfect assignment of a square integer matrix (rows to columns), O(n^3); returns col_of_row"""
    cost = np.asarray(cost, dtype=np.int64)
    n = cost.shape[0]
    u, v = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    p, way = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    big = np.iinfo(np.int64).max // 4
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, big, dtype=np.int64)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], big)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col_of_row = np.zeros(n, dtype=np.int64)
    col_of_row[p[1:] - 1] = np.arange(n)
    return col_of_row


def motmetrics_matrices(c, oc, hc):
    """fpmatrix, fnmatrix of motmetrics' id_global_assignment, NaN replaced by FORBIDDEN"""
    no, nh = c.shape
    fp = np.zeros((no + nh, no + nh), dtype=np.int64)
    fn = np.zeros((no + nh, no + nh), dtype=np.int64)
    fp[no:, :nh] = FORBIDDEN
    fn[:no, nh:] = FORBIDDEN
    for r in range(no):
        fn[r, :nh] = oc[r]
        fn[r, nh + r] = oc[r]
    for k in range(nh):
        fp[:no, k] = hc[k]
        fp[k + no, k] = hc[k]
    fp[:no, :nh] -= c
    fn[:no, :nh] -= c
    return fp, fn


def id_scores(c, oc, hc):
    """(idtp, idfp, idfn, matches as (row, column) with C > 0) from the full motmetrics problem"""
    no, nh = c.shape
    num_objects, num_predictions = int(np.sum(oc)), int(np.sum(hc))
    if no + nh == 0:
        return 0, 0, 0, []
    fp, fn = motmetrics_matrices(c.astype(np.int64), np.asarray(oc, dtype=np.int64), np.asarray(hc, dtype=np.int64))
    cols = hungarian(fp + fn)
    rows = np.arange(no + nh)
    idfn, idfp = int(fn[rows, cols].sum()), int(fp[rows, cols].sum())
    assert idfn < FORBIDDEN and idfp < FORBIDDEN
    idtp = num_objects - idfn
    assert idtp == num_predictions - idfp
    matches = [(r, int(cols[r])) for r in range(no) if cols[r] < nh and c[r, cols[r]] > 0]
    return idtp, idfp, idfn, matches


def _div(a, b):
    return a / b if b else float("nan")


def idf1(gt, pred, max_dist=0.75, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None, image_size=None):
    gt, pred = np.asarray(gt), np.asarray(pred)
    kept = filter_predictions(pred, min_cameras, drop_repeats, roi, roi_cameras, border, image_size)
    kept_gt = border_keep(gt, border, image_size) if border is not None else np.ones(gt.shape[0], dtype=bool)
    g, p = gt[kept_gt], pred[kept]
    c_small, gids, pids = overlap_counts(g, p, max_dist)
    # C over the identities of the UNFILTERED tables, as the library indexes it
    gt_ids, pred_ids = np.unique(gt[:, 1].astype(np.int64)), np.unique(pred[:, 1].astype(np.int64))
    c = np.zeros((len(gt_ids), len(pred_ids)), dtype=np.int32)
    c[np.ix_(np.searchsorted(gt_ids, gids), np.searchsorted(pred_ids, pids))] = c_small
    oc = [int(np.sum(g[:, 1].astype(np.int64) == v)) for v in gids]
    hc = [int(np.sum(p[:, 1].astype(np.int64) == v)) for v in pids]
    idtp, idfp, idfn, pairs = id_scores(c_small, oc, hc)
    no, nh = g.shape[0], p.shape[0]
    return Result(_div(2 * idtp, no + nh), _div(idtp, idtp + idfp), _div(idtp, idtp + idfn), idtp, idfp, idfn, no, nh, c,
                  gt_ids, pred_ids, kept, kept_gt, sorted((int(gids[r]), int(pids[k])) for r, k in pairs))


def component_stats(c):
    """(components, rows, columns of the largest) of the support graph of C, as `mtmc_id_assign` reports them: union-find
    over the identities that have a non-zero cell; largest = most rows x columns, ties by more rows"""
    c = np.asarray(c)
    no, nh = c.shape
    parent = list(range(no + nh))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    rr, cc = np.nonzero(c)
    for r, k in zip(rr.tolist(), cc.tolist()):
        a, b = find(r), find(no + k)
        if a != b:
            parent[b] = a
    rows, cols = collections.Counter(), collections.Counter()
    for r in set(rr.tolist()):
        rows[find(r)] += 1
    for k in set(cc.tolist()):
        cols[find(no + k)] += 1
    best = max(((rows[root] * cols[root], rows[root], cols[root]) for root in rows), default=(0, 0, 0))
    return len(rows), best[1], best[2]
