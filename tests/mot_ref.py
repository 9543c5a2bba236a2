"""The yardstick of `mtmc_mpn.mot_scores`: numpy only.  The filters and the pair test are those of the IDF1
yardstick (tests/idf1_ref.py); the rest is the definition written out -- a loop over the (camera, frame) groups in ascending
order, the continuity step in input order, then ONE assignment per group over all rows not taken, posed as motmetrics
poses it: a plain Hungarian on a square matrix in which a big cost stands for every pair that is no candidate.  That is
deliberately NOT the per-component lexicographic form the library solves.  `solver=` lets tests/golden/make_golden_mot.py
put scipy's linear_sum_assignment in its place.

While it runs the yardstick asserts the condition on the inputs: wherever the assignment has a choice, the optimum is
unique by a margin -- with any one chosen pair forbidden the result has fewer pairs or a sum larger by more than 1e-9."""
import collections
import math

import numpy as np

import idf1_ref

FIELDS = ("mota motp recall precision num_matches num_switches num_false_positives num_misses num_fragmentations "
          "mostly_tracked partially_tracked mostly_lost num_unique_objects num_objects num_predictions num_frames")
Result = collections.namedtuple("Result", FIELDS + " matched kept kept_gt pairs dist_sum solver_groups largest")
COUNTS = ("num_matches num_switches num_misses num_false_positives num_fragmentations mostly_tracked partially_tracked "
          "mostly_lost num_unique_objects num_objects num_predictions num_frames").split()       # the fixture's order
BIG = 1024.0                   # above every sum of distances (each <= 1) of a group of fewer than 1024 rows; a power of two
MARGIN = 1e-9


def distance(a, b):
    """1 - I / U of two boxes (x, y, width, height), every operation a separate fp64 rounding; U = 0 gives NaN"""
    ax, ay, aw, ah = (np.float64(v) for v in a)
    bx, by, bw, bh = (np.float64(v) for v in b)
    iw = max(np.float64(0), min(ax + aw, bx + bw) - max(ax, bx))
    ih = max(np.float64(0), min(ay + ah, by + bh) - max(ay, by))
    inter = iw * ih
    union = aw * ah + bw * bh - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(1) - inter / union)


def hungarian(cost):
    """Minimum-cost perfect assignment of a square fp64 matrix (rows to columns), O(n^3); returns col_of_row"""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], np.inf)
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


def big_cost(d):
    """the square matrix of the assignment: BIG for a pair that is no candidate (NaN in d) and for the padding"""
    n, m = d.shape
    assert max(n, m) < BIG
    cost = np.full((max(n, m), max(n, m)), BIG)
    cost[:n, :m] = np.where(np.isnan(d), BIG, d)
    return cost


def solve(d):
    """[(row, column)] of the assignment of d [n, m] (NaN = no candidate): the most pairs, then the smallest sum"""
    cols = hungarian(big_cost(d))
    return [(i, int(cols[i])) for i in range(d.shape[0]) if cols[i] < d.shape[1] and not np.isnan(d[i, cols[i]])]


def pair_sum(d, pairs):
    return math.fsum(d[i, j] for i, j in pairs)


def assert_unique(d, pairs, solver, where):
    """the condition on the inputs: forbid each chosen pair in turn and solve again"""
    best = pair_sum(d, pairs)
    for i, j in pairs:
        other = d.copy()
        other[i, j] = np.nan
        again = solver(other)
        assert len(again) < len(pairs) or pair_sum(other, again) > best + MARGIN, \
            f"{where}: the assignment is not unique by {MARGIN} (an error of the test data): without ({i}, {j}) " \
            f"{len(again)} pairs, sum {pair_sum(other, again)!r} against {len(pairs)} pairs, sum {best!r}"


def candidates(gt, pred, kept_gt, kept, max_dist):
    """{(camera, frame): (rows of gt, rows of pred, d [ng, np] with NaN where the pair is no candidate)}, kept rows in input
    order; a pair is a candidate exactly when `idf1_ref.pair_counts` counts it"""
    groups = collections.defaultdict(lambda: ([], []))
    for i in np.nonzero(kept_gt)[0]:
        groups[(int(gt[i, 0]), int(gt[i, 2]))][0].append(int(i))
    for j in np.nonzero(kept)[0]:
        groups[(int(pred[j, 0]), int(pred[j, 2]))][1].append(int(j))
    out = {}
    for key, (rows, cols) in groups.items():
        d = np.full((len(rows), len(cols)), np.nan)
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                if idf1_ref.pair_counts(gt[i, 3:7], pred[j, 3:7], max_dist):
                    d[a, b] = distance(gt[i, 3:7], pred[j, 3:7])
                    assert d[a, b] <= max_dist
        out[key] = (rows, cols, d)
    return out


def _div(a, b):
    return a / b if b else float("nan")


def mot_scores(gt, pred, max_dist=0.75, min_cameras=2, drop_repeats=True, roi=None, roi_cameras=None, border=None,
               image_size=None, solver=solve, check_unique=True):
    assert drop_repeats
    gt, pred = np.asarray(gt), np.asarray(pred)
    kept = idf1_ref.filter_predictions(pred, min_cameras, True, roi, roi_cameras, border, image_size)
    kept_gt = idf1_ref.border_keep(gt, border, image_size) if border is not None else np.ones(gt.shape[0], dtype=bool)
    groups = candidates(gt, pred, kept_gt, kept, max_dist)
    gid, pid = gt[:, 1].astype(np.int64), pred[:, 1].astype(np.int64)
    last = {}                                                    # m[o]
    history = collections.defaultdict(list)                      # per identity: 1 tracked, 0 a miss, in visiting order
    matched = np.where(kept_gt, -1, -2).astype(np.int64)
    counts = collections.Counter()
    dist_sum, pairs, solver_groups, largest = 0.0, [], 0, (0, 0)
    for key in sorted(groups):
        rows, cols, d = groups[key]
        assert len({int(pid[j]) for j in cols}) == len(cols), "predicted ids repeat inside a group"
        mate, taken, event = {}, set(), {}
        for a, i in enumerate(rows):                             # step 1: continuity, in input order
            h = last.get(int(gid[i]))
            for b, j in enumerate(cols):
                if h is not None and int(pid[j]) == h and b not in taken and not np.isnan(d[a, b]):
                    mate[a] = b
                    taken.add(b)
                    event[a] = "MATCH"
        fa = [a for a in range(len(rows)) if a not in mate and not np.isnan(d[a]).all()]
        fb = [b for b in range(len(cols)) if b not in taken]
        sub = d[np.ix_(fa, fb)] if fa and fb else np.zeros((0, 0))
        has = ~np.isnan(sub)
        chosen = []
        if has.any():                                            # step 2: the assignment over the rows not taken
            # a candidate pair whose two rows have no other candidate is a pair of every optimum: no choice there
            alone = has & (has.sum(1, keepdims=True) == 1) & (has.sum(0, keepdims=True) == 1)
            chosen = list(zip(*np.nonzero(alone)))
            ra = np.nonzero(has.any(1) & ~alone.any(1))[0]
            rb = np.nonzero(has.any(0) & ~alone.any(0))[0]
            if len(ra):
                rest = sub[np.ix_(ra, rb)]
                got = solver(rest)
                if check_unique:
                    assert_unique(rest, got, solver, f"group {key}")
                chosen += [(ra[x], rb[y]) for x, y in got]
                solver_groups += 1
                if len(ra) * len(rb) > largest[0] * largest[1]:
                    largest = (len(ra), len(rb))
        for x, y in chosen:
            a, b = fa[x], fb[y]
            o, h = int(gid[rows[a]]), int(pid[cols[b]])
            mate[a] = b
            taken.add(b)
            event[a] = "SWITCH" if o in last and last[o] != h else "MATCH"
        for a in sorted(range(len(rows)), key=lambda a: (int(gid[rows[a]]), a)):      # ascending ground-truth id
            o = int(gid[rows[a]])
            if a in mate:
                b = mate[a]
                last[o] = int(pid[cols[b]])
                matched[rows[a]] = cols[b]
                counts[event[a]] += 1
                dist_sum = dist_sum + float(d[a, b])             # one sequential fp64 addition per pair
                history[o].append(1)
            else:
                counts["MISS"] += 1
                history[o].append(0)
        counts["FP"] += len(cols) - len(taken)
        counts["frames"] += 1
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                if not np.isnan(d[a, b]):
                    pairs.append((key[0], key[1], int(gid[i]), int(pid[j]), i, j, float(d[a, b])))
    mt = pt = ml = frag = 0
    for seq in history.values():
        t, n = sum(seq), len(seq)
        if 5 * t >= 4 * n:
            mt += 1
        elif 5 * t < n:
            ml += 1
        else:
            pt += 1
        if t:
            first, end = seq.index(1), n - seq[::-1].index(1)
            frag += sum(1 for k in range(first + 1, end) if seq[k] == 0 and seq[k - 1] == 1)
    no, nh = int(kept_gt.sum()), int(kept.sum())
    matches, switches, misses, fps = counts["MATCH"], counts["SWITCH"], counts["MISS"], counts["FP"]
    det = matches + switches
    assert det + misses == no and det + fps == nh
    pairs.sort()
    return Result(1.0 - _div(misses + switches + fps, no), _div(dist_sum, det), _div(det, no), _div(det, det + fps), matches,
                  switches, fps, misses, frag, mt, pt, ml, len(history), no, nh, counts["frames"], matched, kept, kept_gt,
                  [(i, j, dd) for _, _, _, _, i, j, dd in pairs], dist_sum, solver_groups, largest)
