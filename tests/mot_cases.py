"""The named cases of the CLEAR MOT tests, shared by the yardstick test and the walk test (CPU), the GPU
test and tests/golden/make_golden_mot.py: every case of tests/idf1_cases.py, plus the ones below that exercise the walk.
A case is (gt, pred, kwargs, hand): two [n, 7] numpy tables (camera, id, frame, x, y, width, height), the keyword arguments
of `mot_scores`, and the values derived by hand (a dict, possibly empty; only fields of MotScores).  Everything comes from
fixed seeds.

The boxes of the hand cases are 100 x 10 on one line, so that two of them offset by s along x have I = 100 - s,
U = 100 + s and d = 2 s / (100 + s): a candidate up to s = 60."""
import os

import numpy as np

import idf1_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mot_cases.npz")


def d_of(s):
    """the distance of two such boxes offset by s, with the roundings of the definition: 1 - I / U"""
    return 1.0 - (100 - s) * 10 / (2 * 100 * 10 - (100 - s) * 10)


def rows(*items, dtype=np.int64):
    """(camera, id, frame, x) -> table rows of 100 x 10 boxes at y = 0"""
    return np.array([(cam, ident, frame, x, 0, 100, 10) for cam, ident, frame, x in items], dtype=dtype).reshape(-1, 7)


def _continuity_keeps(with_frame_0):
    # frame 1: o1 at 0, o2 at 20, h1 at 30, h2 at -10.  Straight (o1-h1, o2-h2): s = 30 twice, sum 120 / 130; crossed
    # (o1-h2, o2-h1): s = 10 twice, sum 40 / 110: the assignment alone crosses.  Frame 0 (exact boxes, far apart)
    # establishes the straight pairs, and continuity keeps them: two MATCHes, no switch.
    gt = rows((1, 1, 1, 0), (1, 2, 1, 20))
    pred = rows((1, 1, 1, 30), (1, 2, 1, -10))
    if not with_frame_0:
        return gt, pred, dict(min_cameras=1), dict(num_matches=2, num_switches=0, num_misses=0, num_false_positives=0,
                                                   matched=[1, 0], motp=(d_of(10) + d_of(10)) / 2, mota=1.0, num_frames=1)
    first = rows((1, 1, 0, 0), (1, 2, 0, 500))
    gt, pred = np.concatenate([first, gt]), np.concatenate([first, pred])
    return gt, pred, dict(min_cameras=1), dict(num_matches=4, num_switches=0, num_misses=0, num_false_positives=0,
                                               matched=[0, 1, 2, 3], motp=(0.0 + 0.0 + d_of(30) + d_of(30)) / 4, num_frames=2)


def _continuity_order(swapped):
    # o1 remembers h from frame 0.  In frame 1 o1 is there but far from h, which o2 takes: now both remember h.  In frame 2
    # both are candidates of h alone (o1 at s = 6, o2 at s = 2): the first in INPUT order keeps it, the other is a MISS.
    o1, o2, h = 1, 2, 7
    last = [(1, o1, 2, 0), (1, o2, 2, 8)]
    gt = rows((1, o1, 0, 0), (1, o1, 1, 1000), (1, o2, 1, 0), *(last[::-1] if swapped else last))
    pred = rows((1, h, 0, 0), (1, h, 1, 0), (1, h, 2, 6))
    hand = dict(num_matches=3, num_switches=0, num_misses=2, num_false_positives=0, num_frames=3, mostly_lost=0)
    if swapped:       # o2: 1 1, o1: 1 0 0
        hand.update(matched=[0, -1, 1, 2, -1], motp=(0.0 + 0.0 + d_of(2)) / 3, num_fragmentations=0, mostly_tracked=1,
                    partially_tracked=1)
    else:             # o1: 1 0 1 (one fragmentation), o2: 1 0
        hand.update(matched=[0, -1, 1, 2, -1], motp=(0.0 + 0.0 + d_of(6)) / 3, num_fragmentations=1, mostly_tracked=0,
                    partially_tracked=2)
    return gt, pred, dict(min_cameras=1), hand


def _switch_across_cameras(same_id):
    # one identity, two frames in camera 1 (predicted id 7) and two in camera 2 (predicted id 8, or 7 again): the state
    # carries over from camera 1, so the first row in camera 2 is a SWITCH and the second a MATCH
    gt = rows((1, 5, 0, 0), (1, 5, 1, 3), (2, 5, 0, 0), (2, 5, 1, 3))
    pred = gt.copy()
    pred[:, 1] = [7, 7, 7, 7] if same_id else [7, 7, 8, 8]
    hand = dict(num_matches=4 if same_id else 3, num_switches=0 if same_id else 1, num_misses=0, num_false_positives=0,
                mota=1.0 if same_id else 1.0 - 1 / 4, motp=0.0, matched=[0, 1, 2, 3], num_frames=4, mostly_tracked=1)
    return gt, pred, dict(min_cameras=1), hand


def _fragment():
    # identity 0 is tracked 1 0 0 1 1 0 1 0 0: tracked -> miss three times, but the last one is behind its last tracked
    # row and does not count: 2 fragmentations; 4 of 9 rows: partially tracked.  Identity 1 is never tracked: no
    # fragmentation, mostly lost.
    pattern = [1, 0, 0, 1, 1, 0, 1, 0, 0]
    gt = rows(*[(1, ident, f, 300 * ident + f) for ident in (0, 1) for f in range(9)])
    pred = rows(*[(1, 0, f, f) for f in range(9) if pattern[f]])
    return gt, pred, dict(min_cameras=1), dict(num_fragmentations=2, num_matches=4, num_misses=14, num_switches=0,
                                               mostly_tracked=0, partially_tracked=1, mostly_lost=1, num_unique_objects=2,
                                               num_frames=9, recall=4 / 18, precision=1.0, mota=1.0 - 14 / 18)


def _ratio_edges():
    # 4 of 5, 1 of 5, 3 of 5 and 0 of 5 rows tracked: 5 t >= 4 n only for the first, 5 t < n only for the last
    tracked = {0: 4, 1: 1, 2: 3, 3: 0}
    gt = rows(*[(1, ident, f, 300 * ident) for ident in tracked for f in range(5)])
    pred = rows(*[(1, ident, f, 300 * ident) for ident, t in tracked.items() for f in range(t)])
    return gt, pred, dict(min_cameras=1), dict(mostly_tracked=1, partially_tracked=2, mostly_lost=1, num_matches=8,
                                               num_misses=12, num_fragmentations=0, num_unique_objects=4, num_frames=5)


def _one_sided(gt_rows, pred_rows):
    # frame 0 has ground truth only, frame 1 predictions only
    gt = rows(*[(1, 0, 0, 0)] * gt_rows)
    pred = rows(*[(1, 0, 1, 0)] * pred_rows)
    nan = float("nan")
    hand = dict(num_matches=0, num_switches=0, num_misses=gt_rows, num_false_positives=pred_rows, num_frames=gt_rows + pred_rows,
                motp=nan, recall=0.0 if gt_rows else nan, precision=0.0 if pred_rows else nan,
                mota=1.0 - (gt_rows + pred_rows) / gt_rows if gt_rows else nan, mostly_lost=gt_rows, num_unique_objects=gt_rows)
    return gt, pred, dict(min_cameras=1), hand


def _crowded(seed=0):
    """2 cameras x 12 identities x 30 frames of 40 x 30 boxes that random-walk by up to +-9 a frame inside 220 x 160, each
    present with probability 0.9; the predictions are the ground truth with 10 % of the rows dropped, positions jittered
    by +-10 and sizes by x [0.8, 1.25] (floats), the predicted ids of two identities exchanged from mid-sequence on in
    camera 2, and the rows shuffled"""
    g = np.random.default_rng(seed)
    table = []
    for cam in (1, 2):
        pos = np.stack([g.uniform(0, 180, 12), g.uniform(0, 130, 12)], axis=1)
        for f in range(30):
            pos = np.clip(pos + g.integers(-9, 10, size=pos.shape), 0, [180, 130])
            for ident in np.nonzero(g.random(12) < 0.9)[0]:
                table.append((cam, ident, f, pos[ident, 0], pos[ident, 1], 40, 30))
    gt = np.array(table, dtype=np.float64)
    pred = gt[g.random(gt.shape[0]) >= 0.1].copy()
    pred[:, 3:5] += g.uniform(-10, 10, (pred.shape[0], 2))
    pred[:, 5:7] *= g.uniform(0.8, 1.25, (pred.shape[0], 2))
    late = (pred[:, 0] == 2) & (pred[:, 2] >= 15)
    a, b = late & (pred[:, 1] == 3), late & (pred[:, 1] == 8)
    pred[a, 1], pred[b, 1] = 8, 3
    return gt, pred[g.permutation(pred.shape[0])], dict(min_cameras=1), {}


def _equal_boxes():
    """one 80 x 80 group of equal boxes (6 400 candidates, all at d = 0) beside 10 single rows: for the pair list alone --
    every assignment of the big group is an optimum"""
    big = rows(*[(1, ident, 0, 0) for ident in range(80)])
    single = rows(*[(2, 100 + k, k, 50 * k) for k in range(10)])
    gt = np.concatenate([single[:5], big, single[5:]])
    return gt, gt[::-1].copy(), dict(min_cameras=1), {}


def _tables_of(make):
    return lambda: make()[:3] + ({},)                      # (the hand values there are IdScores fields: not taken over)


CASES = {name: _tables_of(make) for name, make in idf1_cases.CASES.items()}
CASES.update({
    "continuity_keeps": lambda: _continuity_keeps(True), "continuity_keeps_alone": lambda: _continuity_keeps(False),
    "continuity_order": lambda: _continuity_order(False), "continuity_order_swapped": lambda: _continuity_order(True),
    "switch_across_cameras": lambda: _switch_across_cameras(False), "switch_same_id": lambda: _switch_across_cameras(True),
    "fragment": _fragment, "ratio_edges": _ratio_edges,
    "one_sided": lambda: _one_sided(1, 1), "one_sided_no_pred": lambda: _one_sided(1, 0),
    "one_sided_no_gt": lambda: _one_sided(0, 1), "one_sided_nothing": lambda: _one_sided(0, 0),
    "crowded": _crowded,
})
ORDER_DEPENDENT = ("continuity_order", "continuity_order_swapped")      # the result depends on the input order by definition
PAIR_CASES = {"equal_boxes": _equal_boxes}                               # for `mot_pairs` alone: the assignment has ties
CROSSING_A_WORKGROUP = ("big_group_last", "big_group_first")             # one 70 x 130 group: 9 100 pairs, 4 096 a workgroup


def case(name):
    return (CASES.get(name) or PAIR_CASES[name])()


_yardstick = {}


def yardstick(name):
    """(the yardstick's Result, the hand values) of a case, computed once and shared by every test that asks"""
    if name not in _yardstick:
        import mot_ref
        gt, pred, kw, hand = case(name)
        _yardstick[name] = (mot_ref.mot_scores(gt, pred, check_unique=name not in PAIR_CASES, **kw), hand)
    return _yardstick[name]


def same_float(a, b):
    return (a != a and b != b) or a == b


def check_hand(r, hand):
    """the hand-derived values against a result (the yardstick's, or the library's with `matched` as a numpy array)"""
    for key, want in hand.items():
        got = getattr(r, key)
        if key == "matched":
            assert np.asarray(got).tolist() == want, (key, np.asarray(got).tolist(), want)
        elif isinstance(want, float):
            assert same_float(got, want), (key, got, want)
        else:
            assert got == want, (key, got, want)
