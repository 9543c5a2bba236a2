"""The named cases of the IDF1 tests, shared by the yardstick test (CPU), the GPU test and tests/golden/make_golden_idf1.py.
Every case is (gt, pred, kwargs, hand): two [n, 7] numpy tables (camera, id, frame, x, y, width, height), the keyword
arguments of `idf1`, and the values derived by hand (a dict, possibly empty).  Everything comes from fixed seeds."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idf1_cases.npz")


def tracks(n_cam=3, n_id=4, n_frames=5):
    """identity i drives along x in every camera: boxes of distinct identities never touch"""
    rows = [(cam, ident, f, 100 * ident + 7 * f, 50 * cam + 3 * f, 40, 30)
            for cam in range(1, n_cam + 1) for ident in range(n_id) for f in range(n_frames)]
    return np.array(rows, dtype=np.int64)


def _identical():
    gt = tracks()
    return gt, gt.copy(), {}, dict(idf1=1.0, idp=1.0, idr=1.0, idtp=60, idfp=0, idfn=0, num_objects=60, num_predictions=60,
                                   matches=[(0, 0), (1, 1), (2, 2), (3, 3)])


def _merged():
    # predicted ids 1 and 2 merged into 1: the rows that were id 2 now repeat (camera, 1, frame) and go (15 of 60); ground
    # truth 2 is left without a partner
    gt = tracks()
    pred = gt.copy()
    pred[pred[:, 1] == 2, 1] = 1
    return gt, pred, {}, dict(idtp=45, idfp=0, idfn=15, idf1=90 / 105, idp=1.0, idr=45 / 60, num_predictions=45)


def _split():
    # identity 0 changes its predicted id to 100 from frame 3 on: 9 of its 15 rows stay with the matched id
    gt = tracks()
    pred = gt.copy()
    pred[(pred[:, 1] == 0) & (pred[:, 2] >= 3), 1] = 100
    return gt, pred, {}, dict(idtp=54, idfp=6, idfn=6, idf1=108 / 120, matches=[(0, 0), (1, 1), (2, 2), (3, 3)])


def _threshold(max_dist):
    # id 1: (0,0,10,10) against (0,6,10,10): I / U = 40 / 160, d = 0.75 exactly; id 2: zero-area boxes, U = 0; id 3: disjoint
    gt = np.array([(cam, ident, 0) + box for cam in (1, 2)
                   for ident, box in ((1, (0, 0, 10, 10)), (2, (50, 50, 0, 0)), (3, (100, 100, 10, 10)))], dtype=np.int64)
    pred = np.array([(cam, ident, 0) + box for cam in (1, 2)
                     for ident, box in ((1, (0, 6, 10, 10)), (2, (50, 50, 0, 0)), (3, (200, 200, 10, 10)))], dtype=np.int64)
    on = max_dist >= 0.75
    return gt, pred, dict(max_dist=max_dist), dict(idtp=2 if on else 0, idfp=4 if on else 6, idfn=4 if on else 6,
                                                   idf1=(4 if on else 0) / 12, matches=[(1, 1)] if on else [])


def _empty_sides():
    # camera 3 only in the ground truth, camera 4 only in the predictions; in camera 1 frame 0 has no prediction and frame 9
    # no ground truth
    gt = tracks(3, 3, 4)
    pred = gt.copy()
    pred[pred[:, 0] == 3, 0] = 4
    pred = pred[~((pred[:, 0] == 1) & (pred[:, 2] == 0))]
    pred[(pred[:, 0] == 1) & (pred[:, 2] == 3), 2] = 9
    return gt, pred, {}, dict(idtp=3 * (2 + 4), num_objects=36, num_predictions=33)


def _big_group(first):
    """one (camera, frame) of 70 x 130 rows beside 200 groups of 1 x 1 and 1 x 2"""
    g = np.random.default_rng(11)
    big_cam, small_cam = (0, 5) if first else (9, 5)
    gx, gy = np.meshgrid(np.arange(10) * 60, np.arange(7) * 50)
    gt_big = np.stack([np.full(70, big_cam), np.arange(70), np.zeros(70, dtype=np.int64), gx.ravel(), gy.ravel(),
                       np.full(70, 40), np.full(70, 30)], axis=1)
    near = gt_big.copy()
    near[:, 3:5] += g.integers(-6, 7, size=(70, 2))
    far = np.stack([np.full(60, big_cam), 70 + np.arange(60), np.zeros(60, dtype=np.int64), g.integers(0, 600, 60),
                    g.integers(0, 350, 60), g.integers(10, 60, 60), g.integers(10, 60, 60)], axis=1)
    pred_big = np.concatenate([near, far])[g.permutation(130)]
    gt_small = np.stack([np.full(200, small_cam), np.arange(200) % 70, np.arange(200), np.full(200, 10), np.full(200, 10),
                         np.full(200, 20), np.full(200, 20)], axis=1)
    extra = gt_small[::2].copy()                       # every other small group has a second prediction, off by a few pixels
    extra[:, 1] += 70
    extra[:, 3] += 4
    pred = np.concatenate([gt_small, pred_big, extra]).astype(np.int64)
    gt = np.concatenate([gt_small, gt_big]).astype(np.int64)
    return gt, pred, dict(min_cameras=1), {}


def _id_values():
    gt = tracks()
    pred = gt.copy()
    for table, names in ((gt, {0: -7, 1: 2 ** 33 + 5, 2: 10 ** 6, 3: 3}), (pred, {0: 2 ** 40, 1: -1, 2: -2 ** 35, 3: 17})):
        col = table[:, 1].copy()
        for old, new in names.items():
            table[col == old, 1] = new
    return gt, pred, {}, dict(idf1=1.0, idtp=60, matches=[(-7, 2 ** 40), (3, 17), (10 ** 6, -2 ** 35), (2 ** 33 + 5, -1)])


def _fractional():
    """float boxes with fractional coordinates; max_dist is the distance of the first pair itself, so that pair sits on the
    threshold and a fused multiply-add in U would be free to flip it"""
    g = np.random.default_rng(5)
    n = 40
    keys = np.stack([1 + np.arange(n) % 2, np.arange(n) // 2 % 5, np.arange(n) // 10], axis=1).astype(np.float64)
    box = np.concatenate([g.uniform(0, 50, (n, 2)), g.uniform(20.3, 61.7, (n, 2))], axis=1)
    gt = np.concatenate([keys, box], axis=1)
    pred = gt.copy()
    pred[:, 3:5] += g.uniform(-9, 9, (n, 2))
    pred[:, 5:7] *= g.uniform(0.8, 1.25, (n, 2))
    import idf1_ref
    a, b = gt[0, 3:7], pred[0, 3:7]
    iw = max(0.0, min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]))
    inter = iw * ih
    d = 1.0 - inter / (a[2] * a[3] + b[2] * b[3] - inter)
    assert idf1_ref.pair_counts(a, b, d)
    return gt, pred, dict(max_dist=float(d)), {}


def _min_cameras():
    # id 7 lives in camera 1 only: dropped
    gt = tracks(2, 2, 3)
    pred = np.concatenate([gt, np.array([(1, 7, f, 500, 10, 40, 30) for f in range(3)], dtype=np.int64)])
    return gt, pred, {}, dict(idtp=12, idfp=0, idfn=0, num_predictions=12)


ROI = np.full((2, 12, 16), 255, dtype=np.uint8)
ROI[1, :, :] = 254                                     # camera 2's plane: every pixel just below 255
ROI[0, 3, 5] = 254
ROI[0, 11, 15] = 0


def _min_cameras_after_roi():
    # id 1 is in cameras 1 and 2, but every row of camera 2 is an ROI outlier: one camera is left, so id 1 goes altogether;
    # id 0 stays in cameras 1 and 3 (plane of camera 3 = all 255)
    rows = [(cam, ident, f, 1 + ident, 1, 2, 2) for cam, ident in ((1, 0), (3, 0), (1, 1), (2, 1)) for f in range(2)]
    gt = np.array(rows, dtype=np.int64)
    roi = np.concatenate([ROI, np.full((1, 12, 16), 255, dtype=np.uint8)])
    return gt, gt.copy(), dict(roi=roi, roi_cameras=[1, 2, 3]), dict(idtp=4, num_predictions=4, num_objects=8)


def _drop_repeats():
    # (camera 1, id 0, frame 0) twice with different boxes: the first one (which misses the ground truth) decides
    gt = tracks(2, 2, 2)
    pred = gt.copy()
    first = np.array([(1, 0, 0, 900, 900, 40, 30)], dtype=np.int64)
    pred = np.concatenate([first, pred])
    return gt, pred, {}, dict(idtp=7, num_predictions=8, idfp=1, idfn=1)


def _drop_repeats_after_roi():
    # the first of two repeats is an ROI outlier (corner (5, 3) of camera 1 is 254): the second stays
    gt = np.array([(cam, 0, f, 1, 1, 2, 2) for cam in (1, 3) for f in range(2)], dtype=np.int64)
    pred = np.concatenate([np.array([(1, 0, 0, 5, 3, 2, 2)], dtype=np.int64), gt])
    roi = np.concatenate([ROI, np.full((1, 12, 16), 255, dtype=np.uint8)])
    return gt, pred, dict(roi=roi, roi_cameras=[1, 2, 3]), dict(idtp=4, num_predictions=4, idf1=1.0)


def _roi_corners():
    """12 x 16 mask, camera 1: (row 3, column 5) = 254, (row 11, column 15) = 0, everything else 255"""
    boxes = {
        10: (5, 3, 2, 2),        # corner on the 254 pixel: out
        11: (4, 3, 1, 0),        # x + width = 5, y = 3: the right corners hit it: out
        12: (6, 3, 2, 2),        # next to it: stays
        13: (14, 10, 2, 2),      # x + width = 16 = Wr, y + height = 12 = Hr: not looked up; (14, 10) is 255: stays
        14: (15, 11, 4, 4),      # corner on the 0 pixel: out
        15: (-3, -2, 2, 1),      # all corners negative: stays
        16: (-1, 11, 16, 5),     # x = -1 not looked up, x + width = 15 with y = 11: out
        17: (15, 5, 10 ** 12, 1),    # a huge corner is outside the mask; (15, 5), (15, 6) are 255: stays
    }
    rows = [(cam, ident, 0) + box for cam in (1, 3) for ident, box in boxes.items()]
    gt = np.array(rows, dtype=np.int64)
    roi = np.concatenate([ROI, np.full((1, 12, 16), 255, dtype=np.uint8)])
    kept1 = [False, False, True, True, False, True, False, True]
    # (an identity whose camera-1 row went has one camera left, so its camera-3 row goes too)
    return gt, gt.copy(), dict(roi=roi, roi_cameras=[1, 2, 3]), dict(kept=kept1 + kept1, num_predictions=8, idtp=8)


def _roi_254_against_255():
    # the same rows in camera 2 (plane of 254s: every in-mask corner is an outlier) and camera 3 (255s)
    rows = [(cam, ident, 0, 2 + ident, 2, 3, 3) for cam in (2, 3) for ident in range(3)]
    rows += [(1, ident, 0, 2 + ident, 6, 3, 3) for ident in range(3)]
    gt = np.array(rows, dtype=np.int64)
    roi = np.concatenate([ROI, np.full((1, 12, 16), 255, dtype=np.uint8)])
    return gt, gt.copy(), dict(roi=roi, roi_cameras=[1, 2, 3]), dict(kept=[False] * 3 + [True] * 6, idtp=6, num_objects=9)


def _border():
    # W = 200, H = 100, p = 0.1: keep iff 20 <= x + w / 2 <= 180 and 10 <= y + h <= 90, ground truth and predictions alike
    boxes = [(15, 0, 10, 10), (14, 0, 11, 10), (175, 50, 10, 40), (176, 50, 10, 40), (100, 0, 10, 9), (100, 50, 10, 41),
             (50, 20, 20, 20)]
    rows = [(cam, ident, 0) + box for cam in (1, 2) for ident, box in enumerate(boxes)]
    gt = np.array(rows, dtype=np.float64)
    pred = gt.copy()
    pred[6, 3] = 1.0                 # camera 1, id 6: the prediction leaves the band (the ground truth stays), which leaves
    keep = [True, False, True, False, False, False, False]               # predicted id 6 one camera: gone in camera 2 as well
    return gt, pred, dict(border=0.1, image_size=(200, 100)), dict(kept=keep + keep, num_objects=6, num_predictions=4,
                                                                   idtp=4, idfn=2, idfp=0)


def s02_table():
    return np.load(GOLDEN)["s02_gt"].astype(np.int64)


def _s02_identity():
    gt = s02_table()
    return gt, gt.copy(), {}, dict(idf1=1.0, idp=1.0, idr=1.0, idtp=gt.shape[0], idfp=0, idfn=0)


def s02_perturbed(gt):
    """5 % of the rows dropped, boxes jittered by integers, 10 identities merged pairwise, 10 split at mid-sequence"""
    g = np.random.default_rng(2021)
    pred = gt[g.random(gt.shape[0]) >= 0.05].copy()
    pred[:, 3:5] += g.integers(-12, 13, size=(pred.shape[0], 2))
    pred[:, 5:7] = np.maximum(1, pred[:, 5:7] + g.integers(-8, 9, size=(pred.shape[0], 2)))
    ids = g.permutation(np.unique(pred[:, 1]))
    for a, b in zip(ids[:10], ids[10:20]):
        pred[pred[:, 1] == b, 1] = a
    for k, a in enumerate(ids[20:30]):
        rows = np.nonzero(pred[:, 1] == a)[0]
        late = rows[pred[rows, 2] >= np.median(pred[rows, 2])]
        pred[late, 1] = 100000 + k
    return pred


def _s02_perturbed():
    gt = s02_table()
    return gt, s02_perturbed(gt), {}, {}


CASES = {
    "identical": _identical, "merged": _merged, "split": _split,
    "threshold_0.75": lambda: _threshold(0.75), "threshold_0.7499": lambda: _threshold(0.7499),
    "empty_sides": _empty_sides, "big_group_last": lambda: _big_group(False), "big_group_first": lambda: _big_group(True),
    "id_values": _id_values, "fractional": _fractional, "min_cameras": _min_cameras,
    "min_cameras_after_roi": _min_cameras_after_roi, "drop_repeats": _drop_repeats,
    "drop_repeats_after_roi": _drop_repeats_after_roi, "roi_corners": _roi_corners,
    "roi_254_against_255": _roi_254_against_255, "border": _border,
    "s02_identity": _s02_identity, "s02_perturbed": _s02_perturbed,
}
S02_CASES = ("s02_identity", "s02_perturbed")


def case(name):
    return CASES[name]()


_yardstick = {}


def yardstick(name):
    """(the yardstick's Result, the hand values) of a case, computed once and shared by every test that asks"""
    if name not in _yardstick:
        import idf1_ref
        gt, pred, kw, hand = case(name)
        _yardstick[name] = (idf1_ref.idf1(gt, pred, **kw), hand)
    return _yardstick[name]


def check_hand(r, hand, ids=lambda m: m):
    """the hand-derived values against a result (the yardstick's or the library's, `ids` turning its matches into a list)"""
    for key, want in hand.items():
        got = getattr(r, key)
        if key == "kept":
            assert np.asarray(got).tolist() == want
        elif key == "matches":
            assert sorted(map(tuple, ids(got))) == sorted(want)
        else:
            assert got == want, (key, got, want)
