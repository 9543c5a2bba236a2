"""GPU test of `mtmc_mpn.idf1` (IDF1 / IDP / IDR as the reference's eval/eval.py reports them) against the
numpy yardstick of tests/idf1_ref.py on the cases of tests/idf1_cases.py.  IDTP is an integer optimum and every score one
fp64 division of integers, so EVERYTHING is compared with ==: the overlap counts C, the five counts, the three scores,
the row mask, and IDTP once more against the optimum scipy recorded in tests/golden/idf1_cases.npz.

The two S02 cases run the whole fixture (20 956 ground-truth rows): the yardstick takes 0.34 s for the perturbed one on
the MI355X host (`tools/idf1_time.py`) and 2.3 s for all 19 cases where the fixture was written, so the table is not
thinned; either result is computed once and shared."""
import math

import numpy as np
import pytest
import torch

import idf1_cases
from idf1_cases import check_hand, yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_args(gt, pred, kw, dtype=None):
    kw = dict(kw)
    if "roi" in kw:
        kw["roi"] = torch.from_numpy(kw["roi"]).to(DEV)
    to = lambda t: torch.from_numpy(t).to(DEV) if dtype is None else torch.from_numpy(t).to(DEV).to(dtype)   # noqa: E731
    return to(gt), to(pred), kw


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def compare(got, counts, ref):
    c, gt_ids, pred_ids, kept_gt, kept = counts
    assert gt_ids.cpu().tolist() == ref.gt_ids.tolist() and pred_ids.cpu().tolist() == ref.pred_ids.tolist()
    assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), ref.C)
    assert np.array_equal(kept.cpu().numpy(), ref.kept) and np.array_equal(kept_gt.cpu().numpy(), ref.kept_gt)
    assert got.kept.dtype == torch.bool and np.array_equal(got.kept.cpu().numpy(), ref.kept)
    for key in ("idtp", "idfp", "idfn", "num_objects", "num_predictions"):
        assert type(getattr(got, key)) is int and getattr(got, key) == getattr(ref, key), key
    for key in ("idf1", "idp", "idr"):
        assert type(getattr(got, key)) is float and same_float(getattr(got, key), getattr(ref, key)), key
    m = got.matches.cpu()
    assert m.dtype == torch.int64 and m.dim() == 2 and m.shape[1] == 2
    assert len(set(m[:, 0].tolist())) == m.shape[0] == len(set(m[:, 1].tolist()))                # one-to-one
    rows, cols = np.searchsorted(ref.gt_ids, m[:, 0].numpy()), np.searchsorted(ref.pred_ids, m[:, 1].numpy())
    assert (ref.C[rows, cols] > 0).all() and int(ref.C[rows, cols].sum()) == got.idtp         # an optimum of C > 0 pairs


@pytest.mark.parametrize("name", list(idf1_cases.CASES))
def test_case_equals_the_yardstick(name):
    import mtmc_mpn
    gt, pred, kw, hand = idf1_cases.case(name)
    ref, _ = yardstick(name)
    dgt, dpred, dkw = device_args(gt, pred, kw)
    got = mtmc_mpn.idf1(dgt, dpred, **dkw)
    compare(got, mtmc_mpn.metrics.id_overlap_counts(dgt, dpred, **dkw), ref)
    assert [got.idtp, got.idfp, got.idfn] == np.load(idf1_cases.GOLDEN)[name + "/scipy"].tolist()
    check_hand(got._replace(kept=got.kept.cpu().numpy()), hand, ids=lambda m: m.cpu().tolist())


def test_identity_matching_and_all_rows_kept():
    import mtmc_mpn
    gt = torch.from_numpy(idf1_cases.tracks()).to(DEV)
    got = mtmc_mpn.idf1(gt, gt.clone())
    assert got.idf1 == 1.0 and got.idtp == gt.shape[0] == 60 and bool(got.kept.all())
    assert got.matches.cpu().tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]]


@pytest.mark.parametrize("name", ["split", "threshold_0.75", "empty_sides"])
def test_narrow_tables_give_the_same_bits(name):
    """int32 and float32 tables (the values are small integers) give what int64 / float64 give"""
    import mtmc_mpn
    gt, pred, kw, _ = idf1_cases.case(name)
    ref, _ = yardstick(name)
    for dtype in (torch.int32, torch.float32, torch.float64):
        dgt, dpred, dkw = device_args(gt, pred, kw, dtype)
        compare(mtmc_mpn.idf1(dgt, dpred, **dkw), mtmc_mpn.metrics.id_overlap_counts(dgt, dpred, **dkw), ref)


def test_rows_in_any_order_and_strided_tables():
    import mtmc_mpn
    gt, pred, kw, _ = idf1_cases.case("big_group_first")
    ref, _ = yardstick("big_group_first")
    g = np.random.default_rng(1)
    pg, pp = g.permutation(gt.shape[0]), g.permutation(pred.shape[0])
    wide = torch.zeros((pred.shape[0], 9), dtype=torch.int64, device=DEV)
    wide[:, :7] = torch.from_numpy(pred[pp]).to(DEV)
    got = mtmc_mpn.idf1(torch.from_numpy(gt[pg]).to(DEV), wide[:, :7], **kw)
    assert (got.idtp, got.idfp, got.idfn, got.idf1) == (ref.idtp, ref.idfp, ref.idfn, ref.idf1)
    assert np.array_equal(got.kept.cpu().numpy(), ref.kept[pp])


def test_two_calls_give_the_same_bits():
    import mtmc_mpn
    gt, pred, kw = device_args(*idf1_cases.case("big_group_last")[:3])
    a, b = (mtmc_mpn.metrics.id_overlap_counts(gt, pred, **kw) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
    x, y = mtmc_mpn.idf1(gt, pred, **kw), mtmc_mpn.idf1(gt, pred, **kw)
    assert x[:8] == y[:8] and torch.equal(x.matches, y.matches) and torch.equal(x.kept, y.kept)


def test_empty_tables():
    import mtmc_mpn
    gt = torch.from_numpy(idf1_cases.tracks()).to(DEV)
    none = gt[:0]
    got = mtmc_mpn.idf1(gt, none)
    assert (got.idtp, got.idfp, got.idfn, got.num_objects, got.num_predictions) == (0, 0, 60, 60, 0)
    assert got.idf1 == 0.0 and math.isnan(got.idp) and got.idr == 0.0 and got.matches.shape == (0, 2) and got.kept.shape == (0,)
    got = mtmc_mpn.idf1(none, gt)
    assert (got.idtp, got.idfp, got.idfn) == (0, 60, 0) and got.idp == 0.0 and math.isnan(got.idr) and bool(got.kept.all())
    got = mtmc_mpn.idf1(none, none)
    assert got.idtp == 0 and math.isnan(got.idf1)


def test_refusals():
    import mtmc_mpn
    table = idf1_cases.tracks()
    gt = torch.from_numpy(table).to(DEV)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.idf1(gt.cpu(), gt)
    with pytest.raises(ValueError, match=r"\[n, 7\]"):
        mtmc_mpn.idf1(gt[:, :6], gt)
    with pytest.raises(ValueError, match=r"\[n, 7\]"):
        mtmc_mpn.idf1(gt, gt.to(torch.int16))
    # 8193 x 8193 identities are past the cap of 2^26 cells: ids only, one row each, boxes of no size
    many = torch.zeros((8193, 7), dtype=torch.int64, device=DEV)
    many[:, 1] = torch.arange(8193, device=DEV)
    with pytest.raises(ValueError, match="cells"):
        mtmc_mpn.idf1(many, many)
    cams = torch.zeros((65, 7), dtype=torch.int64, device=DEV)
    cams[:, 0] = torch.arange(65, device=DEV)
    with pytest.raises(ValueError, match="65 cameras"):
        mtmc_mpn.idf1(cams, cams)
    roi = torch.full((1, 12, 16), 255, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="no plane"):
        mtmc_mpn.idf1(gt, gt, roi=roi, roi_cameras=[1])                  # cameras 2 and 3 have none
    with pytest.raises(ValueError, match="roi must be"):
        mtmc_mpn.idf1(gt, gt, roi=roi[0], roi_cameras=[1])
    with pytest.raises(ValueError, match="image_size"):
        mtmc_mpn.idf1(gt, gt, border=0.1)


def test_relabel_then_score():
    """postprocess's ID_pred written back into the detections (inference.py:538-551), then the score"""
    import mtmc_mpn
    table = idf1_cases.tracks()
    gt = torch.from_numpy(table).to(DEV)
    node = torch.from_numpy(table[:, 0] * 4 + table[:, 1]).to(DEV)         # one tracklet per (camera, identity)
    id_pred = torch.zeros(16, dtype=torch.int64, device=DEV)
    for cam in (1, 2, 3):
        id_pred[cam * 4:cam * 4 + 4] = torch.tensor([50, 51, 52, 53], device=DEV)     # the clusters, numbered otherwise
    det = gt.clone()
    det[:, 1] = -1
    pred = mtmc_mpn.relabel_detections(det, node, id_pred)
    got = mtmc_mpn.idf1(gt, pred)
    assert got.idf1 == 1.0 and got.matches.cpu().tolist() == [[0, 50], [1, 51], [2, 52], [3, 53]]
