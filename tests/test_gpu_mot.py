"""GPU test of `mtmc_mpn.mot_scores`, `mot_pairs` and `tracking_summary` (the CLEAR MOT columns of the reference's result
row) against the numpy yardstick of tests/mot_ref.py on the cases of tests/mot_cases.py.  The candidate
distance is one fp64 expression without fused multiply-adds, the counts are integers, the distance sum is added in a
defined order and every score is one fp64 division: EVERYTHING is compared with ==, NaN fields by isnan, and the counts
and the sum once more against what the walk gave with scipy's solver (tests/golden/mot_cases.npz).

The yardstick's results are computed once per case and shared (tests/mot_cases.py::yardstick); the two S02 cases run the
whole table, about 1.7 s each on the host."""
import math

import numpy as np
import pytest
import torch

import mot_cases
import mot_ref
from mot_cases import check_hand, same_float, yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INTS = mot_ref.COUNTS
FLOATS = ("mota", "motp", "recall", "precision")


def device_args(gt, pred, kw):
    kw = dict(kw)
    if "roi" in kw:
        kw["roi"] = torch.from_numpy(kw["roi"]).to(DEV)
    return torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV), kw


def compare(got, ref):
    for key in INTS:
        assert type(getattr(got, key)) is int and getattr(got, key) == getattr(ref, key), (key, getattr(got, key), getattr(ref, key))
    for key in FLOATS:
        assert type(getattr(got, key)) is float and same_float(getattr(got, key), getattr(ref, key)), \
            (key, getattr(got, key), getattr(ref, key))
    assert got.matched.dtype == torch.int64 and np.array_equal(got.matched.cpu().numpy(), ref.matched)
    assert got.kept.dtype == torch.bool and np.array_equal(got.kept.cpu().numpy(), ref.kept)


def compare_pairs(got, ref):
    gi, pi, d = (t.cpu().numpy() for t in got)
    assert gi.dtype == np.int64 and pi.dtype == np.int64 and d.dtype == np.float64
    assert list(zip(gi.tolist(), pi.tolist())) == [(i, j) for i, j, _ in ref.pairs]
    assert d.tolist() == [dd for _, _, dd in ref.pairs]                       # the same bits


@pytest.mark.parametrize("name", list(mot_cases.CASES) + list(mot_cases.PAIR_CASES))
def test_pairs_equal_the_yardstick(name):
    """`fractional` and `threshold_0.75` are where a fused multiply-add or a < in place of <= shows; `equal_boxes` has
    6 410 candidates against a first list of 4 096, so the pass runs a second time; the big_group cases cross a workgroup"""
    import mtmc_mpn
    gt, pred, kw, _ = mot_cases.case(name)
    ref, _ = yardstick(name)
    dgt, dpred, dkw = device_args(gt, pred, kw)
    compare_pairs(mtmc_mpn.mot_pairs(dgt, dpred, **dkw), ref)
    if name == "equal_boxes":
        assert len(ref.pairs) == 6410 > max(4096, 4 * (gt.shape[0] + pred.shape[0]))


@pytest.mark.parametrize("name", list(mot_cases.CASES))
def test_scores_equal_the_yardstick_and_the_fixture(name):
    import mtmc_mpn
    gt, pred, kw, hand = mot_cases.case(name)
    ref, _ = yardstick(name)
    dgt, dpred, dkw = device_args(gt, pred, kw)
    got = mtmc_mpn.mot_scores(dgt, dpred, **dkw)
    compare(got, ref)
    golden = np.load(mot_cases.GOLDEN)
    assert [getattr(got, k) for k in INTS] == golden[name + "/counts"].tolist()
    det = got.num_matches + got.num_switches
    assert same_float(got.motp, float(golden[name + "/dist_sum"]) / det if det else float("nan"))
    check_hand(got._replace(matched=got.matched.cpu().numpy()), hand)


@pytest.mark.parametrize("name", ["s02_perturbed", "crowded"])
def test_tracking_summary_is_both_calls(name):
    import mtmc_mpn
    dgt, dpred, dkw = device_args(*mot_cases.case(name)[:3])
    ids, mot = mtmc_mpn.tracking_summary(dgt, dpred, **dkw)
    want_ids, want_mot = mtmc_mpn.idf1(dgt, dpred, **dkw), mtmc_mpn.mot_scores(dgt, dpred, **dkw)
    assert type(ids) is mtmc_mpn.IdScores and type(mot) is mtmc_mpn.MotScores
    assert ids[:8] == want_ids[:8] and torch.equal(ids.matches, want_ids.matches) and torch.equal(ids.kept, want_ids.kept)
    assert all(same_float(a, b) for a, b in zip(mot[:4], want_mot[:4])) and mot[4:16] == want_mot[4:16]
    assert torch.equal(mot.matched, want_mot.matched) and torch.equal(mot.kept, want_mot.kept)
    assert (ids.num_objects, ids.num_predictions) == (mot.num_objects, mot.num_predictions)


def test_two_calls_give_the_same_bits():
    import mtmc_mpn
    dgt, dpred, dkw = device_args(*mot_cases.case("crowded")[:3])
    x, y = mtmc_mpn.mot_scores(dgt, dpred, **dkw), mtmc_mpn.mot_scores(dgt, dpred, **dkw)
    assert x[:16] == y[:16] and torch.equal(x.matched, y.matched) and torch.equal(x.kept, y.kept)
    a, b = mtmc_mpn.mot_pairs(dgt, dpred, **dkw), mtmc_mpn.mot_pairs(dgt, dpred, **dkw)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


def shuffled(table, g):
    """a random order of the rows in which rows of equal (camera, id, frame) keep their relative order: `drop_repeats`
    keeps the FIRST of them, by definition"""
    perm = g.permutation(table.shape[0])
    places = {}
    for at, row in enumerate(perm):
        places.setdefault(tuple(table[row, :3].tolist()), []).append(at)
    for at in places.values():
        perm[at] = np.sort(perm[at])
    return perm


@pytest.mark.parametrize("name", [n for n in mot_cases.CASES if n not in mot_cases.ORDER_DEPENDENT])
def test_rows_in_any_order_give_the_same_scores(name):
    """(the continuity-order cases depend on the input order by definition and are left out)"""
    import mtmc_mpn
    gt, pred, kw, _ = mot_cases.case(name)
    ref, _ = yardstick(name)
    g = np.random.default_rng(31)
    pg, pp = shuffled(gt, g), shuffled(pred, g)
    dgt, dpred, dkw = device_args(np.ascontiguousarray(gt[pg]), np.ascontiguousarray(pred[pp]), kw)
    got = mtmc_mpn.mot_scores(dgt, dpred, **dkw)
    for key in INTS:
        assert getattr(got, key) == getattr(ref, key), key
    for key in FLOATS:
        assert same_float(getattr(got, key), getattr(ref, key)), key
    # the same pairs, named by the rows' new places
    inv = np.empty(pred.shape[0], dtype=np.int64)
    inv[pp] = np.arange(pred.shape[0])
    want = np.where(ref.matched[pg] >= 0, inv[np.maximum(ref.matched[pg], 0)] if pred.shape[0] else ref.matched[pg], ref.matched[pg])
    assert np.array_equal(got.matched.cpu().numpy(), want) and np.array_equal(got.kept.cpu().numpy(), ref.kept[pp])


def test_narrow_and_strided_tables():
    import mtmc_mpn
    gt, pred, kw, _ = mot_cases.case("continuity_keeps")
    ref, _ = yardstick("continuity_keeps")
    for dtype in (torch.int32, torch.float32, torch.float64):
        wide = torch.zeros((pred.shape[0], 9), dtype=dtype, device=DEV)
        wide[:, :7] = torch.from_numpy(pred).to(DEV).to(dtype)
        compare(mtmc_mpn.mot_scores(torch.from_numpy(gt).to(DEV).to(dtype), wide[:, :7], **kw), ref)


def test_refusals():
    import mtmc_mpn
    gt = torch.from_numpy(mot_cases.case("identical")[0]).to(DEV)
    for fn in (mtmc_mpn.mot_scores, mtmc_mpn.mot_pairs, mtmc_mpn.tracking_summary):
        with pytest.raises(ValueError, match=f"mtmc_mpn.{fn.__name__}: drop_repeats must be True"):
            fn(gt, gt, drop_repeats=False)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            fn(gt.cpu(), gt)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            fn(gt, gt.cpu())
        with pytest.raises(ValueError, match=rf"mtmc_mpn.{fn.__name__}: pred must be an \[n, 7\]"):
            fn(gt, gt[:, :6])
        with pytest.raises(ValueError, match="image_size"):
            fn(gt, gt, border=0.1)
    assert math.isnan(mtmc_mpn.mot_scores(gt[:0], gt[:0]).mota)
