"""CPU test of the CLEAR MOT yardstick (tests/mot_ref.py) that the walk test and the GPU test hold the
library to: on every case of tests/mot_cases.py it gives the values derived by hand and, with ==, the counts and the
distance sum that the same walk gave with scipy's linear_sum_assignment as the solver when tests/golden/mot_cases.npz was
written.  The yardstick asserts the condition on the inputs while it runs (a unique optimum wherever the assignment has a
choice); that the assertion bites is checked here."""
import math

import numpy as np
import pytest

import mot_cases
import mot_ref
from mot_cases import check_hand, yardstick


@pytest.mark.parametrize("name", list(mot_cases.CASES))
def test_yardstick_equals_the_fixture_and_hand_values(name):
    golden = np.load(mot_cases.GOLDEN)
    assert name in golden["names"].tolist() and golden["fields"].tolist() == mot_ref.COUNTS
    r, hand = yardstick(name)                           # (asserts the uniqueness condition group by group)
    assert [getattr(r, k) for k in mot_ref.COUNTS] == golden[name + "/counts"].tolist()
    assert r.dist_sum == float(golden[name + "/dist_sum"])
    check_hand(r, hand)
    det = r.num_matches + r.num_switches
    assert det + r.num_misses == r.num_objects and det + r.num_false_positives == r.num_predictions
    assert r.mostly_tracked + r.partially_tracked + r.mostly_lost == r.num_unique_objects
    assert int((r.matched >= 0).sum()) == det and int((r.matched == -2).sum()) == int((~r.kept_gt).sum())
    assert mot_cases.same_float(r.motp, r.dist_sum / det if det else float("nan"))


def test_the_fixture_holds_numbers_only():
    golden = np.load(mot_cases.GOLDEN)
    want = {"scipy_version", "names", "fields"}
    for name in mot_cases.CASES:
        want |= {name + "/counts", name + "/dist_sum"}
        assert golden[name + "/counts"].dtype == np.int64 and golden[name + "/counts"].shape == (len(mot_ref.COUNTS),)
        assert golden[name + "/dist_sum"].dtype == np.float64 and golden[name + "/dist_sum"].shape == ()
    assert set(golden.files) == want


def test_what_the_issue_records_of_the_named_cases():
    r, _ = yardstick("s02_perturbed")
    assert (r.num_matches, r.num_switches, r.num_false_positives, r.num_misses, r.num_fragmentations) == (19847, 33, 0, 1076, 955)
    assert (r.mostly_tracked, r.partially_tracked, r.mostly_lost, r.num_frames) == (144, 1, 0, 7435)
    for name in mot_cases.CROSSING_A_WORKGROUP:
        r, _ = yardstick(name)
        assert (r.num_matches, r.num_false_positives) == (270, 160) and r.motp > 0 and len(r.pairs) > 270
    r, _ = yardstick("crowded")
    assert r.num_switches == 2 and r.num_false_positives == 0 and r.num_frames == 60 and r.solver_groups >= 1
    r, _ = yardstick("s02_identity")
    assert (r.num_matches, r.mota, r.motp, r.recall, r.precision) == (20956, 1.0, 0.0, 1.0, 1.0)


def test_continuity_changes_what_a_plain_assignment_gives():
    keeps, alone = yardstick("continuity_keeps")[0], yardstick("continuity_keeps_alone")[0]
    assert keeps.matched.tolist()[2:] == [2, 3] and alone.matched.tolist() == [1, 0]
    a, b = yardstick("continuity_order")[0], yardstick("continuity_order_swapped")[0]
    assert a.motp != b.motp and a.num_fragmentations != b.num_fragmentations


def test_distance_and_solver():
    assert mot_ref.distance((0, 0, 10, 10), (0, 6, 10, 10)) == 0.75 and math.isnan(mot_ref.distance((5, 5, 0, 0), (5, 5, 0, 0)))
    nan = np.nan
    assert mot_ref.solve(np.array([[0.5, 0.1], [0.2, nan]])) == [(0, 1), (1, 0)]
    assert mot_ref.solve(np.array([[0.1, nan], [0.2, nan]])) == [(0, 0)]                         # one column: one pair
    assert mot_ref.solve(np.array([[0.0, 0.7, nan], [nan, 0.1, 0.6]])) == [(0, 0), (1, 1)]
    # the most pairs first: (0, 0) alone would be cheaper than (0, 1) + (1, 0)
    assert mot_ref.solve(np.array([[0.0, 0.7], [0.7, nan]])) == [(0, 1), (1, 0)]
    assert mot_ref.solve(np.full((2, 3), nan)) == []
    g = np.random.default_rng(12)
    for _ in range(30):                                                                          # against brute force
        import itertools
        n, m = g.integers(1, 5, size=2)
        d = np.where(g.random((n, m)) < 0.6, g.random((n, m)), nan)
        best = None
        for k in range(min(n, m), -1, -1):
            sums = [sum(d[i, j] for i, j in zip(rr, cc)) for rr in itertools.combinations(range(n), k)
                    for cc in itertools.permutations(range(m), k)]
            sums = [s for s in sums if not np.isnan(s)]
            if sums:
                best = (k, min(sums))
                break
        got = mot_ref.solve(d)
        assert len(got) == best[0] and abs(mot_ref.pair_sum(d, got) - best[1]) < 1e-12


def test_the_uniqueness_condition_bites():
    """two equal boxes against two equal predictions: either assignment is an optimum, which the yardstick refuses"""
    gt = mot_cases.rows((1, 0, 0, 0), (1, 1, 0, 0))
    with pytest.raises(AssertionError, match="not unique"):
        mot_ref.mot_scores(gt, gt.copy(), min_cameras=1)
    r = mot_ref.mot_scores(gt, gt.copy(), min_cameras=1, check_unique=False)                    # (the pair list needs none)
    assert len(r.pairs) == 4 and r.num_matches == 2
    gt, pred, kw, _ = mot_cases.case("equal_boxes")                                             # hence: pair list alone
    with pytest.raises(AssertionError, match="not unique"):
        mot_ref.mot_scores(gt, pred, **kw)
