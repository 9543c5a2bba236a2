"""CPU test of `mtmc_mot_walk` through ctypes: the host half of the CLEAR MOT scores -- the correspondence
walk over the sorted candidates, its assignment per connected component -- fed with the yardstick's candidate list
(tests/mot_ref.py) on every case of tests/mot_cases.py and compared with ==: the counts, the matched rows, the distance sum
(also against the scipy fixture).  The entry point touches no GPU."""
import ctypes
import time

import numpy as np
import pytest

import mot_cases
import mot_ref
from mot_cases import yardstick


def grouped(gt, pred, kept_gt, kept):
    """The two tables as the library's Python layer groups them, in numpy: per side the stable order by ((camera, frame)
    group, identity), the group number, the compact identity and the keep byte of every row in that order."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    keys = np.concatenate([gt[:, :3], pred[:, :3]]).astype(np.int64)
    _, cam_inv = np.unique(keys[:, 0], return_inverse=True)
    frames, frame_inv = np.unique(keys[:, 2], return_inverse=True)
    groups, group_inv = np.unique(cam_inv * max(len(frames), 1) + frame_inv, return_inverse=True)
    out = {"n_groups": len(groups)}
    for name, table, group, keep in (("gt", gt, group_inv[:len(gt)], kept_gt), ("pred", pred, group_inv[len(gt):], kept)):
        ids, ident = np.unique(table[:, 1].astype(np.int64), return_inverse=True)
        perm = np.lexsort((np.arange(len(table)), ident, group))
        rank = np.empty(len(table), dtype=np.int64)
        rank[perm] = np.arange(len(table))
        out[name] = dict(perm=perm.astype(np.int64), rank=rank, n_ident=len(ids), group=group[perm].astype(np.int32),
                         ident=ident[perm].astype(np.int32), keep=np.asarray(keep)[perm].astype(np.uint8))
    return out


def sorted_pairs(g, pairs):
    """the yardstick's (ground-truth input row, prediction input row, d) as the library's sorted candidate list"""
    rows = np.array([(g["gt"]["group"][g["gt"]["rank"][i]], g["gt"]["rank"][i], g["pred"]["rank"][j]) for i, j, _ in pairs],
                    dtype=np.int32).reshape(-1, 3)
    dist = np.array([d for _, _, d in pairs], dtype=np.float64)
    order = np.lexsort((rows[:, 2], rows[:, 1]))
    return np.ascontiguousarray(rows[order]), np.ascontiguousarray(dist[order])


def walk(g, pairs, dist, gt_keep=True, position=None):
    """(rc, counts, dist_sum, match_of_row, stats) of one call"""
    from mtmc_mpn import _lib
    lib = _lib.load()
    a, b = g["gt"], g["pred"]
    at = lambda x: x.ctypes.data if x is not None and x.size else None                            # noqa: E731
    pairs, dist = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 3), np.ascontiguousarray(dist, dtype=np.float64)
    position = a["perm"] if position is None else position
    counts, total = np.full(_lib.MOT_COUNTS, -1, dtype=np.int64), ctypes.c_double(-1.0)
    match, stats = np.full(max(len(a["perm"]), 1), -9, dtype=np.int32), np.full(3, -1, dtype=np.int64)
    rc = lib.mtmc_mot_walk(at(pairs), at(dist), len(pairs), at(a["group"]), at(a["ident"]), at(position),
                           at(a["keep"]) if gt_keep else None, len(a["perm"]), at(b["group"]), at(b["ident"]), at(b["keep"]),
                           len(b["perm"]), g["n_groups"], a["n_ident"], b["n_ident"], counts.ctypes.data, ctypes.addressof(total),
                           match.ctypes.data, stats.ctypes.data)
    return rc, counts.tolist(), float(total.value), match[:len(a["perm"])], stats.tolist()


def matched_in_input_order(g, match):
    out = np.empty(len(match), dtype=np.int64)
    out[g["gt"]["perm"]] = np.where(match >= 0, g["pred"]["perm"][np.maximum(match, 0)] if len(g["pred"]["perm"]) else match, match)
    return out


@pytest.mark.parametrize("name", list(mot_cases.CASES))
def test_case_equals_the_yardstick(name):
    gt, pred, _, _ = mot_cases.case(name)
    ref, _ = yardstick(name)
    g = grouped(gt, pred, ref.kept_gt, ref.kept)
    pairs, dist = sorted_pairs(g, ref.pairs)
    rc, counts, total, match, stats = walk(g, pairs, dist)
    assert rc == 0
    assert counts == [getattr(ref, k) for k in mot_ref.COUNTS] == np.load(mot_cases.GOLDEN)[name + "/counts"].tolist()
    assert total == ref.dist_sum == float(np.load(mot_cases.GOLDEN)[name + "/dist_sum"])
    assert np.array_equal(matched_in_input_order(g, match), ref.matched)
    # the groups that needed a solver are the yardstick's; it solves a whole group, the library one component at a time
    assert stats[0] == ref.solver_groups and stats[1] * stats[2] <= ref.largest[0] * ref.largest[1]


def test_solver_statistics():
    ref, _ = yardstick("continuity_keeps_alone")
    gt, pred, _, _ = mot_cases.case("continuity_keeps_alone")
    g = grouped(gt, pred, ref.kept_gt, ref.kept)
    assert walk(g, *sorted_pairs(g, ref.pairs))[4] == [1, 2, 2]
    ref, _ = yardstick("continuity_keeps")                                   # continuity takes both rows: nothing to solve
    gt, pred, _, _ = mot_cases.case("continuity_keeps")
    g = grouped(gt, pred, ref.kept_gt, ref.kept)
    assert walk(g, *sorted_pairs(g, ref.pairs))[4] == [0, 0, 0]
    ref, _ = yardstick("s02_perturbed")
    gt, pred, _, _ = mot_cases.case("s02_perturbed")
    g = grouped(gt, pred, ref.kept_gt, ref.kept)
    stats = walk(g, *sorted_pairs(g, ref.pairs))[4]
    assert stats[0] <= 3 and stats[1] * stats[2] <= 81                        # of 7 435 groups


def one_group(d):
    """tables of one (camera, frame) with d [n, m] as its candidate matrix (NaN: none): boxes do not matter to the walk"""
    n, m = d.shape
    gt = np.array([(1, i, 0, 0, 0, 1, 1) for i in range(n)], dtype=np.int64).reshape(-1, 7)
    pred = np.array([(1, j, 0, 0, 0, 1, 1) for j in range(m)], dtype=np.int64).reshape(-1, 7)
    g = grouped(gt, pred, np.ones(n, dtype=bool), np.ones(m, dtype=bool))
    pairs = [(i, j, float(d[i, j])) for i in range(n) for j in range(m) if not np.isnan(d[i, j])]
    return g, pairs


def test_small_random_groups_against_the_yardstick_solver():
    g_ = np.random.default_rng(21)
    for _ in range(60):
        n, m = g_.integers(1, 7, size=2)
        d = np.where(g_.random((n, m)) < 0.5, g_.random((n, m)), np.nan)
        want = mot_ref.solve(d)
        g, pairs = one_group(d)
        rc, counts, total, match, _ = walk(g, *sorted_pairs(g, pairs))
        assert rc == 0 and counts[0] == len(want) and counts[1] == 0
        got = [(i, int(match[i])) for i in range(n) if match[i] >= 0]
        assert abs(mot_ref.pair_sum(d, got) - mot_ref.pair_sum(d, want)) < 1e-12 and all(not np.isnan(d[i, j]) for i, j in got)
        assert counts[2] == n - len(want) and counts[3] == m - len(want)


def test_one_component_of_60_by_60_against_the_yardstick():
    g_ = np.random.default_rng(22)
    d = np.where(g_.random((60, 60)) < 0.3, g_.random((60, 60)), np.nan)
    want = mot_ref.solve(d)
    mot_ref.assert_unique(d, want, mot_ref.solve, "60 x 60")
    g, pairs = one_group(d)
    rc, counts, total, match, stats = walk(g, *sorted_pairs(g, pairs))
    assert rc == 0 and stats == [1, 60, 60]
    assert [(i, int(match[i])) for i in range(60) if match[i] >= 0] == want
    assert total == sum(d[i, j] for i, j in want)                            # (added in the order of the ground-truth rows)


def test_2000_groups_of_2_by_2_return_at_once():
    g_ = np.random.default_rng(23)
    n = 2000
    gt = np.array([(1, i, f, 0, 0, 1, 1) for f in range(n) for i in (0, 1)], dtype=np.int64)
    pred = gt.copy()
    pred[:, 1] += 10 * (pred[:, 2] % 7)                                       # other predicted ids every frame: no continuity
    g = grouped(gt, pred, np.ones(2 * n, dtype=bool), np.ones(2 * n, dtype=bool))
    d = g_.random((n, 2, 2))
    pairs = [(2 * f + i, 2 * f + j, float(d[f, i, j])) for f in range(n) for i in (0, 1) for j in (0, 1)]
    t0 = time.perf_counter()
    rc, counts, total, match, stats = walk(g, *sorted_pairs(g, pairs))
    took = time.perf_counter() - t0
    straight = d[:, 0, 0] + d[:, 1, 1] <= d[:, 0, 1] + d[:, 1, 0]
    assert rc == 0 and counts[0] + counts[1] == 2 * n and counts[2] == counts[3] == 0 and stats == [n, 2, 2]
    assert np.array_equal(match.reshape(n, 2)[:, 0] % 2 == 0, straight)
    assert took < 0.5, took                                                   # (a few milliseconds; a per-frame dense solve of 4 000 rows would not)


def test_ground_truth_keep_bytes_and_positions():
    """a ground-truth row that is not kept is -2 and counts for nothing; NULL keep bytes mean all kept"""
    gt, pred, kw, hand = mot_cases.case("border")
    ref, _ = yardstick("border")
    assert not ref.kept_gt.all()
    g = grouped(gt, pred, ref.kept_gt, ref.kept)
    rc, counts, _, match, _ = walk(g, *sorted_pairs(g, ref.pairs))
    assert rc == 0 and sorted(set(matched_in_input_order(g, match)[~ref.kept_gt].tolist())) == [-2]
    rc, counts_all, _, match, _ = walk(g, *sorted_pairs(g, ref.pairs), gt_keep=False)
    assert rc == 0 and counts_all[9] == len(gt) and (match != -2).all()


def test_refusals_and_their_text():
    from mtmc_mpn import _lib
    lib = _lib.load()
    err = lambda: lib.mtmc_mpn_last_error().decode()                           # noqa: E731
    gt, pred, _, _ = mot_cases.case("continuity_keeps")
    ref, _ = yardstick("continuity_keeps")
    g = grouped(gt, pred, ref.kept_gt, ref.kept)
    pairs, dist = sorted_pairs(g, ref.pairs)
    assert walk(g, pairs, dist)[0] == 0
    assert walk(g, pairs[::-1], dist[::-1])[0] == _lib.E_ARG and "mot_walk: candidate" in err() and "not sorted" in err()
    twice = np.concatenate([pairs[:1], pairs])
    assert walk(g, twice, np.concatenate([dist[:1], dist]))[0] == _lib.E_ARG and "listed twice" in err()
    for row, col in ((len(gt), 0), (-1, 0), (0, len(pred)), (0, -1)):
        bad = pairs.copy()
        bad[-1, 1:] = (row, col)
        assert walk(g, bad, dist)[0] == _lib.E_ARG and "names a row outside" in err(), (row, col)
    across = pairs.copy()
    across[0, 2] = pairs[-1, 2]                                               # a prediction row of the other frame
    assert walk(g, across, dist)[0] == _lib.E_ARG and "two groups" in err()
    nan = dist.copy()
    nan[0] = np.nan
    assert walk(g, pairs, nan)[0] == _lib.E_ARG and "NaN" in err()
    # a predicted id twice inside one group: what drop_repeats=False could leave
    repeated = pred.copy()
    repeated[3, 1] = repeated[2, 1]
    g2 = grouped(gt, repeated, ref.kept_gt, ref.kept)
    assert walk(g2, np.zeros((0, 3)), np.zeros(0))[0] == _lib.E_ARG
    assert "mot_walk: predicted identity 0 is kept twice in group 1" in err() and "drop_repeats" in err()
    g2["pred"]["keep"][3] = 0                                                 # ... and fine once the repeat is dropped
    assert walk(g2, np.zeros((0, 3)), np.zeros(0))[0] == 0
    unsorted = grouped(gt, pred, ref.kept_gt, ref.kept)
    unsorted["gt"]["group"] = unsorted["gt"]["group"][::-1].copy()
    assert walk(unsorted, np.zeros((0, 3)), np.zeros(0))[0] == _lib.E_ARG and "ground truth: rows are not sorted" in err()
    counts = np.zeros(_lib.MOT_COUNTS, dtype=np.int64)
    total = ctypes.c_double(0)
    assert lib.mtmc_mot_walk(None, None, 1, None, None, None, None, 0, None, None, None, 0, 0, 0, 0, counts.ctypes.data,
                             ctypes.addressof(total), None, None) == _lib.E_ARG and "mot_walk: NULL" in err()
    assert lib.mtmc_mot_walk(None, None, 0, None, None, None, None, 0, None, None, None, 0, 0, 0, 0, None, None, None,
                             None) == _lib.E_ARG and "mot_walk: NULL" in err()
    assert lib.mtmc_mot_walk(None, None, 0, None, None, None, None, 2 ** 31, None, None, None, 0, 0, 0, 0, counts.ctypes.data,
                             ctypes.addressof(total), None, None) == _lib.E_ARG and "2^31" in err()
    assert lib.mtmc_mot_walk(None, None, 0, None, None, None, None, 0, None, None, None, 0, 0, 0, 0, counts.ctypes.data,
                             ctypes.addressof(total), None, None) == 0 and counts.tolist() == [0] * _lib.MOT_COUNTS
    # the device entry refuses the same sizes before it touches a GPU
    assert lib.mtmc_mot_pairs_workspace_bytes(2 ** 31) == 0 and lib.mtmc_mot_pairs_workspace_bytes(-1) == 0
    assert lib.mtmc_mot_pairs_workspace_bytes(10) >= 88
    assert lib.mtmc_mot_pairs(None, None, None, 2 ** 31, None, None, None, 0, 0, 0.75, None, None, 0, None, None, 0, None) == _lib.E_ARG
    assert "mot_pairs: n_gt, n_pred and n_groups must be in [0, 2^31)" in err()
    assert lib.mtmc_mot_pairs(None, None, None, 0, None, None, None, 0, 0, 0.75, None, None, 0, None, None, 0, None) == _lib.E_ARG
    assert "mot_pairs: NULL" in err()
