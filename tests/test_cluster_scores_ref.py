"""CPU: the yardstick of the cluster-score tests (cluster_scores_ref) against scikit-learn's recorded values, the host-only
size query, the bindings and the refusals of `mtmc_mpn.cluster_scores` / `edge_prf` / `evaluate`.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cluster_scores_ref as ref
from abi_refusal import refused
from cs_cases import cpu_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtmc_cluster_scores_workspace_bytes", "mtmc_cluster_scores", "mtmc_edge_prf"]
FIVE = ref.NAMES[:5]
BAR = 1e-9


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cs_cases.npz"))


@pytest.fixture(scope="module")
def computed(golden):
    """the reference's answer for every case of the fixture, computed once"""
    return {str(name): ref.cluster_scores_ref(golden[f"{name}/true"], golden[f"{name}/pred"]) for name in golden["names"]}


def test_fixture_holds_the_case_list(golden):
    cases = cpu_cases()
    assert [str(n) for n in golden["names"]] == list(cases)
    for name, (t, p) in cases.items():
        assert np.array_equal(golden[f"{name}/true"], t) and np.array_equal(golden[f"{name}/pred"], p), name
    assert len(cases) >= 25


def test_reference_is_within_the_bar_of_the_recorded_scikit_learn_values(golden, computed):
    worst = dict.fromkeys(FIVE, 0.0)
    for name, (scores, _counts) in computed.items():
        want = golden[f"{name}/sklearn"]
        for k, key in enumerate(FIVE):
            worst[key] = max(worst[key], abs(scores[key] - float(want[k])))
            assert abs(scores[key] - float(want[k])) <= BAR, (name, key, scores[key], float(want[k]))
    print("largest |reference - scikit-learn|:", worst)


def test_reference_is_within_the_bar_of_scikit_learn_itself(golden, computed):
    metrics = pytest.importorskip("sklearn.metrics")
    fns = (metrics.adjusted_rand_score, metrics.adjusted_mutual_info_score, metrics.homogeneity_score,
           metrics.completeness_score, metrics.v_measure_score)
    for name, (scores, _counts) in computed.items():
        t, p = golden[f"{name}/true"], golden[f"{name}/pred"]
        for key, fn in zip(FIVE, fns):
            assert abs(scores[key] - float(fn(t, p))) <= BAR, (name, key)


def test_reference_special_cases_are_exact(computed):
    s, c = computed["n1"]
    assert [s[k] for k in FIVE] == [1.0] * 5 and c == [1, 1, 1, 0, 0, 0, 0]
    s, c = computed["one_cluster_both"]
    assert [s[k] for k in FIVE] == [1.0] * 5 and s["entropy_true"] == 0.0 and s["mi"] == 0.0 and c[:3] == [1, 1, 1]
    s, c = computed["one_vs_singletons"]
    assert (s["ari"], s["ami"], s["homogeneity"], s["completeness"], s["v_measure"]) == (0.0, 0.0, 1.0, 0.0, 0.0)
    s, c = computed["singletons_vs_one"]
    assert (s["ari"], s["ami"], s["homogeneity"], s["completeness"], s["v_measure"]) == (0.0, 0.0, 0.0, 1.0, 0.0)
    s, c = computed["two_swapped"]
    assert s["ari"] == 1.0 and abs(s["ami"] - 1.0) <= 1e-15 and c[:3] == [2, 2, 2]
    s, c = computed["independent_2x2"]
    assert s["ari"] == -0.5 and s["mi"] == 0.0 and c == [2, 2, 4, 0, 4, 4, 4]
    s, c = computed["values_extreme"]
    assert (s, c) == computed["values_compact"]                     # the scores see the partition, not the label values


def test_size_histogram_emi_equals_the_sum_over_all_cluster_pairs(golden):
    for name in ("emi_lower_bound", "edge_n65", "random_100_50_2", "random_777_120_4"):
        a, b, _ = ref.contingency(golden[f"{name}/true"], golden[f"{name}/pred"])
        n = sum(a)
        assert abs(ref.emi_sizes(a, b, n) - ref.emi_full(a, b, n)) <= 1e-12, name
    a, b, _ = ref.contingency(golden["emi_lower_bound/true"], golden["emi_lower_bound/pred"])
    assert sorted(a) == [3, 7] and sorted(b) == [2, 8]               # 7 + 8 - 10 = 5: the n_ij sum starts above 1


def test_edge_prf_reference():
    counts, out = ref.edge_prf_ref([1, 1, 0, 0, 1, 0, 1], [1, 0, 0, 1, 1, -100, 0])
    assert counts == [2, 2, 1, 1]
    assert out == [0.5, 2 / 3, 2 * (0.5 * (2 / 3)) / (0.5 + 2 / 3), 1 / 3 * 100.0, 2 / 3 * 100.0]
    assert ref.edge_prf_ref([], []) == ([0, 0, 0, 0], [0.0] * 5)
    assert ref.edge_prf_ref([0, 0], [1, 0]) == ([0, 0, 1, 1], [0.0, 0.0, 0.0, 100.0, 0.0])


def test_entry_points_are_declared_and_bound():
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert "#define MTMC_MPN_ABI_VERSION 6" in header                 # additive: the ABI version stays
    assert "#define MTMC_CLUSTER_SCORES 9" in header and _lib.CLUSTER_SCORES == 9 and _lib.CLUSTER_COUNTS == 7
    lib = _lib.load()
    assert len(lib.mtmc_cluster_scores.argtypes) == 10 and len(lib.mtmc_edge_prf.argtypes) == 8


def test_workspace_query_is_host_only_monotonic_and_linear():
    from mtmc_mpn import _lib
    q = _lib.load().mtmc_cluster_scores_workspace_bytes
    sizes = [q(n) for n in (1, 64, 450, 46000, 1048576)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    for n, s in zip((1, 64, 450, 46000, 1048576), sizes):
        assert s <= 256 * n + 64 * 1024, (n, s)
    assert q(0) == 0 and q(-5) == 0 and q(1048577) == 0


def test_c_entry_points_refuse_before_any_launch():
    """MTMC_E_ARG, checked with NULL / host values only (every check precedes the first launch); each refusal names its
    entry point in mtmc_mpn_last_error()"""
    from mtmc_mpn import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    need = lib.mtmc_cluster_scores_workspace_bytes(10)

    def cs(t=p, st=1, pr=p, sp=1, n=10, scores=p, counts=p, ws=p, nbytes=need):
        return lib.mtmc_cluster_scores(t, st, pr, sp, n, scores, counts, ws, nbytes, None)
    for bad in (dict(n=0), dict(n=-1), dict(n=1048577), dict(t=None), dict(pr=None), dict(scores=None), dict(counts=None),
                dict(ws=None), dict(ws=p + 4), dict(nbytes=need - 1), dict(st=-1), dict(sp=-2)):
        assert refused(lib, lambda: cs(**bad), _lib.E_ARG, "cluster_scores"), bad

    def prf(y=p, sy=1, x=p, sx=1, e=10, counts=p, out=p):
        return lib.mtmc_edge_prf(y, sy, x, sx, e, counts, out, None)
    for bad in (dict(e=-1), dict(y=None), dict(x=None), dict(counts=None), dict(out=None), dict(sy=-1), dict(sx=-1)):
        assert refused(lib, lambda: prf(**bad), _lib.E_ARG, "edge_prf"), bad


def test_python_surface_refuses():
    import mtmc_mpn
    a = torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mtmc_mpn.cluster_scores(a, a)
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(a, torch.zeros(5, dtype=torch.long))                     # unequal lengths
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(a[:0], a[:0])                                            # n = 0
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(torch.zeros(1048577, dtype=torch.int8), torch.zeros(1048577, dtype=torch.int8))
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(a.float(), a)                                            # labels are integers
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(a.view(2, 2), a.view(2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mtmc_mpn.edge_prf(a, a.float())
    with pytest.raises(ValueError):
        mtmc_mpn.edge_prf(a, torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mtmc_mpn.evaluate(a, a, torch.zeros((2, 4), dtype=torch.long), a.float(), 4)
    for name in ("cluster_scores", "edge_prf", "evaluate", "ClusterScores", "EdgePRF"):
        assert getattr(mtmc_mpn, name) is getattr(mtmc_mpn.metrics, name) and name in mtmc_mpn.__all__
    assert mtmc_mpn.ClusterScores._fields == ref.NAMES + ("counts",)
    assert mtmc_mpn.EdgePRF._fields == ("confusion", "precision", "recall", "f_score", "class_precision")
