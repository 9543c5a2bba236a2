"""CPU test of the IDF1 yardstick (tests/idf1_ref.py) that the GPU test holds `mtmc_mpn.idf1` to: on every case of
tests/idf1_cases.py it gives the optimum scipy's linear_sum_assignment found when tests/golden/idf1_cases.npz was written,
and the values derived by hand.  `relabel_detections` is plain torch and is checked here on CPU tensors (it is NOT
refused on the CPU: it runs no kernel)."""
import math

import numpy as np
import pytest
import torch

import idf1_cases
import idf1_ref

from idf1_cases import check_hand, yardstick


@pytest.mark.parametrize("name", list(idf1_cases.CASES))
def test_yardstick_equals_scipy_and_hand_values(name):
    golden = np.load(idf1_cases.GOLDEN)
    assert name in golden["names"].tolist()
    r, hand = yardstick(name)
    assert [r.idtp, r.idfp, r.idfn] == golden[name + "/scipy"].tolist()
    assert r.idfn == r.num_objects - r.idtp and r.idfp == r.num_predictions - r.idtp
    assert r.idtp == sum(int(r.C[np.searchsorted(r.gt_ids, o), np.searchsorted(r.pred_ids, h)]) for o, h in r.matches)
    check_hand(r, hand)


def test_the_fixture_holds_the_table_and_nothing_else():
    golden = np.load(idf1_cases.GOLDEN)
    t = golden["s02_gt"]
    assert t.shape == (20956, 7) and t.dtype == np.int32
    assert len({tuple(r) for r in t[:, :3].tolist()}) == t.shape[0]          # the precondition: unique (camera, id, frame)
    assert set(golden.files) == {"s02_gt", "scipy_version", "names"} | {n + "/scipy" for n in idf1_cases.CASES}


def test_threshold_pair_is_exactly_on_it():
    a, b = (0, 0, 10, 10), (0, 6, 10, 10)
    assert idf1_ref.pair_counts(a, b, 0.75) and not idf1_ref.pair_counts(a, b, 0.7499)
    assert not idf1_ref.pair_counts((5, 5, 0, 0), (5, 5, 0, 0), 0.75)        # U = 0: NaN never counts
    assert not idf1_ref.pair_counts((0, 0, 10, 10), (20, 20, 10, 10), 0.75)


def test_scores_of_nothing_are_nan():
    empty = np.zeros((0, 7), dtype=np.int64)
    r = idf1_ref.idf1(empty, empty)
    assert math.isnan(r.idf1) and math.isnan(r.idp) and math.isnan(r.idr) and r.idtp == 0


def test_component_stats():
    c = np.zeros((5, 6), dtype=np.int32)
    c[0, 0] = c[0, 1] = c[1, 1] = 1                     # rows 0-1 x columns 0-1
    c[3, 4] = 2                                        # 1 x 1
    c[4, 2] = c[4, 3] = c[4, 5] = 1                    # 1 x 3
    assert idf1_ref.component_stats(c) == (3, 2, 2)
    assert idf1_ref.component_stats(np.zeros((3, 3), dtype=np.int32)) == (0, 0, 0)


def test_relabel_detections_on_cpu_tensors():
    import mtmc_mpn
    table = torch.tensor([[1, -1, 0, 5, 5, 10, 10], [2, -1, 0, 6, 5, 10, 10], [1, -1, 1, 7, 5, 10, 10]], dtype=torch.int64)
    index = torch.tensor([0, 1, 0])                     # the node (tracklet) of each detection
    id_pred = torch.tensor([42, 7])
    out = mtmc_mpn.relabel_detections(table, index, id_pred)
    assert out[:, 1].tolist() == [42, 7, 42] and torch.equal(out[:, [0, 2, 3, 4, 5, 6]], table[:, [0, 2, 3, 4, 5, 6]])
    assert table[:, 1].tolist() == [-1, -1, -1]         # the input is not modified
    assert mtmc_mpn.relabel_detections(table.double(), index, id_pred).dtype == torch.float64
    with pytest.raises(ValueError, match="relabel_detections"):
        mtmc_mpn.relabel_detections(table, index[:2], id_pred)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.idf1(table, table)                     # the score itself has no CPU path
