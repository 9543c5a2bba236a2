#!/usr/bin/env python3
"""Generate tests/golden/idf1_cases.npz: the seven integer columns (camera, id, frame, x, y, width, height) of the
reference's eval/ground_truth_S02.txt as int32, and for every case of tests/idf1_cases.py the optimum that
`scipy.optimize.linear_sum_assignment` finds on motmetrics' (objects + hypotheses)^2 matrix fpmatrix + fnmatrix
(tests/idf1_ref.py::motmetrics_matrices over the yardstick's overlap counts).  Needs scipy (1.15.3 wrote the committed
file); the tests read the file and need neither scipy nor the reference.

    python tests/golden/make_golden_idf1.py <reference>/eval/ground_truth_S02.txt
"""
import os
import sys

import numpy as np
import scipy
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import idf1_cases  # noqa: E402
import idf1_ref  # noqa: E402


def main():
    table = np.loadtxt(sys.argv[1], dtype=np.int64)[:, :7]
    assert table.shape == (20956, 7) and len({tuple(r) for r in table[:, :3].tolist()}) == 20956   # unique (camera, id, frame)
    out = {"scipy_version": np.array(scipy.__version__), "s02_gt": table.astype(np.int32)}
    np.savez_compressed(idf1_cases.GOLDEN, **out)      # the S02 cases read the table from the file
    names = []
    for name in idf1_cases.CASES:
        gt, pred, kw, _ = idf1_cases.case(name)
        r = idf1_ref.idf1(gt, pred, **kw)
        g, p = gt[r.kept_gt], pred[r.kept]
        oc = [int(np.sum(g[:, 1].astype(np.int64) == v)) for v in r.gt_ids]
        hc = [int(np.sum(p[:, 1].astype(np.int64) == v)) for v in r.pred_ids]
        fp, fn = idf1_ref.motmetrics_matrices(r.C.astype(np.int64), np.array(oc), np.array(hc))
        rows, cols = linear_sum_assignment(fp + fn)
        idfp, idfn = int(fp[rows, cols].sum()), int(fn[rows, cols].sum())
        out[name + "/scipy"] = np.array([r.num_objects - idfn, idfp, idfn], dtype=np.int64)     # idtp, idfp, idfn
        names.append(name)
        print(name, out[name + "/scipy"].tolist(), "yardstick", [r.idtp, r.idfp, r.idfn])
    out["names"] = np.array(names)
    np.savez_compressed(idf1_cases.GOLDEN, **out)
    print(f"{idf1_cases.GOLDEN}: {len(names)} cases, {os.path.getsize(idf1_cases.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
