#!/usr/bin/env python3
"""Generate tests/golden/mot_cases.npz: for every case of tests/mot_cases.py the integer counts and the distance sum of the
CLEAR MOT walk with the assignment of every group solved by `scipy.optimize.linear_sum_assignment` on
the big-cost matrix (tests/mot_ref.py::big_cost), a solver independent of the yardstick's own Hungarian.  Numbers only, a
few kilobytes.  Needs scipy (1.15.3 wrote the committed file); the tests read the file and need no scipy.  The S02 cases
read their table from tests/golden/idf1_cases.npz, which this script does not write.

    python tests/golden/make_golden_mot.py
"""
import os
import sys

import numpy as np
import scipy
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mot_cases  # noqa: E402
import mot_ref  # noqa: E402


def scipy_solve(d):
    rows, cols = linear_sum_assignment(mot_ref.big_cost(d))
    return [(int(i), int(j)) for i, j in zip(rows, cols) if i < d.shape[0] and j < d.shape[1] and not np.isnan(d[i, j])]


def main():
    out = {"scipy_version": np.array(scipy.__version__), "fields": np.array(mot_ref.COUNTS)}
    names = []
    for name in mot_cases.CASES:
        gt, pred, kw, _ = mot_cases.case(name)
        r = mot_ref.mot_scores(gt, pred, solver=scipy_solve, **kw)
        own, _ = mot_cases.yardstick(name)
        out[name + "/counts"] = np.array([getattr(r, k) for k in mot_ref.COUNTS], dtype=np.int64)
        out[name + "/dist_sum"] = np.array(r.dist_sum, dtype=np.float64)
        names.append(name)
        print(name, out[name + "/counts"].tolist(), repr(r.dist_sum), "yardstick",
              [getattr(own, k) for k in mot_ref.COUNTS] == out[name + "/counts"].tolist(), own.dist_sum == r.dist_sum)
    out["names"] = np.array(names)
    np.savez_compressed(mot_cases.GOLDEN, **out)
    print(f"{mot_cases.GOLDEN}: {len(names)} cases, {os.path.getsize(mot_cases.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
