#!/usr/bin/env python3
"""Generate tests/golden/cs_cases.npz: the label vectors of tests/cs_cases.py::cpu_cases and what scikit-learn makes of
each (adjusted_rand_score, adjusted_mutual_info_score, homogeneity_score, completeness_score, v_measure_score -- the five
calls of the reference's inference loop, inference.py:509-519).  Needs scikit-learn (1.7.2 wrote the committed file; the
formulas are those of the 0.24.2 the reference pins); the tests read the file and need none.

    python tests/golden/make_golden_cs.py
"""
import os
import sys

import numpy as np
import sklearn
from sklearn import metrics

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from cs_cases import cpu_cases  # noqa: E402


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    names = []
    for name, (t, p) in cpu_cases().items():
        names.append(name)
        out[name + "/true"], out[name + "/pred"] = t, p
        out[name + "/sklearn"] = np.array([metrics.adjusted_rand_score(t, p), metrics.adjusted_mutual_info_score(t, p),
                                           metrics.homogeneity_score(t, p), metrics.completeness_score(t, p),
                                           metrics.v_measure_score(t, p)], dtype=np.float64)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "cs_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
