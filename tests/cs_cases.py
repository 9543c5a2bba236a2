"""Label-vector cases of the cluster-score tests (numpy only; every case is a pair of int64 vectors made from a fixed seed)."""
import numpy as np

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def random_pair(n, k, seed, flip=0.2):
    """k random true clusters over n nodes; the prediction is the truth with `flip` of the nodes moved to a random cluster"""
    g = np.random.default_rng(seed)
    t = g.integers(0, k, size=n, dtype=np.int64)
    p = t.copy()
    moved = g.random(n) < flip
    p[moved] = g.integers(0, k, size=int(moved.sum()), dtype=np.int64)
    return t, p


def degenerate_cases():
    z = lambda n: np.zeros(n, dtype=np.int64)
    r = lambda n: np.arange(n, dtype=np.int64)
    return {
        "n1": (z(1), np.array([5], dtype=np.int64)),
        "one_cluster_both": (z(9), np.full(9, 3, dtype=np.int64)),
        "singletons_both": (r(9), r(9)[::-1].copy()),
        "one_vs_singletons": (z(9), r(9)),
        "singletons_vs_one": (r(9), z(9)),
        "two_swapped": (np.array([0, 0, 0, 1, 1], dtype=np.int64), np.array([1, 1, 1, 0, 0], dtype=np.int64)),
        "independent_2x2": (np.array([0, 0, 1, 1], dtype=np.int64), np.array([0, 1, 0, 1], dtype=np.int64)),
        "emi_lower_bound": (np.array([0] * 7 + [1] * 3, dtype=np.int64), np.array([0] * 8 + [1] * 2, dtype=np.int64)),
    }


def extreme_value_case(n=200, seed=7):
    """compact labels 0..9 and the same vectors with the ids replaced by extreme and non-compact int64 values"""
    t, p = random_pair(n, 10, seed)
    values = np.array([I64_MIN, -1, 0, 7, I64_MAX, 3 * 5 + 11, 3 * 6 + 11, 3 * 7 + 11, 3 * 1000 + 11, -(2 ** 40)], dtype=np.int64)
    other = values[::-1].copy()
    return (t, p), (values[t], other[p])


def edge_cases():
    """wave and workgroup edges: n around 64, 256, 1024 with 2..n/3 clusters"""
    out = {}
    for i, n in enumerate((63, 64, 65, 257, 1025)):
        k = int(np.random.default_rng(100 + i).integers(2, n // 3 + 1))
        out[f"edge_n{n}"] = random_pair(n, k, 200 + i)
    return out


def cpu_cases():
    """the case list of the committed fixture (tests/golden/cs_cases.npz): everything above and random pairs up to n = 3000
    with up to 3000 clusters"""
    cases = dict(degenerate_cases())
    (ct, cp), (et, ep) = extreme_value_case()
    cases["values_compact"], cases["values_extreme"] = (ct, cp), (et, ep)
    cases.update(edge_cases())
    for i, (n, k, flip) in enumerate(((10, 3, 0.3), (100, 7, 0.1), (100, 50, 0.5), (500, 2, 0.4), (777, 120, 0.05),
                                      (1500, 1500, 0.9), (2000, 40, 0.2), (3000, 3000, 0.5), (3000, 900, 0.02),
                                      (3000, 3, 0.0))):
        cases[f"random_{n}_{k}_{i}"] = random_pair(n, k, 300 + i, flip)
    return cases
