"""Cases and the host reference (numpy) of the stable grouping `mtmc_group_by_index`: a stable grouping has exactly one
answer, so every comparison is an equality."""
import numpy as np

INT64_MIN, INT64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
DIGIT_BITS = (0, 1, 3, 8, 11)
PATTERNS = ("random", "sorted", "decreasing", "one_group", "alternating", "last_only", "outside_mixed", "outside_only")


def reference(index: np.ndarray, n_groups: int):
    """(perm, offsets, lost): np.argsort(kind="stable") of the keys, searchsorted of the sorted keys, rows keyed n_groups."""
    index = np.asarray(index, dtype=np.int64)
    key = np.where((index >= 0) & (index < n_groups), index, n_groups)
    perm = np.argsort(key, kind="stable").astype(np.int64)
    offsets = np.searchsorted(key[perm], np.arange(n_groups + 1)).astype(np.int64)
    return perm, offsets, int((key == n_groups).sum())


def row_counts(tile: int):
    return (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17)


def group_counts(n_rows: int):
    return tuple(dict.fromkeys((0, 1, 2, 37, 255, 256, 257, 70000, n_rows)))       # (in this order, each once)


def outside_values(n_groups: int):
    return np.array([-1, n_groups, 2 ** 40, INT64_MIN, INT64_MAX], dtype=np.int64)


def keys(pattern: str, n_rows: int, n_groups: int, seed: int = 0) -> np.ndarray:
    """index [n_rows] int64 of one key pattern."""
    rng = np.random.default_rng(seed + 17 * n_rows + n_groups)
    n = max(n_groups, 1)
    rows = np.arange(n_rows, dtype=np.int64)
    if pattern == "random":
        out = rng.integers(0, n, n_rows)
    elif pattern == "sorted":
        out = np.sort(rng.integers(0, n, n_rows))
    elif pattern == "decreasing":                       # strictly: needs n_groups >= n_rows, else as steep as the range allows
        out = (n_rows - 1 - rows) if n >= n_rows else ((n_rows - 1 - rows) * n) // max(n_rows, 1)
    elif pattern == "one_group":
        out = np.full(n_rows, n // 2)
    elif pattern == "alternating":
        out = np.where(rows % 2 == 0, n - 1, 0)
    elif pattern == "last_only":
        out = np.full(n_rows, n - 1)
    elif pattern == "outside_mixed":
        out = rng.integers(0, n, n_rows)
        bad = rng.random(n_rows) < 0.3
        out = np.where(bad, rng.choice(outside_values(n_groups), n_rows), out)
    elif pattern == "outside_only":
        out = rng.choice(outside_values(n_groups), n_rows)
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(out, dtype=np.int64)
