"""CPU test of `mtmc_id_assign` through ctypes: the host half of IDF1 (the exact assignment on the overlap counts, one
connected component of their support graph at a time) against the yardstick's Hungarian on motmetrics' full problem
(tests/idf1_ref.py).  The entry point touches no GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import idf1_ref


def assign(c=None, cells=None, shape=None):
    """(rc, idtp, match_of_obj, stats) of one call; `c` a dense matrix, or `cells` [k, 3] with `shape`"""
    from mtmc_mpn import _lib
    lib = _lib.load()
    if c is not None:
        c = np.asarray(c, dtype=np.int32)
        shape = c.shape
        rr, cc = np.nonzero(c)
        cells = np.stack([rr, cc, c[rr, cc]], axis=1)
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
    idtp, stats = ctypes.c_int64(-1), np.full(3, -1, dtype=np.int64)
    match = np.full(max(shape[0], 1), -2, dtype=np.int32)
    rc = lib.mtmc_id_assign(cells.ctypes.data if len(cells) else None, len(cells), shape[0], shape[1], ctypes.addressof(idtp),
                            match.ctypes.data, stats.ctypes.data)
    return rc, int(idtp.value), match[:shape[0]], stats.tolist()


def check(c, want=None):
    c = np.asarray(c, dtype=np.int32)
    rc, idtp, match, stats = assign(c)
    assert rc == 0
    if want is None:
        want = idf1_ref.id_scores(c, c.sum(1), c.sum(0))[0]
    assert idtp == want
    cols = match[match >= 0]
    assert len(set(cols.tolist())) == len(cols) and all(0 <= k < c.shape[1] for k in cols)       # one-to-one
    assert all(c[o, h] > 0 for o, h in enumerate(match) if h >= 0)                              # only pairs with C > 0
    assert sum(int(c[o, h]) for o, h in enumerate(match) if h >= 0) == idtp
    assert stats == list(idf1_ref.component_stats(c))
    return match, stats


def brute(c):
    c = np.asarray(c)
    n, m = c.shape
    if n > m:
        return brute(c.T)
    return max(sum(int(c[i, p[i]]) for i in range(n)) for p in itertools.permutations(range(m), n))


def test_hand_cases():
    rc, idtp, match, stats = assign(cells=np.zeros((0, 3)), shape=(0, 0))
    assert (rc, idtp, stats) == (0, 0, [0, 0, 0]) and len(match) == 0
    rc, idtp, match, stats = assign(cells=np.zeros((0, 3)), shape=(3, 2))                        # nothing overlaps
    assert (rc, idtp, stats) == (0, 0, [0, 0, 0]) and match.tolist() == [-1, -1, -1]
    assert check([[7]], 7)[0].tolist() == [0]
    rc, idtp, match, stats = assign(cells=[[0, 0, 0], [1, 1, 0]], shape=(2, 2))                  # all-zero C, listed as cells
    assert (rc, idtp, stats) == (0, 0, [0, 0, 0]) and match.tolist() == [-1, -1]
    assert check([[5, 4], [4, 0]], 8)[0].tolist() == [1, 0]                                     # greedy would take the 5
    wide = [[3, 0, 2, 9, 1], [4, 8, 0, 9, 0], [0, 1, 7, 9, 2]]                                  # three rows want column 3
    assert brute(wide) == 24
    assert check(wide, 24)[1] == [1, 3, 5]
    tall = np.array(wide).T
    assert check(tall, 24)[1] == [1, 5, 3]
    match, _ = check([[2, 2], [2, 2]], 4)                                                       # ties: either optimum
    assert sorted(match.tolist()) == [0, 1]
    check([[1, 1, 0], [1, 1, 0], [0, 0, 0]], 2)
    check([[0, 3, 0], [0, 3, 0], [0, 3, 0]], 3)                                                 # a star: one match only


def test_small_random_matrices_against_brute_force():
    g = np.random.default_rng(3)
    for _ in range(60):
        n, m = g.integers(1, 6, size=2)
        c = g.integers(0, 5, size=(n, m)) * (g.random((n, m)) < 0.6)
        check(c, brute(c))


def test_dense_40_by_60_against_the_yardstick():
    g = np.random.default_rng(4)
    c = g.integers(0, 10, size=(40, 60))
    _, stats = check(c)
    assert stats == [1, 40, 60]
    check(c.T.copy())


def test_block_diagonal_300_components():
    g = np.random.default_rng(6)
    blocks = [g.integers(1, 10, size=(g.integers(1, 7), g.integers(1, 7))) for _ in range(300)]
    n, m = sum(b.shape[0] for b in blocks), sum(b.shape[1] for b in blocks)
    c = np.zeros((n, m), dtype=np.int32)
    r0 = k0 = want = 0
    for b in blocks:
        c[r0:r0 + b.shape[0], k0:k0 + b.shape[1]] = b
        want += idf1_ref.id_scores(b, b.sum(1), b.sum(0))[0]                 # the yardstick, block by block
        r0, k0 = r0 + b.shape[0], k0 + b.shape[1]
    perm_r, perm_c = g.permutation(n), g.permutation(m)                      # (the components are not contiguous)
    c = c[perm_r][:, perm_c]
    _, stats = check(c, want)
    big = max(((b.shape[0] * b.shape[1], b.shape[0], b.shape[1]) for b in blocks))
    assert stats == [300, big[1], big[2]] == list(idf1_ref.component_stats(c))


def test_4096_square_of_2048_components_returns_at_once():
    """a dense O(n^3) solve of 4096 x 4096 would not return in test time: the split into components is what this shows"""
    g = np.random.default_rng(8)
    n = 4096
    perm_r, perm_c = g.permutation(n), g.permutation(n)
    vals = g.integers(1, 100, size=(n // 2, 2, 2))
    cells, want = [], 0
    for k in range(n // 2):
        b = vals[k]
        want += max(int(b[0, 0] + b[1, 1]), int(b[0, 1] + b[1, 0]))
        cells += [(perm_r[2 * k + i], perm_c[2 * k + j], b[i, j]) for i in (0, 1) for j in (0, 1)]
    cells = np.array(cells, dtype=np.int32)[g.permutation(2 * n)]
    rc, idtp, match, stats = assign(cells=cells, shape=(n, n))
    assert rc == 0 and idtp == want and stats == [n // 2, 2, 2]
    assert sorted(match.tolist()) == list(range(n))


def test_refusals_and_their_text():
    from mtmc_mpn import _lib
    lib = _lib.load()
    err = lambda: lib.mtmc_mpn_last_error().decode()                       # noqa: E731
    assert assign(cells=[[0, 2, 1]], shape=(2, 2))[0] == _lib.E_ARG and "id_assign: cell 0 = (0, 2, 1) is outside" in err()
    assert assign(cells=[[-1, 0, 1]], shape=(2, 2))[0] == _lib.E_ARG and "id_assign: cell 0" in err()
    assert assign(cells=[[0, 0, -3]], shape=(2, 2))[0] == _lib.E_ARG and "negative" in err()
    assert assign(cells=[[0, 1, 1], [0, 1, 2]], shape=(2, 2))[0] == _lib.E_ARG and "listed twice" in err()
    assert assign(cells=np.zeros((0, 3)), shape=(8193, 8193))[0] == _lib.E_ARG and "MTMC_ID_MAX_CELLS" in err()
    idtp = ctypes.c_int64(0)
    assert lib.mtmc_id_assign(None, 1, 2, 2, ctypes.addressof(idtp), None, None) == _lib.E_ARG and "NULL" in err()
    assert lib.mtmc_id_assign(None, 0, 0, 0, None, None, None) == _lib.E_ARG and "NULL" in err()
    assert lib.mtmc_id_assign(None, -1, 0, 0, ctypes.addressof(idtp), None, None) == _lib.E_ARG and "id_assign" in err()
    # the device entry points refuse the same sizes before they touch a GPU
    assert lib.mtmc_id_overlap_workspace_bytes(8193, 8193, 10) == 0 and lib.mtmc_id_overlap_workspace_bytes(8192, 8192, 10) > 0
    assert lib.mtmc_id_overlap_workspace_bytes(-1, 4, 4) == 0
    assert lib.mtmc_id_overlap(None, None, None, None, 0, None, None, None, None, 0, 0, 8193, 8193, 0.75, None, 0, None) == _lib.E_ARG
    assert "id_overlap: n_obj * n_hyp is above MTMC_ID_MAX_CELLS" in err()
    assert lib.mtmc_id_overlap(None, None, None, None, 2 ** 31, None, None, None, None, 0, 0, 1, 1, 0.75, None, 0, None) == _lib.E_ARG
    assert "2^31" in err()
    assert lib.mtmc_id_overlap(None, None, None, None, 0, None, None, None, None, 0, 0, 1, 1, 0.75, None, 0, None) == _lib.E_ARG
    assert "id_overlap: NULL" in err()
    assert lib.mtmc_id_filter(None, None, None, None, 0, 0, 65, 0, 0.0, 0.0, 0.0, 0.0, None, None, 0, 0, 0, 2, 1, None, None, None,
                              None, None) == _lib.E_ARG
    assert "id_filter: 65 cameras, at most 64" in err()
    assert lib.mtmc_id_filter(None, None, None, None, 4, 2, 3, 0, 0.0, 0.0, 0.0, 0.0, None, None, 0, 0, 0, 2, 1, None, None, None,
                              None, None) == _lib.E_ARG
    assert "id_filter: NULL" in err()
    assert lib.mtmc_id_cells(None, 2, 2, None, 0, None, None) == _lib.E_ARG and "id_cells: NULL" in err()
