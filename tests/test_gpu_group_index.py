"""GPU tests of the stable grouping `mtmc_group_by_index` (csrc/group_index.hip) against numpy's stable argsort and
searchsorted (tests/group_cases.py).  A stable grouping has one answer: perm, offsets and the info word must be EQUAL.

With T = mtmc_group_tile_rows(): row counts around the wave (64) and the tile, group counts around the digit widths, and
digit widths 1 .. 11, which at these sizes take one, two, three and more passes, the one-workgroup scan (tables up to 4096
entries) and the two-level one."""
import functools

import numpy as np
import pytest
import torch

import group_cases as gc

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A5A5A5A5A
PAD = 8


def _lib():
    from mtmc_mpn import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _tile():
    return int(_lib().load().mtmc_group_tile_rows())


def _group(index, n_groups, digit_bits=0, short=0):
    """One raw call into poisoned buffers: (perm, offsets, info word) as numpy / int, after checking the poison."""
    from mtmc_mpn import _call
    lib = _lib().load()
    idx = torch.from_numpy(index).cuda()
    n = idx.numel()
    perm = torch.full((n + 2 * PAD,), POISON, dtype=torch.int64, device="cuda")
    offsets = torch.full((n_groups + 1 + 2 * PAD,), POISON, dtype=torch.int64, device="cuda")
    info = torch.full((1 + 2 * PAD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    need = lib.mtmc_group_by_index_workspace_bytes(n, n_groups, digit_bits)
    assert need > 0
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = lib.mtmc_group_by_index(idx.data_ptr() if n else None, n, n_groups, digit_bits, perm.data_ptr() + 8 * PAD,
                                 offsets.data_ptr() + 8 * PAD, info.data_ptr() + 4 * PAD, ws.data_ptr(), need - short,
                                 _call.stream(idx.device))
    if short:
        return rc
    _lib().check(rc)
    torch.cuda.synchronize()
    for buf, body in ((perm, n), (offsets, n_groups + 1), (info, 1)):
        poison = 0x5A5A5A5A if buf.dtype == torch.int32 else POISON
        assert bool((buf[:PAD] == poison).all()) and bool((buf[PAD + body:] == poison).all()), "poison overwritten"
    assert bool((ws[need:] == 0x5A).all()), "the workspace was overrun"
    return perm[PAD:PAD + n].cpu().numpy(), offsets[PAD:PAD + n_groups + 1].cpu().numpy(), int(info[PAD])


def _check(index, n_groups, digit_bits):
    perm, offsets, lost = _group(index, n_groups, digit_bits)
    want_perm, want_offsets, want_lost = gc.reference(index, n_groups)
    where = (index.size, n_groups, digit_bits)
    assert np.array_equal(offsets, want_offsets), where
    assert np.array_equal(perm, want_perm), where
    assert lost == want_lost, where


@pytest.mark.parametrize("digit_bits", gc.DIGIT_BITS)
@pytest.mark.parametrize("rows", range(9))
def test_sizes(rows, digit_bits):
    n_rows = gc.row_counts(_tile())[rows]
    for n_groups in gc.group_counts(n_rows):
        _check(gc.keys("random", n_rows, n_groups), n_groups, digit_bits)


@pytest.mark.parametrize("digit_bits", (0, 3))
@pytest.mark.parametrize("n_groups", (2, 37, 70000))
@pytest.mark.parametrize("pattern", gc.PATTERNS)
def test_key_patterns(pattern, n_groups, digit_bits):
    n_rows = 3 * _tile() + 17
    _check(gc.keys(pattern, n_rows, n_groups), n_groups, digit_bits)
    if pattern == "decreasing":                          # strictly decreasing: as many groups as rows
        _check(gc.keys(pattern, n_rows, n_rows), n_rows, digit_bits)


@pytest.mark.parametrize("tiles,n_groups,digit_bits", [
    (4, 900, 10),                      # 4 * 2^10 = 4096 table entries: the one-workgroup scan, two trips
    (41, 2000, 11),                    # 41 scan blocks and their totals
    (2101, 2000, 11),                  # more than 2048 totals: the walk over the totals takes two trips
    (301, 300000, 0),                  # the library's own choice with more than one pass
])
def test_scan_levels(tiles, n_groups, digit_bits):
    n_rows = (tiles - 1) * _tile() + 5
    for pattern in ("random", "one_group"):
        _check(gc.keys(pattern, n_rows, n_groups), n_groups, digit_bits)


@pytest.mark.parametrize("digit_bits", (0, 3))
def test_a_short_workspace_is_refused(digit_bits):
    lib = _lib().load()
    index = gc.keys("random", 1000, 37)
    assert _group(index, 37, digit_bits, short=1) == _lib().E_ARG
    text = lib.mtmc_mpn_last_error()
    assert text.startswith(b"group_by_index: ") and b"workspace" in text
    _check(index, 37, digit_bits)                        # and the exact size is taken


@pytest.mark.parametrize("n_groups", (37, 70000))
def test_python_forms_return_the_same_grouping(n_groups):
    import mtmc_mpn
    from mtmc_mpn import pool
    index = gc.keys("outside_mixed", 2 * _tile() + 5, n_groups)
    want_perm, want_offsets, _ = gc.reference(index, n_groups)
    dev = torch.from_numpy(index).cuda()
    perm, offsets = pool.group_by_index(dev, n_groups)
    g = mtmc_mpn.group_by_index(dev, n_groups)
    for p, o in ((perm, offsets), (g.perm, g.offsets)):
        assert p.dtype == o.dtype == torch.int64
        assert np.array_equal(p.cpu().numpy(), want_perm) and np.array_equal(o.cpu().numpy(), want_offsets)
    narrow = index.astype(np.int32)                      # an int32 index is converted: the keys are its values
    g32 = mtmc_mpn.group_by_index(torch.from_numpy(narrow).cuda(), n_groups)
    want32 = gc.reference(narrow.astype(np.int64), n_groups)
    assert np.array_equal(g32.perm.cpu().numpy(), want32[0]) and np.array_equal(g32.offsets.cpu().numpy(), want32[1])
    assert g.num_groups == n_groups and g.index.dtype == torch.int64 and g.index.shape == dev.shape
    if n_groups == 70000:
        assert torch.equal(g.index, dev)


@pytest.mark.parametrize("n_groups", (37, 70000))
def test_a_captured_call_is_replayed_on_new_keys(n_groups):
    n_rows = 2 * _tile() + 5
    first, second = gc.keys("random", n_rows, n_groups), gc.keys("outside_mixed", n_rows, n_groups, seed=3)
    index = torch.from_numpy(first).cuda()
    torch.ops.mtmc_mpn.group_by_index(index, n_groups)   # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        perm, offsets = torch.ops.mtmc_mpn.group_by_index(index, n_groups)
    for keys in (first, second):
        index.copy_(torch.from_numpy(keys))
        graph.replay()
        torch.cuda.synchronize()
        want_perm, want_offsets, _ = gc.reference(keys, n_groups)
        assert np.array_equal(perm.cpu().numpy(), want_perm) and np.array_equal(offsets.cpu().numpy(), want_offsets)
