"""CPU tests of `pool_tracklets`: the host-side offsets, the exports and the host-only sizing, the argument errors, and the
yardstick (tests/pool_ref.py) against itself.  Nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pool_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mtmc_pool_chunk_rows", "mtmc_pool_tracklets_workspace_bytes", "mtmc_pool_tracklets", "mtmc_pool_tracklets_backward"]


def test_offsets_from_lengths():
    from mtmc_mpn import pool
    for lengths, d, want in (([1], 1, [0, 1]), ([3, 1, 2], 6, [0, 3, 4, 6])):
        for form in (lengths, tuple(lengths), np.asarray(lengths), np.asarray(lengths, dtype=np.int32),
                     torch.tensor(lengths), torch.tensor(lengths, dtype=torch.int32)):
            got = pool.offsets_from_lengths(form, d)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == want
    assert pool.offsets_from_lengths([], 0).tolist() == [0]


@pytest.mark.parametrize("lengths,d", [([3, 0, 2], 5), ([3, -1, 2], 4), ([3, 1, 2], 7), ([3, 1, 2], 5), ([], 1)])
def test_offsets_from_lengths_refuses(lengths, d):
    from mtmc_mpn import pool
    with pytest.raises(ValueError):
        pool.offsets_from_lengths(lengths, d)
    with pytest.raises(ValueError):
        pool.offsets_from_lengths(np.asarray(lengths, dtype=np.int64), d)


def test_exports_and_header():
    import mtmc_mpn
    from mtmc_mpn import _lib, pool
    assert mtmc_mpn.pool is pool and mtmc_mpn.pool_tracklets is pool.pool_tracklets
    assert {"pool", "pool_tracklets"} <= set(mtmc_mpn.__all__)
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    assert set(NAMES) <= set(_lib.EXPORTS) and set(NAMES) <= declared
    assert "train.py:305-316" in header and "libs/reid_feature_extraction.py:177-178" in header
    lib = _lib.load()
    assert lib.mtmc_mpn_abi_version() == 6
    assert all(hasattr(lib, n) for n in NAMES)
    r = lib.mtmc_pool_chunk_rows()
    assert r in (16, 32, 64, 128) and r == pool.CHUNK_ROWS


def test_workspace_sizing_needs_no_gpu():
    from mtmc_mpn import _lib, pool
    lib = _lib.load()
    r = pool.CHUNK_ROWS
    for d, f in ((30000, 2048), (1, 4), (r, 256), (r + 1, 100), (5000, 16384)):
        need = lib.mtmc_pool_tracklets_workspace_bytes(d, f)
        assert 0 < need <= 2 * -(-d // r) * f * 4 + 4096, (d, f, need)
    for d, f in ((30000, 6), (30000, 16388), (30000, 0), (-1, 2048), (2 ** 31, 2048)):
        assert lib.mtmc_pool_tracklets_workspace_bytes(d, f) == 0, (d, f)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Refused before anything is enqueued (no GPU needed), with a text."""
    from mtmc_mpn import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    cases = [dict(f=6), dict(f=16388), dict(stride=2050), dict(stride=1024), dict(embeds=p + 4), dict(out=p + 8), dict(ws_bytes=16),
             dict(d=2 ** 31), dict(n=-1), dict(offsets=None)]
    for kw in cases:
        a = dict(embeds=p, stride=2048, d=64, f=2048, offsets=p, n=3, out=p, info=p, ws=p, ws_bytes=1 << 30)
        a.update(kw)
        rc = lib.mtmc_pool_tracklets(a["embeds"], a["stride"], a["d"], a["f"], a["offsets"], a["n"], a["out"], a["info"], a["ws"],
                                     a["ws_bytes"], None)
        assert rc == _lib.E_ARG and b"pool_tracklets" in lib.mtmc_mpn_last_error(), kw
    for kw in (dict(f=6), dict(stride=1024), dict(stride=2049), dict(g=p + 4), dict(out=None)):
        a = dict(g=p, d=64, f=2048, offsets=p, n=3, out=p, stride=2048)
        a.update(kw)
        rc = lib.mtmc_pool_tracklets_backward(a["g"], a["d"], a["f"], a["offsets"], a["n"], a["out"], a["stride"], None)
        assert rc == _lib.E_ARG and b"pool_tracklets_backward" in lib.mtmc_mpn_last_error(), kw
    # nothing to do: success without touching a pointer
    assert lib.mtmc_pool_tracklets(None, 2048, 0, 2048, None, 0, None, None, None, 0, None) == 0
    assert lib.mtmc_pool_tracklets_backward(None, 0, 2048, None, 0, None, 2048, None) == 0


def test_argument_errors():
    from mtmc_mpn import pool_tracklets
    e = torch.zeros(6, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pool_tracklets(e, [3, 1, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pool_tracklets(e, offsets=torch.tensor([0, 3, 4, 6]))
    with pytest.raises(RuntimeError):
        pool_tracklets(e.double(), [3, 1, 2])
    with pytest.raises((ValueError, TypeError)):
        pool_tracklets(e)
    with pytest.raises((ValueError, TypeError)):
        pool_tracklets(e, [3, 1, 2], offsets=torch.tensor([0, 3, 4, 6]))


def test_yardstick_against_itself():
    lengths = [1, 2, 7, 64, 3, 130]
    d = sum(lengths)
    e = pool_ref.integer_embeds(d, 12, seed=3)
    assert e.dtype == np.float32 and np.array_equal(e, np.round(e)) and np.abs(e).min() >= 1 and np.abs(e).max() <= 64
    sums = pool_ref.column_sums(e, lengths)
    at = 0
    for s, n in enumerate(lengths):                    # the exact integer column sums, the slow way
        assert np.array_equal(sums[s], e[at:at + n].astype(np.int64).sum(axis=0))
        at += n
    ref = pool_ref.pool_ref(e, lengths)
    assert np.array_equal(np.rint(ref * np.asarray(lengths)[:, None]).astype(np.int64), sums)
    assert np.abs(ref * np.asarray(lengths)[:, None] - sums).max() <= 1e-9
    g = pool_ref.gaussian_embeds(len(lengths), 12, seed=4)
    gb = pool_ref.pool_backward_ref(g, lengths)
    assert gb.shape == (d, 12) and np.array_equal(gb[0], g[0].astype(np.float64)) and np.array_equal(gb[2], g[1] / 2.0)
    # the mean's adjoint: <pool(e), g> == <e, pool_backward(g)>
    assert abs((ref * g).sum() - (e.astype(np.float64) * gb).sum()) <= 1e-9 * np.abs(ref * g).sum()
    pool_ref.check_forward(ref, e, lengths, "integer")
    pool_ref.check_forward(pool_ref.pool_ref(gb, lengths), gb, lengths, "gaussian")
    pool_ref.check_backward(gb.astype(np.float32)[:3], g[:2], lengths[:2])
