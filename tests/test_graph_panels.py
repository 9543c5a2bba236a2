"""CPU: the paneled graph builder's C ABI (`mtmc_build_graph_paneled`, `mtmc_graph_paneled_workspace_bytes`,
`mtmc_graph_panel_rows`): declared, bound, exported, sized and argument-checked without a GPU."""
import ctypes
import os
import re

import pytest

import gram_cases
from abi_refusal import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtmc_build_graph_paneled", "mtmc_graph_paneled_workspace_bytes", "mtmc_graph_panel_rows")
GIB = 1 << 30


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "#define MTMC_MPN_ABI_VERSION 6" in header and _lib.load().mtmc_mpn_abi_version() == 6
    assert "| `mtmc_build_graph_paneled`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_workspace_query_refuses_what_the_entry_refuses():
    from mtmc_mpn import _lib
    q = _lib.load().mtmc_graph_paneled_workspace_bytes
    for n in (0, -3, 262145):
        assert q(n, 2048, 8, 0) == 0, n
    for f in (0, 31):
        assert q(450, f, 8, 0) == 0, f
    assert q(8000, 64, 4097, 0) == 0 and q(8000, 64, 4096, 0) > 0          # k above 4096 after clipping to n ...
    assert q(450, 64, 4097, 0) == q(450, 64, 450, 0) > 0                   # ... and one that the clipping brings under it
    assert q(450, 64, -1, 0) == 0
    assert q(450, 64, 8, -1) == 0 and q(450, 64, 0, -128) == 0
    assert q(46001, 32, 4, 0) > 0 and q(262144, 2048, 50, 0) > 0
    assert q(450, 64, 0, 0) > 0                                            # the gate alone: no picks


def whole_split(lib, n, f):
    """The split-K factor of the whole product's plan.  Above 46 000 nodes the dense query answers 0, and the plan has long
    been one 128 x 128 tile per CU or more: unsplit (tests/gram_cases.py)."""
    return gram_cases.workspace_split(n, f, lib.mtmc_graph_workspace_bytes(n, f)) if n <= 46000 else 1


@pytest.mark.parametrize("n", [450, 8000, 46000, 100000])
def test_workspace_is_bounded_by_the_panel_and_the_lists(n):
    from mtmc_mpn import _lib
    lib = _lib.load()
    for f in (32, 2048):
        split = whole_split(lib, n, f)
        for k in (1, 50):
            for rows in (128, 1024):
                got = lib.mtmc_graph_paneled_workspace_bytes(n, f, k, rows)
                bound = (1 + split) * rows * n * 4 + 8 * n * k + 64 * n + 8 * f + 65536
                assert 0 < got <= bound, (n, f, k, rows, got, bound)
                assert got >= min(rows, n) * n * 4                         # the panel itself


def test_workspace_at_the_old_limit_is_under_a_gib():
    from mtmc_mpn import _lib
    lib = _lib.load()
    assert lib.mtmc_graph_paneled_workspace_bytes(46000, 2048, 32, 1024) < GIB
    assert lib.mtmc_graph_knn_workspace_bytes(46000, 2048) > 8.7e9


def test_panel_rows():
    from mtmc_mpn import _lib
    rows = _lib.load().mtmc_graph_panel_rows
    assert rows(450, 64, 1000) == 450 and rows(450, 64, 450) == 450 and rows(450, 64, 17) == 17 and rows(9, 64, 1) == 1
    for n in (1, 9, 127, 128, 450, 8000, 46000, 46001, 100000, 262144):
        p = rows(n, 2048, 0)
        assert 1 <= p <= n and (p % 128 == 0 or p == n), (n, p)
    for n in (46001, 100000, 262144):
        p = rows(n, 32, 0)
        assert p % 128 == 0 and p * n * 4 <= GIB < (p + 128) * n * 4, (n, p)   # the largest such multiple
    assert rows(262144, 32, 0) == 1024 and rows(100000, 32, 0) == 2560
    assert rows(2_000_000, 64, 0) == 0 and rows(0, 64, 0) == 0 and rows(450, 31, 0) == 0 and rows(450, 64, -1) == 0


def call(lib, **kw):
    n, f, e = 450, 2048, 150454
    a = dict(feats=0x10000, stride=f, n=n, f=f, in_list=0x20000, in_off=0x30000, out_list=0x40000, out_off=0x50000,
             block_off=0x60000, n_cams=4, e=e, labels=None, x=0x70000, index=0x80000, attr=0x90000, elabels=None,
             start=0xd0000, gap=300, k=8, rows=128, cap=7200, pos=0xa0000, n_kept=0xb0000, ws=0x100000, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.mtmc_graph_paneled_workspace_bytes(450, 2048, 8, 128)
    return lib.mtmc_build_graph_paneled(
        a["feats"], a["stride"], a["n"], a["f"], 1, a["in_list"], a["in_off"], a["out_list"], a["out_off"], a["block_off"],
        a["n_cams"], a["e"], a["labels"], a["x"], a["index"], a["attr"], a["elabels"], a["start"], a["gap"], a["k"],
        a["rows"], a["cap"], a["pos"], a["n_kept"], a["ws"], a["ws_bytes"], None)


def test_bad_arguments_are_refused_before_any_launch():
    from mtmc_mpn import _lib
    lib = _lib.load()
    need = lib.mtmc_graph_paneled_workspace_bytes(450, 2048, 8, 128)
    assert need > 0
    for bad in (dict(feats=None), dict(x=None), dict(in_list=None), dict(out_off=None), dict(index=None), dict(attr=None),
                dict(elabels=0xc0000),                          # edge labels without node labels
                dict(feats=0x10004), dict(x=0x70008), dict(stride=2049), dict(ws=0x100080), dict(index=0x80008),
                dict(attr=0x90004), dict(n=0), dict(n=262145), dict(f=2040), dict(f=0), dict(n_cams=0),
                dict(k=-1), dict(cap=-1), dict(pos=None), dict(n_kept=None),
                dict(k=0, start=None),                          # neither k nor a gate
                dict(k=0, start=None, gap=0), dict(gap=0), dict(gap=-5), dict(k=0, gap=0),
                dict(rows=-1), dict(n=8000, k=4097, ws_bytes=1 << 40)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_ARG, "build_graph_paneled"), bad
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(rows=0, ws_bytes=need),                    # the library's choice (all 450 rows) needs more than 128 rows do
                dict(n=46001, e=10 ** 9, cap=10 ** 6, ws_bytes=need)):   # beyond the old limit: sized, not refused outright
        assert refused(lib, lambda: call(lib, **bad), _lib.E_WORKSPACE, "build_graph_paneled"), bad
    # the other entries and their queries keep the old limit
    assert lib.mtmc_graph_knn_workspace_bytes(46001, 2048) == 0 and lib.mtmc_graph_workspace_bytes(46001, 2048) == 0
