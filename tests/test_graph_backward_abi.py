"""CPU: the C ABI of the graph builder's backward -- declared, exported, sized and argument-checked without a GPU (every
refusal below happens before any launch, so the pointers are never read)."""
import ctypes
import os
import re

from abi_refusal import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtmc_graph_backward_workspace_bytes", "mtmc_build_graph_backward")


def test_symbols_are_declared_bound_and_exported():
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "| `mtmc_build_graph_backward`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_workspace_query_needs_no_gpu():
    from mtmc_mpn import _lib
    lib = _lib.load()
    q = lib.mtmc_graph_backward_workspace_bytes
    s02 = q(450, 2048)
    npad = (450 + 31) // 32 * 32
    assert 450 * npad * 4 <= s02 <= 450 * npad * 4 + 2 * 2048 * 8 + 5 * 450 * 4 + 16 * 256   # O(N^2 + N + F): no [N, F], no [E, F]
    assert q(1, 32) > 0 and q(46000, 2048) > 0
    assert q(0, 2048) == 0 and q(-3, 2048) == 0 and q(46001, 2048) == 0
    assert q(450, 0) == 0 and q(450, 2040) == 0
    assert q(900, 2048) > 3 * s02


def call(lib, **kw):
    n, f, e = 450, 2048, 150454
    a = dict(feats=0x10000, stride=f, n=n, f=f, l2norm=1, in_list=0x20000, in_off=0x30000, out_list=0x40000,
             out_off=0x50000, block_off=0x60000, n_cams=4, e=e, x=0x70000, edge_attr=0x80000, d_x=0x90000,
             d_attr=0xa0000, out=0xb0000, ws=0x100000, ws_bytes=lib.mtmc_graph_backward_workspace_bytes(n, f))
    a.update(kw)
    return lib.mtmc_build_graph_backward(
        a["feats"], a["stride"], a["n"], a["f"], a["l2norm"], a["in_list"], a["in_off"], a["out_list"], a["out_off"],
        a["block_off"], a["n_cams"], a["e"], a["x"], a["edge_attr"], a["d_x"], a["d_attr"], a["out"], a["ws"],
        a["ws_bytes"], None)


def test_bad_arguments_are_refused_before_any_launch():
    from mtmc_mpn import _lib
    lib = _lib.load()
    for bad in (dict(feats=None), dict(x=None), dict(out=None), dict(in_list=None), dict(out_off=None), dict(edge_attr=None),
                dict(d_x=None, d_attr=None),                     # both gradients missing on a graph with edges
                dict(feats=0x10004), dict(x=0x70008), dict(d_x=0x90004), dict(out=0xb0008), dict(edge_attr=0x80004),
                dict(d_attr=0xa0004), dict(stride=2049), dict(ws=0x100080),
                dict(n=0), dict(n=46001), dict(f=2040), dict(f=0), dict(n_cams=0), dict(e=-1), dict(out=0x90000)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_ARG, "build_graph_backward"), bad
    for bad in (dict(ws=None), dict(ws_bytes=lib.mtmc_graph_backward_workspace_bytes(450, 2048) - 1), dict(ws_bytes=0)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_WORKSPACE, "build_graph_backward"), bad
