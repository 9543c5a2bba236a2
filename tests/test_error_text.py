"""CPU: a refusal of a stand-alone operator's C entry point names that entry point in mtmc_mpn_last_error(), and reaches
Python as an exception with that text.  Host values only: every refusal below precedes the first HIP call, so no pointer is
read and no GPU is touched.  (The edge-loss, cluster-score, graph-backward and post-processing entry points have the same
assertion in the argument loops of their own test files.)"""
import ctypes

import pytest

from abi_refusal import refused
from mtmc_mpn import _call, _lib

P = 0x10000                                  # an aligned address that is never read


def test_cross_entropy_and_confusion_refusals_name_their_entry_point():
    lib = _lib.load()

    def fwd(logits=P, labels=P, n=10, c=2, mode=0, sums=P):
        return lib.mtmc_cross_entropy_forward(logits, labels, None, n, c, -100, mode, None, sums, P, None)
    for bad in (dict(logits=None), dict(labels=None), dict(sums=None), dict(n=-1), dict(c=0), dict(c=5), dict(logits=P + 4)):
        assert refused(lib, lambda: fwd(**bad), _lib.E_ARG, "cross_entropy_forward"), bad

    def bwd(logits=P, labels=P, n=10, c=2, mode=0, grad=P, sums=P, d=P):
        return lib.mtmc_cross_entropy_backward(logits, labels, None, n, c, -100, mode, grad, sums, d, None)
    for bad in (dict(logits=None), dict(labels=None), dict(grad=None), dict(d=None), dict(n=-1), dict(c=0), dict(c=5),
                dict(mode=-1), dict(mode=3), dict(mode=0, sums=None), dict(logits=P + 4), dict(d=P + 4)):
        assert refused(lib, lambda: bwd(**bad), _lib.E_ARG, "cross_entropy_backward"), bad

    def sfwd(logits=P, labels=P, n=10, c=2, s=3, mode=0, sums=P):
        return lib.mtmc_cross_entropy_steps_forward(logits, labels, None, n, c, s, -100, mode, sums, P, None)
    for bad in (dict(logits=None), dict(labels=None), dict(sums=None), dict(n=-1), dict(s=0), dict(c=0), dict(c=5),
                dict(mode=2), dict(mode=-1), dict(logits=P + 4)):
        assert refused(lib, lambda: sfwd(**bad), _lib.E_ARG, "cross_entropy_steps_forward"), bad

    def sbwd(logits=P, labels=P, n=10, c=2, s=3, mode=0, grad=P, sums=P, d=P):
        return lib.mtmc_cross_entropy_steps_backward(logits, labels, None, n, c, s, -100, mode, grad, sums, d, None)
    for bad in (dict(logits=None), dict(labels=None), dict(grad=None), dict(sums=None), dict(d=None), dict(n=-1), dict(s=0),
                dict(c=0), dict(c=5), dict(mode=2), dict(logits=P + 4), dict(d=P + 4)):
        assert refused(lib, lambda: sbwd(**bad), _lib.E_ARG, "cross_entropy_steps_backward"), bad

    def conf(logits=P, labels=P, n=10, c=2, counts=P):
        return lib.mtmc_edge_confusion(logits, labels, n, c, counts, None)
    for bad in (dict(logits=None), dict(labels=None), dict(counts=None), dict(n=-1), dict(c=1), dict(c=5)):
        assert refused(lib, lambda: conf(**bad), _lib.E_ARG, "edge_confusion"), bad


def test_build_graph_refusals_name_their_entry_point():
    lib = _lib.load()
    n, f, e = 450, 2048, 150454
    need = lib.mtmc_graph_workspace_bytes(n, f)

    def call(**kw):
        a = dict(feats=0x10000, stride=f, n=n, f=f, in_list=0x20000, in_off=0x30000, out_list=0x40000, out_off=0x50000,
                 block_off=0x60000, n_cams=4, e=e, labels=None, x=0x70000, index=0x80000, attr=0x90000, elabels=None,
                 ws=0x100000, ws_bytes=need)
        a.update(kw)
        return lib.mtmc_build_graph(a["feats"], a["stride"], a["n"], a["f"], 1, a["in_list"], a["in_off"], a["out_list"],
                                    a["out_off"], a["block_off"], a["n_cams"], a["e"], a["labels"], a["x"], a["index"],
                                    a["attr"], a["elabels"], a["ws"], a["ws_bytes"], None)
    for bad in (dict(feats=None), dict(x=None), dict(n=0), dict(n=46001), dict(f=2040), dict(f=0), dict(n_cams=0),
                dict(in_list=None), dict(out_off=None), dict(index=None), dict(attr=None), dict(elabels=0xa0000),
                dict(feats=0x10004), dict(x=0x70008), dict(stride=2049), dict(ws=0x100080)):
        assert refused(lib, lambda: call(**bad), _lib.E_ARG, "build_graph"), bad
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert refused(lib, lambda: call(**bad), _lib.E_WORKSPACE, "build_graph"), bad


def test_scatter_refusals_name_their_entry_point():
    lib = _lib.load()

    def args(src=P, index=P, n_src=10, n_cols=4, dim_size=5, out=P):
        return src, index, n_src, n_cols, dim_size, out
    bads = (dict(n_src=-1), dict(n_cols=0), dict(dim_size=-1), dict(out=None), dict(src=None), dict(index=None))
    for bad in bads:
        assert refused(lib, lambda: lib.mtmc_scatter_add(*args(**bad), None), _lib.E_ARG, "scatter_add"), bad
        assert refused(lib, lambda: lib.mtmc_scatter_add_i64(*args(**bad), None), _lib.E_ARG, "scatter_add_i64"), bad
        assert refused(lib, lambda: lib.mtmc_scatter_mean(*args(**bad), P, None), _lib.E_ARG, "scatter_mean"), bad
        assert refused(lib, lambda: lib.mtmc_scatter_max(*args(**bad), P, None), _lib.E_ARG, "scatter_max"), bad
    assert refused(lib, lambda: lib.mtmc_scatter_mean(*args(), None, None), _lib.E_ARG, "scatter_mean")   # no count scratch


def test_a_refusal_reaches_python_with_the_entry_points_name():
    """Through `_call.run`, the way every stand-alone operator calls the library (device -1: torch.cuda.device's no-op, so
    nothing initialises a GPU)."""
    lib = _lib.load()
    assert lib.mtmc_pool_tracklets(None, 0, -1, 4, None, 0, None, None, None, 0, None) == _lib.E_ARG     # another entry's text
    buf = (ctypes.c_int64 * 8)()
    with pytest.raises(RuntimeError, match=r"edge_prf: .*\(code -1\)"):
        _call.run(-1, lib.mtmc_edge_prf, ctypes.addressof(buf), 1, ctypes.addressof(buf), 1, -1, ctypes.addressof(buf),
                  ctypes.addressof(buf), None)
    with pytest.raises(RuntimeError, match=r"edge_loss_forward: .*\(code -1\)"):
        _call.run(-1, lib.mtmc_edge_loss_forward, None, None, 10, 2, 3, 0, None, 0.0, None, 0, None, None, None, None)
