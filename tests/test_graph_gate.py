"""CPU: the temporal gate's C entry (declared, bound, exported and argument-checked without a GPU), the rule's CPU
restatement (tests/gate_ref.py) on a case small enough to decide by hand, and the host count that sizes the gate-only
call's outputs (`graph_build.gated_edge_count`) against that restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gate_cases
import gate_ref
import knn_ref
from abi_refusal import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported_and_the_abi_version_stays():
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    name = "mtmc_build_graph_gated"
    assert name in declared and name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "#define MTMC_MPN_ABI_VERSION 6" in header and _lib.load().mtmc_mpn_abi_version() == 6
    assert "inference.py:420-441" in header
    assert "| `mtmc_build_graph_gated`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def call(lib, **kw):
    n, f, e = 450, 2048, 150454
    a = dict(feats=0x10000, stride=f, n=n, f=f, in_list=0x20000, in_off=0x30000, out_list=0x40000, out_off=0x50000,
             block_off=0x60000, n_cams=4, e=e, labels=None, x=0x70000, index=0x80000, attr=0x90000, elabels=None,
             start=0xd0000, gap=300, k=8, cap=7200, pos=0xa0000, n_kept=0xb0000, ws=0x100000,
             ws_bytes=lib.mtmc_graph_knn_workspace_bytes(n, f))
    a.update(kw)
    return lib.mtmc_build_graph_gated(
        a["feats"], a["stride"], a["n"], a["f"], 1, a["in_list"], a["in_off"], a["out_list"], a["out_off"], a["block_off"],
        a["n_cams"], a["e"], a["labels"], a["x"], a["index"], a["attr"], a["elabels"], a["start"], a["gap"], a["k"], a["cap"],
        a["pos"], a["n_kept"], a["ws"], a["ws_bytes"], None)


def test_bad_arguments_are_refused_before_any_launch():
    from mtmc_mpn import _lib
    lib = _lib.load()
    for bad in (dict(start=None), dict(gap=0), dict(gap=-1), dict(k=-1), dict(cap=-1), dict(n_kept=None), dict(pos=None),
                dict(start=None, k=0), dict(gap=0, k=0), dict(cap=-1, k=0), dict(n_kept=None, k=0), dict(pos=None, k=0),
                # what the k entry refuses, through the shared body
                dict(feats=None), dict(x=None), dict(in_list=None), dict(index=None), dict(attr=None), dict(elabels=0xc0000),
                dict(feats=0x10004), dict(ws=0x100080), dict(index=0x80008), dict(attr=0x90004), dict(n=0), dict(n=46001),
                dict(f=2040), dict(n_cams=0)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_ARG, "build_graph_gated"), bad
    need = lib.mtmc_graph_knn_workspace_bytes(450, 2048)
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=need - 1, k=0)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_WORKSPACE, "build_graph_gated"), bad


def pairs(ei, pos):
    return {(int(a), int(b)) for a, b in ei[:, pos].T}


def test_the_rule_on_nine_nodes_decided_by_hand():
    ei, pos = gate_cases.dense_gate("nine")
    assert ei.shape == (2, 52)
    want = gate_cases.NINE_PAIRS | {(j, i) for i, j in gate_cases.NINE_PAIRS}
    assert len(want) == 20 and pairs(ei, pos) == want
    assert pos.dtype == torch.int64 and torch.all(pos[1:] > pos[:-1])
    s = gate_cases.NINE_STARTS
    for i, j in ((0, 5), (2, 5), (2, 7)):                     # |delta| == max_gap: out (the comparison is strict)
        assert abs(s[i] - s[j]) == 100 and (i, j) not in want
    assert abs(s[1] - s[6]) == 99 and (1, 6) in want and s[1] == s[5] and (1, 5) in want
    assert not {7, 8} & {n for p in want for n in p}          # nodes 7 and 8 are isolated
    assert torch.equal(gate_cases.dense_gate("nine, whole span")[1], torch.arange(52))
    assert gate_cases.dense_gate("nine, nothing kept")[1].numel() == 0


def test_gate_then_k_is_not_the_k_list_filtered_on_nine_nodes():
    """The composition on keys made by hand: key(i, j) = |i - j| / 10.  Node 0's nearest cross-camera node is 3 either way;
    node 2's is 3 without the gate, and 4 among its candidates {4, 6}."""
    ei, pg = gate_cases.dense_gate("nine")
    key = (ei[0] - ei[1]).abs().float() / 10
    assert torch.equal(pg, gate_ref.select(gate_cases.NINE_STARTS, ei, 100))
    composed = pg[knn_ref.select(key[pg], ei[:, pg], gate_cases.NINE_CAMS, 1)]
    kept = pairs(ei, composed)
    assert {(b, a) for a, b in kept} == kept and kept <= pairs(ei, pg) and (2, 4) in kept
    k_list = set(knn_ref.select(key, ei, gate_cases.NINE_CAMS, 1).tolist())
    filtered = sorted(k_list & set(pg.tolist()))
    assert (2, 4) not in pairs(ei, torch.tensor(filtered)) and filtered != composed.tolist()


@pytest.mark.parametrize("name", list(gate_cases.COUNTS))
def test_gated_edge_count_against_the_loop(name):
    from mtmc_mpn import graph_build
    cams, starts, gap, expected = gate_cases.COUNTS[name]
    assert gate_cases.dense_gate(name)[1].numel() == expected
    assert graph_build.gated_edge_count(cams, starts, gap) == expected
    # ... for every kind of input the call accepts, and shifted to both ends of the accepted range
    assert graph_build.gated_edge_count(list(cams), [int(v) for v in starts], np.int64(gap)) == expected
    assert graph_build.gated_edge_count(cams, torch.from_numpy(starts).to(torch.int32), gap) == expected
    top = graph_build.FRAME_LIMIT
    assert top == 1 << 62
    assert graph_build.gated_edge_count(cams, starts - starts.max() + top, gap) == expected
    assert graph_build.gated_edge_count(cams, starts - starts.min() - top, gap) == expected


def test_gated_edge_count_at_the_ends_of_int64():
    """Starts at -2^62 and 2^62 lie 2^63 apart, more than any int64 gap: the count must not wrap."""
    from mtmc_mpn import graph_build
    top = graph_build.FRAME_LIMIT
    cams, starts = [0, 1, 0, 1], [-top, top, top - 5, -top + 5]
    assert graph_build.gated_edge_count(cams, starts, (1 << 63) - 1) == 2 * 3      # all cross pairs but (0, 1)
    assert graph_build.gated_edge_count(cams, starts, 5) == 0
    assert graph_build.gated_edge_count(cams, starts, 6) == 2 * 2                  # (0, 3) and (1, 2), each 5 apart


def test_gated_edge_count_refusals():
    from mtmc_mpn import graph_build
    cams, starts = gate_cases.NINE_CAMS, gate_cases.NINE_STARTS
    for gap in (0, -1, 2.5, "3", True, None, 1 << 63):
        with pytest.raises(RuntimeError, match="max_gap"):
            graph_build.gated_edge_count(cams, starts, gap)
    big = starts.astype(object)
    big[3] = (1 << 63) - 1
    for frames in (starts[:8], starts.astype(np.float32), starts > 100, [0.5] * 9, starts.reshape(3, 3),
                   np.where(np.arange(9) == 3, (1 << 63) - 1, starts), list(big), np.where(np.arange(9) == 3, -(1 << 62) - 1, starts),
                   torch.from_numpy(starts).double()):
        with pytest.raises(RuntimeError, match="start"):
            graph_build.gated_edge_count(cams, frames, 100)
