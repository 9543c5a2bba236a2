"""CPU: the k-nearest graph builder's C ABI (declared, exported, sized and argument-checked without a GPU) and the
selection rule's CPU restatement (tests/knn_ref.py) on a case small enough to rank by hand."""
import ctypes
import os
import re

import numpy as np
import torch

import knn_ref
from abi_refusal import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtmc_graph_knn_workspace_bytes", "mtmc_build_graph_knn")


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "#define MTMC_MPN_ABI_VERSION 6" in header and _lib.load().mtmc_mpn_abi_version() == 6
    assert "inference.py:407-456" in header
    assert "| `mtmc_build_graph_knn`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_workspace_query_needs_no_gpu():
    from mtmc_mpn import _lib
    lib = _lib.load()
    q, dense = lib.mtmc_graph_knn_workspace_bytes, lib.mtmc_graph_workspace_bytes
    assert q(0, 2048) == 0 and q(-3, 2048) == 0 and q(46001, 2048) == 0 and q(450, 0) == 0 and q(450, 31) == 0
    for n, f in ((1, 32), (9, 64), (450, 2048), (2000, 64), (8000, 2048), (46000, 2048)):
        assert q(n, f) >= dense(n, f) > 0, (n, f)
        # beyond the dense builder's workspace: a bit matrix of N^2 / 8 bytes and 8 bytes per node, no dense-sized edge array
        assert q(n, f) - dense(n, f) <= n * n // 8 + 8 * n + 3 * 256, (n, f)


def call(lib, **kw):
    n, f, e = 450, 2048, 150454
    a = dict(feats=0x10000, stride=f, n=n, f=f, in_list=0x20000, in_off=0x30000, out_list=0x40000, out_off=0x50000,
             block_off=0x60000, n_cams=4, e=e, labels=None, x=0x70000, index=0x80000, attr=0x90000, elabels=None,
             k=8, cap=7200, pos=0xa0000, n_kept=0xb0000, ws=0x100000, ws_bytes=lib.mtmc_graph_knn_workspace_bytes(n, f))
    a.update(kw)
    return lib.mtmc_build_graph_knn(
        a["feats"], a["stride"], a["n"], a["f"], 1, a["in_list"], a["in_off"], a["out_list"], a["out_off"], a["block_off"],
        a["n_cams"], a["e"], a["labels"], a["x"], a["index"], a["attr"], a["elabels"], a["k"], a["cap"], a["pos"],
        a["n_kept"], a["ws"], a["ws_bytes"], None)


def test_bad_arguments_are_refused_before_any_launch():
    from mtmc_mpn import _lib
    lib = _lib.load()
    for bad in (dict(feats=None), dict(x=None), dict(in_list=None), dict(out_off=None), dict(index=None), dict(attr=None),
                dict(elabels=0xc0000),                          # edge labels without node labels
                dict(feats=0x10004), dict(x=0x70008), dict(stride=2049), dict(ws=0x100080), dict(index=0x80008),
                dict(attr=0x90004), dict(n=0), dict(n=46001), dict(f=2040), dict(f=0), dict(n_cams=0),
                dict(k=0), dict(k=-1), dict(cap=-1), dict(pos=None), dict(n_kept=None)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_ARG, "build_graph_knn"), bad
    for bad in (dict(ws=None), dict(ws_bytes=lib.mtmc_graph_knn_workspace_bytes(450, 2048) - 1), dict(ws_bytes=0)):
        assert refused(lib, lambda: call(lib, **bad), _lib.E_WORKSPACE, "build_graph_knn"), bad


# nine nodes on a line: cameras A = {0, 1, 2}, B = {3, 4}, C = {5, 6, 7, 8}; key(i, j) = |p_i - p_j| / 100
P = np.array([0, 10, 20, 1, 11, 2, 12, 21, 30], dtype=np.float32)
CAMS = np.repeat(np.array([1, 2, 3]), (3, 2, 4))


def line_case():
    from oracle import graph_oracle
    ei = graph_oracle.topology(CAMS)
    assert ei.shape == (2, 52)
    key = torch.from_numpy(np.abs(P[ei[0].numpy()] - P[ei[1].numpy()]) / np.float32(100))
    return key, ei


def test_the_rule_on_nine_nodes_ranked_by_hand():
    key, ei = line_case()
    # nearest cross-camera node of 0..8: 3, 4, 7, 0 (tie with 5 at 0.01: the lower column), 1 (tie with 6), 3, 4, 2, 2
    nearest = {0: 3, 1: 4, 2: 7, 3: 0, 4: 1, 5: 3, 6: 4, 7: 2, 8: 2}
    want = {(i, j) for i, j in nearest.items()} | {(j, i) for i, j in nearest.items()}
    assert len(want) == 12
    pos = knn_ref.select(key, ei, CAMS, 1)
    assert {(int(a), int(b)) for a, b in ei[:, pos].T} == want
    # second nearest of node 3 (1 <- tie broken, then 5 at the same key): k = 2 admits (3, 5), which k = 1 left to 5's own pick
    rank = knn_ref.ranks(key, ei)
    row3 = {int(ei[1, e]): int(rank[e]) for e in range(52) if int(ei[0, e]) == 3}
    assert row3[0] == 0 and row3[5] == 1 and row3[1] == 2


def test_the_rule_is_symmetric_a_subsequence_bounded_and_dense_from_k_6():
    key, ei = line_case()
    pairs = lambda pos: {(int(a), int(b)) for a, b in ei[:, pos].T}
    sizes = []
    for k in (1, 2, 3, 5, 6, 7, 100):
        pos = knn_ref.select(key, ei, CAMS, k)
        assert pos.dtype == torch.int64 and torch.all(pos[1:] > pos[:-1]) and 0 <= int(pos[0]) and int(pos[-1]) < 52
        kept = pairs(pos)
        assert {(b, a) for a, b in kept} == kept
        assert len(pos) <= min(52, 2 * k * 9)
        sizes.append(len(pos))
        if k >= 6:                               # every row of cameras A and C (out-degrees 6 and 5) admits all of B
            assert torch.equal(pos, torch.arange(52))
    assert sizes == sorted(sizes) and sizes[0] == 12 and sizes[1] < 52
    assert knn_ref.select(torch.zeros(0), torch.zeros(2, 0, dtype=torch.int64), np.zeros(5, dtype=int), 3).numel() == 0
