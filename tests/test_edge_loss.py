"""CPU: the edge-loss entry points are declared and bound, `mtmc_mpn.edge_loss` refuses what it must, and the fp64 yardstick
of the GPU tests (edge_loss_ref) equals the reference's piece-by-piece formulation.  No GPU is touched."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from abi_refusal import refused
from edge_loss_ref import edge_loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtmc_edge_loss_scratch_bytes", "mtmc_edge_loss_forward", "mtmc_edge_loss_backward"]


def test_entry_points_are_declared_and_bound():
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert "#define MTMC_MPN_ABI_VERSION 6" in header                 # additive: the ABI version stays
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.mtmc_edge_loss_forward.argtypes) == 14 and len(lib.mtmc_edge_loss_backward.argtypes) == 9
    # the size query is host-only: 16 replicas of 128 bytes per step, nothing for a step count that is refused
    assert lib.mtmc_edge_loss_scratch_bytes(3) == 3 * _lib.STAT_REPLICAS * 128
    assert lib.mtmc_edge_loss_scratch_bytes(0) == 0


def test_argument_errors_are_refused_before_any_launch():
    """MTMC_E_ARG of the C entry points, checked with NULL / host values only (every check precedes the first launch); each
    refusal names its entry point in mtmc_mpn_last_error()."""
    import ctypes
    from mtmc_mpn import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 1024)()                       # 8-byte aligned host memory: only its address is looked at
    p = ctypes.addressof(buf)
    need = lib.mtmc_edge_loss_scratch_bytes(3)

    def fwd(logits=p, labels=p, n=10, c=2, s=3, mode=0, weight=None, scratch=p, nbytes=need, record=p, out=p, conf=p):
        return lib.mtmc_edge_loss_forward(logits, labels, n, c, s, mode, weight, 0.0, scratch, nbytes, record, out, conf, None)
    for bad in (dict(c=0), dict(c=3), dict(s=0), dict(n=-1), dict(logits=None), dict(labels=None), dict(scratch=None),
                dict(record=None), dict(out=None), dict(conf=None), dict(mode=3), dict(mode=-1), dict(mode=1, weight=None),
                dict(logits=p + 4), dict(nbytes=need - 8)):
        assert refused(lib, lambda: fwd(**bad), _lib.E_ARG, "edge_loss_forward"), bad

    def bwd(logits=p, labels=p, n=10, c=2, s=3, grad=p, record=p, d=p):
        return lib.mtmc_edge_loss_backward(logits, labels, n, c, s, grad, record, d, None)
    for bad in (dict(c=0), dict(c=4), dict(s=0), dict(n=-1), dict(logits=None), dict(labels=None), dict(grad=None),
                dict(record=None), dict(d=None), dict(logits=p + 4), dict(d=p + 4)):
        assert refused(lib, lambda: bwd(**bad), _lib.E_ARG, "edge_loss_backward"), bad


def test_edge_loss_refuses():
    import mtmc_mpn
    y = torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.edge_loss([torch.zeros(4, 2)], y)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.edge_loss([torch.zeros(4, 1)], y.float(), pos_weight="balanced")
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 3)], y)                                   # C not in {1, 2}
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2, dtype=torch.float64)], y)              # dtype
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2)], torch.zeros(5, dtype=torch.long))    # labels of another length
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2), torch.zeros(4, 1)], y)                # steps of different shapes
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(8)], torch.zeros(8, dtype=torch.long))
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2)], y, pos_weight=2.0)                   # the one-logit argument on two classes
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 1)], y, weight=torch.ones(2))             # and the other way round
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2)], y, weight="balance")                 # unknown weight string
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 1)], y, pos_weight="auto")
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([], y)
    assert mtmc_mpn.edge_loss is mtmc_mpn.ops.edge_loss and "edge_loss" in mtmc_mpn.__all__


def _inputs(e, s, c, seed, positives=0.02):
    g = torch.Generator().manual_seed(seed)
    steps = [(torch.randn(e, c, generator=g, dtype=torch.float64) * 3).requires_grad_(True) for _ in range(s)]
    y = (torch.rand(e, generator=g) < positives).long()
    y[::53] = -100
    y[1], y[2] = 1, 0                                      # neither class empty
    return steps, y


def test_reference_helper_equals_the_piece_by_piece_balanced_formulation():
    """reference train.py:124-142 restated: per-row CE times w[y], summed, divided by w[y].sum(), w = (1, n0/n1) from the
    counts of the batch -- what edge_loss_ref takes from F.cross_entropy(weight=w) -- and the FPR term of :194-195."""
    steps, y = _inputs(20011, 3, 2, seed=1)
    r = edge_loss_ref(steps, y, weight="balanced", fpr_alpha=1.0)
    keep = (y == 0) | (y == 1)
    yk = y[keep]
    n1 = float(yk.sum())
    n0 = float(len(yk)) - n1
    w = torch.tensor([1.0, n0 / n1], dtype=torch.float64)
    want = 0.0
    for i, x in enumerate(steps):
        xk = x.detach()[keep]
        per = F.cross_entropy(xk, yk, reduction="none")
        want = want + (per * w[yk]).sum() / w[yk].sum()
        pred = torch.argmax(xk, 1)
        fp = float(pred[yk == 0].sum())
        tn = float((yk == 0).sum()) - fp
        want = want + fp / (fp + tn)
        assert abs(fp / (fp + tn) - float(r.fpr[i])) <= 1e-12
        assert r.confusion[i].tolist() == [int(pred[yk == 1].sum()), int(fp), int(tn), int((yk == 1).sum() - pred[yk == 1].sum())]
        for cls in (0, 1):
            assert abs(float(per[yk == cls].mean()) - float(r.class_loss[i, cls])) <= 1e-12
            # the weighted shares of the training branch (train.py:131-142) follow from the class means
            share = float((per * w[yk])[yk == cls].sum() / w[yk].sum())
            assert abs(share - float(w[cls]) * float(r.class_loss[i, cls]) * (n0, n1)[cls] / (n0 + n1 * float(w[1]))) <= 1e-12
    assert abs(float(r.loss.detach()) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert torch.equal(r.class_weight, w)


def test_reference_helper_one_logit_and_the_empty_class_fillers():
    steps, y = _inputs(5003, 2, 1, seed=2)
    r = edge_loss_ref(steps, y, pos_weight="balanced")
    keep = (y == 0) | (y == 1)
    t = y[keep].double()
    n1 = float(t.sum())
    n0 = float(len(t)) - n1
    want = 0.0
    for x in steps:
        z = x.detach()[keep][:, 0]
        want = want + ((n0 / n1) * t * F.softplus(-z) + (1 - t) * F.softplus(z)).sum() / (n0 + n1)
    assert abs(float(r.loss.detach()) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    # one empty class: balanced falls back to (1, 1); the empty class reports 0 / 0.5; no label-0 rows: FPR 0
    for c in (1, 2):
        steps, y = _inputs(257, 2, c, seed=3)
        kw = dict(weight="balanced") if c == 2 else dict(pos_weight="balanced")
        ones = edge_loss_ref(steps, torch.ones_like(y), fpr_alpha=1.0, **kw)
        zeros = edge_loss_ref(steps, torch.zeros_like(y), fpr_alpha=1.0, **kw)
        assert ones.class_weight.tolist() == [1.0, 1.0] and zeros.class_weight.tolist() == [1.0, 1.0]
        assert ones.class_loss[:, 0].tolist() == [0.0, 0.0] and ones.class_prob[:, 0].tolist() == [0.5, 0.5]
        assert zeros.class_loss[:, 1].tolist() == [0.0, 0.0] and zeros.class_prob[:, 1].tolist() == [0.5, 0.5]
        assert ones.fpr.tolist() == [0.0, 0.0] and ones.confusion[:, 1:3].sum().item() == 0
        assert zeros.confusion[:, [0, 3]].sum().item() == 0 and torch.isfinite(zeros.loss).item()
