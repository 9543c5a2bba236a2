"""CPU: the focal-loss entry points are declared and bound, they and `mtmc_mpn.edge_loss(gamma=...)` / `focal_loss` refuse what
they must, and the fp64 yardstick of the GPU tests (focal_ref) equals edge_loss_ref at gamma = 0, the reference's own
FocalLoss_binary rows (tests/golden/focal_binary.npz) and the gradient form the kernels use.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from abi_refusal import refused
from edge_loss_ref import edge_loss_ref
from focal_ref import focal_ref, focal_weighted_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtmc_edge_focal_forward", "mtmc_edge_focal_backward"]


def test_entry_points_are_declared_and_bound():
    import mtmc_mpn
    from mtmc_mpn import _lib
    header = open(os.path.join(ROOT, "include", "mtmc_mpn.h")).read()
    declared = set(re.findall(r"\b(mtmc_[a-z_0-9]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert "#define MTMC_MPN_ABI_VERSION 6" in header                 # additive: the ABI version stays
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NEW[0]) and hasattr(ctypes.CDLL(_lib.LIB_PATH), NEW[1])
    # the plain entries' arguments plus (gamma, per_row) resp. (gamma, grad_per_row), the stream last
    fwd, bwd = lib.mtmc_edge_focal_forward.argtypes, lib.mtmc_edge_focal_backward.argtypes
    assert len(fwd) == 16 and fwd[:13] == lib.mtmc_edge_loss_forward.argtypes[:13] and fwd[13] is ctypes.c_float
    assert len(bwd) == 11 and bwd[:8] == lib.mtmc_edge_loss_backward.argtypes[:8] and bwd[8] is ctypes.c_float
    assert bwd[9] is ctypes.c_int32
    assert {"focal_loss", "FocalLoss", "edge_loss"} <= set(mtmc_mpn.__all__)
    assert mtmc_mpn.focal_loss is mtmc_mpn.ops.focal_loss and mtmc_mpn.FocalLoss is mtmc_mpn.ops.FocalLoss


def test_argument_errors_are_refused_before_any_launch():
    """MTMC_E_ARG with host values only (every check precedes the first HIP call); each refusal names its entry point."""
    from mtmc_mpn import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 1024)()                       # 8-byte aligned host memory: only its address is looked at
    p = ctypes.addressof(buf)
    need = lib.mtmc_edge_loss_scratch_bytes(3)

    def fwd(logits=p, labels=p, n=10, c=2, s=3, mode=0, weight=None, scratch=p, nbytes=need, record=p, out=p, conf=p, gamma=2.0):
        return lib.mtmc_edge_focal_forward(logits, labels, n, c, s, mode, weight, 0.0, scratch, nbytes, record, out, conf,
                                           gamma, None, None)
    for bad in (dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=-float("inf")),
                dict(c=0), dict(c=3), dict(s=0), dict(n=-1), dict(logits=None), dict(labels=None), dict(scratch=None),
                dict(record=None), dict(out=None), dict(conf=None), dict(mode=3), dict(mode=-1), dict(mode=1, weight=None),
                dict(logits=p + 4), dict(nbytes=need - 8)):
        assert refused(lib, lambda: fwd(**bad), _lib.E_ARG, "edge_focal_forward"), bad

    def bwd(logits=p, labels=p, n=10, c=2, s=3, grad=p, record=p, d=p, gamma=2.0, per_row=0):
        return lib.mtmc_edge_focal_backward(logits, labels, n, c, s, grad, record, d, gamma, per_row, None)
    for bad in (dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=-0.5, per_row=1),
                dict(c=0), dict(c=4), dict(s=0), dict(n=-1), dict(logits=None), dict(labels=None), dict(grad=None),
                dict(record=None), dict(d=None), dict(logits=p + 4), dict(d=p + 4)):
        assert refused(lib, lambda: bwd(**bad), _lib.E_ARG, "edge_focal_backward"), bad


def test_python_refusals():
    import mtmc_mpn
    y = torch.zeros(4, dtype=torch.long)
    x2, x1 = torch.zeros(4, 2), torch.zeros(4, 1)
    for bad in (-1, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            mtmc_mpn.edge_loss([x2], y, gamma=bad)
        with pytest.raises(ValueError, match="gamma"):
            mtmc_mpn.focal_loss(x1, y, gamma=bad)
    # the refusals of edge_loss hold with gamma = 2
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.edge_loss([x2], y, gamma=2.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.edge_loss([x1], y.float(), pos_weight="balanced", gamma=2.0)
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 3)], y, gamma=2.0)
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2, dtype=torch.float64)], y, gamma=2.0)
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([x2], torch.zeros(5, dtype=torch.long), gamma=2.0)
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([x2, x1], y, gamma=2.0)
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([x2], y, pos_weight=2.0, gamma=2.0)
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([x1], y, weight=torch.ones(2), gamma=2.0)
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([x2], y, weight="balance", gamma=2.0)
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([], y, gamma=2.0)
    # focal_loss and the module: the same, and the reduction
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.focal_loss(x2, y)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.focal_loss(x1, y, reduction="none")
    with pytest.raises(ValueError):
        mtmc_mpn.focal_loss(x2, y, reduction="avg")
    with pytest.raises(NotImplementedError):
        mtmc_mpn.focal_loss(torch.zeros(4, 3), y)
    with pytest.raises(ValueError):
        mtmc_mpn.focal_loss(x2, y, pos_weight=2.0)
    with pytest.raises(ValueError):
        mtmc_mpn.FocalLoss(alpha=1.5)
    with pytest.raises(ValueError):
        mtmc_mpn.FocalLoss(alpha=1.0)(x1, y)                          # one logit: pos_weight = alpha / (1 - alpha)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.FocalLoss(gamma=2, alpha=0.25)(x2, y)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.FocalLoss(gamma=2, alpha=0.25, reduction="none")(x1, y)


def _inputs(e, s, c, seed, positives=0.02):
    g = torch.Generator().manual_seed(seed)
    steps = [(torch.randn(e, c, generator=g, dtype=torch.float64) * 3).requires_grad_(True) for _ in range(s)]
    y = (torch.rand(e, generator=g) < positives).long()
    y[::53] = -100
    y[1], y[2] = 1, 0                                      # neither class empty
    return steps, y


@pytest.mark.parametrize("c", [2, 1])
def test_yardstick_at_gamma_0_is_edge_loss_ref(c):
    steps, y = _inputs(5003, 3, c, seed=c)
    modes = [dict(), dict(weight="balanced"), dict(weight=torch.tensor([0.7, 4.2]))] if c == 2 else \
            [dict(), dict(pos_weight="balanced"), dict(pos_weight=torch.tensor([4.2]))]
    for kw in modes:
        a = focal_ref(steps, y, 0.0, fpr_alpha=1.0, **kw)
        b = edge_loss_ref(steps, y, fpr_alpha=1.0, **kw)
        assert abs(float(a.loss.detach()) - float(b.loss.detach())) <= 1e-12 * max(1.0, abs(float(b.loss.detach())))
        for name in ("class_loss", "class_prob", "fpr", "class_weight"):
            assert (getattr(a, name) - getattr(b, name)).abs().max().item() <= 1e-12, (kw, name)
        assert torch.equal(a.confusion, b.confusion)
        ga = torch.autograd.grad(a.loss, steps)
        gb = torch.autograd.grad(b.loss, steps)
        assert max((u - v).abs().max().item() for u, v in zip(ga, gb)) <= 1e-12


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "focal_binary.npz"))


def test_yardstick_against_the_references_focal_loss_binary():
    """balance * f == utils.FocalLoss_binary(gamma, balance, reduction='none') of the reference, row by row."""
    g = golden()
    x, t = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["t"])
    assert x.numel() >= 300 and set(t.tolist()) == {0.0, 1.0}
    assert {0.0, 80.0, -80.0} <= set(x.tolist())
    for gamma, balance in g["settings"].tolist():
        want = torch.from_numpy(g[f"rows_g{int(gamma)}"])
        assert want.dtype == torch.float64
        got = balance * focal_weighted_rows(x.view(-1, 1), t.long(), gamma)
        assert (got - want).abs().max().item() <= 1e-12, gamma


def margin_gradient(x, y, gamma):
    """d f / d x by the factored margin form of the kernels, fp64: -q^gamma (gamma p l + q) * d z / d x."""
    if x.shape[1] == 2:
        z = torch.where(y == 1, x[:, 1] - x[:, 0], x[:, 0] - x[:, 1])
    else:
        z = torch.where(y == 1, x[:, 0], -x[:, 0])
    e = torch.exp(-z.abs())
    l = (-z).clamp(min=0) + torch.log1p(e)
    p = torch.where(z >= 0, 1 / (1 + e), e / (1 + e))
    q = torch.where(z >= 0, e / (1 + e), 1 / (1 + e))
    dz = -q ** gamma * (gamma * p * l + q)
    sign = torch.where(y == 1, 1.0, -1.0).double()
    if x.shape[1] == 2:
        return torch.stack([-sign * dz, sign * dz], 1)
    return (sign * dz).view(-1, 1)


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
def test_yardstick_gradient_is_the_factored_margin_form(gamma, c):
    """autograd of focal_ref == -w q^gamma (gamma p l + q) / D, rows at +-80 (margins +-160 for two logits) included."""
    steps, y = _inputs(2003, 2, c, seed=10 + c, positives=0.2)
    with torch.no_grad():
        for x in steps:
            x[5::29] = torch.tensor([80.0, -80.0])[:c] if c == 2 else 80.0
            x[7::31] = torch.tensor([-80.0, 80.0])[:c] if c == 2 else -80.0
    kw = dict(weight=torch.tensor([0.7, 4.2])) if c == 2 else dict(pos_weight=torch.tensor([4.2]))
    r = focal_ref(steps, y, gamma, **kw)
    got = torch.autograd.grad(r.loss, steps)
    keep = (y == 0) | (y == 1)
    n0, n1 = int((y == 0).sum()), int((y == 1).sum())
    w = r.class_weight
    d = float(w[0]) * n0 + float(w[1]) * n1 if c == 2 else n0 + n1
    for x, g in zip(steps, got):
        want = torch.zeros_like(g)
        yk = y[keep]
        want[keep] = margin_gradient(x.detach()[keep], yk, gamma) * w[yk].view(-1, 1) / d
        assert torch.isfinite(g).all()
        assert (g - want).abs().max().item() <= 1e-9 * want.abs().max().item()
        assert (g[~keep] == 0).all()
