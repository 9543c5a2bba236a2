"""mtmc_mpn.edge_loss(gamma > 0), focal_loss and FocalLoss (row loss q^gamma * softplus(-z) in the edge-loss pass, HIP forward
and backward) against focal_ref: the textbook focal loss in fp64 torch on the same inputs.

Bars: those of test_gpu_edge_loss.py -- fields <= BAR * max(1, |ref|), gradients <= BAR * max|grad_ref|, confusion counts
exactly -- with BAR = max(2e-6, 4 x the same ratio of the kernels' margin formula evaluated by torch in fp32 on the CPU
(margin_fp32 below) against the yardstick on the same inputs): the rule test_gpu_parity.py holds the forward to.  Every
comparison prints its worst ratios (device, and fp32 CPU) per gamma; DESIGN.md 3.5b keeps the table."""
import copy
import os

import numpy as np
import pytest
import torch

import mtmc_mpn
from edge_loss_cases import DEV, make_inputs, nodrop, one_logit_params, to_gpu, weight_modes
from focal_ref import class_weights, focal_ref, focal_weighted_rows
from golden_util import ARCH
from mtmc_mpn import graphs

pytestmark = pytest.mark.gpu
FLOOR = 2e-6
FIELDS = ("loss", "class_loss", "class_prob", "fpr", "class_weight")
GAMMAS = (0.5, 1.0, 2.0, 5.0)


def margin_fp32(x, y, gamma, up, ref, weight=None, pos_weight=None, fpr_alpha=0.0):
    """The kernels' arithmetic in torch fp32 on the CPU: z, e = exp(-|z|), l, p, q as el_row, f = q^gamma l, d f / d z =
    -q^gamma (gamma p l + q), fp64 sums.  Returns (fields, gradient); counts and FPR, which are exact, are the yardstick's."""
    s, _, c = x.shape
    keep = (y == 0) | (y == 1)
    yk = y[keep]
    m1 = yk == 1
    m0 = ~m1
    n0, n1 = int(m0.sum()), int(m1.sum())
    w = class_weights(c, n0, n1, weight, pos_weight)
    d = float(w[0]) * n0 + float(w[1]) * n1 if c == 2 else float(n0 + n1)
    gw = torch.where(m1, torch.tensor(up / d * float(w[1])).float(), torch.tensor(up / d * float(w[0])).float())
    sign = torch.where(m1, 1.0, -1.0)
    grad = torch.zeros_like(x)
    loss, class_loss, class_prob = 0.0, [], []
    for i in range(s):
        xs = x[i][keep]
        z = sign * (xs[:, 1] - xs[:, 0] if c == 2 else xs[:, 0])
        e = torch.exp(-z.abs())
        inv = 1.0 / (1.0 + e)
        l = (-z).clamp(min=0) + torch.log1p(e)
        p, q = torch.where(z >= 0, inv, e * inv), torch.where(z >= 0, e * inv, inv)
        m = q.pow(gamma)
        assert m.dtype == torch.float32
        f, pd = (m * l).double(), p.double()
        dz = gw * (-m * (gamma * p * l + q)) * sign
        grad[i][keep] = torch.stack([-dz, dz], 1) if c == 2 else dz.view(-1, 1)
        f0, f1 = f[m0].sum().item(), f[m1].sum().item()
        loss += (float(w[0]) * f0 + float(w[1]) * f1) / d
        class_loss.append([f0 / n0 if n0 else 0.0, f1 / n1 if n1 else 0.0])
        class_prob.append([pd[m0].sum().item() / n0 if n0 else 0.5, pd[m1].sum().item() / n1 if n1 else 0.5])
    fields = dict(loss=torch.tensor(loss + fpr_alpha * float(ref.fpr.sum())), class_loss=torch.tensor(class_loss),
                  class_prob=torch.tensor(class_prob), fpr=ref.fpr, class_weight=w.float())
    return fields, grad


def ratios(fields, grad, ref, ref_grad):
    """(worst field error / max(1, |ref|), gradient error / max|grad_ref|)"""
    worst = 0.0
    for name in FIELDS:
        got, want = fields[name].detach().cpu().double(), getattr(ref, name).detach().double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if got.numel():
            worst = max(worst, ((got - want).abs() / want.abs().clamp(min=1.0)).max().item())
    scale = ref_grad.abs().max().item()
    return worst, ((grad.cpu().double() - ref_grad).abs().max().item() / scale if scale > 0 else 0.0)


def run_ours(x, y, up=1.7, **kw):
    block = x.to(DEV).requires_grad_(True)
    r = mtmc_mpn.edge_loss([block[i] for i in range(block.shape[0])], y.to(DEV), **kw)
    (r.loss * up).backward()
    return r, block.grad


def run_ref(x, y, gamma, up=1.7, **kw):
    xb = x.double().requires_grad_(True)
    kw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    ref = focal_ref([xb[i] for i in range(xb.shape[0])], y, gamma, **kw)
    (ref.loss * up).backward()
    return ref, xb.grad


def check(x, y, gamma, tag, up=1.7, **kw):
    """One call against the yardstick at the bar; returns the four ratios (device fields, device grad, fp32 fields, fp32 grad)."""
    r, grad = run_ours(x, y, up=up, gamma=gamma, **kw)
    ref, ref_grad = run_ref(x, y, gamma, up=up, **kw)
    cpu_kw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    f32, g32 = ratios(*margin_fp32(x, y, gamma, up, ref, **cpu_kw), ref, ref_grad)
    s = ref.confusion.shape[0]
    assert r.loss.dtype == torch.float32 and r.loss.dim() == 0 and r.confusion.dtype == torch.int64
    assert r.class_loss.shape == (s, 2) and r.class_prob.shape == (s, 2) and r.fpr.shape == (s,) and r.class_weight.shape == (2,)
    assert torch.equal(r.confusion.cpu(), ref.confusion), (tag, r.confusion.cpu().tolist(), ref.confusion.tolist())
    assert torch.isfinite(grad).all().item(), tag
    fd, gd = ratios(r._asdict(), grad, ref, ref_grad)
    assert fd <= max(FLOOR, 4 * f32), f"{tag} fields: {fd:.3e} of max(1, |ref|); fp32 on the CPU: {f32:.3e}"
    assert gd <= max(FLOOR, 4 * g32), f"{tag} grad: {gd:.3e} of max|grad_ref|; fp32 on the CPU: {g32:.3e}"
    return fd, gd, f32, g32


def check_all_modes(x, y, gamma, tag):
    worst = [0.0] * 4
    for kw in weight_modes(x.shape[2]):
        for alpha in (0.0, 1.0):
            got = check(x, y, gamma, f"{tag} {sorted(kw)} alpha={alpha}", fpr_alpha=alpha, **kw)
            worst = [max(a, b) for a, b in zip(worst, got)]
    return worst


def report(gamma, c, worst):
    print(f"\nfocal worst ratios gamma={gamma} C={c}: device fields {worst[0]:.2e} grad {worst[1]:.2e} | "
          f"fp32 CPU fields {worst[2]:.2e} grad {worst[3]:.2e}")


def balanced(c):
    return dict(weight="balanced") if c == 2 else dict(pos_weight="balanced")


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_matches_the_fp64_yardstick(gamma, c):
    """E in {1, 63, 257, 20011} x S in {1, 3}, every weight mode, with and without the FPR term."""
    worst = [0.0] * 4
    for e in (1, 63, 257, 20011):
        for s in (1, 3):
            x, y = make_inputs(e, s, c, seed=1000 * c + 10 * e + s)
            worst = [max(a, b) for a, b in zip(worst, check_all_modes(x, y, gamma, f"gamma={gamma} E={e} S={s} C={c}"))]
    report(gamma, c, worst)


@pytest.mark.parametrize("c", [2, 1])
def test_gamma_0_is_the_plain_loss_bit_for_bit(c):
    x, y = make_inputs(20011, 3, c, seed=61 + c)
    for kw in weight_modes(c):
        a, ga = run_ours(x, y, fpr_alpha=1.0, gamma=0.0, **kw)
        b, gb = run_ours(x, y, fpr_alpha=1.0, **kw)
        for name in a._fields:
            assert torch.equal(getattr(a, name), getattr(b, name)), (sorted(kw), name)
        assert torch.equal(ga, gb), sorted(kw)


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("e, s", [(65, 1025), (140003, 3)])
def test_grid_edges(e, s, c):
    """S = 1025: one step more than the grid's y dimension takes, so a workgroup reduces two steps; E = 140 003: past the
    forward's 512-workgroup cap, so the row loop strides."""
    x, y = make_inputs(e, s, c, seed=900 + 10 * c + s)
    r, _ = run_ours(x, y, gamma=2.0, fpr_alpha=1.0, **balanced(c))
    assert r.confusion.shape == (s, 4) and r.confusion.sum(1).tolist() == [int(((y == 0) | (y == 1)).sum())] * s
    report(2.0, c, check(x, y, 2.0, f"E={e} S={s} C={c}", fpr_alpha=1.0, **balanced(c)))


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("only", ["0", "1"])
def test_one_class_only(only, c):
    """All labels 0 / all labels 1: balanced falls back to (1, 1), the empty class reports 0 / 0.5, the loss is finite."""
    x, y = make_inputs(257, 3, c, seed=5 + c, labels=only)
    check_all_modes(x, y, 2.0, f"only {only} C={c}")
    r = mtmc_mpn.edge_loss(list(x.to(DEV)), y.to(DEV), fpr_alpha=1.0, gamma=2.0, **balanced(c))
    empty = 1 - int(only)
    assert r.class_weight.tolist() == [1.0, 1.0]
    assert r.class_loss[:, empty].tolist() == [0.0] * 3 and r.class_prob[:, empty].tolist() == [0.5] * 3
    assert torch.isfinite(r.loss).item()


def test_no_counted_row_at_all():
    x, _ = make_inputs(63, 2, 2, seed=3)
    r, grad = run_ours(x, torch.full((63,), -100, dtype=torch.long), gamma=2.0)
    assert torch.isnan(r.loss).item() and r.confusion.sum().item() == 0 and (grad == 0).all().item()


@pytest.mark.parametrize("c", [2, 1])
def test_float_labels(c):
    x, y = make_inputs(20011, 3, c, seed=21)
    a, ga = run_ours(x, y.float(), gamma=2.0, fpr_alpha=1.0, **balanced(c))
    b, gb = run_ours(x, y, gamma=2.0, fpr_alpha=1.0, **balanced(c))
    for name in a._fields:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(ga, gb)


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("gamma", [0.5, 5.0])
def test_extreme_margins_only(gamma, c):
    """Nothing but rows at +-80 (margins +-160 with two logits), correctly and wrongly labelled: everything finite, at the
    bar, and where q^gamma is 0 in fp32 (q = 0: margin +160; q = 2e-35 at gamma 5) the gradient is exactly 0."""
    e = 257
    x = torch.empty(2, e, c)
    x[:, 0::2] = torch.tensor([80.0, -80.0])[:c]
    x[:, 1::2] = torch.tensor([-80.0, 80.0])[:c]
    y = torch.tensor([0, 0, 1, 1] * e)[:e]                              # row pattern: right, wrong, wrong, right (C = 2)
    y[11::37] = -100
    for kw in weight_modes(c):
        check(x, y, gamma, f"+-80 only gamma={gamma} C={c} {sorted(kw)}", **kw)
        r, grad = run_ours(x, y, gamma=gamma, **kw)
        for t in r:
            assert torch.isfinite(t.float()).all().item()
        assert torch.isfinite(grad).all().item()
        z = torch.where(y == 1, 1.0, -1.0) * (x[..., 1] - x[..., 0] if c == 2 else x[..., 0])
        q = torch.exp(-z.abs()) / (1 + torch.exp(-z.abs()))
        dead = (z > 0) & (q.pow(gamma) == 0) & (y != -100)
        assert dead.any().item() or (c == 1 and gamma == 0.5)
        assert (grad.cpu()[dead] == 0).all().item()
        wrong = (z < 0) & (y != -100)
        assert (grad.cpu()[wrong].abs().sum(-1) > 0).all().item()        # and the wrong rows do get one


# ---- focal_loss / FocalLoss ------------------------------------------------------------------------------------------
def bar_rows(x, y, gamma, want, **kw):
    """The file's bar for per-row values: 4 x what the margin formula in fp32 on the CPU misses them by, or the floor."""
    keep = (y == 0) | (y == 1)
    sign = torch.where(y == 1, 1.0, -1.0)
    z = sign * (x[:, 1] - x[:, 0] if x.shape[1] == 2 else x[:, 0])
    e = torch.exp(-z.abs())
    l = (-z).clamp(min=0) + torch.log1p(e)
    q = torch.where(z >= 0, e / (1 + e), 1 / (1 + e))
    w = class_weights(x.shape[1], int((y == 0).sum()), int((y == 1).sum()), kw.get("weight"), kw.get("pos_weight")).float()
    rows = torch.where(keep, w[y.clamp(min=0)] * (q.pow(gamma) * l), torch.zeros(()))
    return max(FLOOR, 4 * ((rows.double() - want).abs() / want.abs().clamp(min=1.0)).max().item())


def check_reductions(x, y, gamma, c):
    """focal_loss "mean" against edge_loss, "none" and "sum" with their gradients (the per-row backward) against focal_ref."""
    xd, yd = x.to(DEV), y.to(DEV)
    for kw in weight_modes(c):
        cpu_kw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        mean = mtmc_mpn.focal_loss(xd, yd, gamma, **kw)
        assert torch.equal(mean, mtmc_mpn.edge_loss([xd], yd, gamma=gamma, **kw).loss)
        xr = x.double().requires_grad_(True)
        want = focal_weighted_rows(xr, y, gamma, **cpu_kw)
        up = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(9), dtype=torch.float64)
        (want * up).sum().backward()
        bar = bar_rows(x, y, gamma, want.detach(), **cpu_kw)
        xg = xd.clone().requires_grad_(True)
        rows = mtmc_mpn.focal_loss(xg, yd, gamma, reduction="none", **kw)
        assert rows.shape == (x.shape[0],) and rows.dtype == torch.float32
        assert (rows[yd == -100] == 0).all().item()
        err = ((rows.detach().cpu().double() - want.detach()).abs() / want.detach().abs().clamp(min=1.0)).max().item()
        assert err <= bar, f"none {sorted(kw)}: {err:.3e} > {bar:.3e}"
        rows.backward(up.float().to(DEV))
        gerr = (xg.grad.cpu().double() - xr.grad).abs().max().item() / xr.grad.abs().max().item()
        assert gerr <= bar, f"none backward {sorted(kw)}: {gerr:.3e} > {bar:.3e}"
        print(f"\nfocal_loss none gamma={gamma} C={c} {sorted(kw)}: rows {err:.2e} grad {gerr:.2e} bar {bar:.2e}")
        xs = xd.clone().requires_grad_(True)
        total = mtmc_mpn.focal_loss(xs, yd, gamma, reduction="sum", **kw)
        wsum = want.detach().sum().item()
        assert total.dim() == 0 and abs(total.item() - wsum) <= bar * max(1.0, abs(wsum))
        total.backward()
        xr2 = x.double().requires_grad_(True)
        focal_weighted_rows(xr2, y, gamma, **cpu_kw).sum().backward()
        assert (xs.grad.cpu().double() - xr2.grad).abs().max().item() <= bar * xr2.grad.abs().max().item()


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("gamma", [2.0, 5.0])
def test_focal_loss_reductions(gamma, c):
    x, y = make_inputs(20011, 1, c, seed=71 + c)
    check_reductions(x[0], y, gamma, c)


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("e", [1, 63, 257])
def test_focal_loss_reductions_at_wave_and_workgroup_edges(e, c):
    """The rows kernel and the per-row backward on one row, just under one wave, and one row past a workgroup."""
    x, y = make_inputs(e, 1, c, seed=71 + 10 * e + c)
    check_reductions(x[0], y, 2.0, c)


def test_focal_loss_module():
    x, y = make_inputs(5003, 1, 2, seed=81)
    xd, yd = x[0].to(DEV), y.to(DEV)
    got = mtmc_mpn.FocalLoss(gamma=2, alpha=0.25)(xd, yd)
    assert torch.equal(got, mtmc_mpn.focal_loss(xd, yd, 2.0, weight=torch.tensor([0.75, 0.25], device=DEV)))
    assert torch.equal(mtmc_mpn.FocalLoss(gamma=2, alpha="balanced")(xd, yd), mtmc_mpn.focal_loss(xd, yd, 2.0, weight="balanced"))
    w = torch.tensor([0.3, 1.9], device=DEV)
    assert torch.equal(mtmc_mpn.FocalLoss(gamma=1.5, alpha=w, reduction="sum")(xd, yd),
                       mtmc_mpn.focal_loss(xd, yd, 1.5, weight=w, reduction="sum"))
    # one logit: the weights (1 - a, a) as pos_weight = a / (1 - a), times (1 - a)
    x1, y1 = make_inputs(5003, 1, 1, seed=82)
    x1d, y1d = x1[0].to(DEV), y1.to(DEV)
    rows = mtmc_mpn.FocalLoss(gamma=2, alpha=0.25, reduction="none")(x1d, y1d)
    want = focal_weighted_rows(x1[0].double(), y1, 2.0, pos_weight=torch.tensor([1.0 / 3.0])) * 0.75
    assert (rows.cpu().double() - want).abs().max().item() <= FLOOR * max(1.0, want.abs().max().item())
    both = mtmc_mpn.FocalLoss(gamma=2, alpha=torch.tensor([0.75, 0.25]), reduction="none")(x1d, y1d)
    assert (both - rows).abs().max().item() <= FLOOR * max(1.0, want.abs().max().item())


def test_one_logit_rows_against_the_references_focal_loss_binary():
    """0.9 * focal_loss(x, t, gamma=5, reduction="none") == utils.FocalLoss_binary(5, 0.9, 'none') of the reference
    (tests/golden/focal_binary.npz), and the (2, 0.25) setting; float 0/1 targets as the reference passes them."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focal_binary.npz"))
    x, t = torch.from_numpy(g["x"]).view(-1, 1), torch.from_numpy(g["t"])
    for gamma, balance in g["settings"].tolist():
        want = torch.from_numpy(g[f"rows_g{int(gamma)}"])
        got = balance * mtmc_mpn.focal_loss(x.to(DEV), t.to(DEV), gamma=gamma, reduction="none")
        bar = bar_rows(x, t.long(), gamma, want / balance)
        err = ((got.cpu().double() - want).abs() / want.abs().clamp(min=1.0)).max().item()
        print(f"\nFocalLoss_binary rows gamma={gamma}: {err:.2e} bar {bar:.2e}")
        assert err <= bar, (gamma, err, bar)


# ---- on a model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 1])
def test_model_gradients_against_fp64_autograd(c):
    """Dropout off, training mode: all 34 parameter gradients of edge_loss(gamma=2, balanced) against fp64 CPU autograd of the
    oracle under the yardstick, at the bar of test_one_logit_model_gradients_against_fp64_autograd."""
    from oracle import mpn_oracle
    d = graphs.camera_graph((12, 9, 10), seed=3)
    params = one_logit_params() if c == 1 else nodrop(mtmc_mpn.default_params(num_enc_steps=3, num_class_steps=3))
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH)
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    labels = (torch.rand(d.edge_index.shape[1], generator=torch.Generator().manual_seed(1)) < 0.2).long()
    out, _ = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, d.x, d.edge_index, d.edge_attr, training=True,
                                dtype=torch.float64)
    want_loss = focal_ref(out["classified_edges"], labels, 2.0, **balanced(c)).loss
    want_loss.backward()
    m = m.cuda().train()
    got, _ = m(to_gpu(d))
    assert got["classified_edges"][0].shape[1] == c
    r = mtmc_mpn.edge_loss(got["classified_edges"], labels.cuda(), gamma=2.0, **balanced(c))
    r.loss.backward()
    assert abs(r.loss.item() - want_loss.item()) <= 2e-5 * max(1.0, abs(want_loss.item()))
    named = list(m.named_parameters())
    assert len(named) == 34
    for k, p in named:
        want = sd[k].grad
        assert p.grad is not None and want is not None, k
        err = (p.grad.cpu().double() - want).abs().max().item()
        floor = 1e-6 + 2e-4 * want.abs().max().item()
        assert err <= floor, f"{k}: |dgrad| {err:.3e} > {floor:.3e} (|grad|max {want.abs().max().item():.3e})"


def test_captured_training_step_with_focal_loss():
    """test_captured_training_step_with_edge_loss with gamma = 2 inside the HIP graph: the replayed losses follow the eager
    steps of a twin model, and the counts of the last replay are whole."""
    d = graphs.camera_graph((30, 25, 28), seed=6)
    params = mtmc_mpn.default_params(num_enc_steps=2, num_class_steps=2)
    g = to_gpu(d)
    labels = (torch.rand(d.edge_index.shape[1], generator=torch.Generator().manual_seed(5)) < 0.15).long().cuda()

    def make():
        torch.manual_seed(0)
        m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).cuda().train()
        m.device_seed = torch.tensor([4242], dtype=torch.int64, device="cuda")
        return m, torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, fused=True)
    kept = {}

    def loss_fn(o, _h):
        r = mtmc_mpn.edge_loss(o["classified_edges"], labels, weight="balanced", fpr_alpha=1.0, gamma=2.0)
        kept["confusion"] = r.confusion                         # (not differentiable: holds no autograd graph)
        return r.loss
    m1, opt1 = make()
    replay = m1.capture_training_step(g, loss_fn, opt1, warmup=3)
    captured = kept["confusion"]
    assert int(m1.device_seed.item()) == 4242 + 3
    losses = [float(replay()) for _ in range(4)]
    assert int(m1.device_seed.item()) == 4242 + 7
    assert captured.shape == (2, 4) and captured.sum(1).tolist() == [labels.numel()] * 2     # n0 + n1 in every row
    m2, opt2 = make()
    eager = []
    for _ in range(7):
        opt2.zero_grad(set_to_none=True)
        out, h = m2(g)
        loss = loss_fn(out, h)
        loss.backward()
        opt2.step()
        eager.append(float(loss))
    assert len(set(losses)) == 4
    for a, b in zip(losses, eager[3:]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (losses, eager)
    for (k, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p - q).abs().max().item() <= 2e-3 * max(q.abs().max().item(), 1e-3), k
