"""mtmc_mpn.edge_loss (loss, per-class losses / probabilities, confusion counts and FPR of every classified step in one pass,
fused backward) against edge_loss_ref: torch's own losses in fp64 on the same inputs.

Bars: loss, class_loss, class_prob, fpr <= 2e-6 * max(1, |ref|); gradients <= 2e-6 * max|grad_ref| (the bars test_gpu_loss.py
holds the same fp32 row arithmetic with fp64 sums to); confusion counts exactly."""
import copy

import pytest
import torch
import torch.nn.functional as F

import mtmc_mpn
from edge_loss_cases import DEV, make_inputs, nodrop, one_logit_params, to_gpu, weight_modes
from edge_loss_ref import edge_loss_ref
from golden_util import ARCH
from mtmc_mpn import graphs

pytestmark = pytest.mark.gpu
BAR = 2e-6


def run_ours(x, y, up=1.7, separate=False, **kw):
    block = x.to(DEV).requires_grad_(True)
    if separate:
        steps = [block.detach()[i].clone().requires_grad_(True) for i in range(block.shape[0])]
    else:
        steps = [block[i] for i in range(block.shape[0])]
    r = mtmc_mpn.edge_loss(steps, y.to(DEV), **kw)
    (r.loss * up).backward()
    grad = torch.stack([t.grad for t in steps]) if separate else block.grad
    return r, grad


def run_ref(x, y, up=1.7, **kw):
    xb = x.double().requires_grad_(True)
    kw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    ref = edge_loss_ref([xb[i] for i in range(xb.shape[0])], y, **kw)
    (ref.loss * up).backward()
    return ref, xb.grad


def compare(r, grad, ref, ref_grad, tag):
    def close(got, want, name):
        got, want = got.detach().cpu().double(), torch.as_tensor(want).detach().double()
        assert got.shape == want.shape, (tag, name, got.shape, want.shape)
        err = ((got - want).abs() / want.abs().clamp(min=1.0)).max().item() if got.numel() else 0.0
        assert err <= BAR, f"{tag} {name}: {err:.3e} of max(1, |ref|)"
    s = ref.confusion.shape[0]
    assert r.loss.dtype == torch.float32 and r.loss.dim() == 0 and r.confusion.dtype == torch.int64
    assert r.class_loss.shape == (s, 2) and r.class_prob.shape == (s, 2) and r.fpr.shape == (s,) and r.class_weight.shape == (2,)
    assert torch.equal(r.confusion.cpu(), ref.confusion), (tag, r.confusion.cpu().tolist(), ref.confusion.tolist())
    close(r.loss, ref.loss, "loss")
    close(r.class_loss, ref.class_loss, "class_loss")
    close(r.class_prob, ref.class_prob, "class_prob")
    close(r.fpr, ref.fpr, "fpr")
    close(r.class_weight, ref.class_weight, "class_weight")
    assert torch.isfinite(grad).all().item(), tag
    gerr = (grad.cpu().double() - ref_grad).abs().max().item()
    assert gerr <= BAR * ref_grad.abs().max().item(), f"{tag} grad: {gerr:.3e} vs max|grad| {ref_grad.abs().max().item():.3e}"


def check_all_modes(x, y, tag):
    for kw in weight_modes(x.shape[2]):
        for alpha in (0.0, 1.0):
            r, grad = run_ours(x, y, fpr_alpha=alpha, **kw)
            ref, ref_grad = run_ref(x, y, fpr_alpha=alpha, **kw)
            compare(r, grad, ref, ref_grad, f"{tag} {sorted(kw)} alpha={alpha}")


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("s", [1, 3, 5])
@pytest.mark.parametrize("e", [1, 63, 257, 20011])
def test_matches_the_fp64_reference(e, s, c):
    x, y = make_inputs(e, s, c, seed=1000 * c + 10 * e + s)
    check_all_modes(x, y, f"E={e} S={s} C={c}")


@pytest.mark.parametrize("c", [2, 1])
def test_past_the_forward_grids_cap(c):
    """E = 140 003, S = 3: more rows per step than the forward's row blocks cover at once (at most 512 workgroups of 256 rows
    over all steps), so the grid-stride loop and the step boundaries inside it run."""
    x, y = make_inputs(140003, 3, c, seed=77 + c)
    check_all_modes(x, y, f"E=140003 C={c}")


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("e, s", [(65, 1), (257, 3), (65, 1025)])
def test_counts_at_wave_edges_and_past_the_step_grids_cap(e, s, c):
    """confusion [S, 4] exactly, one row past a wave and past a workgroup; S = 1025 is one step more than the 1024 the grid's
    y dimension takes, so one workgroup reduces two steps and uses its LDS words twice.  Loss and gradient at the file's
    bars there as well."""
    x, y = make_inputs(e, s, c, seed=900 + 10 * c + s)
    kw = dict(weight="balanced") if c == 2 else dict(pos_weight="balanced")
    r, grad = run_ours(x, y, fpr_alpha=1.0, **kw)
    ref, ref_grad = run_ref(x, y, fpr_alpha=1.0, **kw)
    assert r.confusion.shape == (s, 4) and r.confusion.sum(1).tolist() == [int(((y == 0) | (y == 1)).sum())] * s
    compare(r, grad, ref, ref_grad, f"E={e} S={s} C={c}")


@pytest.mark.parametrize("c", [2, 1])
@pytest.mark.parametrize("only", ["0", "1"])
def test_one_class_only(only, c):
    """All labels 0 / all labels 1: balanced falls back to (1, 1), the empty class reports 0 / 0.5, FPR is 0 without
    label-0 rows."""
    x, y = make_inputs(257, 3, c, seed=5 + c, labels=only)
    check_all_modes(x, y, f"only {only} C={c}")
    kw = dict(weight="balanced") if c == 2 else dict(pos_weight="balanced")
    r = mtmc_mpn.edge_loss(list(x.to(DEV)), y.to(DEV), fpr_alpha=1.0, **kw)
    empty = 1 - int(only)
    assert r.class_weight.tolist() == [1.0, 1.0]
    assert r.class_loss[:, empty].tolist() == [0.0] * 3 and r.class_prob[:, empty].tolist() == [0.5] * 3
    if only == "1":
        assert r.fpr.tolist() == [0.0] * 3
    assert torch.isfinite(r.loss).item()


def test_no_counted_row_at_all():
    """Every label skipped: 0/0 = NaN as torch's mean over no rows; gradients are 0 (skipped rows get 0), counts 0."""
    x, _ = make_inputs(63, 2, 2, seed=3)
    r, grad = run_ours(x, torch.full((63,), -100, dtype=torch.long))
    assert torch.isnan(r.loss).item() and r.confusion.sum().item() == 0 and (grad == 0).all().item()


@pytest.mark.parametrize("c", [2, 1])
def test_float_labels_and_a_number_as_pos_weight(c):
    x, y = make_inputs(20011, 3, c, seed=21)
    kw = dict(weight="balanced") if c == 2 else dict(pos_weight=7.0)
    r, grad = run_ours(x, y.float(), fpr_alpha=1.0, **kw)                  # the float 0/1 labels the reference keeps
    ref, ref_grad = run_ref(x, y, fpr_alpha=1.0, **kw)
    compare(r, grad, ref, ref_grad, f"float labels C={c}")


def test_equals_cross_entropy_steps_without_weights():
    x, y = make_inputs(20011, 3, 2, seed=31)
    r, grad = run_ours(x, y, up=1.0)
    block = x.to(DEV).requires_grad_(True)
    yy = y.to(DEV)
    loss = mtmc_mpn.cross_entropy_steps([block[i] for i in range(3)], yy)        # (-100 is its ignore_index)
    loss.backward()
    assert abs(r.loss.item() - loss.item()) <= BAR * max(1.0, abs(loss.item()))
    assert (grad - block.grad).abs().max().item() <= BAR * block.grad.abs().max().item()


@pytest.mark.parametrize("c", [2, 1])
def test_separate_step_tensors(c):
    """A list that is not one block is stacked: same values, and the gradients reach the separate tensors."""
    x, y = make_inputs(5003, 3, c, seed=41)
    kw = dict(weight="balanced") if c == 2 else dict(pos_weight="balanced")
    r, grad = run_ours(x, y, separate=True, fpr_alpha=1.0, **kw)
    ref, ref_grad = run_ref(x, y, fpr_alpha=1.0, **kw)
    compare(r, grad, ref, ref_grad, f"separate C={c}")
    rb, gradb = run_ours(x, y, fpr_alpha=1.0, **kw)
    assert torch.equal(r.confusion, rb.confusion)
    assert abs(r.loss.item() - rb.loss.item()) <= BAR * max(1.0, abs(rb.loss.item()))
    assert (grad - gradb).abs().max().item() <= BAR * gradb.abs().max().item()


def test_refusals_on_device_tensors():
    y = torch.zeros(4, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError):
        mtmc_mpn.edge_loss([torch.zeros(4, 3, device=DEV)], y)
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2, device=DEV)], y, pos_weight=1.0)
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 1, device=DEV)], y, weight="balanced")
    with pytest.raises(ValueError):
        mtmc_mpn.edge_loss([torch.zeros(4, 2, device=DEV)], y, weight="inverse")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mtmc_mpn.edge_loss([torch.zeros(4, 2, device=DEV)], y.cpu())


# ---- on a model ------------------------------------------------------------------------------------------------------
def test_balanced_loss_on_the_outputs_of_a_training_forward():
    """Parameter gradients through edge_loss(weight="balanced") == through cross_entropy(weight=w), w from the label counts
    read on the host (what a caller had to do before); same Dropout masks."""
    d = graphs.camera_graph((12, 9, 10), seed=3)
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(mtmc_mpn.default_params(num_enc_steps=3, num_class_steps=3)), None, ARCH).cuda().train()
    data = to_gpu(d)
    labels = (torch.rand(d.edge_index.shape[1], generator=torch.Generator().manual_seed(1)) < 0.2).long().cuda()
    n1 = float(labels.sum())
    w = torch.tensor([1.0, (labels.numel() - n1) / n1], device=DEV)
    grads = []
    for fused in (True, False):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        out, _ = m(data)
        steps = out["classified_edges"]
        loss = (mtmc_mpn.edge_loss(steps, labels, weight="balanced").loss if fused
                else sum(mtmc_mpn.cross_entropy(s, labels, weight=w) for s in steps))
        loss.backward()
        grads.append((loss.item(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-5 * max(1.0, abs(grads[1][0]))
    for k in grads[0][1]:
        a, b = grads[0][1][k], grads[1][1][k]
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item() + 1e-6, k


def test_one_logit_model_eval_logits_against_the_oracle():
    from oracle import mpn_oracle
    d = graphs.camera_graph((12, 9, 10), seed=3)
    params = one_logit_params()
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        want, want_h = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, d.x, d.edge_index, d.edge_attr)
        got, got_h = m.cuda()(to_gpu(d))
    assert len(got["classified_edges"]) == 3
    for a, b in zip(got["classified_edges"], want["classified_edges"]):
        assert a.shape == b.shape == (d.edge_index.shape[1], 1)
        assert (a.cpu() - b).abs().max().item() <= 1e-4
    assert (got_h.cpu() - want_h).abs().max().item() <= 1e-4 * max(1.0, want_h.abs().max().item())


def test_one_logit_model_gradients_against_fp64_autograd():
    """Dropout off, training mode: all 34 parameter gradients of edge_loss(pos_weight=7.0) against fp64 CPU autograd of the
    oracle under F.binary_cross_entropy_with_logits, at the bar of the G6 fixture test (1e-6 + 2e-4 * |grad|max).

    (The first edge-encoder weight sits in front of a BatchNorm over raw distances with mean 11.5 and deviation 0.18: its
    gradient, 2e-3, is what is left after the batch terms cancel.  The backward sums it against the centred attributes;
    summed against the raw ones it missed this bar by 5x, for two-class models too.)"""
    from oracle import mpn_oracle
    d = graphs.camera_graph((12, 9, 10), seed=3)
    params = one_logit_params()
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH)
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    labels = (torch.rand(d.edge_index.shape[1], generator=torch.Generator().manual_seed(1)) < 0.2).long()
    out, _ = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, d.x, d.edge_index, d.edge_attr, training=True,
                                dtype=torch.float64)
    pw = torch.tensor([7.0], dtype=torch.float64)
    want_loss = sum(F.binary_cross_entropy_with_logits(o[:, 0], labels.double(), pos_weight=pw) for o in out["classified_edges"])
    want_loss.backward()
    m = m.cuda().train()
    got, _ = m(to_gpu(d))
    r = mtmc_mpn.edge_loss(got["classified_edges"], labels.cuda(), pos_weight=7.0)
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


def test_captured_training_step_with_edge_loss():
    """As test_captured_training_step_follows_eager_steps, with the balanced loss + FPR term inside the HIP graph (it has no
    host read): the replayed losses follow the eager steps of a twin model, and the counts of the last replay are whole."""
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
        r = mtmc_mpn.edge_loss(o["classified_edges"], labels, weight="balanced", fpr_alpha=1.0)
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
