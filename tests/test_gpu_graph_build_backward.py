"""GPU tests of the differentiable graph builder: `build_graph` on features that require grad carries the gradient of
`x` and `edge_attr` back to the features (`mtmc_build_graph_backward`).  Reference for every gradient: fp64 CPU autograd
of the oracle's restatement of the reference's statements (train.py:316-342), contracted with seeded random gX / g_attr.
Bar: the project's gradient bar (tests/test_gpu_training.py, G6): |d| <= 1e-6 + 2e-4 |grad|max."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_cases
import mtmc_mpn
from golden_util import ARCH

pytestmark = pytest.mark.gpu


def oracle_grad(feats, cams, l2norm, g_x, g_attr):
    from oracle import graph_oracle
    f64 = feats.double().requires_grad_()
    x, _, attr, _ = graph_oracle.build(f64, cams, None, l2norm)
    loss = 0
    if g_x is not None:
        loss = loss + (x * g_x.double()).sum()
    if g_attr is not None and attr.shape[0]:
        loss = loss + (attr * g_attr.double()).sum()
    loss.backward()
    return f64.grad


def meets_bar(got, want, what):
    scale = want.abs().max().item()
    err = (got.double().cpu() - want).abs().max().item()
    print(f"{what}: |dgrad| {err:.3e}, |grad|max {scale:.3e}, ratio {err / max(scale, 1e-30):.2e}")
    assert torch.isfinite(got).all(), what
    assert err <= 1e-6 + 2e-4 * scale, f"{what}: |dgrad| {err:.3e} > bar (|grad|max {scale:.3e})"


def run(feats, cams, l2norm=True, with_x=True, with_attr=True, seed=11, what=""):
    leaf = feats.cuda().requires_grad_()
    g = mtmc_mpn.build_graph(leaf, cams, None, l2norm)
    assert g.x.requires_grad and g.edge_attr.requires_grad and not g.edge_index.requires_grad
    gen = torch.Generator().manual_seed(seed)
    g_x = torch.randn(g.x.shape, generator=gen) if with_x else None
    g_attr = torch.randn(g.edge_attr.shape, generator=gen) if with_attr else None
    outs, grads = [], []
    if with_x:
        outs.append(g.x), grads.append(g_x.cuda())
    if with_attr:
        outs.append(g.edge_attr), grads.append(g_attr.cuda())
    torch.autograd.backward(outs, grads)
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape
    meets_bar(leaf.grad, oracle_grad(feats, cams, l2norm, g_x, g_attr), what)
    return leaf.grad


@pytest.mark.parametrize("name", graph_cases.CASES)
def test_both_gradients(name):
    feats, cams, _ = graph_cases.inputs(name)
    run(feats, cams, what=name)


def test_x_gradient_only_and_attr_gradient_only():
    feats, cams, _ = graph_cases.inputs("cams3")
    run(feats, cams, with_attr=False, what="cams3 gX only")
    run(feats, cams, with_x=False, what="cams3 g_attr only")
    feats, cams, _ = graph_cases.inputs("interleaved")
    run(feats, cams, with_x=False, what="interleaved g_attr only")


def test_unnormalised_branch():
    feats, cams, _ = graph_cases.inputs("interleaved")
    run(feats.abs(), cams, l2norm=False, what="interleaved |feats|, l2norm=False")


def test_two_nodes_two_cameras_and_single_camera():
    feats = torch.randn(2, 2048, generator=torch.Generator().manual_seed(1))
    run(feats, np.array([3, 7]), what="two nodes")
    feats = torch.randn(5, 2048, generator=torch.Generator().manual_seed(4))
    leaf = feats.cuda().requires_grad_()
    g = mtmc_mpn.build_graph(leaf, np.zeros(5, dtype=int))
    assert g.edge_attr.shape == (0, 2)
    g_x = torch.randn(5, 2048, generator=torch.Generator().manual_seed(6))
    (g.x * g_x.cuda()).sum().backward()                            # E = 0: the normalise backward of gX alone
    meets_bar(leaf.grad, oracle_grad(feats, np.zeros(5, dtype=int), True, g_x, None), "single camera")


def test_strided_view_gets_its_gradient_in_the_callers_layout():
    feats, cams, _ = graph_cases.inputs("cams3")
    wide = torch.zeros(9, 4096)
    wide[:, ::2] = feats
    base = wide.cuda().requires_grad_()
    view = base[:, ::2]
    assert not view.is_contiguous()
    g = mtmc_mpn.build_graph(view, cams)
    gen = torch.Generator().manual_seed(11)
    g_x, g_attr = torch.randn(g.x.shape, generator=gen), torch.randn(g.edge_attr.shape, generator=gen)
    torch.autograd.backward([g.x, g.edge_attr], [g_x.cuda(), g_attr.cuda()])
    assert base.grad.shape == (9, 4096) and torch.count_nonzero(base.grad[:, 1::2]).item() == 0
    meets_bar(base.grad[:, ::2], oracle_grad(feats, cams, True, g_x, g_attr), "strided view")


def test_exactly_equal_rows_across_cameras():
    feats, cams, _ = graph_cases.inputs("cams3")
    feats = feats.clone()
    feats[4] = feats[0]                                            # node 0: camera 1, node 4: camera 2
    grad = run(feats, cams, what="equal rows")
    assert torch.isfinite(grad).all()


def test_requires_grad_false_and_no_grad_are_todays_path_bit_for_bit():
    feats, cams, ids = graph_cases.inputs("cams3")
    dev = feats.cuda()
    plain = mtmc_mpn.build_graph(dev, cams, ids)
    with torch.no_grad():
        quiet = mtmc_mpn.build_graph(dev.clone().requires_grad_(), cams, ids)
    diff = mtmc_mpn.build_graph(dev.clone().requires_grad_(), cams, ids)
    assert diff.x.grad_fn is not None and diff.edge_attr.grad_fn is not None
    assert not diff.edge_labels.requires_grad and not diff.edge_index.requires_grad
    for g in (plain, quiet):
        assert g.x.grad_fn is None and g.edge_attr.grad_fn is None and not g.x.requires_grad
        for k in ("x", "edge_index", "edge_attr", "edge_labels", "y"):
            assert torch.equal(getattr(g, k), getattr(diff, k).detach()), k


def test_backward_needs_no_edge_sized_feature_buffer():
    """S02 size: the backward through build_graph alone may raise the peak allocation by < 5 % of E * F * 4 bytes (61 MB);
    the gather formulation saves two [E, F] tensors (1.2 GB each)."""
    feats, cams, _ = graph_cases.inputs("s02_gt")
    leaf = feats.cuda().requires_grad_()
    g = mtmc_mpn.build_graph(leaf, cams)
    e, f = g.edge_attr.shape[0], leaf.shape[1]
    g_x, g_attr = torch.randn_like(g.x), torch.randn_like(g.edge_attr)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    torch.autograd.backward([g.x, g.edge_attr], [g_x, g_attr])
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak growth in backward: {grown / 1e6:.2f} MB (E*F*4 = {e * f * 4 / 1e6:.0f} MB)")
    assert grown < 0.05 * e * f * 4


def test_fine_tune_chain_end_to_end():
    """feats -> build_graph -> MOTMPNet -> cross_entropy_steps -> backward against fp64 CPU autograd of the oracles; the 34
    parameter gradients are those of a run on the detached graph."""
    from oracle import graph_oracle, mpn_oracle
    cams = np.repeat(np.arange(3), (20, 17, 25))
    ids = torch.randint(0, 20, (cams.size,), generator=torch.Generator().manual_seed(9)).numpy()
    feats = torch.randn(cams.size, 2048, generator=torch.Generator().manual_seed(8))
    params = mtmc_mpn.default_params(num_enc_steps=2, num_class_steps=2)
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval()
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items()}

    f64 = feats.double().requires_grad_()
    x, ei, attr, lab = graph_oracle.build(f64, cams, ids)
    want, _ = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, x, ei, attr)
    loss_ref = sum(F.cross_entropy(o, lab.long()) for o in want["classified_edges"])
    loss_ref.backward()

    m = m.cuda()

    def step(detach):
        m.zero_grad(set_to_none=True)
        leaf = feats.cuda().requires_grad_()
        g = mtmc_mpn.build_graph(leaf, cams, ids)
        if detach:
            g.x, g.edge_attr = g.x.detach(), g.edge_attr.detach()
        out, _ = m(g)
        loss = mtmc_mpn.cross_entropy_steps(out["classified_edges"], g.edge_labels.long())
        loss.backward()
        return loss.item(), leaf.grad, {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    loss, grad, pgrads = step(detach=False)
    _, none_grad, pgrads_detached = step(detach=True)
    assert none_grad is None
    assert abs(loss - loss_ref.item()) <= 1e-4 * max(1.0, abs(loss_ref.item()))
    meets_bar(grad, f64.grad, "fine-tune chain d feats")
    assert len(pgrads) == 34
    # the parameter gradients do not depend on whether d x / d edge_attr are asked for; the backward's sums are atomic, so
    # two runs may differ in their last bits: compared at the gradient bar, per tensor
    for k in pgrads:
        scale = pgrads_detached[k].abs().max().item()
        assert (pgrads[k] - pgrads_detached[k]).abs().max().item() <= 1e-6 + 2e-4 * scale, k
