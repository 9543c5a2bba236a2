"""GPU tests of `build_graph` in every regime of its Gram product (tests/gram_cases.py: exact fp32 with split-K 4 / 2 / none
and BK 64 / 32, bf16x6 from 1921 nodes, the scalar path above F = 6144), at the tile edges, on row-strided input, and of its
backward on near-duplicate tracklets, where gb_bwd_near_kernel takes the distance gradient of the flagged edges.

Forward reference: fp64 on the CPU from the F-dimensional rows themselves (gram_cases.reference_attr).  Distance bar, per edge:
|d^2 - d_ref^2| <= 2 c_model(F) (rho_r^2 + rho_c^2), c_model from a CPU model of the Gram form with the longest fp32 chain
(gram_cases.gram_model); cosine bar max(5e-6, 2 cos_model(F)).  Each forward case prints one `envelope` line; those of the
recorded run are profiles/graph_build_envelope.txt.
Backward reference and bar: tests/test_gpu_graph_build_backward.py's (fp64 CPU autograd of the oracle, 1e-6 + 2e-4 |grad|max).
"""
import time

import numpy as np
import pytest
import torch

import gram_cases as gc
import mtmc_mpn
from test_gpu_graph_build_backward import meets_bar, oracle_grad

pytestmark = pytest.mark.gpu


def check_forward(g, feats, cams, ids, l2norm, what, regime=""):
    """Integers in full and exactly; x at the project's bar; distance and cosine per edge inside the envelope."""
    n, f = feats.shape
    edges = gc.topology(cams)
    got_index = g.edge_index.cpu()
    assert g.edge_index.dtype == torch.int64 and not g.edge_index.is_contiguous()      # the callers' [E, 2].T view
    assert torch.equal(got_index, edges)
    lab = torch.from_numpy(np.asarray(ids))
    assert torch.equal(g.edge_labels.cpu(), (lab[edges[0]] == lab[edges[1]]).float())
    pick = gc.float_sample(cams, ids, edges)
    for trip in range(gc.edge_trips(edges.shape[1])):       # every grid-stride trip of gb_edges_kernel (1 048 576 edges each)
        assert ((pick >= trip << 20) & (pick < (trip + 1) << 20)).any()
    sub = edges[:, pick]
    x64, attr64 = gc.reference_attr(feats, cams, l2norm, sub)
    assert (g.x.cpu().double() - x64).abs().max().item() <= 1e-6 * max(1.0, x64.abs().max().item())
    attr = g.edge_attr.cpu()[pick].double()
    assert torch.isfinite(attr).all()
    r2 = gc.rho2(x64)
    c_d2, c_cos = gc.gram_model(f, gc.FORWARD_NOISE, l2norm)
    ratio_d = ((attr[:, 0].square() - attr64[:, 0].square()).abs() / (r2[sub[0]] + r2[sub[1]]).clamp_min(1e-300)).max().item()
    ratio_d /= 2 * c_d2
    cos_bar = max(5e-6, 2 * c_cos)
    ratio_c = (attr[:, 1] - attr64[:, 1]).abs().max().item() / cos_bar
    n_near = int(gc.flagged(attr64[:, 0], r2, sub).sum())
    print(f"envelope {what}: regime [{regime}] N {n} F {f} l2norm {int(l2norm)} E {edges.shape[1]} compared {pick.numel()} "
          f"near {n_near} c_model {c_d2:.3e} cos_model {c_cos:.3e} d2_err/bar {ratio_d:.3f} cos_err/bar {ratio_c:.3f}")
    assert ratio_d <= 1.0, f"{what}: |d^2 - d_ref^2| is {ratio_d:.2f} x its bar 2 c_model (rho_r^2 + rho_c^2)"
    assert ratio_c <= 1.0, f"{what}: |cos - cos_ref| is {ratio_c:.2f} x its bar {cos_bar:.1e}"
    return edges, x64, attr64


@pytest.mark.parametrize("case", gc.FORWARD_CASES, ids=gc.case_id)
def test_forward_regime(case):
    n, f, _, l2norm, _, regime = case
    feats, cams, ids = gc.forward_inputs(case)
    t0 = time.perf_counter()
    g = mtmc_mpn.build_graph(feats.cuda(), cams, ids, l2norm)
    check_forward(g, feats, cams, ids, l2norm, gc.case_id(case), regime)
    print(f"{gc.case_id(case)}: {time.perf_counter() - t0:.2f} s")


def test_row_strided_input_is_read_in_place():
    case = next(c for c in gc.FORWARD_CASES if c[:2] == (65, 96))
    feats, cams, ids = gc.forward_inputs(case)
    wide = torch.full((65, 128), 7.0)                       # a kernel that ignored the row stride would read the 7s
    wide[:, :96] = feats
    view = wide.cuda()[:, :96]
    assert view.stride(0) == 128 and view.stride(1) == 1 and not view.is_contiguous()
    g = mtmc_mpn.build_graph(view, cams, ids)
    check_forward(g, feats, cams, ids, True, "65x96 in [65,128]", case[5])
    flat = mtmc_mpn.build_graph(feats.cuda(), cams, ids)
    assert torch.equal(g.edge_index, flat.edge_index) and torch.equal(g.edge_labels, flat.edge_labels)
    assert torch.equal(g.y, flat.y)
    assert (g.x - flat.x).abs().max().item() <= 1e-6 * max(1.0, flat.x.abs().max().item())


def test_zero_row():
    case = next(c for c in gc.FORWARD_CASES if c[:2] == (65, 96))
    feats, cams, ids = gc.forward_inputs(case)
    feats = feats.clone()
    feats[7] = 0
    g = mtmc_mpn.build_graph(feats.cuda(), cams, ids)
    edges, _, _ = check_forward(g, feats, cams, ids, True, "65x96, row 7 zero", case[5])    # distances inside the envelope
    touches = (edges[0] == 7) | (edges[1] == 7)
    assert int(touches.sum()) == 2 * int((cams != cams[7]).sum())
    assert torch.equal(g.edge_attr.cpu()[touches, 1], torch.ones(int(touches.sum())))        # 1 - cos == 1 exactly


def test_scalar_path_refuses_more_than_2048_nodes():
    feats, cams, _ = gc.near_case(2049, 6176, 3, 0.01, 1)
    with pytest.raises(RuntimeError, match="build_graph"):
        mtmc_mpn.build_graph(feats.cuda(), cams)


# ---- backward on near-duplicate tracklets ----

def run_backward(case, with_x=True, strided=False):
    n, f, _, _, l2norm, n_flagged = case
    what = gc.case_id(case) + ("" if with_x else ", g_attr only") + (", strided" if strided else "")
    feats, cams, _ = gc.backward_inputs(case)
    if strided:
        wide = torch.zeros(n, f + 64)
        wide[:, :f] = feats
        base = wide.cuda().requires_grad_()
        leaf = base[:, :f]
        assert leaf.stride(0) == f + 64 and not leaf.is_contiguous()
    else:
        base = leaf = feats.cuda().requires_grad_()
    t0 = time.perf_counter()
    g = mtmc_mpn.build_graph(leaf, cams, None, l2norm)
    # the coverage this case exists for, from the device's own outputs: gb_near's rule with rho from g.x
    x, attr, ei = g.x.detach(), g.edge_attr.detach(), g.edge_index
    rho_sq = x.double().square().sum(1).float().sqrt().square()
    near = attr[:, 0] * attr[:, 0] < 1e-3 * (rho_sq[ei[0]] + rho_sq[ei[1]])
    print(f"{what}: {int(near.sum())} edges flagged on the device, {n_flagged} in fp64")
    assert int(near.sum()) >= 0.9 * n_flagged
    gen = torch.Generator().manual_seed(11)                 # as test_gpu_graph_build_backward.run
    g_x = torch.randn(g.x.shape, generator=gen) if with_x else None
    g_attr = torch.randn(g.edge_attr.shape, generator=gen)
    outs, grads = ([g.x], [g_x.cuda()]) if with_x else ([], [])
    torch.autograd.backward(outs + [g.edge_attr], grads + [g_attr.cuda()])
    assert base.grad is not None and base.grad.shape == base.shape
    if strided:
        assert torch.count_nonzero(base.grad[:, f:]).item() == 0
    meets_bar(base.grad[:, :f], oracle_grad(feats, cams, l2norm, g_x, g_attr), what)
    print(f"{what}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("case", gc.BACKWARD_CASES, ids=gc.case_id)
def test_backward_near_duplicates(case):
    run_backward(case)


@pytest.mark.parametrize("case", [c for c in gc.BACKWARD_CASES if c[:2] in ((72, 2048), (300, 64))], ids=gc.case_id)
def test_backward_near_duplicates_attr_gradient_only(case):
    run_backward(case, with_x=False)


def test_backward_near_duplicates_through_a_row_strided_view():
    run_backward(next(c for c in gc.BACKWARD_CASES if c[:2] == (65, 256) and c[4]), strided=True)
