"""CPU checks of tests/gram_cases.py: the fp64 reference agrees with the oracle, the error yardstick is stable, and every
case of tests/test_gpu_graph_build_regimes.py still reaches the code it was made for -- its split-K factor (host-only query
of the library, as tests/test_postprocess_workspace.py) and its count of near-duplicate edges."""
import numpy as np
import pytest
import torch

import gram_cases as gc
import graph_cases


def test_reference_agrees_with_the_oracle_in_fp64():
    from oracle import graph_oracle
    f3, c3, _ = graph_cases.inputs("cams3")
    fn, cn, _ = gc.near_case(33, 96, 3, 0.01, gc.case_seed(33, 96))
    for feats, cams, l2norm in ((f3, c3, True), (fn, cn, True), (fn.abs(), cn, False)):
        x_ref, ei_ref, attr_ref, _ = graph_oracle.build(feats.double(), cams, None, l2norm)
        edges = gc.topology(cams)
        assert torch.equal(edges, ei_ref)
        x, attr = gc.reference_attr(feats, cams, l2norm, edges)
        assert (x - x_ref).abs().max().item() <= 1e-12
        assert (attr - attr_ref).abs().max().item() <= 1e-12
        pick = torch.tensor([5, 0, edges.shape[1] - 1, 5])            # any subset, any order
        assert torch.equal(gc.reference_attr(feats, cams, l2norm, edges[:, pick])[1], attr[pick])


def test_near_case_layout():
    feats, cams, ids = gc.near_case(14, 32, 4, 0.01, 3, equal_pairs=2)
    assert cams.tolist() == [0, 1, 2, 3] * 3 + [0, 1] and ids.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 2
    assert torch.equal(feats[1], feats[0]) and torch.equal(feats[5], feats[4]) and not torch.equal(feats[9], feats[8])
    again, _, _ = gc.near_case(14, 32, 4, 0.01, 3, equal_pairs=2)
    assert torch.equal(feats, again)


@pytest.mark.parametrize("f", [32, 256, 2048])
def test_model_reproduces_within_a_factor_of_two(f):
    a, b = gc.gram_model(f, 0.01, True, 0), gc.gram_model(f, 0.01, True, 1)
    print(f"F {f}: c_d2 {a[0]:.2e} / {b[0]:.2e}, c_cos {a[1]:.2e} / {b[1]:.2e}")
    for u, v in zip(a, b):
        assert 0 < u <= 2 * v and v <= 2 * u
    # the comment this yardstick replaces said ~1e-6: it is the right order, and the chain length is what moves it
    assert 1e-7 < a[0] < 1e-5 and a[1] < 5e-6


def test_model_grows_with_k():
    assert gc.gram_model(2048, 0.01, True)[0] > 2 * gc.gram_model(32, 0.01, True)[0]


@pytest.mark.parametrize("case", gc.FORWARD_CASES, ids=gc.case_id)
def test_forward_case_is_in_its_regime(case):
    """Fails when a retuned gemm_plan moves a case into another split.  Which kernel an unsplit case takes (exact fp32 BK 64 /
    BK 32, bf16x6 from 1921 nodes, scalar above F = 6144) is not visible in the size: see the table in gram_cases."""
    from mtmc_mpn import _lib
    n, f, _, _, split, _ = case
    assert gc.workspace_split(n, f, _lib.load().mtmc_graph_workspace_bytes(n, f)) == split


@pytest.mark.parametrize("n, f, split", [(130, 384, 2), (130, 256, 4), (200, 2048, 4), (960, 2048, 4), (961, 2048, 1),
                                         (1921, 2048, 1), (150, 6176, 1), (960, 384, 2), (960, 128, 1)])
def test_split_thresholds(n, f, split):
    from mtmc_mpn import _lib
    assert gc.workspace_split(n, f, _lib.load().mtmc_graph_workspace_bytes(n, f)) == split


def test_large_cases_take_three_grid_stride_trips_and_the_sample_reaches_them():
    for case in gc.FORWARD_CASES:
        if case[0] != 1921:
            continue
        _, cams, ids = gc.forward_inputs(case)
        edges = gc.topology(cams)
        assert gc.edge_trips(edges.shape[1]) == 3
        pick = gc.float_sample(cams, ids, edges)
        assert 20_000 < pick.numel() < 40_000
        assert ((pick >= 1 << 20) & (pick < 2 << 20)).any() and (pick >= 2 << 20).any()


@pytest.fixture(scope="module", params=gc.BACKWARD_CASES, ids=gc.case_id)
def backward_case(request):
    case = request.param
    n, f, _, _, l2norm, _ = case
    feats, cams, _ = gc.backward_inputs(case)
    edges = gc.topology(cams)
    x64, attr = gc.reference_attr(feats, cams, l2norm, edges)
    near = gc.flagged(attr[:, 0], gc.rho2(x64), edges)
    g_x, g_attr = gc.seeded_grads(n, f, edges.shape[1])
    want = gc.oracle_grad(feats, cams, l2norm, g_x, g_attr)
    return case, feats, cams, near, g_x, g_attr, want


def test_backward_case_flags_its_edges(backward_case):
    case, _, _, near, *_ = backward_case
    print(f"{gc.case_id(case)}: {int(near.sum())} flagged edges of {near.numel()}")
    assert int(near.sum()) >= case[5]


def test_fp32_reference_is_well_inside_the_gradient_bar(backward_case):
    case, feats, cams, _, g_x, g_attr, want = backward_case
    got = gc.oracle_grad(feats, cams, case[4], g_x, g_attr, torch.float32)
    err = (got.double() - want).abs().max().item()
    print(f"{gc.case_id(case)}: fp32 autograd off by {err / gc.grad_bar(want):.4f} of the bar")
    assert err <= 0.05 * gc.grad_bar(want)


def test_a_lost_flagged_edge_is_far_above_the_gradient_bar(backward_case):
    """What gb_bwd_near_kernel contributes, in fp64 on the CPU: the feature gradient moves by this much when the distance term
    of one flagged edge (the one with the largest |g_D|) or of all flagged edges is lost -- a wrong sign moves it by twice
    that.  The gradient bar sees it with a wide margin, so the GPU cases test that kernel."""
    case, feats, cams, near, _, g_attr, want = backward_case
    idx = torch.nonzero(near).flatten()

    def moved(sel):
        only = torch.zeros_like(g_attr, dtype=torch.float64)
        only[sel, 0] = g_attr[sel, 0].double()
        return gc.oracle_grad(feats, cams, case[4], None, only).abs().max().item() / gc.grad_bar(want)

    one, every = moved(idx[g_attr[idx, 0].abs().argmax()]), moved(idx)
    print(f"{gc.case_id(case)}: one flagged edge lost {one:.0f} x bar, all lost {every:.0f} x bar")
    assert one >= 49 and every >= 300
