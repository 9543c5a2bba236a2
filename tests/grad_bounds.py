"""The bounds a HIP backward (fp32, float atomics) is held to against fp64 CPU autograd of the oracle: shared by
tests/test_gpu_training.py (through autograd) and tests/test_gpu_backward_abi.py (the C entry points directly)."""
import torch


def rel_err(a, b):
    scale = max(b.abs().max().item(), 1e-6)
    return (a - b).abs().max().item() / scale


def assert_param_grads_close(named_grads, ref_grads, n_edges):
    """named_grads: (name, gradient or None) pairs; ref_grads: name -> fp64 gradient or None.
    The CPU run is fp64, the GPU fp32: a ReLU whose pre-activation sits within rounding of 0 can switch sides,
    which moves one row of a weight gradient by O(1/N).  So: tight bound on the relative L2 error (a real bug
    is O(1)), looser bound on the worst element; gradients that are exactly 0 in exact arithmetic (biases in
    front of a BatchNorm) are compared on an absolute floor."""
    for k, grad in named_grads:
        want = ref_grads[k]
        if want is None or grad is None:                 # a parameter the forward never touched (L == 0: the update MLPs)
            assert want is None and grad is None, k
            continue
        got = grad.detach().cpu().double()
        scale = max(want.abs().max().item(), 1e-4)
        err = (got - want)
        # (absolute floor: rounding noise of float-atomic sums over E terms that cancel exactly in exact arithmetic grows with E)
        floor = 1e-6 + 2e-11 * n_edges
        assert err.abs().max().item() <= floor + 0.05 * scale, f"{k}: max err {err.abs().max().item():.3e} (scale {scale:.3e})"
        if want.norm().item() > 1e-6:
            assert (err.norm() / want.norm()).item() <= 5e-3, f"{k}: rel L2 {(err.norm() / want.norm()).item():.3e}"


def assert_input_grads_close(d_x, d_edge_attr, ref_dx, ref_dea):
    assert rel_err(d_x.detach().cpu().double(), ref_dx) <= 5e-4
    # d edge_attr of an edge depends on that edge's own ReLU states only: on a graph of tens of thousands of edges a
    # handful sit within fp32 rounding of a kink and come out on the other side than in the fp64 run (13 of 70 100
    # measured, the rest agree to 8e-6) -- leave out the worst 0.1 % of the edges, none on the small graphs
    got_ea = d_edge_attr.detach().cpu().double()
    per_edge = (got_ea - ref_dea).abs().amax(1)
    keep = torch.ones_like(per_edge, dtype=torch.bool)
    if per_edge.numel() >= 1000:
        keep[per_edge.topk(per_edge.numel() // 1000).indices] = False
    assert rel_err(got_ea[keep], ref_dea[keep]) <= 5e-4
