"""GPU tests of `pool_tracklets` against tests/pool_ref.py (numpy float64).

The bounds are derived, not measured (u = 2^-24; pool_ref.check_forward / check_backward):
  integer inputs   |got - S/len| <= 3u |S/len|, exactly 0 where the column sum S is 0 (the sums themselves are exact)
  gaussian inputs  |got - ref64| <= (len + 4) u mean_i|x_i| per element (any-order summation bound + the scale)
  backward         |got - g/len| <= 3u |g/len|, bit-equal to g/len where len is a power of two
R below is pool.CHUNK_ROWS, the rows per chunk of the kernels' decomposition.
"""
import functools

import numpy as np
import pytest
import torch

import pool_ref

pytestmark = pytest.mark.gpu

FAMILIES = ("integer", "gaussian")
GEN = {"integer": pool_ref.integer_embeds, "gaussian": pool_ref.gaussian_embeds}


def _r():
    from mtmc_mpn import pool
    return pool.CHUNK_ROWS


@functools.lru_cache(maxsize=None)
def _inputs(lengths, f, family, seed=0):
    """embeds [D, f] and a gradient [N, f] of one family (numpy, read-only: shared between tests)."""
    e = GEN[family](sum(lengths), f, seed + 1)
    g = GEN[family](len(lengths), f, seed + 2)
    e.setflags(write=False)
    g.setflags(write=False)
    return e, g


def _offsets(lengths, dev="cuda"):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _both_ways(lengths, f, family):
    """Forward through the public function, backward through the raw entry; both against the yardstick."""
    from mtmc_mpn import pool
    lengths = tuple(int(v) for v in lengths)
    e, g = _inputs(lengths, f, family)
    out = pool.pool_tracklets(_cuda(e), list(lengths))
    assert out.shape == (len(lengths), f) and out.dtype == torch.float32 and out.is_contiguous()
    pool_ref.check_forward(out.cpu().numpy(), e, lengths, family)
    grad = pool._backward_raw(_cuda(g), _offsets(lengths), e.shape[0])
    assert grad.shape == e.shape
    pool_ref.check_backward(grad.cpu().numpy(), g, lengths)
    return out, grad


def _skew():
    r = _r()
    return (1, 20 * r + 3, 1, 2, 7 * r, 1)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,f", [(1, 4), (5, 32), (3, 2048)])
def test_length_one_is_a_copy(n, f, family):
    lengths = (1,) * n
    e, g = _inputs(lengths, f, family)
    out, grad = _both_ways(lengths, f, family)
    assert np.array_equal(out.cpu().numpy(), e) and np.array_equal(grad.cpu().numpy(), g)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_every_length_across_the_chunk_edges(order, family):
    r = _r()
    lengths = np.arange(1, 2 * r + 3)
    if order == "shuffled":
        lengths = np.random.default_rng(5).permutation(lengths)
    _both_ways(lengths, 256, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_chunk_edges_at_full_width(family):
    r = _r()
    _both_ways([r - 1, r, r + 1, 2 * r, 2 * r + 1, 1, 3 * r + 5], 2048, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("f", [100, 2080])
def test_skew(f, family):
    _both_ways(_skew(), f, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_strided_input(family):
    from mtmc_mpn import pool
    r = _r()
    lengths, f = (3, r + 2, 1, 2 * r, 5), 192
    e, g = _inputs(lengths, f, family)
    d = e.shape[0]
    buf = torch.full((d, f + 64), float("nan"), device="cuda")
    buf[:, 32:32 + f] = _cuda(e)
    view = buf[:, 32:32 + f]
    assert view.stride(0) == f + 64 and not view.is_contiguous()
    out = pool.pool_tracklets(view, lengths)
    pool_ref.check_forward(out.cpu().numpy(), e, lengths, family)
    wide = torch.full((d, 2 * f), float("nan"), device="cuda")
    wide[:, ::2] = _cuda(e)
    every_other = wide[:, ::2]
    assert every_other.stride(1) == 2
    out2 = pool.pool_tracklets(every_other, lengths)
    assert torch.equal(out, out2)
    # the same through a strided gradient buffer
    gbuf = torch.full((d, f + 64), float("nan"), device="cuda")
    grad = pool._backward_raw(_cuda(g), _offsets(lengths), d, out=gbuf[:, 32:32 + f])
    pool_ref.check_backward(grad.cpu().numpy(), g, lengths)
    assert torch.isnan(gbuf[:, :32]).all() and torch.isnan(gbuf[:, 32 + f:]).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_neighbours_are_poison(family):
    from mtmc_mpn import pool
    lengths, f, pad = _skew(), 2080, 3
    e, g = _inputs(lengths, f, family)
    d, n = e.shape[0], len(lengths)
    nan = float("nan")
    big = torch.full((d + 2 * pad, f), nan, device="cuda")
    big[pad:pad + d] = _cuda(e)
    out_buf = torch.full((n + 2, f), nan, device="cuda")
    out = pool._forward_raw(big[pad:pad + d], _offsets(lengths), out=out_buf[1:n + 1])
    assert out.data_ptr() == out_buf[1].data_ptr()
    assert not torch.isnan(out).any()
    pool_ref.check_forward(out.cpu().numpy(), e, lengths, family)
    assert torch.isnan(out_buf[0]).all() and torch.isnan(out_buf[-1]).all()
    assert torch.isnan(big[:pad]).all() and torch.isnan(big[pad + d:]).all() and torch.equal(big[pad:pad + d], _cuda(e))
    grad_buf = torch.full((d + 2 * pad, f), nan, device="cuda")
    g_buf = torch.full((n + 2, f), nan, device="cuda")
    g_buf[1:n + 1] = _cuda(g)
    grad = pool._backward_raw(g_buf[1:n + 1], _offsets(lengths), d, out=grad_buf[pad:pad + d])
    assert not torch.isnan(grad).any()
    pool_ref.check_backward(grad.cpu().numpy(), g, lengths)
    assert torch.isnan(grad_buf[:pad]).all() and torch.isnan(grad_buf[pad + d:]).all()


@pytest.mark.parametrize("f", [100, 2080])
def test_repeatable(f):
    from mtmc_mpn import pool
    lengths = _skew()
    e, g = _inputs(lengths, f, "gaussian")
    e_dev, g_dev, off = _cuda(e), _cuda(g), _offsets(lengths)
    a, b = pool.pool_tracklets(e_dev, lengths), pool.pool_tracklets(e_dev, offsets=off)
    assert torch.equal(a, b)
    ga, gb = pool._backward_raw(g_dev, off, e.shape[0]), pool._backward_raw(g_dev, off, e.shape[0])
    assert torch.equal(ga, gb)


@pytest.mark.parametrize("family", FAMILIES)
def test_autograd(family):
    from mtmc_mpn import pool_tracklets
    r = _r()
    lengths, f = (2, r + 1, 1, 3 * r, 4, r), 320
    e, w = _inputs(lengths, f, family)
    leaf = _cuda(e).requires_grad_()
    out = pool_tracklets(leaf, lengths)
    assert out.requires_grad and type(out.grad_fn).__name__ == "_PoolTrackletsBackward"
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.int64          # the offsets only: embeds is not kept
    (out * _cuda(w)).sum().backward()
    pool_ref.check_backward(leaf.grad.cpu().numpy(), w, lengths)
    pool_ref.check_forward(out.detach().cpu().numpy(), e, lengths, family)
    with torch.no_grad():
        assert not pool_tracklets(leaf, lengths).requires_grad
    assert not pool_tracklets(leaf.detach(), lengths).requires_grad


def test_autograd_chain_with_build_graph():
    import mtmc_mpn
    r = _r()
    n, f = 12, 64
    lengths = tuple(int(v) for v in np.linspace(1, r + 3, n).round())
    assert lengths[0] == 1 and lengths[-1] == r + 3 and len(lengths) == n
    cams = np.arange(n) % 3
    labels = np.arange(n) // 3
    e, _ = _inputs(lengths, f, "gaussian", seed=20)

    def loss(g):
        wx = torch.randn(g.x.shape, generator=torch.Generator().manual_seed(22)).cuda()
        wa = torch.randn(g.edge_attr.shape, generator=torch.Generator().manual_seed(23)).cuda()
        return (g.x * wx).sum() + (g.edge_attr * wa).sum()

    leaf = _cuda(e).requires_grad_()
    loss(mtmc_mpn.build_graph(mtmc_mpn.pool_tracklets(leaf, lengths), cams, labels)).backward()
    pooled = mtmc_mpn.pool_tracklets(leaf.detach(), lengths).requires_grad_()
    loss(mtmc_mpn.build_graph(pooled, cams, labels)).backward()
    pool_ref.check_backward(leaf.grad.cpu().numpy(), pooled.grad.cpu().numpy(), lengths)


def _bad_offsets():
    return {1: [0, 5, 3, 8], 2: [0, 3, 6]}


@pytest.mark.parametrize("family", FAMILIES)
def test_device_offsets(family):
    from mtmc_mpn import pool
    lengths, f = _skew(), 100
    e, _ = _inputs(lengths, f, family)
    e_dev, off = _cuda(e), _offsets(lengths)
    want = pool.pool_tracklets(e_dev, lengths)
    assert torch.equal(pool.pool_tracklets(e_dev, offsets=off), want)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        quiet = pool.pool_tracklets(e_dev, offsets=off, check=False)            # a host read would raise here
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(quiet, want)


@pytest.mark.parametrize("status", [1, 2])
def test_device_offsets_status(status):
    from mtmc_mpn import pool
    e = _cuda(pool_ref.gaussian_embeds(8, 32, 9))
    off = torch.tensor(_bad_offsets()[status], dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="offsets"):
        pool.pool_tracklets(e, offsets=off)
    with pytest.raises(RuntimeError, match="offsets"):
        pool.pool_tracklets(e.clone().requires_grad_(), offsets=off, check=True)
    out = pool.pool_tracklets(e, offsets=off, check=False)                       # no exception
    assert out.shape == (off.numel() - 1, 32)
    info = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    out = pool._forward_raw(e, off, info=info)
    assert info.cpu().tolist()[0] == status
    if status == 1:                                                              # the inverted range [5, 3) is a zero row
        assert (out[1] == 0).all()
        pool_ref.check_forward(out[:1].cpu().numpy(), e[:5].cpu().numpy(), [5], "gaussian")
    else:                                                                        # the ranges themselves are fine
        pool_ref.check_forward(out.cpu().numpy(), e[:6].cpu().numpy(), [3, 3], "gaussian")
    good = torch.tensor([0, 3, 8], dtype=torch.int64, device="cuda")
    pool._forward_raw(e, good, info=info)
    assert info.cpu().tolist() == [0, 0, 0, 0]


def test_argument_errors_on_the_device():
    from mtmc_mpn import pool_tracklets
    e = torch.zeros(6, 8, device="cuda")
    for bad in (e.double(), e.half(), torch.zeros(6, 6, device="cuda"), torch.zeros(6, device="cuda")):
        with pytest.raises(RuntimeError):
            pool_tracklets(bad, [6])
    with pytest.raises(RuntimeError):
        pool_tracklets(e, offsets=torch.tensor([0, 6]))                          # offsets on the host
    with pytest.raises(RuntimeError):
        pool_tracklets(e, offsets=torch.tensor([0, 6], dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        pool_tracklets(e, [3, 2])


@pytest.mark.parametrize("family", FAMILIES)
def test_captured(family):
    from mtmc_mpn import pool
    r = _r()
    first, second, f = (r + 5, 2, 3 * r, 1), (1, 2 * r + 1, r + 4, r + 2), 512
    assert sum(first) == sum(second)
    e1, _ = _inputs(first, f, family, seed=30)
    e2, _ = _inputs(second, f, family, seed=31)
    e_dev, off_dev = _cuda(e1), _offsets(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool.pool_tracklets(e_dev, offsets=off_dev, check=False)                 # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = pool.pool_tracklets(e_dev, offsets=off_dev, check=False)
    graph.replay()
    torch.cuda.synchronize()
    pool_ref.check_forward(out.cpu().numpy(), e1, first, family)
    e_dev.copy_(_cuda(e2))
    off_dev.copy_(_offsets(second))
    graph.replay()
    torch.cuda.synchronize()
    pool_ref.check_forward(out.cpu().numpy(), e2, second, family)


def test_empty():
    from mtmc_mpn import pool
    e = torch.zeros(0, 2048, device="cuda")
    for out in (pool.pool_tracklets(e, []), pool.pool_tracklets(e, offsets=torch.zeros(1, dtype=torch.int64, device="cuda")),
                pool.pool_tracklets(e.requires_grad_(), [])):
        assert out.shape == (0, 2048) and out.dtype == torch.float32 and out.is_cuda
    assert pool._backward_raw(torch.zeros(0, 2048, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), 0).shape == (0, 2048)
