"""GPU tests of the backward of scatter_add / scatter_mean / scatter_max (csrc/scatter_ops.hip, torch_ops.py).

The yardstick is the test-only stand-in tests/golden/_standin/torch_scatter (pinned by tests/test_oracle.py::
test_scatter_known_answers), run on the CPU under torch autograd on the rows whose index is in range (the stand-in's
scatter_add_ refuses the others; indexing them away gives their rows the zero gradient the forward's skip implies), and for
max also the explicit rule d_src[e, c] = g[r, c] if arg[r, c] == e else 0 with arg recomputed on the CPU.

The bounds are derived, not measured (u = 2^-24):
  add, max   copies of g: torch.equal with the yardstick's fp32 gradient
  mean       |got - g64/count| <= 3u |g64/count| (the bound pool_ref.check_backward uses for g/len; a correctly rounded
             division needs u), exactly 0 where g is 0, bit-equal to g/count where count is a power of two.  On the one large
             case (the S02 message shape) "equals the yardstick" is taken with this bound for mean, torch.equal for add and max.
Gradients g are gaussian with the small values set to exactly 0: no denormals, and zeros to find again.
"""
import functools
import importlib.util
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
OPS = ("add", "mean", "max")
COLS = ((), (3,), (4,), (5,), (32,), (36,), (2, 4))           # (): the 1-D call form, C = 1
ES = (1, 63, 257, 1000)
NS = (1, 7, 301)


@functools.lru_cache(maxsize=None)
def _standin():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "_standin", "torch_scatter", "__init__.py")
    spec = importlib.util.spec_from_file_location("torch_scatter_standin", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _weights(shape, gen):
    r = torch.randn(shape, generator=gen)
    r[r.abs() < 0.1] = 0.0
    return r


def _inputs(cols, e, n, seed, integer=False, stray=False):
    """src [e, *cols], index [e] with destination row n - 1 left empty (n > 1), the weights R [n, *cols] of the loss."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 3, (e,) + cols, generator=gen).float() if integer else torch.randn((e,) + cols, generator=gen)
    idx = torch.randint(0, max(n - 1, 1), (e,), generator=gen)
    if stray:                                                   # a fifth of the rows point outside [0, n)
        where = torch.rand(e, generator=gen) < 0.2
        bad = torch.tensor([-1, -7, n, n + 100, -(2 ** 40), 2 ** 40])[torch.randint(0, 6, (e,), generator=gen)]
        idx = torch.where(where, bad, idx)
    return src, idx, _weights((n,) + cols, gen)


def _yardstick(src, idx, n, R):
    """The stand-in's gradients of sum(scatter(src) * R) with respect to src, the CPU argmax, the explicit max rule, counts."""
    ts = _standin()
    e = src.shape[0]
    pos = ((idx >= 0) & (idx < n)).nonzero()[:, 0]
    r = idx[pos]
    out = types.SimpleNamespace(pos=pos, count=torch.bincount(r, minlength=n))
    for name in OPS:
        leaf = src.clone().requires_grad_()
        y = getattr(ts, "scatter_" + name)(leaf[pos], r, dim=0, dim_size=n)
        if name == "max":
            y, arg_sub = y
            hit = arg_sub < pos.numel()
            out.arg = torch.where(hit, pos[arg_sub.clamp(max=max(pos.numel() - 1, 0))], torch.full_like(arg_sub, e)) \
                if pos.numel() else torch.full_like(arg_sub, e)
        (y * R).sum().backward()
        setattr(out, name if name != "max" else "max_autograd", leaf.grad)
    c = max(R[0].numel(), 1)
    rule = torch.zeros(e, c)
    rule[pos] = torch.where(out.arg.reshape(n, c)[r] == pos[:, None], R.reshape(n, c)[r], torch.zeros(()))
    out.max = rule.reshape(src.shape)
    return out


def _gpu(name, src, idx, n, R, loss=None):
    """src.grad (and the forward's argmax) of the loss through mtmc_mpn.ops.scatter_<name> on the GPU."""
    from mtmc_mpn import ops
    leaf = src.cuda().requires_grad_()
    out = getattr(ops, "scatter_" + name)(leaf, idx.cuda(), dim=0, dim_size=n)
    arg = None
    if name == "max":
        out, arg = out
        assert arg.dtype == torch.int64 and not arg.requires_grad
    assert out.requires_grad and out.dtype == torch.float32
    (loss(out) if loss else (out * R.cuda()).sum()).backward()
    assert leaf.grad.shape == src.shape and leaf.grad.dtype == src.dtype
    return leaf.grad.cpu(), (arg.cpu() if arg is not None else None)


def _check_mean(got, idx, n, R, scale=1.0):
    e = got.shape[0]
    c = max(R[0].numel(), 1)
    got, R2 = got.reshape(e, c), R.reshape(n, c) * scale
    keep = (idx >= 0) & (idx < n)
    pos = keep.nonzero()[:, 0]
    r = idx[pos]
    count = torch.bincount(r, minlength=n).clamp(min=1)[r]
    ref = torch.zeros(e, c, dtype=torch.float64)
    ref[pos] = R2[r].double() / count.double()[:, None]
    assert (got[~keep] == 0).all()
    assert ((got.double() - ref).abs() <= 3 * U * ref.abs()).all()
    assert (got[ref == 0] == 0).all()
    pow2 = (count & (count - 1)) == 0
    assert torch.equal(got[pos][pow2], (R2[r] / count.float()[:, None])[pow2])


def _check(name, got, arg, src, idx, n, R, ties=False):
    want = _yardstick(src, idx, n, R)
    if name == "add":
        assert torch.equal(got, want.add)
    elif name == "mean":
        _check_mean(got, idx, n, R)
    else:
        assert torch.equal(arg, want.arg)
        assert torch.equal(got, want.max)
        if not ties:
            assert torch.equal(got, want.max_autograd)


@pytest.mark.parametrize("e", ES)
@pytest.mark.parametrize("cols", COLS, ids=lambda c: "x".join(map(str, c)) or "1d")
def test_every_shape_against_the_stand_in(cols, e):
    for k, n in enumerate(NS):
        src, idx, R = _inputs(cols, e, n, seed=17 * e + n)
        for name in OPS:
            got, arg = _gpu(name, src, idx.int() if (e + k) % 2 else idx, n, R)          # int32 and int64 index in turn
            _check(name, got, arg, src, idx, n, R)


@pytest.mark.parametrize("name", OPS)
def test_int32_and_int64_index_agree(name):
    src, idx, R = _inputs((32,), 1000, 301, seed=3)
    a, _ = _gpu(name, src, idx, 301, R)
    b, arg = _gpu(name, src, idx.int(), 301, R)
    assert torch.equal(a, b)
    _check(name, b, arg, src, idx, 301, R)


@pytest.mark.parametrize("cols", [(), (4,), (5,), (32,)], ids=lambda c: "x".join(map(str, c)) or "1d")
@pytest.mark.parametrize("name", OPS)
def test_rows_outside_the_range_get_zeros(name, cols):
    e, n = 1000, 7
    src, idx, R = _inputs(cols, e, n, seed=5, stray=True)
    stray = (idx < 0) | (idx >= n)
    assert 100 < int(stray.sum()) < 400 and (idx < 0).any() and (idx >= n).any()
    got, arg = _gpu(name, src, idx, n, R)
    assert (got[stray] == 0).all()
    _check(name, got, arg, src, idx, n, R)
    # the rows in range get what they get without the strays
    alone, _ = _gpu(name, src[~stray], idx[~stray], n, R)
    assert torch.equal(got[~stray], alone)


@pytest.mark.parametrize("name", OPS)
def test_no_rows(name):
    from mtmc_mpn import ops
    for shape in ((0, 4), (0,), (0, 2, 4)):
        leaf = torch.zeros(shape, device="cuda", requires_grad=True)
        out = getattr(ops, "scatter_" + name)(leaf, torch.zeros(0, dtype=torch.int64, device="cuda"), dim=0, dim_size=5)
        out = out[0] if name == "max" else out
        assert out.shape == (5,) + shape[1:] and (out == 0).all()
        out.sum().backward()
        assert leaf.grad.shape == shape and leaf.grad.dtype == torch.float32
    g = torch.ones(5, 4, device="cuda")
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert torch.ops.mtmc_mpn.scatter_add_backward(g, none, 0).shape == (0, 4)
    assert torch.ops.mtmc_mpn.scatter_mean_backward(g, none, 0).shape == (0, 4)
    assert torch.ops.mtmc_mpn.scatter_max_backward(g, torch.zeros(5, 4, dtype=torch.int64, device="cuda"), none, 0).shape == (0, 4)


def test_no_destination_rows_give_zeros():
    """dim_size = 0 through the backward ops: every index is out of range, there is no gradient row to read."""
    idx = torch.tensor([0, 3, -1], device="cuda")
    g = torch.zeros(0, 4, device="cuda")
    for d in (torch.ops.mtmc_mpn.scatter_add_backward(g, idx, 3), torch.ops.mtmc_mpn.scatter_mean_backward(g, idx, 3),
              torch.ops.mtmc_mpn.scatter_max_backward(g, torch.zeros(0, 4, dtype=torch.int64, device="cuda"), idx, 3)):
        assert d.shape == (3, 4) and (d == 0).all()


def test_misaligned_gradient_and_argmax():
    """C = 4 with g (then arg) 4 (8) bytes off a 16-byte boundary: contiguous, so no copy is made -- the one-column-per-lane
    kernels must take it, and give what the 16-byte kernels give on the aligned copy."""
    e, n = 257, 7
    src, idx, R = _inputs((4,), e, n, seed=9)
    want = _yardstick(src, idx, n, R)
    buf = torch.zeros(4 * n + 1).cuda()
    g = buf[1:].view(n, 4)
    g.copy_(R)
    assert g.is_contiguous() and g.data_ptr() % 16 == 4
    abuf = torch.zeros(4 * n + 1, dtype=torch.int64).cuda()
    arg_off = abuf[1:].view(n, 4)
    arg_off.copy_(want.arg)
    assert arg_off.is_contiguous() and arg_off.data_ptr() % 16 == 8
    arg, i = want.arg.cuda(), idx.cuda()
    assert torch.equal(torch.ops.mtmc_mpn.scatter_add_backward(g, i, e).cpu(), want.add)
    _check_mean(torch.ops.mtmc_mpn.scatter_mean_backward(g, i, e).cpu(), idx, n, R)
    assert torch.equal(torch.ops.mtmc_mpn.scatter_mean_backward(g, i, e), torch.ops.mtmc_mpn.scatter_mean_backward(R.cuda(), i, e))
    for grad, a in ((g, arg), (R.cuda(), arg_off), (g, arg_off), (R.cuda(), arg)):
        assert torch.equal(torch.ops.mtmc_mpn.scatter_max_backward(grad, a, i, e).cpu(), want.max)


@pytest.mark.parametrize("cols", [(), (4,), (5,)], ids=lambda c: "x".join(map(str, c)) or "1d")
def test_max_with_ties_gives_the_gradient_to_the_smallest_row(cols):
    e, n = 1000, 7
    src, idx, R = _inputs(cols, e, n, seed=11, integer=True)
    got, arg = _gpu("max", src, idx, n, R)
    _check("max", got, arg, src, idx, n, R, ties=True)
    c = max(R[0].numel(), 1)
    got2, src2, R2 = got.reshape(e, c), src.reshape(e, c), R.reshape(n, c)
    for r in range(n - 1):                                  # many rows attain the maximum, one gets the gradient: the first
        rows = (idx == r).nonzero()[:, 0]
        for col in range(c):
            attain = rows[src2[rows, col] == src2[rows, col].max()]
            assert attain.numel() > 1
            assert got2[attain[0], col] == R2[r, col] and (got2[attain[1:], col] == 0).all()
            assert int((got2[rows, col] != 0).sum()) == int(R2[r, col] != 0)


def test_max_gradient_of_an_unwritten_destination_goes_nowhere():
    e, n = 63, 7
    src, idx, R = _inputs((4,), e, n, seed=13)
    R[n - 1] = 12345.0
    assert not (idx == n - 1).any()
    got, arg = _gpu("max", src, idx, n, R)
    assert (arg[n - 1] == e).all() and not (got == 12345.0).any()
    _check("max", got, arg, src, idx, n, R)


@pytest.mark.parametrize("name", OPS)
def test_expanded_gradient(name):
    """out.sum().backward() hands the backward a stride-0 gradient of ones."""
    e, n = 257, 7
    src, idx, _ = _inputs((4,), e, n, seed=15)
    got, arg = _gpu(name, src, idx, n, None, loss=lambda out: out.sum())
    _check(name, got, arg, src, idx, n, torch.ones(n, 4))


@pytest.mark.parametrize("name", OPS)
def test_upstream_of_the_aggregation(name):
    """a -> src = 2 a -> scatter -> loss: a.grad = 2 d_src, the path that got no gradient before."""
    from mtmc_mpn import ops
    e, n = 257, 7
    src, idx, R = _inputs((5,), e, n, seed=19)
    a = (src / 2).cuda().requires_grad_()
    out = getattr(ops, "scatter_" + name)(a * 2, idx.cuda(), dim=0, dim_size=n)
    out = out[0] if name == "max" else out
    (out * R.cuda()).sum().backward()
    assert a.grad is not None
    want = _yardstick(src, idx, n, R)
    if name == "mean":
        _check_mean(a.grad.cpu(), idx, n, R, scale=2.0)
    else:
        assert torch.equal(a.grad.cpu(), 2 * getattr(want, name))


@pytest.mark.parametrize("name", OPS)
def test_half_precision_src_gets_a_half_precision_gradient(name):
    e, n = 257, 7
    src, idx, R = _inputs((4,), e, n, seed=21)
    src = src.half()
    got, _ = _gpu(name, src, idx, n, R)
    assert got.dtype == torch.float16
    want = _yardstick(src.float(), idx, n, R)
    assert torch.equal(got, getattr(want, name).half())


def test_mean_with_more_destinations_than_the_on_chip_counters():
    """dim_size above the 8192 counters a workgroup keeps on chip: the count goes straight to memory."""
    e, n = 1000, 9000
    src, idx, R = _inputs((4,), e, n, seed=23)
    idx[:300] = 8999 - torch.arange(300) % 3                 # some rows share a far destination
    got, _ = _gpu("mean", src, idx, n, R)
    _check_mean(got, idx, n, R)
    counts = torch.bincount(idx, minlength=n)
    assert int(counts.max()) >= 100 and int((counts == 0).sum()) > 8000


@functools.lru_cache(maxsize=None)
def _s02():
    """The message shape of the S02 graph: E = 150 454 messages of C = 32 onto N = 450 nodes, index = camera_graph()'s rows
    (a stride-2 view, as the callers pass it).  The yardstick is computed once."""
    from mtmc_mpn import graphs
    cam_of_node = torch.repeat_interleave(torch.arange(len(graphs.S02_GT_CAMS)), torch.tensor(graphs.S02_GT_CAMS))
    idx = graphs.camera_edge_index(cam_of_node)[0]
    gen = torch.Generator().manual_seed(30)
    src, R = torch.randn(idx.numel(), 32, generator=gen), _weights((450, 32), gen)
    assert idx.numel() == 150454 and not idx.is_contiguous()
    want = _yardstick(src, idx, 450, R)
    assert torch.equal(want.max, want.max_autograd)          # (of the data: no two rows of a node share a column's maximum)
    return src, idx, R, want


@pytest.mark.parametrize("name", OPS)
def test_s02_messages_repeat_bit_for_bit(name):
    src, idx, R, want = _s02()
    a, arg = _gpu(name, src, idx, 450, R)
    b, _ = _gpu(name, src, idx, 450, R)
    assert torch.equal(a, b)
    if name == "mean":
        _check_mean(a, idx, 450, R)
    else:
        assert torch.equal(a, getattr(want, name))
    if name == "max":
        assert torch.equal(arg, want.arg) and torch.equal(a, want.max_autograd)


@pytest.mark.parametrize("name", OPS)
def test_opcheck_with_gradients(name):
    src, idx, _ = _inputs((4,), 63, 7, seed=31)
    op = getattr(torch.ops.mtmc_mpn, "scatter_" + name)
    torch.library.opcheck(op, (src.cuda().requires_grad_(), idx.cuda(), 0, 7),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


@pytest.mark.parametrize("name", OPS)
def test_captured_forward_and_backward(name):
    """Forward + backward inside torch.cuda.graph with dim_size given: nothing synchronises or allocates outside torch's
    allocator, and a replay gives the eager gradient."""
    e, n = 1000, 301
    src, idx, R = _inputs((32,), e, n, seed=37)
    eager, _ = _gpu(name, src, idx, n, R)
    op = getattr(torch.ops.mtmc_mpn, "scatter_" + name)
    leaf, i, w = src.cuda().requires_grad_(), idx.cuda(), R.cuda()

    def grad():
        out = op(leaf, i, 0, n)
        out = out[0] if name == "max" else out
        return torch.autograd.grad((out * w).sum(), leaf)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        grad()                                              # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        d = grad()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), eager)
    w.mul_(2.0)                                             # the replay reads the tensors of the capture
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), 2 * eager)
