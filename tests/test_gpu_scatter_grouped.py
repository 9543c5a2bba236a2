"""GPU tests of the repeatable scatter forwards, `scatter_add / scatter_mean / scatter_max(..., deterministic=)`
(mtmc_scatter_grouped over mtmc_group_by_index), against numpy float64 sums written here and against the atomics ops.

Bounds (u = 2^-24; they hold for ANY order of addition, so they fix no implementation): for a group of n rows
  add   |out - exact| <= gamma(n - 1) * sum|x|            gamma(k) = k u / (1 - k u)
  mean  |out - exact / n| <= gamma(n) * sum|x| / n        (n - 1 additions and one division)
A group of one row equals its row bit for bit, integer-valued floats give the exact answer, the maximum and its argmax
equal the atomics op's bit for bit, and every repetition, every way of getting the grouping and a captured replay give
the same bits."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ES, NS, CS = (0, 1, 257, 5000), (1, 7, 450), (1, 3, 4, 32, 33, 260)
PATTERNS = ("uniform", "skew", "sorted", "outside")
U = 2.0 ** -24


def _ops():
    from mtmc_mpn import ops
    return ops


@functools.lru_cache(maxsize=None)
def _index(e, n, pattern):
    rng = np.random.default_rng(1000 * e + n)
    idx = rng.integers(0, n, e)
    if pattern == "skew":                                # one group holds 90 % of the rows: it crosses many chunks
        idx = np.where(rng.random(e) < 0.9, n // 2, idx)
    elif pattern == "sorted":
        idx = np.sort(idx)
    elif pattern == "outside":
        bad = rng.random(e) < 0.2
        idx = np.where(bad, rng.choice(np.array([-1, n, n + 5, 2 ** 40, np.iinfo(np.int64).min]), e), idx)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def _src(e, c, family):
    rng = np.random.default_rng(7 * e + c)
    if family == "gauss":
        x = rng.standard_normal((e, c)).astype(np.float32)
    else:                                                # small integers with ties, +0 and -0
        x = rng.integers(-3, 4, (e, c)).astype(np.float32)
        x[(x == 0) & (rng.random((e, c)) < 0.5)] = -0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _exact(e, n, c, pattern, family):
    """(sum [n, c], sum of |x| [n, c], count [n]) in float64."""
    idx, x = _index(e, n, pattern), _src(e, c, family).astype(np.float64)
    ok = (idx >= 0) & (idx < n)
    s, a = np.zeros((n, c)), np.zeros((n, c))
    np.add.at(s, idx[ok], x[ok])
    np.add.at(a, idx[ok], np.abs(x[ok]))
    return s, a, np.bincount(idx[ok], minlength=n).astype(np.int64)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _gamma(k):
    k = np.maximum(k, 0).astype(np.float64)
    return k * U / (1.0 - k * U)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("e", ES)
def test_max_equals_the_atomics_op_bit_for_bit(e, n, pattern):
    ops = _ops()
    index = _cuda(_index(e, n, pattern))
    for c in CS:
        src = _cuda(_src(e, c, "ints"))
        want, want_arg = ops.scatter_max(src, index, dim_size=n)
        got, got_arg = ops.scatter_max(src, index, dim_size=n, deterministic=True)
        assert _same_bits(got, want), (e, n, c)
        assert got_arg.dtype == torch.int64 and torch.equal(got_arg, want_arg), (e, n, c)
        count = _exact(e, n, c, pattern, "ints")[2]
        empty = _cuda(count == 0)
        assert bool((got[empty] == 0).all()) and bool((got_arg[empty] == e).all())     # untouched rows: 0, argmax E


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("e", ES)
def test_integer_valued_sums_are_exact(e, n, pattern):
    ops = _ops()
    index = _cuda(_index(e, n, pattern))
    for c in CS:
        src = _cuda(_src(e, c, "ints"))                  # |sum| <= 3 * 5000: exact in fp32
        s, _, count = _exact(e, n, c, pattern, "ints")
        add = ops.scatter_add(src, index, dim_size=n, deterministic=True).cpu().numpy()
        mean = ops.scatter_mean(src, index, dim_size=n, deterministic=True).cpu().numpy()
        assert add.shape == (n, c) and add.dtype == np.float32
        assert np.array_equal(add.astype(np.float64), s), (e, n, c)
        want_mean = (s.astype(np.float32) / np.maximum(count, 1).astype(np.float32)[:, None])      # one fp32 division
        assert np.array_equal(mean, want_mean), (e, n, c)
        assert not np.signbit(add[count == 0]).any() and not add[count == 0].any()                 # untouched rows: +0


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("e", ES)
def test_gaussian_sums_within_the_bound_of_any_order(e, n, pattern):
    ops = _ops()
    idx = _index(e, n, pattern)
    index = _cuda(idx)
    for c in CS:
        x = _src(e, c, "gauss")
        src = _cuda(x)
        s, a, count = _exact(e, n, c, pattern, "gauss")
        cnt = count[:, None]
        add = ops.scatter_add(src, index, dim_size=n, deterministic=True).cpu().numpy().astype(np.float64)
        mean = ops.scatter_mean(src, index, dim_size=n, deterministic=True).cpu().numpy().astype(np.float64)
        err_add, bound_add = np.abs(add - s), _gamma(cnt - 1) * a
        err_mean, bound_mean = np.abs(mean - s / np.maximum(cnt, 1)), _gamma(cnt) * a / np.maximum(cnt, 1)
        print(f"E={e} N={n} C={c} {pattern}: add err/bound {err_add.max():.3e}/{bound_add.max():.3e}, "
              f"mean {err_mean.max():.3e}/{bound_mean.max():.3e}")
        assert (err_add <= bound_add).all(), (e, n, c)
        assert (err_mean <= bound_mean).all(), (e, n, c)
        ok = (idx >= 0) & (idx < n)
        for g in np.flatnonzero(count == 1):             # a group of one row: that row, bit for bit (add and mean)
            row = x[np.flatnonzero(ok & (idx == g))[0]]
            assert np.array_equal(add[g].astype(np.float32).view(np.int32), row.view(np.int32))
            assert np.array_equal(mean[g].astype(np.float32).view(np.int32), row.view(np.int32))


def test_a_single_row_group_keeps_minus_zero():
    ops = _ops()
    src = torch.tensor([[-0.0, 0.0, 1.5, -2.0]], device="cuda")
    index = torch.tensor([2], device="cuda")
    for fn in (ops.scatter_add, ops.scatter_mean):
        out = fn(src, index, dim_size=4, deterministic=True)
        assert _same_bits(out[2:3], src) and not bool(_bits(out[[0, 1, 3]]).any())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("e,n,c", [(5000, 450, 32), (5000, 7, 4), (257, 1, 33), (5000, 7, 260)])
def test_every_way_of_calling_gives_the_same_bits(e, n, c, pattern):
    import mtmc_mpn
    ops = _ops()
    src, index = _cuda(_src(e, c, "gauss")), _cuda(_index(e, n, pattern))
    made = mtmc_mpn.group_by_index(index, n)
    key = torch.where((index >= 0) & (index < n), index, torch.full_like(index, n))
    skey, perm = torch.sort(key, stable=True)
    by_torch = mtmc_mpn.Grouping(index, perm, torch.searchsorted(skey, torch.arange(n + 1, device="cuda")), n)
    assert torch.equal(made.perm, by_torch.perm) and torch.equal(made.offsets, by_torch.offsets)
    for fn in (ops.scatter_add, ops.scatter_mean, ops.scatter_max):
        first = fn(src, index, dim_size=n, deterministic=True)
        calls = [fn(src, index, dim_size=n, deterministic=True), fn(src, index, dim_size=n, deterministic=True),
                 fn(src, index, deterministic=made), fn(src, None, deterministic=made), fn(src, made.index, dim_size=n, deterministic=by_torch)]
        static = src.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = fn(static, index, dim_size=n, deterministic=True)
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for other in calls + [captured]:
            if isinstance(first, tuple):
                assert _same_bits(other[0], first[0]) and torch.equal(other[1], first[1])
            else:
                assert _same_bits(other, first)


@pytest.mark.parametrize("name", ("scatter_add", "scatter_mean", "scatter_max"))
@pytest.mark.parametrize("e,n,c,pattern", [(5000, 450, 32, "uniform"), (5000, 7, 4, "skew"), (257, 7, 33, "outside"),
                                           (1, 1, 1, "uniform"), (0, 7, 4, "uniform")])
def test_gradients_equal_the_atomics_ops(name, e, n, c, pattern):
    import mtmc_mpn
    ops = _ops()
    fn = getattr(ops, name)
    x, index = _cuda(_src(e, c, "ints" if name == "scatter_max" else "gauss")), _cuda(_index(e, n, pattern))
    upstream = _cuda(np.random.default_rng(3).standard_normal((n, c)).astype(np.float32))
    made = mtmc_mpn.group_by_index(index, n)
    grads = []
    for det in (False, True, made):
        leaf = x.clone().requires_grad_()
        out = fn(leaf, index, dim_size=n, deterministic=det)
        out = out[0] if isinstance(out, tuple) else out
        if name == "scatter_max":                        # the forward is bit-equal: the whole chain is compared
            (out * upstream).sum().backward()
        else:
            out.backward(upstream)
        assert leaf.grad is not None and leaf.grad.shape == x.shape
        grads.append(leaf.grad)
    assert _same_bits(grads[1], grads[0]) and _same_bits(grads[2], grads[0])


@pytest.mark.parametrize("name", ("scatter_add", "scatter_mean", "scatter_max"))
def test_forward_and_backward_can_be_captured(name):
    ops = _ops()
    fn = getattr(ops, name)
    e, n, c = 5000, 450, 32
    x, index = _cuda(_src(e, c, "gauss")), _cuda(_index(e, n, "uniform"))
    upstream = _cuda(np.random.default_rng(4).standard_normal((n, c)).astype(np.float32))

    def step(leaf):
        out = fn(leaf, index, dim_size=n, deterministic=True)
        out = out[0] if isinstance(out, tuple) else out
        (grad,) = torch.autograd.grad(out, leaf, upstream)
        return out.detach(), grad
    want_out, want_grad = step(x.clone().requires_grad_())
    static = torch.zeros_like(x).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # (autograd's side-stream warm-up before a capture)
        step(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_out, got_grad = step(static)
    with torch.no_grad():
        static.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(got_out, want_out) and _same_bits(got_grad, want_grad)


def test_other_forms_of_src_behave_as_the_existing_ops_do():
    ops = _ops()
    e, n = 5000, 7
    index = _cuda(_index(e, n, "uniform"))
    wide = _cuda(_src(e, 32, "ints"))
    strided = wide[:, ::2]                               # not contiguous
    assert not strided.is_contiguous()
    flat = wide[:, 0].contiguous()                       # [E]
    cube = wide.reshape(e, 4, 8)                         # [E, 4, 8]
    half = flat.half()
    for src in (strided, flat, cube, half):
        for name in ("scatter_add", "scatter_mean", "scatter_max"):
            want = getattr(ops, name)(src, index, dim_size=n)
            got = getattr(ops, name)(src, index, dim_size=n, deterministic=True)
            if name == "scatter_max":
                assert torch.equal(got[1], want[1]) and _same_bits(got[0], want[0])
                got, want = got[0], want[0]
            assert got.shape == want.shape == (n,) + tuple(src.shape[1:]) and got.dtype == want.dtype
            assert torch.equal(got, want), name          # (integer-valued src: the atomics' sums are exact too)
    # integer src: the exact int64 path of the default call, with either form
    ints = torch.arange(e, device="cuda")
    import mtmc_mpn
    want = ops.scatter_add(ints, index, dim_size=n)
    assert want.dtype == torch.int64
    assert torch.equal(ops.scatter_add(ints, index, dim_size=n, deterministic=True), want)
    assert torch.equal(ops.scatter_add(ints, None, deterministic=mtmc_mpn.group_by_index(index, n)), want)
    with pytest.raises(NotImplementedError):
        ops.scatter_add(wide, index, dim=1, dim_size=n, deterministic=True)
