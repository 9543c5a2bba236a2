"""GPU tests of `pool_tracklets(index=, num_tracklets=, weights=)` against tests/pool_weighted_ref.py (numpy float64).

The bounds are derived in the yardstick's docstring, not measured (u = 2^-24, len = rows of the tracklet):
  forward    (2 len + 4) u A;  integer embeds with integer weights: 3u |S/W|, exactly 0 where S = 0
  d_embeds   (len + 3) u |want|;  3u with integer weights
  d_weights  (F + 3 len + 8) u B_r
Bit-equalities: all weights 1 (or one power of two) against the plain call; a sorted index against lengths; an order-keeping
interleaving against the grouped call; a 0/1 mask on integer embeds against the repacked call.
R below is pool.CHUNK_ROWS, the rows per chunk of the kernels' decomposition.
"""
import functools

import numpy as np
import pytest
import torch

import pool_ref
import pool_weighted_ref as ref

pytestmark = pytest.mark.gpu

FAMILIES = ("integer", "gaussian")
GEN = {"integer": pool_ref.integer_embeds, "gaussian": pool_ref.gaussian_embeds}
WGEN = {"integer": ref.integer_weights, "uniform": ref.uniform_weights}


def _r():
    from mtmc_mpn import pool
    return pool.CHUNK_ROWS


def _lengths(name):
    r = _r()
    every = tuple(range(1, 2 * r + 3))
    return {"ascending": every, "shuffled": tuple(int(v) for v in np.random.default_rng(5).permutation(every)),
            "edges": (r - 1, r, r + 1, 2 * r, 2 * r + 1, 1, 3 * r + 5), "skew": (1, 20 * r + 3, 1, 2, 7 * r, 1)}[name]


@functools.lru_cache(maxsize=None)
def _inputs(name, f, family, wfamily="uniform", seed=0):
    """embeds [D, f], a gradient [N, f] and weights [D] of one case (numpy, read-only: shared between tests)."""
    lengths = _lengths(name)
    e = GEN[family](sum(lengths), f, seed + 1)
    g = GEN[family](len(lengths), f, seed + 2)
    w = WGEN[wfamily](sum(lengths), seed + 3)
    for a in (e, g, w):
        a.setflags(write=False)
    return e, g, w


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _run(e, g, w=None, lengths=None, index=None, n=None, want_dw=True):
    """Forward and backward through the public function: (out, d_embeds, d_weights or None) as numpy arrays."""
    from mtmc_mpn import pool_tracklets
    leaf = _cuda(e).requires_grad_()
    wleaf = None if w is None else _cuda(w).requires_grad_(want_dw)
    kw = {} if index is None else {"index": _cuda(index), "num_tracklets": n}
    out = pool_tracklets(leaf, None if lengths is None else list(lengths), weights=wleaf, **kw)
    out.backward(_cuda(g))
    dw = None if wleaf is None or wleaf.grad is None else wleaf.grad.cpu().numpy()
    return out.detach().cpu().numpy(), leaf.grad.cpu().numpy(), dw


CASES = [("ascending", 256), ("shuffled", 260), ("edges", 2048), ("skew", 100), ("skew", 4)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,f", CASES)
def test_weights_of_one_have_the_bits_of_the_plain_call(name, f, family):
    lengths = _lengths(name)
    e, g, _ = _inputs(name, f, family)
    plain, plain_grad, _ = _run(e, g, lengths=lengths)
    for c in (1.0, 4.0, 0.25):                                   # a constant power of two scales every sum exactly
        out, grad, dw = _run(e, g, np.full(e.shape[0], c, np.float32), lengths=lengths)
        assert np.array_equal(out, plain) and np.array_equal(grad, plain_grad), c
        assert dw.shape == (e.shape[0],) and np.isfinite(dw).all()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("wfamily", ["integer", "uniform"])
@pytest.mark.parametrize("name,f", CASES)
def test_against_the_yardstick(name, f, wfamily, family):
    lengths = _lengths(name)
    e, g, w = _inputs(name, f, family, wfamily)
    seg, n = ref.seg_of_lengths(lengths), len(lengths)
    out, grad, dw = _run(e, g, w, lengths=lengths)
    assert out.shape == (n, f) and out.dtype == np.float32
    worst = [ref.check_forward(out, e, seg, w, n),
             ref.check_d_embeds(grad, g, seg, w, n, integer_weights=wfamily == "integer"),
             ref.check_d_weights(dw, e, g, seg, w, n)]
    if family == "integer" and wfamily == "integer":
        worst.append(ref.check_forward(out, e, seg, w, n, exact_integers=True))
    print(f"{name} F={f} {family}/{wfamily}: worst err / bound = " + ", ".join(f"{v:.3f}" for v in worst))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,f", [("shuffled", 260), ("edges", 2048), ("skew", 100)])
def test_index_forms_have_the_bits_of_the_grouped_call(name, f, family):
    from mtmc_mpn import pool_tracklets
    lengths = _lengths(name)
    e, g, w = _inputs(name, f, family)
    seg, n = ref.seg_of_lengths(lengths), len(lengths)
    grouped = _run(e, g, w, lengths=lengths)
    # a sorted index is the lengths form
    for got, want in zip(_run(e, g, w, index=seg, n=n), grouped):
        assert np.array_equal(got, want)
    assert torch.equal(pool_tracklets(_cuda(e), index=_cuda(seg), num_tracklets=n), pool_tracklets(_cuda(e), list(lengths)))
    # frame order: tracklets interleaved, each keeping its internal order
    index, place = ref.interleave(lengths, seed=7)
    mixed_e, mixed_w = np.empty_like(e), np.empty_like(w)
    mixed_e[place], mixed_w[place] = e, w
    out, grad, dw = _run(mixed_e, g, mixed_w, index=index, n=n)
    assert np.array_equal(out, grouped[0]) and np.array_equal(grad[place], grouped[1]) and np.array_equal(dw[place], grouped[2])
    ref.check_forward(out, mixed_e, index, mixed_w, n)
    ref.check_d_weights(dw, mixed_e, g, index, mixed_w, n)
    # ... and without weights: the plain call's bits
    out, grad, _ = _run(mixed_e, g, index=index, n=n)
    plain = _run(e, g, lengths=lengths)
    assert np.array_equal(out, plain[0]) and np.array_equal(grad[place], plain[1])


def test_a_single_weight_of_one_copies_the_row():
    lengths = _lengths("edges")
    e, g, _ = _inputs("edges", 260, "gaussian")
    seg, n = ref.seg_of_lengths(lengths), len(lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    pick = starts + np.array([(3 * k) % m for k, m in enumerate(lengths)])     # first, middle and last chunks alike
    w = np.zeros(e.shape[0], np.float32)
    w[pick] = 1.0
    out, grad, dw = _run(e, g, w, lengths=lengths)
    assert np.array_equal(out, e[pick])
    want = np.zeros_like(e)
    want[pick] = g
    assert np.array_equal(grad, want)
    ref.check_d_weights(dw, e, g, seg, w, n)
    assert np.all(dw[pick] == 0)                                  # x_r - out[s] is exactly 0 there


def test_a_mask_equals_the_repacked_call():
    from mtmc_mpn import pool_tracklets
    lengths = _lengths("shuffled")
    e, _, _ = _inputs("shuffled", 260, "integer")
    seg, n = ref.seg_of_lengths(lengths), len(lengths)
    keep = np.random.default_rng(3).random(e.shape[0]) < 0.6
    keep[seg == 4] = False                                        # one tracklet loses every row
    kept = np.bincount(seg[keep], minlength=n)
    some = kept > 0
    assert (~some).sum() >= 1 and some.sum() > n // 2
    masked = pool_tracklets(_cuda(e), list(lengths), weights=_cuda(keep.astype(np.float32)))
    repacked = pool_tracklets(_cuda(e[keep & some[seg]]), kept[some].tolist())
    assert torch.equal(masked[_cuda(some)], repacked) and (masked[_cuda(~some)] == 0).all()


def test_weight_in_the_middle_chunk_and_chunks_of_zeros():
    from mtmc_mpn import pool
    r = _r()
    lengths = (5, 4 * r + 7, 3, 2 * r, r, 2)                      # tracklet 1 spans chunks 0..4, tracklet 3 has no weight
    seg, n, f = ref.seg_of_lengths(lengths), len(lengths), 260
    d = seg.size
    e, g = pool_ref.gaussian_embeds(d, f, 41), pool_ref.gaussian_embeds(n, f, 42)
    w = ref.uniform_weights(d, 43) + np.float32(0.125)
    w[(seg == 1) & ((np.arange(d) // r) != 2)] = 0.0              # all of tracklet 1's weight in its middle chunk
    w[seg == 3] = 0.0
    assert w[2 * r:3 * r].min() > 0 and w[r:2 * r].max() == 0     # a whole chunk of zeros on either side of it
    out, grad, dw = _run(e, g, w, lengths=lengths)
    ref.check_forward(out, e, seg, w, n)
    ref.check_d_embeds(grad, g, seg, w, n)
    ref.check_d_weights(dw, e, g, seg, w, n)
    assert np.all(out[3] == 0) and np.all(grad[seg == 3] == 0) and np.all(dw[seg == 3] == 0)
    info = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device="cuda")
    _, wsum = pool._forward_weighted_raw(_cuda(e), off, weights=_cuda(w), info=info)
    assert info.cpu().tolist() == [0, 0, 1, 0]                    # one zero row, counted; no offence
    assert wsum.cpu()[3] == 0 and np.allclose(wsum.cpu().numpy(), ref.weight_sums(seg, w, n), rtol=d * ref.U)


def test_index_values_nobody_names_and_values_out_of_range():
    from mtmc_mpn import pool, pool_tracklets
    r = _r()
    n, f, d = 9, 100, 3 * r + 5
    rng = np.random.default_rng(51)
    index = rng.choice([0, 2, 3, 7], size=d).astype(np.int64)     # ids 1, 4, 5, 6, 8 never occur
    e, g, w = pool_ref.gaussian_embeds(d, f, 52), pool_ref.gaussian_embeds(n, f, 53), ref.uniform_weights(d, 54)
    out, grad, dw = _run(e, g, w, index=index, n=n)
    ref.check_forward(out, e, index, w, n)
    assert np.all(out[[1, 4, 5, 6, 8]] == 0)
    ref.check_d_embeds(grad, g, index, w, n)
    ref.check_d_weights(dw, e, g, index, w, n)
    perm, off = pool.group_by_index(_cuda(index), n)
    want_perm, want_off = ref.stable_group(index, n)
    assert np.array_equal(perm.cpu().numpy(), want_perm) and np.array_equal(off.cpu().numpy(), want_off)
    info = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    pool._forward_weighted_raw(_cuda(e), off, perm=perm, info=info)
    assert info.cpu().tolist() == [0, 0, 5, 0]
    # -1, N and 2^40 belong to no tracklet
    bad = index.copy()
    where = np.array([0, r, d - 1])
    bad[where] = [-1, n, 2 ** 40]
    for kw in ({}, {"weights": _cuda(w)}):
        with pytest.raises(RuntimeError, match="index"):
            pool_tracklets(_cuda(e), index=_cuda(bad), num_tracklets=n, **kw)
    leaf, wleaf = _cuda(e).requires_grad_(), _cuda(w).requires_grad_()
    out = pool_tracklets(leaf, index=_cuda(bad), num_tracklets=n, weights=wleaf, check=False)
    out.backward(_cuda(g))
    ref.check_forward(out.detach().cpu().numpy(), e, bad, w, n)
    ref.check_d_embeds(leaf.grad.cpu().numpy(), g, bad, w, n)
    ref.check_d_weights(wleaf.grad.cpu().numpy(), e, g, bad, w, n)
    assert (leaf.grad[_cuda(where)] == 0).all() and (wleaf.grad[_cuda(where)] == 0).all()
    perm, off = pool.group_by_index(_cuda(bad), n)
    pool._forward_weighted_raw(_cuda(e), off, perm=perm, info=info)
    assert info.cpu().tolist()[0] == 0 and info.cpu().tolist()[3] == 3


def test_raw_entry_point_with_a_bad_perm():
    """The kernels' own guard (as test_device_offsets_status for the offsets): a perm entry outside [0, D) names no row."""
    from mtmc_mpn import pool
    r = _r()
    lengths = (3, r + 4, 2)
    seg, n, f = ref.seg_of_lengths(lengths), len(lengths), 32
    d = seg.size
    e, g = pool_ref.gaussian_embeds(d, f, 61), pool_ref.gaussian_embeds(n, f, 62)
    perm = np.arange(d, dtype=np.int64)
    perm[[1, r + 2]] = [-1, d + 5]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device="cuda")
    info = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    out, wsum = pool._forward_weighted_raw(_cuda(e), off, perm=_cuda(perm), info=info)
    assert info.cpu().tolist() == [4, 0, 0, 2]
    dropped = seg.copy()
    dropped[[1, r + 2]] = -1
    ref.check_forward(out.cpu().numpy(), e, dropped, np.ones(d, np.float32), n)
    assert wsum.cpu().tolist() == [2.0, float(r + 3), 2.0]
    buf = torch.full((d, f), float("nan"), device="cuda")
    grad = pool._backward_weighted_raw(_cuda(g), off, d, wsum, perm=_cuda(perm), out=buf).cpu().numpy()
    assert np.isnan(grad[[1, r + 2]]).all()                       # named by no entry: not written
    keep = dropped >= 0
    ref.check_d_embeds(grad[keep], g, seg[keep], np.ones(keep.sum(), np.float32), n)
    dw = pool._weight_grad_raw(_cuda(e), _cuda(g), out, off, wsum, perm=_cuda(perm)).cpu().numpy()
    assert np.all(dw[[1, r + 2]] == 0) and np.isfinite(dw).all()
    pool._forward_weighted_raw(_cuda(e), off, perm=_cuda(np.arange(d, dtype=np.int64)), info=info)
    assert info.cpu().tolist() == [0, 0, 0, 0]


def test_bad_weights_are_reported_and_count_as_zero():
    from mtmc_mpn import pool, pool_tracklets
    lengths = (4, _r() + 3, 2)
    seg, n, f = ref.seg_of_lengths(lengths), len(lengths), 32
    d = seg.size
    e = pool_ref.gaussian_embeds(d, f, 71)
    w = ref.uniform_weights(d, 72) + np.float32(0.5)
    w[[0, 6, d - 1]] = [-1.0, np.inf, np.nan]
    with pytest.raises(RuntimeError, match="weights"):
        pool_tracklets(_cuda(e), list(lengths), weights=_cuda(w))
    out = pool_tracklets(_cuda(e), list(lengths), weights=_cuda(w), check=False)
    cleaned = w.copy()
    cleaned[[0, 6, d - 1]] = 0.0
    ref.check_forward(out.cpu().numpy(), e, seg, cleaned, n)
    info = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device="cuda")
    pool._forward_weighted_raw(_cuda(e), off, weights=_cuda(w), info=info)
    assert info.cpu().tolist() == [8, 0, 0, 0]


@pytest.mark.parametrize("family", FAMILIES)
def test_strided_views_and_poisoned_neighbours(family):
    from mtmc_mpn import pool
    name, f, pad = "edges", 260, 3
    lengths = _lengths(name)
    e, g, w = _inputs(name, f, family)
    seg, n = ref.seg_of_lengths(lengths), len(lengths)
    d = e.shape[0]
    index, place = ref.interleave(lengths, seed=8)
    mixed_e, mixed_w = np.empty_like(e), np.empty_like(w)
    mixed_e[place], mixed_w[place] = e, w
    nan = float("nan")
    big = torch.full((d + 2 * pad, f + 64), nan, device="cuda")
    big[pad:pad + d, 32:32 + f] = _cuda(mixed_e)
    view = big[pad:pad + d, 32:32 + f]
    assert view.stride(0) == f + 64 and not view.is_contiguous()
    wbuf = torch.full((2 * d + 2,), nan, device="cuda")
    wbuf[1:2 * d + 1:2] = _cuda(mixed_w)
    wview = wbuf[1:2 * d + 1:2]
    assert wview.stride(0) == 2
    out = pool.pool_tracklets(view, index=_cuda(index), num_tracklets=n, weights=wview)
    assert out.is_contiguous() and not torch.isnan(out).any()
    ref.check_forward(out.cpu().numpy(), mixed_e, index, mixed_w, n)
    # the raw calls into buffers with poison around them
    perm, off = pool.group_by_index(_cuda(index), n)
    wdev = _cuda(mixed_w)
    out_buf = torch.full((n + 2, f), nan, device="cuda")
    sum_buf = torch.full((n + 2,), nan, device="cuda")
    out2, wsum = pool._forward_weighted_raw(view, off, perm=perm, weights=wdev, out=out_buf[1:n + 1], wsum=sum_buf[1:n + 1])
    assert torch.equal(out2, out) and not torch.isnan(wsum).any()
    assert torch.isnan(out_buf[0]).all() and torch.isnan(out_buf[-1]).all() and torch.isnan(sum_buf[[0, -1]]).all()
    assert torch.isnan(big[:pad]).all() and torch.isnan(big[pad + d:]).all() and torch.isnan(big[:, :32]).all()
    assert torch.isnan(big[:, 32 + f:]).all()
    gbuf = torch.full((d + 2 * pad, f + 64), nan, device="cuda")
    grad = pool._backward_weighted_raw(_cuda(g), off, d, wsum, perm=perm, weights=wdev, out=gbuf[pad:pad + d, 32:32 + f])
    assert not torch.isnan(grad).any()                            # every row written through the permutation ...
    ref.check_d_embeds(grad.cpu().numpy(), g, index, mixed_w, n)  # ... with its own value: once
    assert torch.isnan(gbuf[:pad]).all() and torch.isnan(gbuf[pad + d:]).all()
    assert torch.isnan(gbuf[:, :32]).all() and torch.isnan(gbuf[:, 32 + f:]).all()
    dw = pool._weight_grad_raw(view, _cuda(g), out, off, wsum, perm=perm)
    ref.check_d_weights(dw.cpu().numpy(), mixed_e, g, index, mixed_w, n)


def test_no_host_synchronisation_without_check():
    from mtmc_mpn import pool_tracklets
    name, f = "skew", 100
    lengths = _lengths(name)
    e, g, w = _inputs(name, f, "gaussian")
    n = len(lengths)
    index, place = ref.interleave(lengths, seed=9)
    mixed_e, mixed_w = np.empty_like(e), np.empty_like(w)
    mixed_e[place], mixed_w[place] = e, w
    e_dev, w_dev, i_dev, g_dev = _cuda(mixed_e), _cuda(mixed_w), _cuda(index), _cuda(g)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device="cuda")
    want = [pool_tracklets(e_dev, index=i_dev, num_tracklets=n), pool_tracklets(e_dev, offsets=off, weights=w_dev),
            pool_tracklets(e_dev, index=i_dev, num_tracklets=n, weights=w_dev)]
    leaf, wleaf = e_dev.clone().requires_grad_(), w_dev.clone().requires_grad_()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:                                                          # a host read would raise here
        got = [pool_tracklets(e_dev, index=i_dev, num_tracklets=n, check=False),
               pool_tracklets(e_dev, offsets=off, weights=w_dev, check=False),
               pool_tracklets(e_dev, index=i_dev, num_tracklets=n, weights=w_dev, check=False)]
        pool_tracklets(leaf, index=i_dev, num_tracklets=n, weights=wleaf, check=False).backward(g_dev)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    ref.check_d_weights(wleaf.grad.cpu().numpy(), mixed_e, g, index, mixed_w, n)


def test_captured_with_offsets_and_weights():
    from mtmc_mpn import pool
    r = _r()
    first, second, f = (r + 5, 2, 3 * r, 1), (1, 2 * r + 1, r + 4, r + 2), 260
    assert sum(first) == sum(second)
    d = sum(first)
    cases = [(pool_ref.gaussian_embeds(d, f, 80 + k), ref.uniform_weights(d, 82 + k), lengths)
             for k, lengths in enumerate((first, second))]

    def offsets(lengths):
        return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device="cuda")
    e_dev, w_dev, off_dev = _cuda(cases[0][0]), _cuda(cases[0][1]), offsets(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool.pool_tracklets(e_dev, offsets=off_dev, weights=w_dev, check=False)  # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = pool.pool_tracklets(e_dev, offsets=off_dev, weights=w_dev, check=False)
    for e, w, lengths in cases:
        e_dev.copy_(_cuda(e))
        w_dev.copy_(_cuda(w))
        off_dev.copy_(offsets(lengths))
        graph.replay()
        torch.cuda.synchronize()
        ref.check_forward(out.cpu().numpy(), e, ref.seg_of_lengths(lengths), w, len(lengths))


@pytest.mark.parametrize("f", [100, 2048])
def test_repeatable(f):
    name = "skew" if f == 100 else "edges"
    lengths = _lengths(name)
    e, g, w = _inputs(name, f, "gaussian")
    index, place = ref.interleave(lengths, seed=10)
    mixed_e, mixed_w = np.empty_like(e), np.empty_like(w)
    mixed_e[place], mixed_w[place] = e, w
    a, b = (_run(mixed_e, g, mixed_w, index=index, n=len(lengths)) for _ in range(2))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("needs", ["embeds", "weights", "both"])
def test_autograd(needs):
    from mtmc_mpn import pool_tracklets
    r = _r()
    lengths, f = (2, r + 1, 1, 3 * r, 4, r), 320
    seg, n = ref.seg_of_lengths(lengths), len(lengths)
    d = seg.size
    e, g, w = pool_ref.gaussian_embeds(d, f, 91), pool_ref.gaussian_embeds(n, f, 92), ref.uniform_weights(d, 93)
    leaf = _cuda(e).requires_grad_(needs != "weights")
    wleaf = _cuda(w).requires_grad_(needs != "embeds")
    out = pool_tracklets(leaf, list(lengths), weights=wleaf)
    assert out.requires_grad and type(out.grad_fn).__name__ == "_PoolWeightedBackward"
    saved = [t for t in out.grad_fn.saved_tensors if t is not None]
    big = [t for t in saved if t.dim() == 2]
    if needs == "embeds":                                         # offsets, weights, weight sums: no [D, F], no [N, F]
        assert not big and sorted(t.numel() for t in saved) == sorted([n + 1, d, n])
    else:
        assert sorted(tuple(t.shape) for t in big) == sorted([(d, f), (n, f)])
    out.backward(_cuda(g))
    ref.check_forward(out.detach().cpu().numpy(), e, seg, w, n)
    if needs != "weights":
        ref.check_d_embeds(leaf.grad.cpu().numpy(), g, seg, w, n)
    else:
        assert leaf.grad is None
    if needs != "embeds":
        ref.check_d_weights(wleaf.grad.cpu().numpy(), e, g, seg, w, n)
    else:
        assert wleaf.grad is None
    with torch.no_grad():
        assert not pool_tracklets(leaf, list(lengths), weights=wleaf).requires_grad
    assert not pool_tracklets(leaf.detach(), list(lengths), weights=wleaf.detach()).requires_grad


def test_autograd_chain_with_build_graph():
    import mtmc_mpn
    r = _r()
    n, f = 12, 64
    lengths = tuple(int(v) for v in np.linspace(1, r + 3, n).round())
    cams = np.arange(n) % 3
    labels = np.arange(n) // 3
    d = sum(lengths)
    e, w = pool_ref.gaussian_embeds(d, f, 95), ref.uniform_weights(d, 96) + np.float32(0.25)
    index, place = ref.interleave(lengths, seed=11)
    mixed_e, mixed_w = np.empty_like(e), np.empty_like(w)
    mixed_e[place], mixed_w[place] = e, w
    i_dev = _cuda(index)

    def loss(g):
        wx = torch.randn(g.x.shape, generator=torch.Generator().manual_seed(22)).cuda()
        wa = torch.randn(g.edge_attr.shape, generator=torch.Generator().manual_seed(23)).cuda()
        return (g.x * wx).sum() + (g.edge_attr * wa).sum()

    leaf, wleaf = _cuda(mixed_e).requires_grad_(), _cuda(mixed_w).requires_grad_()
    loss(mtmc_mpn.build_graph(mtmc_mpn.pool_tracklets(leaf, index=i_dev, num_tracklets=n, weights=wleaf), cams, labels)).backward()
    pooled = mtmc_mpn.pool_tracklets(leaf.detach(), index=i_dev, num_tracklets=n, weights=wleaf.detach()).requires_grad_()
    loss(mtmc_mpn.build_graph(pooled, cams, labels)).backward()
    gp = pooled.grad.cpu().numpy()
    ref.check_d_embeds(leaf.grad.cpu().numpy(), gp, index, mixed_w, n)
    ref.check_d_weights(wleaf.grad.cpu().numpy(), mixed_e, gp, index, mixed_w, n)


def test_empty_and_argument_errors():
    from mtmc_mpn import pool_tracklets
    e = torch.zeros(0, 2048, device="cuda")
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    out = pool_tracklets(e, index=none, num_tracklets=3, weights=torch.zeros(0, device="cuda"))
    assert out.shape == (3, 2048) and (out == 0).all()
    assert pool_tracklets(e, index=none, num_tracklets=0).shape == (0, 2048)
    e = torch.ones(6, 8, device="cuda")
    idx = torch.zeros(6, dtype=torch.int64, device="cuda")
    for kw in ({"index": idx.int(), "num_tracklets": 2}, {"index": idx[:5], "num_tracklets": 2}, {"index": idx.cpu(), "num_tracklets": 2},
               {"index": idx, "num_tracklets": 2, "weights": torch.ones(6, device="cuda").double()},
               {"index": idx, "num_tracklets": 2, "weights": torch.ones(5, device="cuda")},
               {"index": idx, "num_tracklets": 2, "weights": torch.ones(6)}):
        with pytest.raises(RuntimeError):
            pool_tracklets(e, **kw)
    with pytest.raises(ValueError):
        pool_tracklets(e, index=idx, num_tracklets=torch.tensor(2, device="cuda"))
    assert torch.equal(pool_tracklets(e, index=idx, num_tracklets=2), torch.tensor([[1.0] * 8, [0.0] * 8], device="cuda"))
