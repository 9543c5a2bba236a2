"""CPU tests of the weighted-pool yardstick (tests/pool_weighted_ref.py): its three results against torch float64 autograd
of the (w[:, None] * x) segment sums, tracklets with zero total weight and empty ones included; the stable grouping; the
fp32 emulation of the kernels' order of operations against the derived bounds; and the new exports.  No GPU."""
import numpy as np
import pytest
import torch

import pool_ref
import pool_weighted_ref as ref


def _case(seed=0):
    lengths = [3, 1, 7, 2, 5, 4]
    n = len(lengths) + 2                                         # tracklets 6 and 7 are named by no row
    seg = ref.seg_of_lengths(lengths)
    d, f = seg.size, 12
    e = pool_ref.gaussian_embeds(d, f, seed + 1)
    g = pool_ref.gaussian_embeds(n, f, seed + 2)
    w = ref.uniform_weights(d, seed + 3)
    w[seg == 2] = 0.0                                            # a tracklet whose weights add up to 0
    w[seg == 1] = 0.5
    return e, g, w, seg, n


def _torch_pool(e, w, seg, n):
    s = torch.from_numpy(seg)
    num = torch.zeros((n, e.shape[1]), dtype=torch.float64).index_add(0, s, w[:, None] * e)
    den = torch.zeros(n, dtype=torch.float64).index_add(0, s, w)
    safe = torch.where(den > 0, den, torch.ones_like(den))
    return torch.where(den[:, None] > 0, num / safe[:, None], torch.zeros_like(num))


@pytest.mark.parametrize("order", ["grouped", "interleaved"])
def test_yardstick_against_torch_autograd(order):
    e, g, w, seg, n = _case()
    if order == "interleaved":
        shuffle = np.random.default_rng(9).permutation(seg.size)
        e, w, seg = e[shuffle], w[shuffle], seg[shuffle]
    assert (ref.weight_sums(seg, w, n) == 0).sum() == 3 and (ref.rows_per_tracklet(seg, n) == 0).sum() == 2
    te = torch.from_numpy(e).double().requires_grad_()
    tw = torch.from_numpy(w).double().requires_grad_()
    out = _torch_pool(te, tw, seg, n)
    out.backward(torch.from_numpy(g).double())
    assert np.allclose(ref.weighted_ref(e, seg, w, n), out.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert np.allclose(ref.d_embeds_ref(g, seg, w, n), te.grad.numpy(), rtol=1e-13, atol=1e-15)
    assert np.allclose(ref.d_weights_ref(e, g, seg, w, n), tw.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert np.all(ref.weighted_ref(e, seg, w, n)[[2, 6, 7]] == 0) and np.all(ref.d_embeds_ref(g, seg, w, n)[seg == 2] == 0)
    # all weights 1: the plain yardstick
    if order == "grouped":
        lengths = np.bincount(seg)
        assert np.allclose(ref.weighted_ref(e, seg, np.ones_like(w), lengths.size), pool_ref.pool_ref(e, lengths), rtol=1e-14)


def test_stable_grouping_reproduces_the_grouped_layout():
    lengths = [4, 1, 6, 3]
    e = pool_ref.integer_embeds(sum(lengths), 8, seed=5)
    index, place = ref.interleave(lengths, seed=6)
    assert sorted(index.tolist()) == ref.seg_of_lengths(lengths).tolist() and not np.array_equal(index, np.sort(index))
    mixed = np.empty_like(e)
    mixed[place] = e
    perm, offsets = ref.stable_group(index, len(lengths))
    assert offsets.tolist() == [0, 4, 5, 11, 14] and np.array_equal(perm, place)
    assert np.array_equal(mixed[perm], e)
    for s in range(len(lengths)):                                # increasing row order inside every tracklet
        assert np.all(np.diff(perm[offsets[s]:offsets[s + 1]]) > 0)
    # ids outside [0, n) sort behind offsets[n]; an id nobody names is an empty range
    perm, offsets = ref.stable_group(np.array([2, -1, 0, 5, 2, 2 ** 40, 0]), 4)
    assert offsets.tolist() == [0, 2, 2, 4, 4] and perm.tolist() == [2, 6, 0, 4, 1, 3, 5]


def _emulate(e, g, w, seg, n, chunk=32):
    """The kernels' order of operations in numpy float32: fused multiply-adds in row order inside chunks of `chunk` rows
    (an fma is emulated in float64 and rounded once), partial sums added in chunk order, one division."""
    f32 = np.float32
    out, total = np.zeros((n, e.shape[1]), f32), np.zeros(n, f32)
    for s in range(n):
        rows = np.flatnonzero(seg == s)
        acc, wacc, first = None, None, True
        for c in np.unique(rows // chunk):
            part, wpart = np.zeros(e.shape[1], f32), f32(0)
            for r in rows[rows // chunk == c]:
                part = (np.float64(w[r]) * e[r].astype(np.float64) + part.astype(np.float64)).astype(f32)
                wpart = f32(wpart + w[r])
            acc, wacc = (part, wpart) if first else ((acc + part).astype(f32), f32(wacc + wpart))
            first = False
        if not first and wacc > 0:
            out[s], total[s] = acc / wacc, wacc
    safe = np.where(total > 0, total, f32(1))
    d_e = np.where((total[seg] > 0)[:, None], w[:, None] * (g[seg] / safe[seg][:, None]).astype(f32), f32(0)).astype(f32)
    dots = np.zeros(seg.size, f32)
    for c in range(e.shape[1]):                                  # a column-by-column fp32 dot product
        dots = (dots + g[seg][:, c] * (e[:, c] - out[seg][:, c]).astype(f32)).astype(f32)
    d_w = np.where(total[seg] > 0, dots / safe[seg], f32(0)).astype(f32)
    return out, d_e, d_w


@pytest.mark.parametrize("weights", ["uniform", "integer"])
def test_fp32_emulation_stays_inside_the_bounds(weights):
    lengths = [1, 31, 33, 70, 2, 64]
    seg = ref.seg_of_lengths(lengths)
    n, d, f = len(lengths), seg.size, 24
    e, g = pool_ref.gaussian_embeds(d, f, 11), pool_ref.gaussian_embeds(n, f, 12)
    w = ref.uniform_weights(d, 13) if weights == "uniform" else ref.integer_weights(d, 13)
    out, d_e, d_w = _emulate(e, g, w, seg, n)
    worst = (ref.check_forward(out, e, seg, w, n), ref.check_d_embeds(d_e, g, seg, w, n, integer_weights=weights == "integer"),
             ref.check_d_weights(d_w, e, g, seg, w, n))
    assert max(worst) <= 1.0, worst                              # (the checks assert it element by element)


def test_integer_sums_are_exact():
    lengths = [5, 40, 3]
    seg = ref.seg_of_lengths(lengths)
    e, w = pool_ref.integer_embeds(seg.size, 16, 21), ref.integer_weights(seg.size, 22)
    out, _, _ = _emulate(e, np.zeros((3, 16), np.float32), w, seg, 3)
    ref.check_forward(out, e, seg, w, 3, exact_integers=True)


def test_exports_and_sizing():
    from mtmc_mpn import _lib, pool
    lib = _lib.load()
    for name in ("mtmc_pool_tracklets_weighted_workspace_bytes", "mtmc_pool_tracklets_weighted",
                 "mtmc_pool_tracklets_weighted_backward", "mtmc_pool_tracklets_weight_grad"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    r = pool.CHUNK_ROWS
    for d, f in ((1, 4), (r, 256), (r + 1, 260), (37844, 2048)):
        chunks = -(-d // r)
        plain, need = lib.mtmc_pool_tracklets_workspace_bytes(d, f), lib.mtmc_pool_tracklets_weighted_workspace_bytes(d, f)
        assert need >= 2 * chunks * f * 4 + 2 * chunks * 4 and need % 256 == 0 and need - plain <= 3 * chunks * 4 + 512
    for d, f in ((-1, 4), (8, 6), (8, 0), (2 ** 31, 4), (8, 16388)):
        assert lib.mtmc_pool_tracklets_weighted_workspace_bytes(d, f) == 0
    # refused on the host, before any HIP call, with the entry point's name in the text
    assert lib.mtmc_pool_tracklets_weighted(None, 4, -1, 4, None, 1, None, None, None, None, None, None, 0, None) == _lib.E_ARG
    assert lib.mtmc_mpn_last_error().startswith(b"pool_tracklets_weighted: ")
    assert lib.mtmc_pool_tracklets_weighted_backward(None, 8, 6, None, 1, None, None, None, None, 8, None) == _lib.E_ARG
    assert lib.mtmc_mpn_last_error().startswith(b"pool_tracklets_weighted_backward: ")
    assert lib.mtmc_pool_tracklets_weight_grad(None, 4, 8, 4, None, -1, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.mtmc_mpn_last_error().startswith(b"pool_tracklets_weight_grad: ")
    assert lib.mtmc_pool_tracklets_weighted(None, 2048, 0, 2048, None, 0, None, None, None, None, None, None, 0, None) == 0


def test_argument_errors_on_the_host():
    from mtmc_mpn import pool_tracklets
    e = torch.zeros(6, 8)
    idx = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError):
        pool_tracklets(e, [6], index=idx, num_tracklets=1)
    with pytest.raises(ValueError):
        pool_tracklets(e, index=idx)                             # num_tracklets is required with index
    with pytest.raises(ValueError):
        pool_tracklets(e, [6], num_tracklets=1)
    with pytest.raises(RuntimeError):
        pool_tracklets(e, index=idx, num_tracklets=1)            # no CPU path
