"""The yardstick of `pool_tracklets(index=, weights=)`: weighted per-tracklet mean, its two backwards and the stable grouping
in numpy float64, the weight families, and the bound checks of the GPU tests.

A tracklet assignment is `seg` [D]: the tracklet of each detection row, any value outside [0, n) for a detection of no
tracklet.  Rows count in increasing row order.  u = 2^-24; `len` is the number of rows of a tracklet, zero-weight ones
included (they take part in the fp32 sums as exact zeros, so the count is an upper bound of the roundings).

  forward    |got - ref64| <= (2 len + 4) u A,  A = sum_i w_i |x_i| / sum_i w_i per column: numerator and denominator are
             each a sum of `len` terms in some order ((len - 1) u each, the numerator's products fused: no rounding of
             their own, one more u for an fp32 weight sum that is not exact), one division
  d_embeds   |got - want| <= (len + 3) u |want|: the fp32 weight sum ((len - 1) u), a division and a product; with integer
             weights the sum is exact: 3u
  d_weights  |got - want| <= (F + 3 len + 8) u B_r,  B_r = sum_c |g_sc| (|x_rc| + A_sc) / W_s: a dot product of F terms in
             some order against sum |terms|, each term with the error of the fp32 out[s] ((2 len + 4) u A, in B through
             A) and of the subtraction, then the division by the fp32 W_s ((len - 1) u)
  integers   embeds from +-{1..64} and weights from {0, 1, 2, 3}: every partial sum is an integer below 2^24, so
             |got - S/W| <= 3u |S/W| and exactly 0 where S = 0
"""
import numpy as np

import pool_ref

U = pool_ref.U


def seg_of_lengths(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)


def stable_group(index, n):
    """(perm [D], offsets [n + 1]): the rows tracklet by tracklet, each tracklet's in increasing row order; rows whose index
    is outside [0, n) behind offsets[n]."""
    index = np.asarray(index, dtype=np.int64)
    key = np.where((index >= 0) & (index < n), index, n)
    perm = np.argsort(key, kind="stable")
    offsets = np.searchsorted(key[perm], np.arange(n + 1), side="left")
    return perm.astype(np.int64), offsets.astype(np.int64)


def interleave(lengths, seed):
    """A frame-ordered arrangement of a grouped layout: (index [D], place [D]) with row place[r] of the interleaved matrix
    holding grouped row r; each tracklet keeps its internal order."""
    index = np.random.default_rng(seed).permutation(seg_of_lengths(lengths))
    place, _ = stable_group(index, len(lengths))
    return index, place


def _owned(seg, n):
    seg = np.asarray(seg, dtype=np.int64)
    ok = (seg >= 0) & (seg < n)
    return np.where(ok, seg, 0), ok


def integer_weights(d, seed):
    return np.random.default_rng(seed).integers(0, 4, size=d).astype(np.float32)


def uniform_weights(d, seed):
    rng = np.random.default_rng(seed)
    w = (1.0 - rng.random(d)).astype(np.float32)                 # (0, 1]
    w[rng.random(d) < 0.3] = 0.0
    return w


def weight_sums(seg, w, n):
    s, ok = _owned(seg, n)
    return np.bincount(s[ok], weights=np.asarray(w, dtype=np.float64)[ok], minlength=n)


def rows_per_tracklet(seg, n):
    s, ok = _owned(seg, n)
    return np.bincount(s[ok], minlength=n)


def _segment_sum(rows, seg, n):
    s, ok = _owned(seg, n)
    out = np.zeros((n, rows.shape[1]), dtype=np.float64)
    np.add.at(out, s[ok], rows[ok])
    return out


def weighted_ref(embeds, seg, w, n):
    """out [n, F] float64: sum w x / sum w; a zero row where the weights add up to 0 (or no row names the tracklet)."""
    e, w = np.asarray(embeds, dtype=np.float64), np.asarray(w, dtype=np.float64)
    total = weight_sums(seg, w, n)
    num = _segment_sum(w[:, None] * e, seg, n)
    return np.divide(num, total[:, None], out=np.zeros_like(num), where=total[:, None] > 0)


def mean_abs(embeds, seg, w, n):
    """A = sum w |x| / sum w per tracklet and column."""
    return weighted_ref(np.abs(np.asarray(embeds, dtype=np.float64)), seg, w, n)


def d_embeds_ref(g, seg, w, n):
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    total = weight_sums(seg, w, n)
    s, ok = _owned(seg, n)
    scale = np.where(ok & (total[s] > 0), w / np.where(total[s] > 0, total[s], 1.0), 0.0)
    return scale[:, None] * g[s]


def d_weights_ref(embeds, g, seg, w, n):
    e, g = np.asarray(embeds, dtype=np.float64), np.asarray(g, dtype=np.float64)
    total = weight_sums(seg, w, n)
    out = weighted_ref(e, seg, w, n)
    s, ok = _owned(seg, n)
    dot = np.einsum("rc,rc->r", g[s], e - out[s])
    return np.where(ok & (total[s] > 0), dot / np.where(total[s] > 0, total[s], 1.0), 0.0)


def check_forward(got, embeds, seg, w, n, exact_integers=False):
    got = np.asarray(got, dtype=np.float64)
    want = weighted_ref(embeds, seg, w, n)
    err = np.abs(got - want)
    if exact_integers:
        bound = 3 * U * np.abs(want)
    else:
        bound = (2 * rows_per_tracklet(seg, n)[:, None] + 4) * U * mean_abs(embeds, seg, w, n)
    bad = err > bound
    assert not bad.any(), (f"forward: {int(bad.sum())} elements past the bound, worst err {err[bad].max():.3e} against "
                           f"{bound[bad][np.argmax(err[bad])]:.3e}")
    assert np.all(got[weight_sums(seg, w, n) == 0] == 0)
    return float((err / np.where(bound > 0, bound, np.inf)).max())


def check_d_embeds(got, g, seg, w, n, integer_weights=False):
    got = np.asarray(got, dtype=np.float64)
    want = d_embeds_ref(g, seg, w, n)
    s, _ = _owned(seg, n)
    factor = 3 if integer_weights else rows_per_tracklet(seg, n)[s][:, None] + 3
    err, bound = np.abs(got - want), factor * U * np.abs(want)
    bad = err > bound
    assert not bad.any(), f"d_embeds: {int(bad.sum())} elements past the bound, worst err {err[bad].max():.3e}"
    return float((err / np.where(bound > 0, bound, np.inf)).max())


def check_d_weights(got, embeds, g, seg, w, n):
    got = np.asarray(got, dtype=np.float64)
    want = d_weights_ref(embeds, g, seg, w, n)
    total = weight_sums(seg, w, n)
    s, ok = _owned(seg, n)
    live = ok & (total[s] > 0)
    a = mean_abs(embeds, seg, w, n)
    f = np.asarray(embeds).shape[1]
    spread = np.einsum("rc,rc->r", np.abs(np.asarray(g, dtype=np.float64))[s], np.abs(np.asarray(embeds, dtype=np.float64)) + a[s])
    b = np.where(live, spread / np.where(live, total[s], 1.0), 0.0)
    err, bound = np.abs(got - want), (f + 3 * rows_per_tracklet(seg, n)[s] + 8) * U * b
    bad = err > bound
    assert not bad.any(), (f"d_weights: {int(bad.sum())} rows past the bound, worst err {err[bad].max():.3e} against "
                           f"{bound[bad][np.argmax(err[bad])]:.3e}")
    assert np.all(got[~live] == 0)
    return float((err / np.where(bound > 0, bound, np.inf)).max())
