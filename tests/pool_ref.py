"""The yardstick of `pool_tracklets`: per-tracklet mean and its backward in numpy float64, and the two input families.

integer_embeds: values from +-{1..64} stored as float32.  Any order of fp32 additions over fewer than 2^18 such rows is
exact (every partial sum is an integer below 2^24), so the only rounding left in a mean is the scale by 1 / len.
"""
import numpy as np

U = 2.0 ** -24           # unit round-off of fp32


def pool_ref(embeds, lengths):
    e = np.asarray(embeds, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64)
    out = np.zeros((lengths.size, e.shape[1]), dtype=np.float64)
    at = 0
    for s, n in enumerate(lengths):
        out[s] = e[at:at + n].sum(axis=0) / float(n)
        at += n
    return out


def pool_backward_ref(g, lengths):
    g = np.asarray(g, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.repeat(g / lengths[:, None].astype(np.float64), lengths, axis=0)


def integer_embeds(d, f, seed):
    rng = np.random.default_rng(seed)
    mag = rng.integers(1, 65, size=(d, f))
    sign = rng.integers(0, 2, size=(d, f)) * 2 - 1
    return (mag * sign).astype(np.float32)


def gaussian_embeds(d, f, seed):
    return np.random.default_rng(seed).standard_normal((d, f)).astype(np.float32)


def column_sums(embeds, lengths):
    """Exact int64 column sums per tracklet (integer inputs)."""
    e = np.asarray(embeds).astype(np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return np.add.reduceat(e, starts, axis=0) if lengths.size else np.zeros((0, e.shape[1]), np.int64)


def mean_abs(embeds, lengths):
    """mean_i |x_i| per tracklet and column, float64 (the gaussian bound's scale)."""
    return pool_ref(np.abs(np.asarray(embeds, dtype=np.float64)), lengths)


def check_forward(got, embeds, lengths, family):
    """The issue's bounds.  integer: |got - S/len| <= 3u |S/len|, exactly 0 where S = 0;
    gaussian: |got - ref64| <= (len + 4) u mean_i|x_i| per element."""
    got = np.asarray(got, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64)
    if family == "integer":
        want = column_sums(embeds, lengths).astype(np.float64) / lengths[:, None]
        err, bound = np.abs(got - want), 3 * U * np.abs(want)
    else:
        want = pool_ref(embeds, lengths)
        err, bound = np.abs(got - want), (lengths[:, None] + 4) * U * mean_abs(embeds, lengths)
    bad = err > bound
    assert not bad.any(), (f"{family}: {int(bad.sum())} elements past the bound, worst err {err[bad].max():.3e} "
                           f"against {bound[bad][np.argmax(err[bad])]:.3e}")


def check_backward(got, g, lengths):
    """|got - g/len| <= 3u |g/len|; bit-equal to g/len in fp32 where len is a power of two."""
    got = np.asarray(got)
    lengths = np.asarray(lengths, dtype=np.int64)
    want = pool_backward_ref(g, lengths)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 3 * U * np.abs(want)).all(), f"backward: worst err {err.max():.3e}"
    pow2 = np.repeat((lengths & (lengths - 1)) == 0, lengths)
    assert np.array_equal(got[pow2], want[pow2].astype(np.float32))
