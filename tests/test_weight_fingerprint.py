"""The weight-plane cache's fingerprint (csrc/split_body.h) must see every structured edit of a chunk's weights, not only
single-word ones: a chunk whose fingerprint survives an edit keeps its old planes, and the forward runs with the OLD
weights without any error.  Round 5's linear hash gave positions with equal (2i+1)(2t+1) one multiplier: swapping two such
words, or +d at one and -d at the other, went unseen.

CPU only.  The fingerprint is tests/wcache_util.py's mirror of the kernel (tests/test_gpu_weight_cache.py pins the mirror to
what the GPU stores); each edit is priced by the terms it changes, finalise(sum + delta), never by hashing the chunk again.
Chunks 0, a middle one and the last of seeded randn weights of every node-encoder layer of the shipped model."""
import numpy as np
import pytest

import wcache_util as wu

U64 = np.uint64
SHAPES = [(2048, 1024), (1024, 512), (512, 128), (128, 32)]        # (K, O) of node-encoder layers 0..3
IDS = [f"K{K}xO{O}" for K, O in SHAPES]


class Chunk:
    def __init__(self, K, O, chunk, seed):
        W = np.random.default_rng(seed).standard_normal((O, K)).astype(np.float32)
        self.K, self.chunk, self.W = K, chunk, W
        self.bits, live = wu.chunk_bits(W, chunk)
        assert live == wu.CHUNK_ROWS
        self.U = wu.pair_values(self.bits)
        self.T = wu.slot_terms(self.bits)
        self.S = U64(int(self.T.sum(dtype=U64)))
        self.fp = wu.finalise(self.S)
        assert int(self.fp) == wu.fingerprint(W, chunk)

    def word(self, r, k):
        return self.bits[r, k]

    def after(self, ra, ka, wa, rb=None, kb=None, wb=None):
        """Fingerprints after writing the 32-bit patterns wa at (ra, ka) and (if given) wb at (rb, kb), vectorised."""
        pa, ha = wu.slot_of(ra, ka)
        ua = _put(self.U[pa], ha, wa)
        with np.errstate(over="ignore"):
            if rb is None:
                return wu.finalise(self.S + (wu.term(pa, ua) - self.T[pa]))
            pb, hb = wu.slot_of(rb, kb)
            same = pa == pb
            ua = np.where(same, _put(ua, hb, wb), ua)                     # both words in one pair: one term changes
            ub = _put(self.U[pb], hb, wb)
            delta = wu.term(pa, ua) - self.T[pa] + np.where(same, U64(0), wu.term(pb, ub) - self.T[pb])
            return wu.finalise(self.S + delta)


def _put(u, half, w):
    u, w = np.asarray(u, dtype=U64), np.asarray(w).astype(U64)
    return np.where(np.asarray(half) == 0, (u & U64(0xFFFFFFFF00000000)) | w, (u & U64(0xFFFFFFFF)) | (w << U64(32)))


def _chunks(K, O):
    n = O // wu.CHUNK_ROWS
    return [Chunk(K, O, c, seed=K * 7 + c) for c in sorted({0, n // 2, n - 1})]


_CACHE = {}


def chunks(K, O):
    if (K, O) not in _CACHE:
        _CACHE[(K, O)] = _chunks(K, O)
    return _CACHE[(K, O)]


def _assert_all_seen(c, fps, what, ra=None, ka=None, rb=None, kb=None):
    bad = np.flatnonzero(fps == c.fp)
    assert bad.size == 0, (f"chunk {c.chunk} (K={c.K}): {bad.size} of {fps.size} {what} leave the fingerprint "
                           f"{int(c.fp):#018x}; first: " + (f"({ra[bad[0]]},{ka[bad[0]]})" if ra is not None else "") +
                           (f" <-> ({rb[bad[0]]},{kb[bad[0]]})" if rb is not None else ""))


def _pairs(c, rng, n_random):
    """Position pairs for the +-d / sign / pruning classes: every pair of positions that shared a multiplier under round 5's
    hash, and n_random seeded random pairs of distinct positions."""
    K = c.K
    r, k = np.divmod(np.arange(wu.CHUNK_ROWS * K), K)
    key = wu.legacy_multiplier_key(r, k)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    a, b = [], []
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], ks.size]
    for s, e in zip(starts, ends):
        if e - s > 1:
            g = order[s:e]
            ia, ib = np.triu_indices(e - s, 1)
            a.append(g[ia])
            b.append(g[ib])
    shared = (np.concatenate(a), np.concatenate(b)) if a else (np.zeros(0, int), np.zeros(0, int))
    ra_, rb_ = rng.integers(0, wu.CHUNK_ROWS * K, (2, n_random))
    keep = ra_ != rb_
    pa = np.concatenate([shared[0], ra_[keep]])
    pb = np.concatenate([shared[1], rb_[keep]])
    return (r[pa], k[pa], r[pb], k[pb]), shared[0].size


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_every_single_bit_flip_is_seen(K, O):
    """Control: every hash that is a bijection of each word passes this."""
    for c in chunks(K, O):
        r, k = np.divmod(np.arange(wu.CHUNK_ROWS * K), K)
        for bit in range(32):
            fps = c.after(r, k, c.bits[r, k] ^ np.uint32(1 << bit))
            _assert_all_seen(c, fps, f"flips of bit {bit}", r, k)


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_every_swap_within_a_row_is_seen(K, O):
    """Every swap of two unequal words of rows 0, 1 and 7 of a chunk (round 5: W[r][1] <-> W[r][8] of row 0 went unseen)."""
    ia, ib = np.triu_indices(K, 1)
    for c in chunks(K, O):
        for row in (0, 1, 7):
            wa, wb = c.bits[row, ia], c.bits[row, ib]
            sel = wa != wb
            ka, kb = ia[sel], ib[sel]
            r = np.full(ka.size, row)
            fps = c.after(r, ka, wb[sel], r, kb, wa[sel])
            _assert_all_seen(c, fps, f"swaps inside row {row}", r, ka, r, kb)


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_every_column_swap_between_rows_is_seen(K, O):
    """Every swap of two unequal words in one column across two rows of a chunk, for all 28 row pairs."""
    k = np.arange(K)
    for c in chunks(K, O):
        for r1, r2 in zip(*np.triu_indices(wu.CHUNK_ROWS, 1)):
            wa, wb = c.bits[r1, k], c.bits[r2, k]
            sel = wa != wb
            ra, rb = np.full(sel.sum(), r1), np.full(sel.sum(), r2)
            fps = c.after(ra, k[sel], wb[sel], rb, k[sel], wa[sel])
            _assert_all_seen(c, fps, f"column swaps between rows {r1} and {r2}", ra, k[sel], rb, k[sel])


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_every_row_swap_is_seen(K, O):
    for c in chunks(K, O):
        for r1, r2 in zip(*np.triu_indices(wu.CHUNK_ROWS, 1)):
            bits = c.bits.copy()
            bits[[r1, r2]] = bits[[r2, r1]]
            assert wu.finalise(wu.chunk_sum(bits)) != c.fp, f"chunk {c.chunk}: swapping rows {r1} and {r2} went unseen"


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_plus_d_minus_d_is_seen(K, O):
    """+d on the 32-bit pattern of one word and -d on another's: every pair that shared a multiplier in round 5, and 10^5
    random pairs."""
    rng = np.random.default_rng(K + 1)
    for c in chunks(K, O):
        (ra, ka, rb, kb), n_shared = _pairs(c, rng, 100_000)
        assert n_shared > 0
        for d in (1, 0x1000, 0x7FFFFF, int(rng.integers(1, 1 << 32))):
            wa = (c.bits[ra, ka].astype(np.uint64) + d) & 0xFFFFFFFF
            wb = (c.bits[rb, kb].astype(np.uint64) - d) & 0xFFFFFFFF
            fps = c.after(ra, ka, wa, rb, kb, wb)
            _assert_all_seen(c, fps, f"+{d:#x}/-{d:#x} pairs", ra, ka, rb, kb)


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_two_sign_flips_or_two_zeroed_words_are_seen(K, O):
    """Sign flips and pruning (zeroing) of two words at once, for the position pairs of the +-d class."""
    rng = np.random.default_rng(K + 2)
    for c in chunks(K, O):
        (ra, ka, rb, kb), _ = _pairs(c, rng, 100_000)
        wa, wb = c.bits[ra, ka], c.bits[rb, kb]
        sign = np.uint32(0x80000000)
        _assert_all_seen(c, c.after(ra, ka, wa ^ sign, rb, kb, wb ^ sign), "double sign flips", ra, ka, rb, kb)
        sel = (wa != 0) | (wb != 0)
        zero = np.zeros(sel.sum(), dtype=np.uint32)
        _assert_all_seen(c, c.after(ra[sel], ka[sel], zero, rb[sel], kb[sel], zero), "double prunings",
                         ra[sel], ka[sel], rb[sel], kb[sel])


@pytest.mark.parametrize("K,O", SHAPES, ids=IDS)
def test_advisor_swap_of_row_entries_1_and_8(K, O):
    """The regression the round-5 review found: in the first row of a chunk, column 1 is word slot 1 of thread 0 and column 8
    is word slot 0 of thread 1 -- one multiplier (3 G D) in round 5, so swapping W[r][1] and W[r][8] kept the fingerprint."""
    assert wu.legacy_multiplier_key(0, 1) == wu.legacy_multiplier_key(0, 8)
    W = np.random.default_rng(11).standard_normal((O, K)).astype(np.float32)
    for chunk in (0, O // 8 - 1):
        r = chunk * 8
        W[r, 1], W[r, 8] = 2.0, -2.0
        before = wu.fingerprint(W, chunk)
        W[r, [1, 8]] = W[r, [8, 1]]
        after = wu.fingerprint(W, chunk)
        print(f"K={K} chunk {chunk}: fingerprint {before:#018x} before the swap, {after:#018x} after")
        assert before != after


def test_mirror_index_map_and_dead_rows():
    """Every word of a chunk has exactly one (pair position, half); words at k >= K and rows >= O are what the kernel makes of
    them (zeros / nothing)."""
    p, h = wu.slot_of(wu.PAIR_ROW, wu.PAIR_K)
    assert (p == np.arange(wu.SLOTS)[:, None]).all() and (h == np.arange(2)[None, :]).all()
    assert len(set(zip(wu.PAIR_ROW.ravel().tolist(), wu.PAIR_K.ravel().tolist()))) == wu.CHUNK_ROWS * 2048
    assert (wu.PAIR_K[:, 1] == wu.PAIR_K[:, 0] + 1).all() and (wu.PAIR_K[:, 0] % 2 == 0).all()
    W = np.random.default_rng(5).standard_normal((13, 96)).astype(np.float32)      # last chunk: 5 live rows
    bits, live = wu.chunk_bits(W, 1)
    assert live == 5 and not bits[:, 96:].any() and not bits[5:].any()
    t = wu.slot_terms(bits, live)
    assert not t[wu.ROW_OF_SLOT >= 5].any() and t[wu.ROW_OF_SLOT < 5].all()
    W2 = W.copy()
    W2[:8] = 0.0                                                          # chunk 0 changes, chunk 1 does not
    assert wu.fingerprint(W2, 1) == wu.fingerprint(W, 1) and wu.fingerprint(W2, 0) != wu.fingerprint(W, 0)
    assert all(f & 1 for f in wu.fingerprints(W).view(np.uint64).tolist())
