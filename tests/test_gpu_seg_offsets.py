"""Every kernel that walks chunks by device offsets (csrc/seg_walk.h), on offsets that are NOT a clean grouping: the plain
and the weighted pooling forward, both backwards, the weight gradient, and mtmc_scatter_grouped through the raw ABI.
All data are small integers (pool_ref.integer_embeds, pool_weighted_ref.integer_weights), so every sum is exact and every
comparison is ==.  Shapes: three chunks with a partial last one (D = 75 at 32 rows, E = 150 at 64), F / C with one partial
slab and with two slabs.  The host model below is a port of seg_walk's rule; on sorted offsets it is checked here against
the declarative rule (the one range that holds a position) before it is used.  On the decreasing and the out-of-range
offsets there is no independent truth: what the tests pin there is that every kernel agrees with that one rule (and so
with each other), that every row is written, and that nothing next to the outputs is touched."""
import numpy as np
import pytest
import torch

import pool_ref
import pool_weighted_ref as wref

pytestmark = pytest.mark.gpu

N = 5
OFFSETS = {"sorted": [4, 4, 40, 40, 70, 70],            # non-decreasing, free ends, empty ranges
           "decreasing": [0, 50, 20, 60, 10, 75],
           "outside": [-3, 10, 90, 40, 75, 200]}
POISON = -7.0


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _clamped(offsets, d):
    return [min(max(int(v), 0), d) for v in offsets]


def owners(offsets, d, chunk):
    """owner [d] (-1: nobody) by the rule of seg_walk, chunk by chunk."""
    off, n = _clamped(offsets, d), len(offsets) - 1
    own = np.full(d, -1, dtype=np.int64)
    for r0 in range(0, d, chunk):
        r1, lo_s, hi_s = min(r0 + chunk, d), 0, n - 1
        while lo_s < hi_s:
            mid = lo_s + (hi_s - lo_s + 1) // 2
            lo_s, hi_s = (mid, hi_s) if off[mid] <= r0 else (lo_s, mid - 1)
        cur = r0
        for s in range(lo_s, n):
            a, b = off[s], off[s + 1]
            if cur >= r1:
                break
            if b <= a or b <= cur:
                continue
            lo, hi = (min(a, r1) if a > cur else cur), min(b, r1)
            cur = lo
            if lo >= r1:
                break
            own[lo:hi] = s
            cur = hi
            if b > r1:
                break
    return own


def declared_owners(offsets, d):
    own = np.full(d, -1, dtype=np.int64)
    for s in range(len(offsets) - 1):
        own[max(offsets[s], 0):max(min(offsets[s + 1], d), 0)] = s
    return own


@pytest.mark.parametrize("chunk", [32, 64])
def test_model_is_the_declarative_rule_on_sorted_offsets(chunk):
    d = 75 if chunk == 32 else 150
    assert np.array_equal(owners(OFFSETS["sorted"], d, chunk), declared_owners(OFFSETS["sorted"], d))
    assert np.array_equal(owners([0, 10, 40, 41, 70, d], d, chunk), declared_owners([0, 10, 40, 41, 70, d], d))


def _plain_info(offsets, d):
    bad, ends = [], []
    for s in range(N):
        ra, rb = offsets[s], offsets[s + 1]
        bad.append(ra >= rb or ra < 0 or rb > d)
        ends.append((s == 0 and ra != 0) or (s == N - 1 and rb != d))
    return [2 if any(ends) else int(any(bad)), sum(x or y for x, y in zip(bad, ends))]


def _weighted_info(offsets, d):                           # with a permutation: empty ranges are legal, the last end is free
    bits, count = 0, 0
    for s in range(N):
        ra, rb = offsets[s], offsets[s + 1]
        st = (1 if (ra > rb or ra < 0 or rb > d) else 0) | (2 if (s == 0 and ra != 0) else 0)
        bits |= st
        count += st != 0
    return [bits, count]


def _around(buf, lo, hi):
    """the rows in front of buf[lo:hi] and behind it still hold the poison"""
    return bool((buf[:lo] == POISON).all() and (buf[hi:] == POISON).all())


@pytest.mark.parametrize("f", [8, 260])
@pytest.mark.parametrize("kind", list(OFFSETS))
def test_plain_pooling(kind, f):
    from mtmc_mpn import _lib, pool
    d, offsets = 75, OFFSETS[kind]
    off = _clamped(offsets, d)
    e, g = pool_ref.integer_embeds(d, f, seed=3), pool_ref.integer_embeds(N, f, seed=4)
    own = owners(offsets, d, pool.CHUNK_ROWS)
    out_buf = torch.full((N + 2, f), POISON, device="cuda")
    info = torch.full((_lib.POOL_INFO,), -1, dtype=torch.int32, device="cuda")
    out = pool._forward_raw(_cuda(e), _cuda(np.array(offsets, dtype=np.int64)), out=out_buf[1:N + 1], info=info).cpu().numpy()
    assert _around(out_buf, 1, N + 1)
    assert info.cpu().tolist() == _plain_info(offsets, d) + [0, 0]
    for s in range(N):
        a, b = off[s], off[s + 1]
        if b <= a:
            assert not out[s].any()
        elif kind == "sorted":
            assert np.array_equal(out[s], e[a:b].sum(0, dtype=np.float32) / np.float32(b - a))
        # else: not asserted.  With offsets that decrease, a chunk may never write the partial slot that the finish kernel
        # adds for a crossing range, and the workspace is uninitialised memory
    pad = 3
    gbuf = torch.full((d + 2 * pad, f + 64), POISON, device="cuda")
    grad = pool._backward_raw(_cuda(g), _cuda(np.array(offsets, dtype=np.int64)), d, out=gbuf[pad:pad + d, 32:32 + f]).cpu().numpy()
    want = np.zeros((d, f), dtype=np.float32)
    for j in range(d):
        if own[j] >= 0:
            want[j] = g[own[j]] / np.float32(off[own[j] + 1] - off[own[j]])
    assert np.array_equal(grad, want)                      # every row written, by its owner or as a gap
    assert _around(gbuf, pad, pad + d) and bool((gbuf[:, :32] == POISON).all() and (gbuf[:, 32 + f:] == POISON).all())


@pytest.mark.parametrize("f", [8, 260])
@pytest.mark.parametrize("kind", list(OFFSETS))
def test_weighted_pooling(kind, f):
    from mtmc_mpn import _lib, pool
    d, offsets = 75, OFFSETS[kind]
    off = _clamped(offsets, d)
    e, g = pool_ref.integer_embeds(d, f, seed=5), pool_ref.integer_embeds(N, f, seed=6)
    w = wref.integer_weights(d, seed=7)
    assert (w == 0).any() and (w > 0).any()
    perm = np.random.default_rng(8).permutation(d).astype(np.int64)
    own = owners(offsets, d, pool.CHUNK_ROWS)
    off_dev, perm_dev, w_dev = _cuda(np.array(offsets, dtype=np.int64)), _cuda(perm), _cuda(w)
    # W_s over the positions [a, b) of each range, in float32 (small integers: exact in any order)
    wsum_model = np.array([w[perm[off[s]:off[s + 1]]].sum(dtype=np.float32) if off[s + 1] > off[s] else 0.0 for s in range(N)],
                          dtype=np.float32)
    out_buf = torch.full((N + 2, f), POISON, device="cuda")
    sum_buf = torch.full((N + 2,), POISON, device="cuda")
    info = torch.full((_lib.POOL_INFO,), -1, dtype=torch.int32, device="cuda")
    out, wsum = pool._forward_weighted_raw(_cuda(e), off_dev, perm=perm_dev, weights=w_dev, out=out_buf[1:N + 1], info=info,
                                           wsum=sum_buf[1:N + 1])
    out, wsum, got_info = out.cpu().numpy(), wsum.cpu().numpy(), info.cpu().tolist()
    assert _around(out_buf, 1, N + 1) and _around(sum_buf, 1, N + 1)
    assert got_info[:2] == _weighted_info(offsets, d)
    for s in range(N):
        a, b = off[s], off[s + 1]
        if b <= a:
            assert not out[s].any() and wsum[s] == 0
        elif kind == "sorted":
            rows = perm[a:b]
            acc = (e[rows] * w[rows, None]).sum(0, dtype=np.float32)
            assert wsum[s] == wsum_model[s]
            assert np.array_equal(out[s], acc / wsum_model[s] if wsum_model[s] > 0 else np.zeros(f, dtype=np.float32))
        # else: rows of crossing ranges are not asserted, for the reason given in test_plain_pooling
    # info[3]: the positions behind offsets[N] (every perm entry names a row here).  info[2], the tracklets that got a zero
    # row: exact on sorted offsets; otherwise the weight sum of a crossing range is as unasserted as its row, and what is
    # certain is the ranges with b <= a
    assert got_info[3] == d - off[N]
    if kind == "sorted":
        assert got_info[2] == int((wsum_model <= 0).sum())
    else:
        assert sum(off[s + 1] <= off[s] for s in range(N)) <= got_info[2] <= N
    # the backwards take the weight sums as an argument: the model's, so that they do not depend on unasserted rows
    pad = 3
    gbuf = torch.full((d + 2 * pad, f + 64), POISON, device="cuda")
    grad = pool._backward_weighted_raw(_cuda(g), off_dev, d, _cuda(wsum_model), perm=perm_dev, weights=w_dev,
                                       out=gbuf[pad:pad + d, 32:32 + f]).cpu().numpy()
    want = np.zeros((d, f), dtype=np.float32)
    for j in range(d):
        s = own[j]
        if s >= 0 and wsum_model[s] > 0:
            want[perm[j]] = (g[s] / wsum_model[s]) * w[perm[j]]
    assert np.array_equal(grad, want)                      # every row written through the permutation
    assert _around(gbuf, pad, pad + d) and bool((gbuf[:, :32] == POISON).all() and (gbuf[:, 32 + f:] == POISON).all())
    # the weight gradient is g[s] . (x - pooled[s]) / W_s with `pooled` an argument: an integer-valued one keeps every
    # product and sum an integer below 2^24 (64 * 128 * 260), so the dot product is exact in the kernel's order too
    # (its kernel walks four positions a wave, not a 32-row chunk: on offsets that decrease, the owner of a position depends
    # on where the walk begins, so the model walks its chunks too)
    own = owners(offsets, d, 4)
    pooled = pool_ref.integer_embeds(N, f, seed=9)
    dw = pool._weight_grad_raw(_cuda(e), _cuda(g), _cuda(pooled), off_dev, _cuda(wsum_model), perm=perm_dev).cpu().numpy()
    want_w = np.zeros(d, dtype=np.float32)
    for j in range(d):
        s = own[j]
        if s >= 0 and wsum_model[s] > 0:
            dot = (g[s].astype(np.float64) * (e[perm[j]].astype(np.float64) - pooled[s])).sum()
            want_w[perm[j]] = np.float32(dot) / wsum_model[s]
    assert np.array_equal(dw, want_w)


@pytest.mark.parametrize("mode", [0, 2], ids=["add", "max"])
@pytest.mark.parametrize("c", [4, 33])
@pytest.mark.parametrize("kind", list(OFFSETS))
def test_grouped_scatter(kind, c, mode):
    from mtmc_mpn import _call, _lib
    e_rows = 150
    offsets = [2 * v for v in OFFSETS[kind]]              # the same three families over 150 positions in chunks of 64
    off = _clamped(offsets, e_rows)
    src = pool_ref.integer_embeds(e_rows, c, seed=10)
    perm = np.random.default_rng(11).permutation(e_rows).astype(np.int64)
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    out_buf = torch.full((N + 2, c), POISON, device=dev)
    arg_buf = torch.full((N + 2, c), int(POISON), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.mtmc_scatter_grouped_workspace_bytes(e_rows, c), dtype=torch.uint8, device=dev)
    src_dev, perm_dev, off_dev = _cuda(src), _cuda(perm), _cuda(np.array(offsets, dtype=np.int64))
    _call.run(dev, lib.mtmc_scatter_grouped, src_dev.data_ptr(), e_rows, c, perm_dev.data_ptr(), off_dev.data_ptr(), N, mode,
              out_buf[1:N + 1].data_ptr(), arg_buf[1:N + 1].data_ptr() if mode == 2 else None, ws.data_ptr(), ws.numel(),
              _call.stream(dev))
    out, arg = out_buf[1:N + 1].cpu().numpy(), arg_buf[1:N + 1].cpu().numpy()
    assert _around(out_buf, 1, N + 1)
    assert _around(arg_buf, 1, N + 1) and (mode == 2 or bool((arg_buf == int(POISON)).all()))
    for s in range(N):
        a, b = off[s], off[s + 1]
        if b <= a:
            assert not out[s].any() and (mode != 2 or (arg[s] == e_rows).all())
        elif kind == "sorted":
            rows = perm[a:b]
            if mode == 0:
                assert np.array_equal(out[s], src[rows].sum(0, dtype=np.float32))
            else:
                assert np.array_equal(out[s], src[rows].max(0))
                first = [min(r for r in rows if src[r, k] == out[s, k]) for k in range(c)]
                assert np.array_equal(arg[s], first)
        # else: rows of crossing groups are not asserted, for the reason given in test_plain_pooling
