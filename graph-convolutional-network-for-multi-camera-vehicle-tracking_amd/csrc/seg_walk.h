// Segmented reductions over row ranges: the one decomposition behind pool_tracklets.hip and the grouped scatter of
// scatter_ops.hip.  offsets [N + 1] cut the D positions into N ranges; the positions are cut into chunks of
// R rows, one wave per (chunk, column slab); a chunk finds its first range by binary search and walks the ranges that
// meet it (SegCursor, seg_walk).  A range inside one chunk is finished there; one that crosses chunks leaves a partial per
// chunk in partial[chunk][2][cols] -- slot "tail" in its first chunk, slot "head" in the others -- and a finish kernel, one
// wave per (range, slab), folds tail, head, head, ... in chunk order.
// The offsets live in device memory and the host never sees them: every value is clamped into [0, D] before it is compared
// or indexes anything, offsets is read at [0, N] alone, and whatever it holds a walk tiles its chunk with non-empty pieces
// in ascending order.  The walking part has no HIP in it: tests/abi/seg_walk_check.cpp checks exactly that on the host.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MTMC_SEG_FN __host__ __device__ __forceinline__
#else
#define MTMC_SEG_FN inline
#endif

namespace mtmc {

MTMC_SEG_FN int64_t seg_clamp(int64_t v, int64_t D) { return v < 0 ? 0 : (v > D ? D : v); }

// the largest s in [0, N-1] with offsets[s] <= r (s = 0 if there is none); any contents of offsets end the search
template <class Offsets>
MTMC_SEG_FN int64_t seg_find(Offsets offsets, int64_t N, int64_t D, int64_t r) {
  int64_t lo = 0, hi = N - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (seg_clamp(offsets[mid], D) <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The walk over positions [r0, r1), as a cursor: next() moves to the next piece -- the part [lo, hi) of range s = [a, b)
// (clamped ends) -- in ascending order and says whether there is one.  A range that is empty, inverted (b <= a) or wholly
// behind the walk owns nothing: with offsets that decrease somewhere the walk never moves backwards, and a position belongs
// to the first range, in index order from seg_find(r0), that reaches it.  Positions between the pieces belong to no range.
template <class Offsets> struct SegCursor {
  Offsets offsets;
  int64_t N, D, r1, cur, next_s;
  int64_t s, a, b, lo, hi;
  MTMC_SEG_FN SegCursor(Offsets o, int64_t n, int64_t d, int64_t r0, int64_t r1_)
      : offsets(o), N(n), D(d), r1(r1_), cur(r0), next_s(seg_find(o, n, d, r0)), s(0), a(0), b(0), lo(r0), hi(r0) {}
  MTMC_SEG_FN bool next() {
    for (; next_s < N && cur < r1; ++next_s) {
      a = seg_clamp(offsets[next_s], D), b = seg_clamp(offsets[next_s + 1], D);
      if (b <= a || b <= cur) continue;                    // empty, inverted or behind us
      lo = a > cur ? (a < r1 ? a : r1) : cur, hi = b < r1 ? b : r1;
      if (lo >= r1) break;
      s = next_s, cur = hi;
      next_s = b > r1 ? N : next_s + 1;                    // a range that goes on behind r1 is the chunk's last
      return true;
    }
    return false;
  }
};
// The same with callbacks: piece(s, a, b, lo, hi) and, for positions of no range, gap(lo, hi); they tile [r0, r1) in order.
template <class Offsets, class Piece, class Gap>
MTMC_SEG_FN void seg_walk(Offsets offsets, int64_t N, int64_t D, int64_t r0, int64_t r1, Piece&& piece, Gap&& gap) {
  int64_t at = r0;
  for (SegCursor<Offsets> w(offsets, N, D, r0, r1); w.next(); at = w.hi) {
    if (at < w.lo) gap(at, w.lo);
    piece(w.s, w.a, w.b, w.lo, w.hi);
  }
  if (at < r1) gap(at, r1);
}
struct SegNoGap { MTMC_SEG_FN void operator()(int64_t, int64_t) const {} };   // of a forward: nothing to do between ranges

// chunk c of D positions cut by R: [c R, min(c R + R, D))
MTMC_SEG_FN int64_t seg_chunks(int64_t D, int R) { return (D + R - 1) / R; }
MTMC_SEG_FN int64_t seg_chunk_end(int64_t r0, int R, int64_t D) { return r0 + R < D ? r0 + R : D; }

// Chunk side: the range [a, b) met in chunk [r0, r1) is finished there, or else leaves its partial in this slot of
// partial[chunk][2].  Finish side: a non-empty range spans chunks seg_first_chunk .. seg_last_chunk; it was finished in its
// chunk iff the two are equal (the same condition), else its sum is tail(first), head(first + 1), ..., head(last).
MTMC_SEG_FN bool seg_inside(int64_t a, int64_t b, int64_t r0, int64_t r1) { return a >= r0 && b <= r1; }
MTMC_SEG_FN int64_t seg_head(int64_t c) { return c * 2; }
MTMC_SEG_FN int64_t seg_tail(int64_t c) { return c * 2 + 1; }
MTMC_SEG_FN int64_t seg_slot(int64_t c, int64_t a, int64_t r0) { return a < r0 ? seg_head(c) : seg_tail(c); }
MTMC_SEG_FN int64_t seg_first_chunk(int64_t a, int R) { return a / R; }
MTMC_SEG_FN int64_t seg_last_chunk(int64_t b, int R) { return (b - 1) / R; }

// host side: the bytes of a [chunks][2][cols] float plane, and the grid of items * slabs waves at four per workgroup
inline size_t seg_plane_bytes(int64_t D, int R, int64_t cols) { return (size_t)seg_chunks(D, R) * 2 * (size_t)cols * sizeof(float); }
inline unsigned seg_grid(int64_t items, int64_t slabs) {   // kernels.h's blocks_for(items * slabs, 4, INT_MAX), without kernels.h
  const int64_t b = (items * slabs + 3) / 4;
  return (unsigned)(b < 1 ? 1 : (b > INT_MAX ? INT_MAX : b));
}

#ifdef __HIPCC__
// which (item, slab) this wave works on (neighbouring slabs of one item first); the lane's part in the slab is the kernel's own
__device__ __forceinline__ void seg_wave(int slabs, int64_t* item, int* slab) {
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  *item = w / slabs;
  *slab = (int)(w - *item * slabs);
}
#endif

}  // namespace mtmc
