// From detections to node features: the mean of the ReID embeddings of each tracklet's detections (reference
// train.py:305-316: one torch.mean(bboxes_embeds, 0) per tracklet, then torch.stack; libs/reid_feature_extraction.py:177-178
// the same once per tracklet), forward and backward.
//   mtmc_pool_tracklets           out[s] = mean of rows [offsets[s], offsets[s+1]) of embeds [D][F]
//   mtmc_pool_tracklets_backward  d_embeds[r] = g[s(r)] / len_s
//   mtmc_pool_tracklets_weighted (+ _backward, mtmc_pool_tracklets_weight_grad)  the same through a row permutation and
//                                 with per-detection weights: out[s] = sum w_r x_r / sum w_r (further down)
// A pure streaming problem (F = 2048: 8 KB per row, tracklets of 1 to a few thousand rows); what there is to get right is the
// load balance and the order of the additions.  The decomposition is seg_walk.h's with chunks of kPoolR
// rows and slabs of 256 columns: one float4 per lane, so every row read is 1 KiB coalesced and no wave ever walks more
// than kPoolR rows.  The finish kernels also write the zero row of an empty range and check the offsets.  No atomics on
// floats anywhere: every sum has one fixed order.  What was wrong with the offsets is reported in info[0] (0 ok; 1 not strictly
// increasing or outside [0, D]; 2 offsets[0] != 0 or offsets[N] != D -- the larger one if both), info[1] = tracklets with a bad range.
#include "api_internal.h"
#include "seg_walk.h"
#include <limits.h>

namespace mtmc {

constexpr int kPoolR = 32;            // rows per chunk
constexpr int kPoolSlab = 256;        // columns per wave
constexpr int kPoolMaxF = 16384;
typedef float pool_f4 __attribute__((ext_vector_type(4)));

// the item (chunk or tracklet) and the four columns of this lane; false: nothing to do
__device__ __forceinline__ bool pool_wave(int64_t items, int slabs, int F, int64_t* item, int* col) {
  int slab;
  seg_wave(slabs, item, &slab);
  *col = slab * kPoolSlab + (int)(threadIdx.x & 63) * 4;
  return *item < items && *col < F;
}

// sum of rows [lo, hi) of one lane's four columns, in row order; 8 (then 4) independent 16-byte loads before the adds
__device__ __forceinline__ pool_f4 pool_sum_rows(const float* base, int64_t stride, int64_t lo, int64_t hi) {
  pool_f4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* p = base + lo * stride;
  int64_t n = hi - lo;
  for (; n >= 8; n -= 8, p += 8 * stride) {
    pool_f4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const pool_f4*>(p + j * stride);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += v[j];
  }
  if (n >= 4) {
    pool_f4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const pool_f4*>(p + j * stride);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += v[j];
    n -= 4; p += 4 * stride;
  }
  for (; n > 0; --n, p += stride) acc += *reinterpret_cast<const pool_f4*>(p);
  return acc;
}

__global__ __launch_bounds__(256) void pool_chunks_kernel(const float* embeds, int64_t stride, int64_t D, int F,
                                                          const int64_t* offsets, int64_t N, float* out, float* partial,
                                                          int* info) {
  // the status words start at 0 for pool_finish_kernel, the next launch on the stream (instead of a memset node of its own)
  if (info && blockIdx.x == 0 && threadIdx.x == 0) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
  const int slabs = (F + kPoolSlab - 1) / kPoolSlab;
  int64_t c;
  int col;
  if (!pool_wave(seg_chunks(D, kPoolR), slabs, F, &c, &col)) return;
  const int64_t r0 = c * kPoolR, r1 = seg_chunk_end(r0, kPoolR, D);
  seg_walk(offsets, N, D, r0, r1, [&](int64_t s, int64_t a, int64_t b, int64_t lo, int64_t hi) {
    const pool_f4 acc = pool_sum_rows(embeds + col, stride, lo, hi);
    if (seg_inside(a, b, r0, r1)) {
      *reinterpret_cast<pool_f4*>(out + s * F + col) = acc / (float)(b - a);
    } else {
      *reinterpret_cast<pool_f4*>(partial + seg_slot(c, a, r0) * F + col) = acc;
    }
  }, SegNoGap());
}

__global__ __launch_bounds__(256) void pool_finish_kernel(int64_t D, int F, const int64_t* offsets, int64_t N, float* out,
                                                          const float* partial, int* info) {
  const int slabs = (F + kPoolSlab - 1) / kPoolSlab;
  int64_t s;
  int col;
  if (!pool_wave(N, slabs, F, &s, &col)) return;
  const int64_t ra = offsets[s], rb = offsets[s + 1];
  if (info && col == 0) {                                  // one lane per tracklet
    const int st1 = (ra >= rb || ra < 0 || rb > D) ? 1 : 0;
    const int st2 = ((s == 0 && ra != 0) || (s == N - 1 && rb != D)) ? 2 : 0;
    if (st1 | st2) {
      atomicMax(info, st2 ? st2 : st1);
      atomicAdd(info + 1, 1);
    }
  }
  const int64_t a = seg_clamp(ra, D), b = seg_clamp(rb, D);
  pool_f4* dst = reinterpret_cast<pool_f4*>(out + s * F + col);
  if (b <= a) {
    *dst = pool_f4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const int64_t c0 = seg_first_chunk(a, kPoolR), c1 = seg_last_chunk(b, kPoolR);
  if (c0 == c1) return;                                    // finished inside its chunk
  // the tail of chunk c0, then the heads of chunks c0 + 1 .. c1: rows of stride 2 F starting at the first head
  const pool_f4 tail = *reinterpret_cast<const pool_f4*>(partial + seg_tail(c0) * F + col);
  const pool_f4 heads = pool_sum_rows(partial + col, 2 * (int64_t)F, c0 + 1, c1 + 1);
  *dst = (tail + heads) / (float)(b - a);
}

// Same chunks as the forward.  A wave keeps g[s] / len_s of the tracklet it is in, streams it over that tracklet's rows of
// the chunk and reloads at the next tracklet: each of the D rows is written once (rows no tracklet owns -- bad offsets
// only -- get zeros).
__global__ __launch_bounds__(256) void pool_backward_kernel(const float* g, int64_t D, int F, const int64_t* offsets, int64_t N,
                                                            float* d_embeds, int64_t stride) {
  const int slabs = (F + kPoolSlab - 1) / kPoolSlab;
  int64_t c;
  int col;
  if (!pool_wave(seg_chunks(D, kPoolR), slabs, F, &c, &col)) return;
  const int64_t r0 = c * kPoolR, r1 = seg_chunk_end(r0, kPoolR, D);
  float* dst = d_embeds + col;
  seg_walk(offsets, N, D, r0, r1, [&](int64_t s, int64_t a, int64_t b, int64_t lo, int64_t hi) {
    const pool_f4 v = *reinterpret_cast<const pool_f4*>(g + s * F + col) / (float)(b - a);
    // (non-temporal: D F 4 bytes nobody in this launch reads again; measured 84 -> 55 us on 310 MB against plain stores)
    for (int64_t r = lo; r < hi; ++r) __builtin_nontemporal_store(v, reinterpret_cast<pool_f4*>(dst + r * stride));
  }, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) *reinterpret_cast<pool_f4*>(dst + r * stride) = pool_f4{0.f, 0.f, 0.f, 0.f};
  });
}

// ---- detections in any order (perm) and per-detection weights: out[s] = sum_r w_r x_r / sum_r w_r ----
// The same chunks, slabs, head / tail partial sums and chunk order as above, over the POSITIONS j of a row permutation:
// position j holds detection row perm[j] (perm == NULL: j itself) with weight weights[perm[j]] (weights == NULL: 1).
// Lane l of a wave fetches row and weight of position r0 + l once; the row loop broadcasts them with v_readlane, so the
// gather costs one 8-byte and one 4-byte load per row and wave beside the 1 KiB of the row.  A perm entry outside [0, D)
// and a weight that is negative or not finite count as weight 0 and never become an address or a factor; they are reported
// in info (each chunk leaves a word in cflag[chunk], which one wave of pool_finish_wp_kernel folds).  The weight sums take the same route as the row sums: wsum[s] for a tracklet inside its chunk, wpart[chunk][2]
// for heads and tails, added in chunk order by pool_finish_wp_kernel.  fmaf(1, x, acc) = acc + x, so with every weight 1
// the result has the bits of the plain kernels.
constexpr int kPoolBadOffsets = 1, kPoolBadEnds = 2, kPoolBadPerm = 4, kPoolBadWeight = 8;   // bits of info[0]

struct PoolRowRef { int row; float w; };      // of one position, held by the lane of that position

// as pool_wave, but lanes past F stay: they work on column 0 and store nothing
__device__ __forceinline__ bool pool_wave_all(int64_t items, int slabs, int F, int64_t* item, int* col, bool* live) {
  int slab;
  seg_wave(slabs, item, &slab);
  const int c = slab * kPoolSlab + (int)(threadIdx.x & 63) * 4;
  *live = c < F;
  *col = *live ? c : 0;
  return *item < items;
}

template <bool kPerm, bool kWeighted>
__device__ __forceinline__ PoolRowRef pool_row_ref(const int64_t* perm, const float* weights, int64_t D, int64_t r0, int64_t r1,
                                                   int* flags) {
  const int64_t j = r0 + (int)(threadIdx.x & 63);
  PoolRowRef ref = {0, 0.f};
  if (j < r1) {
    const int64_t p = kPerm ? perm[j] : j;
    if (p >= 0 && p < D) {
      ref.row = (int)p;                                   // D < 2^31
      ref.w = kWeighted ? weights[p] : 1.f;
      if (!(ref.w >= 0.f && ref.w <= __FLT_MAX__)) { ref.w = 0.f; *flags |= kPoolBadWeight; }
    } else {
      *flags |= kPoolBadPerm;
    }
  }
  return ref;
}

__device__ __forceinline__ pool_f4 pool_fma(float w, pool_f4 x, pool_f4 acc) {
  if (w == 0.f) return acc;                               // (wave-uniform) a masked row counts for nothing, whatever it holds
  return pool_f4{fmaf(w, x.x, acc.x), fmaf(w, x.y, acc.y), fmaf(w, x.z, acc.z), fmaf(w, x.w, acc.w)};
}

// kB positions from `at` (counted from the chunk's first row): kB independent 16-byte loads, then the fmas in row order
template <int kB>
__device__ __forceinline__ void pool_wrows_step(const float* base, int64_t stride, PoolRowRef ref, int at, pool_f4* acc, float* W) {
  pool_f4 v[kB];
  float w[kB];
#pragma unroll
  for (int k = 0; k < kB; ++k) {
    const int row = __builtin_amdgcn_readlane(ref.row, at + k);
    w[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ref.w), at + k));
    v[k] = *reinterpret_cast<const pool_f4*>(base + (int64_t)row * stride);
  }
#pragma unroll
  for (int k = 0; k < kB; ++k) {
    *acc = pool_fma(w[k], v[k], *acc);
    *W += w[k];
  }
}

template <bool kPerm, bool kWeighted>
__global__ __launch_bounds__(256) void pool_chunks_wp_kernel(const float* embeds, int64_t stride, int64_t D, int F,
                                                             const int64_t* offsets, int64_t N, const int64_t* perm,
                                                             const float* weights, float* out, float* wsum, float* partial,
                                                             float* wpart, int* cflag, int* info) {
  // the status words start at 0 for pool_finish_wp_kernel, the next launch on the stream (no memset node), as above
  if (info && blockIdx.x == 0 && threadIdx.x == 0) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
  const int slabs = (F + kPoolSlab - 1) / kPoolSlab;
  int64_t c;
  int col;
  bool live;
  if (!pool_wave_all(seg_chunks(D, kPoolR), slabs, F, &c, &col, &live)) return;
  const int64_t r0 = c * kPoolR, r1 = seg_chunk_end(r0, kPoolR, D);
  int flags = 0;
  const PoolRowRef ref = pool_row_ref<kPerm, kWeighted>(perm, weights, D, r0, r1, &flags);
  const bool first = col == 0 && live;                     // lane 0 of the chunk's first slab: the scalars are its to write
  {  // what was wrong with this chunk's positions: the offence bits, and from bit 8 up how many positions name no row
    const unsigned long long lost = __ballot(flags & kPoolBadPerm), badw = __ballot(flags & kPoolBadWeight);
    if (first) cflag[c] = (lost ? kPoolBadPerm : 0) | (badw ? kPoolBadWeight : 0) | ((int)__popcll(lost) << 8);
  }
  seg_walk(offsets, N, D, r0, r1, [&](int64_t s, int64_t a, int64_t b, int64_t lo, int64_t hi) {
    pool_f4 acc = {0.f, 0.f, 0.f, 0.f};
    float W = 0.f;
    int at = (int)(lo - r0);
    const int end = (int)(hi - r0);
    for (; at + 8 <= end; at += 8) pool_wrows_step<8>(embeds + col, stride, ref, at, &acc, &W);
    if (at + 4 <= end) { pool_wrows_step<4>(embeds + col, stride, ref, at, &acc, &W); at += 4; }
    for (; at < end; ++at) pool_wrows_step<1>(embeds + col, stride, ref, at, &acc, &W);
    if (seg_inside(a, b, r0, r1)) {
      const pool_f4 mean = W > 0.f ? acc / W : pool_f4{0.f, 0.f, 0.f, 0.f};
      if (live) *reinterpret_cast<pool_f4*>(out + s * F + col) = mean;
      if (first) wsum[s] = W;
    } else {
      const int64_t slot = seg_slot(c, a, r0);
      if (live) *reinterpret_cast<pool_f4*>(partial + slot * F + col) = acc;
      if (first) wpart[slot] = W;
    }
  }, SegNoGap());
}

// sum of wpart[2 c] for c in [lo, hi), in chunk order (every lane the same loads: one broadcast each)
__device__ __forceinline__ float pool_sum_heads(const float* wpart, int64_t lo, int64_t hi) {
  float acc = 0.f;
  int64_t c = lo;
  for (; c + 8 <= hi; c += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = wpart[2 * (c + k)];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  for (; c < hi; ++c) acc += wpart[2 * c];
  return acc;
}

// With a permutation the positions behind offsets[N] belong to no tracklet (info[3] counts them) and an empty tracklet
// is legal: a zero row.  info[2] counts the tracklets that got a zero row, empty ones and ones whose weights add up to 0.
template <bool kPerm>
__global__ __launch_bounds__(256) void pool_finish_wp_kernel(int64_t D, int F, const int64_t* offsets, int64_t N, float* out,
                                                             float* wsum, const float* partial, const float* wpart,
                                                             const int* cflag, int* info) {
  if (info && blockIdx.x == 0 && threadIdx.x < 64) {       // one wave folds the chunks' words into info
    int bits = 0, lost = 0;
    for (int64_t c = threadIdx.x; c < seg_chunks(D, kPoolR); c += 64) {
      const int v = cflag[c];
      bits |= v & 0xff;
      lost += v >> 8;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      bits |= __shfl_xor(bits, m, 64);
      lost += __shfl_xor(lost, m, 64);
    }
    if (threadIdx.x == 0 && bits) atomicOr(info, bits);
    if (threadIdx.x == 0 && lost) atomicAdd(info + 3, lost);
  }
  const int slabs = (F + kPoolSlab - 1) / kPoolSlab;
  int64_t s;
  int col;
  bool live;
  if (!pool_wave_all(N, slabs, F, &s, &col, &live)) return;
  const bool first = col == 0 && live;
  const int64_t ra = offsets[s], rb = offsets[s + 1];
  const int64_t a = seg_clamp(ra, D), b = seg_clamp(rb, D);
  if (info && first) {                                     // one lane per tracklet
    int st = ((kPerm ? ra > rb : ra >= rb) || ra < 0 || rb > D) ? kPoolBadOffsets : 0;
    if ((s == 0 && ra != 0) || (!kPerm && s == N - 1 && rb != D)) st |= kPoolBadEnds;
    if (st) {
      atomicOr(info, st);
      atomicAdd(info + 1, 1);
    }
    if (kPerm && s == N - 1 && b < D) atomicAdd(info + 3, (int)(D - b));
  }
  pool_f4* dst = reinterpret_cast<pool_f4*>(out + s * F + col);
  float W = 0.f;
  if (b <= a) {
    if (live) *dst = pool_f4{0.f, 0.f, 0.f, 0.f};
    if (first) wsum[s] = 0.f;
  } else {
    const int64_t c0 = seg_first_chunk(a, kPoolR), c1 = seg_last_chunk(b, kPoolR);
    if (c0 == c1) {                                        // finished inside its chunk
      W = wsum[s];
    } else {
      // the tail of chunk c0, then the heads of chunks c0 + 1 .. c1, rows and weight sums alike
      const pool_f4 tail = *reinterpret_cast<const pool_f4*>(partial + seg_tail(c0) * F + col);
      const pool_f4 heads = pool_sum_rows(partial + col, 2 * (int64_t)F, c0 + 1, c1 + 1);
      W = wpart[seg_tail(c0)] + pool_sum_heads(wpart, c0 + 1, c1 + 1);
      const pool_f4 mean = W > 0.f ? (tail + heads) / W : pool_f4{0.f, 0.f, 0.f, 0.f};
      if (live) *dst = mean;
      if (first) wsum[s] = W;
    }
  }
  if (info && first && !(W > 0.f)) atomicAdd(info + 2, 1);
}

// d_embeds[perm[j]] = w_j (g[s] / W_s) for every position j of tracklet s: the chunks of the forward, each position's row
// written once.  Positions no tracklet owns get a zero row, and so do the rows of a tracklet whose weights add up to 0;
// a position whose perm entry is outside [0, D) names no row and writes nothing.
template <bool kPerm, bool kWeighted>
__global__ __launch_bounds__(256) void pool_backward_wp_kernel(const float* g, int64_t D, int F, const int64_t* offsets, int64_t N,
                                                               const int64_t* perm, const float* weights, const float* wsum,
                                                               float* d_embeds, int64_t stride) {
  const int slabs = (F + kPoolSlab - 1) / kPoolSlab;
  int64_t c;
  int col;
  bool live;
  if (!pool_wave_all(seg_chunks(D, kPoolR), slabs, F, &c, &col, &live)) return;
  const int64_t r0 = c * kPoolR, r1 = seg_chunk_end(r0, kPoolR, D);
  int flags = 0;
  const PoolRowRef ref = pool_row_ref<kPerm, kWeighted>(perm, weights, D, r0, r1, &flags);
  const unsigned long long lost = __ballot(flags & kPoolBadPerm);
  float* dst = d_embeds + col;
  const pool_f4 zero = {0.f, 0.f, 0.f, 0.f};
  auto put = [&](int64_t pos, pool_f4 v) {
    const int at = (int)(pos - r0);
    if ((lost >> at) & 1) return;
    const int row = __builtin_amdgcn_readlane(ref.row, at);
    if (kWeighted) v = v * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ref.w), at));
    if (live) __builtin_nontemporal_store(v, reinterpret_cast<pool_f4*>(dst + (int64_t)row * stride));
  };
  seg_walk(offsets, N, D, r0, r1, [&](int64_t s, int64_t, int64_t, int64_t lo, int64_t hi) {
    const float W = wsum[s];
    const pool_f4 v = W > 0.f ? *reinterpret_cast<const pool_f4*>(g + s * F + col) / W : zero;
    for (int64_t r = lo; r < hi; ++r) put(r, v);
  }, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) put(r, zero);
  });
}

// d_w[perm[j]] = g[s] . (x[perm[j]] - out[s]) / W_s: one wave per kPoolGradRows positions, every load of the slab loop
// issued before the first fma; a lane adds its columns slab by slab, then the 64 lanes fold in a fixed butterfly, so the
// dot product has one order.  D F 4 bytes of embeds are read once; g[s] and out[s] (16 KiB a tracklet at F = 2048) come
// out of the caches.  A position of no tracklet or of a tracklet whose weights add up to 0 gets 0.
constexpr int kPoolGradRows = 4;

template <bool kPerm>
__global__ __launch_bounds__(256) void pool_weight_grad_kernel(const float* embeds, int64_t stride, int64_t D, int F,
                                                               const int64_t* offsets, int64_t N, const int64_t* perm,
                                                               const float* g, const float* out, const float* wsum, float* d_w) {
  const int64_t j0 = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * kPoolGradRows;
  if (j0 >= D) return;
  const int lane = (int)(threadIdx.x & 63);
  int64_t row[kPoolGradRows], seg[kPoolGradRows];         // -1: no such row / no tracklet
#pragma unroll
  for (int i = 0; i < kPoolGradRows; ++i) {
    const int64_t j = j0 + i;
    row[i] = seg[i] = -1;
    if (j < D) {
      const int64_t p = kPerm ? perm[j] : j;
      if (p >= 0 && p < D) row[i] = p;
    }
  }
  // each position's owner by the rule of the other kernels, walked over this wave's own positions (on offsets that decrease
  // it can differ from the 32-row chunks': it depends on where a walk begins).  Unrolled compares: seg[] stays in registers
  const int64_t j1 = j0 + kPoolGradRows < D ? j0 + kPoolGradRows : D;
  seg_walk(offsets, N, D, j0, j1, [&](int64_t s, int64_t, int64_t, int64_t lo, int64_t hi) {
#pragma unroll
    for (int i = 0; i < kPoolGradRows; ++i) {
      if (j0 + i >= lo && j0 + i < hi) seg[i] = s;
    }
  }, SegNoGap());
  float acc[kPoolGradRows];
  const float *px[kPoolGradRows], *pg[kPoolGradRows], *po[kPoolGradRows];
#pragma unroll
  for (int i = 0; i < kPoolGradRows; ++i) {               // rows that count for nothing read row 0 / tracklet 0
    acc[i] = 0.f;
    px[i] = embeds + (row[i] < 0 ? 0 : row[i]) * stride;
    pg[i] = g + (seg[i] < 0 ? 0 : seg[i]) * F;
    po[i] = out + (seg[i] < 0 ? 0 : seg[i]) * F;
  }
  for (int base = 0; base < F; base += kPoolSlab) {
    const int col = base + lane * 4;
    const bool live = col < F;
    const int cc = live ? col : 0;
    pool_f4 x[kPoolGradRows], gv[kPoolGradRows], ov[kPoolGradRows];
#pragma unroll
    for (int i = 0; i < kPoolGradRows; ++i) {
      x[i] = *reinterpret_cast<const pool_f4*>(px[i] + cc);
      gv[i] = *reinterpret_cast<const pool_f4*>(pg[i] + cc);
      ov[i] = *reinterpret_cast<const pool_f4*>(po[i] + cc);
    }
#pragma unroll
    for (int i = 0; i < kPoolGradRows; ++i) {
      if (!live) continue;
      const pool_f4 d = x[i] - ov[i];
      acc[i] = fmaf(gv[i].w, d.w, fmaf(gv[i].z, d.z, fmaf(gv[i].y, d.y, fmaf(gv[i].x, d.x, acc[i]))));
    }
  }
#pragma unroll
  for (int i = 0; i < kPoolGradRows; ++i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[i] += __shfl_xor(acc[i], m, 64);
    if (lane == 0 && row[i] >= 0) {
      const float W = seg[i] < 0 ? 0.f : wsum[seg[i]];
      d_w[row[i]] = W > 0.f ? acc[i] / W : 0.f;
    }
  }
}

// host side: sizes and launch grids
static inline bool pool_sizes_ok(int64_t n_rows, int32_t feat_dim) {
  return n_rows >= 0 && n_rows < (1ll << 31) && feat_dim >= 4 && feat_dim <= kPoolMaxF && feat_dim % 4 == 0;
}
static inline unsigned pool_grid(int64_t items, int32_t feat_dim) { return seg_grid(items, (feat_dim + kPoolSlab - 1) / kPoolSlab); }
// the weighted entry points' workspace: the partial rows, then wpart[chunks][2] and cflag[chunks]
static inline size_t pool_wpart_offset(int64_t n_rows, int32_t feat_dim) {
  return mtmc_api::align_up(seg_plane_bytes(n_rows, kPoolR, feat_dim));
}
static inline size_t pool_weighted_bytes(int64_t n_rows, int32_t feat_dim) {
  return pool_wpart_offset(n_rows, feat_dim) + (size_t)seg_chunks(n_rows, kPoolR) * 3 * sizeof(float);
}
// what every entry point checks first: MTMC_OK, or the refusal with its text
static inline int pool_args(const char* entry, int64_t n_rows, int32_t feat_dim, int64_t n_tracklets) {
  if (!pool_sizes_ok(n_rows, feat_dim))
    return mtmc_api::fail(MTMC_E_ARG, "%s: n_rows must be in [0, 2^31) and feat_dim a multiple of 4 in [4, %d]", entry, kPoolMaxF);
  if (n_tracklets < 0 || n_tracklets >= (1ll << 31)) return mtmc_api::fail(MTMC_E_ARG, "%s: n_tracklets must be in [0, 2^31)", entry);
  return MTMC_OK;
}
static inline bool pool_rows_ok(const float* rows, int64_t stride, int32_t feat_dim) {
  return rows && !((uintptr_t)rows & 15) && !(stride & 3) && stride >= feat_dim;
}
// one of the four instantiations of a kernel template <bool kPerm, bool kWeighted>
#define POOL_LAUNCH_WP(kernel, perm, weights, grid, stream, ...)                                                          \
  do {                                                                                                                     \
    if ((perm) && (weights)) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(256), 0, stream, __VA_ARGS__);            \
    else if (perm) hipLaunchKernelGGL((kernel<true, false>), grid, dim3(256), 0, stream, __VA_ARGS__);                     \
    else if (weights) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(256), 0, stream, __VA_ARGS__);                  \
    else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(256), 0, stream, __VA_ARGS__);                              \
  } while (0)

}  // namespace mtmc

extern "C" {

int32_t mtmc_pool_chunk_rows(void) { return mtmc::kPoolR; }

size_t mtmc_pool_tracklets_workspace_bytes(int64_t n_rows, int32_t feat_dim) {
  if (!mtmc::pool_sizes_ok(n_rows, feat_dim)) return 0;
  return mtmc_api::align_up(mtmc::seg_plane_bytes(n_rows, mtmc::kPoolR, feat_dim) + 1);
}

int32_t mtmc_pool_tracklets(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                            int64_t n_tracklets, float* out, int32_t* info, void* workspace, size_t workspace_bytes,
                            void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (const int rc = pool_args("pool_tracklets", n_rows, feat_dim, n_tracklets)) return rc;
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!embeds || !offsets || !out) return fail(MTMC_E_ARG, "pool_tracklets: NULL embeds, offsets or out");
  if (!pool_rows_ok(embeds, row_stride, feat_dim))
    return fail(MTMC_E_ARG, "pool_tracklets: embeds must be 16-byte aligned with a row stride that is a multiple of 4 and >= feat_dim");
  if (((uintptr_t)out & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)info & 3) || ((uintptr_t)workspace & 15))
    return fail(MTMC_E_ARG, "pool_tracklets: out and workspace must be 16-byte, offsets 8-byte and info 4-byte aligned");
  const size_t need = seg_plane_bytes(n_rows, kPoolR, feat_dim);
  if (!workspace || workspace_bytes < need)
    return fail(MTMC_E_ARG, "pool_tracklets: workspace has %zu bytes, %zu needed (mtmc_pool_tracklets_workspace_bytes)", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(pool_chunks_kernel, dim3(pool_grid(seg_chunks(n_rows, kPoolR), feat_dim)), dim3(256), 0, s, embeds, row_stride,
                     n_rows, (int)feat_dim, offsets, n_tracklets, out, partial, reinterpret_cast<int*>(info));
  hipLaunchKernelGGL(pool_finish_kernel, dim3(pool_grid(n_tracklets, feat_dim)), dim3(256), 0, s, n_rows, (int)feat_dim, offsets,
                     n_tracklets, out, (const float*)partial, reinterpret_cast<int*>(info));
  return mtmc_api::launched("pool_tracklets");
}

int32_t mtmc_pool_tracklets_backward(const float* grad_out, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                                     int64_t n_tracklets, float* grad_embeds, int64_t grad_row_stride, void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (const int rc = pool_args("pool_tracklets_backward", n_rows, feat_dim, n_tracklets)) return rc;
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!grad_out || !offsets || !grad_embeds) return fail(MTMC_E_ARG, "pool_tracklets_backward: NULL grad_out, offsets or grad_embeds");
  if (((uintptr_t)grad_out & 15) || ((uintptr_t)offsets & 7) || !pool_rows_ok(grad_embeds, grad_row_stride, feat_dim))
    return fail(MTMC_E_ARG, "pool_tracklets_backward: grad_out and grad_embeds must be 16-byte aligned, the row stride a multiple of 4 and >= feat_dim");
  hipLaunchKernelGGL(pool_backward_kernel, dim3(pool_grid(seg_chunks(n_rows, kPoolR), feat_dim)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), grad_out, n_rows, (int)feat_dim, offsets, n_tracklets, grad_embeds,
                     grad_row_stride);
  return mtmc_api::launched("pool_tracklets_backward");
}

size_t mtmc_pool_tracklets_weighted_workspace_bytes(int64_t n_rows, int32_t feat_dim) {
  if (!mtmc::pool_sizes_ok(n_rows, feat_dim)) return 0;
  return mtmc_api::align_up(mtmc::pool_weighted_bytes(n_rows, feat_dim) + 1);
}

int32_t mtmc_pool_tracklets_weighted(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim,
                                     const int64_t* offsets, int64_t n_tracklets, const int64_t* perm, const float* weights,
                                     float* out, float* wsum, int32_t* info, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (const int rc = pool_args("pool_tracklets_weighted", n_rows, feat_dim, n_tracklets)) return rc;
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!offsets || !out || !wsum) return fail(MTMC_E_ARG, "pool_tracklets_weighted: NULL offsets, out or wsum");
  if (!pool_rows_ok(embeds, row_stride, feat_dim))
    return fail(MTMC_E_ARG, "pool_tracklets_weighted: embeds must be 16-byte aligned with a row stride that is a multiple of 4 and >= feat_dim");
  if (((uintptr_t)out & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)perm & 7) || ((uintptr_t)weights & 3) ||
      ((uintptr_t)wsum & 3) || ((uintptr_t)info & 3) || ((uintptr_t)workspace & 15))
    return fail(MTMC_E_ARG, "pool_tracklets_weighted: out and workspace must be 16-byte, offsets and perm 8-byte, weights, wsum and info 4-byte aligned");
  const size_t need = pool_weighted_bytes(n_rows, feat_dim);
  if (!workspace || workspace_bytes < need)
    return fail(MTMC_E_ARG, "pool_tracklets_weighted: workspace has %zu bytes, %zu needed (mtmc_pool_tracklets_weighted_workspace_bytes)", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  float* wpart = reinterpret_cast<float*>(static_cast<char*>(workspace) + pool_wpart_offset(n_rows, feat_dim));
  int* cflag = reinterpret_cast<int*>(wpart + 2 * seg_chunks(n_rows, kPoolR));
  int* inf = reinterpret_cast<int*>(info);
  POOL_LAUNCH_WP(pool_chunks_wp_kernel, perm, weights, dim3(pool_grid(seg_chunks(n_rows, kPoolR), feat_dim)), s, embeds, row_stride, n_rows,
                 (int)feat_dim, offsets, n_tracklets, perm, weights, out, wsum, partial, wpart, cflag, inf);
  const dim3 grid(pool_grid(n_tracklets, feat_dim));
  if (perm)
    hipLaunchKernelGGL(pool_finish_wp_kernel<true>, grid, dim3(256), 0, s, n_rows, (int)feat_dim, offsets, n_tracklets, out, wsum,
                       (const float*)partial, (const float*)wpart, (const int*)cflag, inf);
  else
    hipLaunchKernelGGL(pool_finish_wp_kernel<false>, grid, dim3(256), 0, s, n_rows, (int)feat_dim, offsets, n_tracklets, out, wsum,
                       (const float*)partial, (const float*)wpart, (const int*)cflag, inf);
  return mtmc_api::launched("pool_tracklets_weighted");
}

int32_t mtmc_pool_tracklets_weighted_backward(const float* grad_out, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                                              int64_t n_tracklets, const int64_t* perm, const float* weights, const float* wsum,
                                              float* grad_embeds, int64_t grad_row_stride, void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (const int rc = pool_args("pool_tracklets_weighted_backward", n_rows, feat_dim, n_tracklets)) return rc;
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!grad_out || !offsets || !wsum) return fail(MTMC_E_ARG, "pool_tracklets_weighted_backward: NULL grad_out, offsets or wsum");
  if (((uintptr_t)grad_out & 15) || !pool_rows_ok(grad_embeds, grad_row_stride, feat_dim))
    return fail(MTMC_E_ARG, "pool_tracklets_weighted_backward: grad_out and grad_embeds must be 16-byte aligned, the row stride a multiple of 4 and >= feat_dim");
  if (((uintptr_t)offsets & 7) || ((uintptr_t)perm & 7) || ((uintptr_t)weights & 3) || ((uintptr_t)wsum & 3))
    return fail(MTMC_E_ARG, "pool_tracklets_weighted_backward: offsets and perm must be 8-byte, weights and wsum 4-byte aligned");
  POOL_LAUNCH_WP(pool_backward_wp_kernel, perm, weights, dim3(pool_grid(seg_chunks(n_rows, kPoolR), feat_dim)),
                 static_cast<hipStream_t>(stream), grad_out, n_rows, (int)feat_dim, offsets, n_tracklets, perm, weights, wsum,
                 grad_embeds, grad_row_stride);
  return mtmc_api::launched("pool_tracklets_weighted_backward");
}

int32_t mtmc_pool_tracklets_weight_grad(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim,
                                        const int64_t* offsets, int64_t n_tracklets, const int64_t* perm, const float* grad_out,
                                        const float* out, const float* wsum, float* grad_weights, void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (const int rc = pool_args("pool_tracklets_weight_grad", n_rows, feat_dim, n_tracklets)) return rc;
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!offsets || !grad_out || !out || !wsum || !grad_weights)
    return fail(MTMC_E_ARG, "pool_tracklets_weight_grad: NULL offsets, grad_out, out, wsum or grad_weights");
  if (!pool_rows_ok(embeds, row_stride, feat_dim) || ((uintptr_t)grad_out & 15) || ((uintptr_t)out & 15))
    return fail(MTMC_E_ARG, "pool_tracklets_weight_grad: embeds, grad_out and out must be 16-byte aligned, the row stride a multiple of 4 and >= feat_dim");
  if (((uintptr_t)offsets & 7) || ((uintptr_t)perm & 7) || ((uintptr_t)wsum & 3) || ((uintptr_t)grad_weights & 3))
    return fail(MTMC_E_ARG, "pool_tracklets_weight_grad: offsets and perm must be 8-byte, wsum and grad_weights 4-byte aligned");
  const dim3 grid(seg_grid(seg_chunks(n_rows, kPoolGradRows), 1));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (perm)
    hipLaunchKernelGGL(pool_weight_grad_kernel<true>, grid, dim3(256), 0, s, embeds, row_stride, n_rows, (int)feat_dim, offsets,
                       n_tracklets, perm, grad_out, out, wsum, grad_weights);
  else
    hipLaunchKernelGGL(pool_weight_grad_kernel<false>, grid, dim3(256), 0, s, embeds, row_stride, n_rows, (int)feat_dim, offsets,
                       n_tracklets, perm, grad_out, out, wsum, grad_weights);
  return mtmc_api::launched("pool_tracklets_weight_grad");
}

}  // extern "C"
