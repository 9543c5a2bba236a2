// From detections to node features: the mean of the ReID embeddings of each tracklet's detections (reference
// train.py:305-316: one torch.mean(bboxes_embeds, 0) per tracklet, then torch.stack; libs/reid_feature_extraction.py:177-178
// the same once per tracklet), forward and backward.
//   mtmc_pool_tracklets           out[s] = mean of rows [offsets[s], offsets[s+1]) of embeds [D][F]
//   mtmc_pool_tracklets_backward  d_embeds[r] = g[s(r)] / len_s
// A pure streaming problem (F = 2048: 8 KB per row, tracklets of 1 to a few thousand rows); what there is to get right is the
// load balance and the order of the additions:
//   * the D rows are cut into chunks of kPoolR rows, the F columns into slabs of 256: ONE WAVE per (chunk, slab), one
//     float4 per lane, so every row read is 1 KiB coalesced and no wave ever walks more than kPoolR rows, however long the
//     longest tracklet is;
//   * a chunk finds its first tracklet by binary search in offsets, finishes the tracklets that lie wholly inside it (sum,
//     divide, store) and leaves at most two partial sums, in partial[chunk][2][F]: slot 0 ("head") for the tracklet that
//     came in from the previous chunk, slot 1 ("tail") for the one that goes on into the next;
//   * pool_finish_kernel, one wave per (tracklet, slab), adds the partial sums of a chunk-crossing tracklet IN CHUNK ORDER
//     (its first chunk's tail, then the heads of the chunks after it), divides and stores; it also writes the zero row of an
//     empty range and checks the offsets.
// No atomics on floats anywhere: every sum has one fixed order, so the result is the same bits on every run.
// The offsets live in device memory and the host never sees them: every value is clamped into [0, D] before it indexes
// anything, and what was wrong with them is reported in info[0] (0 ok; 1 not strictly increasing or outside [0, D];
// 2 offsets[0] != 0 or offsets[N] != D -- the larger one if both), info[1] = how many tracklets had a bad range.
#include "api_internal.h"
#include <limits.h>

namespace mtmc {

constexpr int kPoolR = 32;            // rows per chunk
constexpr int kPoolSlab = 256;        // columns per wave
constexpr int kPoolMaxF = 16384;
typedef float pool_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int64_t pool_clamp(int64_t v, int64_t D) { return v < 0 ? 0 : (v > D ? D : v); }

// the largest s in [0, N-1] with offsets[s] <= r (s = 0 if there is none); any contents of offsets end the search
__device__ __forceinline__ int64_t pool_find(const int64_t* offsets, int64_t N, int64_t D, int64_t r) {
  int64_t lo = 0, hi = N - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (pool_clamp(offsets[mid], D) <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// which (item, slab) this wave works on: the waves of a workgroup take neighbouring slabs of one item first
__device__ __forceinline__ bool pool_wave(int64_t items, int slabs, int F, int64_t* item, int* col) {
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  *item = w / slabs;
  *col = (int)(w - *item * slabs) * kPoolSlab + (int)(threadIdx.x & 63) * 4;
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
  if (!pool_wave((D + kPoolR - 1) / kPoolR, slabs, F, &c, &col)) return;
  const int64_t r0 = c * kPoolR, r1 = r0 + kPoolR < D ? r0 + kPoolR : D;
  int64_t cur = r0;
  for (int64_t s = pool_find(offsets, N, D, r0); s < N && cur < r1;) {
    const int64_t a = pool_clamp(offsets[s], D), b = pool_clamp(offsets[s + 1], D);
    if (b <= cur) { ++s; continue; }                      // empty, inverted or behind us: pool_finish_kernel's
    const int64_t lo = a > cur ? a : cur, hi = b < r1 ? b : r1;
    if (lo >= r1) break;
    const pool_f4 acc = pool_sum_rows(embeds + col, stride, lo, hi);
    if (a >= r0 && b <= r1) {
      *reinterpret_cast<pool_f4*>(out + s * F + col) = acc / (float)(b - a);
    } else {
      *reinterpret_cast<pool_f4*>(partial + (c * 2 + (a < r0 ? 0 : 1)) * F + col) = acc;
    }
    cur = hi;
    if (b > r1) break;
    ++s;
  }
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
  const int64_t a = pool_clamp(ra, D), b = pool_clamp(rb, D);
  pool_f4* dst = reinterpret_cast<pool_f4*>(out + s * F + col);
  if (b <= a) {
    *dst = pool_f4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const int64_t c0 = a / kPoolR, c1 = (b - 1) / kPoolR;
  if (c0 == c1) return;                                    // finished inside its chunk
  // the tail of chunk c0, then the heads of chunks c0 + 1 .. c1: rows of stride 2 F starting at the first head
  const pool_f4 tail = *reinterpret_cast<const pool_f4*>(partial + (c0 * 2 + 1) * F + col);
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
  if (!pool_wave((D + kPoolR - 1) / kPoolR, slabs, F, &c, &col)) return;
  const int64_t r0 = c * kPoolR, r1 = r0 + kPoolR < D ? r0 + kPoolR : D;
  float* dst = d_embeds + col;
  const pool_f4 zero = {0.f, 0.f, 0.f, 0.f};
  int64_t cur = r0;
  for (int64_t s = pool_find(offsets, N, D, r0); s < N && cur < r1;) {
    const int64_t a = pool_clamp(offsets[s], D), b = pool_clamp(offsets[s + 1], D);
    if (b <= cur) { ++s; continue; }
    const int64_t lo = a > cur ? (a < r1 ? a : r1) : cur, hi = b < r1 ? b : r1;
    for (; cur < lo; ++cur) *reinterpret_cast<pool_f4*>(dst + cur * stride) = zero;
    if (lo >= r1) break;
    const pool_f4 v = *reinterpret_cast<const pool_f4*>(g + s * F + col) / (float)(b - a);
    // (non-temporal: D F 4 bytes nobody in this launch reads again; measured 84 -> 55 us on 310 MB against plain stores)
    for (; cur < hi; ++cur) __builtin_nontemporal_store(v, reinterpret_cast<pool_f4*>(dst + cur * stride));
    if (b > r1) break;
    ++s;
  }
  for (; cur < r1; ++cur) *reinterpret_cast<pool_f4*>(dst + cur * stride) = zero;
}

// host side: sizes and launch grids
static inline bool pool_sizes_ok(int64_t n_rows, int32_t feat_dim) {
  return n_rows >= 0 && n_rows < (1ll << 31) && feat_dim >= 4 && feat_dim <= kPoolMaxF && feat_dim % 4 == 0;
}
static inline int64_t pool_chunks(int64_t n_rows) { return (n_rows + kPoolR - 1) / kPoolR; }
static inline size_t pool_partial_bytes(int64_t n_rows, int32_t feat_dim) {
  return (size_t)pool_chunks(n_rows) * 2 * (size_t)feat_dim * sizeof(float);
}
static inline unsigned pool_grid(int64_t items, int32_t feat_dim) {      // four waves per workgroup
  const int64_t waves = items * ((feat_dim + kPoolSlab - 1) / kPoolSlab);
  return (unsigned)blocks_for(waves, 4, INT_MAX);
}

}  // namespace mtmc

extern "C" {

int32_t mtmc_pool_chunk_rows(void) { return mtmc::kPoolR; }

size_t mtmc_pool_tracklets_workspace_bytes(int64_t n_rows, int32_t feat_dim) {
  if (!mtmc::pool_sizes_ok(n_rows, feat_dim)) return 0;
  return mtmc_api::align_up(mtmc::pool_partial_bytes(n_rows, feat_dim) + 1);
}

int32_t mtmc_pool_tracklets(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                            int64_t n_tracklets, float* out, int32_t* info, void* workspace, size_t workspace_bytes,
                            void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (!pool_sizes_ok(n_rows, feat_dim))
    return fail(MTMC_E_ARG, "pool_tracklets: n_rows must be in [0, 2^31) and feat_dim a multiple of 4 in [4, %d]", kPoolMaxF);
  if (n_tracklets < 0 || n_tracklets >= (1ll << 31)) return fail(MTMC_E_ARG, "pool_tracklets: n_tracklets must be in [0, 2^31)");
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!embeds || !offsets || !out) return fail(MTMC_E_ARG, "pool_tracklets: NULL embeds, offsets or out");
  if (((uintptr_t)embeds & 15) || (row_stride & 3) || row_stride < feat_dim)
    return fail(MTMC_E_ARG, "pool_tracklets: embeds must be 16-byte aligned with a row stride that is a multiple of 4 and >= feat_dim");
  if (((uintptr_t)out & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)info & 3) || ((uintptr_t)workspace & 15))
    return fail(MTMC_E_ARG, "pool_tracklets: out and workspace must be 16-byte, offsets 8-byte and info 4-byte aligned");
  const size_t need = pool_partial_bytes(n_rows, feat_dim);
  if (!workspace || workspace_bytes < need)
    return fail(MTMC_E_ARG, "pool_tracklets: workspace has %zu bytes, %zu needed (mtmc_pool_tracklets_workspace_bytes)", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(pool_chunks_kernel, dim3(pool_grid(pool_chunks(n_rows), feat_dim)), dim3(256), 0, s, embeds, row_stride,
                     n_rows, (int)feat_dim, offsets, n_tracklets, out, partial, reinterpret_cast<int*>(info));
  hipLaunchKernelGGL(pool_finish_kernel, dim3(pool_grid(n_tracklets, feat_dim)), dim3(256), 0, s, n_rows, (int)feat_dim, offsets,
                     n_tracklets, out, (const float*)partial, reinterpret_cast<int*>(info));
  return mtmc_api::launched("pool_tracklets");
}

int32_t mtmc_pool_tracklets_backward(const float* grad_out, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                                     int64_t n_tracklets, float* grad_embeds, int64_t grad_row_stride, void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (!pool_sizes_ok(n_rows, feat_dim))
    return fail(MTMC_E_ARG, "pool_tracklets_backward: n_rows must be in [0, 2^31) and feat_dim a multiple of 4 in [4, %d]", kPoolMaxF);
  if (n_tracklets < 0 || n_tracklets >= (1ll << 31)) return fail(MTMC_E_ARG, "pool_tracklets_backward: n_tracklets must be in [0, 2^31)");
  if (n_tracklets == 0 || n_rows == 0) return MTMC_OK;
  if (!grad_out || !offsets || !grad_embeds) return fail(MTMC_E_ARG, "pool_tracklets_backward: NULL grad_out, offsets or grad_embeds");
  if (((uintptr_t)grad_out & 15) || ((uintptr_t)grad_embeds & 15) || ((uintptr_t)offsets & 7) || (grad_row_stride & 3) ||
      grad_row_stride < feat_dim)
    return fail(MTMC_E_ARG, "pool_tracklets_backward: grad_out and grad_embeds must be 16-byte aligned, the row stride a multiple of 4 and >= feat_dim");
  hipLaunchKernelGGL(pool_backward_kernel, dim3(pool_grid(pool_chunks(n_rows), feat_dim)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), grad_out, n_rows, (int)feat_dim, offsets, n_tracklets, grad_embeds,
                     grad_row_stride);
  return mtmc_api::launched("pool_tracklets_backward");
}

}  // extern "C"
