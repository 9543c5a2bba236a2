// Stand-alone scatter_{add,mean,max}(src[E,C], index[E], dim=0, dim_size) for gfx950: the functional
// surface of the third-party op the reference aggregates with (pytorch-scatter 2.0.8; call sites
// reference models/mpn.py:196,199,202).  Inside MOTMPNet.forward the aggregation is fused into
// pass_c_kernel; these kernels serve callers that use the op on its own.
//   add : out zero-filled, out[index[e], c] += src[e, c]
//   mean: add, then divide by max(count, 1)
//   max : per-column maximum, rows nobody writes stay 0, argmax = smallest e attaining it (E if none)
// These three add with atomics: the last bits of a float sum change from run to run.  mtmc_scatter_grouped, further down, is the
// repeatable forward of the same three: a segmented reduction over a stable grouping of the rows (group_index.hip).
#include "api_error.h"
#include "kernels.h"
#include "seg_walk.h"
#include <limits.h>

namespace mtmc {

__device__ __forceinline__ int float_key(float f) {       // order-preserving float -> signed int
  const int b = __float_as_int(f);
  return b >= 0 ? b : (b ^ 0x7fffffff);
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k >= 0 ? k : (k ^ 0x7fffffff)); }

__global__ void scatter_fill_kernel(float* out, int64_t n, int bits) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = __int_as_float(bits);
}
__global__ void scatter_fill_i64_kernel(int64_t* out, int64_t n, int64_t v) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = v;
}

__global__ void scatter_add_kernel(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                                   int64_t dim_size, float* out, float* count) {
  const int64_t total = n_src * n_cols, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t e = i / n_cols, c = i % n_cols;
    const int64_t r = index[e];
    if (r < 0 || r >= dim_size) continue;
    unsafeAtomicAdd(out + r * n_cols + c, src[i]);
    if (count && c == 0) unsafeAtomicAdd(count + r, 1.0f);
  }
}
__global__ void scatter_div_kernel(float* out, const float* count, int64_t dim_size, int64_t n_cols) {
  const int64_t total = dim_size * n_cols, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const float cnt = count[i / n_cols];
    out[i] = out[i] / (cnt < 1.f ? 1.f : cnt);
  }
}
__global__ void scatter_max_kernel(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                                   int64_t dim_size, float* out) {
  const int64_t total = n_src * n_cols, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t e = i / n_cols, c = i % n_cols;
    const int64_t r = index[e];
    if (r < 0 || r >= dim_size) continue;
    atomicMax(reinterpret_cast<int*>(out) + r * n_cols + c, float_key(src[i]));
  }
}
__global__ void scatter_argmax_kernel(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                                      int64_t dim_size, const float* out_keys, int64_t* arg) {
  const int64_t total = n_src * n_cols, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t e = i / n_cols, c = i % n_cols;
    const int64_t r = index[e];
    if (r < 0 || r >= dim_size) continue;
    if (float_key(src[i]) == reinterpret_cast<const int*>(out_keys)[r * n_cols + c])
      atomicMin(reinterpret_cast<unsigned long long*>(arg) + r * n_cols + c, (unsigned long long)e);
  }
}
__global__ void scatter_unkey_kernel(float* out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int k = reinterpret_cast<int*>(out)[i];
    out[i] = (k == INT_MIN) ? 0.f : key_float(k);
  }
}

// the 1-D integer call form of the post-processing (reference utils.py:173-174, :308-309): int64 in, int64 out, exact
__global__ void scatter_add_i64_kernel(const int64_t* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                                       int64_t dim_size, int64_t* out) {
  const int64_t total = n_src * n_cols, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = index[i / n_cols];
    if (r < 0 || r >= dim_size) continue;
    atomicAdd(reinterpret_cast<unsigned long long*>(out) + r * n_cols + i % n_cols, (unsigned long long)src[i]);
  }
}

constexpr int kScatterBlocks = 4096;      // most workgroups (of 256 elements) of a launch

// mode 0 add, 1 mean, 2 max
static void launch_scatter(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                           float* out, float* count, int64_t* arg_out, int mode, hipStream_t s) {
  const int64_t n_out = dim_size * n_cols, n_in = n_src * n_cols;
  const dim3 g_out(blocks_for(n_out, 256, kScatterBlocks)), g_in(blocks_for(n_in, 256, kScatterBlocks));
  if (mode == 2) {
    hipLaunchKernelGGL(scatter_fill_kernel, g_out, dim3(256), 0, s, out, n_out, INT_MIN);
    if (n_in > 0) hipLaunchKernelGGL(scatter_max_kernel, g_in, dim3(256), 0, s, src, index, n_src, n_cols, dim_size, out);
    if (arg_out) {
      hipLaunchKernelGGL(scatter_fill_i64_kernel, g_out, dim3(256), 0, s, arg_out, n_out, n_src);
      if (n_in > 0)
        hipLaunchKernelGGL(scatter_argmax_kernel, g_in, dim3(256), 0, s, src, index, n_src, n_cols, dim_size, out, arg_out);
    }
    hipLaunchKernelGGL(scatter_unkey_kernel, g_out, dim3(256), 0, s, out, n_out);
    return;
  }
  hipLaunchKernelGGL(scatter_fill_kernel, g_out, dim3(256), 0, s, out, n_out, 0);
  if (mode == 1)
    hipLaunchKernelGGL(scatter_fill_kernel, dim3(blocks_for(dim_size, 256, kScatterBlocks)), dim3(256), 0, s, count, dim_size, 0);
  if (n_in > 0)
    hipLaunchKernelGGL(scatter_add_kernel, g_in, dim3(256), 0, s, src, index, n_src, n_cols, dim_size, out,
                       mode == 1 ? count : nullptr);
  if (mode == 1) hipLaunchKernelGGL(scatter_div_kernel, g_out, dim3(256), 0, s, out, count, dim_size, n_cols);
}

static void launch_scatter_add_i64(const int64_t* src, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                                   int64_t* out, hipStream_t s) {
  const int64_t n_out = dim_size * n_cols, n_in = n_src * n_cols;
  hipLaunchKernelGGL(scatter_fill_i64_kernel, dim3(blocks_for(n_out, 256, kScatterBlocks)), dim3(256), 0, s, out, n_out, (int64_t)0);
  if (n_in > 0)
    hipLaunchKernelGGL(scatter_add_i64_kernel, dim3(blocks_for(n_in, 256, kScatterBlocks)), dim3(256), 0, s, src, index, n_src,
                       n_cols, dim_size, out);
}

// The backward passes with respect to src: gathers.  With g = d loss / d out [dim_size, C] and r = index[e],
//   add : d_src[e, c] = g[r, c]
//   mean: d_src[e, c] = g[r, c] / (float)max(count[r], 1), count recounted with integer atomics (the forward's is not kept)
//   max : d_src[e, c] = arg[r, c] == e ? g[r, c] : 0, arg the forward's second output
// and a row of zeros where r lies outside [0, dim_size).  Every element of d_src is written once, by one thread: no fill,
// no float atomics, the same bits on every run.  A stream of 4 C E bytes of stores that nobody in the launch reads again
// (non-temporal, as pool_backward_kernel's) beside the 8 E bytes of the index; g (and arg) are re-read once per edge of a row
// and mostly come from cache (default policy).
typedef float sc_f4 __attribute__((ext_vector_type(4)));
typedef long long sc_l2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float sc_keep(float g, const int64_t* arg, int64_t at, int64_t e) { return arg[at] == e ? g : 0.f; }
__device__ __forceinline__ sc_f4 sc_keep(sc_f4 g, const int64_t* arg, int64_t at, int64_t e) {
  const sc_l2 a = *reinterpret_cast<const sc_l2*>(arg + 4 * at), b = *reinterpret_cast<const sc_l2*>(arg + 4 * at + 2);
  return sc_f4{a.x == e ? g.x : 0.f, a.y == e ? g.y : 0.f, b.x == e ? g.z : 0.f, b.y == e ? g.w : 0.f};
}

constexpr int kScatterBwdBlocks = 2048;   // 8 waves per SIMD on every CU: one resident round
constexpr int kScatterBwdUnroll = 2;      // independent index -> g -> store chains per thread and trip

// V = float: one column per lane; V = sc_f4: four (C % 4 == 0, 16-byte aligned g, d_src and arg).  `units` = V's per row.
// Consecutive lanes take consecutive units, then rows: a wave's stores are whole lines.  A thread finds its (row, unit) once
// from a 32-bit first index and advances it by the launch's stride, which the host has cut into whole rows (step_rows) and a
// rest (step_rest): no division in the loop.  dim_size >= 1: the loads of a row that is out of range go to row 0 and the
// result is dropped, so all loads of a trip are in flight together.
template <int MODE, typename V>
__global__ __launch_bounds__(256) void scatter_backward_kernel(const V* __restrict__ g, const int64_t* __restrict__ arg,
                                                               const int64_t* __restrict__ index, const int* __restrict__ count,
                                                               int64_t n_src, int64_t units, int64_t dim_size, int64_t step_rows,
                                                               int64_t step_rest, V* __restrict__ d_src) {
  constexpr int U = kScatterBwdUnroll;
  const unsigned first = blockIdx.x * 256u + threadIdx.x;                           // < kScatterBwdBlocks * 256
  const unsigned units32 = units > 0xffffffffll ? 0xffffffffu : (unsigned)units;    // (then first < units32: row 0)
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t e = first / units32, c = first % units32, q = first;
  while (e < n_src) {
    int64_t ee[U], qq[U], at[U], rr[U];
    bool ok[U];
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ee[u] = e; qq[u] = q; at[u] = c;
      e += step_rows; c += step_rest; q += stride;
      if (c >= units) { c -= units; ++e; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = index[ee[u] < n_src ? ee[u] : n_src - 1];
      ok[u] = r >= 0 && r < dim_size;
      rr[u] = ok[u] ? r : 0;
      at[u] += rr[u] * units;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = g[at[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (MODE == 1) {
        const int n = count[rr[u]];
        v[u] = v[u] / (float)(n < 1 ? 1 : n);
      }
      if (MODE == 2) v[u] = sc_keep(v[u], arg, at[u], ee[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ee[u] < n_src) __builtin_nontemporal_store(ok[u] ? v[u] : V(0.f), d_src + qq[u]);
  }
}

// count[r] += rows e with index[e] == r.  Each workgroup takes one contiguous piece of the index, each wave 64 consecutive
// rows of it at a time.  Few destinations (dim_size <= kCountBins): the workgroup counts in LDS and adds its non-empty bins
// to count[] at the end -- a handful of global atomics per workgroup instead of one per row on a few hundred addresses.
// More: straight to count[].
constexpr int kCountBins = 8192;
constexpr int kCountRows = 2048;          // rows per workgroup (before the cap)
constexpr int kCountBlocks = 1024;

template <bool LDS>
__global__ __launch_bounds__(256) void scatter_count_kernel(const int64_t* index, int64_t n_src, int64_t dim_size, int64_t piece,
                                                            int* count) {
  __shared__ int bins[LDS ? kCountBins : 1];
  if (LDS) {
    for (int b = threadIdx.x; b < dim_size; b += 256) bins[b] = 0;
    __syncthreads();
  }
  const int64_t lo = blockIdx.x * piece, hi = lo + piece < n_src ? lo + piece : n_src;
  const int lane = threadIdx.x & 63;
  for (int64_t base = lo; base < hi; base += 256) {        // (the same trips in every lane: all 64 reach the ballot)
    const int64_t e = base + threadIdx.x;
    const int64_t r = e < hi ? index[e] : -1;
    // A wave holds 64 consecutive rows: the first lane of every run of equal destinations adds the run's length (a sorted
    // index: one or two adds per wave instead of 64 on the same address)
    const int64_t left = __shfl_up(r, 1);                  // (by all 64 lanes: not behind the `lane == 0 ||`)
    const bool head = lane == 0 || left != r;
    const unsigned long long heads = __ballot(head), later = lane == 63 ? 0ull : heads >> (lane + 1);
    if (!head || r < 0 || r >= dim_size) continue;
    const int len = later ? __ffsll(later) : 64 - lane;
    if (LDS) atomicAdd(bins + r, len); else atomicAdd(count + r, len);
  }
  if (LDS) {
    __syncthreads();
    for (int b = threadIdx.x; b < dim_size; b += 256)
      if (bins[b]) atomicAdd(count + b, bins[b]);
  }
}

template <int MODE, typename V>
static void launch_scatter_backward_as(const float* g, const int64_t* arg, const int64_t* index, const int* count, int64_t n_src,
                                       int64_t units, int64_t dim_size, float* d_src, hipStream_t s) {
  const int blocks = blocks_for(n_src * units, 256 * kScatterBwdUnroll, kScatterBwdBlocks);
  const int64_t stride = (int64_t)blocks * 256;
  hipLaunchKernelGGL((scatter_backward_kernel<MODE, V>), dim3(blocks), dim3(256), 0, s, reinterpret_cast<const V*>(g), arg, index,
                     count, n_src, units, dim_size, stride / units, stride % units, reinterpret_cast<V*>(d_src));
}

// mode 0 add, 1 mean, 2 max; n_src, n_cols >= 1.  count: int[dim_size], zeroed by the caller on this stream (mean only)
static void launch_scatter_backward(const float* g, const int64_t* arg, const int64_t* index, int64_t n_src, int64_t n_cols,
                                    int64_t dim_size, int* count, float* d_src, int mode, hipStream_t s) {
  if (dim_size == 0) {                                     // every row is out of range, and g has none to read
    const int64_t n = n_src * n_cols;
    hipLaunchKernelGGL(scatter_fill_kernel, dim3(blocks_for(n, 256, kScatterBlocks)), dim3(256), 0, s, d_src, n, 0);
    return;
  }
  if (mode == 1) {
    const int blocks = blocks_for(n_src, kCountRows, kCountBlocks);
    const int64_t piece = (n_src + blocks - 1) / blocks;
    if (dim_size <= kCountBins)
      hipLaunchKernelGGL(scatter_count_kernel<true>, dim3(blocks), dim3(256), 0, s, index, n_src, dim_size, piece, count);
    else
      hipLaunchKernelGGL(scatter_count_kernel<false>, dim3(blocks), dim3(256), 0, s, index, n_src, dim_size, piece, count);
  }
  const bool wide = n_cols % 4 == 0 && !(((uintptr_t)g | (uintptr_t)d_src | (mode == 2 ? (uintptr_t)arg : 0)) & 15);
  const int64_t units = wide ? n_cols / 4 : n_cols;
#define MTMC_SCATTER_BWD(MODE)                                                                                         \
  (wide ? launch_scatter_backward_as<MODE, sc_f4>(g, arg, index, count, n_src, units, dim_size, d_src, s)               \
        : launch_scatter_backward_as<MODE, float>(g, arg, index, count, n_src, units, dim_size, d_src, s))
  if (mode == 0) MTMC_SCATTER_BWD(0);
  else if (mode == 1) MTMC_SCATTER_BWD(1);
  else MTMC_SCATTER_BWD(2);
#undef MTMC_SCATTER_BWD
}

// ---- the repeatable forward: a segmented reduction over a grouping (group_index.hip) ----
// perm [E] lists the source rows group by group, offsets [N + 1] cut its POSITIONS: out[g] reduces the rows perm[j],
// offsets[g] <= j < offsets[g + 1].  No fill, no float atomic, no count buffer: every output element has one writer and every
// sum ONE ORDER, fixed by (E, C, offsets) alone.  The decomposition is seg_walk.h's, with chunks of kSegR = 64 positions and
// slabs of 64 lanes' columns:
//   * a lane holds W columns (4 when C % 4 == 0, else 1) of one row: U = C / W lanes cover a row, rounded up to a power of two
//     U' <= 64, so a wave covers P = 64 / U' rows at a time (C = 4: 64 rows, C = 32: 8 rows; C > 256 or 64: one row, in
//     slabs).  The same lanes hold the same columns whether the loads are 16-byte ones or, on unaligned pointers, four
//     scalar ones: the alignment changes the instructions, not the order;
//   * the piece [lo, hi) of a group inside a chunk: sub-row q = lane / U' adds positions lo + q, lo + q + P, ... in that order,
//     starting from -0.0 (x + -0.0 = x for every x, so a group of one row is a copy of that row), then the P sub-rows fold in
//     a butterfly, partner q ^ (P / 2) first and q ^ 1 last;
//   * scatter_seg_finish_kernel folds the list tail, head, head, ... of a crossing group by the same rule (sub-row q takes
//     items q, q + P, ...; then the butterfly).
//   mean divides the sum by (float)max(offsets[g + 1] - offsets[g], 1); max compares float_key and keeps the smallest source
//   row of the maximum, which is order-free.  A perm entry outside [0, E) names no row.  (A crossing group all of whose
//   entries name no row sums to -0.0.)
constexpr int kSegR = 64;

// what a lane carries: W sums, or W (key, source row) pairs
template <int W, bool MAX> struct SegAcc {
  float v[W];
  int key[W], arg[W];
  __device__ __forceinline__ void clear(int none) {
#pragma unroll
    for (int k = 0; k < W; ++k) { v[k] = -0.f; key[k] = INT_MIN; arg[k] = none; }
  }
  __device__ __forceinline__ void take(int k, int okey, int oarg) {
    if (okey > key[k] || (okey == key[k] && oarg < arg[k])) { key[k] = okey; arg[k] = oarg; }
  }
  __device__ __forceinline__ void fold(int up) {           // the butterfly over the sub-rows: every lane ends with the result
    for (int m = 32; m >= up; m >>= 1) {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if (MAX) take(k, __shfl_xor(key[k], m, 64), __shfl_xor(arg[k], m, 64));
        else v[k] += __shfl_xor(v[k], m, 64);
      }
    }
  }
};

template <int W, bool AL> __device__ __forceinline__ void seg_load(const float* p, float* v) {
  if (W == 4 && AL) {
    const sc_f4 t = *reinterpret_cast<const sc_f4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = p[k];
  }
}
template <int W, bool AL> __device__ __forceinline__ void seg_store(float* p, const float* v) {
  if (W == 4 && AL) {
    *reinterpret_cast<sc_f4*>(p) = sc_f4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = v[k];
  }
}

struct SegArgs {
  const float* src;
  const int64_t *perm, *offsets;
  int64_t E, C, N;
  int lg_up, slabs, mean;
  float *out, *partial;
  int64_t *arg_out, *parg;
};

// which (item, columns, sub-row) this lane works on; false: the wave has no item
struct SegLane { int64_t item, col; int q; bool live; };
template <int W> __device__ __forceinline__ bool seg_lane(const SegArgs& a, int64_t items, SegLane* l) {
  int slab;
  seg_wave(a.slabs, &l->item, &slab);
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)slab * 64 + (lane & ((1 << a.lg_up) - 1));
  l->q = lane >> a.lg_up;
  l->live = unit < a.C / W;
  l->col = l->live ? unit * W : 0;
  return l->item < items;
}

// the finished row of group s, by the lanes of sub-row 0
template <int W, bool MAX, bool AL>
__device__ __forceinline__ void seg_finish_row(const SegArgs& a, const SegLane& l, int64_t s, int64_t count, SegAcc<W, MAX>& acc) {
  if (l.q != 0 || !l.live) return;
  float v[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (MAX) v[k] = acc.key[k] == INT_MIN ? 0.f : key_float(acc.key[k]);
    else v[k] = a.mean ? acc.v[k] / (float)(count < 1 ? 1 : count) : acc.v[k];
  }
  seg_store<W, AL>(a.out + s * a.C + l.col, v);
  if (MAX && a.arg_out) {
#pragma unroll
    for (int k = 0; k < W; ++k) a.arg_out[s * a.C + l.col + k] = acc.arg[k];
  }
}

template <int W, bool MAX, bool AL>
__global__ __launch_bounds__(256) void scatter_seg_chunks_kernel(SegArgs a) {
  SegLane l;
  if (!seg_lane<W>(a, seg_chunks(a.E, kSegR), &l)) return;
  const int up = 1 << a.lg_up, P = 64 >> a.lg_up, lane = threadIdx.x & 63;
  const int64_t c = l.item, r0 = c * kSegR, r1 = seg_chunk_end(r0, kSegR, a.E);
  int row = -1;                                            // of position r0 + lane; -1: names no row
  if (r0 + lane < r1) {
    const int64_t p = a.perm[r0 + lane];
    if (p >= 0 && p < a.E) row = (int)p;                   // E < 2^31
  }
  for (SegCursor<const int64_t*> w(a.offsets, a.N, a.E, r0, r1); w.next();) {
    const int64_t s = w.s, ga = w.a, gb = w.b, lo = w.lo, hi = w.hi;
    SegAcc<W, MAX> acc;
    acc.clear((int)a.E);
    const int end = (int)(hi - r0);
    bool any = false;
    for (int base = (int)(lo - r0); base < end; base += 2 * P) {      // (the same trips in every lane: all 64 shuffle)
      int rr[2];
      bool ok[2];
      float v[2][W];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int at = base + t * P + l.q;
        rr[t] = __shfl(row, at & 63, 64);
        ok[t] = at < end && rr[t] >= 0;
        any |= __ballot(ok[t]) != 0;
        ok[t] = ok[t] && l.live;
        if (ok[t]) seg_load<W, AL>(a.src + (int64_t)rr[t] * a.C + l.col, v[t]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (!ok[t]) continue;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if (MAX) acc.take(k, float_key(v[t][k]), rr[t]); else acc.v[k] += v[t][k];
        }
      }
    }
    acc.fold(up);
    if (seg_inside(ga, gb, r0, r1)) {
      if (!any) {                                          // no entry named a row: the row nobody writes
#pragma unroll
        for (int k = 0; k < W; ++k) acc.v[k] = 0.f;
      }
      seg_finish_row<W, MAX, AL>(a, l, s, gb - ga, acc);
    } else if (l.q == 0 && l.live) {
      const int64_t at = seg_slot(c, ga, r0) * a.C + l.col;
      if (MAX) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
          a.partial[at + k] = __int_as_float(acc.key[k]);
          a.parg[at + k] = acc.arg[k];
        }
      } else {
        seg_store<W, AL>(a.partial + at, acc.v);
      }
    }
  }
}

template <int W, bool MAX, bool AL>
__global__ __launch_bounds__(256) void scatter_seg_finish_kernel(SegArgs a) {
  SegLane l;
  if (!seg_lane<W>(a, a.N, &l)) return;
  const int up = 1 << a.lg_up, P = 64 >> a.lg_up;
  const int64_t s = l.item, ga = seg_clamp(a.offsets[s], a.E), gb = seg_clamp(a.offsets[s + 1], a.E);
  SegAcc<W, MAX> acc;
  acc.clear((int)a.E);
  if (gb <= ga) {                                          // nobody writes this row: 0, argmax E
#pragma unroll
    for (int k = 0; k < W; ++k) acc.v[k] = 0.f;
    seg_finish_row<W, MAX, AL>(a, l, s, 1, acc);
    return;
  }
  const int64_t c0 = seg_first_chunk(ga, kSegR), c1 = seg_last_chunk(gb, kSegR);
  if (c0 == c1) return;                                    // finished inside its chunk
  const int64_t items = c1 - c0 + 1;                       // the tail of chunk c0, then the heads of c0 + 1 .. c1
  for (int64_t i = l.q; i < items && l.live; i += P) {
    const int64_t at = (i == 0 ? seg_tail(c0) : seg_head(c0 + i)) * a.C + l.col;
    float v[W];
    seg_load<W, AL>(a.partial + at, v);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (MAX) acc.take(k, __float_as_int(v[k]), (int)a.parg[at + k]); else acc.v[k] += v[k];
    }
  }
  acc.fold(up);
  seg_finish_row<W, MAX, AL>(a, l, s, gb - ga, acc);
}

static inline size_t seg_parg_offset(int64_t n_src, int64_t n_cols) {
  return (seg_plane_bytes(n_src, kSegR, n_cols) + 255) / 256 * 256;
}
static inline bool seg_sizes_ok(int64_t n_src, int64_t n_cols) {
  return n_src >= 0 && n_src < (1ll << 31) && n_cols >= 1 && n_cols < (1ll << 31);
}
static inline size_t seg_bytes(int64_t n_src, int64_t n_cols) {
  return seg_parg_offset(n_src, n_cols) + (size_t)seg_chunks(n_src, kSegR) * 2 * (size_t)n_cols * sizeof(int64_t) + 256;
}

template <int W, bool MAX, bool AL> static void launch_scatter_seg_as(const SegArgs& a, hipStream_t s) {
  if (a.E > 0)
    hipLaunchKernelGGL((scatter_seg_chunks_kernel<W, MAX, AL>), dim3(seg_grid(seg_chunks(a.E, kSegR), a.slabs)), dim3(256), 0, s, a);
  hipLaunchKernelGGL((scatter_seg_finish_kernel<W, MAX, AL>), dim3(seg_grid(a.N, a.slabs)), dim3(256), 0, s, a);
}

// mode 0 add, 1 mean, 2 max; dim_size >= 1
static void launch_scatter_seg(SegArgs a, int mode, hipStream_t s) {
  const bool four = a.C % 4 == 0;
  const bool al = four && !(((uintptr_t)a.src | (uintptr_t)a.out | (uintptr_t)a.partial) & 15);
  const int64_t units = four ? a.C / 4 : a.C;
  a.lg_up = 0;
  while (a.lg_up < 6 && (1ll << a.lg_up) < units) ++a.lg_up;
  a.slabs = (int)((units + 63) / 64);
  a.mean = mode == 1;
#define MTMC_SCATTER_SEG(MAX)                                                                                           \
  (!four ? launch_scatter_seg_as<1, MAX, false>(a, s)                                                                   \
         : al ? launch_scatter_seg_as<4, MAX, true>(a, s) : launch_scatter_seg_as<4, MAX, false>(a, s))
  if (mode == 2) MTMC_SCATTER_SEG(true); else MTMC_SCATTER_SEG(false);
#undef MTMC_SCATTER_SEG
}

}  // namespace mtmc

extern "C" {

using mtmc_api::fail;
using mtmc_api::launched;

static int scatter_common(const char* entry, const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                          int64_t dim_size, float* out, float* count, int64_t* arg_out, int mode, void* stream) {
  if (n_src < 0 || n_cols < 1 || dim_size < 0 || !out || (n_src > 0 && (!src || !index)))
    return fail(MTMC_E_ARG, "%s: n_src and dim_size must be >= 0, n_cols >= 1, and out (with rows: src and index) not NULL", entry);
  if (mode == 1 && !count) return fail(MTMC_E_ARG, "%s: needs count_scratch[dim_size]", entry);
  if (dim_size == 0) return MTMC_OK;
  mtmc::launch_scatter(src, index, n_src, n_cols, dim_size, out, count, arg_out, mode, static_cast<hipStream_t>(stream));
  return launched(entry);
}
int32_t mtmc_scatter_add(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                         float* out, void* stream) {
  return scatter_common("scatter_add", src, index, n_src, n_cols, dim_size, out, nullptr, nullptr, 0, stream);
}
int32_t mtmc_scatter_add_i64(const int64_t* src, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                             int64_t* out, void* stream) {
  if (n_src < 0 || n_cols < 1 || dim_size < 0 || !out || (n_src > 0 && (!src || !index)))
    return fail(MTMC_E_ARG, "scatter_add_i64: n_src and dim_size must be >= 0, n_cols >= 1, and out (with rows: src and index) not NULL");
  if (dim_size == 0) return MTMC_OK;
  mtmc::launch_scatter_add_i64(src, index, n_src, n_cols, dim_size, out, static_cast<hipStream_t>(stream));
  return launched("scatter_add_i64");
}
int32_t mtmc_scatter_mean(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                          float* out, float* count_scratch, void* stream) {
  return scatter_common("scatter_mean", src, index, n_src, n_cols, dim_size, out, count_scratch, nullptr, 1, stream);
}
int32_t mtmc_scatter_max(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                         float* out, int64_t* arg_out, void* stream) {
  return scatter_common("scatter_max", src, index, n_src, n_cols, dim_size, out, nullptr, arg_out, 2, stream);
}

size_t mtmc_scatter_grouped_workspace_bytes(int64_t n_src, int64_t n_cols) {
  return mtmc::seg_sizes_ok(n_src, n_cols) ? mtmc::seg_bytes(n_src, n_cols) : 0;
}

int32_t mtmc_scatter_grouped(const float* src, int64_t n_src, int64_t n_cols, const int64_t* perm, const int64_t* offsets,
                             int64_t dim_size, int32_t mode, float* out, int64_t* arg_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (!mtmc::seg_sizes_ok(n_src, n_cols) || dim_size < 0 || dim_size >= (1ll << 31) || mode < 0 || mode > 2)
    return fail(MTMC_E_ARG, "scatter_grouped: n_src and dim_size must be in [0, 2^31), n_cols in [1, 2^31), mode 0 (add), 1 (mean) or 2 (max)");
  if (dim_size == 0) return MTMC_OK;
  if (!out || !offsets || (n_src > 0 && (!src || !perm)))
    return fail(MTMC_E_ARG, "scatter_grouped: out and offsets (with rows: src and perm) must not be NULL");
  if ((((uintptr_t)src | (uintptr_t)out) & 3) || (((uintptr_t)perm | (uintptr_t)offsets | (uintptr_t)arg_out) & 7))
    return fail(MTMC_E_ARG, "scatter_grouped: src and out must be 4-byte, perm, offsets and arg_out 8-byte aligned");
  const size_t need = mtmc::seg_bytes(n_src, n_cols);
  if (n_src > 0 && (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need))
    return fail(MTMC_E_ARG, "scatter_grouped: workspace (16-byte aligned) has %zu bytes, %zu needed (mtmc_scatter_grouped_workspace_bytes)",
                workspace_bytes, need);
  mtmc::SegArgs a = {};
  a.src = src; a.perm = perm; a.offsets = offsets;
  a.E = n_src; a.C = n_cols; a.N = dim_size;
  a.out = out; a.arg_out = arg_out;
  a.partial = static_cast<float*>(workspace);
  a.parg = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + mtmc::seg_parg_offset(n_src, n_cols));
  mtmc::launch_scatter_seg(a, mode, static_cast<hipStream_t>(stream));
  return launched("scatter_grouped");
}

static int scatter_backward_common(const char* entry, const float* grad_out, const int64_t* arg, const int64_t* index,
                                   int64_t n_src, int64_t n_cols, int64_t dim_size, int32_t* count, float* grad_src, int mode,
                                   void* stream) {
  if (n_src < 0 || n_cols < 0 || dim_size < 0) return fail(MTMC_E_ARG, "%s: n_src, n_cols and dim_size must be >= 0", entry);
  if (n_src == 0 || n_cols == 0) return MTMC_OK;
  // (without destination rows there is no gradient to read: every row of grad_src is zero)
  if (!index || !grad_src || (dim_size > 0 && !grad_out)) return fail(MTMC_E_ARG, "%s: NULL grad_out, index or grad_src", entry);
  if (mode == 2 && dim_size > 0 && !arg) return fail(MTMC_E_ARG, "%s: NULL arg", entry);
  if (mode == 1 && dim_size > 0 && !count) return fail(MTMC_E_ARG, "%s: needs count_scratch[dim_size]", entry);
  if ((((uintptr_t)grad_out | (uintptr_t)grad_src | (uintptr_t)count) & 3) || (((uintptr_t)index | (uintptr_t)arg) & 7))
    return fail(MTMC_E_ARG, "%s: grad_out, grad_src and count_scratch must be 4-byte, index and arg 8-byte aligned", entry);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == 1 && dim_size > 0 && hipMemsetAsync(count, 0, (size_t)dim_size * sizeof(int32_t), s) != hipSuccess)
    return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
  mtmc::launch_scatter_backward(grad_out, arg, index, n_src, n_cols, dim_size, count, grad_src, mode, s);
  return launched(entry);
}
int32_t mtmc_scatter_add_backward(const float* grad_out, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                                  float* grad_src, void* stream) {
  return scatter_backward_common("scatter_add_backward", grad_out, nullptr, index, n_src, n_cols, dim_size, nullptr, grad_src, 0,
                                 stream);
}
int32_t mtmc_scatter_mean_backward(const float* grad_out, const int64_t* index, int64_t n_src, int64_t n_cols, int64_t dim_size,
                                   int32_t* count_scratch, float* grad_src, void* stream) {
  return scatter_backward_common("scatter_mean_backward", grad_out, nullptr, index, n_src, n_cols, dim_size, count_scratch,
                                 grad_src, 1, stream);
}
int32_t mtmc_scatter_max_backward(const float* grad_out, const int64_t* arg, const int64_t* index, int64_t n_src, int64_t n_cols,
                                  int64_t dim_size, float* grad_src, void* stream) {
  return scatter_backward_common("scatter_max_backward", grad_out, arg, index, n_src, n_cols, dim_size, nullptr, grad_src, 2,
                                 stream);
}

}  // extern "C"
