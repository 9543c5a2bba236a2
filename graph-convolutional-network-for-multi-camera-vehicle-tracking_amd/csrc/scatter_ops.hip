// Stand-alone scatter_{add,mean,max}(src[E,C], index[E], dim=0, dim_size) for gfx950: the functional
// surface of the third-party op the reference aggregates with (pytorch-scatter 2.0.8; call sites
// reference models/mpn.py:196,199,202).  Inside MOTMPNet.forward the aggregation is fused into
// pass_c_kernel; these kernels serve callers that use the op on its own.
//   add : out zero-filled, out[index[e], c] += src[e, c]
//   mean: add, then divide by max(count, 1)
//   max : per-column maximum, rows nobody writes stay 0, argmax = smallest e attaining it (E if none)
#include "api_error.h"
#include "kernels.h"
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
