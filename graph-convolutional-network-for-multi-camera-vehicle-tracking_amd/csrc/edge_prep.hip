// Per-edge passes of the message-passing network on gfx950 (MI355X), one translation unit per pass:
//   edge_prep.hip    prep, the edge encoder's hidden-layer moments, the L == 0 classifier           (this file)
//   edge_pass_a.hip  statistics of z1 = We.[h[row]|h[col]|e] + be                  (EdgeModel, mpn.py:67-69)
//   edge_pass_b.hip  e' = relu(bn(z1)) stored; moments of e'; per-node segment sums of e'
//   edge_pass_c.hip  m = relu(bn(Wn.[h[row]|e'] + bn)); h' = agg_row(m); logits      (NodeModel, mpn.py:97-99)
//   edge_common.h    what more than one of them uses
// These are the HBM-bound kernels: each streams the edge list once, gathers 16-byte per-node projections instead of the
// reference's 128-byte node rows (W.[h[row]|h[col]|e] = Pr[row]+Pc[col]+We.e), and never materialises the [E,68] / [E,36] /
// [E,32] intermediates of the reference (reference models/mpn.py:68, :97-98).  BatchNorm batch statistics are accumulated
// in fp64.
//
//   prep_kernel        int64 strided edge_index -> int32 row/col, out-degree, moments of edge_attr
//   enc2_kernel        moments of the edge-encoder hidden activations
//   classify_e0_kernel logits of the encoded edges when L == 0                      (mpn.py:295-297)
#include "edge_common.h"
#include "prep_body.h"
#include "split_body.h"

namespace mtmc {

// ------------------------------------------------------------------------------------------------
// prep
// ------------------------------------------------------------------------------------------------
template <bool SPLIT>      // SPLIT: the kernel also carries operand-split jobs (64 more registers per lane: few-edge graphs only)
__device__ void amax_jobs(const PrepParams& p, int block) {
  __shared__ float wmax[4];
  int j = 0;
  while (j + 1 < p.n_jobs && block >= p.jobs[j + 1].block0) ++j;      // every passenger workgroup serves ONE job
  const AmaxJob job = p.jobs[j];
  if (SPLIT && job.kind == kJobSplit) {        // operand split (x planes of few-row graphs / the weight-plane cache): split_body.h
    __shared__ unsigned long long fp_red[4];
    split_rows_body(job.ptr, job.ld, job.rows, job.cols, job.planes, job.rows * (int64_t)job.cols, job.inv, 0, job.rows,
                    block - job.block0, job.fp, fp_red, job.out);
    return;
  }
  const int c4n = job.cols / 4;                         // cols is a multiple of 32 (check_model)
  const int64_t total = job.rows * c4n;
  const bool dense = job.ld == job.cols;                // weights and contiguous x: no row arithmetic
  float m = 0.f;
  const int64_t stride = (int64_t)job.n_blocks * 256;
  auto at = [&](int64_t i) {
    const float* src = dense ? job.ptr + i * 4 : job.ptr + (i / c4n) * job.ld + (i % c4n) * 4;
    return *reinterpret_cast<const float4*>(src);
  };
  auto fold = [&](const float4 v) { m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w))); };
  int64_t i = (int64_t)(block - job.block0) * 256 + threadIdx.x;
  for (; i + 3 * stride < total; i += 4 * stride) {       // four independent 16-byte loads in flight per lane
    const float4 v0 = at(i), v1 = at(i + stride), v2 = at(i + 2 * stride), v3 = at(i + 3 * stride);
    fold(v0); fold(v1); fold(v2); fold(v3);
  }
  for (; i < total; i += stride) fold(at(i));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float b = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (b > 0.f) atomicMax(job.out + (block % kAmaxRep), __float_as_uint(b));
  }
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void prep_kernel(PrepParams p) {
  // passenger workgroups (operand scales / operand splits of the node encoder, the weight-plane cache's verification) come
  // FIRST in the grid: they are the longest (64 KB of reads each) and nothing else of the forward can start before the last
  // of them is done
  if ((int)blockIdx.x < p.n_pass_blocks) {
    amax_jobs<SPLIT>(p, blockIdx.x);
    return;
  }
  prep_edge_body<4>(p, (int)blockIdx.x - p.n_pass_blocks);      // (prep_body.h)
}

// The operand-split jobs by themselves (many-edge graphs: inside prep_kernel their 64 registers per lane cost the edge loop
// three waves per SIMD of occupancy -- 67 -> 109 us at config 4, profiles/r05_cfg4_kernel_stats.csv before / after)
__global__ __launch_bounds__(256) void split_jobs_kernel(PrepParams p) { amax_jobs<true>(p, blockIdx.x); }

// MTMC_F_SEED_ON_DEVICE: this forward's Dropout seed = the caller's device counter, which moves on by one
__global__ void seed_tick_kernel(unsigned long long* counter, unsigned long long* word) {
  const unsigned long long v = *counter;
  *word = v;
  *counter = v + 1;
}

// ------------------------------------------------------------------------------------------------
// edge encoder: hidden-layer moments; the classifier on the encoded edges (L == 0)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void enc2_kernel(EdgeEncParams enc, const float* attr, int64_t n_edges,
                                                   double e_total, double* stat_enc2) {
  enc2_body(enc, attr, n_edges, e_total, stat_enc2, blockIdx.x, gridDim.x);   // (common.h: also carried by the few-row GEMM)
}
__global__ __launch_bounds__(256) void classify_e0_kernel(EdgeEncParams enc, const float* attr, int64_t n_edges,
                                                          double e_total, const float* cls_w, const float* cls_b,
                                                          int n_classes, float* logits) {
  drop_resolve(enc.drop);
  __shared__ EdgeEncAffine af;
  __shared__ double scratch[kStatAttr + kStatEnc2];
  edge_enc_affine_to_smem(enc, e_total, 2, &af, scratch);
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += nthreads) {
    float a0, a1, u[4], e0[4];
    load_attr(attr, enc.fe, e, a0, a1);
    edge_enc_hidden(enc, af, e, a0, a1, u);
    edge_enc_out(enc, af, e, u, e0);
    classify_edge(cls_w, cls_b, n_classes, make_float4(e0[0], e0[1], e0[2], e0[3]), logits + e * n_classes);
  }
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
static int size_jobs(PrepParams& p) {                    // block ranges of the passenger jobs; returns their total
  int extra = 0;
  for (int j = 0; j < p.n_jobs; ++j) {                  // ~16 float4 per lane, at most 2048 workgroups per operand
    const int64_t f4 = p.jobs[j].rows * (p.jobs[j].cols / 4), want = (f4 + 4095) / 4096;
    p.jobs[j].block0 = extra;
    p.jobs[j].n_blocks = p.jobs[j].kind == kJobSplit ? (int)((p.jobs[j].rows + 7) / 8)       // 8 rows per workgroup
                                                     : (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    extra += p.jobs[j].n_blocks;
  }
  return extra;
}
void launch_prep(const PrepParams& p0, hipStream_t s) {
  PrepParams p = p0;
  p.n_edge_blocks = p.n_edges > 0 ? edge_grid(p.n_edges, 256) : 0;
  bool any_split = false;
  for (int j = 0; j < p.n_jobs; ++j) any_split = any_split || p.jobs[j].kind == kJobSplit;
  if (any_split && p.n_edges > kSmallEdges) {           // many edges: the split jobs in a launch of their own (see above)
    PrepParams q = p0;
    q.n_edges = 0; q.n_edge_blocks = 0; q.n_jobs = 0;
    p.n_jobs = 0;
    for (int j = 0; j < p0.n_jobs; ++j) {
      if (p0.jobs[j].kind == kJobSplit) q.jobs[q.n_jobs++] = p0.jobs[j];
      else p.jobs[p.n_jobs++] = p0.jobs[j];
    }
    q.n_pass_blocks = size_jobs(q);
    hipLaunchKernelGGL(split_jobs_kernel, dim3(q.n_pass_blocks), dim3(256), 0, s, q);
    any_split = false;
  }
  p.n_pass_blocks = size_jobs(p);
  if (p.n_edge_blocks + p.n_pass_blocks == 0) return;
  if (any_split) hipLaunchKernelGGL(prep_kernel<true>, dim3(p.n_edge_blocks + p.n_pass_blocks), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(prep_kernel<false>, dim3(p.n_edge_blocks + p.n_pass_blocks), dim3(256), 0, s, p);
}
void launch_enc2(const EdgeEncParams& enc, const float* attr, int64_t n_edges, double e_total, double* stat_enc2,
                 hipStream_t s) {
  hipLaunchKernelGGL(enc2_kernel, dim3(edge_grid(n_edges, 256)), dim3(256), 0, s, enc, attr, n_edges, e_total,
                     stat_enc2);
}
void launch_seed_tick(unsigned long long* counter, unsigned long long* word, hipStream_t s) {
  hipLaunchKernelGGL(seed_tick_kernel, dim3(1), dim3(1), 0, s, counter, word);
}
void launch_classify_e0(const EdgeEncParams& enc, const float* attr, int64_t n_edges, double e_total,
                        const float* cls_w, const float* cls_b, int n_classes, float* logits, hipStream_t s) {
  hipLaunchKernelGGL(classify_e0_kernel, dim3(edge_grid(n_edges, 256)), dim3(256), 0, s, enc, attr, n_edges, e_total,
                     cls_w, cls_b, n_classes, logits);
}

}  // namespace mtmc
