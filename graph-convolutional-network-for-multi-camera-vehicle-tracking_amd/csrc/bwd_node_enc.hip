// Dense helpers of the node-encoder backward and the first launch of the backward (bwd_node_encoder_layer,
// bwd_clear_and_transpose in api_train.hip).
#include "bwd_common.h"

namespace mtmc {

// ------------------------------------------------------------------------------------------------
// dense helpers of the node-encoder backward
// ------------------------------------------------------------------------------------------------
// column statistics of g = (a > 0 ? dA/keep : 0) against zh = (Y-mu)*istd: stats[0..d) = sum g, [d..2d) = sum g*zh;
// MODE 1: dY = gamma*istd*(g - mean_g - zh*mean_gz) written over dA, and column sums of dY -> d_bias
constexpr int kBnBwdRows = 16;   // rows per workgroup: a few hundred node rows must still spread over the chip (64 rows
                                 // per workgroup: 12.4 / 8.1 us per launch at 430 x 1024)
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_kernel(BnBwdParams p) {
  if (MODE == 1 && blockIdx.z == 1) {               // passenger: relu(bn(Y_{l-1})) and its transpose (rows_body.h)
    RowsTJob j = p.rc;
    drop_resolve(j.drop);
    if ((int)blockIdx.x * 64 < j.dim) bn_relu_rows_t_body(j, blockIdx.x, blockIdx.y, gridDim.y);
    return;
  }
  if ((int)blockIdx.x * 64 >= p.dim) return;        // (the grid is as wide as the wider of the two jobs)
  drop_resolve(p.drop);
  __shared__ double red[2 * 4 * 64];
  __shared__ float tile[MODE == 1 ? kBnBwdRows : 1][65];          // MODE 1: dY^T leaves as 16-byte stores, one per thread
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.y * kBnBwdRows;
  double s0 = 0, s1 = 0;
  float dymax = 0.f;
  if (col < p.dim) {
    float mu, istd;
    mean_istd(p.stats_fwd[col], p.stats_fwd[p.dim + col], p.count, mu, istd);
    const float gam = p.gamma[col], bet = p.beta[col];
    const float ik = p.drop.on ? p.drop.inv_keep : 1.f;
    const float mg = MODE == 1 ? (float)(p.stats_bwd[col] / p.count) : 0.f;
    const float mgz = MODE == 1 ? (float)(p.stats_bwd[p.dim + col] / p.count) : 0.f;
#pragma unroll
    for (int i = 0; i < kBnBwdRows / 4; ++i) {
      const int64_t row = r0 + rg + 4 * i;
      if (MODE == 1) tile[rg + 4 * i][cl] = 0.f;                  // (rows past the end: the transposed copy's zero padding)
      if (row >= p.rows) continue;
      const float zh = (p.Y[row * p.dim + col] - mu) * istd;
      const float y = fmaf(gam, zh, bet);
      const bool live = y > 0.f && drop_keep(p.drop, p.drop_stream, (unsigned long long)row * p.dim + col);
      const float g = live ? p.dA[row * p.dim + col] * ik : 0.f;
      if (MODE == 0) {
        s0 += g;
        s1 += (double)g * zh;
      } else {
        const float dy = bn_bwd_dz(gam, istd, g, mg, zh, mgz);
        p.dA[row * p.dim + col] = dy;
        tile[rg + 4 * i][cl] = dy;
        dymax = fmaxf(dymax, fabsf(dy));
        s0 += dy;
      }
    }
  }
  if (MODE == 1 && p.dT && blockIdx.y == gridDim.y - 1 && col < p.dim)      // the transposed copy's padding rows behind the last tile
    for (int64_t row = r0 + kBnBwdRows + rg; row < p.ldt; row += 4) p.dT[(int64_t)col * p.ldt + row] = 0.f;
  red[rg * 64 + cl] = s0;
  red[256 + rg * 64 + cl] = s1;
  __syncthreads();
  if (MODE == 1 && p.dT) {
    static_assert(kBnBwdRows == 16, "a thread stores a quarter of a column's 16 rows");
    const int c = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (blockIdx.x * 64 + c < p.dim && r0 + 4 * q < p.ldt)        // (ldt: the row count padded to 32)
      *reinterpret_cast<float4*>(p.dT + (int64_t)(blockIdx.x * 64 + c) * p.ldt + r0 + 4 * q) =
          make_float4(tile[4 * q][c], tile[4 * q + 1][c], tile[4 * q + 2][c], tile[4 * q + 3][c]);
  }
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, c = blockIdx.x * 64 + (threadIdx.x & 63);
    if (c < p.dim) {
      const double* q = red + which * 256 + (threadIdx.x & 63);
      const double s = q[0] + q[64] + q[128] + q[192];
      if (MODE == 0) unsafeAtomicAdd(p.stats_bwd + which * p.dim + c, s);
      else if (which == 0) unsafeAtomicAdd(p.gr.b + c, (float)s);
    }
  }
  if (MODE == 1 && p.amax_out) {                   // operand scale of the weight- / input-gradient GEMMs
    __shared__ float wmax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dymax = fmaxf(dymax, __shfl_xor(dymax, off, 64));
    if (cl == 0) wmax[rg] = dymax;
    __syncthreads();
    if (threadIdx.x == 0)
      amax_publish(p.amax_out + (blockIdx.x + blockIdx.y) % kAmaxRep, fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
  }
  if (MODE == 1 && blockIdx.y == 0 && threadIdx.x < 64 && col < p.dim) {
    p.gr.g[col] = (float)p.stats_bwd[p.dim + col];
    p.gr.bt[col] = (float)p.stats_bwd[col];
  }
}

// dst[c][r] = src[r][c] for r < rows, 0 for rows <= r < rows_pad (dst leading dimension rows_pad), for several matrices in ONE
// launch (the node encoder's backward needs x^T and every W_l^T, all of them known before its first kernel: four 5 us launches
// on the chain become one).  1-D grid; a block finds its matrix by the block prefix.
__device__ __forceinline__ void transpose_job_body(const TransposeJobs& p, unsigned block) {
  __shared__ float tile[32][33];
  int j = 0;
  while (j + 1 < p.n && block >= p.job[j + 1].first_block) ++j;
  const TransposeJob& q = p.job[j];
  const unsigned b = block - q.first_block;
  const int64_t r0 = (int64_t)(b % q.blocks_r) * 32;
  const int c0 = (int)(b / q.blocks_r) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int64_t r = r0 + i;
    const int c = c0 + tx;
    tile[i][tx] = (r < q.rows && c < q.cols) ? q.src[r * q.ld_src + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i;
    const int64_t r = r0 + tx;
    if (c < q.cols && r < q.rows_pad) q.dst[(int64_t)c * q.rows_pad + r] = tile[tx][i];
  }
}
__global__ __launch_bounds__(256) void transpose_multi_kernel(TransposeJobs p) { transpose_job_body(p, blockIdx.x); }

void launch_bn_bwd(const BnBwdParams& p, int mode, hipStream_t s) {
  dim3 grid((p.dim + 63) / 64, (unsigned)((p.rows + kBnBwdRows - 1) / kBnBwdRows));
  if (mode == 0) { hipLaunchKernelGGL(bn_bwd_kernel<0>, grid, dim3(256), 0, s, p); return; }
  if (p.rc_on) {                                     // + the recomputation job: z = 1, the wider of the two in x
    static_assert(kBnBwdRows == 16, "both jobs cut the rows in 16s");
    const unsigned xb = (unsigned)(p.rc.dim + 63) / 64;
    grid.x = grid.x > xb ? grid.x : xb;
    grid.z = 2;
  }
  hipLaunchKernelGGL(bn_bwd_kernel<1>, grid, dim3(256), 0, s, p);
}

// The backward's first launch: what it accumulates into is cleared by the first n_zero workgroups, x^T and every W_l^T (which
// depend on nothing the backward computes) are made by the rest.
__global__ __launch_bounds__(256) void bwd_begin_kernel(ZeroRanges z, TransposeJobs t, unsigned n_zero) {
  if (blockIdx.x < n_zero) {
    const size_t nthreads = (size_t)n_zero * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int j = 0; j < z.n; ++j)
      for (size_t i = t0; i < z.r[j].n16; i += nthreads) z.r[j].p[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  transpose_job_body(t, blockIdx.x - n_zero);
}
void launch_bwd_begin(const ZeroRanges& z, const TransposeJobs& t, hipStream_t s) {
  size_t total = 0;
  for (int j = 0; j < z.n; ++j) total += z.r[j].n16;
  const size_t blocks = (total + 1023) / 1024;
  const unsigned nz = (unsigned)(blocks > 2048 ? 2048 : blocks);
  if (nz + t.n_blocks == 0) return;
  hipLaunchKernelGGL(bwd_begin_kernel, dim3(nz + t.n_blocks), dim3(256), 0, s, z, t, nz);
}

void transpose_jobs_add(TransposeJobs& p, const float* src, int64_t rows, int cols, int64_t ld_src, float* dst, int64_t rows_pad) {
  TransposeJob& q = p.job[p.n];
  q.src = src; q.rows = rows; q.cols = cols; q.ld_src = ld_src; q.dst = dst; q.rows_pad = rows_pad;
  q.blocks_r = (unsigned)((rows_pad + 31) / 32);
  q.first_block = p.n_blocks;
  p.n_blocks += q.blocks_r * (unsigned)((cols + 31) / 32);
  ++p.n;
}
void launch_transpose_multi(const TransposeJobs& p, hipStream_t s) {
  if (p.n_blocks == 0) return;
  hipLaunchKernelGGL(transpose_multi_kernel, dim3(p.n_blocks), dim3(256), 0, s, p);
}

}  // namespace mtmc
