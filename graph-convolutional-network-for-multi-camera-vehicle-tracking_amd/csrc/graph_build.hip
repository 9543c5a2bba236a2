// Tracklet-graph construction on gfx950 (SURVEY.md 8(f)-1,2): everything the reference's callers do on the host /
// with O(E) 2048-d gathers between the per-tracklet features and the MPN call (reference inference.py:402-456,
// train.py:316-342):
//     x = F.normalize(feats, p=2, dim=0);  edges = cross-camera cartesian products;  edge labels;
//     edge_attr[e] = [ ||x_r - x_c + 1e-6||_2 ,  1 - cos(x_r, x_c) ]
// The per-edge 2048-d gather (16 KB per edge in the reference) becomes ONE Gram matrix G = X X^T plus an
// 8-byte-per-edge epilogue:
//     ||a-b+eps||^2 = |a|^2 + |b|^2 - 2 a.b + 2 eps (sum a - sum b) + F eps^2,    cos = a.b / (max(|a|,e) max(|b|,e))
// G goes through launch_gemm_bn without |.|max words (M = Nout = N, K = F), so gemm_plan picks, at fp32 accuracy throughout:
//     N <= 960            gemm_bn_kernel<1,1,*> (exact fp32 MFMA, 64 x 64 tiles): split-K 4 where F % 256 == 0, split-K 2 where
//                         only F % 128 == 0, unsplit where F <= 128 or F % 128 != 0; BK = 64 where the slice is a multiple of 64,
//                         else BK = 32
//     961 <= N <= 1920    the same kernel, unsplit at every F (256 tiles or more)
//     N >= 1921           gemm_bn_bf16x6_kernel<2,2,32> (128 x 128 tiles, six bf16 products per fp32 product)
//     F > 6144            linear_generic_kernel (one thread per element, a chain of F fmaf) up to N = 2048; refused above that
// tests/gram_cases.py names a case for each line and tests/test_gram_cases.py pins the splits.
#include "graph_build.h"

namespace mtmc {

// column sums of squares over the nodes (fp64): block = 64 columns x 64 rows
__global__ __launch_bounds__(256) void gb_colnorm_kernel(const float* x, int64_t ld, int64_t n, int f, double* colsq) {
  __shared__ double red[4 * 64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.y * 64;
  double s = 0;
  if (col < f)
    for (int64_t r = r0 + rg; r < r0 + 64 && r < n; r += 4) { const double v = x[r * ld + col]; s += v * v; }
  red[rg * 64 + cl] = s;
  __syncthreads();
  if (threadIdx.x < 64 && col < f) unsafeAtomicAdd(colsq + col, red[cl] + red[64 + cl] + red[128 + cl] + red[192 + cl]);
}

// x_out = x / max(||col||, 1e-12) (or a copy); per node |x|^2 and sum x of the normalised row (fp64 -> f32)
__global__ __launch_bounds__(256) void gb_normalize_kernel(const float* x, int64_t ld, int64_t n, int f,
                                                           const double* colsq, int l2norm, float* x_out,
                                                           float* row_sq, float* row_sum) {
  __shared__ double red[2 * 4];
  const int64_t r = blockIdx.x;
  double sq = 0, sm = 0;
  for (int c = threadIdx.x; c < f; c += 256) {
    float v = x[r * ld + c];
    if (l2norm) {
      const float nrm = (float)sqrt(colsq[c]);
      v = v / fmaxf(nrm, 1e-12f);
    }
    x_out[r * f + c] = v;
    sq += (double)v * v;
    sm += v;
  }
  sq = wave_sum(sq);
  sm = wave_sum(sm);
  if ((threadIdx.x & 63) == kWaveSumLane) { red[threadIdx.x >> 6] = sq; red[4 + (threadIdx.x >> 6)] = sm; }
  __syncthreads();
  if (threadIdx.x == 0) {
    row_sq[r] = (float)(red[0] + red[1] + red[2] + red[3]);
    row_sum[r] = (float)(red[4] + red[5] + red[6] + red[7]);
  }
}

__global__ __launch_bounds__(256) void gb_edges_kernel(EdgeBuildParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < p.n_edges; e += stride) {
    int lo = 0, hi = p.n_cams;                   // camera block containing e
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.block_off[mid] <= e) lo = mid; else hi = mid; }
    const int c = lo;
    const int64_t local = e - p.block_off[c];
    const int64_t n_out = p.out_off[c + 1] - p.out_off[c];
    const int row = p.in_list[p.in_off[c] + (int)(local / n_out)];
    const int col = p.out_list[p.out_off[c] + local % n_out];
    reinterpret_cast<longlong2*>(p.edge_index)[e] = make_longlong2(row, col);
    const float g = p.G[(int64_t)row * p.n_nodes + col];
    reinterpret_cast<float2*>(p.edge_attr)[e] =
        gb_edge_attr(g, p.row_sq[row], p.row_sq[col], p.row_sum[row], p.row_sum[col], p.f);
    if (p.edge_labels) p.edge_labels[e] = p.node_labels[row] == p.node_labels[col] ? 1.f : 0.f;
  }
}

// ---- backward of the construction: d(x, edge_attr) -> d feats without any per-edge 2048-d gather ----
// With a_e = gD_e / d_e (0 where d_e == 0), b_e = -gC_e, s_e = cos_e = 1 - edge_attr[e][1], rho_i = |x_i|:
//     S[i][j] = m_ij + m_ji,  m_e = -a_e + b_e / (rho_r rho_c)                       (0 where (i, j) is no edge)
//     delta_i = sum over edges that start or end at i of (a_e - b_e s_e / rho_i^2),   kappa_i = sum_{row=i} a_e - sum_{col=i} a_e
//     dXn     = gX + S . Xn + diag(delta) . Xn + 1e-6 kappa 1^T
//     dX[:,k] = (dXn[:,k] - Xn[:,k] <Xn[:,k], dXn[:,k]>) / n_k                        (l2norm; dX = dXn otherwise)
// The eps clamps of the forward (1e-8 on rho, 1e-12 on n_k) count as constants where they are active, as in autograd.

// node -> (camera block, position inside it): the inverse of in_list
__global__ __launch_bounds__(256) void gb_bwd_nodemap_kernel(const int* in_list, const int* in_off, int n_cams, int64_t n,
                                                             int* node_cam, int* node_loc) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int k = gb_segment_of(in_off, n_cams, q);
  const int node = in_list[q];
  if (node >= 0 && node < n) { node_cam[node] = k; node_loc[node] = (int)(q - in_off[k]); }
}

// rho_i = |x_i| exactly as the forward formed it: fp64 sum of squares -> f32 -> sqrtf
__global__ __launch_bounds__(256) void gb_bwd_rownorm_kernel(const float* x, int f, float* rho) {
  __shared__ double red[4];
  const int64_t r = blockIdx.x;
  double sq = 0;
  for (int c = threadIdx.x; c < f; c += 256) { const double v = x[r * f + c]; sq += v * v; }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == kWaveSumLane) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) rho[r] = sqrtf((float)(red[0] + red[1] + red[2] + red[3]));
}

struct GraphBwdCoef {
  const int* in_list; const int* in_off; const int* out_list; const int64_t* out_off; const int64_t* block_off;
  int n_cams; int64_t n_nodes; int64_t n_edges; int npad;
  const int* node_cam; const int* node_loc; const float* rho;
  const float* edge_attr; const float* d_attr;      // [E][2] each
  float* S;                                         // [N][npad], zero on entry
  float* delta; float* kappa;                       // [N]
  const float* X; float* out; int f;                // gb_bwd_near_kernel: x [N][F] and dXn [N][F]
};

// Near-duplicate ends (d^2 < 1e-3 (rho_r^2 + rho_c^2)): the Gram form of the forward has lost d to cancellation there and
// -a x_c + a x_r would cancel again in the product, so the distance term of such an edge stays out of S / delta / kappa and
// gb_bwd_near_kernel takes it from the F-dimensional difference itself.  The forward's absolute error on d^2 is
// c (rho_r^2 + rho_c^2) with c growing with the length of the fp32 chain; measured worst case per regime on MI355X
// (profiles/graph_build_envelope.txt; every case within 0.66 of twice a CPU model of the unsplit fp32 chain):
//     exact fp32, F <= 384 (BK 32 / BK 64 / split 2): 1.9e-7 .. 5.8e-7        split-K 4, F = 256: 2.7e-7
//     exact fp32 unsplit, F = 2048 (N 961..1920):     2.9e-6                  bf16x6: 3.6e-7 (F = 64), 1.5e-6 (F = 2048)
//     scalar path, F = 6176:                          2.8e-6
// i.e. 2e-4 to 3e-3 of the threshold: an edge just above it has its d^2 to 0.3 % or better.
__device__ __forceinline__ bool gb_near(float d, float rho_r, float rho_c) {
  return d * d < 1e-3f * (rho_r * rho_r + rho_c * rho_c);
}

// One workgroup per node i: row i of S, delta_i, kappa_i.  The edges that START at i are one contiguous run of the list
// (plain stores); the edge that ENDS at i from node j of camera k sits at block_off[k] + pos(j) * n_out(k) + rank of i in
// k's out_list -- every (i, j) once in each direction, so the second pass adds exactly one value per element.
__global__ __launch_bounds__(256) void gb_bwd_coef_kernel(GraphBwdCoef p) {
  __shared__ double red[8];
  const int i = blockIdx.x;
  const int ci = p.node_cam[i];
  if (ci < 0 || ci >= p.n_cams) {                   // node missing from in_list: no edges
    if (threadIdx.x == 0) { p.delta[i] = 0.f; p.kappa[i] = 0.f; }
    return;
  }
  const float rho_i = p.rho[i], r_i = fmaxf(rho_i, 1e-8f);
  const float inv_rho2 = rho_i > 1e-8f ? 1.f / (rho_i * rho_i) : 0.f;
  float* s_row = p.S + (int64_t)i * p.npad;
  const float2* attr = reinterpret_cast<const float2*>(p.edge_attr);
  const float2* grad = reinterpret_cast<const float2*>(p.d_attr);
  double dl = 0, kp = 0;
  auto coef = [&](int64_t e, int j, float sign) {
    const float2 at = attr[e], g = grad[e];
    const float a = (at.x > 0.f && !gb_near(at.x, rho_i, p.rho[j])) ? g.x / at.x : 0.f, b = -g.y, s = 1.f - at.y;
    dl += a - b * s * inv_rho2;
    kp += sign * a;
    return b / (r_i * fmaxf(p.rho[j], 1e-8f)) - a;
  };
  {
    const int64_t n_out = p.out_off[ci + 1] - p.out_off[ci];
    const int64_t e0 = p.block_off[ci] + p.node_loc[i] * n_out;
    const int* ol = p.out_list + p.out_off[ci];
    for (int64_t t = threadIdx.x; t < n_out; t += 256) {
      const int j = ol[t];
      if (e0 + t >= p.n_edges || j < 0 || j >= p.n_nodes) continue;
      s_row[j] = coef(e0 + t, j, 1.f);
    }
  }
  __threadfence();
  __syncthreads();
  for (int64_t q = threadIdx.x; q < p.n_nodes; q += 256) {
    const int k = gb_segment_of(p.in_off, p.n_cams, q);
    const int j = p.in_list[q];
    if (k == ci || j < 0 || j >= p.n_nodes) continue;
    const int* ol = p.out_list + p.out_off[k];
    const int64_t n_out = p.out_off[k + 1] - p.out_off[k];
    int64_t lo = 0, hi = n_out;                     // rank of i in camera k's ascending out_list
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (ol[mid] < i) lo = mid + 1; else hi = mid; }
    const int64_t e = p.block_off[k] + (q - p.in_off[k]) * n_out + lo;
    if (lo >= n_out || ol[lo] != i || e >= p.n_edges) continue;
    unsafeAtomicAdd(s_row + j, coef(e, j, -1.f));
  }
  dl = wave_sum(dl);
  kp = wave_sum(kp);
  if ((threadIdx.x & 63) == kWaveSumLane) { red[threadIdx.x >> 6] = dl; red[4 + (threadIdx.x >> 6)] = kp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.delta[i] = (float)(red[0] + red[1] + red[2] + red[3]);
    p.kappa[i] = (float)(red[4] + red[5] + red[6] + red[7]);
  }
}

// dXn = gX + S . Xn + diag(delta) . Xn + 1e-6 kappa 1^T on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32:
// 1 / d spreads S over orders of magnitude on near-duplicate tracklets).  NN operand form: S [N][npad] is k-contiguous
// like the A tiles of gemm_bn_kernel, Xn [N][F] has the node (= k) as its strided index -- its tile goes into LDS as
// [k][column], which is the order the B operand of the MFMA reads anyway (lane l: k = l / 32, column = l % 32).
// 64 x 64 tile per workgroup, 2 x 2 waves, BK = 32; npad is a multiple of 32 and S is zero beyond column N, Xn rows
// beyond N are read as zero.  Register-staged double buffering as in gemm_bn_kernel.
struct GraphBwdGemm {
  const float* S; int npad; const float* X; const float* gX; const float* delta; const float* kappa;
  float* out; int64_t n; int f;
};
typedef float gb_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void gb_bwd_gemm_kernel(GraphBwdGemm p) {
  constexpr int BM = 64, BN = 64, BK = 32, LDA = BK + 4, LDB = BN + 4;
  __shared__ __attribute__((aligned(16))) float As[BM * LDA];   // [row][k]
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];   // [k][column]
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[2], rb[2];
  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = threadIdx.x + i * 256;
      const int64_t row = m0 + t / 8;
      ra[i] = row < p.n ? *reinterpret_cast<const float4*>(p.S + row * p.npad + k0 + (t % 8) * 4) : zero4;
      const int64_t k = k0 + t / 16;
      const int col = n0 + (t % 16) * 4;
      rb[i] = (k < p.n && col < p.f) ? *reinterpret_cast<const float4*>(p.X + k * p.f + col) : zero4;
    }
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = threadIdx.x + i * 256;
      *reinterpret_cast<float4*>(As + (t / 8) * LDA + (t % 8) * 4) = ra[i];
      *reinterpret_cast<float4*>(Bs + (t / 16) * LDB + (t % 16) * 4) = rb[i];
    }
  };
  gb_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int a_off = (wm * 32 + (lane & 31)) * LDA + (lane >> 5) * 4;
  const int b_off = (lane >> 5) * 4 * LDB + wn * 32 + (lane & 31);
  load_tiles(0);
  for (int k0 = 0; k0 < p.npad; k0 += BK) {
    __syncthreads();                 // previous tile fully consumed
    store_tiles();
    __syncthreads();
    if (k0 + BK < p.npad) load_tiles(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      // lane half h supplies k = 8 kk + 4 h + j in step j, for both operands
      const float4 a = *reinterpret_cast<const float4*>(As + a_off + kk * 8);
      const float* b = Bs + b_off + kk * 8 * LDB;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[LDB], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[2 * LDB], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[3 * LDB], acc, 0, 0, 0);
    }
  }
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= p.f) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < p.n) {
      const int64_t at = row * p.f + col;
      float v = fmaf(p.delta[row], p.X[at], acc[r]) + 1e-6f * p.kappa[row];
      if (p.gX) v += p.gX[at];
      p.out[at] = v;
    }
  }
}

// The distance term of the near-duplicate edges (gb_near), after the product: one workgroup per node i walks the edges that
// start or end at i in windows of 256 (one candidate per thread, no atomics, fixed order) and adds, for each flagged one,
//     sign (gD / |v|) v,   v = sign (x_i - x_j) + 1e-6      (sign +1: the edge starts at i, -1: it ends there)
// to row i of dXn -- what autograd does for every edge, here for the few where it matters.  |v| in fp64.
__global__ __launch_bounds__(256) void gb_bwd_near_kernel(GraphBwdCoef p) {
  __shared__ unsigned long long masks[4];
  __shared__ int sj[256];
  __shared__ float sg[256], ss[256];
  __shared__ double red[4];
  const int i = blockIdx.x;
  const int ci = p.node_cam[i];
  if (ci < 0 || ci >= p.n_cams) return;
  const float rho_i = p.rho[i];
  const float2* attr = reinterpret_cast<const float2*>(p.edge_attr);
  const float2* grad = reinterpret_cast<const float2*>(p.d_attr);
  const int64_t n_out_i = p.out_off[ci + 1] - p.out_off[ci];
  const int64_t e0 = p.block_off[ci] + p.node_loc[i] * n_out_i;
  const float* xi = p.X + (int64_t)i * p.f;
  float* oi = p.out + (int64_t)i * p.f;
  for (int64_t base = 0; base < n_out_i + p.n_nodes; base += 256) {
    const int64_t cand = base + threadIdx.x;
    int64_t e = -1;
    int j = -1;
    float sign = 1.f;
    if (cand < n_out_i) {
      j = p.out_list[p.out_off[ci] + cand];
      e = e0 + cand;
    } else if (cand < n_out_i + p.n_nodes) {
      const int64_t q = cand - n_out_i;
      const int k = gb_segment_of(p.in_off, p.n_cams, q);
      if (k != ci) {
        j = p.in_list[q];
        const int* ol = p.out_list + p.out_off[k];
        const int64_t n_out = p.out_off[k + 1] - p.out_off[k];
        int64_t lo = 0, hi = n_out;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (ol[mid] < i) lo = mid + 1; else hi = mid; }
        if (lo < n_out && ol[lo] == i) e = p.block_off[k] + (q - p.in_off[k]) * n_out + lo;
        sign = -1.f;
      }
    }
    bool flagged = false;
    if (e >= 0 && e < p.n_edges && j >= 0 && j < p.n_nodes) {
      const float d = attr[e].x;
      if (gb_near(d, rho_i, p.rho[j])) { flagged = true; sj[threadIdx.x] = j; sg[threadIdx.x] = grad[e].x; ss[threadIdx.x] = sign; }
    }
    const unsigned long long m = __ballot(flagged);
    if ((threadIdx.x & 63) == 0) masks[threadIdx.x >> 6] = m;
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
      unsigned long long left = masks[w];
      while (left) {
        const int idx = w * 64 + __builtin_ctzll(left);
        left &= left - 1;
        const float sgn = ss[idx], gd = sg[idx];
        const float* xj = p.X + (int64_t)sj[idx] * p.f;
        double sq = 0;
        for (int c = threadIdx.x; c < p.f; c += 256) { const float v = sgn * (xi[c] - xj[c]) + 1e-6f; sq += (double)v * v; }
        sq = wave_sum(sq);
        if ((threadIdx.x & 63) == kWaveSumLane) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        const double d2 = red[0] + red[1] + red[2] + red[3];
        __syncthreads();
        const float a = d2 > 0 ? sgn * gd / (float)sqrt(d2) : 0.f;
        for (int c = threadIdx.x; c < p.f; c += 256) oi[c] = fmaf(a, sgn * (xi[c] - xj[c]) + 1e-6f, oi[c]);
      }
    }
    __syncthreads();
  }
}

// dot[c] += sum over a 64-row block of x[r][c] * g[r][c] (fp64), laid out like gb_colnorm_kernel
__global__ __launch_bounds__(256) void gb_bwd_coldot_kernel(const float* x, const float* g, int64_t n, int f, double* dot) {
  __shared__ double red[4 * 64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.y * 64;
  double s = 0;
  if (col < f)
    for (int64_t r = r0 + rg; r < r0 + 64 && r < n; r += 4) s += (double)x[r * f + col] * g[r * f + col];
  red[rg * 64 + cl] = s;
  __syncthreads();
  if (threadIdx.x < 64 && col < f) unsafeAtomicAdd(dot + col, red[cl] + red[64 + cl] + red[128 + cl] + red[192 + cl]);
}

// backward of x / max(||col||, 1e-12), in place on g = dXn
__global__ __launch_bounds__(256) void gb_bwd_normalize_kernel(const float* x, int64_t n, int f, const double* colsq,
                                                               const double* dot, float* g) {
  const int64_t total = n * f / 4, stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += stride) {
    const int c = (int)(q * 4 % f);
    const float4 xv = reinterpret_cast<const float4*>(x)[q];
    float4 gv = reinterpret_cast<float4*>(g)[q];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    float gs[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float nrm = (float)sqrt(colsq[c + j]);
      gs[j] = nrm > 1e-12f ? fmaf(-xs[j], (float)dot[c + j], gs[j]) / nrm : gs[j] / 1e-12f;
    }
    reinterpret_cast<float4*>(g)[q] = make_float4(gs[0], gs[1], gs[2], gs[3]);
  }
}

static inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

GraphLayout graph_layout(int64_t n, int f) {
  GraphLayout l;
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off = up256(off + b); return o; };
  l.colsq = take((size_t)f * sizeof(double));
  l.row_sq = take((size_t)n * sizeof(float));
  l.row_sum = take((size_t)n * sizeof(float));
  l.G = take((size_t)n * n * sizeof(float));
  l.zeros = take((size_t)n * sizeof(float));
  int sk = 1;
  gemm_plan(n, f, (int)n, &sk);
  l.slab = take(sk > 1 ? (size_t)sk * n * n * sizeof(float) : 0);
  l.total = off;
  return l;
}

int graph_check_args(const char* entry, const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim,
                     const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                     const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                     const float* x_out, const int64_t* edge_index_out, const float* edge_attr_out,
                     const float* edge_labels_out, const void* workspace) {
  using mtmc_api::fail;
  if (!feats || !x_out) return fail(MTMC_E_ARG, "%s: NULL feats or x_out", entry);
  if (n_nodes < 1 || n_nodes > 46000 || feat_dim % 32 != 0 || feat_dim < 32 || n_cams < 1)
    return fail(MTMC_E_ARG, "%s: n_nodes must be in [1, 46000], feat_dim a multiple of 32 and n_cams >= 1", entry);
  if (n_edges > 0 && (!in_list || !in_off || !out_list || !out_off || !block_off || !edge_index_out || !edge_attr_out))
    return fail(MTMC_E_ARG, "%s: NULL camera table or edge output with n_edges > 0", entry);
  if (edge_labels_out && !node_labels) return fail(MTMC_E_ARG, "%s: edge_labels_out needs node_labels", entry);
  if (((uintptr_t)feats & 15) || (feat_row_stride & 3) || ((uintptr_t)x_out & 15) || ((uintptr_t)workspace & 255))
    return fail(MTMC_E_ARG, "%s: feats and x_out must be 16-byte and the workspace 256-byte aligned, the row stride a "
                            "multiple of 4", entry);
  return MTMC_OK;
}

int graph_normalize_gram(const char* entry, const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim,
                         int32_t l2norm, float* x_out, char* ws, const GraphLayout& l, bool gram, hipStream_t s) {
  using mtmc_api::fail;
  double* colsq = reinterpret_cast<double*>(ws + l.colsq);
  float* row_sq = reinterpret_cast<float*>(ws + l.row_sq);
  float* row_sum = reinterpret_cast<float*>(ws + l.row_sum);
  float* zeros = reinterpret_cast<float*>(ws + l.zeros);
  if (hipMemsetAsync(colsq, 0, (size_t)feat_dim * sizeof(double), s) != hipSuccess ||
      hipMemsetAsync(zeros, 0, (size_t)n_nodes * sizeof(float), s) != hipSuccess)
    return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
  if (l2norm)
    hipLaunchKernelGGL(gb_colnorm_kernel, dim3((feat_dim + 63) / 64, (unsigned)((n_nodes + 63) / 64)), dim3(256), 0, s,
                       feats, feat_row_stride, n_nodes, feat_dim, colsq);
  hipLaunchKernelGGL(gb_normalize_kernel, dim3((unsigned)n_nodes), dim3(256), 0, s, feats, feat_row_stride, n_nodes,
                     feat_dim, colsq, l2norm, x_out, row_sq, row_sum);
  if (gram) {
    GemmParams g = plain_gemm(x_out, feat_dim, x_out, zeros, reinterpret_cast<float*>(ws + l.G), n_nodes, n_nodes, feat_dim,
                              (int)n_nodes);
    int sk = 1;
    gemm_plan(n_nodes, feat_dim, (int)n_nodes, &sk);
    if (sk > 1 && l.slab != l.total) g.slab = reinterpret_cast<float*>(ws + l.slab);
    if (launch_gemm_bn(g, s) != MTMC_OK) return fail(MTMC_E_ARG, "%s: the Gram-matrix GEMM refused its shape", entry);
  }
  return MTMC_OK;
}

}  // namespace mtmc

namespace {
using mtmc::up256;
struct GBLayout { size_t colsq, dot, rho, delta, kappa, node_cam, node_loc, S, total; int npad; };
GBLayout graph_bwd_layout(int64_t n, int f) {
  GBLayout l;
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off = up256(off + b); return o; };
  l.npad = (int)((n + 31) / 32 * 32);               // the GEMM's K loop runs in steps of 32 without a tail
  l.colsq = take((size_t)2 * f * sizeof(double));   // colsq | dot: cleared by one memset
  l.dot = l.colsq + (size_t)f * sizeof(double);
  l.rho = take((size_t)n * sizeof(float));
  l.delta = take((size_t)n * sizeof(float));
  l.kappa = take((size_t)n * sizeof(float));
  l.node_cam = take((size_t)n * sizeof(int));
  l.node_loc = take((size_t)n * sizeof(int));
  l.S = take((size_t)n * l.npad * sizeof(float));
  l.total = off;
  return l;
}
}  // namespace

extern "C" {

using mtmc_api::fail;
using mtmc_api::launched;

size_t mtmc_graph_workspace_bytes(int64_t n_nodes, int32_t feat_dim) {
  if (n_nodes < 1 || n_nodes > 46000 || feat_dim < 32) return 0;
  return mtmc::graph_layout(n_nodes, feat_dim).total;
}

int32_t mtmc_build_graph(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                         const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                         const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                         float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  int rc = mtmc::graph_check_args("build_graph", feats, feat_row_stride, n_nodes, feat_dim, in_list, in_off, out_list, out_off,
                                  block_off, n_cams, n_edges, node_labels, x_out, edge_index_out, edge_attr_out,
                                  edge_labels_out, workspace);
  if (rc != MTMC_OK) return rc;
  const mtmc::GraphLayout l = mtmc::graph_layout(n_nodes, feat_dim);
  if (!workspace || workspace_bytes < l.total)
    return fail(MTMC_E_WORKSPACE, "build_graph: workspace has %zu bytes, %zu needed (mtmc_graph_workspace_bytes)",
                workspace ? workspace_bytes : (size_t)0, l.total);
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = mtmc::graph_normalize_gram("build_graph", feats, feat_row_stride, n_nodes, feat_dim, l2norm, x_out, ws, l, n_edges > 0, s);
  if (rc != MTMC_OK) return rc;
  if (n_edges > 0) {
    mtmc::EdgeBuildParams p;
    p.in_list = in_list; p.in_off = in_off; p.out_list = out_list; p.out_off = out_off; p.block_off = block_off;
    p.n_cams = n_cams; p.n_nodes = n_nodes; p.n_edges = n_edges; p.f = feat_dim;
    p.G = reinterpret_cast<float*>(ws + l.G); p.row_sq = reinterpret_cast<float*>(ws + l.row_sq);
    p.row_sum = reinterpret_cast<float*>(ws + l.row_sum); p.node_labels = node_labels;
    p.edge_index = edge_index_out; p.edge_attr = edge_attr_out; p.edge_labels = edge_labels_out;
    hipLaunchKernelGGL(mtmc::gb_edges_kernel, dim3(mtmc::blocks_for(n_edges, 256, 4096)), dim3(256), 0, s, p);
  }
  return launched("build_graph");
}

size_t mtmc_graph_backward_workspace_bytes(int64_t n_nodes, int32_t feat_dim) {
  if (n_nodes < 1 || n_nodes > 46000 || feat_dim < 32 || feat_dim % 32 != 0) return 0;
  return graph_bwd_layout(n_nodes, feat_dim).total;
}

int32_t mtmc_build_graph_backward(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                                  const int32_t* in_list, const int32_t* in_off, const int32_t* out_list,
                                  const int64_t* out_off, const int64_t* block_off, int32_t n_cams, int64_t n_edges,
                                  const float* x, const float* edge_attr, const float* d_x, const float* d_edge_attr,
                                  float* d_feats_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!feats || !x || !d_feats_out) return fail(MTMC_E_ARG, "build_graph_backward: NULL feats, x or d_feats_out");
  if (n_nodes < 1 || n_nodes > 46000 || feat_dim % 32 != 0 || feat_dim < 32 || n_cams < 1 || n_edges < 0)
    return fail(MTMC_E_ARG, "build_graph_backward: n_nodes must be in [1, 46000], feat_dim a multiple of 32, n_cams >= 1 and "
                            "n_edges >= 0");
  if (n_edges > 0 && (!in_list || !in_off || !out_list || !out_off || !block_off || !edge_attr))
    return fail(MTMC_E_ARG, "build_graph_backward: NULL camera table or edge_attr with n_edges > 0");
  if (n_edges > 0 && !d_x && !d_edge_attr) return fail(MTMC_E_ARG, "build_graph_backward: neither d_x nor d_edge_attr is given");
  if (d_x == d_feats_out || x == d_feats_out) return fail(MTMC_E_ARG, "build_graph_backward: d_feats_out must not alias x or d_x");
  if (((uintptr_t)feats & 15) || (feat_row_stride & 3) || ((uintptr_t)x & 15) || ((uintptr_t)d_x & 15) ||
      ((uintptr_t)d_feats_out & 15) || ((uintptr_t)edge_attr & 7) || ((uintptr_t)d_edge_attr & 7) || ((uintptr_t)workspace & 255))
    return fail(MTMC_E_ARG, "build_graph_backward: feats, x, d_x and d_feats_out must be 16-byte, edge_attr and d_edge_attr "
                            "8-byte and the workspace 256-byte aligned, the row stride a multiple of 4");
  const GBLayout l = graph_bwd_layout(n_nodes, feat_dim);
  if (!workspace || workspace_bytes < l.total)
    return fail(MTMC_E_WORKSPACE, "build_graph_backward: workspace has %zu bytes, %zu needed (mtmc_graph_backward_workspace_bytes)",
                workspace ? workspace_bytes : (size_t)0, l.total);
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* colsq = reinterpret_cast<double*>(ws + l.colsq);
  double* dot = reinterpret_cast<double*>(ws + l.dot);
  const size_t nf_bytes = (size_t)n_nodes * feat_dim * sizeof(float);
  if (n_edges > 0 && d_edge_attr) {
    float* rho = reinterpret_cast<float*>(ws + l.rho);
    int* node_cam = reinterpret_cast<int*>(ws + l.node_cam);
    int* node_loc = reinterpret_cast<int*>(ws + l.node_loc);
    mtmc::GraphBwdCoef c;
    c.in_list = in_list; c.in_off = in_off; c.out_list = out_list; c.out_off = out_off; c.block_off = block_off;
    c.n_cams = n_cams; c.n_nodes = n_nodes; c.n_edges = n_edges; c.npad = l.npad;
    c.node_cam = node_cam; c.node_loc = node_loc; c.rho = rho; c.edge_attr = edge_attr; c.d_attr = d_edge_attr;
    c.S = reinterpret_cast<float*>(ws + l.S);
    c.delta = reinterpret_cast<float*>(ws + l.delta); c.kappa = reinterpret_cast<float*>(ws + l.kappa);
    c.X = x; c.out = d_feats_out; c.f = feat_dim;
    if (hipMemsetAsync(c.S, 0, (size_t)n_nodes * l.npad * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(node_cam, 0xFF, (size_t)n_nodes * sizeof(int), s) != hipSuccess)
      return fail(MTMC_E_HIP, "build_graph_backward: hipMemsetAsync failed");
    hipLaunchKernelGGL(mtmc::gb_bwd_nodemap_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, in_list, in_off,
                       n_cams, n_nodes, node_cam, node_loc);
    hipLaunchKernelGGL(mtmc::gb_bwd_rownorm_kernel, dim3((unsigned)n_nodes), dim3(256), 0, s, x, feat_dim, rho);
    hipLaunchKernelGGL(mtmc::gb_bwd_coef_kernel, dim3((unsigned)n_nodes), dim3(256), 0, s, c);
    mtmc::GraphBwdGemm g;
    g.S = c.S; g.npad = l.npad; g.X = x; g.gX = d_x; g.delta = c.delta; g.kappa = c.kappa; g.out = d_feats_out;
    g.n = n_nodes; g.f = feat_dim;
    hipLaunchKernelGGL(mtmc::gb_bwd_gemm_kernel, dim3((feat_dim + 63) / 64, (unsigned)((n_nodes + 63) / 64)), dim3(256), 0, s, g);
    hipLaunchKernelGGL(mtmc::gb_bwd_near_kernel, dim3((unsigned)n_nodes), dim3(256), 0, s, c);
  } else if (d_x) {                                   // no edge gradient: dXn = gX
    if (hipMemcpyAsync(d_feats_out, d_x, nf_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(MTMC_E_HIP, "build_graph_backward: hipMemcpyAsync failed");
  } else {
    if (hipMemsetAsync(d_feats_out, 0, nf_bytes, s) != hipSuccess) return fail(MTMC_E_HIP, "build_graph_backward: hipMemsetAsync failed");
  }
  if (l2norm) {
    if (hipMemsetAsync(colsq, 0, (size_t)2 * feat_dim * sizeof(double), s) != hipSuccess)
      return fail(MTMC_E_HIP, "build_graph_backward: hipMemsetAsync failed");
    const dim3 col_grid((feat_dim + 63) / 64, (unsigned)((n_nodes + 63) / 64));
    hipLaunchKernelGGL(mtmc::gb_colnorm_kernel, col_grid, dim3(256), 0, s, feats, feat_row_stride, n_nodes, feat_dim, colsq);
    hipLaunchKernelGGL(mtmc::gb_bwd_coldot_kernel, col_grid, dim3(256), 0, s, x, d_feats_out, n_nodes, feat_dim, dot);
    hipLaunchKernelGGL(mtmc::gb_bwd_normalize_kernel, dim3(mtmc::blocks_for((int64_t)n_nodes * feat_dim / 4, 256, 4096)),
                       dim3(256), 0, s, x, n_nodes, feat_dim, colsq, dot, d_feats_out);
  }
  return launched("build_graph_backward");
}

}  // extern "C"
