// Backward of the tracklet-graph construction (graph_build.hip), mtmc_build_graph_backward: d(x, edge_attr)
// -> d feats without any per-edge 2048-d gather.  The table walks, the workgroup sum and the column sums are graph_build.h's.
// With a_e = gD_e / d_e (0 where d_e == 0), b_e = -gC_e, s_e = cos_e = 1 - edge_attr[e][1], rho_i = |x_i|:
//     S[i][j] = m_ij + m_ji,  m_e = -a_e + b_e / (rho_r rho_c)                       (0 where (i, j) is no edge)
//     delta_i = sum over edges that start or end at i of (a_e - b_e s_e / rho_i^2),   kappa_i = sum_{row=i} a_e - sum_{col=i} a_e
//     dXn     = gX + S . Xn + diag(delta) . Xn + 1e-6 kappa 1^T
//     dX[:,k] = (dXn[:,k] - Xn[:,k] <Xn[:,k], dXn[:,k]>) / n_k                        (l2norm; dX = dXn otherwise)
// The eps clamps of the forward (1e-8 on rho, 1e-12 on n_k) count as constants where they are active, as in autograd.
#include "graph_build.h"

namespace mtmc {

// node -> (camera block, position inside it): the inverse of in_list
__global__ __launch_bounds__(256) void gb_bwd_nodemap_kernel(const int* in_list, const int* in_off, int n_cams, int64_t n,
                                                             int* node_cam, int* node_loc) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int k = gb_segment_of(in_off, n_cams, q);
  const int node = in_list[q];
  if (node >= 0 && node < n) { node_cam[node] = k; node_loc[node] = (int)(q - in_off[k]); }
}

int graph_node_map(const GraphTables& t, int* node_cam, int* node_loc, hipStream_t s) {
  if (hipMemsetAsync(node_cam, 0xFF, (size_t)t.n_nodes * sizeof(int), s) != hipSuccess) return MTMC_E_HIP;
  hipLaunchKernelGGL(gb_bwd_nodemap_kernel, dim3((unsigned)((t.n_nodes + 255) / 256)), dim3(256), 0, s, t.in_list, t.in_off,
                     t.n_cams, t.n_nodes, node_cam, node_loc);
  return MTMC_OK;
}

// rho_i = |x_i| exactly as the forward formed it: fp64 sum of squares -> f32 -> sqrtf
__global__ __launch_bounds__(256) void gb_bwd_rownorm_kernel(const float* x, int f, float* rho) {
  __shared__ double red[4];
  const int64_t r = blockIdx.x;
  double sq[1] = {0};
  for (int c = threadIdx.x; c < f; c += 256) { const double v = x[r * f + c]; sq[0] += v * v; }
  block_sum(sq, red);
  if (threadIdx.x == 0) rho[r] = sqrtf((float)sq[0]);
}

struct GraphBwdCoef {
  GraphTables t; int npad;
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
  if (ci < 0 || ci >= p.t.n_cams) {                 // node missing from in_list: no edges
    if (threadIdx.x == 0) { p.delta[i] = 0.f; p.kappa[i] = 0.f; }
    return;
  }
  const float rho_i = p.rho[i], r_i = fmaxf(rho_i, 1e-8f);
  const float inv_rho2 = rho_i > 1e-8f ? 1.f / (rho_i * rho_i) : 0.f;
  float* s_row = p.S + (int64_t)i * p.npad;
  const float2* attr = reinterpret_cast<const float2*>(p.edge_attr);
  const float2* grad = reinterpret_cast<const float2*>(p.d_attr);
  double sums[2] = {0, 0};                          // delta_i, kappa_i
  auto coef = [&](int64_t e, int j, float sign) {
    const float2 at = attr[e], g = grad[e];
    const float a = (at.x > 0.f && !gb_near(at.x, rho_i, p.rho[j])) ? g.x / at.x : 0.f, b = -g.y, s = 1.f - at.y;
    sums[0] += a - b * s * inv_rho2;
    sums[1] += sign * a;
    return b / (r_i * fmaxf(p.rho[j], 1e-8f)) - a;
  };
  {
    const int64_t n_out = p.t.out_off[ci + 1] - p.t.out_off[ci];
    const int64_t e0 = p.t.block_off[ci] + p.node_loc[i] * n_out;
    const int* ol = p.t.out_list + p.t.out_off[ci];
    for (int64_t t = threadIdx.x; t < n_out; t += 256) {
      const int j = ol[t];
      if (e0 + t >= p.t.n_edges || j < 0 || j >= p.t.n_nodes) continue;
      s_row[j] = coef(e0 + t, j, 1.f);
    }
  }
  __threadfence();
  __syncthreads();
  for (int64_t q = threadIdx.x; q < p.t.n_nodes; q += 256) {
    int j;
    const int64_t e = gb_edge_into(p.t, q, i, ci, &j);
    if (e < 0 || j < 0 || j >= p.t.n_nodes) continue;
    unsafeAtomicAdd(s_row + j, coef(e, j, -1.f));
  }
  block_sum(sums, red);
  if (threadIdx.x == 0) { p.delta[i] = (float)sums[0]; p.kappa[i] = (float)sums[1]; }
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
  if (ci < 0 || ci >= p.t.n_cams) return;
  const float rho_i = p.rho[i];
  const float2* attr = reinterpret_cast<const float2*>(p.edge_attr);
  const float2* grad = reinterpret_cast<const float2*>(p.d_attr);
  const int64_t n_out_i = p.t.out_off[ci + 1] - p.t.out_off[ci];
  const int64_t e0 = p.t.block_off[ci] + p.node_loc[i] * n_out_i;
  const float* xi = p.X + (int64_t)i * p.f;
  float* oi = p.out + (int64_t)i * p.f;
  for (int64_t base = 0; base < n_out_i + p.t.n_nodes; base += 256) {
    const int64_t cand = base + threadIdx.x;
    int64_t e = -1;
    int j = -1;
    float sign = 1.f;
    if (cand < n_out_i) {
      j = p.t.out_list[p.t.out_off[ci] + cand];
      e = e0 + cand;
    } else if (cand < n_out_i + p.t.n_nodes) {
      e = gb_edge_into(p.t, cand - n_out_i, i, ci, &j);
      sign = -1.f;
    }
    bool flagged = false;
    if (e >= 0 && e < p.t.n_edges && j >= 0 && j < p.t.n_nodes) {
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
        double d2[1] = {0};
        for (int c = threadIdx.x; c < p.f; c += 256) { const float v = sgn * (xi[c] - xj[c]) + 1e-6f; d2[0] += (double)v * v; }
        block_sum(d2, red);
        __syncthreads();                 // red is written again for the next flagged edge
        const float a = d2[0] > 0 ? sgn * gd / (float)sqrt(d2[0]) : 0.f;
        for (int c = threadIdx.x; c < p.f; c += 256) oi[c] = fmaf(a, sgn * (xi[c] - xj[c]) + 1e-6f, oi[c]);
      }
    }
    __syncthreads();
  }
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

}  // namespace mtmc

namespace {
using mtmc_api::fail;

struct GBLayout { size_t colsq, dot, rho, delta, kappa, node_cam, node_loc, S, total; int npad; };
GBLayout graph_bwd_layout(int64_t n, int f) {
  GBLayout l;
  mtmc::Carver ws;
  l.npad = (int)((n + 31) / 32 * 32);               // the GEMM's K loop runs in steps of 32 without a tail
  l.colsq = ws.take((size_t)2 * f * sizeof(double));   // colsq | dot: cleared by one memset
  l.dot = l.colsq + (size_t)f * sizeof(double);
  l.rho = ws.take((size_t)n * sizeof(float));
  l.delta = ws.take((size_t)n * sizeof(float));
  l.kappa = ws.take((size_t)n * sizeof(float));
  l.node_cam = ws.take((size_t)n * sizeof(int));
  l.node_loc = ws.take((size_t)n * sizeof(int));
  l.S = ws.take((size_t)n * l.npad * sizeof(float));
  l.total = ws.off;
  return l;
}
}  // namespace

extern "C" {

size_t mtmc_graph_backward_workspace_bytes(int64_t n_nodes, int32_t feat_dim) {
  return mtmc::graph_size_ok(n_nodes, feat_dim) && feat_dim % 32 == 0 ? graph_bwd_layout(n_nodes, feat_dim).total : 0;
}

int32_t mtmc_build_graph_backward(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                                  const int32_t* in_list, const int32_t* in_off, const int32_t* out_list,
                                  const int64_t* out_off, const int64_t* block_off, int32_t n_cams, int64_t n_edges,
                                  const float* x, const float* edge_attr, const float* d_x, const float* d_edge_attr,
                                  float* d_feats_out, void* workspace, size_t workspace_bytes, void* stream) {
  const mtmc::GraphTables t = {in_list, in_off, out_list, out_off, block_off, n_cams, n_nodes, n_edges};
  if (!feats || !x || !d_feats_out) return fail(MTMC_E_ARG, "build_graph_backward: NULL feats, x or d_feats_out");
  if (!mtmc::graph_dims_ok(t, feat_dim) || n_edges < 0)
    return fail(MTMC_E_ARG, "build_graph_backward: n_nodes must be in [1, 46000], feat_dim a multiple of 32, n_cams >= 1 and "
                            "n_edges >= 0");
  if (n_edges > 0 && (!mtmc::graph_tables_given(t) || !edge_attr))
    return fail(MTMC_E_ARG, "build_graph_backward: NULL camera table or edge_attr with n_edges > 0");
  if (n_edges > 0 && !d_x && !d_edge_attr) return fail(MTMC_E_ARG, "build_graph_backward: neither d_x nor d_edge_attr is given");
  if (d_x == d_feats_out || x == d_feats_out) return fail(MTMC_E_ARG, "build_graph_backward: d_feats_out must not alias x or d_x");
  if (((uintptr_t)feats & 15) || (feat_row_stride & 3) || ((uintptr_t)x & 15) || ((uintptr_t)d_x & 15) ||
      ((uintptr_t)d_feats_out & 15) || ((uintptr_t)edge_attr & 7) || ((uintptr_t)d_edge_attr & 7) || ((uintptr_t)workspace & 255))
    return fail(MTMC_E_ARG, "build_graph_backward: feats, x, d_x and d_feats_out must be 16-byte, edge_attr and d_edge_attr "
                            "8-byte and the workspace 256-byte aligned, the row stride a multiple of 4");
  const GBLayout l = graph_bwd_layout(n_nodes, feat_dim);
  if (int rc = mtmc::graph_check_workspace("build_graph_backward", workspace, workspace_bytes, l.total,
                                           "mtmc_graph_backward_workspace_bytes")) return rc;
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double *colsq = reinterpret_cast<double*>(ws + l.colsq), *dot = reinterpret_cast<double*>(ws + l.dot);
  const size_t nf_bytes = (size_t)n_nodes * feat_dim * sizeof(float);
  if (n_edges > 0 && d_edge_attr) {
    float* rho = reinterpret_cast<float*>(ws + l.rho);
    int* node_cam = reinterpret_cast<int*>(ws + l.node_cam);
    int* node_loc = reinterpret_cast<int*>(ws + l.node_loc);
    mtmc::GraphBwdCoef c;
    c.t = t; c.npad = l.npad;
    c.node_cam = node_cam; c.node_loc = node_loc; c.rho = rho; c.edge_attr = edge_attr; c.d_attr = d_edge_attr;
    c.S = reinterpret_cast<float*>(ws + l.S);
    c.delta = reinterpret_cast<float*>(ws + l.delta); c.kappa = reinterpret_cast<float*>(ws + l.kappa);
    c.X = x; c.out = d_feats_out; c.f = feat_dim;
    if (hipMemsetAsync(c.S, 0, (size_t)n_nodes * l.npad * sizeof(float), s) != hipSuccess ||
        mtmc::graph_node_map(t, node_cam, node_loc, s) != MTMC_OK)
      return fail(MTMC_E_HIP, "build_graph_backward: hipMemsetAsync failed");
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
    mtmc::graph_column_sums(feats, feat_row_stride, nullptr, n_nodes, feat_dim, colsq, s);
    mtmc::graph_column_sums(x, feat_dim, d_feats_out, n_nodes, feat_dim, dot, s);
    hipLaunchKernelGGL(mtmc::gb_bwd_normalize_kernel, dim3(mtmc::blocks_for((int64_t)n_nodes * feat_dim / 4, 256, 4096)),
                       dim3(256), 0, s, x, n_nodes, feat_dim, colsq, dot, d_feats_out);
  }
  return mtmc_api::launched("build_graph_backward");
}

}  // extern "C"
