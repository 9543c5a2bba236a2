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
// A row panel of G (graph_gram with fewer than N rows) is planned by N all the same, so its elements carry the same bits.
// tests/gram_cases.py names a case for each line and tests/test_gram_cases.py pins the splits.
// Here: the normalise -> Gram sequence, argument checks and workspace layout of every builder, and the dense builder itself.
// graph_knn.hip thins its list, graph_backward.hip differentiates it; graph_build.h holds what the three share.
#include "graph_build.h"

namespace mtmc {

// column sums over the nodes (fp64) of x^2 (kDot = false) or x g: block = 64 columns x 64 rows, one atomic per column
template <bool kDot>
__global__ __launch_bounds__(256) void gb_colsum_kernel(const float* x, int64_t ld, const float* g, int64_t n, int f, double* out) {
  __shared__ double red[4 * 64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.y * 64;
  double s = 0;
  if (col < f)
    for (int64_t r = r0 + rg; r < r0 + 64 && r < n; r += 4) {
      const double v = x[r * ld + col];
      s += v * (kDot ? (double)g[r * f + col] : v);
    }
  red[rg * 64 + cl] = s;
  __syncthreads();
  if (threadIdx.x < 64 && col < f) unsafeAtomicAdd(out + col, red[cl] + red[64 + cl] + red[128 + cl] + red[192 + cl]);
}

void graph_column_sums(const float* x, int64_t ld, const float* g, int64_t n, int f, double* out, hipStream_t s) {
  const dim3 grid((f + 63) / 64, (unsigned)((n + 63) / 64));
  if (g) hipLaunchKernelGGL(gb_colsum_kernel<true>, grid, dim3(256), 0, s, x, ld, g, n, f, out);
  else hipLaunchKernelGGL(gb_colsum_kernel<false>, grid, dim3(256), 0, s, x, ld, g, n, f, out);
}

// x_out = x / max(||col||, 1e-12) (or a copy); per node |x|^2 and sum x of the normalised row (fp64 -> f32)
__global__ __launch_bounds__(256) void gb_normalize_kernel(const float* x, int64_t ld, int64_t n, int f,
                                                           const double* colsq, int l2norm, float* x_out,
                                                           float* row_sq, float* row_sum) {
  __shared__ double red[2 * 4];
  const int64_t r = blockIdx.x;
  double sums[2] = {0, 0};                         // |x|^2, sum x
  for (int c = threadIdx.x; c < f; c += 256) {
    float v = x[r * ld + c];
    if (l2norm) {
      const float nrm = (float)sqrt(colsq[c]);
      v = v / fmaxf(nrm, 1e-12f);
    }
    x_out[r * f + c] = v;
    sums[0] += (double)v * v;
    sums[1] += v;
  }
  block_sum(sums, red);
  if (threadIdx.x == 0) { row_sq[r] = (float)sums[0]; row_sum[r] = (float)sums[1]; }
}

__global__ __launch_bounds__(256) void gb_edges_kernel(EdgeBuildParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < p.t.n_edges; e += stride) {
    int row, col;
    gb_edge_ends(p.t, e, &row, &col);
    gb_write_edge(p, e, row, col);
  }
}

GraphLayout graph_layout(int64_t n, int f, int64_t g_rows) {
  GraphLayout l;
  Carver ws;
  l.colsq = ws.take((size_t)f * sizeof(double));
  l.row_sq = ws.take((size_t)n * sizeof(float));
  l.row_sum = ws.take((size_t)n * sizeof(float));
  l.G = ws.take((size_t)g_rows * n * sizeof(float));
  l.zeros = ws.take((size_t)n * sizeof(float));
  int sk = 1;
  gemm_plan(n, f, (int)n, &sk);
  l.slab = ws.take(sk > 1 ? (size_t)sk * g_rows * n * sizeof(float) : 0);
  l.total = ws.off;
  return l;
}

int graph_check_args(const char* entry, const GraphCall& c, int64_t max_nodes) {
  using mtmc_api::fail;
  if (!c.feats || !c.x_out) return fail(MTMC_E_ARG, "%s: NULL feats or x_out", entry);
  if (!graph_dims_ok(c.t, c.feat_dim, max_nodes))
    return fail(MTMC_E_ARG, "%s: n_nodes must be in [1, %lld], feat_dim a multiple of 32 and n_cams >= 1", entry, (long long)max_nodes);
  if (c.t.n_edges > 0 && (!graph_tables_given(c.t) || !c.edge_index_out || !c.edge_attr_out))
    return fail(MTMC_E_ARG, "%s: NULL camera table or edge output with n_edges > 0", entry);
  if (c.edge_labels_out && !c.node_labels) return fail(MTMC_E_ARG, "%s: edge_labels_out needs node_labels", entry);
  if (((uintptr_t)c.feats & 15) || (c.feat_row_stride & 3) || ((uintptr_t)c.x_out & 15) || ((uintptr_t)c.workspace & 255))
    return fail(MTMC_E_ARG, "%s: feats and x_out must be 16-byte and the workspace 256-byte aligned, the row stride a "
                            "multiple of 4", entry);
  return MTMC_OK;
}

int graph_normalize(const char* entry, const GraphCall& c, const GraphLayout& l) {
  using mtmc_api::fail;
  const int64_t n = c.t.n_nodes;
  double* colsq = c.at<double>(l.colsq);
  float* zeros = c.at<float>(l.zeros);
  hipStream_t s = c.stream;
  if (hipMemsetAsync(colsq, 0, (size_t)c.feat_dim * sizeof(double), s) != hipSuccess ||
      hipMemsetAsync(zeros, 0, (size_t)n * sizeof(float), s) != hipSuccess)
    return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
  if (c.l2norm) graph_column_sums(c.feats, c.feat_row_stride, nullptr, n, c.feat_dim, colsq, s);
  hipLaunchKernelGGL(gb_normalize_kernel, dim3((unsigned)n), dim3(256), 0, s, c.feats, c.feat_row_stride, n, c.feat_dim, colsq,
                     c.l2norm, c.x_out, c.at<float>(l.row_sq), c.at<float>(l.row_sum));
  return MTMC_OK;
}

int graph_gram(const char* entry, const GraphCall& c, const GraphLayout& l, int64_t row0, int64_t rows) {
  const int64_t n = c.t.n_nodes;
  GemmParams g = plain_gemm(c.x_out + row0 * c.feat_dim, c.feat_dim, c.x_out, c.at<float>(l.zeros), c.at<float>(l.G), n, rows,
                            c.feat_dim, (int)n);
  g.plan_rows = n;
  int sk = 1;
  gemm_plan(n, c.feat_dim, (int)n, &sk);
  if (sk > 1) g.slab = c.at<float>(l.slab);
  if (launch_gemm_bn(g, c.stream) != MTMC_OK)
    return mtmc_api::fail(MTMC_E_ARG, "%s: the Gram-matrix GEMM refused its shape", entry);
  return MTMC_OK;
}

EdgeBuildParams edge_build_params(const GraphCall& c, const GraphLayout& l) {
  EdgeBuildParams p;
  p.t = c.t; p.f = c.feat_dim;
  p.G = c.at<float>(l.G); p.row_sq = c.at<float>(l.row_sq); p.row_sum = c.at<float>(l.row_sum); p.node_labels = c.node_labels;
  p.edge_index = c.edge_index_out; p.edge_attr = c.edge_attr_out; p.edge_labels = c.edge_labels_out;
  return p;
}

}  // namespace mtmc

extern "C" {

size_t mtmc_graph_workspace_bytes(int64_t n_nodes, int32_t feat_dim) {
  return mtmc::graph_size_ok(n_nodes, feat_dim) ? mtmc::graph_layout(n_nodes, feat_dim).total : 0;
}

int32_t mtmc_build_graph(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                         const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                         const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                         float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  const mtmc::GraphCall c = {{in_list, in_off, out_list, out_off, block_off, n_cams, n_nodes, n_edges},
                             feats, feat_row_stride, feat_dim, l2norm, node_labels, x_out, edge_index_out, edge_attr_out,
                             edge_labels_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
  if (int rc = mtmc::graph_check_args("build_graph", c)) return rc;
  const mtmc::GraphLayout l = mtmc::graph_layout(n_nodes, feat_dim);
  if (int rc = mtmc::graph_check_workspace("build_graph", workspace, workspace_bytes, l.total, "mtmc_graph_workspace_bytes")) return rc;
  if (int rc = mtmc::graph_normalize_gram("build_graph", c, l)) return rc;
  if (n_edges > 0)
    hipLaunchKernelGGL(mtmc::gb_edges_kernel, dim3(mtmc::blocks_for(n_edges, 256, 4096)), dim3(256), 0, c.stream,
                       mtmc::edge_build_params(c, l));
  return mtmc_api::launched("build_graph");
}

}  // extern "C"
