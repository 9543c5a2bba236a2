// What graph_build.hip (normalise -> Gram, the reference's all-pairs list), graph_knn.hip (its thinning by a temporal gate
// and / or to a symmetric k-nearest list) and graph_backward.hip share: the description of a call, the walks of the camera
// tables, the edge-attribute expression and the stores of one edge, the workgroup sum and the workspace carving.  One copy
// of each, so an edge every builder emits carries the same bits and every kernel finds it at the same place.
#pragma once
#include "api_internal.h"

namespace mtmc {

// The camera tables: the dense list is, camera by camera, (every node of in_list) x (every node of out_list)
struct GraphTables {
  const int* in_list; const int* in_off;        // nodes of camera c: in_list[in_off[c] .. in_off[c+1])
  const int* out_list; const int64_t* out_off;  // nodes NOT in camera c, ascending
  const int64_t* block_off;                     // first edge of camera c's block; block_off[n_cams] = E
  int n_cams; int64_t n_nodes; int64_t n_edges;
};

template <class T>
__device__ __forceinline__ int gb_segment_of(const T* off, int n_seg, int64_t v) {   // off[s] <= v < off[s + 1]
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)off[mid] <= v) lo = mid; else hi = mid; }
  return lo;
}

struct GbRow { int i; const int* ol; int n_out; int64_t e0; };   // node, its camera's out_list, its first dense edge

// row of in_list position q; false where in_list names no node (such a row has no edges in any of the kernels)
__device__ __forceinline__ bool gb_row_of(const GraphTables& t, int64_t q, GbRow* r) {
  const int c = gb_segment_of(t.in_off, t.n_cams, q);
  const int64_t n_out = t.out_off[c + 1] - t.out_off[c];
  r->i = t.in_list[q];
  r->ol = t.out_list + t.out_off[c];
  r->n_out = (int)n_out;
  r->e0 = t.block_off[c] + (q - t.in_off[c]) * n_out;
  return r->i >= 0 && r->i < t.n_nodes;
}

// (row, col) of dense edge e < n_edges
__device__ __forceinline__ void gb_edge_ends(const GraphTables& t, int64_t e, int* row, int* col) {
  const int c = gb_segment_of(t.block_off, t.n_cams, e);
  const int64_t local = e - t.block_off[c];
  const int64_t n_out = t.out_off[c + 1] - t.out_off[c];
  *row = t.in_list[t.in_off[c] + (int)(local / n_out)];
  *col = t.out_list[t.out_off[c] + local % n_out];
}

// rank of node i in the ascending list ol[0 .. n_out); -1 where it is not in it
__device__ __forceinline__ int64_t gb_rank_in(const int* ol, int64_t n_out, int i) {
  int64_t lo = 0, hi = n_out;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (ol[mid] < i) lo = mid + 1; else hi = mid; }
  return lo < n_out && ol[lo] == i ? lo : -1;
}

// dense position of the edge from in_list position q into node i of camera ci: block_off[k] + pos(q) * n_out(k) + rank of i
// in camera k's ascending out_list; -1 where q is of camera ci itself or the tables hold no such edge.  *j = the node at q.
__device__ __forceinline__ int64_t gb_edge_into(const GraphTables& t, int64_t q, int i, int ci, int* j) {
  const int k = gb_segment_of(t.in_off, t.n_cams, q);
  *j = t.in_list[q];
  if (k == ci) return -1;
  const int64_t n_out = t.out_off[k + 1] - t.out_off[k];
  const int64_t lo = gb_rank_in(t.out_list + t.out_off[k], n_out, i);
  if (lo < 0) return -1;
  const int64_t e = t.block_off[k] + (q - t.in_off[k]) * n_out + lo;
  return e < t.n_edges ? e : -1;
}

// edge_attr[e] = [ ||x_r - x_c + 1e-6||_2 , 1 - cos(x_r, x_c) ] from the Gram entry g = x_r . x_c, nr = |x_r|^2, nc = |x_c|^2,
// sr = sum x_r, sc = sum x_c (graph_build.hip's header comment has the algebra)
__device__ __forceinline__ float2 gb_edge_attr(float g, float nr, float nc, float sr, float sc, int f) {
  const float eps = 1e-6f;                     // F.pairwise_distance eps
  const float d2 = nr + nc - 2.f * g + 2.f * eps * (sr - sc) + (float)f * eps * eps;
  const float dist = sqrtf(fmaxf(d2, 0.f));
  const float cosv = g / (fmaxf(sqrtf(nr), 1e-8f) * fmaxf(sqrtf(nc), 1e-8f));   // F.cosine_similarity eps
  return make_float2(dist, 1.f - cosv);
}

struct EdgeBuildParams {
  GraphTables t; int f;
  const float* G; const float* row_sq; const float* row_sum; const int64_t* node_labels;
  int64_t g_row0 = 0;                           // G holds the Gram rows of the nodes from g_row0 on: [rows][N] (a row panel)
  int64_t* edge_index;                          // [E][2] (row, col): its .T is the [2,E] view the callers pass on
  float* edge_attr; float* edge_labels;
};

__device__ __forceinline__ float2 gb_edge_attr_of(const EdgeBuildParams& p, int i, int j) {
  return gb_edge_attr(p.G[(i - p.g_row0) * p.t.n_nodes + j], p.row_sq[i], p.row_sq[j], p.row_sum[i], p.row_sum[j], p.f);
}

// edge (row, col) into output slot `slot`: index pair, attributes, label.  (A thinned list's edge_pos is its caller's.)
__device__ __forceinline__ void gb_write_edge(const EdgeBuildParams& p, int64_t slot, int row, int col) {
  reinterpret_cast<longlong2*>(p.edge_index)[slot] = make_longlong2(row, col);
  reinterpret_cast<float2*>(p.edge_attr)[slot] = gb_edge_attr_of(p, row, col);
  if (p.edge_labels) p.edge_labels[slot] = p.node_labels[row] == p.node_labels[col] ? 1.f : 0.f;
}

// v[j] = the sum of v[j] over the 256 threads of the workgroup, in every thread: wave_sum, then the four wave totals in
// wave order.  red: 4 NV doubles of LDS; every thread must call, and a caller that sums again puts a barrier in between.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = wave_sum(v[j]);
  if ((threadIdx.x & 63) == kWaveSumLane) {
#pragma unroll
    for (int j = 0; j < NV; ++j) red[4 * j + (threadIdx.x >> 6)] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = red[4 * j] + red[4 * j + 1] + red[4 * j + 2] + red[4 * j + 3];
}

// out[c] += sum over the rows of x[r][c]^2 (g == null) or of x[r][c] g[r][c] (g: [n][f]), in fp64; out is zero on entry
void graph_column_sums(const float* x, int64_t ld, const float* g, int64_t n, int f, double* out, hipStream_t s);
// node -> (camera block, position inside it), the inverse of in_list; a node that in_list does not name keeps node_cam < 0
int graph_node_map(const GraphTables& t, int* node_cam, int* node_loc, hipStream_t s);

struct GraphCall {                              // one call of a forward entry, as the host sees it
  GraphTables t;
  const float* feats; int64_t feat_row_stride; int feat_dim; int l2norm;
  const int64_t* node_labels;
  float* x_out; int64_t* edge_index_out; float* edge_attr_out; float* edge_labels_out;
  void* workspace; size_t workspace_bytes; hipStream_t stream;
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(workspace) + off); }
};

// The sizes every entry accepts.  The workspace queries of the forward entries answer for any feat_dim >= 32 (the calls
// themselves then refuse one that is no multiple of 32: graph_dims_ok); the backward's query wants the multiple as well.
// max_nodes: 46000 where G is formed whole (N^2 x 4 bytes), 262144 where it is formed in row panels (graph_knn.hip).
constexpr int64_t kGraphMaxNodes = 46000, kGraphMaxNodesPaneled = 262144;
inline bool graph_size_ok(int64_t n, int f, int64_t max_nodes = kGraphMaxNodes) { return n >= 1 && n <= max_nodes && f >= 32; }
inline bool graph_dims_ok(const GraphTables& t, int f, int64_t max_nodes = kGraphMaxNodes) {
  return graph_size_ok(t.n_nodes, f, max_nodes) && f % 32 == 0 && t.n_cams >= 1;
}
inline bool graph_tables_given(const GraphTables& t) { return t.in_list && t.in_off && t.out_list && t.out_off && t.block_off; }

// workspace carving: every region starts 256-byte aligned
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off = mtmc_api::align_up(off + bytes); return o; }
};

// G and the split-K slab hold g_rows Gram rows: all N, or a row panel
struct GraphLayout { size_t colsq, row_sq, row_sum, G, zeros, slab, total; };
GraphLayout graph_layout(int64_t n, int f, int64_t g_rows);
inline GraphLayout graph_layout(int64_t n, int f) { return graph_layout(n, f, n); }

// what the forward entries refuse alike; `entry` heads the message.  MTMC_OK or the failure's code.
int graph_check_args(const char* entry, const GraphCall& c, int64_t max_nodes = kGraphMaxNodes);
// the call's workspace holds `need` bytes, the answer of `query`
inline int graph_check_workspace(const char* entry, const void* workspace, size_t have, size_t need, const char* query) {
  if (workspace && have >= need) return MTMC_OK;
  return mtmc_api::fail(MTMC_E_WORKSPACE, "%s: workspace has %zu bytes, %zu needed (%s)", entry, workspace ? have : (size_t)0,
                        need, query);
}

// x_out = the (column-normalised) features, row_sq / row_sum of its rows, in the workspace laid out by `l`
int graph_normalize(const char* entry, const GraphCall& c, const GraphLayout& l);
// G = x_out[row0 .. row0 + rows) x_out^T, [rows][N] at l.G.  Planned as the whole product is (GemmParams::plan_rows = N):
// same kernel, BK and split, so an element of G has the same bits whichever panel forms it.
int graph_gram(const char* entry, const GraphCall& c, const GraphLayout& l, int64_t row0, int64_t rows);
// both, G whole and only where the call has edges.  MTMC_OK or the failure's code.
inline int graph_normalize_gram(const char* entry, const GraphCall& c, const GraphLayout& l) {
  if (int rc = graph_normalize(entry, c, l)) return rc;
  return c.t.n_edges > 0 ? graph_gram(entry, c, l, 0, c.t.n_nodes) : MTMC_OK;
}

// the device-side view of the call's tables, Gram matrix and edge outputs
EdgeBuildParams edge_build_params(const GraphCall& c, const GraphLayout& l);

}  // namespace mtmc
