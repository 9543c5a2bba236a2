// build_graph(k=..., start_frames=..., max_gap=...): the cross-camera list of graph_build.hip thinned by a temporal gate, to
// a symmetric k-nearest list, or both (the reference's authors left both ideas as one commented-out
// block, inference.py:415-441).
//     cand(i, j) = j is in another camera than i, and |start_i - start_j| < max_gap where a gate is given (:420-441)
//     key(i, j)  = the cosine distance edge_attr[e][1] that the dense builder writes for the directed edge (i, j)
//     top_i      = the first min(k, n_cand(i)) candidates j of row i in the order (key, j) ascending
//     keep (i,j) iff j in top_i or i in top_j            -- a union: symmetric whether or not G[i][j] == G[j][i] bitwise
//     k == 0     : keep (i, j) iff cand(i, j); no selection and no bit matrix
// Kept edges appear in the dense list's order with the dense list's bits (gb_write_edge, graph_build.h) and carry their dense
// position in edge_pos.  Only G and an N x N BIT matrix are N^2-sized; the dense edge arrays are never formed.
//     gk_select_kernel   one workgroup per row: radix select of the k-th (key, j), then bit (i, j) and bit (j, i) per pick
//     gk_count_kernel    one workgroup per row: kept columns of its out_list
//     gk_scan_kernel     exclusive int64 scan of the counts in in_list position order (= the dense list's row order)
//     gk_fill_kernel     one workgroup per row: ordered compaction of its kept columns at its row offset
// No atomics on any output cursor and the ORs commute, so two calls on the same G give the same bits.
#include "graph_build.h"

namespace mtmc {

struct KnnParams {
  EdgeBuildParams e;          // camera tables, G, row norms, labels; the edge outputs hold `capacity` edges
  int k; int64_t capacity;    // k == 0: the gate alone, `bits` is not touched
  const int64_t* start;       // [N] first frame of every tracklet; null: no gate
  int64_t max_gap;            // cand(i, j) needs |start[i] - start[j]| < max_gap
  unsigned* bits;             // bit i * N + j: edge (i, j) is kept
  int64_t* row_off;           // [N] by in_list position: kept edges of the row, then (scanned in place) its first output slot
  int64_t* edge_pos;          // [capacity]: dense position of every kept edge
};

// the temporal gate of the node pair (i, j); symmetric in i and j
__device__ __forceinline__ bool knn_gate(const KnnParams& p, int i, int j) {
  if (!p.start) return true;
  const int64_t a = p.start[i], b = p.start[j];
  return (a > b ? (uint64_t)a - (uint64_t)b : (uint64_t)b - (uint64_t)a) < (uint64_t)p.max_gap;   // no overflow at any starts
}

// order-preserving uint32 image of key(i, j); false where j is no candidate: no node, or outside the gate
__device__ __forceinline__ bool knn_key(const KnnParams& kp, int i, int j, uint32_t* u) {
  if (j < 0 || j >= kp.e.t.n_nodes || !knn_gate(kp, i, j)) return false;
  const uint32_t b = __float_as_uint(gb_edge_attr_of(kp.e, i, j).y);
  *u = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  return true;
}

__device__ __forceinline__ void knn_set(unsigned* bits, int64_t n, int i, int j) {
  const int64_t b = (int64_t)i * n + j;
  atomicOr(bits + (b >> 5), 1u << (b & 31));
}
__device__ __forceinline__ bool knn_get(const unsigned* bits, int64_t n, int i, int j) {
  const int64_t b = (int64_t)i * n + j;
  return (bits[b >> 5] >> (b & 31)) & 1u;
}
// edge (i, j) is in the result: its bit where rows selected (the gate is symmetric, so only candidates have bits), the
// candidate test itself where the gate stands alone.  p.k is uniform over the grid.
__device__ __forceinline__ bool knn_kept(const KnnParams& p, int i, int j) {
  if (j < 0 || j >= p.e.t.n_nodes) return false;
  return p.k ? knn_get(p.bits, p.e.t.n_nodes, i, j) : knn_gate(p, i, j);
}

// exclusive prefix of v over the 256 threads of the workgroup in thread order, *total = the sum; smem: 4 ints.
// Every thread must call.
__device__ __forceinline__ int block_excl_scan(int v, int* smem, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
  __syncthreads();                                // the previous call's readers are done with smem
  if (lane == 63) smem[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) { const int s = smem[x]; if (x < w) base += s; tot += s; }
  *total = tot;
  return base + inc - v;
}

// Radix select over the key images, most significant byte first: after pass b, `prefix` holds the top 8 (b + 1) bits of the
// k-th smallest image and `want` its rank among the keys that share them.  The row is read again on every pass (184 KB at
// the most: it stays in L2).  After four passes `want` of the keys equal to the k-th are admitted with every smaller one;
// out_list ascends, so a prefix count in sweep order admits the lowest columns first.  Only candidates have a key
// (knn_key): with a gate the row ranks what passes it, want = min(k, candidates), and a row without any sets no bit.
__global__ __launch_bounds__(256) void gk_select_kernel(KnnParams p) {
  __shared__ int hist[256];
  __shared__ int scan_s[4];
  __shared__ int pick[2];
  GbRow r;
  if (!gb_row_of(p.e.t, blockIdx.x, &r)) return;
  uint32_t prefix = 0, mask = 0;
  int want = p.k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < r.n_out; t += 256) {
      uint32_t u;
      if (knn_key(p, r.i, r.ol[t], &u) && (u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
    }
    __syncthreads();
    const int h = hist[threadIdx.x];
    int total;
    const int excl = block_excl_scan(h, scan_s, &total);
    if (pass == 0) {                              // total = the row's candidates
      if (total == 0) return;
      want = min(want, total);
    }
    if (excl < want && want <= excl + h) { pick[0] = threadIdx.x; pick[1] = want - excl; }   // one bin holds the k-th
    __syncthreads();
    prefix |= (uint32_t)pick[0] << shift;
    mask |= 0xFFu << shift;
    want = pick[1];
    __syncthreads();
  }
  int seen = 0;                                   // keys equal to the k-th in earlier sweeps
  for (int t0 = 0; t0 < r.n_out; t0 += 256) {
    const int t = t0 + threadIdx.x;
    uint32_t u = 0;
    int j = -1;
    bool ok = false;
    if (t < r.n_out) { j = r.ol[t]; ok = knn_key(p, r.i, j, &u); }
    const bool eq = ok && u == prefix;
    int total;
    const int rank = block_excl_scan(eq ? 1 : 0, scan_s, &total);
    if (ok && (u < prefix || (eq && seen + rank < want))) {
      knn_set(p.bits, p.e.t.n_nodes, r.i, j);
      knn_set(p.bits, p.e.t.n_nodes, j, r.i);
    }
    seen += total;
  }
}

__global__ __launch_bounds__(256) void gk_count_kernel(KnnParams p) {
  __shared__ int scan_s[4];
  GbRow r;
  int c = 0;
  if (gb_row_of(p.e.t, blockIdx.x, &r))
    for (int t = threadIdx.x; t < r.n_out; t += 256)
      if (knn_kept(p, r.i, r.ol[t])) ++c;
  int total;
  block_excl_scan(c, scan_s, &total);
  if (threadIdx.x == 0) p.row_off[blockIdx.x] = total;
}

// one workgroup: counts -> first output slot of every row, the total to n_kept (a sweep's counts fit an int: 256 x 46000)
__global__ __launch_bounds__(256) void gk_scan_kernel(int64_t* row_off, int64_t n, int64_t* n_kept) {
  __shared__ int scan_s[4];
  int64_t carry = 0;
  for (int64_t q0 = 0; q0 < n; q0 += 256) {
    const int64_t q = q0 + threadIdx.x;
    const int v = q < n ? (int)row_off[q] : 0;
    int total;
    const int excl = block_excl_scan(v, scan_s, &total);
    if (q < n) row_off[q] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) *n_kept = carry;
}

// Slots at or beyond `capacity` are not written: a caller whose buffers are too short reads n_kept > capacity and has
// the first `capacity` edges.
__global__ __launch_bounds__(256) void gk_fill_kernel(KnnParams p) {
  __shared__ int scan_s[4];
  GbRow r;
  if (!gb_row_of(p.e.t, blockIdx.x, &r)) return;
  int64_t at = p.row_off[blockIdx.x];
  for (int t0 = 0; t0 < r.n_out; t0 += 256) {
    const int t = t0 + threadIdx.x;
    int j = -1;
    bool kept = false;
    if (t < r.n_out) { j = r.ol[t]; kept = knn_kept(p, r.i, j); }
    int total;
    const int64_t pos = at + block_excl_scan(kept ? 1 : 0, scan_s, &total);
    if (kept && pos < p.capacity) {
      gb_write_edge(p.e, pos, r.i, j);
      p.edge_pos[pos] = r.e0 + t;
    }
    at += total;
  }
}

}  // namespace mtmc

namespace {
using mtmc::GraphCall, mtmc::KnnParams;

struct KnnLayout { mtmc::GraphLayout g; size_t bits, bits_bytes, row_off, total; };
KnnLayout knn_layout(int64_t n, int f) {
  KnnLayout l;
  l.g = mtmc::graph_layout(n, f);
  mtmc::Carver ws{l.g.total};
  l.bits_bytes = ((size_t)n * n + 31) / 32 * sizeof(unsigned);      // N^2 / 8 bytes, rounded up to a word
  l.bits = ws.take(l.bits_bytes);
  l.row_off = ws.take((size_t)n * sizeof(int64_t));
  l.total = ws.off;
  return l;
}

// The one body of mtmc_build_graph_knn (start == null, k >= 1) and mtmc_build_graph_gated (start given, k >= 0).  Each entry
// has checked its own k / gate arguments and put them, the capacity and edge_pos_out into `p`; the rest of `p` is filled
// here.  `entry` heads the messages.
int knn_build(const char* entry, const GraphCall& c, KnnParams p, int64_t* n_kept_out) {
  using mtmc_api::fail;
  if (int rc = mtmc::graph_check_args(entry, c)) return rc;
  if (p.capacity < 0) return fail(MTMC_E_ARG, "%s: edge_capacity must be >= 0", entry);
  if (!n_kept_out || (c.t.n_edges > 0 && !p.edge_pos))
    return fail(MTMC_E_ARG, "%s: NULL n_kept_out, or NULL edge_pos_out with n_edges > 0", entry);
  if (((uintptr_t)c.edge_index_out & 15) || ((uintptr_t)c.edge_attr_out & 7))
    return fail(MTMC_E_ARG, "%s: edge_index_out must be 16-byte and edge_attr_out 8-byte aligned", entry);
  const KnnLayout l = knn_layout(c.t.n_nodes, c.feat_dim);
  if (int rc = mtmc::graph_check_workspace(entry, c.workspace, c.workspace_bytes, l.total, "mtmc_graph_knn_workspace_bytes")) return rc;
  hipStream_t s = c.stream;
  if (int rc = mtmc::graph_normalize_gram(entry, c, l.g)) return rc;
  if (c.t.n_edges <= 0) {
    if (hipMemsetAsync(n_kept_out, 0, sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
    return mtmc_api::launched(entry);
  }
  p.e = mtmc::edge_build_params(c, l.g);
  p.bits = c.at<unsigned>(l.bits); p.row_off = c.at<int64_t>(l.row_off);
  const dim3 rows((unsigned)c.t.n_nodes), wg(256);
  if (p.k > 0) {                                  // k == 0: the gate alone, decided per column in count and fill
    if (hipMemsetAsync(p.bits, 0, l.bits_bytes, s) != hipSuccess) return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
    hipLaunchKernelGGL(mtmc::gk_select_kernel, rows, wg, 0, s, p);
  }
  hipLaunchKernelGGL(mtmc::gk_count_kernel, rows, wg, 0, s, p);
  hipLaunchKernelGGL(mtmc::gk_scan_kernel, dim3(1), wg, 0, s, p.row_off, c.t.n_nodes, n_kept_out);
  hipLaunchKernelGGL(mtmc::gk_fill_kernel, rows, wg, 0, s, p);
  return mtmc_api::launched(entry);
}
}  // namespace

extern "C" {

using mtmc_api::fail;

size_t mtmc_graph_knn_workspace_bytes(int64_t n_nodes, int32_t feat_dim) {
  return mtmc::graph_size_ok(n_nodes, feat_dim) ? knn_layout(n_nodes, feat_dim).total : 0;
}

int32_t mtmc_build_graph_knn(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                             const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                             const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                             float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                             int32_t k, int64_t edge_capacity, int64_t* edge_pos_out, int64_t* n_kept_out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (k < 1) return fail(MTMC_E_ARG, "build_graph_knn: k must be >= 1");
  const GraphCall c = {{in_list, in_off, out_list, out_off, block_off, n_cams, n_nodes, n_edges},
                       feats, feat_row_stride, feat_dim, l2norm, node_labels, x_out, edge_index_out, edge_attr_out,
                       edge_labels_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
  KnnParams p = {};
  p.k = k; p.capacity = edge_capacity; p.edge_pos = edge_pos_out;
  return knn_build("build_graph_knn", c, p, n_kept_out);
}

int32_t mtmc_build_graph_gated(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                               const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                               const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                               float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                               const int64_t* start_frames, int64_t max_gap, int32_t k,
                               int64_t edge_capacity, int64_t* edge_pos_out, int64_t* n_kept_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!start_frames || max_gap < 1 || k < 0)
    return fail(MTMC_E_ARG, "build_graph_gated: NULL start_frames, max_gap < 1 or k < 0");
  const GraphCall c = {{in_list, in_off, out_list, out_off, block_off, n_cams, n_nodes, n_edges},
                       feats, feat_row_stride, feat_dim, l2norm, node_labels, x_out, edge_index_out, edge_attr_out,
                       edge_labels_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
  KnnParams p = {};
  p.k = k; p.capacity = edge_capacity; p.edge_pos = edge_pos_out; p.start = start_frames; p.max_gap = max_gap;
  return knn_build("build_graph_gated", c, p, n_kept_out);
}

}  // extern "C"
