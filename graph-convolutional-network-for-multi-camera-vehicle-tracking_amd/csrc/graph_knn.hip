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
//
// mtmc_build_graph_paneled: the same rule, order and bits with nothing N^2-sized.  G is formed in row panels
// of P node rows ([P][N], graph_gram), twice; the picks live in per-row lists and "kept" is an LDS bitmap per row.
//     gp_select_kernel   per panel, one workgroup per row: the same select, an admitted column goes to picks[i][slot]
//     gp_transpose_kernel  in-degree of every node (integer atomics), gk_scan_kernel, then rev = who picked node i
//     gp_count_kernel    one workgroup per row: bit rank(j in out_list) for every j of picks[i] and rev[i], then a popcount
//     gk_scan_kernel     as above
//     gp_fill_kernel     per panel (G formed again), one workgroup per row: the same bitmap, the same ordered compaction
// The order inside rev[i] varies from run to run; the bitmap it is OR-ed into does not.
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
// 46 000 nodes, 1 MB at the paneled entry's 262 144: it stays in L2).  After four passes `want` of the keys equal to the k-th are admitted with every smaller one;
// out_list ascends, so a prefix count in sweep order admits the lowest columns first.  Only candidates have a key
// (knn_key): with a gate the row ranks what passes it, want = min(k, candidates), and a row without any sets no bit.
// kList: an admitted column goes to picks[slot] instead, slot = its prefix count in sweep order (so a row's picks ascend by
// column and are a function of the keys alone), and *n_pick = their number, min(k, candidates) <= p.k.
template <bool kList>
__device__ __forceinline__ void knn_select_row(const KnnParams& p, const GbRow& r, int* picks, int* n_pick) {
  __shared__ int hist[256];
  __shared__ int scan_s[4];
  __shared__ int pick[2];
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
  int stored = 0;                                 // kList: columns admitted in earlier sweeps
  for (int t0 = 0; t0 < r.n_out; t0 += 256) {
    const int t = t0 + threadIdx.x;
    uint32_t u = 0;
    int j = -1;
    bool ok = false;
    if (t < r.n_out) { j = r.ol[t]; ok = knn_key(p, r.i, j, &u); }
    const bool eq = ok && u == prefix;
    int total;
    const int rank = block_excl_scan(eq ? 1 : 0, scan_s, &total);
    const bool admit = ok && (u < prefix || (eq && seen + rank < want));
    seen += total;
    if constexpr (kList) {
      const int slot = stored + block_excl_scan(admit ? 1 : 0, scan_s, &total);
      if (admit && slot < p.k) picks[slot] = j;
      stored += total;
    } else if (admit) {
      knn_set(p.bits, p.e.t.n_nodes, r.i, j);
      knn_set(p.bits, p.e.t.n_nodes, j, r.i);
    }
  }
  if (kList && threadIdx.x == 0) *n_pick = min(stored, p.k);
}

__global__ __launch_bounds__(256) void gk_select_kernel(KnnParams p) {
  GbRow r;
  if (gb_row_of(p.e.t, blockIdx.x, &r)) knn_select_row<false>(p, r, nullptr, nullptr);
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

// one workgroup: counts -> first output slot of every row, the total to n_kept (a sweep's counts fit an int: 256 x 262144)
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
// kept(t, j): column t of the row's out_list, node j, is in the result.
template <class Kept>
__device__ __forceinline__ void knn_fill_row(const KnnParams& p, const GbRow& r, int64_t at, Kept is_kept) {
  __shared__ int scan_s[4];
  for (int t0 = 0; t0 < r.n_out; t0 += 256) {
    const int t = t0 + threadIdx.x;
    int j = -1;
    bool kept = false;
    if (t < r.n_out) { j = r.ol[t]; kept = is_kept(t, j); }
    int total;
    const int64_t pos = at + block_excl_scan(kept ? 1 : 0, scan_s, &total);
    if (kept && pos < p.capacity) {
      gb_write_edge(p.e, pos, r.i, j);
      p.edge_pos[pos] = r.e0 + t;
    }
    at += total;
  }
}

__global__ __launch_bounds__(256) void gk_fill_kernel(KnnParams p) {
  GbRow r;
  if (!gb_row_of(p.e.t, blockIdx.x, &r)) return;
  knn_fill_row(p, r, p.row_off[blockIdx.x], [&](int, int j) { return knn_kept(p, r.i, j); });
}

// ---- the paneled form: p.k.e.G holds the Gram rows of the nodes [p.k.e.g_row0, + gridDim.x) of the select and fill launches
struct PanelParams {
  KnnParams k;                                  // k.bits is not used; k.k <= 4096
  const int* node_cam; const int* node_loc;     // graph_node_map: the inverse of in_list
  int* picks; int* n_pick;                      // [N][k] top_i ascending by column, [N] their number
  int64_t* rev_off; int* rev_cnt; int* rev;     // rev[rev_off[i] .. + rev_cnt[i]): the rows that picked node i, in any order
};

// the row of NODE i and its in_list position; false where the tables name no such row or one longer than the bitmap
__device__ __forceinline__ bool gp_row_of(const PanelParams& p, int i, GbRow* r, int64_t* q) {
  const GraphTables& t = p.k.e.t;
  const int c = p.node_cam[i];
  if (c < 0 || c >= t.n_cams) return false;
  *q = (int64_t)t.in_off[c] + p.node_loc[i];
  return gb_row_of(t, *q, r) && r->i == i && r->n_out <= t.n_nodes;
}

__global__ __launch_bounds__(256) void gp_select_kernel(PanelParams p) {
  const int i = (int)p.k.e.g_row0 + blockIdx.x;
  GbRow r;
  int64_t q;
  if (gp_row_of(p, i, &r, &q)) knn_select_row<true>(p.k, r, p.picks + (int64_t)i * p.k.k, p.n_pick + i);
}

// one thread per (row i, slot): kFill false counts node picks[i][slot]'s in-degree into rev_off, true enters i in its rev
template <bool kFill>
__global__ __launch_bounds__(256) void gp_transpose_kernel(PanelParams p) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= p.k.e.t.n_nodes * p.k.k) return;
  const int i = (int)(at / p.k.k);
  if ((int)(at % p.k.k) >= p.n_pick[i]) return;
  const int j = p.picks[at];                      // a node: knn_key admits no other
  if (kFill) p.rev[p.rev_off[j] + atomicAdd(p.rev_cnt + j, 1)] = i;
  else atomicAdd(reinterpret_cast<unsigned long long*>(p.rev_off + j), 1ull);
}

// bm = the kept columns of row r as bits over its out_list: bit rank(j) for every j in picks[i] and in rev[i].  ORs commute.
__device__ __forceinline__ void gp_mark(const PanelParams& p, const GbRow& r, unsigned* bm) {
  for (int w = threadIdx.x; w < (r.n_out + 31) >> 5; w += 256) bm[w] = 0;
  __syncthreads();
  const int np = min(p.n_pick[r.i], p.k.k), nr = p.rev_cnt[r.i];
  const int* pk = p.picks + (int64_t)r.i * p.k.k;
  const int* rv = p.rev + p.rev_off[r.i];
  for (int s = threadIdx.x; s < np + nr; s += 256) {
    const int64_t t = gb_rank_in(r.ol, r.n_out, s < np ? pk[s] : rv[s - np]);
    if (t >= 0) atomicOr(bm + (t >> 5), 1u << (t & 31));
  }
  __syncthreads();
}

// dynamic LDS of the next two: (N + 31) / 32 words where k >= 1 (n_out <= N: gp_row_of), none where the gate stands alone
__global__ __launch_bounds__(256) void gp_count_kernel(PanelParams p) {
  extern __shared__ unsigned bm[];
  __shared__ int scan_s[4];
  GbRow r;
  int64_t q;
  if (!gp_row_of(p, blockIdx.x, &r, &q)) return;  // row_off is zero on entry
  int c = 0;
  if (p.k.k) {
    gp_mark(p, r, bm);
    for (int w = threadIdx.x; w < (r.n_out + 31) >> 5; w += 256) c += __popc(bm[w]);
  } else {
    for (int t = threadIdx.x; t < r.n_out; t += 256)
      if (knn_kept(p.k, r.i, r.ol[t])) ++c;
  }
  int total;
  block_excl_scan(c, scan_s, &total);
  if (threadIdx.x == 0) p.k.row_off[q] = total;
}

__global__ __launch_bounds__(256) void gp_fill_kernel(PanelParams p) {
  extern __shared__ unsigned bm[];
  GbRow r;
  int64_t q;
  if (!gp_row_of(p, (int)p.k.e.g_row0 + blockIdx.x, &r, &q)) return;
  if (p.k.k) gp_mark(p, r, bm);
  knn_fill_row(p.k, r, p.k.row_off[q],
               [&](int t, int j) { return p.k.k ? ((bm[t >> 5] >> (t & 31)) & 1u) != 0 : knn_kept(p.k, r.i, j); });
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

// ---- the paneled form
constexpr int kPanelMaxK = 4096;                  // picks: 16 KB per row at the most
constexpr size_t kPanelAutoBytes = (size_t)1 << 30;

// the panel rows a call uses: the request clipped to N; for 0 the largest multiple of 128 whose panel stays within 1 GiB, at
// least 128, clipped to N
int64_t panel_rows_for(int64_t n, int64_t request) {
  if (request > 0) return request < n ? request : n;
  int64_t rows = (int64_t)(kPanelAutoBytes / ((size_t)n * sizeof(float))) / 128 * 128;
  if (rows < 128) rows = 128;
  return rows < n ? rows : n;
}

inline bool panel_sizes_ok(int64_t n, int f, int64_t k, int64_t panel_rows) {   // k: already clipped to n
  return mtmc::graph_size_ok(n, f, mtmc::kGraphMaxNodesPaneled) && f % 32 == 0 && k >= 0 && k <= kPanelMaxK && panel_rows >= 0;
}

// l.g: the family's regions with G and the slab sized for `rows` Gram rows; nothing here grows as N^2
struct PanelLayout {
  mtmc::GraphLayout g; int64_t rows;
  size_t node_cam, node_loc, row_off, n_pick, rev_off, rev_cnt, total_out, picks, rev, total;
};
PanelLayout panel_layout(int64_t n, int f, int k, int64_t panel_rows) {
  PanelLayout l;
  l.rows = panel_rows_for(n, panel_rows);
  l.g = mtmc::graph_layout(n, f, l.rows);
  mtmc::Carver ws{l.g.total};
  l.node_cam = ws.take((size_t)n * sizeof(int));
  l.node_loc = ws.take((size_t)n * sizeof(int));
  l.row_off = ws.take((size_t)n * sizeof(int64_t));
  l.n_pick = ws.take((size_t)n * sizeof(int));
  l.rev_off = ws.take((size_t)n * sizeof(int64_t));
  l.rev_cnt = ws.take((size_t)n * sizeof(int));
  l.total_out = ws.take(sizeof(int64_t));         // the picks' total, which gk_scan_kernel writes and nobody reads
  l.picks = ws.take((size_t)n * k * sizeof(int));
  l.rev = ws.take((size_t)n * k * sizeof(int));
  l.total = ws.off;
  return l;
}

// mtmc_build_graph_paneled's body; the entry has checked k / gate and put them, the capacity and edge_pos_out into `p`
// (p.k clipped to n_nodes).
int paneled_build(const char* entry, const GraphCall& c, KnnParams kp, int64_t panel_rows, int64_t* n_kept_out) {
  using mtmc_api::fail;
  const int64_t n = c.t.n_nodes;
  if (int rc = mtmc::graph_check_args(entry, c, mtmc::kGraphMaxNodesPaneled)) return rc;
  if (kp.k > kPanelMaxK || panel_rows < 0)
    return fail(MTMC_E_ARG, "%s: min(k, n_nodes) must be <= %d and panel_rows >= 0", entry, kPanelMaxK);
  if (c.feat_dim > 6144 && n > 2048)
    return fail(MTMC_E_ARG, "%s: feat_dim > 6144 is handled up to 2048 nodes", entry);
  if (kp.capacity < 0) return fail(MTMC_E_ARG, "%s: edge_capacity must be >= 0", entry);
  if (!n_kept_out || (c.t.n_edges > 0 && !kp.edge_pos))
    return fail(MTMC_E_ARG, "%s: NULL n_kept_out, or NULL edge_pos_out with n_edges > 0", entry);
  if (((uintptr_t)c.edge_index_out & 15) || ((uintptr_t)c.edge_attr_out & 7))
    return fail(MTMC_E_ARG, "%s: edge_index_out must be 16-byte and edge_attr_out 8-byte aligned", entry);
  const PanelLayout l = panel_layout(n, c.feat_dim, kp.k, panel_rows);
  if (int rc = mtmc::graph_check_workspace(entry, c.workspace, c.workspace_bytes, l.total, "mtmc_graph_paneled_workspace_bytes")) return rc;
  hipStream_t s = c.stream;
  if (int rc = mtmc::graph_normalize(entry, c, l.g)) return rc;
  if (c.t.n_edges <= 0) {
    if (hipMemsetAsync(n_kept_out, 0, sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
    return mtmc_api::launched(entry);
  }
  mtmc::PanelParams p = {};
  p.k = kp;
  p.k.e = mtmc::edge_build_params(c, l.g);
  p.k.row_off = c.at<int64_t>(l.row_off);
  p.node_cam = c.at<int>(l.node_cam); p.node_loc = c.at<int>(l.node_loc);
  p.picks = c.at<int>(l.picks); p.n_pick = c.at<int>(l.n_pick);
  p.rev_off = c.at<int64_t>(l.rev_off); p.rev_cnt = c.at<int>(l.rev_cnt); p.rev = c.at<int>(l.rev);
  const dim3 wg(256), all_rows((unsigned)n);
  const size_t lds = kp.k ? (size_t)((n + 31) / 32) * sizeof(unsigned) : 0;
  // row_off .. rev_cnt are adjacent regions: one memset zeroes the counts, in-degrees and cursors
  if (mtmc::graph_node_map(c.t, c.at<int>(l.node_cam), c.at<int>(l.node_loc), s) != MTMC_OK ||
      hipMemsetAsync(p.k.row_off, 0, l.total_out - l.row_off, s) != hipSuccess)
    return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
  // per panel: its Gram rows, then `kernel` with one workgroup per row of it
  auto panels = [&](auto kernel, size_t lds_bytes) {
    for (int64_t r0 = 0; r0 < n; r0 += l.rows) {
      const int64_t rows = n - r0 < l.rows ? n - r0 : l.rows;
      if (int rc = mtmc::graph_gram(entry, c, l.g, r0, rows)) return rc;
      p.k.e.g_row0 = r0;
      hipLaunchKernelGGL(kernel, dim3((unsigned)rows), wg, lds_bytes, s, p);
    }
    return (int)MTMC_OK;
  };
  if (kp.k > 0) {                                 // pass 1: the picks, then who picked whom
    if (int rc = panels(mtmc::gp_select_kernel, 0)) return rc;
    const dim3 slots((unsigned)((n * kp.k + 255) / 256));
    hipLaunchKernelGGL(mtmc::gp_transpose_kernel<false>, slots, wg, 0, s, p);
    hipLaunchKernelGGL(mtmc::gk_scan_kernel, dim3(1), wg, 0, s, p.rev_off, n, c.at<int64_t>(l.total_out));
    hipLaunchKernelGGL(mtmc::gp_transpose_kernel<true>, slots, wg, 0, s, p);
  }
  hipLaunchKernelGGL(mtmc::gp_count_kernel, all_rows, wg, lds, s, p);
  hipLaunchKernelGGL(mtmc::gk_scan_kernel, dim3(1), wg, 0, s, p.k.row_off, n, n_kept_out);
  if (kp.k > 0 && l.rows == n) {                  // one panel: it still holds all of G
    p.k.e.g_row0 = 0;
    hipLaunchKernelGGL(mtmc::gp_fill_kernel, all_rows, wg, lds, s, p);
  } else if (int rc = panels(mtmc::gp_fill_kernel, lds)) {   // pass 2: G again, then the edges of the panel's rows
    return rc;
  }
  return mtmc_api::launched(entry);
}
}  // namespace

extern "C" {

using mtmc_api::fail;

int64_t mtmc_graph_panel_rows(int64_t n_nodes, int32_t feat_dim, int64_t panel_rows) {
  return panel_sizes_ok(n_nodes, feat_dim, 0, panel_rows) ? panel_rows_for(n_nodes, panel_rows) : 0;
}

size_t mtmc_graph_paneled_workspace_bytes(int64_t n_nodes, int32_t feat_dim, int32_t k, int64_t panel_rows) {
  const int64_t kk = k < n_nodes ? k : n_nodes;
  return panel_sizes_ok(n_nodes, feat_dim, kk, panel_rows) ? panel_layout(n_nodes, feat_dim, (int)kk, panel_rows).total : 0;
}

int32_t mtmc_build_graph_paneled(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                                 const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                                 const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                                 float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                                 const int64_t* start_frames, int64_t max_gap, int32_t k, int64_t panel_rows,
                                 int64_t edge_capacity, int64_t* edge_pos_out, int64_t* n_kept_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (k < 0 || (k == 0 && !start_frames) || (start_frames && max_gap < 1))
    return fail(MTMC_E_ARG, "build_graph_paneled: k >= 1 or a gate (start_frames with max_gap >= 1) is needed, and k >= 0");
  const GraphCall c = {{in_list, in_off, out_list, out_off, block_off, n_cams, n_nodes, n_edges},
                       feats, feat_row_stride, feat_dim, l2norm, node_labels, x_out, edge_index_out, edge_attr_out,
                       edge_labels_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
  KnnParams p = {};
  p.k = k < n_nodes ? k : (int)(n_nodes > 0 ? n_nodes : 0);
  p.capacity = edge_capacity; p.edge_pos = edge_pos_out; p.start = start_frames; p.max_gap = max_gap;
  return paneled_build("build_graph_paneled", c, p, panel_rows, n_kept_out);
}

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
