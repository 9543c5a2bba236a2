// Post-processing of the MPN's edge logits on the device.
//
// Replaces reference inference.py:475-489 + post_processing (:70-169) + utils.py compute_SCC_and_Clusters (:30-52),
// splitting (:54-123), remove_edges_single_direction (:125-142), pruning (:144-339): softmax / argmax over the E
// edges, then -- on the few edges predicted active -- symmetric cut, flow pruning, strongly connected components and
// splitting of over-sized clusters, producing the same `predictions [E]` and the same cluster numbering `ID_pred [N]`.
//
// Shape of the work: E-sized, embarrassingly parallel and HBM-bound up to the compaction of the A active edges
// (A ~ 1 % of E on a trained model); everything after that is a data-dependent loop nest on A edges / N nodes whose
// iteration counts are only known on the device.  So:
//   pp_classify_kernel   wide: p1 = softmax(logits)[:,1], prediction = argmax (ties -> 0), per-block active counts
//   pp_scan_kernel       one block: exclusive scan of the block counts -> A
//   pp_compact_kernel    wide: active edges, in ascending edge order, to (edge id, u, v, p1) arrays
//   pp_graph_kernel      ONE workgroup of 1024 lanes, resident for the whole cut / prune / cut / split sequence:
//                        set-parallel steps run on all lanes with block barriers in between; the cluster *numbering*
//                        is defined by networkx's depth-first traversal order (utils.py:31), which is inherently
//                        sequential, so that walk runs on lane 0 -- out of LDS whenever N <= 2048 and A <= 8192.
// No host round trip, no dynamic allocation: a caller can enqueue it right behind the forward.
#include "api_error.h"
#include "kernels.h"

#include <stdint.h>

namespace mtmc {

constexpr int kPpChunk = 1024;            // edges per block in the wide kernels (256 lanes x 4)
constexpr int kPpThreads = 1024;          // the graph kernel's workgroup and its loops' stride (blockDim.x is a load)
constexpr int kPpLdsNodes = 2048;         // LDS-resident graph state up to this many nodes ...
constexpr int kPpLdsEdges = 8192;         // ... and this many active edges
constexpr int kPpNodeArrays = 13;         // rowptr, label, t0..t6, component records (size, tree key, sequence, free ids)
constexpr unsigned kDead = 0x80000000u;
constexpr int kPpMaxSplitIters = 1 << 18;  // splitting iterations before giving up (status 3); real runs need tens

struct PpParams {
  const float* logits;                    // [E][2] or nullptr (then prob1/pred are inputs)
  const int64_t* row; const int64_t* col; int64_t idx_stride;
  int64_t n_nodes, n_edges;
  int num_cameras, flags;
  float* prob1;                           // [E]
  int64_t* pred;                          // [E]
  int64_t* id_pred;                       // [N]
  int32_t* info;                          // [8]: A_in, A_out, clusters, status, split iterations, scc walks, prune rounds
  // workspace
  int* hdr; int* block_count; int* a_idx; int* a_u; int* a_v; float* a_p; int* a_slot; unsigned char* alive;
  unsigned char* mark; int* g_node; unsigned* g_csr; int* g_flags; int* b_idx; int* b_u; int* b_v; float* b_p; int64_t cap;
  int* g_wcc; int* g_dirty;                // [N] each: weakly connected component of a node, per-component dirty flag
};

__device__ __forceinline__ float softmax_p1(float l0, float l1) {
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  return e1 / (e0 + e1);
}

__global__ __launch_bounds__(256) void pp_classify_kernel(PpParams p) {
  __shared__ int wsum[4];
  const int64_t base = (int64_t)blockIdx.x * kPpChunk;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + i * 256 + threadIdx.x;
    int on = 0;
    if (e < p.n_edges) {
      if (p.logits) {
        const float2 l = reinterpret_cast<const float2*>(p.logits)[e];
        p.prob1[e] = softmax_p1(l.x, l.y);
        on = l.y > l.x ? 1 : 0;                         // torch.argmax: first maximum
        p.pred[e] = on;
      } else {
        on = p.pred[e] == 1;
      }
    }
    cnt += __popcll(__ballot(on));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) p.block_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of n ints in place, total returned to every lane (one block, any n)
__device__ int block_exclusive_scan(int* a, int64_t n, int* sh /* [blockDim.x/64 + 1] */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int carry = 0;
  for (int64_t base = 0; base < n; base += blockDim.x) {
    const int64_t i = base + threadIdx.x;
    const int v = i < n ? a[i] : 0;
    int s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(s, off, 64);
      if (lane >= off) s += t;
    }
    if (lane == 63) sh[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0;
      for (int w = 0; w < nw; ++w) { const int t = sh[w]; sh[w] = acc; acc += t; }
      sh[nw] = acc;
    }
    __syncthreads();
    if (i < n) a[i] = carry + sh[wid] + s - v;
    carry += sh[nw];
    __syncthreads();
  }
  return carry;
}

__global__ __launch_bounds__(1024) void pp_scan_kernel(PpParams p, int n_blocks) {
  __shared__ int sh[17];
  const int total = block_exclusive_scan(p.block_count, n_blocks, sh);
  if (threadIdx.x == 0) {
    p.hdr[0] = total;
    p.hdr[2] = 0;
    p.hdr[3] = 0;
    p.hdr[1] = total > p.cap ? 1 : 0;                   // more active edges than the workspace was sized for
    p.info[0] = total;
  }
}

__global__ __launch_bounds__(256) void pp_compact_kernel(PpParams p) {
  __shared__ int woff[4];
  if (p.hdr[1]) return;
  const int64_t base = (int64_t)blockIdx.x * kPpChunk;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int out = p.block_count[blockIdx.x];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + i * 256 + threadIdx.x;
    const int on = (e < p.n_edges && p.pred[e] == 1) ? 1 : 0;
    const unsigned long long b = __ballot(on);
    if (lane == 0) woff[wid] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wid; ++w) before += woff[w];
    const int tot = woff[0] + woff[1] + woff[2] + woff[3];
    if (on) {
      const int k = out + before + __popcll(b & ((1ull << lane) - 1));
      p.a_idx[k] = (int)e;
      int64_t u = p.row[e * p.idx_stride], v = p.col[e * p.idx_stride];
      if (u < 0 || u >= p.n_nodes || v < 0 || v >= p.n_nodes) {   // never index with it: clamp and report (status 4)
        p.hdr[3] = 1;
        u = u < 0 ? 0 : (u >= p.n_nodes ? p.n_nodes - 1 : u);
        v = v < 0 ? 0 : (v >= p.n_nodes ? p.n_nodes - 1 : v);
      }
      p.a_u[k] = (int)u;
      p.a_v[k] = (int)v;
      p.a_p[k] = p.prob1[e];
      p.alive[k] = 1;
    }
    out += tot;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// the resident workgroup
// ------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) int* LdsIntPtr;
typedef __attribute__((address_space(3))) unsigned* LdsUintPtr;

// Templated on the pointer types so that lane 0's walk over an LDS-resident graph compiles to ds_read/ds_write
// instead of flat accesses (pp_run_walk); everything else uses generic pointers.
template <typename IP, typename UP>
struct PpGraphT {
  // N-sized, npad apart from rowptr on
  IP rowptr;       // [N+1] CSR over ALL compacted active edges, rows in ascending active id (= edge order)
  IP label;        // [N]   cluster number of the node's component (output numbering)
  IP t0, t1, t2, t3, t4, t5, t6;                                   // [N] each, phase-dependent (see uses)
  IP csize, ctree, cseq, freel;                                    // [N] each: component records of the splitting loop
  UP csr;          // [A]   target node | kDead
  int n, a, cams;
  size_t npad;
  bool lds_nodes, lds_walk;   // node arrays in LDS; node arrays AND csr in LDS
  __device__ void place_nodes(IP base) {
    rowptr = base; label = base + npad; t0 = base + 2 * npad; t1 = base + 3 * npad; t2 = base + 4 * npad;
    t3 = base + 5 * npad; t4 = base + 6 * npad; t5 = base + 7 * npad; t6 = base + 8 * npad;
    csize = base + 9 * npad; ctree = base + 10 * npad; cseq = base + 11 * npad; freel = base + 12 * npad;
  }
};
typedef PpGraphT<int*, unsigned*> PpGraph;

__device__ __forceinline__ void pp_kill(const PpParams& p, const PpGraph& g, int i) {
  p.alive[i] = 0;
  g.csr[p.a_slot[i]] |= kDead;
}

// CSR of the active edges by source node; each row in ascending active id, i.e. in the order networkx inserts the
// successors when the reference builds nx.DiGraph(list of active edges).
__device__ void pp_build_csr(const PpParams& p, const PpGraph& g, int* sh) {
  int* deg = g.rowptr;
  for (int i = threadIdx.x; i <= g.n; i += kPpThreads) deg[i] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) atomicAdd(&deg[p.a_u[i]], 1);
  __syncthreads();
  block_exclusive_scan(deg, (int64_t)g.n + 1, sh);      // rowptr[n] = A
  int* fill = g.t0;
  for (int i = threadIdx.x; i < g.n; i += kPpThreads) fill[i] = g.rowptr[i];
  __syncthreads();
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) p.a_slot[i] = atomicAdd(&fill[p.a_u[i]], 1);   // any order ...
  __syncthreads();
  // ... then each row's slots re-dealt in ascending active id (rows are short: insertion sort per row)
  int* ids = reinterpret_cast<int*>(g.csr);
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) ids[p.a_slot[i]] = i;
  __syncthreads();
  for (int r = threadIdx.x; r < g.n; r += kPpThreads) {
    const int lo = g.rowptr[r], hi = g.rowptr[r + 1];
    for (int x = lo + 1; x < hi; ++x) {
      const int key = ids[x];
      int y = x - 1;
      while (y >= lo && ids[y] > key) { ids[y + 1] = ids[y]; --y; }
      ids[y + 1] = key;
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < g.a; s += kPpThreads) {
    const int i = ids[s];
    p.a_slot[i] = s;
    p.mark[s] = 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) g.csr[p.a_slot[i]] = (unsigned)p.a_v[i];
  __syncthreads();
}

// utils.py:125-142: an active edge survives only if its reverse is active too -- decided on a snapshot
__device__ void pp_cut(const PpParams& p, const PpGraph& g) {
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) {
    int drop = 0;
    if (p.alive[i]) {
      const unsigned u = (unsigned)p.a_u[i];
      const int v = p.a_v[i];
      drop = 1;
      for (int s = g.rowptr[v]; s < g.rowptr[v + 1]; ++s)
        if (g.csr[s] == u) { drop = 0; break; }          // alive (no kDead bit) and pointing back at u
    }
    p.mark[i] = (unsigned char)drop;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < g.a; i += kPpThreads)
    if (p.mark[i]) pp_kill(p, g, i);
  __syncthreads();
}

// utils.py:144-339 (the live branch): while some node has more than num_cameras-1 active out- (in-) edges, every
// such node drops its least probable active out- (in-) edge (lowest edge index on ties), all chosen on one snapshot
__device__ int pp_prune(const PpParams& p, const PpGraph& g) {
  int* flow_out = g.t0; int* flow_in = g.t1;
  unsigned long long* key_out = reinterpret_cast<unsigned long long*>(g.t2);   // t2|t3
  unsigned long long* key_in = reinterpret_cast<unsigned long long*>(g.t4);    // t4|t5
  int rounds = 0;
  for (;;) {
    for (int n = threadIdx.x; n < g.n; n += kPpThreads) {
      flow_out[n] = 0; flow_in[n] = 0; key_out[n] = ~0ull; key_in[n] = ~0ull;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < g.a; i += kPpThreads) {
      if (!p.alive[i]) continue;
      const int u = p.a_u[i], v = p.a_v[i];
      const unsigned long long key = ((unsigned long long)__float_as_uint(p.a_p[i]) << 32) | (unsigned)i;
      atomicAdd(&flow_out[u], 1);
      atomicAdd(&flow_in[v], 1);
      atomicMin(&key_out[u], key);
      atomicMin(&key_in[v], key);
    }
    __syncthreads();
    int any = 0;
    for (int n = threadIdx.x; n < g.n; n += kPpThreads) {
      if (flow_out[n] > g.cams - 1) { any = 1; pp_kill(p, g, (int)(key_out[n] & 0xffffffffu)); }
      if (flow_in[n] > g.cams - 1) { any = 1; pp_kill(p, g, (int)(key_in[n] & 0xffffffffu)); }
    }
    if (!__syncthreads_or(any)) return rounds;
    ++rounds;
  }
}

// Lane 0's part of utils.py:30-52: nx.strongly_connected_components' traversal (sources in node insertion order,
// successors in insertion order, a component is emitted when its root finishes -- Tarjan's algorithm; networkx
// evaluates the lowlinks at finish time, here they are folded into the single pass over the successors, which finds
// the same roots in the same order).  The two things a pass decides are its policy's (by value: state in registers):
//   pol.enter_tree(first)   a tree starts at an unvisited source, whose t1 still holds `first` (pp_sources)
//   pol.finish(g, v, stop)  the component rooted at v is complete: pop it off the component stack (pp_pop)
template <typename G>
__device__ __forceinline__ int pp_pop(const G& g, int v, int& stop, int id) {   // comp = id down to v; returns how many
  int w, cnt = 0;
  do { w = g.t5[--stop]; g.t2[w] = id; ++cnt; } while (w != v);
  return cnt;
}

template <typename IP, typename UP, typename Policy>
__device__ __forceinline__ Policy pp_walk(const PpGraphT<IP, UP>& g, int n_src, Policy pol) {
  const IP rowptr = g.rowptr, pre = g.t0, low = g.t1, comp = g.t2, cursor = g.t3, dstack = g.t4, sstack = g.t5, src = g.t6;
  const UP csr = g.csr;
  int counter = 0, stop = 0;
  for (int i = 0; i < n_src; ++i) {
    const int source = src[i];
    if (pre[source] != 0) continue;
    pol.enter_tree(low[source]);
    int dtop = 0;
    dstack[dtop++] = source;
    pre[source] = low[source] = ++counter;
    sstack[stop++] = source;
    while (dtop) {
      const int v = dstack[dtop - 1];
      const int end = rowptr[v + 1];
      int c = cursor[v], lv = low[v];
      int child = -1;
      while (c < end) {
        const unsigned t = csr[c++];
        if (t & kDead) continue;
        const int pt = pre[t];
        if (pt == 0) { child = (int)t; break; }
        if (comp[t] < 0) lv = min(lv, pt);               // still on the component stack
      }
      cursor[v] = c;
      low[v] = lv;
      if (child >= 0) {
        dstack[dtop++] = child;
        pre[child] = low[child] = ++counter;
        sstack[stop++] = child;
        continue;
      }
      --dtop;
      if (dtop) {                                        // tree edge parent -> v: hand the lowlink up
        const int par = dstack[dtop - 1];
        if (lv < low[par]) low[par] = lv;
      }
      if (lv == pre[v]) pol.finish(g, v, stop);
    }
  }
  return pol;
}

// the final pass: components numbered in the order networkx emits them
struct PpNumberAll {
  int n_comp;
  __device__ __forceinline__ void enter_tree(int) {}
  template <typename G>
  __device__ __forceinline__ void finish(const G& g, int v, int& stop) { pp_pop(g, v, stop, n_comp++); }
};

// the splitting loop's re-walk: ids from the free list (else a new one), and the key (size, first position of the
// tree's source, sequence within this walk) recorded per component
struct PpRecord {
  int n_free, n_ids, seq, tree_key;
  __device__ __forceinline__ void enter_tree(int first) { tree_key = first; }
  template <typename G>
  __device__ __forceinline__ void finish(const G& g, int v, int& stop) {
    const int id = n_free > 0 ? g.freel[--n_free] : n_ids++;
    g.csize[id] = pp_pop(g, v, stop, id); g.ctree[id] = tree_key; g.cseq[id] = seq++;
  }
};

// Lane 0 only.  The one place that picks the pointer types: LDS address-space pointers only when node arrays and CSR
// are both LDS-resident, generic ones otherwise.
template <typename Policy>
__device__ Policy pp_run_walk(const PpParams& p, const PpGraph& g, int n_src, Policy pol) {
  const long long t_begin = wall_clock64();
  if (g.lds_walk) {
    PpGraphT<LdsIntPtr, LdsUintPtr> l;
    l.npad = g.npad; l.place_nodes((LdsIntPtr)g.rowptr); l.csr = (LdsUintPtr)g.csr;
    pol = pp_walk(l, n_src, pol);
  } else {
    pol = pp_walk(g, n_src, pol);
  }
  p.hdr[2] += (int)(wall_clock64() - t_begin);           // 100 MHz ticks spent walking (diagnostic, info[7])
  return pol;
}

// The ordered source list of a walk over the nodes that `want`: node insertion order of nx.DiGraph(active edge list),
// i.e. first appearance, u before v within an edge.  Resets the walk state (t0 pre, t2 comp, t3 cursor) of those nodes
// -- recycle(n) sees each just before -- and leaves their first positions in t1 (the walk's low, until it visits
// them), the list in t6; returns its length.  `want` holds for both ends of an edge or for neither.
template <typename Want, typename Recycle>
__device__ int pp_sources(const PpParams& p, const PpGraph& g, int* sh, Want want, Recycle recycle) {
  int* pre = g.t0; int* first_pos = g.t1; int* comp = g.t2; int* cursor = g.t3; int* src = g.t6;
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) {
    if (!want(n)) continue;
    recycle(n);
    pre[n] = 0; comp[n] = -1; cursor[n] = g.rowptr[n]; first_pos[n] = 0x7fffffff;
  }
  for (int i = threadIdx.x; i < 2 * g.a; i += kPpThreads) p.g_flags[i] = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < g.a; k += kPpThreads) {
    if (!p.alive[k] || !want(p.a_u[k])) continue;
    atomicMin(&first_pos[p.a_u[k]], 2 * k);
    atomicMin(&first_pos[p.a_v[k]], 2 * k + 1);
  }
  __syncthreads();
  for (int n = threadIdx.x; n < g.n; n += kPpThreads)
    if (want(n) && first_pos[n] != 0x7fffffff) p.g_flags[first_pos[n]] = 1;
  __syncthreads();
  const int n_src = block_exclusive_scan(p.g_flags, 2 * (int64_t)g.a, sh);
  for (int n = threadIdx.x; n < g.n; n += kPpThreads)
    if (want(n) && first_pos[n] != 0x7fffffff) src[p.g_flags[first_pos[n]]] = n;
  __syncthreads();
  return n_src;
}

template <typename IP>
__device__ void pp_place(IP clabel, IP hist, IP csize, int n_comp) {
  for (int k = 0; k < n_comp; ++k) clabel[k] = hist[csize[k] - 1]++;
}

// utils.py:30-52.  Strongly connected components in the order networkx emits them, stably sorted by size; nodes
// without an active edge follow as singletons in index order.  label[v] = position of v's set; returns the number
// of sets; sizes by label in t5.  All lanes prepare the ordered source list and the numbering; the walk is lane 0's.
__device__ int pp_scc(const PpParams& p, const PpGraph& g, int* sh) {
  int* comp = g.t2;
  const int n_src = pp_sources(p, g, sh, [](int) { return true; }, [](int) {});
  __shared__ int s_ncomp;
  if (threadIdx.x == 0) s_ncomp = pp_run_walk(p, g, n_src, PpNumberAll{0}).n_comp;
  __syncthreads();
  const int n_comp = s_ncomp;
  // sizes per emitted component (t3), histogram of sizes (t4, sizes 1..N), stable placement by size (lane 0),
  // isolated nodes numbered after them in index order (scan over t1)
  int* csize = g.t3; int* hist = g.t4; int* clabel = g.t0; int* lsize = g.t5; int* iso = g.t1;
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) { csize[n] = 0; hist[n] = 0; iso[n] = comp[n] < 0 ? 1 : 0; }
  __syncthreads();
  for (int n = threadIdx.x; n < g.n; n += kPpThreads)
    if (comp[n] >= 0) atomicAdd(&csize[comp[n]], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < n_comp; k += kPpThreads) atomicAdd(&hist[csize[k] - 1], 1);
  __syncthreads();
  block_exclusive_scan(hist, g.n, sh);
  const int n_iso = block_exclusive_scan(iso, g.n, sh);
  if (threadIdx.x == 0) {
    if (g.lds_nodes) pp_place((LdsIntPtr)clabel, (LdsIntPtr)hist, (LdsIntPtr)csize, n_comp);
    else pp_place(clabel, hist, csize, n_comp);
  }
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) lsize[n] = 1;
  __syncthreads();
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) g.label[n] = comp[n] >= 0 ? clabel[comp[n]] : n_comp + iso[n];
  for (int k = threadIdx.x; k < n_comp; k += kPpThreads) lsize[clabel[k]] = csize[k];
  __syncthreads();
  return n_comp + n_iso;
}

// ------------------------------------------------------------------------------------------------
// Splitting loop without a full renumbering per iteration.  The loop only needs (a) the first over-sized set in the
// reference's numbering and (b) the set that carries a given number after an edge was dropped.  The numbering is
// "size, then networkx emission order"; emission order is "depth-first trees in order of their source's first
// appearance in the active edge list, components within a tree in finish order".  Dropping an edge changes trees
// only inside the weakly connected component (WCC) it belonged to, and positions in the edge list never move, so
// every component keeps the key (size, first position of its tree's source, sequence within its walk); lane 0
// re-walks the dirty WCCs alone (PpRecord) and the numbers asked for are found by counting smaller keys.
// ------------------------------------------------------------------------------------------------
__device__ void pp_wcc(const PpParams& p, const PpGraph& g) {
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) p.g_wcc[n] = n;
  __syncthreads();
  for (;;) {
    int changed = 0;
    for (int k = threadIdx.x; k < g.a; k += kPpThreads) {
      if (!p.alive[k]) continue;
      const int u = p.a_u[k], v = p.a_v[k];
      const int a = p.g_wcc[u], b = p.g_wcc[v];
      if (a < b) { atomicMin(&p.g_wcc[v], a); changed = 1; }
      else if (b < a) { atomicMin(&p.g_wcc[u], b); changed = 1; }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // pointer jumping to the component minimum (labels only ever decrease towards it)
  for (;;) {
    int changed = 0;
    for (int n = threadIdx.x; n < g.n; n += kPpThreads) {
      const int w = p.g_wcc[n], ww = p.g_wcc[w];
      if (ww != w) { p.g_wcc[n] = ww; changed = 1; }
    }
    if (!__syncthreads_or(changed)) break;
  }
}

// The splitting loop's shared words
struct PpSplitWords {
  int n_free, n_ids;            // component ids on the free list (g.freel); ids in use (high-water mark)
  int pick;                     // the component a search settled on, -1 for none
  int min_size;                 // pp_first_oversized: size of the smallest over-sized component
  int count, n_over;            // pp_number_of: smaller keys counted; pp_carrier_of: over-sized components listed
  unsigned min_prob;            // pp_split_step: minimum probability (its bits) over the edges touching the component
  unsigned long long min_key;   // pp_first_oversized: smallest pp_tree_key at min_size
};

// Re-walk the dirty WCCs: the ids of their components go back to the free list, their nodes are walked again.
__device__ void pp_inc_walk(const PpParams& p, const PpGraph& g, PpSplitWords& s, int* sh) {
  const int n_src = pp_sources(p, g, sh, [&](int n) { return p.g_dirty[p.g_wcc[n]] != 0; },
                               [&](int n) {
                                 const int id = g.t2[n];
                                 if (id >= 0 && atomicExch(&g.csize[id], 0) > 0) g.freel[atomicAdd(&s.n_free, 1)] = id;
                               });
  if (threadIdx.x == 0) {
    const PpRecord r = pp_run_walk(p, g, n_src, PpRecord{s.n_free, s.n_ids, 0, 0});
    s.n_free = r.n_free; s.n_ids = r.n_ids;
  }
  __syncthreads();
}

// (tree source position, sequence within the walk) of component c: what orders components of one size
__device__ __forceinline__ unsigned long long pp_tree_key(const PpGraph& g, int c) {
  return ((unsigned long long)(unsigned)g.ctree[c] << 32) | (unsigned)g.cseq[c];
}

// key(a) < key(b) in the reference's numbering: size, then tree source position, then sequence within the walk
__device__ __forceinline__ bool pp_key_less(const PpGraph& g, int a, int b) {
  if (g.csize[a] != g.csize[b]) return g.csize[a] < g.csize[b];
  if (g.ctree[a] != g.ctree[b]) return g.ctree[a] < g.ctree[b];
  return g.cseq[a] < g.cseq[b];
}

// First over-sized set of the numbering: the smallest key among components of more than num_cameras nodes; -1: none
__device__ int pp_first_oversized(const PpGraph& g, PpSplitWords& s) {
  if (threadIdx.x == 0) { s.min_size = 0x7fffffff; s.min_key = ~0ull; s.pick = -1; }
  __syncthreads();
  const int n_ids = s.n_ids;
  for (int c = threadIdx.x; c < n_ids; c += kPpThreads)
    if (g.csize[c] > g.cams) atomicMin(&s.min_size, g.csize[c]);
  __syncthreads();
  const int min_size = s.min_size;
  if (min_size == 0x7fffffff) return -1;
  for (int c = threadIdx.x; c < n_ids; c += kPpThreads)
    if (g.csize[c] == min_size) atomicMin(&s.min_key, pp_tree_key(g, c));
  __syncthreads();
  for (int c = threadIdx.x; c < n_ids; c += kPpThreads)
    if (g.csize[c] == min_size && pp_tree_key(g, c) == s.min_key) s.pick = c;
  __syncthreads();
  return s.pick;
}

// The number of component `id` = how many components precede it
__device__ int pp_number_of(const PpGraph& g, PpSplitWords& s, int id) {
  if (threadIdx.x == 0) s.count = 0;
  __syncthreads();
  const int n_ids = s.n_ids;
  for (int c = threadIdx.x; c < n_ids; c += kPpThreads)
    if (g.csize[c] > 0 && pp_key_less(g, c, id)) atomicAdd(&s.count, 1);
  __syncthreads();
  return s.count;
}

// Which over-sized component carries number `lab` now (-1: none)?  One wave per candidate counts the smaller keys.
__device__ int pp_carrier_of(const PpGraph& g, PpSplitWords& s, int lab) {
  int* over = g.t4;                                      // list of over-sized components (free outside the walks)
  if (threadIdx.x == 0) { s.n_over = 0; s.pick = -1; }
  __syncthreads();
  const int n_ids = s.n_ids;
  for (int c = threadIdx.x; c < n_ids; c += kPpThreads)
    if (g.csize[c] > g.cams) over[atomicAdd(&s.n_over, 1)] = c;
  __syncthreads();
  const int n_over = s.n_over, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = kPpThreads >> 6;
  for (int o = wave; o < n_over; o += n_waves) {
    const int id = over[o];
    int cnt = 0;
    for (int c = lane; c < n_ids; c += 64)
      if (g.csize[c] > 0 && pp_key_less(g, c, id)) ++cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0 && cnt == lab) s.pick = id;
  }
  __syncthreads();
  const int cur = s.pick;
  __syncthreads();                                       // everyone has it before the next search resets it
  return cur;
}

// One splitting step on component `cur`: drop every edge whose probability equals the minimum over the active edges
// touching cur, and mark the WCCs that lost one dirty (and only those).  false: no active edge touches cur.
__device__ bool pp_split_step(const PpParams& p, const PpGraph& g, PpSplitWords& s, int cur) {
  const int* comp = g.t2;
  if (threadIdx.x == 0) s.min_prob = 0xffffffffu;
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) p.g_dirty[n] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < g.a; i += kPpThreads)
    if (p.alive[i] && (comp[p.a_u[i]] == cur || comp[p.a_v[i]] == cur))
      atomicMin(&s.min_prob, __float_as_uint(p.a_p[i]));
  __syncthreads();
  const unsigned mn = s.min_prob;
  if (mn == 0xffffffffu) return false;
  for (int i = threadIdx.x; i < g.a; i += kPpThreads)
    if (p.alive[i] && __float_as_uint(p.a_p[i]) == mn) {
      pp_kill(p, g, i);
      p.g_dirty[p.g_wcc[p.a_u[i]]] = 1;
    }
  __syncthreads();
  return true;
}

// utils.py:54-123, tail recursion unrolled: pick the first over-sized set of the numbering; drop every edge whose
// probability equals the minimum over the active edges touching it; stay on the SAME NUMBER while the set that
// carries it after the renumbering is over-sized (reference quirk), else pick again.  Returns the status (0, 2, 3).
__device__ int pp_split(const PpParams& p, const PpGraph& g, int* sh, int& split_iters, int& walks) {
  __shared__ PpSplitWords s;
  if (threadIdx.x == 0) { s.n_free = 0; s.n_ids = 0; }
  pp_wcc(p, g);
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) { p.g_dirty[n] = 1; g.t2[n] = -1; g.csize[n] = 0; }
  __syncthreads();
  pp_inc_walk(p, g, s, sh);
  ++walks;
  for (;;) {
    int cur = pp_first_oversized(g, s);
    if (cur < 0) return 0;
    const int lab = pp_number_of(g, s, cur);
    while (cur >= 0) {
      if (!pp_split_step(p, g, s, cur)) return 2;        // cannot happen for a real component; never spin on it
      pp_inc_walk(p, g, s, sh);
      ++walks; ++split_iters;
      if (split_iters >= kPpMaxSplitIters) return 3;     // a resident workgroup must not run unbounded
      cur = pp_carrier_of(g, s, lab);
    }
  }
}

// Drop the dead edges from the active arrays (stable) once the cut / prune stages are over: the walks of the
// splitting loop then step over ~A_alive instead of A_in slots.  Dead edges get their prediction cleared here.
__device__ int pp_compact_alive(const PpParams& p, const PpGraph& g, int* sh) {
  int* pos = p.g_flags;
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) pos[i] = p.alive[i] ? 1 : 0;
  __syncthreads();
  const int kept = block_exclusive_scan(pos, g.a, sh);
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) {
    if (p.alive[i]) {
      const int k = pos[i];
      p.b_idx[k] = p.a_idx[i]; p.b_u[k] = p.a_u[i]; p.b_v[k] = p.a_v[i]; p.b_p[k] = p.a_p[i];
    } else {
      p.pred[p.a_idx[i]] = 0;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kept; k += kPpThreads) {
    p.a_idx[k] = p.b_idx[k]; p.a_u[k] = p.b_u[k]; p.a_v[k] = p.b_v[k]; p.a_p[k] = p.b_p[k];
    p.alive[k] = 1;
  }
  __syncthreads();
  return kept;
}

__global__ __launch_bounds__(kPpThreads) void pp_graph_kernel(PpParams p, int lds_nodes) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  __shared__ int sh[kPpThreads / 64 + 1];
  if (p.hdr[1]) {                                        // capacity exceeded: report, leave predictions = argmax
    if (threadIdx.x == 0) p.info[3] = 1;
    return;
  }
  PpGraph g;
  g.n = (int)p.n_nodes; g.a = p.hdr[0]; g.cams = p.num_cameras; g.lds_nodes = lds_nodes != 0;
  g.npad = ((size_t)g.n + 4) & ~(size_t)3;
  g.place_nodes(lds_nodes ? lds : p.g_node);
  unsigned* lds_csr = reinterpret_cast<unsigned*>(lds + (lds_nodes ? kPpNodeArrays * g.npad : 0));
  auto place_csr = [&]() {                               // by the current number of active edges
    const bool csr_in_lds = g.a <= kPpLdsEdges;
    g.csr = csr_in_lds ? lds_csr : p.g_csr;
    g.lds_walk = g.lds_nodes && csr_in_lds;
  };
  place_csr();
  pp_build_csr(p, g, sh);
  const bool cutting = p.flags & 1, pruning = p.flags & 2, splitting = p.flags & 4;
  int prune_rounds = 0, split_iters = 0, walks = 0, status = 0;
  if (cutting) pp_cut(p, g);
  if (pruning) prune_rounds = pp_prune(p, g);
  if (cutting) pp_cut(p, g);
  if (cutting || pruning) {
    g.a = pp_compact_alive(p, g, sh);
    place_csr();
    pp_build_csr(p, g, sh);
  }
  if (splitting) status = pp_split(p, g, sh, split_iters, walks);
  const int n_sets = pp_scc(p, g, sh);                   // the reference's final numbering
  ++walks;
  // outputs
  int alive_cnt = 0;
  for (int i = threadIdx.x; i < g.a; i += kPpThreads) {
    if (p.alive[i]) ++alive_cnt; else p.pred[p.a_idx[i]] = 0;
  }
  for (int n = threadIdx.x; n < g.n; n += kPpThreads) p.id_pred[n] = g.label[n];
  __shared__ int s_alive;
  if (threadIdx.x == 0) s_alive = 0;
  __syncthreads();
  atomicAdd(&s_alive, alive_cnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    p.info[1] = s_alive; p.info[2] = n_sets; p.info[3] = status ? status : (p.hdr[3] ? 4 : 0); p.info[4] = split_iters; p.info[5] = walks;
    p.info[6] = prune_rounds; p.info[7] = p.hdr[2];
  }
}

// ------------------------------------------------------------------------------------------------
// The workspace, buffer by buffer, each on a 256-byte boundary; from p.n_nodes, p.n_edges and max_active.  Sets p.cap
// and returns the total; given a base pointer it also fills p's workspace fields.
static size_t pp_carve(PpParams& p, int64_t max_active, char* ws) {
  p.cap = (max_active > 0 && max_active < p.n_edges) ? max_active : p.n_edges;
  if (p.cap < 1) p.cap = 1;
  const size_t cap = (size_t)p.cap, nodes = (size_t)p.n_nodes + 4;
  const int64_t nb = (p.n_edges + kPpChunk - 1) / kPpChunk;
  size_t off = 0;
  auto take = [&](auto*& field, size_t count) {
    if (ws) field = reinterpret_cast<decltype(field + 0)>(ws + off);
    off = (off + count * sizeof(*field) + 255) / 256 * 256;
  };
  take(p.hdr, 16); take(p.block_count, (size_t)(nb > 0 ? nb : 1));
  take(p.a_idx, cap); take(p.a_u, cap); take(p.a_v, cap); take(p.a_p, cap); take(p.a_slot, cap);
  take(p.alive, cap); take(p.mark, cap);
  take(p.g_node, kPpNodeArrays * nodes); take(p.g_csr, cap); take(p.g_flags, 2 * cap);
  take(p.b_idx, cap); take(p.b_u, cap); take(p.b_v, cap); take(p.b_p, cap);
  take(p.g_wcc, nodes); take(p.g_dirty, nodes);
  return off;
}

static size_t pp_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t max_active) {
  PpParams p;
  p.n_nodes = n_nodes; p.n_edges = n_edges;
  return pp_carve(p, max_active, nullptr);
}

static int launch_postprocess(const float* logits, const int64_t* row, const int64_t* col, int64_t idx_stride, int64_t n_nodes,
                              int64_t n_edges, int num_cameras, int flags, int64_t max_active, float* prob1, int64_t* pred,
                              int64_t* id_pred, int32_t* info, void* workspace, size_t workspace_bytes, hipStream_t s) {
  PpParams p;
  p.logits = logits; p.row = row; p.col = col; p.idx_stride = idx_stride; p.n_nodes = n_nodes; p.n_edges = n_edges;
  p.num_cameras = num_cameras; p.flags = flags; p.prob1 = prob1; p.pred = pred; p.id_pred = id_pred; p.info = info;
  using mtmc_api::fail;
  const size_t need = pp_carve(p, max_active, nullptr);
  if (workspace_bytes < need)
    return fail(MTMC_E_WORKSPACE, "postprocess: workspace has %zu bytes, %zu needed (mtmc_postprocess_workspace_bytes)",
                workspace_bytes, need);
  pp_carve(p, max_active, static_cast<char*>(workspace));
  const int nb = (int)((n_edges + kPpChunk - 1) / kPpChunk);
  if (nb > 0) hipLaunchKernelGGL(pp_classify_kernel, dim3(nb), dim3(256), 0, s, p);
  hipLaunchKernelGGL(pp_scan_kernel, dim3(1), dim3(1024), 0, s, p, nb);
  if (nb > 0) hipLaunchKernelGGL(pp_compact_kernel, dim3(nb), dim3(256), 0, s, p);
  const int lds_nodes = n_nodes <= kPpLdsNodes ? 1 : 0;
  const size_t npad = ((size_t)n_nodes + 4) & ~(size_t)3;
  const size_t lds = (lds_nodes ? kPpNodeArrays * npad * sizeof(int) : 0) + (size_t)kPpLdsEdges * sizeof(unsigned);
  if (!allow_big_lds(reinterpret_cast<const void*>(pp_graph_kernel), (kPpNodeArrays * (kPpLdsNodes + 4) + kPpLdsEdges) * 4))
    return fail(MTMC_E_HIP, "postprocess: HIP refused the graph kernel's dynamic LDS size");
  hipLaunchKernelGGL(pp_graph_kernel, dim3(1), dim3(kPpThreads), lds, s, p, lds_nodes);
  return mtmc_api::launched("postprocess");
}

}  // namespace mtmc

extern "C" {

size_t mtmc_postprocess_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t max_active) {
  if (n_nodes < 1 || n_edges < 0 || n_nodes >= (1ll << 31) || n_edges >= (1ll << 31)) return 0;
  return mtmc::pp_workspace_bytes(n_nodes, n_edges, max_active);
}

int32_t mtmc_postprocess(const float* logits, const int64_t* row, const int64_t* col, int64_t idx_stride,
                         int64_t n_nodes, int64_t n_edges, int32_t num_cameras, int32_t flags, int64_t max_active,
                         float* prob1, int64_t* predictions, int64_t* id_pred, int32_t* info,
                         void* workspace, size_t workspace_bytes, void* stream) {
  using mtmc_api::fail;
  if (n_nodes < 1 || n_edges < 0 || n_nodes >= (1ll << 31) || n_edges >= (1ll << 31) || num_cameras < 1)
    return fail(MTMC_E_ARG, "postprocess: n_nodes must be in [1, 2^31), n_edges in [0, 2^31) and num_cameras >= 1");
  if (!prob1 || !predictions || !id_pred || !info || !workspace || (n_edges > 0 && (!row || !col)))
    return fail(MTMC_E_ARG, "postprocess: NULL prob1, predictions, id_pred, info or workspace, or NULL row or col with n_edges > 0");
  if (idx_stride < 1) return fail(MTMC_E_ARG, "postprocess: idx_stride must be >= 1");
  if (((uintptr_t)workspace & 255) || (logits && ((uintptr_t)logits & 7)))
    return fail(MTMC_E_ARG, "postprocess: the workspace must be 256-byte and logits 8-byte aligned");
  return mtmc::launch_postprocess(logits, row, col, idx_stride, n_nodes, n_edges, num_cameras, flags, max_active, prob1,
                                  predictions, id_pred, info, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
