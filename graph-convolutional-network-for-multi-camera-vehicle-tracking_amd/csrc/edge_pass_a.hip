// Pass A of a message-passing round: z1 = We.[h[row]|h[col]|e] + be of every edge, stored, and its BatchNorm statistics
// (EdgeModel, mpn.py:67-69) -- in edge order (pass_a_kernel) or by column blocks (pass_a_blocked_kernel).  edge_prep.hip has
// the overview of the per-edge units.
#include "edge_common.h"

#include <type_traits>

namespace mtmc {

// ------------------------------------------------------------------------------------------------
// z1 of one edge: Pr[row] + Pc[col] + We_e . e_in + be
// ------------------------------------------------------------------------------------------------
// The small constants every edge needs in pass A -- the two edge-encoder layers with their BatchNorm affines (first round /
// reattached edges: e0 is recomputed from the 8-byte attributes, never stored) and the edge-update weights: 68 floats in
// the first round, 84 with reattached edges.  As uniform (scalar) operands they did not all fit the SGPR file (105-160
// spills, each a v_readlane in the loop: the first round's launch took 220 us at config 4 against 133 us for the later
// rounds, which move MORE bytes); all in vector registers they cost two waves per SIMD of occupancy.  So they are SPLIT:
// the hidden layer (20 floats) and, without reattached edges, the 4 x 4 update weights (20) stay scalar -- read through
// uniform pointers --, the output layer (28) and the 4 x 8 update weights of the reattached forms (36) are staged once per
// workgroup in LDS and read back by every lane: a load from LDS lands in a VGPR and stays there.
// Same arithmetic, same order as edge_enc_hidden / edge_enc_out (common.h).
struct EdgeConstsV {                       // the LDS-staged (vector-register) part
  float w2[4][4], b2[4], s2[4], t2[4];     // output layer of the edge encoder
  float uw[4][8], ub[4];                   // reattached forms only: [W_e0 | W_e] columns of the edge update, bias
};
constexpr int kEdgeConstsV = sizeof(EdgeConstsV) / sizeof(float);
struct EdgeConstsS {                       // the scalar part: copied out of memory ONCE, before the edge loop -- read through
  float w1[4][2], b1[4], s1[4], t1[4];     // the parameter pointers inside the loop they would be re-fetched after every z1
  float uw[4][4], ub[4];                   // store (which may alias them as far as the compiler knows)
};
template <int MODE>
__device__ __forceinline__ void load_edge_consts_s(const RoundParams& p, EdgeConstsS& k) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    k.w1[i][0] = MODE != 0 ? p.enc.w1[i * p.enc.fe] : 0.f;
    k.w1[i][1] = (MODE != 0 && p.enc.fe > 1) ? p.enc.w1[i * p.enc.fe + 1] : 0.f;
    k.b1[i] = MODE != 0 ? p.enc.b1[i] : 0.f;
    k.s1[i] = MODE != 0 ? p.enc.aff[i] : 0.f;            // p.enc.aff = s1[4] | t1[4] | s2[4] | t2[4] (EdgeEncAffine)
    k.t1[i] = MODE != 0 ? p.enc.aff[4 + i] : 0.f;
    k.ub[i] = (MODE & 2) ? 0.f : p.ue_b[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) k.uw[i][j] = (MODE & 2) ? 0.f : p.ue_w[i * p.ue_ld + p.ue_eoff + j];
  }
}

// whole block; ends with a barrier.  MODE as in pass_a_kernel.
template <int MODE>
__device__ __forceinline__ void stage_edge_consts(const RoundParams& p, EdgeConstsV* cs) {
  float* dst = reinterpret_cast<float*>(cs);
  if (MODE != 0) {
    for (int i = threadIdx.x; i < kEdgeConstsV; i += blockDim.x) {
      float v;
      if (i < 16) v = p.enc.w2[i];
      else if (i < 20) v = p.enc.b2[i - 16];
      else if (i < 28) v = p.enc.aff[8 + i - 20];                                  // s2[4] | t2[4] of EdgeEncAffine
      else if (i < 60) v = (MODE & 2) ? p.ue_w[((i - 28) >> 3) * p.ue_ld + p.ue_eoff + ((i - 28) & 7)] : 0.f;
      else v = p.ue_b[i - 60];
      dst[i] = v;
    }
  }
  __syncthreads();
}

struct PrevAffine { float s[4], t[4]; };   // BatchNorm affine of the previous round's z1 (lazy e')

// z1 of one edge: Pr[row] + Pc[col] + We_e . e_in + be.
// MODE 0: a later round without reattached edges (no attribute loads, no edge-encoder arithmetic, 4 x 4 weights);
// bit 0: first round, bit 1: reattach_initial_edges.
// Loads and arithmetic are separate steps so that a thread's kEPT edges have ALL their loads in flight before the first
// result is stored (the z1 store may alias every input as far as the compiler can tell: interleaved, each edge's load
// chain would start only after the previous edge's store).
struct EdgeIn { float4 pr, pc, ev; float a0, a1; };
template <int MODE>
__device__ __forceinline__ void edge_load_rc(const RoundParams& p, int64_t e, int r, int col, EdgeIn& in);
template <int MODE>
__device__ __forceinline__ void edge_load(const RoundParams& p, int64_t e, EdgeIn& in) {
#if PA_NT & 1
  const int r = __builtin_nontemporal_load(p.row32 + e), col = __builtin_nontemporal_load(p.col32 + e);
#else
  const int r = p.row32[e], col = p.col32[e];
#endif
  edge_load_rc<MODE>(p, e, r, col, in);
}
// ... with the row / column ids in hand (the column-blocked traversal knows the row without loading it)
template <int MODE>
__device__ __forceinline__ void edge_load_rc(const RoundParams& p, int64_t e, int r, int col, EdgeIn& in) {
  // P = [Pr: N x 4 | Pc: N x 4]: the randomly gathered half is a compact 16 B/node table (four nodes per 64-byte sector)
  in.pr = *reinterpret_cast<const float4*>(p.P + (int64_t)r * 4);
  in.pc = *reinterpret_cast<const float4*>(p.P + ((int64_t)p.n_nodes + col) * 4);
  in.a0 = in.a1 = 0.f;
  in.ev = make_float4(0.f, 0.f, 0.f, 0.f);
  if (MODE == 1 && (PA_NT & 8)) load_attr_nt(p.attr, p.enc.fe, e, in.a0, in.a1);   // first round, no reattachment: the last reader
  else if (MODE != 0) load_attr(p.attr, p.enc.fe, e, in.a0, in.a1);
#if PA_NT & 2
  if (!(MODE & 1)) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p.e_prev) + e);
    in.ev = make_float4(v[0], v[1], v[2], v[3]);
  }
#else
  if (!(MODE & 1)) in.ev = reinterpret_cast<const float4*>(p.e_prev)[e];
#endif
}

template <int MODE, bool DROP>
__device__ __forceinline__ void edge_z1(const RoundParams& p, const EdgeConstsS& ks, const EdgeConstsV& c,
                                        const PrevAffine& pa, int64_t e, const EdgeIn& in, float (&z)[4]) {
  constexpr bool first_round = (MODE & 1) != 0, reattach = (MODE & 2) != 0;
  float e0[4] = {0, 0, 0, 0}, ep[4];
  if (first_round || reattach) {
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                       // edge_enc_hidden, scalar operands (edge_in_dim 1: w1[k][1] = a1 = 0)
      const float zz = fmaf(ks.w1[k][1], in.a1, ks.b1[k] + ks.w1[k][0] * in.a0);
      u[k] = fmaxf(fmaf(zz, ks.s1[k], ks.t1[k]), 0.f);
    }
    if (DROP) drop_apply4(p.enc.drop, kDropEncEdge1, (unsigned long long)e * 4, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {                       // edge_enc_out
      float zz = c.b2[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) zz = fmaf(c.w2[k][j], u[j], zz);
      e0[k] = fmaxf(fmaf(zz, c.s2[k], c.t2[k]), 0.f);
    }
    if (DROP) drop_apply4(p.enc.drop, kDropEncEdge2, (unsigned long long)e * 4, e0);
  }
  if (first_round) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ep[j] = e0[j];
  } else {
    ep[0] = in.ev.x; ep[1] = in.ev.y; ep[2] = in.ev.z; ep[3] = in.ev.w;
    if (p.lazy_e) {                               // the buffer holds the previous round's z1: e' = relu(bn(z1))
#pragma unroll
      for (int j = 0; j < 4; ++j) ep[j] = fmaxf(fmaf(ep[j], pa.s[j], pa.t[j]), 0.f);
    }
  }
  const float prv[4] = {in.pr.x, in.pr.y, in.pr.z, in.pr.w}, pcv[4] = {in.pc.x, in.pc.y, in.pc.z, in.pc.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (reattach) {
      float acc = prv[k] + pcv[k] + c.ub[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(c.uw[k][j], e0[j], acc);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(c.uw[k][4 + j], ep[j], acc);
      z[k] = acc;
    } else {                                            // 4 x 4 weights + bias: scalar operands
      float acc = prv[k] + pcv[k] + ks.ub[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(ks.uw[k][j], ep[j], acc);
      z[k] = acc;
    }
  }
}

// What both pass-A kernels do before their loop: the previous round's BatchNorm affine (lazy e'), the LDS-staged constants,
// and per-lane copies of both.  Whole block; a barrier inside.  red: double[8] at least.
template <int MODE>
__device__ __forceinline__ void pass_a_consts(const RoundParams& p, EdgeConstsV* cs_s, PrevAffine* pa_s, double* red,
                                              PrevAffine& pa, EdgeConstsV& c) {
  if (p.lazy_e && !(MODE & 1)) {
    stat_gather(p.prev_stats + kRoundZ1Off, 8, kZ1Stride, red);
    __syncthreads();
    if (threadIdx.x < 4)
      bn_affine(red[threadIdx.x], red[4 + threadIdx.x], p.e_total, p.ue_g[threadIdx.x], p.ue_bt[threadIdx.x],
                pa_s->s[threadIdx.x], pa_s->t[threadIdx.x]);
  }
  stage_edge_consts<MODE>(p, cs_s);                // (barrier inside: pa_s is visible too)
#pragma unroll
  for (int j = 0; j < 4; ++j) { pa.s[j] = pa_s->s[j]; pa.t[j] = pa_s->t[j]; }
  const float* src = reinterpret_cast<const float*>(cs_s);      // per-lane copy: VGPRs (only the fields MODE uses survive)
  float* dst = reinterpret_cast<float*>(&c);
#pragma unroll
  for (int i = 0; i < kEdgeConstsV; ++i) dst[i] = MODE != 0 ? src[i] : 0.f;
}

// z1 of edge e goes to memory (streamed or not: block-uniform) ...
// The random 16-byte P[col] gather is what bounds this pass (one cache line per lane): do it once and hand z1 to pass B
// through memory instead of gathering again there
__device__ __forceinline__ void store_z1(const RoundParams& p, int64_t e, const float (&z)[4]) {
  if ((PA_NT & 4) || p.stream_z1) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    f4v zv = {z[0], z[1], z[2], z[3]};
    __builtin_nontemporal_store(zv, reinterpret_cast<f4v*>(p.e_buf) + e);
  } else {
    reinterpret_cast<float4*>(p.e_buf)[e] = make_float4(z[0], z[1], z[2], z[3]);
  }
}
// ... and, where `ok`, into the thread's fp64 sums of z1 and z1^2
__device__ __forceinline__ void add_z1(const float (&z)[4], bool ok, double (&acc)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float zk = ok ? z[k] : 0.f;
    acc[k] += zk;
    acc[4 + k] += (double)zk * zk;
  }
}

// kEPT = edges per thread and loop trip in passes A/B: four independent load chains in flight on big graphs, one on
// small ones, where filling the 256 CUs with waves matters more (pick_ept).  DROP: the edge encoder's Dropout is compiled
// in (training); eval-mode kernels carry neither its hash arithmetic nor its scalar operands.

template <int kEPT, int MODE, bool DROP>
__global__ __launch_bounds__(256, (MODE == 0 ? 5 : 1)) void pass_a_kernel(RoundParams p) {   // plain later round: <= 96 VGPRs
  if (DROP) drop_resolve(p.enc.drop);
  __shared__ EdgeConstsV cs_s;
  __shared__ double red[8 * 4];
  __shared__ PrevAffine pa_s;
  EdgeConstsS ks;                                  // first thing in the kernel: ahead of every store and barrier these
  load_edge_consts_s<MODE>(p, ks);                 // uniform loads are scalar loads (SGPRs); behind one they become vector loads
  if (p.col_blocks > 0 && p.flags[0] == 0 && p.flags[2] == 0) return;   // pass_a_blocked_kernel, launched just before, did this round
  EK_T(MODE == 0 ? 1 : 2, 0);
  PrevAffine pa;
  EdgeConstsV c;
  pass_a_consts<MODE>(p, &cs_s, &pa_s, red, pa, c);
  EK_T(MODE == 0 ? 1 : 2, 1);
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto finish = [&](int64_t e, const EdgeIn& in) {
    float z[4];
    edge_z1<MODE, DROP>(p, ks, c, pa, e, in, z);
    store_z1(p, e, z);
    add_z1(z, true, acc);
  };
  // whole tiles of 256 * kEPT edges without a bounds check per edge (no exec-mask bookkeeping in the hot loop) ...
  constexpr int64_t kTile = 256 * kEPT;
  const int64_t n_full = p.n_edges / kTile;
  for (int64_t t = blockIdx.x; t < n_full; t += gridDim.x) {
    const int64_t base = t * kTile + threadIdx.x;
    EdgeIn in[kEPT];
#pragma unroll
    for (int i = 0; i < kEPT; ++i) edge_load<MODE>(p, base + i * 256, in[i]);
#pragma unroll
    for (int i = 0; i < kEPT; ++i) finish(base + i * 256, in[i]);
  }
  // ... and the last, partial tile: one 256-edge piece per block
  for (int i = blockIdx.x; i < kEPT; i += gridDim.x) {
    const int64_t e = n_full * kTile + (int64_t)i * 256 + threadIdx.x;
    if (e < p.n_edges) {
      EdgeIn in;
      edge_load<MODE>(p, e, in);
      finish(e, in);
    }
  }
  EK_T(MODE == 0 ? 1 : 2, 2);
  block_atomic_add<8>(acc, p.stats + kRoundZ1Off, kZ1Stride, red);
  EK_T(MODE == 0 ? 1 : 2, 3);
}

// ------------------------------------------------------------------------------------------------
// Pass A by COLUMN BLOCKS (graphs whose Pc table outgrows an XCD's 4 MB L2: config 5, N = 1M -> 16 MB).
// In edge order every 16-byte Pc[col] gather of such a graph misses the L2 and fetches a 64-byte sector of its own from the
// Infinity Cache: 6.1 GB fetched for 2.4 GB of algorithmic reads per launch, 1.85 ms.  A row-sorted list
// with ascending columns inside a row (the reference's lists are: inference.py:407-413 builds them as cartesian products
// of ascending node lists) is also sorted by column INSIDE every row, so the edges of row i whose column falls into block b
// are one contiguous sub-run [sub[i][b], sub[i][b+1]).  colblock_index_kernel finds the B - 1 inner boundaries of every row
// once per forward (binary searches inside the row's own column segment); pass_a_blocked_kernel then walks
// (256-row chunk) x (column block) pieces, the block bound to blockIdx % 8 -- under round-robin placement one XCD, whose L2
// then serves all gathers from a 2 MB slice of Pc (placement changes speed only).  Per wave: 64 rows' sub-run lengths ->
// inclusive scan -> every lane takes slots k, k + 64, ... of the wave's concatenated sub-runs and finds its row by a 6-step
// binary search over the scan in LDS.  z1 lands where it always does (edge order in memory is unchanged), so passes B / C and
// the next round are untouched.  prep_kernel's flags decide on the device: unsorted rows or columns -> this kernel returns
// and pass_a_kernel, launched behind it, does the round (and vice versa).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colblock_index_kernel(const int* __restrict__ col32, const int* __restrict__ row_start,
                                                             const int* __restrict__ deg, const int* __restrict__ flags,
                                                             int64_t row_lo, int64_t row_hi, int B, int blk_nodes,
                                                             int* __restrict__ sub) {
  if (flags[0] != 0 || flags[2] != 0) return;
  const int64_t n_items = (row_hi - row_lo) * (B + 1);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * 256) {
    const int64_t r = row_lo + i / (B + 1);
    const int b = (int)(i % (B + 1));
    const int d = deg[r];
    int pos = 0;
    if (d > 0) {
      const int s0 = row_start[r];
      if (b == 0) pos = s0;
      else if (b == B) pos = s0 + d;
      else {                                                 // first edge of the row with col >= b * blk_nodes
        const int want = b * blk_nodes;
        int lo = s0, hi = s0 + d;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (col32[mid] < want) lo = mid + 1; else hi = mid;
        }
        // Inner boundaries snap DOWN to a multiple of four edges = one 64-byte sector of the 16-byte-per-edge streams (z1 in and
        // out): a sector is then read and written by ONE column block, i.e. one XCD -- unsnapped, the first and last sector of
        // every ~200-byte sub-run were shared with the neighbouring block on another XCD, fetched twice and written in two
        // partial pieces.  The <= 3 edges this moves into the neighbour's block gather from the neighbour's slice of Pc (a miss
        // in this XCD's L2, nothing else); monotone boundaries stay monotone under rounding.
        pos = lo & ~3;
        pos = pos < s0 ? s0 : pos;
      }
    }
    sub[(r - row_lo) * (B + 1) + b] = pos;                   // (a row without edges: all zeros -> empty sub-runs)
  }
}

template <int MODE>
__global__ __launch_bounds__(256, (MODE == 0 ? 4 : 1)) void pass_a_blocked_kernel(RoundParams p, const int* __restrict__ sub,
                                                                                  int B, int64_t row_lo, int64_t row_hi) {
  __shared__ EdgeConstsV cs_s;
  __shared__ double red[8 * 4];
  __shared__ PrevAffine pa_s;
  __shared__ int pre_s[4][64], base_s[4][64];
  EdgeConstsS ks;
  load_edge_consts_s<MODE>(p, ks);
  if (p.flags[0] != 0 || p.flags[2] != 0) return;   // unsorted rows / columns: pass_a_kernel does this round (block-uniform)
  PrevAffine pa;
  EdgeConstsV c;
  pass_a_consts<MODE>(p, &cs_s, &pa_s, red, pa, c);
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // column block of this workgroup: blockIdx % 8 picks the XCD-bound residue, the next bits the block among that XCD's B / 8
  const int per_xcd = B >> 3;
  const int b = (int)(blockIdx.x & 7) + 8 * (int)((blockIdx.x >> 3) % per_xcd);
  const int64_t group = (blockIdx.x >> 3) / per_xcd, n_groups = (gridDim.x >> 3) / per_xcd;
  const int64_t n_chunks = (row_hi - row_lo + 255) / 256;
  constexpr int U = 4;                              // slots per lane and trip: four independent load chains in flight
  // a lane's row of the chunk: its sub-run [s0, s0 + len) of column block b.  The NEXT chunk's pair is requested before this
  // chunk's edges are walked (a dependent global load at the head of every ~800-edge chunk would idle the wave for its latency)
  auto sub_of = [&](int64_t chunk, int& s0, int& len) {
    const int64_t r = row_lo + chunk * 256 + w * 64 + lane;
    s0 = 0; len = 0;
    if (chunk < n_chunks && r < row_hi) {
      const int* sb = sub + (r - row_lo) * (B + 1) + b;
      s0 = sb[0];
      len = sb[1] - s0;
    }
  };
  int s0_n, len_n;
  sub_of(group, s0_n, len_n);
  for (int64_t chunk = group; chunk < n_chunks; chunk += n_groups) {
    const int64_t r0 = row_lo + chunk * 256 + w * 64;          // this wave's 64 rows
    const int s0 = s0_n, len = len_n;
    sub_of(chunk + n_groups, s0_n, len_n);
    int incl = len;                                   // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    const int total = __builtin_amdgcn_readlane(incl, 63);
    pre_s[w][lane] = incl;
    base_s[w][lane] = s0 - (incl - len);              // edge index of slot k inside this row's sub-run: base + k
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // Branch-free up to the stores: slots past the wave's total are clamped to its last slot (loaded and computed again,
    // never stored or counted), so that the UU searches, then the UU column loads, then the UU x 3 data loads are each in
    // flight together -- behind a per-slot `if` every slot's chain (search -> column id -> gather) would run after the
    // previous one's.  Whole trips of U x 64 slots take UU = U; what is left takes single 64-slot trips (a wave's ~800 slots
    // are 3 whole trips + 32: one clamped trip of four would redo a fifth of the work).
    auto trip = [&](int k0, auto uu_tag) {
      constexpr int UU = decltype(uu_tag)::value;
      EdgeIn in[UU];
      int64_t ee[UU];
      int rw[UU], cl[UU];
      bool ok[UU];
#pragma unroll
      for (int u = 0; u < UU; ++u) {
        int k = k0 + u * 64 + lane;
        ok[u] = k < total;
        k = ok[u] ? k : total - 1;
        int j = 0;                                    // first row of the wave whose inclusive count exceeds k
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
          if (pre_s[w][j + step - 1] <= k) j += step;
        ee[u] = (int64_t)base_s[w][j] + k;
        rw[u] = (int)(r0 + j);
      }
#pragma unroll
      for (int u = 0; u < UU; ++u) {
#if PA_NT & 1
        cl[u] = __builtin_nontemporal_load(p.col32 + ee[u]);
#else
        cl[u] = p.col32[ee[u]];
#endif
      }
#pragma unroll
      for (int u = 0; u < UU; ++u) edge_load_rc<MODE>(p, ee[u], rw[u], cl[u], in[u]);
#pragma unroll
      for (int u = 0; u < UU; ++u) {
        float z[4];
        edge_z1<MODE, false>(p, ks, c, pa, ee[u], in[u], z);
        if (ok[u]) store_z1(p, ee[u], z);
        add_z1(z, ok[u], acc);
      }
    };
    int k0 = 0;
    for (; k0 + 64 * U <= total; k0 += 64 * U) trip(k0, std::integral_constant<int, U>());
    for (; k0 < total; k0 += 64) trip(k0, std::integral_constant<int, 1>());
    __builtin_amdgcn_wave_barrier();                  // (the next chunk overwrites this wave's LDS rows)
  }
  block_atomic_add<8>(acc, p.stats + kRoundZ1Off, kZ1Stride, red);
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
#ifndef MTMC_PASS_A_EPT
#define MTMC_PASS_A_EPT 4
#endif
constexpr int kPassAEpt = MTMC_PASS_A_EPT;
template <int MODE>
static void launch_pass_a_mode(const RoundParams& p, hipStream_t s) {
  // (edges per thread 1/2/4/8 x grid caps 1536..16384 swept at config 4: 0.45-0.51 ms for the three launches, flat)
  if (p.enc.drop.on) {            // training (the encoder's Dropout compiled in): graphs are small, one edge per thread
    hipLaunchKernelGGL((pass_a_kernel<1, MODE, true>), dim3(edge_grid(p.n_edges, 256)), dim3(256), 0, s, p);
    return;
  }
  switch (pick_ept(p.n_edges)) {
    case 1: hipLaunchKernelGGL((pass_a_kernel<1, MODE, false>), dim3(edge_grid(p.n_edges, 256)), dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((pass_a_kernel<kPassAEpt, MODE, false>), dim3(edge_grid(p.n_edges, 256 * kPassAEpt)), dim3(256), 0, s, p);
  }
}
// Column-blocked pass A: when, and with how many blocks.  Only where the gathered table cannot live in an XCD's L2 anyway
// (N * 16 B > 3 MB), on many-edge eval-mode lists whose sub-runs stay long enough to pay for their bookkeeping (average
// degree >= 4 per column block).  Blocks of <= 2 MB of Pc, a multiple of 8 (one residue of blockIdx % 8 per block), <= 64.
int plan_col_blocks(int64_t n_nodes, int64_t n_edges, double avg_degree, bool training) {
  const Knobs& kn = knobs();
  if (kn.no_col_blocks || training || n_edges <= kSmallEdges || n_nodes * 16 <= (int64_t)3 << 20 || n_nodes >= (1ll << 31) - 64) return 0;
  int64_t B = (n_nodes * 16 + ((int64_t)2 << 20) - 1) / ((int64_t)2 << 20);
  B = (B + 7) / 8 * 8;
  if (B > 64) B = 64;
  if (kn.col_blocks >= 8 && kn.col_blocks <= 64 && kn.col_blocks % 8 == 0) B = kn.col_blocks;
  return avg_degree >= 4.0 * (double)B ? (int)B : 0;
}
void launch_colblock_index(const RoundParams& p, int* sub, int B, int64_t row_lo, int64_t row_hi, hipStream_t s) {
  if (B <= 0 || row_hi <= row_lo) return;
  const int blk_nodes = (int)((p.n_nodes + B - 1) / B);
  const int64_t items = (row_hi - row_lo) * (B + 1), blocks = (items + 255) / 256;
  hipLaunchKernelGGL(colblock_index_kernel, dim3((int)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, s, p.col32, p.row_start, p.deg,
                     p.flags, row_lo, row_hi, B, blk_nodes, sub);
}
template <int MODE>
static void launch_pass_a_blocked_mode(const RoundParams& p, hipStream_t s) {
  const int B = p.col_blocks;
  const int64_t n_chunks = (p.cb_row_hi - p.cb_row_lo + 255) / 256;
  int64_t groups = 1024 / B;                         // 1024 workgroups: four per CU
  if (groups > n_chunks) groups = n_chunks;
  if (groups < 1) groups = 1;
  hipLaunchKernelGGL((pass_a_blocked_kernel<MODE>), dim3((unsigned)(groups * B)), dim3(256), 0, s, p, p.col_sub, B, p.cb_row_lo, p.cb_row_hi);
}
void launch_pass_a(const RoundParams& p0, hipStream_t s) {
  RoundParams p = p0;
  if (p.col_blocks > 0 && p.enc.drop.on) p.col_blocks = 0;
  // z1 (16 B / edge) is read by pass B, pass C and the next pass A: stored with the default policy it waits for them in the
  // 256 MB Infinity Cache; a z1 that does not fit there only pushes everything else out on its way (config 5: -2 % on the
  // edge passes with a streaming store, config 4: +2 %)
  p.stream_z1 = p.n_edges * 16 > (int64_t)256 << 20;
  if (p.col_blocks > 0) {                    // (returns at once on unsorted rows / columns; pass_a_kernel then does the round)
    switch ((p.first_round ? 1 : 0) | (p.reattach_edges ? 2 : 0)) {
      case 0: launch_pass_a_blocked_mode<0>(p, s); break;
      case 1: launch_pass_a_blocked_mode<1>(p, s); break;
      case 2: launch_pass_a_blocked_mode<2>(p, s); break;
      default: launch_pass_a_blocked_mode<3>(p, s);
    }
  }
  switch ((p.first_round ? 1 : 0) | (p.reattach_edges ? 2 : 0)) {
    case 0: launch_pass_a_mode<0>(p, s); break;
    case 1: launch_pass_a_mode<1>(p, s); break;
    case 2: launch_pass_a_mode<2>(p, s); break;
    default: launch_pass_a_mode<3>(p, s);
  }
}
int plan_edges_per_thread(int64_t n_edges) { return pick_ept(n_edges); }

#if EK_STAMP
int ek_stamps_pass_a(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ek), sizeof(g_ek)); }
#endif

}  // namespace mtmc
