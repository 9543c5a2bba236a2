// Pass C of a message-passing round: m = relu(bn(Wn.[h[row]|e'] + bn)); h' = agg_row(m); logits (NodeModel, mpn.py:97-99), as
// the half-wave walk (pass_c_kernel) and two matrix-core kernels (any row order / sorted rows).  edge_prep.hip has the overview
// of the per-edge units; kernels.h (PassC) names the combinations a call can take.
#include "edge_common.h"

namespace mtmc {

// ------------------------------------------------------------------------------------------------
// pass C: 32 lanes = 32 channels; every half-wave walks 32 consecutive edges of the block's tile
// ------------------------------------------------------------------------------------------------

// Order-independent aggregation for row-sorted lists (MTMC_F_DETERMINISTIC): a 32-edge chunk's first run goes to
// carry[chunk][0], its last run (if different) to carry[chunk][1], runs strictly inside the chunk are complete rows
// and are stored directly; agg_fixup_kernel then adds each row's pieces in chunk order.  slot: 0 / 1 / -1 (inside).
__device__ __forceinline__ void flush_run(const RoundParams& p, bool det, int64_t chunk, int slot, int node, int k,
                                          float acc);

__device__ __forceinline__ void flush_node(const RoundParams& p, int node, int k, float acc) {
  float* dst = p.h_acc + (int64_t)node * kH + k;
  if (p.agg == 2) {
    atomicMax(reinterpret_cast<int*>(dst), __float_as_int(acc));   // values are >= 0: int order == float order
  } else {
    unsafeAtomicAdd(dst, acc);
  }
}

__device__ __forceinline__ void flush_run(const RoundParams& p, bool det, int64_t chunk, int slot, int node, int k,
                                          float acc) {
  if (!det) { flush_node(p, node, k, acc); return; }
  if (slot < 0) p.h_acc[(int64_t)node * kH + k] = acc;
  else p.carry[(chunk * 2 + slot) * kH + k] = acc;
}

__global__ __launch_bounds__(256) void agg_fixup_kernel(RoundParams p) {
  if (p.flags[0] != 0) return;                       // unsorted rows: pass C used atomics, nothing to add up
  const int k = threadIdx.x & 31;
  const int64_t stride = (int64_t)gridDim.x * 8;
  for (int64_t i = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); i < p.n_nodes; i += stride) {
    const int d = p.deg[i];
    if (d == 0) continue;
    const int64_t s = p.row_start[i], t = s + d, len = p.det_len;      // len: edges per carry chunk (walk: 32; sorted: a span)
    const int64_t cs = s / len, ce = (t - 1) / len;
    float v;
    if (cs == ce) {
      if (s % len == 0) v = p.carry[(cs * 2 + 0) * kH + k];
      else if (t % len == 0 || t == p.n_edges) v = p.carry[(cs * 2 + 1) * kH + k];
      else continue;                                 // strictly inside its chunk: already stored
    } else {
      v = p.carry[(cs * 2 + (s % len == 0 ? 0 : 1)) * kH + k];
      for (int64_t c = cs + 1; c <= ce; ++c) v += p.carry[(c * 2 + 0) * kH + k];
    }
    p.h_acc[i * kH + k] = v;
  }
}

// What every pass-C kernel needs before its loop, from the round's statistics: the BatchNorm affine of channel k of z2
// (sk, tk; node_stat_kernel / node_proj + pass B took the moments), cb = sk b_k + tk, and with lazy e' (the edge buffer holds
// z1: e' = relu(s1 z1 + t1), recomputed here) the affine of z1 -- in shared memory (z1.s1 / z1.t1: the walk reads it there, it
// has no eight registers to spare) and per lane.  Whole block; `lazy` block-uniform; one barrier, two when lazy.
// stamp: the EK_STAMP kernel id that marks the end of the gather (0: none).
struct Z1AffineShared { double st[8]; float s1[4], t1[4]; };   // z1 sums | sums of squares, and the affine they give
struct NodeUpdAffine { float sk, tk, cb; float s1[4] = {1.f, 1.f, 1.f, 1.f}, t1[4] = {0.f, 0.f, 0.f, 0.f}; };
// st: e' second moments (10) | z2 sums (32) | z2 sums of squares (32); both in the kernel's shared memory
__device__ __forceinline__ NodeUpdAffine node_upd_affine(const RoundParams& p, bool lazy, int k, int stamp,
                                                         double (&st)[10 + 64], Z1AffineShared& z1) {
  NodeUpdAffine a;
  stat_gather2(p.stats + kRoundMOff + 4, 10, kMStride, p.stats + kRoundZ2Off, 64, kZ2Stride, st);
  if (lazy) stat_gather(p.stats + kRoundZ1Off, 8, kZ1Stride, z1.st);
  __syncthreads();
  if (stamp) EK_T(stamp, 1);
  if (lazy) {
    if (threadIdx.x < 4)
      bn_affine(z1.st[threadIdx.x], z1.st[4 + threadIdx.x], p.e_total, p.ue_g[threadIdx.x], p.ue_bt[threadIdx.x],
                z1.s1[threadIdx.x], z1.t1[threadIdx.x]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) { a.s1[j] = z1.s1[j]; a.t1[j] = z1.t1[j]; }
  }
  const double quad = quad_form(p.un_w + k * p.un_ld + p.un_eoff, 4, st);
  bn_affine(st[10 + k], st[10 + 32 + k] + quad, p.e_total, p.un_g[k], p.un_bt[k], a.sk, a.tk);
  a.cb = fmaf(a.sk, p.un_b[k], a.tk);
  return a;
}

typedef float f32x16c __attribute__((ext_vector_type(16)));
constexpr int kTileC = 256;   // tile = block size (128 and 512 measured slower at every graph size)
__global__ __launch_bounds__(kTileC) void pass_c_kernel(RoundParams p) {
  drop_resolve(p.drop_n);
  __shared__ float4 tile_e[kTileC];
  __shared__ int tile_row[kTileC];
  __shared__ double st[10 + 64];
  __shared__ Z1AffineShared z1s;
  const int k = threadIdx.x & 31;          // channel
  const int hw = threadIdx.x >> 5;         // half-wave
  // sorted rows: a matrix-core kernel, launched just before, did the whole list -- or (kPassCSortedWalk) every whole 64-edge
  // chunk, and what is left for this kernel are the < 64 edges behind the last one
  int64_t e_first = 0;
  if ((p.pass_c == kPassCAnyWalk || p.pass_c == kPassCSortedDet) && p.flags[0] == 0) return;
  if (p.pass_c == kPassCSortedWalk && p.flags[0] == 0) {
    e_first = p.n_edges & ~(int64_t)63;
    if (e_first == p.n_edges) return;
  }
  const int64_t n_tiles = (p.n_edges + kTileC - 1) / kTileC;
  int64_t tile = e_first / kTileC + blockIdx.x;
  if (tile >= n_tiles) return;
  // a tile's operands do not depend on the statistics: fetch the first one before waiting for those
  float4 ev;
  int rw;
  auto fetch = [&](int64_t t) {
    const int64_t e = t * kTileC + threadIdx.x;
    ev = make_float4(0, 0, 0, 0);
    rw = 0;
    if (e < p.n_edges) {
      ev = reinterpret_cast<const float4*>(p.e_out)[e];
      rw = p.row32[e];
    }
  };
  if (tile < n_tiles) fetch(tile);
  const NodeUpdAffine af = node_upd_affine(p, p.lazy_e, k, 0, st, z1s);
  const float sk = af.sk, cb = af.cb;
  float a4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a4[j] = sk * p.un_w[k * p.un_ld + p.un_eoff + j];
  const bool det = p.det && p.agg != 2 && p.flags[0] == 0;      // max is order-independent as it is

  while (tile < n_tiles) {
    const int64_t base = tile * kTileC;
    const int64_t e = base + threadIdx.x;
    if (p.lazy_e) lazy_relu4(ev, z1s.s1, z1s.t1);
    if (e < p.n_edges) {
      tile_row[threadIdx.x] = rw;
      if (p.logits && e >= e_first) {                         // classifier on this edge (mpn.py:291-292)
        float lg[MTMC_MAX_CLASSES];
        classify_edge(p.cls_w, p.cls_b, p.n_classes, ev, lg);
        if (p.n_classes == 2) {
          reinterpret_cast<float2*>(p.logits)[e] = make_float2(lg[0], lg[1]);
        } else {
          for (int c = 0; c < p.n_classes; ++c) p.logits[e * p.n_classes + c] = lg[c];
        }
      }
    }
    tile_e[threadIdx.x] = ev;
    __syncthreads();
    const int n_here = base + hw * 32 < e_first ? 0 : (int)min((int64_t)32, p.n_edges - (base + hw * 32));   // may be <= 0
    const int64_t chunk = (base >> 5) + hw;
    int cur = -1;
    bool first = true;
    float acc = 0.f, c0 = 0.f;
    unsigned long long zd = 0;               // Dropout: the hash of four consecutive edges of this lane's channel (common.h)
    for (int j = 0; j < n_here; ++j) {
      const int r = tile_row[hw * 32 + j];
      const float4 v = tile_e[hw * 32 + j];
      if (p.drop_n.on && (j & 3) == 0)
        zd = drop_hash4(p.drop_n.seed, p.drop_stream + 1, drop_msg_index(base + hw * 32 + j, k, p.n_edges) >> 2);
      if (r != cur) {
        if (cur >= 0) { flush_run(p, det, chunk, first ? 0 : -1, cur, k, acc); first = false; }
        cur = r;
        acc = 0.f;
        c0 = fmaf(sk, p.Q[(int64_t)r * kH + k], cb);
      }
      float m = fmaxf(fmaf(a4[3], v.w, fmaf(a4[2], v.z, fmaf(a4[1], v.y, fmaf(a4[0], v.x, c0)))), 0.f);
      if (p.drop_n.on) m = drop_field(p.drop_n, zd, j & 3) ? m * p.drop_n.inv_keep : 0.f;
      acc = (p.agg == 2) ? fmaxf(acc, m) : acc + m;
    }
    if (cur >= 0) flush_run(p, det, chunk, first ? 0 : 1, cur, k, acc);
    tile += gridDim.x;
    if (tile < n_tiles) fetch(tile);
    __syncthreads();
  }
}

// A 32-edge group g of a chunk that is neither one row nor two (both matrix-core kernels; acc: its 16 registers of E' . (s A)^T
// without the row constants, rw: the lanes' row ids, gm: its valid edges, keep / ikn: DROP's keep bits and 1/(1-p)).  Up to
// four distinct rows take one masked pass each (DET: any number); a group that is all over the place (unsorted or low-degree
// stretch of the list) is cheaper per EDGE: every register adds its own edge's constant and goes to its row with one atomic
// (bounded cost, no run bookkeeping).  c0_of(row) -> s_k (Q[row][k] + b_k) + t_k and account(row, partial sum) are the
// calling kernel's: it owns the lookups' cache and the run state.
template <bool DROP, bool DET, typename C0Of, typename Account>
__device__ __forceinline__ void several_rows_group(const RoundParams& p, const NodeUpdAffine& af, const f32x16c& acc, int rw,
                                                   int g, unsigned gm, int k, int hi, unsigned keep, float ikn, C0Of c0_of,
                                                   Account account) {
  auto relu_c0 = [&](int i, float c0) -> float {
    const float t = fmaxf(acc[i] + c0, 0.f);
    return DROP ? t * (((keep >> i) & 1u) ? ikn : 0.f) : t;
  };
  int n_rows = 0;
  if (!DET) {
    unsigned left = gm;
    while (left != 0 && n_rows <= 4) {
      const int r = __builtin_amdgcn_readfirstlane(__shfl(rw, 32 * g + __ffs(left) - 1, 64));
      left &= ~((unsigned)(__ballot(rw == r) >> (32 * g)));
      ++n_rows;
    }
  }
  if (!DET && n_rows > 4) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int off = (i & 3) + 8 * (i >> 2) + 4 * hi;
      const int r = __shfl(rw, 32 * g + off, 64);
      if ((gm >> off) & 1u)
        unsafeAtomicAdd(p.h_acc + (int64_t)r * kH + k, relu_c0(i, fmaf(af.sk, p.Q[(int64_t)r * kH + k], af.cb)));
    }
    return;
  }
  unsigned done = 0;
  while (done != gm) {                                   // one masked pass per distinct row of the group
    const int pos = __ffs(gm & ~done) - 1;
    const int r = __builtin_amdgcn_readfirstlane(__shfl(rw, 32 * g + pos, 64));
    const unsigned same = (unsigned)(__ballot(rw == r) >> (32 * g)) & gm & ~done;
    done |= same;
    const float c0 = c0_of(r);
    const unsigned mine = same >> (4 * hi);             // bit (i&3) + 8(i>>2): register i's edge of this half-wave
    float sacc = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sacc += ((mine >> ((i & 3) + 8 * (i >> 2))) & 1u) ? relu_c0(i, c0) : 0.f;
    account(r, sacc);
  }
}

// ------------------------------------------------------------------------------------------------
// pass C for many-edge, row-sorted lists: the 32-wide node-update pre-activation of 32 edges at a time on the matrix
// cores.  A resident grid of waves takes spans of span_c consecutive 64-edge chunks round-robin.  Per chunk: one coalesced float4 (e') + row id per lane; two
// v_permlane32_swap turn the four components into the A operands of v_mfma_f32_32x32x2_f32 (A[i][k] = e'_k of edge i),
// the B operand is the channel's BatchNorm-scaled weight row (constant per lane), so
//     Z[32 edges][32 channels] = E' . (s_k A_k)^T             2 MFMAs per 32 edges (K = 4)
// arrives as 16 registers per lane = 16 edges of the lane's channel.  The ReLU and the per-row sums are then 3 VALU ops
// per register (c0 = s_k (Q[row][k] + b_k) + t_k is one value per lane while the group stays in one row -- the common
// case at the average degrees this kernel is launched for); runs are carried in registers across groups and chunks and
// flushed with one 128-byte row of float atomics when the row changes.  Groups that straddle rows take a masked pass
// per distinct row.  Exact same arithmetic per edge as pass_c_kernel (fp32 FMAs in k order inside the MFMA); sum / mean
// aggregation, eval mode, non-deterministic mode only -- everything else stays on pass_c_kernel.
// The walk in pass_c_kernel costs ~4.5 wave-instructions per edge; this one ~1.5.
// ------------------------------------------------------------------------------------------------
// 64-edge chunks per wave span (runs are carried inside a span; one span per wave, so the grid balances itself)

template <bool DROP>        // DROP (training, few-edge lists): the node update's Dropout on the messages, per accumulator register
__global__ __launch_bounds__(256, (DROP ? 3 : 1)) void pass_c_mfma_kernel(RoundParams p, int span_c) {   // DROP: 168 registers, three blocks per CU
  if (DROP) drop_resolve(p.drop_n);
  __shared__ double st[10 + 64];
  __shared__ Z1AffineShared z1s;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: spans, chunks, rows stay scalar
  const int k = lane & 31, hi = lane >> 5;
  if (p.pass_c == kPassCAnyWalk && p.flags[0] != 0) return;  // unsorted rows: pass_c_kernel does this round (block-uniform)
  EK_T(4, 0);
  const NodeUpdAffine af = node_upd_affine(p, p.lazy_e, k, 4, st, z1s);
  const float sk = af.sk, cb = af.cb;
  const float b0 = sk * p.un_w[k * p.un_ld + p.un_eoff + hi];          // B[kk = hi][j = k] of the two K = 2 steps
  const float b1 = sk * p.un_w[k * p.un_ld + p.un_eoff + 2 + hi];
  const bool want_logits = p.logits != nullptr;
  const Cls2 cls = cls2_load(p.cls_w, p.cls_b, want_logits && p.n_classes == 2);

  EK_T(4, 2);
  const int64_t n_chunks = (p.n_edges + 63) / 64;
  const int64_t n_spans = (n_chunks + span_c - 1) / span_c;
  const int64_t wave_stride = (int64_t)gridDim.x * 4;
  for (int64_t span = (int64_t)blockIdx.x * 4 + wid; span < n_spans; span += wave_stride) {
    int cur = -1;                 // wave-uniform: the row whose partial sum `run` holds (this lane's channel, this half's edges)
    float run = 0.f;
    auto flush = [&]() {
      if (cur >= 0) {
        const float tot = run + __shfl_xor(run, 32, 64);
        if (hi == 0) unsafeAtomicAdd(p.h_acc + (int64_t)cur * kH + k, tot);
      }
    };
    const int64_t c_end = min(n_chunks, (span + 1) * span_c);
    // A three-deep software pipeline of PLAIN loads (the compiler counts every one of them, so its own s_waitcnt is exact;
    // round 2 issued the Q lookups from inline asm behind a hand-counted s_waitcnt vmcnt(2)):
    //   chunk c + 2: e' / row ids requested                                  (ev_3, rw_3)
    //   chunk c + 1: row ids have landed -> the Q rows of its first and last row requested   (all of its rows at the degrees
    //                this kernel runs at; other rows of a chunk are looked up on demand)
    //   chunk c    : everything is in registers -> classifier, MFMAs, sums
    // so a k-iteration waits once, at its top, for loads issued a whole iteration earlier, and the table lookups' latency
    // (the Q table lives in L2 / Infinity Cache: 0.3-1 us under load) no longer sits between a chunk's loads and its MFMAs.
    auto fetch = [&](int64_t chunk, float4& ev_o, int& rw_o) {    // clamped address: chunks past the end re-read the last edge
      const int64_t e = min(chunk * 64 + lane, p.n_edges - 1);
      ev_o = reinterpret_cast<const float4*>(p.e_out)[e];
      rw_o = p.row32[e];
    };
    auto rows_of = [&](int rw_raw, int64_t chunk, int& first, int& last) {   // first / last row of a chunk (wave-uniform)
      const int nv = (int)min((int64_t)64, p.n_edges - chunk * 64);
      first = __builtin_amdgcn_readfirstlane(rw_raw);
      last = __builtin_amdgcn_readfirstlane(__shfl(rw_raw, (nv > 0 ? nv : 1) - 1, 64));
    };
    int qa_row = -1, qb_row = -1;
    float qa = 0.f, qb = 0.f;
    auto c0_of = [&](int r) -> float {                         // r wave-uniform
      const float q = r == qa_row ? qa : (r == qb_row ? qb : p.Q[(int64_t)r * kH + k]);
      return fmaf(sk, q, cb);
    };
    auto account = [&](int r, float part) {                     // add a group's partial sum to row r's run
      if (r != cur) {
        flush();
        cur = r;
        run = 0.f;
      }
      run += part;
    };
    // sum of relu over the lane's 16 values.  relu as a signed-integer max: exact for every float (negative values and
    // -0 have the sign bit set), and free of the canonicalising v_max_f32 x, x, x that fmaxf puts in front
    // DROP: keep[g][i] = 1/(1-p) or 0 for register i of group g (edge 64 chunk + 32 g + (i&3) + 8 (i>>2) + 4 hi, channel k:
    // drop_msg_index, what the walk and the backward hash too), taken once per chunk: eight hashes for the 32 registers
    unsigned keepbits[2] = {0u, 0u};                 // (bit i: register i kept -- one register instead of 32 factors)
    const float ikn = DROP ? p.drop_n.inv_keep : 1.f;
    auto keepf = [&](int g, int i) -> float { return ((keepbits[g] >> i) & 1u) ? ikn : 0.f; };
    auto relu_sum = [&](const f32x16c& acc, int g) -> float {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        const float t0 = __int_as_float(max(__float_as_int(acc[i]), 0)), t1 = __int_as_float(max(__float_as_int(acc[i + 1]), 0));
        s0 += DROP ? t0 * keepf(g, i) : t0;
        s1 += DROP ? t1 * keepf(g, i + 1) : t1;
      }
      return s0 + s1;
    };
    const int64_t c0_chunk = span * span_c;
    float4 ev_1, ev_2;
    int rw_1, rw_2;
    // (requesting the wave's first chunk BEFORE the statistics are gathered -- it does not depend on them -- was measured in
    //  round 5 and took 1.6 us MORE per launch on the 150k-edge graph, profiles/r05_s02_edge_trims.txt: not kept)
    fetch(c0_chunk, ev_1, rw_1);
    rows_of(rw_1, c0_chunk, qa_row, qb_row);
    qa = p.Q[(int64_t)qa_row * kH + k];
    qb = p.Q[(int64_t)qb_row * kH + k];
    // Nothing is requested for chunks past the span's end: on few-edge lists a span is ONE chunk, and waiting for the row ids
    // of a next chunk that does not exist was a whole round trip in front of the only chunk's MFMAs (round 5 stamps,
    // profiles/r05_edge_stamps.txt: 7.0 -> 5.7 us per launch)
    ev_2 = ev_1; rw_2 = rw_1;
    if (c0_chunk + 1 < c_end) fetch(c0_chunk + 1, ev_2, rw_2);
    for (int64_t chunk = c0_chunk; chunk < c_end; ++chunk) {
      // ---- chunk + 1: its row ids were requested one iteration ago; request its Q rows.  chunk + 2: request the stream.
      int qa_row_2 = qa_row, qb_row_2 = qb_row;
      float qa_2 = qa, qb_2 = qb;
      if (chunk + 1 < c_end) {
        rows_of(rw_2, chunk + 1, qa_row_2, qb_row_2);
        qa_2 = p.Q[(int64_t)qa_row_2 * kH + k];
        qb_2 = p.Q[(int64_t)qb_row_2 * kH + k];
      }
      float4 ev_3 = ev_2;
      int rw_3 = rw_2;
      if (chunk + 2 < c_end) fetch(chunk + 2, ev_3, rw_3);
      // ---- chunk: all in registers
      const int64_t e = chunk * 64 + lane;
      const bool valid = e < p.n_edges;
      float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) {
        ev = ev_1;
        if (p.lazy_e) lazy_relu4(ev, af.s1, af.t1);
      }
      const int rw = valid ? rw_1 : -1;
      const int n_valid = (int)min((int64_t)64, p.n_edges - chunk * 64);      // scalar
      if (DROP) {
        keepbits[0] = keepbits[1] = 0u;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int q = 0; q < 4; ++q) {                       // registers 4q .. 4q+3: four consecutive edges, one hash
            const unsigned long long zd =
                drop_hash4(p.drop_n.seed, p.drop_stream + 1, drop_msg_index(chunk * 64 + 32 * g + 8 * q + 4 * hi, k, p.n_edges) >> 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) keepbits[g] |= drop_field(p.drop_n, zd, j) ? (1u << (4 * q + j)) : 0u;
          }
      }
      float2 lg = make_float2(0.f, 0.f);                        // classifier on this edge (mpn.py:291-292): arithmetic now,
      if (want_logits && p.n_classes == 2) lg = classify_edge(cls, ev);       // the store behind the group masks
      // A operands: lanes 0..31 carry component k = 0 (2), lanes 32..63 component k = 1 (3) of edge (lane & 31)
      const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(ev.x), __float_as_uint(ev.y), false, false);
      const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ev.z), __float_as_uint(ev.w), false, false);
      const unsigned long long row_first_mask = __ballot(rw == qa_row), row_last_mask = __ballot(rw == qb_row);
      // group g = edges 32g .. 32g+31 of the chunk.  At the degrees this kernel runs at a group touches one row, or two
      // (a row boundary inside it): classify each group by its first row (mask ma), the row of its first other edge
      // (mask mb), and whether those two cover it.  All of this is scalar.
      const int nv1 = n_valid - 32;
      const unsigned gmv[2] = {n_valid >= 32 ? 0xffffffffu : ((1u << n_valid) - 1u),
                               nv1 >= 32 ? 0xffffffffu : (nv1 > 0 ? ((1u << nv1) - 1u) : 0u)};
      int ra[2], rb[2];
      unsigned ma[2], mb[2];
      bool two_rows_max[2];
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        ra[g] = rb[g] = -1;
        ma[g] = mb[g] = 0;
        two_rows_max[g] = true;
        if (gmv[g] == 0) continue;
        ra[g] = g == 0 ? qa_row : __builtin_amdgcn_readlane(rw, 32);
        const unsigned long long fa = g == 0 ? row_first_mask : (ra[g] == qb_row ? row_last_mask : __ballot(rw == ra[g]));
        ma[g] = (unsigned)(fa >> (32 * g)) & gmv[g];
        const unsigned rest = gmv[g] & ~ma[g];
        if (rest != 0) {
          rb[g] = __builtin_amdgcn_readfirstlane(__shfl(rw, 32 * g + __ffs(rest) - 1, 64));
          const unsigned long long fb = rb[g] == qb_row ? row_last_mask : __ballot(rw == rb[g]);
          mb[g] = (unsigned)(fb >> (32 * g)) & gmv[g];
          two_rows_max[g] = (ma[g] | mb[g]) == gmv[g];
        }
      }
      if (want_logits && valid) {
        if (p.n_classes == 2) reinterpret_cast<float2*>(p.logits)[e] = lg;
        else classify_edge(p.cls_w, p.cls_b, p.n_classes, ev, p.logits + e * p.n_classes);
      }
      if (two_rows_max[0] && two_rows_max[1]) {
        // Z = c0[row of edge] + E' . (s A)^T: the row constants ride in as a third K step whose A operand is the
        // membership of edge i in the group's first / second row and whose B operand holds the two constants; both
        // groups' chains are issued before either result is consumed
        f32x16c acc[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const unsigned long long member = (unsigned long long)ma[g] | ((unsigned long long)mb[g] << 32);
          const float a_c = __builtin_amdgcn_inverse_ballot_w64(member) ? 1.0f : 0.0f;
          const float c_a = ra[g] >= 0 ? c0_of(ra[g]) : 0.f, c_b = rb[g] >= 0 ? c0_of(rb[g]) : 0.f;
          f32x16c z = {};
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c, hi == 0 ? c_a : c_b, z, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[g]), b0, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[g]), b1, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          if (ra[g] < 0) break;
          const float total = relu_sum(acc[g], g);
          if (rb[g] < 0) {
            account(ra[g], total);
          } else {                                             // the first row's share through per-register lane masks
            float sa0 = 0.f, sa1 = 0.f;                        // (register i = edge (i&3) + 8(i>>2) + 4*hi of the group)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int c = (i & 3) + 8 * (i >> 2);
              const unsigned long long in_a = (((ma[g] >> c) & 1u) ? 0xffffffffull : 0ull) |
                                              (((ma[g] >> (c + 4)) & 1u) ? 0xffffffff00000000ull : 0ull);
              const float t0 = __int_as_float(max(__float_as_int(acc[g][i]), 0));
              const float t = DROP ? t0 * keepf(g, i) : t0;
              const float v = __builtin_amdgcn_inverse_ballot_w64(in_a) ? t : 0.f;
              if (i & 1) sa1 += v; else sa0 += v;
            }
            const float sa = sa0 + sa1;
            account(ra[g], sa);
            account(rb[g], total - sa);
          }
        }
      } else {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const unsigned gm = gmv[g];
          if (gm == 0) break;
          f32x16c acc = {};
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[g]), b0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[g]), b1, acc, 0, 0, 0);
          several_rows_group<DROP, false>(p, af, acc, rw, g, gm, k, hi, keepbits[g], ikn, c0_of, account);
        }
      }
      // rotate the pipeline
      ev_1 = ev_2; rw_1 = rw_2;
      ev_2 = ev_3; rw_2 = rw_3;
      qa_row = qa_row_2; qb_row = qb_row_2;
      qa = qa_2; qb = qb_2;
    }
    flush();
  }
  EK_T(4, 3);
}

// ------------------------------------------------------------------------------------------------
// pass C for MANY-edge ROW-SORTED lists (kPassCSortedWalk, kPassCSortedDet): the kernel above with everything a sorted list of whole 64-edge chunks
// makes unnecessary taken out of the loop -- counters of round 3 (r03: SQ_INSTS_*) showed that kernel bound by instruction
// issue, 189 vector + 142 scalar instructions per chunk, most of them bookkeeping:
//  * only WHOLE chunks here (the < 64 edges behind the last whole chunk go to pass_c_kernel, launched behind this one):
//    no clamped 64-bit addresses, no validity masks, a chunk's first / last rows are v_readlane of fixed lanes;
//  * sorted rows: a group's first row is its lane 0, its last row its lane 31, and the group is covered by those two iff
//    ballot(row == first) | ballot(row == last) is everything -- no search for "the first other edge";
//  * the row constants c0 = s_k (Q[row][k] + b_k) + t_k ride in as the B operand of a K step whose A operand is the
//    membership in the group's first (kk = 0) / last (kk = 1) row: lanes 0-31 of a B operand hold kk = 0, lanes 32-63 kk = 1,
//    so ONE Q lookup per group -- row = lane < 32 ? first : last -- is that operand; no per-row lookups, no selects;
//  * a two-row group's first share: its edges are a PREFIX of the group, register i of a lane holds edge (i&3) + 8(i>>2) +
//    4 hi, so whole 4-register blocks lie on one side and only block n_first >> 3 is cut: block sums (needed for the total
//    anyway) + four compares in the one cut block, instead of sixteen scalar-built lane masks;
//  * the three-deep pipeline is unrolled by three with the stage registers renamed: no register moves.
// Groups that touch three or more rows (low-degree stretches) go to several_rows_group, as above.
// ------------------------------------------------------------------------------------------------
// DET (MTMC_F_DETERMINISTIC): no atomics.  A span's first run goes to carry[span][0], its last run (if different) to
// carry[span][1], runs strictly inside a span are complete rows and are stored; agg_fixup_kernel adds a row's pieces in span
// order (the walk's scheme, flush_run above, with spans of span_c * 64 edges for its 32-edge chunks).  The < 64 edges behind
// the last whole chunk are then taken here too, by the wave that owns the last span, through the masked passes.
template <bool LAZY, bool DET>
__global__ __launch_bounds__(256) void pass_c_sorted_kernel(RoundParams p, int span_c) {
  __shared__ double st[10 + 64];
  __shared__ Z1AffineShared z1s;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = lane & 31, hi = lane >> 5;
  if (p.flags[0] != 0) return;                                // unsorted rows: pass_c_kernel does this round (block-uniform)
  const NodeUpdAffine af = node_upd_affine(p, LAZY, k, 0, st, z1s);
  const float sk = af.sk, cb = af.cb;
  const float b0 = sk * p.un_w[k * p.un_ld + p.un_eoff + hi];          // B[kk = hi][j = k] of the two K = 2 steps
  const float b1 = sk * p.un_w[k * p.un_ld + p.un_eoff + 2 + hi];
  const bool two_class = p.logits != nullptr && p.n_classes == 2;
  const Cls2 cls = cls2_load(p.cls_w, p.cls_b, two_class);
  const int lim_hi = 4 * hi;
  const unsigned koff = (unsigned)k * 4u;

  const int n_full = (int)(p.n_edges >> 6);                  // whole chunks (launch_pass_c: fewer than 2^31 of them)
  const int n_tail = (int)(p.n_edges & 63);                  // edges behind them (DET: taken here; else by pass_c_kernel)
  const int n_spans = ((DET && n_tail ? n_full + 1 : n_full) + span_c - 1) / span_c;
  const int wave_stride = (int)gridDim.x * 4;
  for (int span = (int)blockIdx.x * 4 + wid; span < n_spans; span += wave_stride) {
    int cur = -1;                 // wave-uniform: the row whose partial sum `run` holds (this lane's channel, this half's edges)
    float run = 0.f;
    bool first_run = true;        // DET: nothing of this span has been flushed yet
    auto flush = [&](bool last) {
      if (cur >= 0) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(run), __float_as_uint(run), false, false);
        const float tot = run + __uint_as_float(hi == 0 ? sw[1] : sw[0]);
        if (!DET) {
          if (hi == 0) unsafeAtomicAdd(p.h_acc + (int64_t)cur * kH + k, tot);
        } else if (hi == 0) {
          if (first_run) p.carry[((int64_t)span * 2 + 0) * kH + k] = tot;
          else if (last) p.carry[((int64_t)span * 2 + 1) * kH + k] = tot;
          else p.h_acc[(int64_t)cur * kH + k] = tot;             // a row that began and ended inside this span
        }
        first_run = false;
      }
    };
    auto account = [&](int r, float part) {                     // add a group's partial sum to row r's run
      if (r != cur) {
        flush(false);
        cur = r;
        run = 0.f;
      }
      run += part;
    };
    auto c0_of = [&](int r) -> float { return fmaf(sk, p.Q[(int64_t)r * kH + k], cb); };
    auto slow_group = [&](const f32x16c& acc, int rwc, int g, unsigned gm) {     // gm: the group's valid edges
      several_rows_group<false, DET>(p, af, acc, rwc, g, gm, k, hi, 0u, 1.f, c0_of, account);
    };
    const int c_beg = span * span_c, c_end = min(n_full, c_beg + span_c);
    // stage registers: chunk c lives in slot c % 3 (literal at every use after inlining)
    float4 ev[3];
    int rw[3];
    float qv[3][2];              // per group: Q[lane < 32 ? first row : last row][k]
    int rows[3][4];              // first / last row of group 0, of group 1 (scalar)
    auto fetch = [&](int c, int slot) {                         // whole chunks only: c is clamped to the last one
      const int cc = min(c, n_full - 1);
      const int64_t e0 = (int64_t)cc * 64;
#if PC_NT
      {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p.e_out + e0 * 4) + lane);
        ev[slot] = make_float4(v[0], v[1], v[2], v[3]);
        rw[slot] = __builtin_nontemporal_load(p.row32 + e0 + lane);
      }
#else
      ev[slot] = reinterpret_cast<const float4*>(p.e_out + e0 * 4)[lane];
      rw[slot] = (p.row32 + e0)[lane];
#endif
    };
    auto lookup = [&](int slot) {                               // the chunk's row ids have landed: its four rows, its Q operands
      rows[slot][0] = __builtin_amdgcn_readlane(rw[slot], 0);
      rows[slot][1] = __builtin_amdgcn_readlane(rw[slot], 31);
      rows[slot][2] = __builtin_amdgcn_readlane(rw[slot], 32);
      rows[slot][3] = __builtin_amdgcn_readlane(rw[slot], 63);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int r = hi ? rows[slot][2 * g + 1] : rows[slot][2 * g];
        // (uniform base + 32-bit byte offset: one shift-add per lookup instead of 64-bit address arithmetic;
        // launch_pass_c takes this kernel only while N * 128 fits 32 bits)
        qv[slot][g] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.Q) + (((unsigned)r << 7) + koff));
      }
    };
    // one chunk: everything of slot sl0 is in registers; slot sl1's row ids have landed; slot sl2 is requested
    auto step = [&](int c, int sl0, int sl1, int sl2) {
      fetch(c + 2, sl2);
      lookup(sl1);
      float4 e4 = ev[sl0];
      if (LAZY) lazy_relu4(e4, af.s1, af.t1);
      const int rwc = rw[sl0];
      if (p.logits != nullptr) {                               // classifier on this edge (mpn.py:291-292)
        if (two_class) reinterpret_cast<float2*>(p.logits + (int64_t)c * 128)[lane] = classify_edge(cls, e4);
        else classify_edge(p.cls_w, p.cls_b, p.n_classes, e4, p.logits + ((int64_t)c * 64 + lane) * p.n_classes);
      }
      // A operands: lanes 0..31 carry component k = 0 (2), lanes 32..63 component k = 1 (3) of edge (lane & 31)
      const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(e4.x), __float_as_uint(e4.y), false, false);
      const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(e4.z), __float_as_uint(e4.w), false, false);
      // membership of the chunk's edges in each group's first / last row (sorted: a prefix / a suffix of the group)
      const int ra0 = rows[sl0][0], rb0 = rows[sl0][1], ra1 = rows[sl0][2], rb1 = rows[sl0][3];
      const unsigned ma0 = (unsigned)__ballot(rwc == ra0);
      const unsigned mb0 = ra0 == rb0 ? 0u : (unsigned)__ballot(rwc == rb0);
      const unsigned ma1 = (unsigned)(__ballot(rwc == ra1) >> 32);
      const unsigned mb1 = ra1 == rb1 ? 0u : (unsigned)(__ballot(rwc == rb1) >> 32);
      const unsigned ma[2] = {ma0, ma1}, mb[2] = {mb0, mb1};
      const int ra[2] = {ra0, ra1}, rb[2] = {rb0, rb1};
      if ((ma0 | mb0) == 0xffffffffu && (ma1 | mb1) == 0xffffffffu) {
        f32x16c acc[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const unsigned long long member = (unsigned long long)ma[g] | ((unsigned long long)mb[g] << 32);
          const float a_c = __builtin_amdgcn_inverse_ballot_w64(member) ? 1.0f : 0.0f;
          f32x16c z = {};
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c, fmaf(sk, qv[sl0][g], cb), z, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[g]), b0, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[g]), b1, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          // relu as a signed-integer max (exact for every float, no canonicalising v_max_f32 x, x, x in front); sums per
          // block of four registers = four consecutive edges of this half
          float t[16], bs[4];
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = __int_as_float(max(__float_as_int(acc[g][i]), 0));
#pragma unroll
          for (int b = 0; b < 4; ++b) bs[b] = (t[4 * b] + t[4 * b + 1]) + (t[4 * b + 2] + t[4 * b + 3]);
          const float total = (bs[0] + bs[1]) + (bs[2] + bs[3]);
          if (mb[g] == 0u) {
            account(ra[g], total);
          } else {
            const int n_a = __builtin_popcount(ma[g]);          // 1..31 edges of the first row: a prefix
            const int q = n_a >> 3;                             // the block the boundary cuts (for one of the halves)
            const int lim = (n_a & 7) - lim_hi;                 // its registers j < lim belong to the first row
            float sa;
            auto cut = [&](int b) {
              const float c0 = 0 < lim ? t[4 * b] : 0.f, c1 = 1 < lim ? t[4 * b + 1] : 0.f;
              const float c2 = 2 < lim ? t[4 * b + 2] : 0.f, c3 = 3 < lim ? t[4 * b + 3] : 0.f;
              return (c0 + c1) + (c2 + c3);
            };
            if (q == 0) sa = cut(0);
            else if (q == 1) sa = bs[0] + cut(1);
            else if (q == 2) sa = (bs[0] + bs[1]) + cut(2);
            else sa = (bs[0] + bs[1]) + (bs[2] + cut(3));
            account(ra[g], sa);
            account(rb[g], total - sa);
          }
        }
      } else {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          f32x16c acc = {};
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[g]), b0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[g]), b1, acc, 0, 0, 0);
          slow_group(acc, rwc, g, 0xffffffffu);
        }
      }
    };
    fetch(c_beg, 0);
    fetch(c_beg + 1, 1);
    lookup(0);
    for (int c = c_beg; c < c_end; c += 3) {
      step(c, 0, 1, 2);
      if (c + 1 < c_end) step(c + 1, 1, 2, 0);
      if (c + 2 < c_end) step(c + 2, 2, 0, 1);
    }
    if (DET && n_tail && span == n_spans - 1) {
      // the partial last chunk (clamped addresses, masked passes only)
      const int64_t e = (int64_t)n_full * 64 + lane;
      const bool valid = lane < n_tail;
      const int64_t ec = valid ? e : p.n_edges - 1;
      float4 e4 = reinterpret_cast<const float4*>(p.e_out)[ec];
      const int rwc = valid ? p.row32[ec] : -1;
      if (LAZY) lazy_relu4(e4, af.s1, af.t1);
      if (p.logits != nullptr && valid) classify_edge(p.cls_w, p.cls_b, p.n_classes, e4, p.logits + e * p.n_classes);
      const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(e4.x), __float_as_uint(e4.y), false, false);
      const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(e4.z), __float_as_uint(e4.w), false, false);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int nv = n_tail - 32 * g;
        const unsigned gm = nv >= 32 ? 0xffffffffu : (nv > 0 ? ((1u << nv) - 1u) : 0u);
        if (gm == 0) break;
        f32x16c acc = {};
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[g]), b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[g]), b1, acc, 0, 0, 0);
        slow_group(acc, rwc, g, gm);
      }
    }
    flush(true);
  }
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
constexpr int64_t kSortedMaxNodes = 1ll << 24;   // pass_c_sorted_kernel keeps row ids in 24 bits
// many-edge lists (and long deterministic ones) take pass_c_sorted_kernel -- unless MTMC_PASS_C_GENERAL asks for the any-order
// kernel (A/B) or the call has >= 2^24 GLOBAL node rows (reachable with row-sharded multi-GPU calls)
static bool pass_c_sorted_taken(int64_t n_nodes) { return !knobs().pass_c_general && n_nodes < kSortedMaxNodes; }

// Which kernels pass C takes (kernels.h: PassC).  Many edges per node: a matrix-core kernel.  On many-edge lists it returns at
// once when prep_kernel found the rows unsorted, and pass_c_kernel, launched behind it, returns at once when they are sorted
// (sortedness is only known on the device).  Few-edge lists, where a second launch would cost as much as the pass: the
// any-order kernel alone -- it is correct for any order, groups that touch many rows just take one masked pass per row.
// MTMC_PASS_C_WALK=1 keeps the walk everywhere (A/B).
PassC plan_pass_c(int agg, bool deterministic, bool dropout, int64_t n_edges, int64_t n_nodes, double avg_degree) {
  const Knobs& kn = knobs();
  if (kn.pass_c_walk || agg == 2 || avg_degree < 24.0) return kPassCWalk;
  if (dropout && (n_edges > kSmallEdges || deterministic)) return kPassCWalk;   // Dropout: only the few-edge any-order kernel knows it
  const bool sorted = pass_c_sorted_taken(n_nodes);
  // fixed-order sums (deterministic): the sorted kernel's DET form where it pays, else the walk -- the any-order kernel only
  // knows float atomics, and the walk's carry[] is what agg_fixup_kernel adds up
  if (n_edges > kSmallEdges) {
    if (deterministic) return sorted ? kPassCSortedDet : kPassCWalk;
    return sorted ? kPassCSortedWalk : kPassCAnyWalk;
  }
  if (deterministic) return (sorted && n_edges > kDetSortedEdges) ? kPassCSortedDet : kPassCWalk;
  return n_edges >= kn.pass_c_small_min ? kPassCAny : kPassCWalk;
}

void launch_pass_c(const RoundParams& p0, hipStream_t s) {
  RoundParams p = p0;
  p.det_len = 32;
  const int span_env = knobs().pass_c_span, max_blocks = knobs().pass_c_blocks;
  if (p.pass_c == kPassCSortedWalk || p.pass_c == kPassCSortedDet) {
    // many-edge sorted lists: a grid of twice what is resident (104 registers: four blocks per CU; the block prologue -- 74 replicated
    // statistics, one BatchNorm affine per channel -- is paid once per block) whose waves all take the same number of
    // equally long spans: the span length is chosen so that spans = waves x m for the smallest m that keeps a span at
    // <= 48 chunks (a span pays one pipeline fill; a wave that gets one span more than the others sets the kernel's time:
    // at config 4, 8-chunk spans round-robin left 6 or 7 spans per wave)
    const bool det = p.pass_c == kPassCSortedDet;             // (max aggregation never gets here)
    const int64_t n_full = p.n_edges >> 6;
    int64_t blocks = (n_full + 3) / 4;
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    const int64_t per_wave = (n_full + blocks * 4 - 1) / (blocks * 4), m = (per_wave + 47) / 48;
    const int span_c = span_env > 0 ? span_env : (int)((per_wave + (m > 0 ? m : 1) - 1) / (m > 0 ? m : 1));
    const int sc = span_c > 0 ? span_c : 1;
    p.det_len = det ? sc * 64 : 32;
    const dim3 grid((int)blocks);
    if (det) {
      if (p.lazy_e) hipLaunchKernelGGL((pass_c_sorted_kernel<true, true>), grid, dim3(256), 0, s, p, sc);
      else hipLaunchKernelGGL((pass_c_sorted_kernel<false, true>), grid, dim3(256), 0, s, p, sc);
    } else {
      if (p.lazy_e) hipLaunchKernelGGL((pass_c_sorted_kernel<true, false>), grid, dim3(256), 0, s, p, sc);
      else hipLaunchKernelGGL((pass_c_sorted_kernel<false, false>), grid, dim3(256), 0, s, p, sc);
    }
  } else if (p.pass_c != kPassCWalk) {
    // the any-order kernel.  Many edges (lists of >= 2^24 nodes, MTMC_PASS_C_GENERAL): short spans round-robin over a
    // resident grid; few edges: one 64-edge chunk per wave, as many waves as there are chunks
    const int span_c = span_env > 0 ? span_env : (p.pass_c == kPassCAny ? 1 : 8);
    const int64_t spans = ((p.n_edges + 63) / 64 + span_c - 1) / span_c, blocks = (spans + 3) / 4;
    const int cap = max_blocks < 256 * 3 ? max_blocks : 256 * 3;           // 130 registers: three blocks per CU
    if (p.drop_n.on) hipLaunchKernelGGL(pass_c_mfma_kernel<true>, dim3((int)(blocks > cap ? cap : blocks)), dim3(256), 0, s, p, span_c);
    else hipLaunchKernelGGL(pass_c_mfma_kernel<false>, dim3((int)(blocks > cap ? cap : blocks)), dim3(256), 0, s, p, span_c);
  }
  // (behind a matrix-core kernel the walk returns at once on sorted lists -- all but the workgroup that owns the < 64 edges
  //  behind the last whole chunk.  Round 5 launched it with 256 workgroups instead of up to 2048 there: the launch still
  //  took 5.3 us (5.1 before: it is the fixed cost of a dependent launch, not the dispatch of 2048 workgroups that return), and
  //  an unsorted many-edge list would walk with an eighth of the workgroups -- reverted, profiles/r05_cfg4_kernel_stats.csv.
  //  With exactly ONE workgroup (-DMTMC_WALK_TAIL_GRID=1, same box, alternating): 5.60 / 5.67 us against 5.51 / 5.54 for the
  //  full grid, profiles/r05_walk_grid1.txt)
#ifdef MTMC_WALK_TAIL_GRID      // A/B builds: the walk behind the sorted kernel with this many workgroups
  if (p.pass_c == kPassCSortedWalk || p.pass_c == kPassCSortedDet) {
    hipLaunchKernelGGL(pass_c_kernel, dim3(MTMC_WALK_TAIL_GRID), dim3(kTileC), 0, s, p);
  } else
#endif
  if (p.pass_c != kPassCAny) hipLaunchKernelGGL(pass_c_kernel, dim3(edge_grid(p.n_edges, kTileC)), dim3(kTileC), 0, s, p);
  if (p.det && p.agg != 2) {
    const int64_t blocks = (p.n_nodes + 7) / 8;
    hipLaunchKernelGGL(agg_fixup_kernel, dim3((int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks))), dim3(256), 0, s, p);
  }
}

#if EK_STAMP
static int ek_stamps_pass_c(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ek), sizeof(g_ek)); }
#endif

}  // namespace mtmc

#if EK_STAMP
// The stamps of the round kernels (ids 1, 2: pass A; 3: pass B; 4: pass C) live in one buffer per translation unit; their
// slots are disjoint and zero-initialised, so the sum of the three buffers is every kernel's own stamps.
extern "C" int mtmc_dbg_ek_stamps_edge(unsigned long long* out) {    // host buffer of 8 * 2 * 8 entries
  constexpr int n = mtmc::kEkKernels * 2 * mtmc::kEkPoints;
  unsigned long long a[n], b[n];
  const int err = mtmc::ek_stamps_pass_a(a) | mtmc::ek_stamps_pass_b(b) | mtmc::ek_stamps_pass_c(out);
  for (int i = 0; i < n; ++i) out[i] += a[i] + b[i];
  return err;
}
#endif
