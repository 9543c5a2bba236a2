// Backward of one message-passing round: node update, edge update + classifier, node projection (bwd_round in api_train.hip).
#include "bwd_common.h"

namespace mtmc {

// ------------------------------------------------------------------------------------------------
// node-update MLP: statistics (mode 0) and apply (mode 1); lanes = channels as in pass_c_kernel.
// Max aggregation routes a node's gradient to ONE edge per channel, the arg max (torch_scatter.scatter_max
// semantics, reference models/mpn.py:199); mode 2 finds it first: smallest edge index attaining the maximum.
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void bwd_node_upd_kernel(BwdRoundParams p) {
  drop_resolve(p.f.drop_n);
  __shared__ float4 tile_e[256];
  __shared__ int tile_row[256];
  __shared__ double st[10 + 64 + 64];     // e' second moments | z2 sum, sumsq | (mode 1) sum g, sum g*zh
  __shared__ double red[8 * 32 * 6];
  // mode 1: dz2 of a half-wave's 32 edges, [edge][channel] with an odd row stride, so that the lanes can swap roles
  // (channel -> edge) and leave A^T.dz2 (4 floats per edge) instead of the 32-wide dz2 itself
  __shared__ float dzt[MODE == 1 ? 8 * 32 * 33 : 1];
  __shared__ float4 a_all[32];
  const int k = threadIdx.x & 31, hw = threadIdx.x >> 5;
  stat_gather2(p.f.stats + kRoundMOff + 4, 10, kMStride, p.f.stats + kRoundZ2Off, 64, kZ2Stride, st);
  if (MODE == 1) stat_gather(p.bst, 64, kBwdStride, st + 74);
  __syncthreads();
  const float* aw = p.f.un_w + k * p.f.un_ld + p.f.un_eoff;
  float a4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a4[j] = aw[j];
  if (MODE == 1 && hw == 0) a_all[k] = make_float4(a4[0], a4[1], a4[2], a4[3]);
  const float bk = p.f.un_b[k], gam = p.f.un_g[k], bet = p.f.un_bt[k];
  float mu, istd, sk, tk;
  const double z2sq = st[10 + 32 + k] + quad_form(aw, 4, st);
  mean_istd(st[10 + k], z2sq, p.f.e_total, mu, istd);
  bn_affine(st[10 + k], z2sq, p.f.e_total, gam, bet, sk, tk);     // the forward's affine, bit for bit (pass_c_kernel)
  float a4s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a4s[j] = sk * a4[j];
  const float cb = fmaf(sk, bk, tk);
  const float ik = p.f.drop_n.on ? p.f.drop_n.inv_keep : 1.f;
  const float mean_g = MODE == 1 ? (float)(st[74 + k] / p.f.e_total) : 0.f;
  const float mean_gz = MODE == 1 ? (float)(st[74 + 32 + k] / p.f.e_total) : 0.f;
  double acc[6] = {0, 0, 0, 0, 0, 0};      // mode 0: sum g, sum g*zh ; mode 1: sum dz2, sum dz2*e[0..3]

  const int64_t n_tiles = (p.f.n_edges + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t base = tile * 256;
    const int64_t e = base + threadIdx.x;
    if (e < p.f.n_edges) {
      tile_e[threadIdx.x] = reinterpret_cast<const float4*>(p.f.e_out)[e];
      tile_row[threadIdx.x] = p.f.row32[e];
    }
    __syncthreads();
    const int n_here = (int)min((int64_t)32, p.f.n_edges - (base + hw * 32));
    int cur = -1;
    float q = 0.f, dh = 0.f, hval = 0.f, dq_acc = 0.f;
    int winner = -1;
    unsigned long long zd = 0;               // Dropout: the hash of four consecutive edges of this lane's channel (common.h)
    for (int j = 0; j < n_here; ++j) {
      const int r = tile_row[hw * 32 + j];
      const float4 v = tile_e[hw * 32 + j];
      if (p.f.drop_n.on && (j & 3) == 0)
        zd = drop_hash4(p.f.drop_n.seed, p.f.drop_stream + 1, drop_msg_index(base + hw * 32 + j, k, p.f.n_edges) >> 2);
      if (r != cur) {
        if (MODE == 1 && cur >= 0) unsafeAtomicAdd(p.g_Q + (int64_t)cur * kH + k, dq_acc);
        cur = r;
        dq_acc = 0.f;
        q = p.f.Q[(int64_t)r * kH + k];
        dh = p.g_h[(int64_t)r * kH + k];
        if (p.f.agg == 1) { const int d = p.deg[r]; dh = dh / (float)(d > 1 ? d : 1); }
        if (p.f.agg == 2) {
          hval = p.h_agg[(int64_t)r * kH + k];
          if (MODE != 2) winner = p.arg[(int64_t)r * kH + k];
        }
      }
      const int64_t eidx = base + hw * 32 + j;
      const float z2 = fmaf(a4[3], v.w, fmaf(a4[2], v.z, fmaf(a4[1], v.y, fmaf(a4[0], v.x, q + bk))));
      const float zh = (z2 - mu) * istd;
      const float y = fmaf(a4s[3], v.w, fmaf(a4s[2], v.z, fmaf(a4s[1], v.y, fmaf(a4s[0], v.x, fmaf(sk, q, cb)))));
      const bool kept = !p.f.drop_n.on || drop_field(p.f.drop_n, zd, j & 3);
      const bool live = kept && y > 0.f;
      if (MODE == 2) {
        if (live && y * ik == hval) atomicMin(p.arg + (int64_t)r * kH + k, (int)eidx);
        continue;
      }
      float dm = dh;
      if (p.f.agg == 2) dm = (winner == (int)eidx) ? dh : 0.f;
      const float g = live ? dm * ik : 0.f;
      if (MODE == 0) {
        acc[0] += g;
        acc[1] += (double)g * zh;
      } else {
        const float dz2 = bn_bwd_dz(gam, istd, g, mean_g, zh, mean_gz);
        dzt[(hw * 32 + j) * 33 + k] = dz2;
        dq_acc += dz2;
        acc[0] += dz2;
        acc[1] += (double)dz2 * v.x; acc[2] += (double)dz2 * v.y; acc[3] += (double)dz2 * v.z; acc[4] += (double)dz2 * v.w;
      }
    }
    if (MODE == 1 && cur >= 0) unsafeAtomicAdd(p.g_Q + (int64_t)cur * kH + k, dq_acc);
    if (MODE == 1) {
      __builtin_amdgcn_wave_barrier();               // the half-wave's own LDS writes, read back below by other lanes
      if (k < n_here) {                              // lane k now stands for edge k of the half-wave's 32
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll 8
        for (int c = 0; c < 32; ++c) {
          const float d = dzt[(hw * 32 + k) * 33 + c];
          const float4 a = a_all[c];
          d0 = fmaf(a.x, d, d0); d1 = fmaf(a.y, d, d1); d2 = fmaf(a.z, d, d2); d3 = fmaf(a.w, d, d3);
        }
        reinterpret_cast<float4*>(p.g_de2)[base + hw * 32 + k] = make_float4(d0, d1, d2, d3);
      }
    }
    __syncthreads();
  }
  if (MODE == 2) return;
  constexpr int NV = MODE == 0 ? 2 : 5;
#pragma unroll
  for (int i = 0; i < NV; ++i) red[(i * 8 + hw) * 32 + k] = acc[i];
  __syncthreads();
  if (threadIdx.x < 32) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double s = 0;
      for (int h = 0; h < 8; ++h) s += red[(i * 8 + h) * 32 + k];
      if (MODE == 0) {
        unsafeAtomicAdd(p.bst + (blockIdx.x % kStatRep) * kBwdStride + i * 32 + k, s);
      } else if (i == 0) {
        gacc_add(p.gacc, kGaUnB + k, (float)s);
      } else {
        gacc_add(p.gacc, kGaUnW + k * 4 + (i - 1), (float)s);
      }
    }
    if (MODE == 1 && blockIdx.x == 0) {      // dgamma = sum g*zh, dbeta = sum g (the statistics of mode 0)
      p.un.g[k] += (float)st[74 + 32 + k];        // += : the update MLPs are shared by all rounds
      p.un.bt[k] += (float)st[74 + k];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// edge-update MLP + classifier: statistics (mode 0) and apply (mode 1); lanes = edges
// ------------------------------------------------------------------------------------------------
struct EdgeBwdShared { float mu1[4], istd1[4], mean_g[4], mean_gz[4]; double sum_g[4], sum_gz[4]; };

template <int MODE>
__global__ __launch_bounds__(256) void bwd_edge_upd_kernel(BwdRoundParams p) {
  __shared__ EdgeEncAffine af;
  __shared__ EdgeBwdShared sh;
  __shared__ double red[64 * 4];
  __shared__ EdgeWeightsLds wl;
  stat_gather(p.f.stats + kRoundZ1Off, 8, kZ1Stride, red);
  if (MODE == 1) stat_gather(p.bst, 8, kBwdStride, red + 8);
  edge_weights_to_lds(p.f.enc, &p.f, &wl);
  const EdgeEncParams enc = enc_from_lds(p.f.enc, &wl);
  const bool need_e0 = MODE == 1 && (p.f.first_round || p.f.reattach_edges);
  if (need_e0) edge_enc_affine_load(p.f.enc, &af); else __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    mean_istd(red[k], red[4 + k], p.f.e_total, sh.mu1[k], sh.istd1[k]);
    if (MODE == 1) {
      sh.sum_g[k] = red[8 + k];
      sh.sum_gz[k] = red[12 + k];
      sh.mean_g[k] = (float)(red[8 + k] / p.f.e_total);
      sh.mean_gz[k] = (float)(red[12 + k] / p.f.e_total);
    }
  }
  __syncthreads();
  const float ik = p.f.drop_e.on ? p.f.drop_e.inv_keep : 1.f;
  const int C = p.f.n_classes;
  constexpr int NV = MODE == 0 ? 8 + 16 + 4 : 4 + 32;
  static_assert(MTMC_MAX_CLASSES == 4, "mode 0: 8 statistics, 4 x 4 classifier weights, 4 classifier biases");
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0;
  const int nin = p.f.reattach_edges ? 8 : 4;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e0w = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); e0w < p.f.n_edges; e0w += nthreads) {
    // wave-uniform trip count: mode 1's run reduction is a cross-lane operation every lane has to reach together;
    // lanes past the end compute on the last edge and are masked out of every side effect
    const int64_t e_raw = e0w + (threadIdx.x & 63);
    const bool active = e_raw < p.f.n_edges;
    if (MODE == 0 && !active) continue;
    const int64_t e = active ? e_raw : p.f.n_edges - 1;
    const float4 er4 = reinterpret_cast<const float4*>(p.f.e_out)[e];
    const float4 z4 = reinterpret_cast<const float4*>(p.f.e_buf)[e];
    const float er[4] = {er4.x, er4.y, er4.z, er4.w}, z1[4] = {z4.x, z4.y, z4.z, z4.w};
    float zh[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) zh[j] = (z1[j] - sh.mu1[j]) * sh.istd1[j];
    if (MODE == 0) {
      // total gradient wrt e_r: later rounds (g_e) + node-update path (A^T dz2) + classifier (Wc^T dlogits)
      float4 ge4 = reinterpret_cast<const float4*>(p.g_e)[e];
      float de[4] = {ge4.x, ge4.y, ge4.z, ge4.w};
      const float4 d2 = reinterpret_cast<const float4*>(p.g_de2)[e];       // A^T dz2, left by bwd_node_upd_kernel<1>
      de[0] += d2.x; de[1] += d2.y; de[2] += d2.z; de[3] += d2.w;
      if (p.d_logits) classifier_bwd<8, 8 + 4 * MTMC_MAX_CLASSES>(wl.cls_w, p.d_logits, e, C, er, de, acc);
      float g1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        g1[j] = er[j] > 0.f ? de[j] * ik : 0.f;
        acc[j] += g1[j];
        acc[4 + j] += (double)g1[j] * zh[j];
      }
      reinterpret_cast<float4*>(p.g_e)[e] = make_float4(g1[0], g1[1], g1[2], g1[3]);
    } else {
      const float4 g4 = reinterpret_cast<const float4*>(p.g_e)[e];
      const float g1[4] = {g4.x, g4.y, g4.z, g4.w};
      float dz1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) dz1[j] = bn_bwd_dz(wl.ue_g[j], sh.istd1[j], g1[j], sh.mean_g[j], zh[j], sh.mean_gz[j]);
      const int r = p.f.row32[e], c = p.f.col32[e];
      // dP: ~E/N atomics land on every one of the N*8 addresses and same-address atomics serialise in L2 (measured
      // 53 us of this 62 us kernel); kGradRep replicas by workgroup cut the chains, bwd_node_proj adds them up
      float* gP = p.g_P + (size_t)(blockIdx.x % kGradRep) * p.f.n_nodes * 8;
      // replica layout: dPr [N][4], then dPc [4][N] -- the lanes of a wave hold consecutive (or nearly so) columns, so
      // channel-major puts a wave's 64 column atomics on 2-3 cache lines instead of 16 (17 of this kernel's 34 us were
      // those scattered atomics)
      wave_run_atomic_add<4>(dz1, r, active, gP, 4);      // rows come in long runs: reduce in the wave first
      if (!active) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += dz1[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) unsafeAtomicAdd(gP + (4 + j) * p.f.n_nodes + c, dz1[j]);
      // the edge input of this round: [e0 | e_prev] (reattach) or e_prev, with e_prev = e0 in the first round
      float e0[4] = {0, 0, 0, 0}, ein[8];
      if (p.f.first_round || p.f.reattach_edges) {
        float a0, a1, u[4];
        load_attr(p.f.attr, enc.fe, e, a0, a1);
        edge_enc_hidden(enc, af, e, a0, a1, u);
        edge_enc_out(enc, af, e, u, e0);
      }
      float ep[4];
      if (p.f.first_round) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ep[j] = e0[j];
      } else {
        const float4 v = reinterpret_cast<const float4*>(p.f.e_prev)[e];
        ep[0] = v.x; ep[1] = v.y; ep[2] = v.z; ep[3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { ein[j] = p.f.reattach_edges ? e0[j] : ep[j]; ein[4 + j] = ep[j]; }
      float din[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {                      // static indices into acc[] / din[] (registers, not scratch)
        if (j < nin) {
          float s = 0.f;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            s = fmaf(wl.ue_w[kk * 8 + j], dz1[kk], s);
            acc[4 + kk * 8 + j] += (double)dz1[kk] * ein[j];
          }
          din[j] = s;
        }
      }
      // route d e_in: the e_prev part goes to the previous round (or to e0 in the first round), the e0 part to e0
      float d0[4] = {0, 0, 0, 0}, dp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dp[j] = p.f.reattach_edges ? din[4 + j] : din[j];
        if (p.f.reattach_edges) d0[j] = din[j];
      }
      if (p.f.first_round) {
#pragma unroll
        for (int j = 0; j < 4; ++j) d0[j] += dp[j];
      } else {
        reinterpret_cast<float4*>(p.g_e_prev)[e] = make_float4(dp[0], dp[1], dp[2], dp[3]);
      }
      if (p.f.first_round || p.f.reattach_edges) {
        float4 cur0 = reinterpret_cast<float4*>(p.g_e0)[e];
        cur0.x += d0[0]; cur0.y += d0[1]; cur0.z += d0[2]; cur0.w += d0[3];
        reinterpret_cast<float4*>(p.g_e0)[e] = cur0;
      }
    }
  }
  const double s = block_sums_f64<NV>(acc, red);
  if (threadIdx.x < NV) {
    const int i = threadIdx.x;
    if (MODE == 0) {
      if (i < 8) unsafeAtomicAdd(p.bst + (blockIdx.x % kStatRep) * kBwdStride + i, s);
      else if (i < 24) { if ((i - 8) / 4 < C) gacc_add(p.gacc, kGaClsW + (i - 8), (float)s); }
      else if (i - 24 < C) gacc_add(p.gacc, kGaClsB + (i - 24), (float)s);
    } else {
      if (i < 4) gacc_add(p.gacc, kGaUeB + i, (float)s);
      else {
        const int kk = (i - 4) / 8, j = (i - 4) % 8;
        if (j < nin) gacc_add(p.gacc, kGaUeW + kk * 8 + j, (float)s);
      }
    }
  }
  if (MODE == 1 && blockIdx.x == 0 && threadIdx.x < 4) {
    p.ue.g[threadIdx.x] += (float)sh.sum_gz[threadIdx.x];      // += : shared by all rounds
    p.ue.bt[threadIdx.x] += (float)sh.sum_g[threadIdx.x];
  }
}

// ------------------------------------------------------------------------------------------------
// node projection backward: d[h0|h] and the node-column blocks of the two update weights
// ------------------------------------------------------------------------------------------------
constexpr int kBwdProjNodes = 16;   // nodes per workgroup: 430 nodes must still give a few dozen workgroups (32: 14 us per
                                    // launch on 14 CUs); the weight-gradient atomics meet N/16 deep on a word
__global__ __launch_bounds__(256) void bwd_node_proj_kernel(BwdProjParams p) {
  constexpr int NB = kBwdProjNodes;
  __shared__ float hs[NB * 65];
  __shared__ float gs[NB * 41];
  const int hn = p.hn, ldh = hn + 1;
  const int64_t n_groups = (p.n_nodes + NB - 1) / NB;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t node0 = g * NB;
    __syncthreads();
    for (int i = threadIdx.x; i < NB * kH; i += blockDim.x) {
      const int n = i >> 5, kk = i & 31;
      const int64_t node = node0 + n;
      float v = 0.f, v0 = 0.f;
      if (node < p.n_nodes) {
        v = p.h_src[node * kH + kk];
        if (p.deg) { const int d = p.deg[node]; v = v / (float)(d > 1 ? d : 1); }
        if (hn == 2 * kH) v0 = p.h0[node * kH + kk];
      }
      hs[n * ldh + (hn - kH) + kk] = v;
      if (hn == 2 * kH) hs[n * ldh + kk] = v0;
    }
    for (int i = threadIdx.x; i < NB * 40; i += blockDim.x) {
      const int n = i / 40, j = i % 40;
      const int64_t node = node0 + n;
      float v = 0.f;
      if (node < p.n_nodes) {
        if (j < 8) {
#pragma unroll
          for (int rep = 0; rep < kGradRep; ++rep)
            v += p.g_P[(size_t)rep * p.n_nodes * 8 + (j < 4 ? node * 4 + j : (size_t)j * p.n_nodes + node)];
        } else {
          v = p.g_Q[node * kH + j - 8];
        }
      }
      gs[n * 41 + j] = v;
    }
    __syncthreads();
    // d[h0|h][node][c] = sum_j g[node][j] * W_j[c]
    for (int i = threadIdx.x; i < NB * hn; i += blockDim.x) {
      const int n = i / hn, c = i % hn;
      const int64_t node = node0 + n;
      if (node >= p.n_nodes) continue;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s = fmaf(gs[n * 41 + j], p.ue_w[j * p.ue_ld + c], s);
        s = fmaf(gs[n * 41 + 4 + j], p.ue_w[j * p.ue_ld + hn + c], s);
      }
      for (int kk = 0; kk < kH; ++kk) s = fmaf(gs[n * 41 + 8 + kk], p.un_w[kk * p.un_ld + c], s);
      const bool is_h0 = (hn == 2 * kH && c < kH) || p.src_is_h0;
      const int cc = c & 31;
      if (is_h0) {
        // [h0|h0] in the first round of a reattach model: both halves land on the same element
        unsafeAtomicAdd(p.g_h0 + node * kH + cc, s);
      } else {
        p.g_h_prev[node * kH + cc] = s;
      }
    }
    // weight gradients: 40 x hn outputs, each summed over this block's NB nodes
    for (int i = threadIdx.x; i < 40 * hn; i += blockDim.x) {
      const int j = i / hn, c = i % hn;
      float s = 0.f;
      for (int n = 0; n < NB; ++n) s = fmaf(gs[n * 41 + j], hs[n * ldh + c], s);
      float* dst = j < 4 ? p.gr_ue_w + j * p.ue_ld + c
                         : (j < 8 ? p.gr_ue_w + (j - 4) * p.ue_ld + hn + c : p.gr_un_w + (j - 8) * p.un_ld + c);
      unsafeAtomicAdd(dst, s);
    }
  }
}

void launch_bwd_node_upd(const BwdRoundParams& p, int mode, hipStream_t s) {
  const int grid = cap((p.f.n_edges + 255) / 256);
  if (mode == 0) hipLaunchKernelGGL(bwd_node_upd_kernel<0>, dim3(grid), dim3(256), 0, s, p);
  else if (mode == 1) hipLaunchKernelGGL(bwd_node_upd_kernel<1>, dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(bwd_node_upd_kernel<2>, dim3(grid), dim3(256), 0, s, p);
}
void launch_bwd_edge_upd(const BwdRoundParams& p, int mode, hipStream_t s) {
  const int grid = cap((p.f.n_edges + 255) / 256);
  if (mode == 0) hipLaunchKernelGGL(bwd_edge_upd_kernel<0>, dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(bwd_edge_upd_kernel<1>, dim3(grid), dim3(256), 0, s, p);
}
void launch_bwd_node_proj(const BwdProjParams& p, hipStream_t s) {
  hipLaunchKernelGGL(bwd_node_proj_kernel, dim3(cap((p.n_nodes + kBwdProjNodes - 1) / kBwdProjNodes)), dim3(256), 0, s, p);
}

}  // namespace mtmc
