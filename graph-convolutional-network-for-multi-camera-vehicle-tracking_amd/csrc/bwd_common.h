// Backward pass of the message-passing network on gfx950 (training: reference train.py:356,424 runs
// `outputs, _ = mpn_model(data); loss.backward()` through models/mpn.py:250-299).
//
// Everything the backward needs was kept by the training-mode forward in the workspace ("tape"): int32
// row/col, per round z1 / e' / aggregated h, the raw encoder outputs Y_l and every BatchNorm's fp64 sums.
// Pre-activations that were never materialised in the forward (the 32-wide z2, the encoder hiddens) are
// recomputed here from the same inputs with the same Dropout masks (counter-based, common.h).
//
// BatchNorm backward with batch statistics, for y = gamma*zh + beta, zh = (z-mu)*istd over R rows, g = dL/dy:
//     dbeta = sum g,  dgamma = sum g*zh,  dz = gamma*istd*(g - dbeta/R - zh*dgamma/R)
// so every BN layer costs one statistics pass (sum g, sum g*zh in fp64) and one apply pass.
//
// Correctness first: these kernels favour simple, checkable structure (training graphs are ~440 nodes /
// ~180k edges, train.py:277); the forward kernels are the tuned ones.
#pragma once
#include "train_kernels.h"

namespace mtmc {

__device__ __forceinline__ void gacc_add(float* gacc, int slot, float v) {
  unsafeAtomicAdd(gacc + (blockIdx.x % kGradRep) * kGaccN + slot, v);
}

// The small weights an edge kernel needs for EVERY edge, copied to LDS once per workgroup: read through the parameter
// struct they are vector loads from global memory that hipcc cannot hoist or make scalar (the kernels store through
// other pointers), and each one is a memory round trip inside the per-edge code -- 54 `s_waitcnt vmcnt(0)` in
// bwd_edge_upd_kernel<1>, 32 us for 173k edges before this, against 8 us for the forward pass over the same edges.
struct EdgeWeightsLds {
  float w1[8], b1[4], w2[16], b2[4], g1[4], g2[4];     // edge encoder
  float ue_w[32], ue_g[4];                             // edge-update Linear: its 4 x (4|8) edge columns, BN gamma
  float cls_w[4 * MTMC_MAX_CLASSES];
};
__device__ __forceinline__ void edge_weights_to_lds(const EdgeEncParams& enc, const RoundParams* f, EdgeWeightsLds* w) {
  const int t = threadIdx.x;
  if (t < 8) w->w1[t] = t < 4 * enc.fe ? enc.w1[t] : 0.f;
  else if (t < 12) w->b1[t - 8] = enc.b1[t - 8];
  else if (t < 28) w->w2[t - 12] = enc.w2[t - 12];
  else if (t < 32) w->b2[t - 28] = enc.b2[t - 28];
  else if (t < 36) w->g1[t - 32] = enc.g1[t - 32];
  else if (t < 40) w->g2[t - 36] = enc.g2[t - 36];
  else if (f && t >= 64 && t < 96) {
    const int kk = (t - 64) >> 3, j = (t - 64) & 7;
    w->ue_w[t - 64] = j < (f->reattach_edges ? 8 : 4) ? f->ue_w[kk * f->ue_ld + f->ue_eoff + j] : 0.f;
  } else if (f && t >= 96 && t < 100) w->ue_g[t - 96] = f->ue_g[t - 96];
  else if (f && t >= 128 && t < 128 + 4 * MTMC_MAX_CLASSES)
    w->cls_w[t - 128] = (t - 128) < 4 * f->n_classes ? f->cls_w[t - 128] : 0.f;
}
__device__ __forceinline__ EdgeEncParams enc_from_lds(const EdgeEncParams& enc, const EdgeWeightsLds* w) {
  EdgeEncParams e = enc;
  drop_resolve(e.drop);
  e.w1 = w->w1; e.b1 = w->b1; e.w2 = w->w2; e.b2 = w->b2; e.g1 = w->g1; e.g2 = w->g2;
  return e;
}

__device__ __forceinline__ void mean_istd(double sum, double sumsq, double count, float& mu, float& istd) {
  double mean, r;
  bn_mean_rstd(sum, sumsq, count, mean, r);      // the forward's statistics, bit for bit (common.h)
  mu = (float)mean;
  istd = (float)r;
}

// The apply pass of the BatchNorm backward (top of this file): dz from g = dL/dy, zh and the two batch means of the statistics pass
__device__ __forceinline__ float bn_bwd_dz(float gamma, float istd, float g, float mean_g, float zh, float mean_gz) {
  return gamma * istd * (g - mean_g - zh * mean_gz);
}

// Block sum of NV per-thread fp64 values (256 threads): thread i < NV gets the sum of value i, the others 0.  red: 256 doubles.
template <int NV>
__device__ __forceinline__ double block_sums_f64(const double (&acc)[NV], double* red) {
  wave_sums_f64<NV>(acc, red + (threadIdx.x >> 6) * 64);      // (5 instructions per value instead of 18: common.h)
  __syncthreads();
  const int i = threadIdx.x;
  return i < NV ? red[i] + red[64 + i] + red[128 + i] + red[192 + i] : 0.0;
}

// Classifier backward of one edge with input x (e_r, or e0 in a model without rounds) and dl = its row of d_logits:
//   de += Wc^T dl,  acc[W + 4 c + j] += dl[c] * x[j] (dWc),  acc[B + c] += dl[c] (dbc).
// W, B and the unrolled class loop keep every index into acc[] a compile-time constant: it must stay in registers (a
// runtime index sends the array to scratch, which tests/test_isa_lint.py refuses in a product kernel).
template <int W, int B, int NV>
__device__ __forceinline__ void classifier_bwd(const float* cls_w, const float* d_logits, int64_t e, int n_classes,
                                               const float (&x)[4], float (&de)[4], double (&acc)[NV]) {
  static_assert(B + MTMC_MAX_CLASSES <= NV && W + 4 * MTMC_MAX_CLASSES <= NV, "classifier sums outside acc[]");
#pragma unroll
  for (int c = 0; c < MTMC_MAX_CLASSES; ++c) {
    if (c < n_classes) {
      const float dl = d_logits[e * n_classes + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        de[j] = fmaf(cls_w[c * 4 + j], dl, de[j]);
        acc[W + c * 4 + j] += (double)dl * x[j];
      }
      acc[B + c] += dl;
    }
  }
}

static inline int cap(int64_t blocks, int64_t hi = 1024) { return (int)(blocks < 1 ? 1 : (blocks > hi ? hi : blocks)); }

}  // namespace mtmc
