// Backward of the edge encoder, of the classifier on the encoded edges (no rounds), and the fold of the replicated small
// gradient sums (bwd_edge_encoder, bwd_seed, bwd_fold in api_train.hip).
#include "bwd_common.h"

namespace mtmc {

// ------------------------------------------------------------------------------------------------
// edge encoder backward (three passes over edge_attr; everything is recomputed from the 8-byte attributes)
// ------------------------------------------------------------------------------------------------
struct EncBwdShared { float mua[4], ia[4], mub[4], ib[4], mgb[4], mgzb[4], mga[4], mgza[4]; double sums[16]; };

// mu/istd of an affine layer's pre-activation from the packed moments of its input (cf. moments_affine)
__device__ __forceinline__ void moments_mean_istd(const float* w, int in_dim, float bias, const double* m1,
                                                  const double* m2, double count, float& mu, float& istd) {
  double sum, sumsq;
  moments_sum_sumsq(w, in_dim, bias, m1, m2, count, sum, sumsq);
  mean_istd(sum, sumsq, count, mu, istd);
}

template <int PASS>   // 0: stats of layer 2; 1: apply layer 2 + stats of layer 1; 2: apply layer 1
__global__ __launch_bounds__(256) void bwd_edge_enc_kernel(BwdEncParams p) {
  drop_resolve(p.enc.drop);
  __shared__ EdgeEncAffine af;
  __shared__ EncBwdShared sh;
  __shared__ double sc[kStatAttr + kStatEnc2 + 16];
  __shared__ double red[64 * 4];
  __shared__ EdgeWeightsLds wl;
  edge_weights_to_lds(p.enc, nullptr, &wl);                       // (the first barrier below publishes it)
  edge_enc_affine_to_smem(p.enc, p.e_total, 2, &af, sc);          // also leaves the summed moments in sc
  if (PASS >= 1) stat_gather(p.bst, 8, kBwdStride, sc + kStatAttr + kStatEnc2);
  if (PASS >= 2) stat_gather(p.bst + 8, 8, kBwdStride, sc + kStatAttr + kStatEnc2 + 8);
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    moments_mean_istd(p.enc.w1 + k * p.enc.fe, p.enc.fe, p.enc.b1[k], sc, sc + 2, p.e_total, sh.mua[k], sh.ia[k]);
    moments_mean_istd(p.enc.w2 + k * 4, 4, p.enc.b2[k], sc + kStatAttr, sc + kStatAttr + 4, p.e_total, sh.mub[k], sh.ib[k]);
    const double* b = sc + kStatAttr + kStatEnc2;
    if (PASS >= 1) {
      sh.mgb[k] = (float)(b[k] / p.e_total); sh.mgzb[k] = (float)(b[4 + k] / p.e_total);
      for (int i = 0; i < 4; ++i) sh.sums[i * 4 + k] = b[i * 4 + k];
    }
    if (PASS >= 2) { sh.mga[k] = (float)(b[8 + k] / p.e_total); sh.mgza[k] = (float)(b[12 + k] / p.e_total); }
  }
  __syncthreads();
  const float ik = p.enc.drop.on ? p.enc.drop.inv_keep : 1.f;
  constexpr int NV = PASS == 0 ? 8 : (PASS == 1 ? 8 + 16 + 4 : 8 + 4);
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0;
  const int fe = p.enc.fe;
  // dW1 = sum_e dza (x) a is summed against the CENTRED attributes: sum_e dza = 0 in exact arithmetic (BatchNorm backward),
  // so the mean's share is 0 -- but in fp32 that sum leaves a residual (the layer-1 bias gradient, ~1e-6), and raw
  // attributes carry it into dW1 times their mean (distances: mean 11.5, deviation 0.18 on a three-camera graph, where the
  // gradient itself is what remains after the batch terms cancel: 8e-6 on a |grad|max of 2e-3)
  const double ma0 = sc[0] / p.e_total, ma1 = sc[1] / p.e_total;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < p.n_edges; e += nthreads) {
    float a0, a1, u[4], e0[4], zha[4], zhb[4];
    load_attr(p.attr, fe, e, a0, a1);
    // the forward's edge_enc_hidden / edge_enc_out (common.h) over again on the LDS weights, keeping the pre-activations
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float z = wl.b1[k] + wl.w1[k * fe] * a0;
      if (fe > 1) z = fmaf(wl.w1[k * fe + 1], a1, z);
      zha[k] = (z - sh.mua[k]) * sh.ia[k];
      u[k] = fmaxf(fmaf(z, af.s1[k], af.t1[k]), 0.f);
    }
    drop_apply4(p.enc.drop, kDropEncEdge1, (unsigned long long)e * 4, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float z = wl.b2[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) z = fmaf(wl.w2[k * 4 + j], u[j], z);
      zhb[k] = (z - sh.mub[k]) * sh.ib[k];
      e0[k] = fmaxf(fmaf(z, af.s2[k], af.t2[k]), 0.f);
    }
    drop_apply4(p.enc.drop, kDropEncEdge2, (unsigned long long)e * 4, e0);
    const float4 d4 = reinterpret_cast<const float4*>(p.g_e0)[e];
    const float de0[4] = {d4.x, d4.y, d4.z, d4.w};
    float gb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gb[k] = e0[k] > 0.f ? de0[k] * ik : 0.f;
    if (PASS == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { acc[k] += gb[k]; acc[4 + k] += (double)gb[k] * zhb[k]; }
      continue;
    }
    float dzb[4], du[4] = {0, 0, 0, 0}, ga[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dzb[k] = bn_bwd_dz(wl.g2[k], sh.ib[k], gb[k], sh.mgb[k], zhb[k], sh.mgzb[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) du[j] = fmaf(wl.w2[k * 4 + j], dzb[k], du[j]);
#pragma unroll
    for (int k = 0; k < 4; ++k) ga[k] = u[k] > 0.f ? du[k] * ik : 0.f;
    if (PASS == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[k] += ga[k];
        acc[4 + k] += (double)ga[k] * zha[k];
        acc[24 + k] += dzb[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[8 + k * 4 + j] += (double)dzb[k] * u[j];
      }
      continue;
    }
    float dza[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dza[k] = bn_bwd_dz(wl.g1[k], sh.ia[k], ga[k], sh.mga[k], zha[k], sh.mgza[k]);
      acc[8 + k] += dza[k];
      acc[k * 2] += (double)dza[k] * ((double)a0 - ma0);
      acc[k * 2 + 1] += (double)dza[k] * ((double)a1 - ma1);
    }
    if (p.d_attr) {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) { s0 = fmaf(wl.w1[k * fe], dza[k], s0); if (fe > 1) s1 = fmaf(wl.w1[k * fe + 1], dza[k], s1); }
      p.d_attr[e * fe] = s0;
      if (fe > 1) p.d_attr[e * fe + 1] = s1;
    }
  }
  const double s = block_sums_f64<NV>(acc, red);
  if (threadIdx.x < NV) {
    const int i = threadIdx.x;
    if (PASS == 0) unsafeAtomicAdd(p.bst + (blockIdx.x % kStatRep) * kBwdStride + i, s);
    else if (PASS == 1) {
      if (i < 8) unsafeAtomicAdd(p.bst + (blockIdx.x % kStatRep) * kBwdStride + 8 + i, s);
      else if (i < 24) gacc_add(p.gacc, kGaW2 + (i - 8), (float)s);
      else gacc_add(p.gacc, kGaB2 + (i - 24), (float)s);
    } else {
      if (i < 8) { if ((i & 1) < fe) gacc_add(p.gacc, kGaW1 + i, (float)s); }
      else gacc_add(p.gacc, kGaB1 + (i - 8), (float)s);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    const int k = threadIdx.x;
    if (PASS == 1) { p.l2.g[k] = (float)sh.sums[4 + k]; p.l2.bt[k] = (float)sh.sums[k]; }
    if (PASS == 2) { p.l1.g[k] = (float)sh.sums[12 + k]; p.l1.bt[k] = (float)sh.sums[8 + k]; }
  }
}

void launch_bwd_edge_enc(const BwdEncParams& p, int pass, hipStream_t s) {
  const int grid = cap((p.n_edges + 255) / 256);
  if (pass == 0) hipLaunchKernelGGL(bwd_edge_enc_kernel<0>, dim3(grid), dim3(256), 0, s, p);
  else if (pass == 1) hipLaunchKernelGGL(bwd_edge_enc_kernel<1>, dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(bwd_edge_enc_kernel<2>, dim3(grid), dim3(256), 0, s, p);
}

// L == 0 (reference models/mpn.py:295-297): the classifier sits directly on the encoded edges.
// d e0 = Wc^T d logits; dWc = sum_e d logits (x) e0; dbc = sum_e d logits.
__global__ __launch_bounds__(256) void bwd_classify_e0_kernel(EdgeEncParams enc, const float* attr, int64_t n_edges,
                                                              double e_total, const float* cls_w, int n_classes,
                                                              const float* d_logits, float* g_e0, float* gr_cls_w,
                                                              float* gr_cls_b) {
  drop_resolve(enc.drop);
  __shared__ EdgeEncAffine af;
  __shared__ double scratch[kStatAttr + kStatEnc2];
  __shared__ double red[64 * 4];
  edge_enc_affine_to_smem(enc, e_total, 2, &af, scratch);
  constexpr int NV = 4 * MTMC_MAX_CLASSES + MTMC_MAX_CLASSES;
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += nthreads) {
    float a0, a1, u[4], e0[4], de[4] = {0, 0, 0, 0};
    load_attr(attr, enc.fe, e, a0, a1);
    edge_enc_hidden(enc, af, e, a0, a1, u);
    edge_enc_out(enc, af, e, u, e0);
    classifier_bwd<0, 4 * MTMC_MAX_CLASSES>(cls_w, d_logits, e, n_classes, e0, de, acc);
    reinterpret_cast<float4*>(g_e0)[e] = make_float4(de[0], de[1], de[2], de[3]);
  }
  const double s = block_sums_f64<NV>(acc, red);
  if (threadIdx.x < NV) {
    const int i = threadIdx.x;
    if (i < 4 * MTMC_MAX_CLASSES) { if (i / 4 < n_classes) unsafeAtomicAdd(gr_cls_w + i, (float)s); }
    else if (i - 4 * MTMC_MAX_CLASSES < n_classes) unsafeAtomicAdd(gr_cls_b + (i - 4 * MTMC_MAX_CLASSES), (float)s);
  }
}

void launch_bwd_classify_e0(const EdgeEncParams& enc, const float* attr, int64_t n_edges, double e_total, const float* cls_w,
                            int n_classes, const float* d_logits, float* g_e0, float* gr_cls_w, float* gr_cls_b,
                            hipStream_t s) {
  hipLaunchKernelGGL(bwd_classify_e0_kernel, dim3(cap((n_edges + 255) / 256)), dim3(256), 0, s, enc, attr, n_edges, e_total,
                     cls_w, n_classes, d_logits, g_e0, gr_cls_w, gr_cls_b);
}

// the replicated small-gradient sums -> the caller's gradient tensors (one workgroup, the last launch of the backward;
// plain += : nothing else touches these words any more, the node-column blocks of the update weights are other words)
__global__ __launch_bounds__(256) void grad_fold_kernel(GradFoldParams p) {
  const int i = threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < kGradRep; ++r) s += p.gacc[r * kGaccN + i];
  float* dst = nullptr;
  if (i < kGaUnW) dst = p.un.b + i;
  else if (i < kGaClsW) dst = p.un.w + ((i - kGaUnW) >> 2) * p.un_ld + p.un_eoff + ((i - kGaUnW) & 3);
  else if (i < kGaClsB) { if ((i - kGaClsW) / 4 < p.n_classes) dst = p.cls.w + (i - kGaClsW); }
  else if (i < kGaUeB) { if (i - kGaClsB < p.n_classes) dst = p.cls.b + (i - kGaClsB); }
  else if (i < kGaUeW) dst = p.ue.b + (i - kGaUeB);
  else if (i < kGaW2) { const int kk = (i - kGaUeW) >> 3, j = (i - kGaUeW) & 7; if (j < p.nin) dst = p.ue.w + kk * p.ue_ld + p.ue_eoff + j; }
  else if (i < kGaB2) dst = p.l2.w + (i - kGaW2);
  else if (i < kGaW1) dst = p.l2.b + (i - kGaB2);
  else if (i < kGaB1) { const int q = i - kGaW1; if ((q & 1) < p.fe) dst = p.l1.w + (q >> 1) * p.fe + (q & 1); }
  else if (i < kGaB1 + 4) dst = p.l1.b + (i - kGaB1);
  if (dst) *dst += s;
}
void launch_grad_fold(const GradFoldParams& p, hipStream_t s) {
  hipLaunchKernelGGL(grad_fold_kernel, dim3(1), dim3(kGaccN), 0, s, p);
}

}  // namespace mtmc
