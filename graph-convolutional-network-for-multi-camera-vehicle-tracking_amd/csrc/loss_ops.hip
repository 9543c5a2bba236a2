// Edge-classification loss of the training callers: F.cross_entropy / nn.CrossEntropyLoss(weight, reduction) on the
// [E, C<=4] logits the MPN emits (reference train.py:88-93, :109-142, :178-186).  torch's nll_loss kernels reduce with a
// single block (126 us forward + 54 us backward per classified step on the 173k-edge training graph, i.e. more than
// the whole MPN forward); here log-softmax, weighting and reduction are one pass forward and one pass backward.
//   forward : l_i = w[y_i] * (logsumexp(x_i) - x_i[y_i]);  sums = (sum_i l_i, sum_i w[y_i])  in fp64
//   backward: d x_i[c] = g_i * w[y_i] * (softmax(x_i)[c] - [c == y_i]),
//             g_i = grad / sum_w (mean), grad (sum), grad_i (none);  rows with y_i == ignore_index contribute nothing
#include "api_error.h"
#include "kernels.h"

#include <float.h>

namespace mtmc {

__device__ __forceinline__ void ce_row(const float* x, int C, float (&p)[MTMC_MAX_CLASSES], float& lse) {
  float m = x[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) { p[c] = expf(x[c] - m); s += p[c]; }
  lse = m + logf(s);
  const float inv = 1.f / s;
  for (int c = 0; c < C; ++c) p[c] *= inv;
}

__global__ __launch_bounds__(256) void ce_forward_kernel(const float* logits, const int64_t* labels, const float* weight,
                                                         int64_t n, int C, int64_t ignore_index, float* per_sample,
                                                         double* sums, int64_t period) {
  __shared__ double red[2 * 4];
  double acc[2] = {0, 0};
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) {
    const int64_t y = labels[period ? i % period : i];    // period: the same labels for every classified step
    float l = 0.f, w = 0.f;
    if (y != ignore_index && y >= 0 && y < C) {
      float x[MTMC_MAX_CLASSES], p[MTMC_MAX_CLASSES], lse;
      if (C == 2) { const float2 v = reinterpret_cast<const float2*>(logits)[i]; x[0] = v.x; x[1] = v.y; }
      else for (int c = 0; c < C; ++c) x[c] = logits[i * C + c];
      ce_row(x, C, p, lse);
      w = weight ? weight[y] : 1.f;
      l = w * (lse - x[y]);
    }
    if (per_sample) per_sample[i] = l;
    acc[0] += l;
    acc[1] += w;
  }
  block_atomic_add<2>(acc, sums, 2, red);
}

// totals to sums[0..1]; loss = mean or sum (one thread: 32 additions)
__global__ void ce_finalize_kernel(double* sums, int mode, float* loss_out, double scale) {
  double s1 = 0, s2 = 0;
  for (int r = 0; r < kStatRep; ++r) { s1 += sums[r * 2]; s2 += sums[r * 2 + 1]; }
  sums[0] = s1; sums[1] = s2;
  if (loss_out) loss_out[0] = (float)(mode == 0 ? scale * s1 / s2 : s1);
}

// mode: 0 = mean, 1 = sum, 2 = none (grad is [n] then)
__global__ __launch_bounds__(256) void ce_backward_kernel(const float* logits, const int64_t* labels, const float* weight,
                                                          int64_t n, int C, int64_t ignore_index, int mode,
                                                          const float* grad, const double* sums, float* d_logits,
                                                          int64_t period, double scale) {
  const float g_all = mode == 0 ? (float)(scale * (double)grad[0] / sums[1]) : (mode == 1 ? grad[0] : 0.f);
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) {
    const int64_t y = labels[period ? i % period : i];
    float d[MTMC_MAX_CLASSES] = {0.f, 0.f, 0.f, 0.f};
    if (y != ignore_index && y >= 0 && y < C) {
      float x[MTMC_MAX_CLASSES], p[MTMC_MAX_CLASSES], lse;
      if (C == 2) { const float2 v = reinterpret_cast<const float2*>(logits)[i]; x[0] = v.x; x[1] = v.y; }
      else for (int c = 0; c < C; ++c) x[c] = logits[i * C + c];
      ce_row(x, C, p, lse);
      const float g = (mode == 2 ? grad[i] : g_all) * (weight ? weight[y] : 1.f);
      for (int c = 0; c < C; ++c) d[c] = g * (p[c] - (c == y ? 1.f : 0.f));
    }
    if (C == 2) reinterpret_cast<float2*>(d_logits)[i] = make_float2(d[0], d[1]);
    else for (int c = 0; c < C; ++c) d_logits[i * C + c] = d[c];
  }
}

// Confusion counts of argmax(logits) against 0/1 labels in one pass: what the training / validation loops derive their
// FPR, TPR, precision and recall from (reference train.py:98-107, inference.py:20-67) with boolean-mask indexing, i.e.
// with a device synchronisation per mask.  counts = {TP, FP, TN, FN}; labels other than 0 / 1 are skipped.
__global__ __launch_bounds__(256) void confusion_kernel(const float* logits, const int64_t* labels, int64_t n, int C,
                                                        unsigned long long* counts) {
  __shared__ unsigned int sh[4];
  unsigned int c[4] = {0, 0, 0, 0};
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) {
    const int64_t y = labels[i];
    if (y != 0 && y != 1) continue;
    int best = 0;
    float bv = logits[i * C];
    for (int k = 1; k < C; ++k) { const float v = logits[i * C + k]; if (v > bv) { bv = v; best = k; } }   // first maximum
    ++c[confusion_slot(y == 1, best == 1)];
  }
  block_count_add<4>(c, counts, sh);
}

// Most workgroups (of 256 rows) of a launch.  The backward passes: 2048.  The forward ends in two fp64 atomics per workgroup
// on 16 replicas: 2048 workgroups of one row per thread spent most of their 14.6 us (3 x 173k rows) queueing on those 32
// words; 512 workgroups, four rows per thread there.  The confusion counts: 256.
constexpr int kCeBlocks = 2048, kCeBlocksFwd = 512, kConfusionBlocks = 256;

// ---- mtmc_edge_loss_*: loss and metrics of every classified step in one pass (include/mtmc_mpn.h) -------------------
// Both class counts reduce to one scalar per row, the margin z of the true class (x[y] - x[1-y]; one logit: +-x): the row
// loss is softplus(-z), the true-class probability sigmoid(z), and d loss / d z = -sigmoid(-z).  e = exp(-|z|) <= 1 serves
// all three, so |x| = 80 (e = 0 or tiny) stays finite.
__device__ __forceinline__ void el_row(float z, float& l, float& p, float& q) {   // l = softplus(-z), p = sigmoid(z), q = 1 - p
  const float e = expf(-fabsf(z));
  const float inv = 1.f / (1.f + e);
  l = fmaxf(-z, 0.f) + log1pf(e);
  p = z >= 0.f ? inv : e * inv;
  q = z >= 0.f ? e * inv : inv;
}
// The row loss f and d f / d z of both forms (mtmc_edge_loss_* / mtmc_edge_focal_*).  Plain: f = l, d f / d z = -q.
// FOCAL: f = q^gamma * l and d f / d z = -q^gamma * (gamma * p * l + q): q^(gamma - 1) never appears, so q = 0 (a margin
// past ~ +104, where e is 0) gives f = 0 and d f / d z = 0 for every gamma > 0, and nothing divides by q.  powf on the q of
// el_row, which has no cancellation on either side of z = 0.
template <bool FOCAL>
__device__ __forceinline__ void el_loss_row(float z, float gamma, float& f, float& df, float& p) {
  float l, q;
  el_row(z, l, p, q);
  if (!FOCAL) { f = l; df = -q; return; }
  const float m = powf(q, gamma);
  f = m * l;
  df = -m * (gamma * p * l + q);
}
template <int C>
__device__ __forceinline__ float el_margin(const float* x, int64_t i, bool y, bool& pred) {
  if (C == 2) {
    const float2 v = reinterpret_cast<const float2*>(x)[i];
    pred = v.y > v.x;                                        // argmax == 1; a tie is class 0 (first maximum)
    return y ? v.y - v.x : v.x - v.y;
  }
  const float v = x[i];
  pred = v >= 0.f;
  return y ? v : -v;
}

// scratch: per step kStatRep replicas of kElStride 64-bit words (128 bytes): L0 L1 P0 P1 (f64) | TP FP TN FN (u64) | padding
constexpr int kElStride = 16;

// grid (x: row blocks, y: steps); both dimensions are strided over, so any n and any n_steps run.  The L0 / L1 words hold
// sum f, so both forms share the scratch and the finalize; gamma is read with FOCAL only
template <int C, bool FOCAL>
__global__ __launch_bounds__(256) void el_forward_kernel(const float* logits, const int64_t* labels, int64_t n, int n_steps,
                                                         float gamma, double* scratch) {
  __shared__ double red[4 * 4];
  __shared__ unsigned int cnt[4];
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int s = blockIdx.y; s < n_steps; s += gridDim.y) {
    const float* x = logits + (int64_t)s * n * C;
    double acc[4] = {0, 0, 0, 0};
    unsigned int c[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) {
      const int64_t lab = labels[i];
      if (lab != 0 && lab != 1) continue;
      const bool y = lab == 1;
      bool pred;
      const float z = el_margin<C>(x, i, y, pred);
      float f, df, p;
      el_loss_row<FOCAL>(z, gamma, f, df, p);
      if (y) { acc[1] += f; acc[3] += p; } else { acc[0] += f; acc[2] += p; }
      ++c[confusion_slot(y, pred)];
    }
    double* rep = scratch + (int64_t)s * kStatRep * kElStride;
    block_atomic_add<4>(acc, rep, kElStride, red);
    block_count_add<4>(c, reinterpret_cast<unsigned long long*>(rep + (blockIdx.x % kStatRep) * kElStride + 4), cnt);
  }
}

// one wave: the class weights from the counts, then lane l takes steps l, l + 64, ...; the loss is their wave sum
__global__ __launch_bounds__(64) void el_finalize_kernel(const double* scratch, int n_steps, int C, int weight_mode,
                                                         const float* weight, float fpr_alpha, double* record, float* out,
                                                         long long* confusion) {
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(scratch);
  unsigned long long k0[4] = {0, 0, 0, 0};                        // the label counts are those of any step: step 0
  for (int r = 0; r < kStatRep; ++r)
    for (int j = 0; j < 4; ++j) k0[j] += words[r * kElStride + 4 + j];
  const double n0 = (double)(k0[1] + k0[2]), n1 = (double)(k0[0] + k0[3]);
  double w0 = 1.0, w1 = 1.0;
  if (weight_mode == MTMC_EDGE_W_GIVEN) {
    if (C == 2) { w0 = weight[0]; w1 = weight[1]; } else w1 = weight[0];
  } else if (weight_mode == MTMC_EDGE_W_BALANCED && n0 > 0 && n1 > 0) {
    w1 = n0 / n1;
  }
  const double D = C == 2 ? w0 * n0 + w1 * n1 : n0 + n1;
  float* class_loss = out + 3;
  float* class_prob = class_loss + 2 * (int64_t)n_steps;
  float* fpr_out = class_prob + 2 * (int64_t)n_steps;
  double part = 0;
  for (int s = threadIdx.x; s < n_steps; s += 64) {
    const int64_t base = (int64_t)s * kStatRep * kElStride;
    double f[4] = {0, 0, 0, 0};
    unsigned long long k[4] = {0, 0, 0, 0};
    for (int r = 0; r < kStatRep; ++r)
      for (int j = 0; j < 4; ++j) { f[j] += scratch[base + r * kElStride + j]; k[j] += words[base + r * kElStride + 4 + j]; }
    const double m0 = (double)(k[1] + k[2]), m1 = (double)(k[0] + k[3]);
    const double fpr = m0 > 0 ? (double)k[1] / m0 : 0.0;
    part += (w0 * f[0] + w1 * f[1]) / D + (double)fpr_alpha * fpr;
    class_loss[2 * s] = (float)(m0 > 0 ? f[0] / m0 : 0.0);
    class_loss[2 * s + 1] = (float)(m1 > 0 ? f[1] / m1 : 0.0);
    class_prob[2 * s] = (float)(m0 > 0 ? f[2] / m0 : 0.5);
    class_prob[2 * s + 1] = (float)(m1 > 0 ? f[3] / m1 : 0.5);
    fpr_out[s] = (float)fpr;
    for (int j = 0; j < 4; ++j) confusion[4 * (int64_t)s + j] = (long long)k[j];
  }
  part = wave_sum(part);
  if (threadIdx.x == kWaveSumLane) {
    out[0] = (float)part; out[1] = (float)w0; out[2] = (float)w1;
    record[0] = w0; record[1] = w1; record[2] = D; record[3] = n0 + n1;
  }
}

// per_row [n_steps][n] = w[y] * f, 0 on skipped rows; after the finalize, whose record holds the (possibly balanced) weights
template <int C>
__global__ __launch_bounds__(256) void el_focal_rows_kernel(const float* logits, const int64_t* labels, int64_t n, int n_steps,
                                                            float gamma, const double* record, float* per_row) {
  const float w0 = (float)record[0], w1 = (float)record[1];
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int s = blockIdx.y; s < n_steps; s += gridDim.y) {
    const float* x = logits + (int64_t)s * n * C;
    float* out = per_row + (int64_t)s * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) {
      const int64_t lab = labels[i];
      float v = 0.f;
      if (lab == 0 || lab == 1) {
        const bool y = lab == 1;
        bool pred;
        float f, df, p;
        el_loss_row<true>(el_margin<C>(x, i, y, pred), gamma, f, df, p);
        v = (y ? w1 : w0) * f;
      }
      out[i] = v;
    }
  }
}

// d_logits of the loss: grad[0] / D times the class weight times d f / d z.  PER_ROW (FOCAL only): grad [n_steps][n] is the
// upstream gradient of per_row, one value per row and no division by D
template <int C, bool FOCAL, bool PER_ROW>
__global__ __launch_bounds__(256) void el_backward_kernel(const float* logits, const int64_t* labels, int64_t n, int n_steps,
                                                          const float* grad, const double* record, float gamma,
                                                          float* d_logits) {
  const double gd = PER_ROW ? 1.0 : (double)grad[0] / record[2];
  const float g0 = (float)(gd * record[0]), g1 = (float)(gd * record[1]);
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int s = blockIdx.y; s < n_steps; s += gridDim.y) {
    const float* x = logits + (int64_t)s * n * C;
    float* d = d_logits + (int64_t)s * n * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) {
      const int64_t lab = labels[i];
      float dz = 0.f;                                        // d loss / d z; skipped rows: 0
      const bool y = lab == 1;
      if (lab == 0 || lab == 1) {
        bool pred;
        float f, df, p;
        el_loss_row<FOCAL>(el_margin<C>(x, i, y, pred), gamma, f, df, p);
        dz = (y ? g1 : g0) * df;
        if (PER_ROW) dz *= grad[(int64_t)s * n + i];
      }
      if (C == 2) reinterpret_cast<float2*>(d)[i] = y ? make_float2(-dz, dz) : make_float2(dz, -dz);
      else d[i] = y ? dz : -dz;
    }
  }
}

// x: row blocks up to `cap` workgroups in all (the forward ends in eight 64-bit atomics per workgroup: 512, as kCeBlocksFwd)
static inline dim3 el_grid(int64_t n, int n_steps, int cap) {
  const int gy = n_steps < 1024 ? n_steps : 1024;
  return dim3((unsigned)blocks_for(n, 256, cap / gy < 1 ? 1 : cap / gy), (unsigned)gy);
}

}  // namespace mtmc

extern "C" {

using mtmc_api::fail;
using mtmc_api::launched;

// The argument checks of the four cross-entropy entry points; `entry` starts the error text.  `steps`: n_steps is an
// argument and the reduction is mean or sum; `backward`: grad and d_logits as well, and the sums wherever the mode reads them
// (the plain forward takes any mode: 0 is the mean, everything else the sum, next to the per-sample losses)
static int ce_check(const char* entry, bool steps, bool backward, const float* logits, const int64_t* labels, int64_t n,
                    int32_t n_classes, int32_t n_steps, int32_t mode, const float* grad, const double* sums,
                    const float* d_logits) {
  if (!logits || !labels || (backward ? !grad || !d_logits || (steps && !sums) : !sums))
    return fail(MTMC_E_ARG, "%s: NULL logits, labels%s", entry,
                !backward ? " or sums" : steps ? ", grad, sums or d_logits" : ", grad or d_logits");
  if (n < 0 || n_steps < 1 || n_classes < 1 || n_classes > MTMC_MAX_CLASSES)
    return fail(MTMC_E_ARG, "%s: n must be >= 0%s and n_classes in [1, %d]", entry, steps ? ", n_steps >= 1" : "", MTMC_MAX_CLASSES);
  if (steps && (mode < 0 || mode > 1)) return fail(MTMC_E_ARG, "%s: mode must be 0 (mean) or 1 (sum)", entry);
  if (!steps && backward && (mode < 0 || mode > 2 || (mode == 0 && !sums)))
    return fail(MTMC_E_ARG, "%s: mode must be 0 (mean, with the forward's sums), 1 (sum) or 2 (none)", entry);
  if (n_classes == 2 && (((uintptr_t)logits & 7) || (backward && ((uintptr_t)d_logits & 7))))
    return fail(MTMC_E_ARG, "%s: [n, 2] logits%s must be 8-byte aligned", entry, backward ? " and d_logits" : "");
  return MTMC_OK;
}

// The training loop's `sum(criterion(step, labels) for step in outputs['classified_edges'])` (reference train.py:118-138:
// every classified step against the SAME labels) is one pass over the [n_steps][n][C] logits block the forward emits, as
// n * n_steps rows whose labels repeat with period n: with equal labels the weight sums of the steps are equal, so
// sum_s mean_s = n_steps * (sum of all terms / sum of all weights).  The plain entry points: n_steps = 1, period = 0.
static int ce_forward(const char* entry, const float* logits, const int64_t* labels, const float* weight, int64_t n,
                      int32_t n_classes, int32_t n_steps, int64_t period, int64_t ignore_index, int32_t mode, float* per_sample,
                      double* sums, float* loss_out, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(sums, 0, sizeof(double) * 2 * mtmc::kStatRep, s) != hipSuccess)
    return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
  if (n > 0)
    hipLaunchKernelGGL(mtmc::ce_forward_kernel, dim3(mtmc::blocks_for(n * n_steps, 256, mtmc::kCeBlocksFwd)), dim3(256), 0, s,
                       logits, labels, weight, n * n_steps, n_classes, ignore_index, per_sample, sums, period);
  hipLaunchKernelGGL(mtmc::ce_finalize_kernel, dim3(1), dim3(1), 0, s, sums, mode, loss_out, (double)n_steps);
  return launched(entry);
}

static int ce_backward(const char* entry, const float* logits, const int64_t* labels, const float* weight, int64_t n,
                       int32_t n_classes, int32_t n_steps, int64_t period, int64_t ignore_index, int32_t mode,
                       const float* grad, const double* sums, float* d_logits, void* stream) {
  if (n > 0)
    hipLaunchKernelGGL(mtmc::ce_backward_kernel, dim3(mtmc::blocks_for(n * n_steps, 256, mtmc::kCeBlocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), logits, labels, weight, n * n_steps, n_classes, ignore_index, mode,
                       grad, sums, d_logits, period, (double)n_steps);
  return launched(entry);
}

int32_t mtmc_cross_entropy_forward(const float* logits, const int64_t* labels, const float* weight, int64_t n, int32_t n_classes,
                                   int64_t ignore_index, int32_t mode, float* per_sample, double* sums, float* loss_out,
                                   void* stream) {
  const char* entry = "cross_entropy_forward";
  if (const int rc = ce_check(entry, false, false, logits, labels, n, n_classes, 1, mode, nullptr, sums, nullptr)) return rc;
  return ce_forward(entry, logits, labels, weight, n, n_classes, 1, 0, ignore_index, mode, per_sample, sums, loss_out, stream);
}

int32_t mtmc_cross_entropy_backward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                    int32_t n_classes, int64_t ignore_index, int32_t mode, const float* grad,
                                    const double* sums, float* d_logits, void* stream) {
  const char* entry = "cross_entropy_backward";
  if (const int rc = ce_check(entry, false, true, logits, labels, n, n_classes, 1, mode, grad, sums, d_logits)) return rc;
  return ce_backward(entry, logits, labels, weight, n, n_classes, 1, 0, ignore_index, mode, grad, sums, d_logits, stream);
}

// mode 0 = mean per step (then summed), 1 = sum
int32_t mtmc_cross_entropy_steps_forward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                         int32_t n_classes, int32_t n_steps, int64_t ignore_index, int32_t mode,
                                         double* sums, float* loss_out, void* stream) {
  const char* entry = "cross_entropy_steps_forward";
  if (const int rc = ce_check(entry, true, false, logits, labels, n, n_classes, n_steps, mode, nullptr, sums, nullptr)) return rc;
  return ce_forward(entry, logits, labels, weight, n, n_classes, n_steps, n, ignore_index, mode, nullptr, sums, loss_out, stream);
}

int32_t mtmc_cross_entropy_steps_backward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                          int32_t n_classes, int32_t n_steps, int64_t ignore_index, int32_t mode,
                                          const float* grad, const double* sums, float* d_logits, void* stream) {
  const char* entry = "cross_entropy_steps_backward";
  if (const int rc = ce_check(entry, true, true, logits, labels, n, n_classes, n_steps, mode, grad, sums, d_logits)) return rc;
  return ce_backward(entry, logits, labels, weight, n, n_classes, n_steps, n, ignore_index, mode, grad, sums, d_logits, stream);
}

int32_t mtmc_edge_confusion(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int64_t* counts,
                            void* stream) {
  if (!logits || !labels || !counts) return fail(MTMC_E_ARG, "edge_confusion: NULL logits, labels or counts");
  if (n < 0 || n_classes < 2 || n_classes > MTMC_MAX_CLASSES)
    return fail(MTMC_E_ARG, "edge_confusion: n must be >= 0 and n_classes in [2, %d]", MTMC_MAX_CLASSES);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "edge_confusion: hipMemsetAsync failed");
  if (n > 0)
    hipLaunchKernelGGL(mtmc::confusion_kernel, dim3(mtmc::blocks_for(n, 256, mtmc::kConfusionBlocks)), dim3(256), 0, s, logits,
                       labels, n, n_classes, reinterpret_cast<unsigned long long*>(counts));
  return launched("edge_confusion");
}

size_t mtmc_edge_loss_scratch_bytes(int32_t n_steps) {
  return n_steps < 1 ? 0 : (size_t)n_steps * mtmc::kStatRep * mtmc::kElStride * sizeof(double);
}

// the argument checks the plain and the focal entry points share; `entry` starts the error text
static int el_check_forward(const char* entry, const float* logits, const int64_t* labels, int64_t n, int32_t n_classes,
                            int32_t n_steps, int32_t weight_mode, const float* weight, const void* scratch,
                            size_t scratch_bytes, const double* record, const float* out, const int64_t* confusion) {
  if (!logits || !labels || !scratch || !record || !out || !confusion)
    return fail(MTMC_E_ARG, "%s: NULL logits, labels, scratch, record, out or confusion", entry);
  if (n < 0 || n_steps < 1 || (n_classes != 1 && n_classes != 2))
    return fail(MTMC_E_ARG, "%s: n must be >= 0, n_steps >= 1 and n_classes 1 or 2", entry);
  if (weight_mode < MTMC_EDGE_W_ONE || weight_mode > MTMC_EDGE_W_BALANCED || (weight_mode == MTMC_EDGE_W_GIVEN && !weight))
    return fail(MTMC_E_ARG, "%s: weight_mode must be MTMC_EDGE_W_ONE, _GIVEN (with weight) or _BALANCED", entry);
  if ((n_classes == 2 && ((uintptr_t)logits & 7)) || ((uintptr_t)scratch & 7))
    return fail(MTMC_E_ARG, "%s: [n, 2] logits and scratch must be 8-byte aligned", entry);
  const size_t need = mtmc_edge_loss_scratch_bytes(n_steps);
  if (scratch_bytes < need)
    return fail(MTMC_E_ARG, "%s: scratch has %zu bytes, %zu needed (mtmc_edge_loss_scratch_bytes)", entry, scratch_bytes, need);
  return MTMC_OK;
}

static int el_check_backward(const char* entry, const float* logits, const int64_t* labels, int64_t n, int32_t n_classes,
                             int32_t n_steps, const float* grad, const double* record, const float* d_logits) {
  if (!logits || !labels || !grad || !record || !d_logits)
    return fail(MTMC_E_ARG, "%s: NULL logits, labels, grad, record or d_logits", entry);
  if (n < 0 || n_steps < 1 || (n_classes != 1 && n_classes != 2))
    return fail(MTMC_E_ARG, "%s: n must be >= 0, n_steps >= 1 and n_classes 1 or 2", entry);
  if (n_classes == 2 && (((uintptr_t)logits & 7) || ((uintptr_t)d_logits & 7)))
    return fail(MTMC_E_ARG, "%s: [n, 2] logits and d_logits must be 8-byte aligned", entry);
  return MTMC_OK;
}

static int el_check_gamma(const char* entry, float gamma) {
  if (!(gamma >= 0.f) || gamma > FLT_MAX) return fail(MTMC_E_ARG, "%s: gamma must be finite and >= 0", entry);
  return MTMC_OK;
}

// Both forward entry points: check, memset, row pass, finalize; with per_row one more launch after the finalize, whose
// record holds the weights.  The plain one passes gamma = 0 and no per_row
static int el_forward(const char* entry, bool focal, const float* logits, const int64_t* labels, int64_t n, int32_t n_classes,
                      int32_t n_steps, int32_t weight_mode, const float* weight, float fpr_alpha, void* scratch,
                      size_t scratch_bytes, double* record, float* out, int64_t* confusion, float gamma, float* per_row,
                      void* stream) {
  if (const int rc = el_check_forward(entry, logits, labels, n, n_classes, n_steps, weight_mode, weight, scratch, scratch_bytes,
                                      record, out, confusion))
    return rc;
  if (const int rc = el_check_gamma(entry, gamma)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(scratch, 0, mtmc_edge_loss_scratch_bytes(n_steps), s) != hipSuccess)
    return fail(MTMC_E_HIP, "%s: hipMemsetAsync failed", entry);
  double* acc = static_cast<double*>(scratch);
  const bool two = n_classes == 2;
  if (n > 0) {
    const auto pass = focal ? (two ? mtmc::el_forward_kernel<2, true> : mtmc::el_forward_kernel<1, true>)
                            : (two ? mtmc::el_forward_kernel<2, false> : mtmc::el_forward_kernel<1, false>);
    hipLaunchKernelGGL(pass, mtmc::el_grid(n, n_steps, 512), dim3(256), 0, s, logits, labels, n, n_steps, gamma, acc);
  }
  hipLaunchKernelGGL(mtmc::el_finalize_kernel, dim3(1), dim3(64), 0, s, acc, n_steps, n_classes, weight_mode, weight,
                     fpr_alpha, record, out, reinterpret_cast<long long*>(confusion));
  if (per_row && n > 0) {
    const auto rows = two ? mtmc::el_focal_rows_kernel<2> : mtmc::el_focal_rows_kernel<1>;
    hipLaunchKernelGGL(rows, mtmc::el_grid(n, n_steps, 2048), dim3(256), 0, s, logits, labels, n, n_steps, gamma, record, per_row);
  }
  return launched(entry);
}

// Both backward entry points: check, then the instantiation (per-row gradients exist in the focal form only)
static int el_backward(const char* entry, bool focal, const float* logits, const int64_t* labels, int64_t n, int32_t n_classes,
                       int32_t n_steps, const float* grad, const double* record, float* d_logits, float gamma, bool per_row,
                       void* stream) {
  if (const int rc = el_check_backward(entry, logits, labels, n, n_classes, n_steps, grad, record, d_logits)) return rc;
  if (const int rc = el_check_gamma(entry, gamma)) return rc;
  if (n > 0) {
    const bool two = n_classes == 2;
    const auto pass = !focal    ? (two ? mtmc::el_backward_kernel<2, false, false> : mtmc::el_backward_kernel<1, false, false>)
                      : per_row ? (two ? mtmc::el_backward_kernel<2, true, true> : mtmc::el_backward_kernel<1, true, true>)
                                : (two ? mtmc::el_backward_kernel<2, true, false> : mtmc::el_backward_kernel<1, true, false>);
    hipLaunchKernelGGL(pass, mtmc::el_grid(n, n_steps, 2048), dim3(256), 0, static_cast<hipStream_t>(stream), logits, labels, n,
                       n_steps, grad, record, gamma, d_logits);
  }
  return launched(entry);
}

int32_t mtmc_edge_loss_forward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                               int32_t weight_mode, const float* weight, float fpr_alpha, void* scratch,
                               size_t scratch_bytes, double* record, float* out, int64_t* confusion, void* stream) {
  return el_forward("edge_loss_forward", false, logits, labels, n, n_classes, n_steps, weight_mode, weight, fpr_alpha, scratch,
                    scratch_bytes, record, out, confusion, 0.f, nullptr, stream);
}

int32_t mtmc_edge_loss_backward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                                const float* grad, const double* record, float* d_logits, void* stream) {
  return el_backward("edge_loss_backward", false, logits, labels, n, n_classes, n_steps, grad, record, d_logits, 0.f, false,
                     stream);
}

int32_t mtmc_edge_focal_forward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                                int32_t weight_mode, const float* weight, float fpr_alpha, void* scratch,
                                size_t scratch_bytes, double* record, float* out, int64_t* confusion, float gamma,
                                float* per_row, void* stream) {
  return el_forward("edge_focal_forward", true, logits, labels, n, n_classes, n_steps, weight_mode, weight, fpr_alpha, scratch,
                    scratch_bytes, record, out, confusion, gamma, per_row, stream);
}

int32_t mtmc_edge_focal_backward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                                 const float* grad, const double* record, float* d_logits, float gamma, int32_t grad_per_row,
                                 void* stream) {
  return el_backward("edge_focal_backward", true, logits, labels, n, n_classes, n_steps, grad, record, d_logits, gamma,
                     grad_per_row != 0, stream);
}

}  // extern "C"
