// C-ABI entry points for ONE linear layer (include/mtmc_mpn.h): the stand-alone MLP layer, and the mtmc_linear_*_raw
// diagnostics that run a layer on the node-encoder kernel the forward would pick for it.  Launch-only, like the forward.
#include "api_error.h"
#include "kernels.h"

using mtmc_api::fail;

extern "C" {

int32_t mtmc_mlp_layer_forward(const mtmc_layer* layer, const float* x, int64_t x_row_stride, int64_t rows, float* y,
                               double* stats_scratch, void* stream) {
  if (!layer || !layer->weight || !layer->bias || !x || !y || rows < 1) return fail(MTMC_E_ARG, "bad mlp layer arguments");
  const bool bn = layer->gamma != nullptr;
  if (bn && (!layer->beta || !stats_scratch)) return fail(MTMC_E_ARG, "BatchNorm layer needs beta and stats_scratch[2*out]");
  if (bn && rows < 2) return fail(MTMC_E_ROWS, "Expected more than 1 value per channel when training");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (bn && hipMemsetAsync(stats_scratch, 0, 2 * (size_t)layer->out_dim * sizeof(double), s) != hipSuccess)
    return fail(MTMC_E_HIP, "hipMemsetAsync failed");
  mtmc::GemmParams g =
      mtmc::plain_gemm(x, x_row_stride, layer->weight, layer->bias, y, layer->out_dim, rows, layer->in_dim, layer->out_dim);
  if (bn) g.stats_out = stats_scratch;
  if (int rc = mtmc::launch_gemm_bn(g, s)) return fail(rc, "unsupported layer shape");
  if (bn)
    mtmc::launch_bn_relu_rows({y, layer->out_dim, rows, layer->out_dim, stats_scratch, layer->gamma, layer->beta, (double)rows, y,
                               mtmc::kNoDrop, 0}, s);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MTMC_OK : fail(MTMC_E_HIP, "mlp layer launch failed: %s", hipGetErrorString(e));
}

// ---- Diagnostics / unit tests: one encoder layer on the kernel the forward would run it on.  In all four, scratch: u32[48] =
// the |A|max, |W|max, |Y|max words; stats: f64[2*N] column sum / sumsq of Y, or NULL; work: kernels.h raw_work unless said.
static int raw_begin(uint32_t* scratch, double* stats, int N, hipStream_t s) {
  return mtmc::clear_raw(scratch, stats, N, s) ? MTMC_OK : fail(MTMC_E_HIP, "hipMemsetAsync failed");
}
static int raw_end(int rc) {       // rc: the launcher's answer (kernels.h: MTMC_OK, MTMC_E_ARG, MTMC_E_HIP)
  if (rc) return fail(rc, "unsupported shape or launch refused");
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MTMC_OK : fail(MTMC_E_HIP, "launch failed: %s", hipGetErrorString(e));
}
// |A|max -> scratch[0] and (W given) |W|max -> scratch[1], by prep_kernel's passenger workgroups as in the forward
static void raw_amax(const float* A, int64_t lda, int64_t M, const float* W, int K, int N, uint32_t* scratch, hipStream_t s) {
  mtmc::PrepParams p = {};
  p.jobs[p.n_jobs++] = {A, M, K, lda, scratch, 0, 0};
  if (W) p.jobs[p.n_jobs++] = {W, N, K, K, scratch + mtmc::kAmaxRep, 0, 0};
  mtmc::launch_prep(p, s);
}

// Y[M][N] = A[M][K] . W[N][K]^T + bias through the node encoder's GEMM dispatch exactly as the forward uses it for layer 0
// (fp16 two-piece kernel where it applies).
int32_t mtmc_linear_raw(const float* A, int64_t lda, const float* W, const float* bias, float* Y, int64_t M, int32_t K,
                        int32_t N, uint32_t* scratch, double* stats, void* stream) {
  if (!A || !W || !bias || !Y || !scratch || M < 1 || K < 32 || K % 32 || N < 1) return fail(MTMC_E_ARG, "bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = raw_begin(scratch, stats, N, s)) return rc;
  raw_amax(A, lda, M, W, K, N, scratch, s);
  mtmc::GemmParams g = mtmc::plain_gemm(A, lda, W, bias, Y, N, M, K, N, scratch, scratch + mtmc::kAmaxRep, scratch + 2 * mtmc::kAmaxRep);
  g.stats_out = stats;
  return raw_end(mtmc::launch_gemm_bn(g, s));
}

// A layer >= 1 of a many-row graph: Y[M][N] = relu(bn(A))[M][K] . W[N][K]^T + bias, bn = BatchNorm with the given column
// statistics (f64 sum[K] | sumsq[K] over `count` rows) and gamma / beta -- on the role-split kernel (gemm_staged.hip:
// N % 256 == 0, or N = 128) or, for the narrow last layer (K = 128, N = 32), the row-streaming kernel (gemm_rows.hip).
// work: >= 4*N*K + 4*N + 256 bytes (the role-split kernel's weight planes, their row scales on the next 256-byte boundary).
int32_t mtmc_linear_staged_raw(const float* A, int64_t lda, const double* stats_in, const float* gamma_in, const float* beta_in,
                               double count, const float* W, const float* bias, float* Y, int64_t M, int32_t K, int32_t N,
                               void* work, uint64_t work_bytes, uint32_t* scratch, double* stats, void* stream) {
  const bool narrow = K == 128 && N == 32;
  if (!A || !stats_in || !gamma_in || !beta_in || !W || !bias || !Y || !work || !scratch || M < 1 || K < 64 || K % 32 || K > 2048 ||
      (!narrow && N != 128 && (N < 256 || N % 256)) || lda < K || (lda & 3) || ((uintptr_t)A & 15))
    return fail(MTMC_E_ARG, "bad arguments");
  const uint64_t iw_off = ((uint64_t)N * K * 4 + 255) / 256 * 256;
  if (work_bytes < iw_off + (uint64_t)N * 4) return fail(MTMC_E_ARG, "work buffer too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = raw_begin(scratch, stats, N, s)) return rc;
  raw_amax(A, lda, M, nullptr, K, N, scratch, s);
  if (narrow) {
    mtmc::GemmParams g = mtmc::plain_gemm(A, lda, W, bias, Y, N, M, K, N, scratch, nullptr, scratch + 2 * mtmc::kAmaxRep);
    g.stats_in = stats_in; g.gamma_in = gamma_in; g.beta_in = beta_in; g.count = count; g.stats_out = stats;
    return raw_end(mtmc::launch_gemm_rows(g, s));
  }
  mtmc::StagedGemmParams g;
  mtmc::set_in(&g, A, lda, stats_in, gamma_in, beta_in, count);
  g.amax_a = scratch;
  float* inv_w = reinterpret_cast<float*>(static_cast<char*>(work) + iw_off);
  mtmc::launch_split_rows(W, K, N, K, work, inv_w, s);
  g.Wh = static_cast<_Float16*>(work); g.inv_w = inv_w;
  mtmc::set_out(&g, bias, Y, N, M, K, N, stats, scratch + 2 * mtmc::kAmaxRep);
  return raw_end(mtmc::launch_gemm_staged(g, s));
}

// A layer of a few-row graph (gemm_few.hip): layer 0 (stats_in == NULL: x is split into planes too) or a layer >= 1.
int32_t mtmc_linear_few_raw(const float* A, int64_t lda, const double* stats_in, const float* gamma_in, const float* beta_in,
                            double count, const float* W, const float* bias, float* Y, int64_t M, int32_t K, int32_t N,
                            void* work, uint64_t work_bytes, double* stats, void* stream) {
  const bool l0 = stats_in == nullptr;
  if (!A || !W || !bias || !Y || !work || M < 1 || K < 32 || K > 2048 || N < 1 || lda < K || (lda & 3) || ((uintptr_t)A & 15) ||
      (l0 ? !mtmc::few_l0_shape(K, N) : (!mtmc::few_wave_shape(K, N) || !gamma_in || !beta_in)))
    return fail(MTMC_E_ARG, "bad arguments");
  const mtmc::RawWork wk = mtmc::raw_work(work, M, K, N, l0);
  if (work_bytes < wk.bytes) return fail(MTMC_E_ARG, "work buffer too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = raw_begin(nullptr, stats, N, s)) return rc;
  mtmc::launch_split_rows(W, K, N, K, wk.Wh, wk.inv_w, s);
  if (l0) {
    mtmc::launch_split_rows(A, lda, M, K, wk.Ah, wk.inv_a, s);
    mtmc::FewL0Params g;
    g.Ah = wk.Ah; g.inv_a = wk.inv_a; g.Wh = wk.Wh; g.inv_w = wk.inv_w;
    mtmc::set_out(&g, bias, Y, N, M, K, N, stats);
    return raw_end(mtmc::launch_few_l0(g, s));
  }
  mtmc::FewWaveParams g;
  mtmc::set_in(&g, A, lda, stats_in, gamma_in, beta_in, count);
  g.Wh = wk.Wh; g.inv_w = wk.inv_w;
  mtmc::set_out(&g, bias, Y, N, M, K, N, stats);
  return raw_end(mtmc::launch_few_wave(g, s));
}

// Layer 0 of a many-row graph on pre-split operands (gemm_presplit.hip); reuse_planes: the planes in `work` are those of the
// call before (times the GEMM alone).
int32_t mtmc_linear_presplit_raw(const float* A, int64_t lda, const float* W, const float* bias, float* Y, int64_t M,
                                 int32_t K, int32_t N, void* work, uint64_t work_bytes, uint32_t* scratch, double* stats,
                                 int32_t reuse_planes, void* stream) {
  if (!A || !W || !bias || !Y || !work || !scratch || M < 1 || K < 64 || K % 64 || K > 2048 || N < 1)
    return fail(MTMC_E_ARG, "bad arguments");
  const mtmc::RawWork wk = mtmc::raw_work(work, M, K, N, true);
  if (work_bytes < wk.bytes) return fail(MTMC_E_ARG, "work buffer too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = raw_begin(scratch, stats, N, s)) return rc;
  if (!reuse_planes) {
    mtmc::launch_split_rows(A, lda, M, K, wk.Ah, wk.inv_a, s);
    mtmc::launch_split_rows(W, K, N, K, wk.Wh, wk.inv_w, s);
  }
  mtmc::SplitGemmParams g;
  g.Ah = wk.Ah; g.inv_a = wk.inv_a; g.Wh = wk.Wh; g.inv_w = wk.inv_w;
  mtmc::set_out(&g, bias, Y, N, M, K, N, stats, scratch + 2 * mtmc::kAmaxRep);
  return raw_end(mtmc::launch_gemm_presplit(g, s));
}

}  // extern "C"
