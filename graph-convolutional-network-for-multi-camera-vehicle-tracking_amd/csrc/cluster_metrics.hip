// How good a tracking result is, on the device (reference inference.py:501-526 with :20-67):
//   mtmc_cluster_scores  the five clustering scores of (ID_GT, ID_pred) that the reference takes from scikit-learn
//                        (adjusted Rand, adjusted mutual information, homogeneity, completeness, V-measure)
//   mtmc_edge_prf        TP / FP / TN / FN, P, R, F and the two per-class figures of compute_P_R_F on int64 predictions
// No dense R x C contingency table is formed: labels and (row, column) cells live in open-addressing tables of
// O(n) slots, and the expected mutual information is summed over pairs of distinct cluster SIZES.
//
// Launch chain of mtmc_cluster_scores (one memset, five kernels, no host read):
//   insert    node i: slot of true[i], slot of pred[i], slot of the cell (row slot, column slot); count each
//   reduce    per slot: R, C, cells, sum a^2, sum b^2, sum n_ij^2, the terms of H_true, H_pred, MI; size histograms
//   sizes     ln k! for k = 0..n; the distinct cluster sizes of either side with their multiplicities
//   emi       one (a, b) size pair per wave, lanes over n_ij
//   finalize  one thread: the scores and the pair confusion
//
// Every fp64 sum over slots or pairs is kept in 2^-55 fixed point in a 64-bit integer: which slot a key lands in depends
// on the order of the insertions, integer addition does not, so the scores are the same bits on every run.  All the
// sums are bounded by a few times ln n < 14, far from 2^8.
#include "api_error.h"
#include "kernels.h"

namespace mtmc {

constexpr int64_t kCsMaxN = 1048576;
// distinct cluster sizes of one side: d of them need d (d + 1) / 2 <= n nodes, so at most 1447 at the n limit
constexpr int kCsMaxSizes = 2048;
constexpr double kCsFix = 36028797018963968.0;      // 2^55
// 64-bit accumulator words
enum { kCsR = 0, kCsC, kCsCells, kCsSumA2, kCsSumB2, kCsSumN2, kCsHt, kCsHp, kCsMi, kCsEmi, kCsNt, kCsNp, kCsAccWords = 16 };

typedef unsigned long long u64;

// byte offsets into the workspace; [0, zero_bytes) is cleared at the start of every call
struct CsLayout {
  int64_t cap;                                       // label / cell table capacity: a power of two >= 2 n (at least 64)
  size_t tkey, pkey, ckey, tcnt, pcnt, ccnt, hist_t, hist_p, sizes, acc, zero_bytes, lg, total;
};

static inline CsLayout cs_layout(int64_t n) {
  CsLayout lo;
  lo.cap = 64;
  while (lo.cap < 2 * n) lo.cap *= 2;
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  const size_t slots = (size_t)lo.cap + 1;           // + the slot of key 0 (cs_slot)
  lo.tkey = take(slots * 8); lo.pkey = take(slots * 8); lo.ckey = take(slots * 8);
  lo.tcnt = take(slots * 4); lo.pcnt = take(slots * 4); lo.ccnt = take(slots * 4);
  lo.hist_t = take((size_t)(n + 1) * 4); lo.hist_p = take((size_t)(n + 1) * 4);
  lo.sizes = take((size_t)4 * kCsMaxSizes * 4);      // sizes true | multiplicities true | sizes pred | multiplicities pred
  lo.acc = take(kCsAccWords * 8);
  lo.zero_bytes = off;
  lo.lg = take((size_t)(n + 1) * 8);                 // ln k!, written in full by cs_sizes_kernel
  lo.total = off;
  return lo;
}

__device__ __forceinline__ u64 cs_mix(u64 x) {       // the splitmix64 finaliser
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// The slot of `key` in a table of `cap` (a power of two) 64-bit words, linear probing, claimed with one 64-bit CAS; no
// lane ever waits for another.  An empty word is 0 (the memset), and the key 0 does not go through the table at all: it
// owns the extra slot `cap`.  So every int64 value, INT64_MIN and INT64_MAX included, is an ordinary label.  At most
// cap / 2 distinct keys are ever inserted, so a probe sequence ends long before it wraps.
__device__ __forceinline__ uint32_t cs_slot(u64* keys, u64 cap, u64 key) {
  if (key == 0) return (uint32_t)cap;
  u64 h = cs_mix(key) & (cap - 1);
  for (u64 probe = 0; probe < cap; ++probe, h = (h + 1) & (cap - 1)) {
    u64 cur = __atomic_load_n(keys + h, __ATOMIC_RELAXED);
    if (cur == 0) {
      cur = atomicCAS(keys + h, 0ull, key);
      if (cur == 0) return (uint32_t)h;
    }
    if (cur == key) return (uint32_t)h;
  }
  return (uint32_t)cap;                              // not reached (the tables are at most half full)
}

__global__ __launch_bounds__(256) void cs_insert_kernel(const int64_t* lt, int64_t st, const int64_t* lp, int64_t sp, int64_t n,
                                                        u64 cap, u64* tkey, u64* pkey, u64* ckey, uint32_t* tcnt,
                                                        uint32_t* pcnt, uint32_t* ccnt) {
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) {
    const uint32_t r = cs_slot(tkey, cap, (u64)lt[i * st]);
    const uint32_t c = cs_slot(pkey, cap, (u64)lp[i * sp]);
    const uint32_t cell = cs_slot(ckey, cap, (((u64)r << 32) | c) + 1);     // r, c <= 2^21: the key is never 0
    atomicAdd(tcnt + r, 1u);
    atomicAdd(pcnt + c, 1u);
    atomicAdd(ccnt + cell, 1u);
  }
}

__device__ __forceinline__ long long cs_fixed(double v) { return __double2ll_rn(v * kCsFix); }

// c / n * ln(num / den) in fixed point.  num and den are integers below 2^53 and the quotient is correctly rounded, so
// a cell that is a whole cluster on both sides (n_ij = a = b: num / den = n a / a^2) gives the very bits of that
// cluster's entropy term (n / a): identical partitions come out as MI == H_true == H_pred, bit for bit.
__device__ __forceinline__ long long cs_term(uint32_t c, double n, double num, double den) {
  return cs_fixed((double)c / n * log(num / den));
}

__global__ __launch_bounds__(256) void cs_reduce_kernel(int64_t n, u64 cap, const u64* ckey, const uint32_t* tcnt,
                                                        const uint32_t* pcnt, const uint32_t* ccnt, uint32_t* hist_t,
                                                        uint32_t* hist_p, u64* acc) {
  __shared__ u64 smem[kCsMi + 1];
  long long v[kCsMi + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double dn = (double)n;
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s <= (int64_t)cap; s += nthreads) {
    const uint32_t a = tcnt[s], b = pcnt[s], c = ccnt[s];
    if (a) {
      ++v[kCsR];
      v[kCsSumA2] += (long long)a * a;
      v[kCsHt] += cs_term(a, dn, dn, (double)a);
      if (a <= n) atomicAdd(hist_t + a, 1u);
    }
    if (b) {
      ++v[kCsC];
      v[kCsSumB2] += (long long)b * b;
      v[kCsHp] += cs_term(b, dn, dn, (double)b);
      if (b <= n) atomicAdd(hist_p + b, 1u);
    }
    if (c) {
      const u64 key = ckey[s] - 1;
      const uint32_t row = (uint32_t)(key >> 32), col = (uint32_t)key;
      ++v[kCsCells];
      v[kCsSumN2] += (long long)c * c;
      if (row <= cap && col <= cap)
        v[kCsMi] += cs_term(c, dn, dn * (double)c, (double)tcnt[row] * (double)pcnt[col]);
    }
  }
  block_count_add<kCsMi + 1>(v, acc, smem);
}

__global__ __launch_bounds__(256) void cs_sizes_kernel(int64_t n, const uint32_t* hist_t, const uint32_t* hist_p,
                                                       uint32_t* sizes, double* lg, u64* acc) {
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= n; k += nthreads) {
    lg[k] = lgamma((double)k + 1.0);
    if (k == 0) continue;
    const uint32_t ct = hist_t[k], cp = hist_p[k];
    if (ct) {
      const u64 at = atomicAdd(acc + kCsNt, 1ull);
      if (at < (u64)kCsMaxSizes) { sizes[at] = (uint32_t)k; sizes[kCsMaxSizes + at] = ct; }
    }
    if (cp) {
      const u64 at = atomicAdd(acc + kCsNp, 1ull);
      if (at < (u64)kCsMaxSizes) { sizes[2 * kCsMaxSizes + at] = (uint32_t)k; sizes[3 * kCsMaxSizes + at] = cp; }
    }
  }
}

// Expected mutual information of two random partitions with the given cluster sizes.  A cluster enters only through its
// size, so the sum over the R x C cluster pairs is a sum over pairs of distinct sizes (a, b), each weighted by how many
// clusters of that size either side has.  One pair per wave, lanes over n_ij = max(1, a + b - n) .. min(a, b):
//   n_ij / n * ln(n n_ij / (a b)) * a! b! (n-a)! (n-b)! / (n! n_ij! (a-n_ij)! (b-n_ij)! (n-a-b+n_ij)!)
__global__ __launch_bounds__(256) void cs_emi_kernel(int64_t n, const uint32_t* sizes, const double* lg, u64* acc) {
  const u64 nt_raw = acc[kCsNt], np_raw = acc[kCsNp];
  const int64_t nt = nt_raw < (u64)kCsMaxSizes ? (int64_t)nt_raw : kCsMaxSizes;
  const int64_t np = np_raw < (u64)kCsMaxSizes ? (int64_t)np_raw : kCsMaxSizes;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const double dn = (double)n, lgn = lg[n];
  long long part = 0;
  for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nt * np; q += nwaves) {
    const int64_t ia = q / np, ib = q - ia * np;
    const int64_t a = sizes[ia], b = sizes[2 * kCsMaxSizes + ib];
    const double weight = (double)sizes[kCsMaxSizes + ia] * (double)sizes[3 * kCsMaxSizes + ib];
    const int64_t lo = a + b - n > 1 ? a + b - n : 1, hi = a < b ? a : b;
    const double ab = (double)a * (double)b;
    const double base = lg[a] + lg[b] + lg[n - a] + lg[n - b] - lgn;
    double sum = 0;
    for (int64_t nij = lo + lane; nij <= hi; nij += 64) {
      const double x = (double)nij;
      const double g = base - lg[nij] - lg[a - nij] - lg[b - nij] - lg[n - a - b + nij];
      sum += x / dn * log(dn * x / ab) * exp(g);
    }
    sum = wave_sum(sum);
    if (lane == kWaveSumLane) part += cs_fixed(weight * sum);
  }
  if (lane == kWaveSumLane && part) atomicAdd(acc + kCsEmi, (u64)part);
}

__device__ __forceinline__ double cs_i128_to_double(__int128 v) {
  const bool neg = v < 0;
  const unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  const double d = (double)(u64)(u >> 64) * 18446744073709551616.0 + (double)(u64)u;
  return neg ? -d : d;
}

// scikit-learn's definitions and special cases (metrics/cluster/_supervised.py), one thread
__global__ void cs_finalize_kernel(int64_t n, const u64* acc, double* scores, long long* counts) {
  const long long R = (long long)acc[kCsR], C = (long long)acc[kCsC];
  const long long A = (long long)acc[kCsSumA2], B = (long long)acc[kCsSumB2], S = (long long)acc[kCsSumN2];
  const double inv = 1.0 / kCsFix;
  const double h_true = (double)(long long)acc[kCsHt] * inv, h_pred = (double)(long long)acc[kCsHp] * inv;
  double mi = (double)(long long)acc[kCsMi] * inv;
  const double emi = (double)(long long)acc[kCsEmi] * inv;
  if (mi < 0.0) mi = 0.0;
  // pair confusion over the n (n - 1) ordered pairs of distinct nodes: the products reach n^4, past int64 from n = 55 000 on, so they are formed in 128 bits
  const long long tp = S - n, fp = B - S, fn = A - S, tn = (long long)n * (n - 1) - tp - fp - fn;
  double ari = 1.0;
  if (fn != 0 || fp != 0) {
    const __int128 num = (__int128)tp * tn - (__int128)fn * fp;
    const __int128 den = (__int128)(tp + fn) * (fn + tn) + (__int128)(tp + fp) * (fp + tn);
    ari = 2.0 * cs_i128_to_double(num) / cs_i128_to_double(den);
  }
  const double hom = h_true == 0.0 ? 1.0 : mi / h_true;
  const double com = h_pred == 0.0 ? 1.0 : mi / h_pred;
  const double v = hom + com == 0.0 ? 0.0 : 2.0 * hom * com / (hom + com);
  double ami = 1.0;
  if (!(R == 1 && C == 1)) {
    const double eps = 2.220446049250313e-16;
    double den = 0.5 * (h_true + h_pred) - emi;
    den = den < 0.0 ? (den < -eps ? den : -eps) : (den > eps ? den : eps);
    ami = (mi - emi) / den;
  }
  scores[0] = ari; scores[1] = ami; scores[2] = hom; scores[3] = com; scores[4] = v;
  scores[5] = h_true; scores[6] = h_pred; scores[7] = mi; scores[8] = emi;
  counts[0] = R; counts[1] = C; counts[2] = (long long)acc[kCsCells];
  counts[3] = tp; counts[4] = fp; counts[5] = fn; counts[6] = tn;
}

// ---- mtmc_edge_prf: compute_P_R_F (reference inference.py:23-68) without its boolean-mask indexing -------------------
__global__ __launch_bounds__(256) void prf_count_kernel(const int64_t* pred, int64_t sp, const int64_t* labels, int64_t sl,
                                                        int64_t n, u64* counts) {
  __shared__ unsigned int sh[4];
  unsigned int c[4] = {0, 0, 0, 0};                  // at most 2^31 / (256 threads) rows per thread
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) {
    const int64_t y = labels[i * sl], p = pred[i * sp];
    if ((y != 0 && y != 1) || (p != 0 && p != 1)) continue;
    ++c[confusion_slot(y == 1, p == 1)];
  }
  block_count_add<4>(c, counts, sh);
}

__global__ void prf_finalize_kernel(const long long* counts, double* out) {
  const double tp = (double)counts[0], fp = (double)counts[1], tn = (double)counts[2], fn = (double)counts[3];
  const double p = tp + fp != 0.0 ? tp / (tp + fp) : 0.0;
  const double r = tp + fn != 0.0 ? tp / (tp + fn) : 0.0;
  out[0] = p; out[1] = r;
  out[2] = p + r != 0.0 ? 2.0 * (p * r) / (p + r) : 0.0;
  out[3] = tn != 0.0 ? tn / (tn + fp) * 100.0 : 0.0;  // "precision_class0": the share of label-0 edges predicted 0, in percent
  out[4] = tp != 0.0 ? tp / (tp + fn) * 100.0 : 0.0;  // "precision_class1"
}

}  // namespace mtmc

extern "C" {

size_t mtmc_cluster_scores_workspace_bytes(int64_t n) {
  return n < 1 || n > mtmc::kCsMaxN ? 0 : mtmc::cs_layout(n).total;
}

int32_t mtmc_cluster_scores(const int64_t* labels_true, int64_t stride_true, const int64_t* labels_pred, int64_t stride_pred,
                            int64_t n, double* scores, int64_t* counts, void* workspace, size_t workspace_bytes,
                            void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  if (n < 1 || n > kCsMaxN) return fail(MTMC_E_ARG, "cluster_scores: n must be in [1, %lld]", (long long)kCsMaxN);
  if (!labels_true || !labels_pred || !scores || !counts || !workspace)
    return fail(MTMC_E_ARG, "cluster_scores: NULL labels_true, labels_pred, scores, counts or workspace");
  if (stride_true < 0 || stride_pred < 0 || ((uintptr_t)workspace & 7))
    return fail(MTMC_E_ARG, "cluster_scores: the strides must be >= 0 and the workspace 8-byte aligned");
  const CsLayout lo = cs_layout(n);
  if (workspace_bytes < lo.total)
    return fail(MTMC_E_ARG, "cluster_scores: workspace has %zu bytes, %zu needed (mtmc_cluster_scores_workspace_bytes)",
                workspace_bytes, lo.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  if (hipMemsetAsync(ws, 0, lo.zero_bytes, s) != hipSuccess) return fail(MTMC_E_HIP, "cluster_scores: hipMemsetAsync failed");
  u64 *tkey = (u64*)(ws + lo.tkey), *pkey = (u64*)(ws + lo.pkey), *ckey = (u64*)(ws + lo.ckey), *acc = (u64*)(ws + lo.acc);
  uint32_t *tcnt = (uint32_t*)(ws + lo.tcnt), *pcnt = (uint32_t*)(ws + lo.pcnt), *ccnt = (uint32_t*)(ws + lo.ccnt);
  uint32_t *hist_t = (uint32_t*)(ws + lo.hist_t), *hist_p = (uint32_t*)(ws + lo.hist_p), *sizes = (uint32_t*)(ws + lo.sizes);
  double* lg = (double*)(ws + lo.lg);
  const u64 cap = (u64)lo.cap;
  hipLaunchKernelGGL(cs_insert_kernel, dim3(blocks_for(n, 256, 1024)), dim3(256), 0, s, labels_true, stride_true, labels_pred,
                     stride_pred, n, cap, tkey, pkey, ckey, tcnt, pcnt, ccnt);
  hipLaunchKernelGGL(cs_reduce_kernel, dim3(blocks_for(lo.cap + 1, 256, 512)), dim3(256), 0, s, n, cap, (const u64*)ckey,
                     (const uint32_t*)tcnt, (const uint32_t*)pcnt, (const uint32_t*)ccnt, hist_t, hist_p, acc);
  hipLaunchKernelGGL(cs_sizes_kernel, dim3(blocks_for(n + 1, 256, 1024)), dim3(256), 0, s, n, (const uint32_t*)hist_t,
                     (const uint32_t*)hist_p, sizes, lg, acc);
  hipLaunchKernelGGL(cs_emi_kernel, dim3(512), dim3(256), 0, s, n, (const uint32_t*)sizes, (const double*)lg, acc);
  hipLaunchKernelGGL(cs_finalize_kernel, dim3(1), dim3(1), 0, s, n, (const u64*)acc, scores,
                     reinterpret_cast<long long*>(counts));
  return mtmc_api::launched("cluster_scores");
}

int32_t mtmc_edge_prf(const int64_t* predictions, int64_t stride_pred, const int64_t* labels, int64_t stride_labels,
                      int64_t n_edges, int64_t* counts, double* out, void* stream) {
  using mtmc_api::fail;
  if (n_edges < 0 || stride_pred < 0 || stride_labels < 0) return fail(MTMC_E_ARG, "edge_prf: n_edges and the strides must be >= 0");
  if (!counts || !out || (n_edges > 0 && (!predictions || !labels)))
    return fail(MTMC_E_ARG, "edge_prf: NULL counts or out, or NULL predictions or labels with n_edges > 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "edge_prf: hipMemsetAsync failed");
  if (n_edges > 0)
    hipLaunchKernelGGL(mtmc::prf_count_kernel, dim3(mtmc::blocks_for(n_edges, 256, 256)), dim3(256), 0, s, predictions, stride_pred,
                       labels, stride_labels, n_edges, reinterpret_cast<mtmc::u64*>(counts));
  hipLaunchKernelGGL(mtmc::prf_finalize_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<const long long*>(counts), out);
  return mtmc_api::launched("edge_prf");
}

}  // extern "C"
