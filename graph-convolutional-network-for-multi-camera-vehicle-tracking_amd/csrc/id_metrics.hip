// The ID-overlap counts behind IDF1 / IDP / IDR (reference main.py:166-213, eval/eval.py::eval):
//   filter    per row of a detection table: the centre band (main.py:171-204), the ROI corners (isROIOutlier), and the
//             camera bits of every identity that still has rows
//   finish    identities seen by fewer than min_cameras cameras (removeOutliersSingleCam), repeated (camera, id, frame)
//             rows (removeRepetition), the count of surviving rows
//   prefix    pairs (ground-truth rows x prediction rows) before each (camera, frame) group: one workgroup, a running scan
//   pairs     the hot pass: lanes walk the linearised pair index, so small groups share a wave and a large group spreads
//             over as many waves as it has pairs for; one int32 atomicAdd into C[o][h] per pair within max_dist
//   compact   the non-zero cells of C as (o, h, count) triples
// Tables arrive grouped (a stable sort by (camera, frame, id) done by the caller); nothing read from device memory becomes
// an address before it is checked against the array it indexes.
#include "id_metrics.h"

namespace mtmc {

typedef unsigned long long u64;

// fp64 -> int64 by truncation, as numpy casts; false where the value has no int64 (NaN, +-inf, beyond 2^63): such a
// corner lies outside every mask and is never looked up
__device__ __forceinline__ bool id_trunc(double v, long long* out) {
  if (!(v > -9.2e18 && v < 9.2e18)) return false;
  *out = (long long)v;
  return true;
}

__global__ __launch_bounds__(256) void id_filter_kernel(IdFilterArgs a) {
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += nthreads) {
    const double x = a.boxes[4 * i], y = a.boxes[4 * i + 1], w = a.boxes[4 * i + 2], h = a.boxes[4 * i + 3];
    const int32_t cam = a.cam[i], ident = a.ident[i];
    bool keep = true;
    if (a.border) {
      const double cx = x + w / 2, by = y + h;
      keep = a.x_lo <= cx && cx <= a.x_hi && a.y_lo <= by && by <= a.y_hi;
    }
    if (keep && a.roi && cam >= 0 && cam < a.n_cameras) {
      const int32_t plane = a.plane_of_cam[cam];
      if (plane >= 0 && plane < a.n_planes) {
        const uint8_t* roi = a.roi + (size_t)plane * a.roi_h * a.roi_w;
        long long xc[2], yc[2];
        const bool xin[2] = {id_trunc(x, &xc[0]) && xc[0] >= 0 && xc[0] < a.roi_w,
                             id_trunc(x + w, &xc[1]) && xc[1] >= 0 && xc[1] < a.roi_w};
        const bool yin[2] = {id_trunc(y, &yc[0]) && yc[0] >= 0 && yc[0] < a.roi_h,
                             id_trunc(y + h, &yc[1]) && yc[1] >= 0 && yc[1] < a.roi_h};
#pragma unroll
        for (int ix = 0; ix < 2; ++ix)
#pragma unroll
          for (int iy = 0; iy < 2; ++iy)
            if (xin[ix] && yin[iy] && roi[yc[iy] * a.roi_w + xc[ix]] < 255) keep = false;
      }
    }
    if (keep && cam >= 0 && cam < 64 && ident >= 0 && ident < a.n_ident) atomicOr(a.cameras + ident, 1ull << cam);
    a.stage[i] = keep ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void id_finish_kernel(IdFilterArgs a) {
  __shared__ unsigned sh[1];
  unsigned count[1] = {0};
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += nthreads) {
    const int32_t ident = a.ident[i], group = a.group[i];
    bool keep = a.stage[i] != 0;
    if (keep && a.min_cameras > 0)
      keep = ident >= 0 && ident < a.n_ident && __popcll(a.cameras[ident]) >= a.min_cameras;
    // repeats of one (camera, frame, id) are adjacent, the earliest first: a row goes when an earlier one of its run
    // passed steps 1-2 (step 3 treats the whole run alike)
    if (keep && a.drop_repeats)
      for (int64_t j = i - 1; j >= 0 && a.group[j] == group && a.ident[j] == ident; --j)
        if (a.stage[j]) { keep = false; break; }
    a.keep[i] = keep ? 1 : 0;
    count[0] += keep ? 1u : 0u;
  }
  block_count_add<1>(count, a.kept, sh);
}

// ---- pairs before each group --------------------------------------------------------------------------------------------
constexpr int kIdScanPerThread = 8;

__device__ __forceinline__ long long id_group_pairs(const IdOverlapArgs& a, int64_t g) {
  long long ng = a.gt_off[g + 1] - a.gt_off[g], np = a.pr_off[g + 1] - a.pr_off[g];
  ng = ng < 0 ? 0 : (ng > a.n_gt ? a.n_gt : ng);
  np = np < 0 ? 0 : (np > a.n_pr ? a.n_pr : np);
  return ng * np;
}

__global__ __launch_bounds__(256) void id_prefix_kernel(IdOverlapArgs a) {
  __shared__ long long sh[256];
  const int tid = threadIdx.x;
  long long carry = 0;
  if (tid == 0) a.prefix[0] = 0;
  for (int64_t base = 0; base < a.n_groups; base += 256 * kIdScanPerThread) {
    const int64_t g0 = base + (int64_t)tid * kIdScanPerThread;
    long long v[kIdScanPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kIdScanPerThread; ++k) {
      v[k] = g0 + k < a.n_groups ? id_group_pairs(a, g0 + k) : 0;
      mine += v[k];
    }
    sh[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const long long t = tid >= off ? sh[tid - off] : 0;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    long long run = carry + sh[tid] - mine;
#pragma unroll
    for (int k = 0; k < kIdScanPerThread; ++k) {
      run += v[k];
      if (g0 + k < a.n_groups) a.prefix[g0 + k + 1] = run;
    }
    carry += sh[255];
    __syncthreads();
  }
}

// ---- the hot pass: one int32 atomicAdd into C[o][h] per pair within max_dist (distance and work split: id_metrics.h) ----
__global__ __launch_bounds__(256) void id_pairs_kernel(IdOverlapArgs a) {
  id_walk_pairs(a, [&a](int64_t, long long r, long long c) {
    const int32_t oi = a.gt_ident[r], hi_ = a.pr_ident[c];
    if (oi >= 0 && oi < a.n_obj && hi_ >= 0 && hi_ < a.n_hyp &&
        id_pair_distance(a.gt_boxes + 4 * r, a.pr_boxes + 4 * c) <= a.max_dist)
      atomicAdd(a.cells + (int64_t)oi * a.n_hyp + hi_, 1);
  });
}

__global__ __launch_bounds__(256) void id_compact_kernel(const int32_t* cells, int64_t n_cells, int64_t n_hyp, int32_t* triples,
                                                         int64_t max_triples, u64* counter) {
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_cells; i += nthreads) {
    const int32_t v = cells[i];
    if (v == 0) continue;
    const u64 at = atomicAdd(counter, 1ull);
    if (at < (u64)max_triples) {
      triples[3 * at] = (int32_t)(i / n_hyp);
      triples[3 * at + 1] = (int32_t)(i % n_hyp);
      triples[3 * at + 2] = v;
    }
  }
}

void launch_id_filter(const IdFilterArgs& a, hipStream_t s) {
  const int blocks = blocks_for(a.n, 256, 1024);
  hipLaunchKernelGGL(id_filter_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(id_finish_kernel, dim3(blocks), dim3(256), 0, s, a);
}

void launch_id_prefix(const IdOverlapArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(id_prefix_kernel, dim3(1), dim3(256), 0, s, a);
}

void launch_id_overlap(const IdOverlapArgs& a, hipStream_t s) {
  launch_id_prefix(a, s);
  hipLaunchKernelGGL(id_pairs_kernel, dim3(id_pair_blocks(a)), dim3(256), 0, s, a);
}

void launch_id_compact(const int32_t* cells, int64_t n_obj, int64_t n_hyp, int32_t* triples, int64_t max_triples,
                       unsigned long long* counter, hipStream_t s) {
  hipLaunchKernelGGL(id_compact_kernel, dim3(blocks_for(n_obj * n_hyp, 256, 2048)), dim3(256), 0, s, cells, n_obj * n_hyp, n_hyp,
                     triples, max_triples, counter);
}

}  // namespace mtmc
