// Launch interface between api_id.hip (the C ABI of mtmc_id_filter / mtmc_id_overlap / mtmc_id_cells) and the kernels of
// id_metrics.hip: the ID-overlap counts behind IDF1 / IDP / IDR.
#pragma once
#include "kernels.h"

namespace mtmc {

constexpr int kIdPairsPerLane = 16;                  // consecutive pairs of the linearised pair index one lane walks
constexpr int kIdPairsPerBlock = 256 * kIdPairsPerLane;

// One table of rows in grouped order for the filter pass ([n] each; boxes [n][4] fp64 = x, y, width, height).
struct IdFilterArgs {
  const double* boxes; const int32_t* cam; const int32_t* ident; const int32_t* group; int64_t n;
  int64_t n_ident; int32_t n_cameras;
  double x_lo, x_hi, y_lo, y_hi; int32_t border;      // step 1: keep iff x_lo <= x + w / 2 <= x_hi and y_lo <= y + h <= y_hi
  const uint8_t* roi; const int32_t* plane_of_cam; int32_t n_planes, roi_h, roi_w;   // step 2 (roi == nullptr: off)
  int32_t min_cameras, drop_repeats;                  // steps 3 and 4
  uint8_t* stage; uint8_t* keep;                      // after steps 1-2 | after all four
  unsigned long long* cameras;                        // [n_ident] camera bits of the rows that passed steps 1-2
  unsigned long long* kept;                           // [1] rows that survive
};

// Byte offsets into the workspace of the overlap pass.
struct IdLayout { size_t cells, prefix, total; };

inline IdLayout id_layout(int64_t n_obj, int64_t n_hyp, int64_t n_groups) {
  IdLayout lo;
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  lo.cells = take((size_t)(n_obj * n_hyp) * 4);      // C [n_obj][n_hyp] int32, at the start: a caller may look at it
  lo.prefix = take((size_t)(n_groups + 1) * 8);      // pairs before each group
  lo.total = off;
  return lo;
}

struct IdOverlapArgs {
  const double* gt_boxes; const double* pr_boxes;     // rows sorted by group, [.][4]
  const int64_t* gt_off; const int64_t* pr_off;       // [n_groups + 1] each, over the union of the group keys
  const int32_t* gt_ident; const int32_t* pr_ident;   // compact identities
  const uint8_t* gt_keep; const uint8_t* pr_keep;     // gt_keep may be nullptr (all kept)
  int64_t n_gt, n_pr, n_groups, n_obj, n_hyp;
  double max_dist;
  long long* prefix; int32_t* cells;
};

// ---- the overlap of one pair ---------------------------------------------------------------------------------------------
// d = 1 - I / U with I = iw ih and U = aw ah + bw bh - I, every operation rounded on its own: a fused multiply-add in U
// moves its last bit and with it a pair that sits on the threshold.  U = 0 gives NaN, which is not <= max_dist.
__device__ __forceinline__ double id_pair_distance(const double* a, const double* b) {
#pragma clang fp contract(off)
  const double ax = a[0], ay = a[1], aw = a[2], ah = a[3], bx = b[0], by = b[1], bw = b[2], bh = b[3];
  const double iw = fmax(0.0, fmin(ax + aw, bx + bw) - fmax(ax, bx));
  const double ih = fmax(0.0, fmin(ay + ah, by + bh) - fmax(ay, by));
  const double inter = iw * ih;
  const double area_a = aw * ah, area_b = bw * bh;
  const double uni = area_a + area_b - inter;
  return 1.0 - inter / uni;
}

// ---- the work split of the pair passes -------------------------------------------------------------------------------------
// Lanes walk the linearised pair index behind a.prefix: a lane owns kIdPairsPerLane consecutive pairs, a workgroup
// kIdPairsPerBlock, grid-stride.  visit(group, ground-truth row, prediction row) is called for every pair whose rows lie
// inside their tables and are both kept; it is the one place where the overlap pass (id_metrics.hip) and the candidate
// pass (mot_metrics.hip) differ.
// One lane's slice [p0, p1) of the pair index (p1 <= prefix[n_groups]; an empty slice is legal):
template <class Visit>
__device__ __forceinline__ void id_walk_slice(const IdOverlapArgs& a, long long p0, long long p1, Visit&& visit) {
  if (p0 >= p1) return;
  int64_t g = 0, hi = a.n_groups;                    // prefix[g] <= p0 < prefix[hi]
  while (hi - g > 1) {
    const int64_t mid = g + (hi - g) / 2;
    if (a.prefix[mid] <= p0) g = mid; else hi = mid;
  }
  long long g0 = a.gt_off[g], q0 = a.pr_off[g], np = a.pr_off[g + 1] - q0;
  np = np > a.n_pr ? a.n_pr : np;                    // (as id_group_pairs clamps it; np >= 1: the group has pairs)
  long long local = p0 - a.prefix[g];
  long long o = local / np, h = local - o * np;
  for (long long p = p0; p < p1; ++p) {
    const long long r = g0 + o, c = q0 + h;
    if (r >= 0 && r < a.n_gt && c >= 0 && c < a.n_pr && a.pr_keep[c] && (!a.gt_keep || a.gt_keep[r])) visit(g, r, c);
    if (++h == np) {
      h = 0;
      ++o;
      if (p + 1 < p1 && a.prefix[g + 1] == p + 1) {    // the group is done: on to the next one that has pairs
        do ++g; while (g + 1 < a.n_groups && a.prefix[g + 1] == a.prefix[g]);
        g0 = a.gt_off[g]; q0 = a.pr_off[g]; np = a.pr_off[g + 1] - q0;
        np = np > a.n_pr ? a.n_pr : np;
        o = 0;
      }
    }
  }
}

// The grid-stride loop over the slices: step(p0, p1) once per lane and round, by EVERY lane of the workgroup (a lane past
// the end gets an empty slice), so a step may use wave-wide operations.
template <class Step>
__device__ __forceinline__ void id_for_slices(const IdOverlapArgs& a, Step&& step) {
  const long long total = a.prefix[a.n_groups];
  const long long stride = (long long)gridDim.x * kIdPairsPerBlock;
  for (long long base = (long long)blockIdx.x * kIdPairsPerBlock; base < total; base += stride) {
    const long long p0 = base + (long long)threadIdx.x * kIdPairsPerLane;
    step(p0 < total ? p0 : total, p0 + kIdPairsPerLane < total ? p0 + kIdPairsPerLane : total);
  }
}

template <class Visit>
__device__ __forceinline__ void id_walk_pairs(const IdOverlapArgs& a, Visit&& visit) {
  id_for_slices(a, [&](long long p0, long long p1) { id_walk_slice(a, p0, p1, visit); });
}

inline int id_pair_blocks(const IdOverlapArgs& a) {
  // the pair count stays on the device: n_gt n_pr (both below 2^31) bounds it, the grid rule caps the launch
  return blocks_for(a.n_gt * a.n_pr, kIdPairsPerBlock, 2048);
}

void launch_id_filter(const IdFilterArgs& a, hipStream_t s);
void launch_id_prefix(const IdOverlapArgs& a, hipStream_t s);  // a.prefix [n_groups + 1] = the pairs before each group
void launch_id_overlap(const IdOverlapArgs& a, hipStream_t s);
void launch_id_compact(const int32_t* cells, int64_t n_obj, int64_t n_hyp, int32_t* triples, int64_t max_triples,
                       unsigned long long* counter, hipStream_t s);

}  // namespace mtmc
