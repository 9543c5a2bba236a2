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

void launch_id_filter(const IdFilterArgs& a, hipStream_t s);
void launch_id_overlap(const IdOverlapArgs& a, hipStream_t s);
void launch_id_compact(const int32_t* cells, int64_t n_obj, int64_t n_hyp, int32_t* triples, int64_t max_triples,
                       unsigned long long* counter, hipStream_t s);

}  // namespace mtmc
