// Launch interface between api_mot.hip (the C ABI of mtmc_mot_pairs) and the kernel of mot_metrics.hip: the candidate pairs
// behind the CLEAR MOT scores.  The grouped sides, offsets, keep bytes, pair prefix, pair distance and
// work split are those of the ID-overlap pass (id_metrics.h).
#pragma once
#include "id_metrics.h"

namespace mtmc {

// Byte offsets into the workspace of the candidate pass.
struct MotLayout { size_t prefix, total; };

inline MotLayout mot_layout(int64_t n_groups) {
  MotLayout lo;
  lo.prefix = 0;                                     // pairs before each group
  lo.total = ((size_t)(n_groups + 1) * 8 + 255) / 256 * 256;
  return lo;
}

struct MotPairsArgs {
  IdOverlapArgs side;                                // cells, identities, n_obj and n_hyp are not used
  int32_t* pairs;                                    // [max_pairs][3] = group, ground-truth row, prediction row
  double* dist;                                      // [max_pairs]
  long long max_pairs;
  unsigned long long* counter;                       // [1] candidates found, which may exceed max_pairs
};

void launch_mot_pairs(const MotPairsArgs& a, hipStream_t s);

}  // namespace mtmc
