// The candidate pairs behind the CLEAR MOT scores (reference eval/eval.py::eval -> motmetrics' compare_to_groundtruth and
// MOTAccumulator.update): every (ground-truth row, kept prediction row) of one (camera, frame) group whose
// boxes lie within max_dist, with that distance.  The pair test is the one of the ID-overlap pass, so a pair is listed
// here exactly when it counts for IDF1; so is the work split (id_metrics.h): small groups share a wave, a large group
// spreads over as many waves as it has pairs for, and no group has a size limit.
// The list is filled behind a device counter in no particular order (no floating-point atomics); the caller sorts it.
// A lane walks its 16 pairs twice: once to count its candidates, then -- after ONE integer atomic add per wave has reserved
// the wave's slots -- once more to write them.  One add per candidate on the one counter word made the pass 24 times
// longer at 2 M candidates.  A slot at or past max_pairs is counted and not written.
#include "mot_metrics.h"

namespace mtmc {

// Slots for n candidates of every lane of the wave: returns the first slot of this lane.  Called by all 64 lanes.
__device__ __forceinline__ unsigned long long mot_reserve(unsigned n, unsigned long long* counter) {
  const int lane = threadIdx.x & 63;
  unsigned incl = n;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  const unsigned total = __shfl(incl, 63, 64);
  unsigned long long base = 0;
  if (lane == 63 && total) base = atomicAdd(counter, (unsigned long long)total);
  return (unsigned long long)__shfl((long long)base, 63, 64) + (incl - n);
}

__global__ __launch_bounds__(256) void mot_pairs_kernel(MotPairsArgs a) {
  id_for_slices(a.side, [&a](long long p0, long long p1) {
    unsigned n = 0;
    id_walk_slice(a.side, p0, p1, [&a, &n](int64_t, long long r, long long c) {
      n += id_pair_distance(a.side.gt_boxes + 4 * r, a.side.pr_boxes + 4 * c) <= a.side.max_dist ? 1u : 0u;
    });
    unsigned long long at = mot_reserve(n, a.counter);
    if (n == 0) return;
    id_walk_slice(a.side, p0, p1, [&a, &at](int64_t g, long long r, long long c) {
      const double d = id_pair_distance(a.side.gt_boxes + 4 * r, a.side.pr_boxes + 4 * c);
      if (!(d <= a.side.max_dist)) return;
      if (at < (unsigned long long)a.max_pairs) {
        a.pairs[3 * at] = (int32_t)g;
        a.pairs[3 * at + 1] = (int32_t)r;
        a.pairs[3 * at + 2] = (int32_t)c;
        a.dist[at] = d;
      }
      ++at;
    });
  });
}

void launch_mot_pairs(const MotPairsArgs& a, hipStream_t s) {
  launch_id_prefix(a.side, s);
  hipLaunchKernelGGL(mot_pairs_kernel, dim3(id_pair_blocks(a.side)), dim3(256), 0, s, a);
}

}  // namespace mtmc
