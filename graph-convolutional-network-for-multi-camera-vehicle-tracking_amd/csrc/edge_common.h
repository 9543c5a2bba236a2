// What more than one of the per-edge units (edge_prep.hip, edge_pass_a.hip, edge_pass_b.hip, edge_pass_c.hip) uses:
// the non-temporal defaults, the launch grid, and the two per-edge device pieces that passes share.
#pragma once
#include "kernels.h"

namespace mtmc {

// Non-temporal access on the edge streams (tools/edge_nt_sweep.sh; config 4 / config 5, all edge passes of a forward, us):
//   none 737 / 8916 | PA 3 698 / 8892 | PA 4 717 / 8759 | PA 7 708 / 8651 | PA 3 + PC 735 / 8876 | PA 3 + PB 684 / 8698 |
//   PA 7 + PC + PB 724 / 8487.  With PA 11 + PB: 675 / 8714; PA 15 + PB: 689 / 8510 (hence RoundParams::stream_z1).
// The streams of a 10M-edge list (z1: 160 MB) survive in the 256 MB Infinity Cache from one pass to the next unless a pass
// in between pushes them out; those of a 100M-edge list never do.  Taken: row / col ids and the previous z1 non-temporal
// in pass A (its L2 keeps the randomly gathered Pc table instead: 117 -> 99 us per launch at config 4), pass B's stream
// loads non-temporal (48 -> 40 us), z1 stored normally and read normally by pass C so that the next pass finds it cached --
// the regime of config 4 and of an eighth of config 5.
#ifndef PA_NT
#define PA_NT 11          // pass A: 1 row / col ids, 2 previous z1, 4 the z1 store, 8 edge_attr in the first round (126 -> 120 us)
#endif
#ifndef PC_NT
#define PC_NT 0           // stream loads of pass_c_sorted_kernel
#endif
#ifndef PB_NT
#define PB_NT 1           // stream loads of pass B (whole tiles)
#endif

#ifndef MTMC_EDGE_GRID_CAP
#define MTMC_EDGE_GRID_CAP 2048
#endif
static inline int edge_grid(int64_t n_edges, int per_block) {
  const int64_t blocks = (n_edges + per_block - 1) / per_block;
  return (int)(blocks < 1 ? 1 : (blocks > MTMC_EDGE_GRID_CAP ? MTMC_EDGE_GRID_CAP : blocks));
}

// Below kSmallEdges (kernels.h) a pass at 4 edges/thread would leave most of the 256 CUs with one or two waves: use the
// finest decomposition there (measured on camera graphs of 50k..12M edges, tools/size_sweep.py, tools/regime_sweep.py).
static inline int pick_ept(int64_t n_edges) { return n_edges <= kSmallEdges ? 1 : 4; }

// Lazy e' (RoundParams::lazy_e): the edge buffer holds z1, and e' = relu(s1 z1 + t1) is recomputed by whoever reads it
__device__ __forceinline__ void lazy_relu4(float4& v, const float (&s1)[4], const float (&t1)[4]) {
  v.x = fmaxf(fmaf(v.x, s1[0], t1[0]), 0.f); v.y = fmaxf(fmaf(v.y, s1[1], t1[1]), 0.f);
  v.z = fmaxf(fmaf(v.z, s1[2], t1[2]), 0.f); v.w = fmaxf(fmaf(v.w, s1[3], t1[3]), 0.f);
}

// The classifier on one edge (mpn.py:291-292): logit c = cls_w[c] . e + cls_b[c], four FMAs in k order.
__device__ __forceinline__ float cls_chain(const float* w, float b, const float4& e) {
  return fmaf(w[3], e.w, fmaf(w[2], e.z, fmaf(w[1], e.y, fmaf(w[0], e.x, b))));
}
// Any class count (1..MTMC_MAX_CLASSES), weights read where they lie; out: the edge's logits[n_classes], or a local array
__device__ __forceinline__ void classify_edge(const float* cls_w, const float* cls_b, int n_classes, const float4& e, float* out) {
  for (int c = 0; c < n_classes; ++c) out[c] = cls_chain(cls_w + c * 4, cls_b[c], e);
}
// Two classes with the weights in registers (the matrix-core kernels; loaded once per kernel, zeros when `on` is false).
// The two chains are kept apart: paired up by the SLP vectoriser they become v_pk_fma_f32 with op_sel, the form
// tools/check_isa.py bans from kernels with MFMAs
struct Cls2 { float w[2][4] = {}, b[2] = {}; };
__device__ __forceinline__ Cls2 cls2_load(const float* cls_w, const float* cls_b, bool on) {
  Cls2 c;
  if (on)
    for (int i = 0; i < 2; ++i) {
      c.b[i] = cls_b[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) c.w[i][j] = cls_w[i * 4 + j];
    }
  return c;
}
__device__ __forceinline__ float2 classify_edge(const Cls2& c, const float4& e) {
  float lg0 = cls_chain(c.w[0], c.b[0], e);
  asm volatile("" : "+v"(lg0));
  return make_float2(lg0, cls_chain(c.w[1], c.b[1], e));
}

}  // namespace mtmc
