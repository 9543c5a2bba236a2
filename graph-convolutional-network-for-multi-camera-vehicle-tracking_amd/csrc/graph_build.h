// What the two graph builders share (graph_build.hip: the reference's all-pairs list; graph_knn.hip: its symmetric
// k-nearest thinning): the edge-attribute expression, the argument checks, the workspace layout and the
// normalise -> Gram sequence.  One copy of each, so an edge both builders emit carries the same bits.
#pragma once
#include "api_error.h"
#include "kernels.h"

namespace mtmc {

// edge_attr[e] = [ ||x_r - x_c + 1e-6||_2 , 1 - cos(x_r, x_c) ] from the Gram entry g = x_r . x_c, nr = |x_r|^2, nc = |x_c|^2,
// sr = sum x_r, sc = sum x_c (graph_build.hip's header comment has the algebra)
__device__ __forceinline__ float2 gb_edge_attr(float g, float nr, float nc, float sr, float sc, int f) {
  const float eps = 1e-6f;                     // F.pairwise_distance eps
  const float d2 = nr + nc - 2.f * g + 2.f * eps * (sr - sc) + (float)f * eps * eps;
  const float dist = sqrtf(fmaxf(d2, 0.f));
  const float cosv = g / (fmaxf(sqrtf(nr), 1e-8f) * fmaxf(sqrtf(nc), 1e-8f));   // F.cosine_similarity eps
  return make_float2(dist, 1.f - cosv);
}

template <class T>
__device__ __forceinline__ int gb_segment_of(const T* off, int n_seg, int64_t v) {   // off[s] <= v < off[s + 1]
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)off[mid] <= v) lo = mid; else hi = mid; }
  return lo;
}

struct EdgeBuildParams {
  const int* in_list; const int* in_off;        // nodes of camera c: in_list[in_off[c] .. in_off[c+1])
  const int* out_list; const int64_t* out_off;  // nodes NOT in camera c, ascending
  const int64_t* block_off;                     // first edge of camera c's block; block_off[n_cams] = E
  int n_cams; int64_t n_nodes; int64_t n_edges; int f;
  const float* G; const float* row_sq; const float* row_sum; const int64_t* node_labels;
  int64_t* edge_index;                          // [E][2] (row, col): its .T is the [2,E] view the callers pass on
  float* edge_attr; float* edge_labels;
};

struct GraphLayout { size_t colsq, row_sq, row_sum, G, zeros, slab, total; };
GraphLayout graph_layout(int64_t n, int f);

// what mtmc_build_graph and mtmc_build_graph_knn refuse alike; `entry` heads the message.  MTMC_OK or the failure's code.
int graph_check_args(const char* entry, const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim,
                     const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                     const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                     const float* x_out, const int64_t* edge_index_out, const float* edge_attr_out,
                     const float* edge_labels_out, const void* workspace);

// x_out = the (column-normalised) features, row_sq / row_sum of its rows and, if `gram`, G = x_out x_out^T, all in the
// workspace `ws` laid out by `l`.  MTMC_OK or the failure's code.
int graph_normalize_gram(const char* entry, const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim,
                         int32_t l2norm, float* x_out, char* ws, const GraphLayout& l, bool gram, hipStream_t s);

}  // namespace mtmc
