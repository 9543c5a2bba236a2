// Internals shared by the C-ABI translation units (api.hip: forward + phases, api_train.hip: backward):
// model and call checks, workspace carving, the call's plan and context, and the parameter blocks both directions fill.
#pragma once
#include "api_error.h"
#include "kernels.h"
#include "train_kernels.h"

#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace mtmc_api {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

struct Layout {
  mtmc_ws_layout pub;
  size_t row32, col32, e_buf[2], Q, slab, enc_aff, row_start, carry;
  size_t col_sub; int col_blocks;              // column-blocked pass A: int[N][col_blocks + 1] sub-run boundaries (0 blocks: none)
  size_t amax;                                 // u32[1 + 2*MTMC_MAX_ENC_LAYERS][kAmaxRep]: |x|max, -, |Y_l|max (zeroed)
  size_t amax_w;                               // u32[MTMC_MAX_ENC_LAYERS][kAmaxRep]: |W_l|max of the in-loop layers
  size_t Y[MTMC_MAX_ENC_LAYERS];
  // training: every round keeps its own buffers (the workspace is the backward tape) + backward scratch
  bool training;
  std::vector<size_t> z_tr, e_tr, h_tr;       // per round: z1 [E][4], e' [E][4], aggregated h [N][32]
  std::vector<size_t> P_tr, Q_tr;             // per round: the node projections [2][N][4], [N][32]
  size_t xh, inv_a;                            // fp16 planes + row scales of x: layer 0 on pre-split operands (w_ws[0]), or few
  bool few;                                    // few-row graphs (gemm_few.hip): xh / inv_a hold the planes of x (W: weight-plane cache)
  // layer l's weight planes + row scales live in the workspace: many-row graphs in eval mode, layer 0 on pre-split operands
  // (gemm_presplit.hip), layers >= 1 on the role-split kernel (gemm_staged.hip).  (A call with a weight-plane cache reads that.)
  size_t wh[MTMC_MAX_ENC_LAYERS], inv_w[MTMC_MAX_ENC_LAYERS]; bool w_ws[MTMC_MAX_ENC_LAYERS];
  size_t g_e[2], g_e0, g_h[2], g_h0, g_P, g_Q, g_de2, g_arg;   // gradients wrt e_r, e0, h_r, h0, P, Q; A^T dz2 [E][4]
  size_t bst;                                  // f64[2L+1][kStatRep][kBwdStride] backward statistics blocks (train_kernels.h)
  size_t bwd_zero, bwd_zero_end;               // the range the backward clears with one memset
  size_t gacc;                                 // f32[kGradRep][kGaccN] (train_kernels.h)
  size_t amax_bwd;                             // u32[2][MTMC_MAX_ENC_LAYERS][kAmaxRep] (zeroed with the backward scratch)
  size_t seed_word = 0;
  size_t gA, gB, tA, tB, tW, tX, zeros, bst_n; // node-encoder backward: gradient ping-pong, transposes, 0-bias, column stats
};

// The weight-plane cache (mtmc_mpn_call::weight_cache; split_body.h): per node-encoder layer the fp16 planes [2][K/32][out][32],
// the inverse row scales [out] and one 64-bit fingerprint per 8-row chunk.  Depends on the model's dimensions only.
struct CacheLayout { size_t planes[MTMC_MAX_ENC_LAYERS], inv[MTMC_MAX_ENC_LAYERS], fp[MTMC_MAX_ENC_LAYERS]; bool has[MTMC_MAX_ENC_LAYERS]; size_t total; };
inline void make_cache_layout(const mtmc_mpn_model* m, CacheLayout* cl) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  for (int l = 0; l < MTMC_MAX_ENC_LAYERS; ++l) {
    cl->has[l] = l < m->n_enc_layers && m->enc_node[l].in_dim % 8 == 0 && m->enc_node[l].in_dim <= 2048;
    cl->planes[l] = cl->inv[l] = cl->fp[l] = 0;
    if (!cl->has[l]) continue;
    const size_t K = m->enc_node[l].in_dim, O = m->enc_node[l].out_dim;
    cl->planes[l] = take(4 * O * K);
    cl->inv[l] = take(4 * O);
    cl->fp[l] = take(8 * ((O + 7) / 8));
  }
  cl->total = off;
}
// the node encoder's shape admits the few-row kernels for `rows` rows (gemm_few.hip; knobs included)
inline bool few_shape(const mtmc_mpn_model* m, int64_t rows) {
  int in_dim[MTMC_MAX_ENC_LAYERS], out_dim[MTMC_MAX_ENC_LAYERS];
  for (int l = 0; l < m->n_enc_layers; ++l) { in_dim[l] = m->enc_node[l].in_dim; out_dim[l] = m->enc_node[l].out_dim; }
  return mtmc::few_rows_path(rows, m->n_enc_layers, in_dim, out_dim);
}

// width of [h0 | h], the node part of the update MLPs' inputs
inline int node_in_width(const mtmc_mpn_model* m) { return (m->reattach_nodes ? 2 : 1) * MTMC_NODE_DIM; }
// the first step (round + 1) whose edge state is classified (mpn.py:277; num_class_steps > num_enc_steps classifies every round)
inline int first_cls_step(const mtmc_mpn_model* m) { return std::max(1, m->num_enc_steps - m->num_class_steps + 1); }

inline int check_model(const mtmc_mpn_model* m) {
  if (!m) return fail(MTMC_E_ARG, "model is NULL");
  if (m->struct_bytes != sizeof(mtmc_mpn_model))
    return fail(MTMC_E_ARG, "mtmc_mpn_model.struct_bytes is %u, this library's struct has %zu bytes (ABI v%d): rebuild the caller against include/mtmc_mpn.h",
                m->struct_bytes, sizeof(mtmc_mpn_model), MTMC_MPN_ABI_VERSION);
  if (m->n_enc_layers < 1 || m->n_enc_layers > MTMC_MAX_ENC_LAYERS) return fail(MTMC_E_ARG, "n_enc_layers out of range");
  for (int l = 0; l < m->n_enc_layers; ++l) {
    const mtmc_layer& L = m->enc_node[l];
    if (!L.weight || !L.bias || !L.gamma || !L.beta) return fail(MTMC_E_ARG, "node encoder layer %d: NULL parameter", l);
    if (L.in_dim % 32 || L.in_dim < 32 || L.out_dim < 1) return fail(MTMC_E_ARG, "node encoder layer %d: in_dim must be a positive multiple of 32", l);
    if (l && L.in_dim != m->enc_node[l - 1].out_dim) return fail(MTMC_E_ARG, "node encoder layer %d: in_dim != previous out_dim", l);
  }
  if (m->enc_node[m->n_enc_layers - 1].out_dim != MTMC_NODE_DIM) return fail(MTMC_E_ARG, "node encoder must end at width %d", MTMC_NODE_DIM);
  if ((m->enc_edge[0].in_dim != 1 && m->enc_edge[0].in_dim != 2) || m->enc_edge[0].out_dim != 4 ||
      m->enc_edge[1].in_dim != 4 || m->enc_edge[1].out_dim != 4)
    return fail(MTMC_E_ARG, "edge encoder must be in(1|2)->4->4");
  const int hn = node_in_width(m), he = (m->reattach_edges ? 2 : 1) * MTMC_EDGE_DIM;
  if (m->upd_edge.in_dim != 2 * hn + he || m->upd_edge.out_dim != 4) return fail(MTMC_E_ARG, "edge update layer must be [4, %d]", 2 * hn + he);
  if (m->upd_node.in_dim != hn + 4 || m->upd_node.out_dim != MTMC_NODE_DIM) return fail(MTMC_E_ARG, "node update layer must be [32, %d]", hn + 4);
  if (m->cls.in_dim != 4 || m->cls.out_dim < 1 || m->cls.out_dim > MTMC_MAX_CLASSES) return fail(MTMC_E_ARG, "classifier must be [C<=4, 4]");
  const mtmc_layer* small[] = {&m->enc_edge[0], &m->enc_edge[1], &m->upd_edge, &m->upd_node};
  for (const mtmc_layer* L : small)
    if (!L->weight || !L->bias || !L->gamma || !L->beta) return fail(MTMC_E_ARG, "NULL parameter in an edge/update layer");
  if (!m->cls.weight || !m->cls.bias) return fail(MTMC_E_ARG, "NULL classifier parameter");
  if (m->agg < 0 || m->agg > 2) return fail(MTMC_E_ARG, "agg must be MTMC_AGG_SUM/MEAN/MAX");
  if (m->num_enc_steps < 0 || m->num_class_steps < 0) return fail(MTMC_E_ARG, "negative step count");
  return MTMC_OK;
}

inline void make_layout(const mtmc_mpn_model* m, int64_t N, int64_t E, Layout* lo, bool training = false) {
  *lo = Layout();
  lo->training = training;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  const int L = m->num_enc_steps;
  lo->pub.flags_off = take(8 * sizeof(int32_t));
  // the edge branch's two statistics blocks sit right in front of node-encoder layer 0's / layer 1's column statistics: a
  // multi-GPU host all-reduces each pair as ONE message (mtmc_ws_layout, distributed.py)
  lo->pub.stat_attr_off = take((size_t)mtmc::kStatRep * mtmc::kAttrStride * sizeof(double));
  lo->pub.stat_enc_layer_off[0] = take(2 * (size_t)m->enc_node[0].out_dim * sizeof(double));
  lo->pub.stat_enc2_off = take((size_t)mtmc::kStatRep * mtmc::kEnc2Stride * sizeof(double));
  for (int l = 1; l < m->n_enc_layers; ++l) lo->pub.stat_enc_layer_off[l] = take(2 * (size_t)m->enc_node[l].out_dim * sizeof(double));
  lo->pub.stat_round_off = take((size_t)(L > 0 ? L : 1) * mtmc::kRoundBlock * sizeof(double));
  lo->pub.deg_off = take((size_t)N * sizeof(int32_t));
  lo->pub.seg_off = take(mtmc::fold_node_stat(E) ? 0 : (size_t)N * 4 * sizeof(double));   // (few-edge lists: none)
  lo->amax = take((size_t)(1 + 2 * MTMC_MAX_ENC_LAYERS) * mtmc::kAmaxRep * sizeof(uint32_t));
  lo->amax_w = take((size_t)MTMC_MAX_ENC_LAYERS * mtmc::kAmaxRep * sizeof(uint32_t));
  lo->pub.zero_bytes = off;
  lo->pub.deg_global_off = take((size_t)N * sizeof(int32_t));
  lo->pub.h0_off = take((size_t)N * 32 * sizeof(float));
  lo->pub.h_acc_off[0] = take((size_t)N * 32 * sizeof(float));
  lo->pub.h_acc_off[1] = take((size_t)N * 32 * sizeof(float));
  lo->enc_aff = take(16 * sizeof(float));
  lo->seed_word = take(sizeof(unsigned long long));     // MTMC_F_SEED_ON_DEVICE: this forward's Dropout seed (stays on the tape)
  lo->row_start = take((size_t)N * sizeof(int32_t));
  lo->carry = take((size_t)((E + 31) / 32) * 2 * 32 * sizeof(float));
  lo->col_blocks = mtmc::plan_col_blocks(N, E, 1e30, training);      // by table size and edge count alone (the call adds the degree)
  lo->col_sub = take(lo->col_blocks > 0 ? (size_t)N * (lo->col_blocks + 1) * sizeof(int32_t) : 0);
  lo->pub.P_off = take((size_t)N * 8 * sizeof(float));
  lo->Q = take((size_t)N * 32 * sizeof(float));
  lo->row32 = take((size_t)E * sizeof(int32_t));
  lo->col32 = take((size_t)E * sizeof(int32_t));
  lo->e_buf[0] = take((size_t)E * 4 * sizeof(float));
  lo->e_buf[1] = take((size_t)E * 4 * sizeof(float));
  for (int l = 0; l < m->n_enc_layers; ++l) lo->Y[l] = take((size_t)N * m->enc_node[l].out_dim * sizeof(float));
  size_t slab = 0;                                 // split-K scratch of the node encoder (few-row graphs only)
  for (int l = 0; l < m->n_enc_layers; ++l) {
    int sk;
    mtmc::gemm_plan(N, m->enc_node[l].in_dim, m->enc_node[l].out_dim, &sk);
    const size_t need = sk > 1 ? (size_t)sk * N * m->enc_node[l].out_dim * sizeof(float) : 0;
    if (need > slab) slab = need;
  }
  lo->slab = take(slab);
  // Layer 0 of a many-row graph runs on operands split ONCE into fp16 pairs (gemm_presplit.hip): planes of x [2][N][K]
  // and of W0 [2][out][K] plus one power-of-two scale per row.  An x-sized region; eval mode only.
  lo->few = few_shape(m, N);                  // (the call also needs a weight-plane cache: make_plan; training forwards too)
  for (int l = 0; l < m->n_enc_layers; ++l) {
    const int K = m->enc_node[l].in_dim, O = m->enc_node[l].out_dim;
    lo->w_ws[l] = !training && (l == 0 ? mtmc::presplit_layer0(N, K, O) : mtmc::staged_layer(N, K, O));
  }
  if (lo->w_ws[0] || lo->few) {
    lo->xh = take((size_t)2 * N * m->enc_node[0].in_dim * sizeof(uint16_t));
    lo->inv_a = take((size_t)N * sizeof(float));
  }
  for (int l = 0; l < m->n_enc_layers; ++l)    // (without a weight-plane cache the layer's weight planes are made per call, here)
    if (lo->w_ws[l]) {
      lo->wh[l] = take((size_t)2 * m->enc_node[l].out_dim * m->enc_node[l].in_dim * sizeof(uint16_t));
      lo->inv_w[l] = take((size_t)m->enc_node[l].out_dim * sizeof(float));
    }
  if (training) {
    for (int r = 0; r < L; ++r) {
      lo->z_tr.push_back(take((size_t)E * 4 * sizeof(float)));
      lo->e_tr.push_back(take((size_t)E * 4 * sizeof(float)));
      lo->h_tr.push_back(take((size_t)N * 32 * sizeof(float)));
      lo->P_tr.push_back(r == 0 ? lo->pub.P_off : take((size_t)N * 8 * sizeof(float)));   // the round's projections stay on
      lo->Q_tr.push_back(r == 0 ? lo->Q : take((size_t)N * 32 * sizeof(float)));          // the tape: the backward reads them as is
    }
    // everything the backward accumulates into, contiguous: ONE memset clears it (api_train.hip)
    size_t maxd = 0, bn_stats = 0;
    for (int l = 0; l < m->n_enc_layers; ++l) {
      maxd = std::max(maxd, (size_t)m->enc_node[l].in_dim);
      maxd = std::max(maxd, (size_t)m->enc_node[l].out_dim);
      bn_stats += 2 * (size_t)m->enc_node[l].out_dim;
    }
    lo->bwd_zero = off;
    lo->bst = take((size_t)(2 * L + 1) * mtmc::kStatRep * mtmc::kBwdStride * sizeof(double));   // per round: node, edge; + encoder
    lo->bst_n = take(bn_stats * sizeof(double));
    lo->gacc = take((size_t)mtmc::kGradRep * mtmc::kGaccN * sizeof(float));   // small-gradient replicas
    lo->amax_bwd = take((size_t)2 * MTMC_MAX_ENC_LAYERS * mtmc::kAmaxRep * sizeof(uint32_t));   // |dY_l|max, |a_{l-1}|max
    lo->g_P = take((size_t)(L > 0 ? L : 1) * mtmc::kGradRep * N * 8 * sizeof(float));   // per round: [kGradRep][N][8]
    lo->g_Q = take((size_t)(L > 0 ? L : 1) * N * 32 * sizeof(float));     // per round
    lo->zeros = take(maxd * sizeof(float));
    lo->g_h0 = take((size_t)N * 32 * sizeof(float));
    lo->g_e0 = take((size_t)E * 4 * sizeof(float));
    lo->g_e[0] = take((size_t)E * 4 * sizeof(float));
    lo->g_h[0] = take((size_t)N * 32 * sizeof(float));
    lo->bwd_zero_end = off;
    lo->g_e[1] = take((size_t)E * 4 * sizeof(float));
    lo->g_h[1] = take((size_t)N * 32 * sizeof(float));
    lo->g_de2 = take((size_t)E * 4 * sizeof(float));
    lo->g_arg = take((size_t)N * 32 * sizeof(int32_t));
    const size_t npad = (size_t)((N + 31) / 32 * 32);
    lo->gA = take((size_t)N * maxd * sizeof(float));
    lo->gB = take((size_t)N * maxd * sizeof(float));
    lo->tA = take(npad * maxd * sizeof(float));
    lo->tB = take(npad * maxd * sizeof(float));
    size_t wsum = 0;                                   // every W_l^T and x^T at once: one transpose launch (api_train.hip)
    for (int l = 0; l < m->n_enc_layers; ++l) wsum += (size_t)m->enc_node[l].in_dim * m->enc_node[l].out_dim;
    lo->tW = take(wsum * sizeof(float));
    lo->tX = take(npad * (size_t)m->enc_node[0].in_dim * sizeof(float));
  }
  lo->pub.total_bytes = off;
}

constexpr int kMaxPanels = 16;
struct SidePipe;                 // side stream + events of the pipelined layer 0 (api.hip)

// Row panels of the pipelined layer 0: cuts[0..np] (multiples of the tile height), np <= kMaxPanels; *bm = the tile height
// of every panel (what the whole matrix would pick).  One round = 256 workgroups = 256 / tiles_n row tiles.
inline int l0_panels(int64_t rows, int Nout, int64_t* cuts, int* bm) {
  const int tiles_n = (Nout + 255) / 256;
  *bm = mtmc::presplit_tile_rows(rows, tiles_n);
  const int64_t per_round = (int64_t)(256 / tiles_n > 0 ? 256 / tiles_n : 1) * *bm;
  const int mode = mtmc::knobs().l0_pipeline;
  int np = 0;
  int64_t at = 0, k = 1;
  cuts[0] = 0;
  while (at < rows) {
    int64_t take = per_round * (mode == 3 ? 2 : mode == 2 ? 1 : k);
    if (np == kMaxPanels - 1 || at + take > rows) take = rows - at;
    at += take;
    cuts[++np] = at;
    if (k < 8) k *= 2;
  }
  return np;
}

// Which kernels one call runs, decided once (make_plan): the launches read it and mtmc_mpn_plan_call reports it.
struct CallPlan {
  int64_t rows;                                  // node_hi - node_lo: the rows the node encoder encodes here
  int enc_kernel[MTMC_MAX_ENC_LAYERS];           // MTMC_GEMM_* per node-encoder layer
  int enc_split_k[MTMC_MAX_ENC_LAYERS];          // > 1: the in-loop kernel slices K into the slab, MTMC_PH_NODE_COMBINE adds up
  bool w_cached[MTMC_MAX_ENC_LAYERS];            // the layer's weight planes are in the weight-plane cache (else the workspace)
  int l0_panels, l0_bm;                          // pre-split layer 0 in row panels [l0_cuts[i], l0_cuts[i+1]) of tile height l0_bm
  int64_t l0_cuts[kMaxPanels + 1];               // (1 panel: one split pass, one GEMM)
  bool enc2_may_ride;                            // enc2 may ride in the last encoder layer's launch (mtmc_mpn_forward decides)
  int edges_per_thread;                          // passes A / B
  bool lazy_edges;                               // e' is never stored: passes B / C and the next pass A recompute it from z1
  bool fold_node_stat;                           // few-edge list: node-update statistics out of node_proj + pass B
  double avg_degree;                             // edges per source row of this call's edges
  int col_blocks;                                // column blocks of pass A (0: edge order)
  mtmc::PassC pass_c;                            // plan_pass_c (RoundParams::pass_c)
  // the public value names the matrix-core kernel the call launches, with or without the walk behind it
  int pass_c_pub() const {
    switch (pass_c) {
      case mtmc::kPassCSortedWalk: case mtmc::kPassCSortedDet: return MTMC_PASS_C_MFMA_SORTED;
      case mtmc::kPassCAnyWalk: case mtmc::kPassCAny: return MTMC_PASS_C_MFMA_ANY;
      default: return MTMC_PASS_C_WALK;
    }
  }
};

inline bool in_loop_kernel(int k) { return k == MTMC_GEMM_GENERIC || k == MTMC_GEMM_INLOOP_64 || k == MTMC_GEMM_INLOOP_128; }

// From the call's sizes, ranges, flags and mode, the layout and the knobs.  No pointer of the call is read (weight_cache is
// only tested for NULL), so the host-only query builds the same plan.  The layout says what the WHOLE graph qualifies for
// (few, w_ws[l]); a layer takes a kernel when this call's rows qualify too.
inline void make_plan(const mtmc_mpn_model* m, const mtmc_mpn_call* c, const Layout& lo, const CacheLayout& cl, CallPlan* p) {
  *p = CallPlan();
  const int64_t N = c->n_nodes, E = c->n_edges, rows = c->node_hi - c->node_lo;
  const mtmc_layer& L0 = m->enc_node[0];
  p->rows = rows;
  const bool pre0 = lo.w_ws[0] && mtmc::presplit_layer0(rows, L0.in_dim, L0.out_dim);
  bool few = lo.few && c->weight_cache != nullptr && few_shape(m, rows);     // (training forwards too)
  for (int l = 0; l < m->n_enc_layers; ++l) few = few && cl.has[l];
  for (int l = 0; l < m->n_enc_layers; ++l) {
    const mtmc_layer& Ll = m->enc_node[l];
    int k, sk = 1;
    if (few) k = l == 0 ? MTMC_GEMM_FEW_L0 : MTMC_GEMM_FEW_WAVE;
    else if (l == 0 && pre0) k = MTMC_GEMM_PRESPLIT_256;
    else if (l >= 1 && lo.w_ws[l] && mtmc::staged_layer(rows, Ll.in_dim, Ll.out_dim)) k = MTMC_GEMM_STAGED_128;
    else if (l >= 1 && !lo.training && mtmc::rows_layer(N, Ll.in_dim, Ll.out_dim) && mtmc::rows_layer(rows, Ll.in_dim, Ll.out_dim))
      k = MTMC_GEMM_ROWS_16;        // narrow last layers of many-row graphs
    else {                          // the slab was sized for N rows; a shard with fewer rows may plan a larger split: then none
      int sk_full = 1, sk_here = 1;
      mtmc::gemm_plan(N, Ll.in_dim, Ll.out_dim, &sk_full);
      const int cfg = rows > 0 ? mtmc::gemm_plan(rows, Ll.in_dim, Ll.out_dim, &sk_here) : 0;
      k = cfg == 2 ? MTMC_GEMM_INLOOP_128 : cfg == 1 ? MTMC_GEMM_INLOOP_64 : MTMC_GEMM_GENERIC;
      if (sk_here > 1 && (size_t)sk_here * rows <= (size_t)(sk_full > 1 ? sk_full : 0) * N) sk = sk_here;
    }
    p->enc_kernel[l] = k;
    p->enc_split_k[l] = sk;
    p->w_cached[l] = c->weight_cache != nullptr && cl.has[l] && !in_loop_kernel(k) && k != MTMC_GEMM_ROWS_16;
  }
  p->l0_panels = 1;
  if (p->enc_kernel[0] == MTMC_GEMM_PRESPLIT_256 && mtmc::knobs().l0_pipeline > 0)
    p->l0_panels = l0_panels(rows, L0.out_dim, p->l0_cuts, &p->l0_bm);
  // Few-row graphs: the last node-encoder layer is a handful of workgroups (S02: 8), and the edge branch's second kernel (enc2:
  // moments of the edge encoder's hidden layer, needed from the first round on) is independent of the whole encoder chain -- it
  // can ride in that launch as passenger workgroups (GemmParams / FewWaveParams::pass_*; -1 launch per forward): on the
  // 64 x 64-tile in-loop kernel, or on the few-row kernel's 256-thread form (enc2_body's workgroup size)
  const int last = m->n_enc_layers - 1, kl = p->enc_kernel[last];
  p->enc2_may_ride = E > 0 && E <= mtmc::kSmallEdges &&
                     (kl == MTMC_GEMM_INLOOP_64 || (kl == MTMC_GEMM_FEW_WAVE && mtmc::few_wave_threads(m->enc_node[last].in_dim) == 256));
  p->edges_per_thread = mtmc::plan_edges_per_thread(E);
  p->lazy_edges = !lo.training && E > mtmc::kSmallEdges;
  p->fold_node_stat = mtmc::fold_node_stat(E);
  // Row-complete shard: local edges over the rows the call owns; anything else (one GPU, or an edge-range shard that shares
  // rows with its neighbours): the whole graph's E / N.  (Round 2 divided the LOCAL edge count by the GLOBAL node count:
  // 8 ranks of config 5 saw 12 instead of 100 and left the matrix-core kernel.)
  if (c->row_hi > 0) p->avg_degree = c->row_hi > c->row_lo ? (double)E / (double)(c->row_hi - c->row_lo) : 0.0;
  else p->avg_degree = N > 0 ? (double)c->n_edges_total / (double)N : 0.0;
  // the layout has the sub-run index (table size, edge count) AND the call's own degree pays
  p->col_blocks = (m->num_enc_steps > 0 && lo.col_blocks > 0 &&
                   mtmc::plan_col_blocks(N, E, p->avg_degree, lo.training) == lo.col_blocks) ? lo.col_blocks : 0;
  const bool drop_n = lo.training && m->dropout_upd_node > 0.f;
  p->pass_c = mtmc::plan_pass_c(m->agg, (c->flags & MTMC_F_DETERMINISTIC) != 0, drop_n, E, N, p->avg_degree);
}

struct Ctx {
  const mtmc_mpn_model* m;
  const mtmc_mpn_call* c;
  Layout lo;
  char* ws;
  hipStream_t stream;
  char* wc = nullptr;                // the call's weight-plane cache (eval and training forwards), or nullptr (none given)
  CacheLayout cl;
  CallPlan plan;                     // which kernels this call runs (make_ctx)
  template <typename T> T* wc_at(size_t off) const { return reinterpret_cast<T*>(wc + off); }
  const SidePipe* pipe = nullptr;    // set by mtmc_mpn_forward: layer 0 runs in row panels (split of panel i+1 beside GEMM i)
  bool enc2_rides = false;           // set by mtmc_mpn_forward (few-row graphs): MTMC_PH_EDGE_ENC's work rides as passenger
                                     // workgroups in the last node-encoder layer's GEMM launch instead of a launch of its own
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
};

// the size guard of the call struct (ABI v5): a caller built against an older, shorter struct is refused, not read past
inline int check_call_size(const mtmc_mpn_call* c) {
  if (!c) return fail(MTMC_E_ARG, "call is NULL");
  if (c->struct_bytes != sizeof(mtmc_mpn_call))
    return fail(MTMC_E_ARG, "mtmc_mpn_call.struct_bytes is %u, this library's struct has %zu bytes (ABI v%d): rebuild the caller against include/mtmc_mpn.h",
                c->struct_bytes, sizeof(mtmc_mpn_call), MTMC_MPN_ABI_VERSION);
  return MTMC_OK;
}

inline int make_ctx(const mtmc_mpn_model* m, const mtmc_mpn_call* c, Ctx* ctx) {
  if (int rc = check_model(m)) return rc;
  if (int rc = check_call_size(c)) return rc;
  if (c->training && (c->node_lo != 0 || c->node_hi != c->n_nodes || c->n_edges_total != c->n_edges))
    return fail(MTMC_E_ARG, "training mode is single-shard only");
  if (c->training && (c->flags & MTMC_F_SEED_ON_DEVICE) && (c->seed == 0 || (c->seed & 7)))
    return fail(MTMC_E_ARG, "MTMC_F_SEED_ON_DEVICE: seed must hold the 8-byte aligned device address of a uint64 counter");
  if (c->n_nodes < 2) return fail(MTMC_E_ROWS, "BatchNorm over %lld node rows: Expected more than 1 value per channel", (long long)c->n_nodes);
  if (c->n_edges_total < 2) return fail(MTMC_E_ROWS, "BatchNorm over %lld edge rows: Expected more than 1 value per channel", (long long)c->n_edges_total);
  if (c->n_edges < 0 || c->n_edges > c->n_edges_total || c->n_edges >= (1ll << 31) || c->n_nodes >= (1ll << 31))
    return fail(MTMC_E_ARG, "edge/node counts out of range");
  if (c->node_lo < 0 || c->node_hi < c->node_lo || c->node_hi > c->n_nodes) return fail(MTMC_E_ARG, "bad node range");
  if (c->row_lo < 0 || c->row_hi < c->row_lo || c->row_hi > c->n_nodes) return fail(MTMC_E_ARG, "bad row range");
  if (c->training && (c->row_lo != 0 || (c->row_hi != 0 && c->row_hi != c->n_nodes)))
    return fail(MTMC_E_ARG, "training calls project every node row (row_lo = row_hi = 0)");
  if (!c->x || !c->edge_attr || !c->logits || !c->h_out || !c->workspace) return fail(MTMC_E_ARG, "NULL tensor pointer");
  if (c->n_edges > 0 && (!c->row || !c->col)) return fail(MTMC_E_ARG, "NULL edge_index pointer");
  if (c->idx_stride < 1) return fail(MTMC_E_ARG, "idx_stride must be >= 1");
  if (((uintptr_t)c->x & 15) || (c->x_row_stride & 3) || c->x_row_stride < m->enc_node[0].in_dim)
    return fail(MTMC_E_ARG, "x must be 16-byte aligned with a row stride that is a multiple of 4 and >= in_dim");
  if (((uintptr_t)c->edge_attr & 7) || ((uintptr_t)c->logits & 7) || ((uintptr_t)c->h_out & 15))
    return fail(MTMC_E_ARG, "edge_attr/logits must be 8-byte and h_out 16-byte aligned");
  if ((uintptr_t)c->workspace & 255) return fail(MTMC_E_WORKSPACE, "workspace must be 256-byte aligned");
  ctx->m = m; ctx->c = c;
  make_layout(m, c->n_nodes, c->n_edges, &ctx->lo, c->training != 0);
  if (c->workspace_bytes < ctx->lo.pub.total_bytes)
    return fail(MTMC_E_WORKSPACE, "workspace has %zu bytes, %zu needed", c->workspace_bytes, ctx->lo.pub.total_bytes);
  ctx->ws = static_cast<char*>(c->workspace);
  ctx->stream = static_cast<hipStream_t>(c->stream);
  make_cache_layout(m, &ctx->cl);
  if (c->weight_cache) {
    if ((uintptr_t)c->weight_cache & 255) return fail(MTMC_E_WORKSPACE, "weight_cache must be 256-byte aligned");
    if (c->weight_cache_bytes < ctx->cl.total)
      return fail(MTMC_E_WORKSPACE, "weight_cache has %zu bytes, %zu needed (mtmc_mpn_weight_cache_bytes)", c->weight_cache_bytes, ctx->cl.total);
    ctx->wc = static_cast<char*>(c->weight_cache);
  }
  make_plan(m, c, ctx->lo, ctx->cl, &ctx->plan);
  return MTMC_OK;
}

inline mtmc::Drop make_drop(const Ctx& x, float p) {
  mtmc::Drop d;
  d.on = (x.c->training && p > 0.f) ? 1 : 0;
  d.seed = x.c->seed;
  if (d.on && (x.c->flags & MTMC_F_SEED_ON_DEVICE)) {   // the seed word of this forward, on the tape (seed_tick_kernel)
    d.on = 2;
    d.seed = (unsigned long long)(uintptr_t)(x.ws + x.lo.seed_word);
  }
  const double t = (double)p * 65536.0;                 // 16-bit fields: four elements per 64-bit hash (common.h)
  d.thresh = t >= 65535.0 ? 65535u : (unsigned)t;
  d.inv_keep = p < 1.f ? 1.f / (1.f - p) : 0.f;
  return d;
}

inline mtmc::EdgeEncParams enc_params(const Ctx& x) {
  mtmc::EdgeEncParams e;
  const mtmc_layer& a = x.m->enc_edge[0];
  const mtmc_layer& b = x.m->enc_edge[1];
  e.w1 = a.weight; e.b1 = a.bias; e.g1 = a.gamma; e.bt1 = a.beta;
  e.w2 = b.weight; e.b2 = b.bias; e.g2 = b.gamma; e.bt2 = b.beta;
  e.stat_attr = x.at<double>(x.lo.pub.stat_attr_off);
  e.stat_enc2 = x.at<double>(x.lo.pub.stat_enc2_off);
  e.aff = x.at<float>(x.lo.enc_aff);
  e.fe = a.in_dim;
  e.drop = make_drop(x, x.m->dropout_enc);
  return e;
}

// Where round r aggregates: the last round of a sum/max model writes latent_node_feats straight into h_out.
inline float* agg_target(const Ctx& x, int r) {
  if (x.lo.training) return x.at<float>(x.lo.h_tr[r]);
  if (r == x.m->num_enc_steps - 1 && x.m->agg != MTMC_AGG_MEAN) return x.c->h_out;
  return x.at<float>(x.lo.pub.h_acc_off[r & 1]);
}
// the (unscaled) node state round r reads: h0 for the first round, else what round r-1 aggregated
// rows whose projections / node-update statistics this call computes (mtmc_mpn_call::row_lo / row_hi; 0,0 = all)
inline int64_t proj_lo(const mtmc_mpn_call* c) { return c->row_hi > 0 ? c->row_lo : 0; }
inline int64_t proj_hi(const mtmc_mpn_call* c) { return c->row_hi > 0 ? c->row_hi : c->n_nodes; }
inline float* round_h_src(const Ctx& x, int r) {
  if (r == 0) return x.at<float>(x.lo.pub.h0_off);
  return x.lo.training ? x.at<float>(x.lo.h_tr[r - 1]) : x.at<float>(x.lo.pub.h_acc_off[(r - 1) & 1]);
}
inline float* round_P(const Ctx& x, int r) { return x.at<float>(x.lo.training ? x.lo.P_tr[r] : x.lo.pub.P_off); }
inline float* round_Q(const Ctx& x, int r) { return x.at<float>(x.lo.training ? x.lo.Q_tr[r] : x.lo.Q); }
inline float* round_z(const Ctx& x, int r) { return x.at<float>(x.lo.training ? x.lo.z_tr[r] : x.lo.e_buf[r & 1]); }
inline float* round_e(const Ctx& x, int r) { return x.at<float>(x.lo.training ? x.lo.e_tr[r] : x.lo.e_buf[r & 1]); }

inline mtmc::RoundParams round_params(const Ctx& x, int r) {
  const mtmc_mpn_model* m = x.m;
  const int hn = node_in_width(m);
  mtmc::RoundParams p;
  p.row32 = x.at<int>(x.lo.row32); p.col32 = x.at<int>(x.lo.col32);
  p.attr = x.c->edge_attr;
  p.e_buf = round_z(x, r); p.e_out = round_e(x, r); p.e_prev = r > 0 ? round_e(x, r - 1) : nullptr;
  p.drop_e = make_drop(x, m->dropout_upd_edge); p.drop_n = make_drop(x, m->dropout_upd_node);
  p.drop_stream = mtmc::kDropRound + 2 * r;
  p.P = round_P(x, r); p.Q = round_Q(x, r);
  p.seg = x.at<double>(x.lo.pub.seg_off); p.fold_z2 = x.plan.fold_node_stat ? 1 : 0;
  p.ue_w = m->upd_edge.weight; p.ue_b = m->upd_edge.bias; p.ue_g = m->upd_edge.gamma; p.ue_bt = m->upd_edge.beta;
  p.ue_ld = m->upd_edge.in_dim; p.ue_eoff = 2 * hn;
  p.un_w = m->upd_node.weight; p.un_b = m->upd_node.bias; p.un_g = m->upd_node.gamma; p.un_bt = m->upd_node.beta;
  p.un_ld = m->upd_node.in_dim; p.un_eoff = hn;
  p.cls_w = m->cls.weight; p.cls_b = m->cls.bias; p.n_classes = m->cls.out_dim;
  p.stats = x.at<double>(x.lo.pub.stat_round_off) + (size_t)r * mtmc::kRoundBlock;
  // (few-edge graphs are latency-bound: there the extra statistics gather in two prologues costs more than the bytes save)
  p.lazy_e = x.plan.lazy_edges ? 1 : 0;
  p.prev_stats = r > 0 ? p.stats - mtmc::kRoundBlock : nullptr;
  p.h_acc = agg_target(x, r);
  const int step = r + 1, first_cls = first_cls_step(m);
  p.logits = step >= first_cls ? x.c->logits + (size_t)(step - first_cls) * x.c->n_edges * m->cls.out_dim : nullptr;
  p.n_edges = x.c->n_edges; p.e_total = (double)x.c->n_edges_total;
  p.first_round = r == 0; p.reattach_edges = m->reattach_edges; p.agg = m->agg;
  p.det = (x.c->flags & MTMC_F_DETERMINISTIC) ? 1 : 0; p.flags = x.at<int>(x.lo.pub.flags_off);
  p.deg = x.at<int>(x.lo.pub.deg_off); p.row_start = x.at<int>(x.lo.row_start); p.carry = x.at<float>(x.lo.carry);
  p.n_nodes = x.c->n_nodes;
  p.avg_degree = x.plan.avg_degree;
  p.pass_c = x.plan.pass_c;
  p.col_blocks = x.plan.col_blocks;
  p.col_sub = x.at<int>(x.lo.col_sub); p.cb_row_lo = proj_lo(x.c); p.cb_row_hi = proj_hi(x.c);
  p.enc = enc_params(x);
  return p;
}

// where layer l's weight planes / inverse row scales are: the cache when the call has one, else the workspace (made per call)
inline _Float16* w_planes(const Ctx& x, int l) {
  if (x.plan.w_cached[l]) return x.wc_at<_Float16>(x.cl.planes[l]);
  return x.at<_Float16>(x.lo.wh[l]);
}
inline float* w_inv(const Ctx& x, int l) {
  if (x.plan.w_cached[l]) return x.wc_at<float>(x.cl.inv[l]);
  return x.at<float>(x.lo.inv_w[l]);
}

// The |.|max words (u32[kAmaxRep] each) of x, of layer l's raw output Y_l and of W_l (Layout::amax, amax_w)
inline unsigned* amax_x(const Ctx& x) { return x.at<unsigned>(x.lo.amax); }
inline unsigned* amax_y(const Ctx& x, int l) { return amax_x(x) + (1 + MTMC_MAX_ENC_LAYERS + l) * mtmc::kAmaxRep; }
inline unsigned* amax_w(const Ctx& x, int l) { return x.at<unsigned>(x.lo.amax_w) + l * mtmc::kAmaxRep; }
inline unsigned* amax_in(const Ctx& x, int l) { return l == 0 ? amax_x(x) : amax_y(x, l - 1); }   // of layer l's input

}  // namespace mtmc_api
