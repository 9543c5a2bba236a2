// C-ABI layer (include/mtmc_mpn.h), the forward: the sizing and layout queries, the per-phase parameter blocks and launches,
// and the phase sequence of one MOTMPNet.forward (reference models/mpn.py:250-299).  Launch-only: nothing here allocates or
// synchronises, so a caller may capture a forward into a hipGraph.
#include "api_internal.h"

#include <mutex>

namespace mtmc_api {
// Side stream + events of the pipelined layer 0 (Ctx::pipe; pipe_for below)
struct SidePipe { hipStream_t stream = nullptr; hipEvent_t fork = nullptr; hipEvent_t ready[kMaxPanels] = {}; };
}  // namespace mtmc_api

using namespace mtmc_api;

namespace {

// The edge branch (index conversion, degree, edge-encoder moments) and the node-encoder GEMM chain are
// independent until the first round.  With MTMC_F_FORK the edge branch runs on a side stream (fork/join with
// events; legal under stream capture too).  Opt-in: measured on MI355X/ROCm 7.2 the two event hops cost more
// (~+20 us per forward on the 150k-edge S02 graph) than the ~17 us of overlap they buy.
// One side stream + event pair per device, created on first use.
struct Side { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; bool ok = false; };
Side* side_for_current_device() {
  static Side sides[64];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  Side& sd = sides[dev];
  if (!sd.ok) {
    if (hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&sd.join, hipEventDisableTiming) != hipSuccess) return nullptr;
    sd.ok = true;
  }
  return &sd;
}

// The pipelined layer 0's side stream and events: one set per (device, CALLER STREAM).  Round 4 had one per device: two host
// threads (or two streams) running many-row forwards on one device then recorded and waited on the SAME event objects, and a
// panel GEMM of one could start on the other's `ready[i]`.  A set whose creation fails half-way is destroyed
// again; at most kMaxPipes sets exist (beyond that: the serial layer 0).
constexpr int kMaxPipes = 64;
struct PipeSlot { int dev; hipStream_t caller; SidePipe pipe; };
void destroy_pipe(SidePipe& sp, int n_events) {
  for (int i = 0; i < n_events; ++i) (void)hipEventDestroy(sp.ready[i]);
  if (sp.fork) (void)hipEventDestroy(sp.fork);
  if (sp.stream) (void)hipStreamDestroy(sp.stream);
  sp = SidePipe();
}
SidePipe* pipe_for(hipStream_t caller) {
  static PipeSlot slots[kMaxPipes];
  static int n_slots = 0;
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  for (int i = 0; i < n_slots; ++i)
    if (slots[i].dev == dev && slots[i].caller == caller) return &slots[i].pipe;
  if (n_slots == kMaxPipes) return nullptr;
  SidePipe sp = SidePipe();
  if (hipStreamCreateWithFlags(&sp.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
  if (hipEventCreateWithFlags(&sp.fork, hipEventDisableTiming) != hipSuccess) { sp.fork = nullptr; destroy_pipe(sp, 0); return nullptr; }
  for (int i = 0; i < kMaxPanels; ++i)
    if (hipEventCreateWithFlags(&sp.ready[i], hipEventDisableTiming) != hipSuccess) { destroy_pipe(sp, i); return nullptr; }
  slots[n_slots] = {dev, caller, sp};
  return &slots[n_slots++].pipe;
}

// Diagnostics (bench.py): HIP events around every layer-0 GEMM launch of a many-row forward -- in the pipelined forward the
// layer is several panel launches beside the operand split on a side stream, and the figure a bench line reports must be
// that of the forward it sits beside.  Off by default; mtmc_dbg_panel_timing / mtmc_dbg_panel_times below.
struct PanelTiming { bool on = false, created = false; hipEvent_t ev[2 * kMaxPanels]; int n = 0; };
PanelTiming& panel_timing() { static PanelTiming t; return t; }

enum { kPhMemset = -1, kPhPrep = -2 };   // the two halves of MTMC_PH_BEGIN, for the forked forward

// the edge part of prep_kernel for this call
void fill_prep_edge(const Ctx& x, mtmc::PrepEdge* p) {
  const mtmc_mpn_call* c = x.c;
  p->row = c->row; p->col = c->col; p->idx_stride = c->idx_stride; p->attr = c->edge_attr; p->fe = x.m->enc_edge[0].in_dim;
  p->n_edges = c->n_edges; p->n_nodes = c->n_nodes;
  p->row32 = x.at<int>(x.lo.row32); p->col32 = x.at<int>(x.lo.col32); p->deg = x.at<int>(x.lo.pub.deg_off);
  p->flags = x.at<int>(x.lo.pub.flags_off); p->stat_attr = x.at<double>(x.lo.pub.stat_attr_off);
  p->row_start = x.at<int>(x.lo.row_start);
}

const int* scale_deg(const Ctx& x) {   // the degree mean aggregation divides by
  return x.at<int>((x.c->flags & MTMC_F_GLOBAL_DEG) ? x.lo.pub.deg_global_off : x.lo.pub.deg_off);
}

// The parts of node-encoder layer l's parameter block (kernels.h), each filled from the call in one place.
// Input: x for layer 0, else the previous layer's raw Y with its statistics, BatchNorm and Dropout
void fill_in(const Ctx& x, int l, mtmc::ActIn* q) {
  if (l == 0) {
    q->A = x.c->x; q->lda = x.c->x_row_stride;
  } else {
    const mtmc_layer& Pv = x.m->enc_node[l - 1];
    q->A = x.at<float>(x.lo.Y[l - 1]); q->lda = Pv.out_dim;
    q->stats_in = x.at<double>(x.lo.pub.stat_enc_layer_off[l - 1]); q->gamma_in = Pv.gamma; q->beta_in = Pv.beta;
  }
  q->count = (double)x.c->n_nodes;
  q->drop_in = make_drop(x, x.m->dropout_enc); q->drop_stream = mtmc::kDropEncNode + l - 1;
}
void fill_out(const Ctx& x, int l, mtmc::LayerOut* q) {
  const mtmc_layer& Lr = x.m->enc_node[l];
  q->bias = Lr.bias; q->Y = x.at<float>(x.lo.Y[l]); q->ldy = Lr.out_dim;
  q->stats_out = x.at<double>(x.lo.pub.stat_enc_layer_off[l]); q->amax_y = amax_y(x, l);
  q->M = x.plan.rows; q->K = Lr.in_dim; q->Nout = Lr.out_dim;
}
void fill_w(const Ctx& x, int l, mtmc::PlanesW* q) { q->Wh = w_planes(x, l); q->inv_w = w_inv(x, l); }
void fill_x(const Ctx& x, mtmc::PlanesA* q) { q->Ah = x.at<_Float16>(x.lo.xh); q->inv_a = x.at<float>(x.lo.inv_a); }
// MTMC_PH_EDGE_ENC's work as passenger workgroups of the last encoder layer's launch
void ride_enc2(const Ctx& x, mtmc::Enc2Ride* q) {
  const int64_t blocks = (x.c->n_edges + 255) / 256;
  q->pass_blocks = (int)(blocks > 2048 ? 2048 : blocks);
  q->pass_enc = enc_params(x); q->pass_attr = x.c->edge_attr; q->pass_edges = x.c->n_edges;
  q->pass_e_total = (double)x.c->n_edges_total; q->pass_stat = x.at<double>(x.lo.pub.stat_enc2_off);
}

// The node-encoder layer launches of MTMC_PH_NODE_ENC, one per form of CallPlan::enc_kernel.  A launcher's refusal
// (kernels.h: MTMC_E_ARG or MTMC_E_HIP) is the phase's code.
// Few-row graphs (gemm_few.hip): one launch per layer, never split along K.
int launch_enc_few(const Ctx& x, int l) {
  int rc;
  if (l == 0) {
    mtmc::FewL0Params q;
    fill_x(x, &q); fill_w(x, 0, &q); fill_out(x, 0, &q);
    rc = mtmc::launch_few_l0(q, x.stream);
  } else {
    mtmc::FewWaveParams q;
    fill_in(x, l, &q); fill_w(x, l, &q); fill_out(x, l, &q);
    if (x.enc2_rides && l == x.m->n_enc_layers - 1) ride_enc2(x, &q);
    rc = mtmc::launch_few_wave(q, x.stream);
  }
  if (rc) return fail(rc, "encoder layer %d: few-row kernel refused the shape or the launch", l);
  return MTMC_OK;
}

// Many-row graphs, layer 0 on the operand planes made in MTMC_PH_BEGIN -- or, in the pipelined forward (x.pipe), in row panels.
int launch_enc_presplit0(const Ctx& x) {
  const mtmc_mpn_call* c = x.c;
  const mtmc_layer& Lr = x.m->enc_node[0];
  const int64_t rows = x.plan.rows;
  hipStream_t s = x.stream;
  mtmc::SplitGemmParams q;
  fill_x(x, &q); fill_w(x, 0, &q); fill_out(x, 0, &q);
  PanelTiming& pt = panel_timing();
  if (x.pipe) {
    // Row panels: the side stream splits panel after panel (HBM-bound), the main stream multiplies panel i as soon as
    // its planes are there (matrix-bound): the split pass leaves the critical path except for the first panel.
    // Panel = whole rounds of workgroups of the tile height the whole matrix would get, so no round is paid twice.
    const int np = x.plan.l0_panels;
    const int64_t* cuts = x.plan.l0_cuts;
    q.bm = x.plan.l0_bm;
    q.M_rows = rows;
    if (hipEventRecord(x.pipe->fork, s) != hipSuccess || hipStreamWaitEvent(x.pipe->stream, x.pipe->fork, 0) != hipSuccess)
      return fail(MTMC_E_HIP, "encoder layer 0: fork onto the side stream failed");
    // from here on the side stream is forked off `s` (inside a capture: part of it): every way out joins it again
    auto join_and = [&](int code, const char* what) {
      if (hipEventRecord(x.pipe->ready[0], x.pipe->stream) == hipSuccess) (void)hipStreamWaitEvent(s, x.pipe->ready[0], 0);
      return fail(code, "%s", what);
    };
    for (int i = 0; i < np; ++i) {
      mtmc::launch_split_rows_range(c->x, c->x_row_stride, rows, Lr.in_dim, x.at<void>(x.lo.xh), x.at<float>(x.lo.inv_a),
                                    cuts[i], cuts[i + 1], x.pipe->stream);
      if (hipEventRecord(x.pipe->ready[i], x.pipe->stream) != hipSuccess) return join_and(MTMC_E_HIP, "hipEventRecord failed");
    }
    if (pt.on) pt.n = 0;
    for (int i = 0; i < np; ++i) {               // (the wait on the last panel's event also joins the side stream)
      if (hipStreamWaitEvent(s, x.pipe->ready[i], 0) != hipSuccess) return join_and(MTMC_E_HIP, "hipStreamWaitEvent failed");
      q.m_lo = cuts[i]; q.M = cuts[i + 1];
      if (pt.on) (void)hipEventRecord(pt.ev[2 * i], s);
      const int rc = mtmc::launch_gemm_presplit(q, s);
      if (pt.on) { (void)hipEventRecord(pt.ev[2 * i + 1], s); pt.n = i + 1; }
      if (rc) return join_and(rc, "encoder layer 0: pre-split GEMM refused a panel");
    }
    return MTMC_OK;
  }
  if (pt.on) { pt.n = 0; (void)hipEventRecord(pt.ev[0], s); }
  const int rc = mtmc::launch_gemm_presplit(q, s);
  if (pt.on) { (void)hipEventRecord(pt.ev[1], s); pt.n = 1; }
  if (rc) return fail(rc, "encoder layer 0: pre-split GEMM refused the shape or the launch");
  return MTMC_OK;
}

// Many-row graphs, layers >= 1 on the role-split kernel (gemm_staged.hip).
int launch_enc_staged(const Ctx& x, int l) {
  mtmc::StagedGemmParams q;
  fill_in(x, l, &q); fill_w(x, l, &q); fill_out(x, l, &q);
  q.amax_a = amax_in(x, l);
  if (int rc = mtmc::launch_gemm_staged(q, x.stream))
    return fail(rc, "encoder layer %d: role-split GEMM refused the shape or the launch", l);
  return MTMC_OK;
}

// The in-loop operand split (gemm_bn.hip; MTMC_PH_NODE_COMBINE adds up the slab's K slices), or the row-streaming kernel
// (gemm_rows.hip) of the narrow last layers of many-row graphs.
int launch_enc_gemm(const Ctx& x, int l, int phase) {
  mtmc::GemmParams g;
  fill_in(x, l, &g); fill_out(x, l, &g);
  g.W = x.m->enc_node[l].weight; g.amax_a = amax_in(x, l); g.amax_w = amax_w(x, l);
  if (x.enc2_rides && phase == MTMC_PH_NODE_ENC && l == x.m->n_enc_layers - 1) ride_enc2(x, &g);
  if (x.plan.enc_kernel[l] == MTMC_GEMM_ROWS_16) {
    if (int rc = mtmc::launch_gemm_rows(g, x.stream)) return fail(rc, "encoder layer %d: row-streaming GEMM refused the shape", l);
    return MTMC_OK;
  }
  if (x.plan.enc_split_k[l] > 1) g.slab = x.at<float>(x.lo.slab);
  if (int rc = mtmc::launch_gemm_bn(g, x.stream, phase == MTMC_PH_NODE_ENC ? 1 : 2))
    return fail(rc, "encoder layer %d: unsupported GEMM shape", l);
  return MTMC_OK;
}

int run_phase(const Ctx& x, int phase, int arg, bool fused_h0 = false) {
  const mtmc_mpn_model* m = x.m;
  const mtmc_mpn_call* c = x.c;
  const int L = m->num_enc_steps;
  hipStream_t s = x.stream;
  switch (phase) {
    case MTMC_PH_BEGIN:
    case kPhMemset:
    case kPhPrep: {
      // What depends on the WEIGHTS alone -- the fp16 planes + row scales of the layers that run on pre-split weights -- lives in
      // the call's weight-plane cache when it has one and is VERIFIED here on every call, chunk by chunk, by passenger
      // workgroups of prep_kernel (split_body.h); without a cache it is made per call in the workspace.
      if (phase != kPhPrep && hipMemsetAsync(x.ws, 0, x.lo.pub.zero_bytes, s) != hipSuccess)
        return fail(MTMC_E_HIP, "hipMemsetAsync failed");
      if (phase != kPhPrep && c->training && (c->flags & MTMC_F_SEED_ON_DEVICE))      // seed word <- counter++ (one thread)
        mtmc::launch_seed_tick(reinterpret_cast<unsigned long long*>((uintptr_t)c->seed), x.at<unsigned long long>(x.lo.seed_word), s);
      if (phase != kPhMemset) {
        const CallPlan& pl = x.plan;
        const int64_t rows = pl.rows;
        mtmc::PrepParams p;
        fill_prep_edge(x, &p);
        // passenger jobs: operand |.|max values / operand splits of the node encoder (this rank's rows of x; the weights)
        p.n_jobs = 0;
        // (training forwards: the jobs also publish the tensors' |.|max -- the backward's GEMMs scale by |x|max and |W_l|max)
        if (rows > 0) {
          if (pl.enc_kernel[0] == MTMC_GEMM_FEW_L0)     // the planes of x, 8 rows per passenger workgroup (no |x|max: one scale per row)
            p.jobs[p.n_jobs++] = {c->x, rows, m->enc_node[0].in_dim, c->x_row_stride, c->training ? amax_x(x) : nullptr, 0, 0, mtmc::kJobSplit,
                                  x.at<_Float16>(x.lo.xh), x.at<float>(x.lo.inv_a), nullptr};
          else if (pl.enc_kernel[0] != MTMC_GEMM_PRESPLIT_256)
            p.jobs[p.n_jobs++] = {c->x, rows, m->enc_node[0].in_dim, c->x_row_stride, amax_x(x), 0, 0, mtmc::kJobAmax, nullptr, nullptr, nullptr};
          for (int l = 0; l < m->n_enc_layers; ++l) {
            const mtmc_layer& Ll = m->enc_node[l];
            if (pl.w_cached[l])         // layer l's planes in the cache: verify every 8-row chunk, split the ones that changed
              p.jobs[p.n_jobs++] = {Ll.weight, Ll.out_dim, Ll.in_dim, Ll.in_dim, c->training ? amax_w(x, l) : nullptr, 0, 0,
                                    mtmc::kJobSplit, x.wc_at<_Float16>(x.cl.planes[l]), x.wc_at<float>(x.cl.inv[l]),
                                    x.wc_at<unsigned long long>(x.cl.fp[l])};
            else if (in_loop_kernel(pl.enc_kernel[l]))   // |W_l|max (row-streaming: in the kernel; planes without a cache: below)
              p.jobs[p.n_jobs++] = {Ll.weight, Ll.out_dim, Ll.in_dim, Ll.in_dim, amax_w(x, l), 0, 0, mtmc::kJobAmax,
                                    nullptr, nullptr, nullptr};
          }
        }
        mtmc::launch_prep(p, s);
        if (pl.col_blocks > 0) {        // sub-run boundaries of the column-blocked pass A, once per forward
          const mtmc::RoundParams rp = round_params(x, 0);
          mtmc::launch_colblock_index(rp, x.at<int>(x.lo.col_sub), rp.col_blocks, rp.cb_row_lo, rp.cb_row_hi, s);
        }
        // instead of the |.|max of x and W0: their fp16 planes and row scales
        // (pipelined layer 0: the x planes are made panel by panel in MTMC_PH_NODE_ENC 0)
        if (pl.enc_kernel[0] == MTMC_GEMM_PRESPLIT_256 && !x.pipe)
          mtmc::launch_split_rows(c->x, c->x_row_stride, rows, m->enc_node[0].in_dim, x.at<void>(x.lo.xh),
                                  x.at<float>(x.lo.inv_a), s);
        for (int l = 0; l < m->n_enc_layers; ++l) {     // the weight planes of the layers whose kernels want them, unless cached
          const mtmc_layer& Ll = m->enc_node[l];
          if ((pl.enc_kernel[l] == MTMC_GEMM_PRESPLIT_256 || pl.enc_kernel[l] == MTMC_GEMM_STAGED_128) && !pl.w_cached[l])
            mtmc::launch_split_rows(Ll.weight, Ll.in_dim, Ll.out_dim, Ll.in_dim, w_planes(x, l), w_inv(x, l), s);
        }
      }
      break;
    }
    case MTMC_PH_EDGE_ENC:
      if (c->n_edges > 0)
        mtmc::launch_enc2(enc_params(x), c->edge_attr, c->n_edges, (double)c->n_edges_total, x.at<double>(x.lo.pub.stat_enc2_off), s);
      break;
    case MTMC_PH_NODE_ENC:
    case MTMC_PH_NODE_COMBINE: {
      if (arg < 0 || arg >= m->n_enc_layers) return fail(MTMC_E_ARG, "encoder layer %d out of range", arg);
      if (x.plan.rows == 0) break;
      const int k = x.plan.enc_kernel[arg];
      if (phase == MTMC_PH_NODE_COMBINE && !in_loop_kernel(k)) break;   // only the in-loop kernel splits along K
      int rc;
      if (k == MTMC_GEMM_FEW_L0 || k == MTMC_GEMM_FEW_WAVE) rc = launch_enc_few(x, arg);
      else if (k == MTMC_GEMM_PRESPLIT_256) rc = launch_enc_presplit0(x);
      else if (k == MTMC_GEMM_STAGED_128) rc = launch_enc_staged(x, arg);
      else rc = launch_enc_gemm(x, arg, phase);
      if (rc) return rc;
      break;
    }
    case MTMC_PH_NODE_H0: {
      const int last = m->n_enc_layers - 1;
      const int64_t rows = c->node_hi - c->node_lo;
      if (rows > 0)
        mtmc::launch_bn_relu_rows({x.at<float>(x.lo.Y[last]), MTMC_NODE_DIM, rows, MTMC_NODE_DIM,
                                   x.at<double>(x.lo.pub.stat_enc_layer_off[last]), m->enc_node[last].gamma, m->enc_node[last].beta,
                                   (double)c->n_nodes, x.at<float>(x.lo.pub.h0_off) + (size_t)c->node_lo * MTMC_NODE_DIM,
                                   make_drop(x, m->dropout_enc), mtmc::kDropEncNode + last, c->node_lo}, s);
      break;
    }
    case MTMC_PH_ROUND_PROJ: {
      if (arg < 0 || arg >= L) return fail(MTMC_E_ARG, "round %d out of range", arg);
      mtmc::NodeProjParams p;
      const int last = m->n_enc_layers - 1;
      p.y_last = (arg == 0 && fused_h0) ? x.at<float>(x.lo.Y[last]) : nullptr;
      p.y_stats = x.at<double>(x.lo.pub.stat_enc_layer_off[last]); p.y_gamma = m->enc_node[last].gamma;
      p.y_beta = m->enc_node[last].beta; p.y_count = (double)c->n_nodes; p.h0_out = x.at<float>(x.lo.pub.h0_off);
      p.finalize_enc = arg == 0; p.enc = enc_params(x); p.e_total = (double)c->n_edges_total;
      p.h_src = round_h_src(x, arg);
      p.drop = make_drop(x, m->dropout_enc); p.drop_stream = mtmc::kDropEncNode + last;
      p.h0 = m->reattach_nodes ? x.at<float>(x.lo.pub.h0_off) : nullptr;
      p.deg = (m->agg == MTMC_AGG_MEAN && arg > 0) ? scale_deg(x) : nullptr;
      p.ue_w = m->upd_edge.weight; p.ue_ld = m->upd_edge.in_dim;
      p.un_w = m->upd_node.weight; p.un_ld = m->upd_node.in_dim;
      p.hn = node_in_width(m);
      p.P = round_P(x, arg); p.Q = round_Q(x, arg);
      p.zero_buf = agg_target(x, arg);
      p.n_nodes = c->n_nodes;
      p.node_begin = proj_lo(c); p.node_end = proj_hi(c);
      p.edge_deg = x.at<int>(x.lo.pub.deg_off); p.un_b = m->upd_node.bias;
      p.z2_stats = x.plan.fold_node_stat
                       ? x.at<double>(x.lo.pub.stat_round_off) + (size_t)arg * mtmc::kRoundBlock + mtmc::kRoundZ2Off : nullptr;
      mtmc::launch_node_proj(p, s);
      break;
    }
    case MTMC_PH_ROUND_A:
    case MTMC_PH_ROUND_B:
    case MTMC_PH_ROUND_C: {
      if (arg < 0 || arg >= L) return fail(MTMC_E_ARG, "round %d out of range", arg);
      if (c->n_edges == 0) break;
      const mtmc::RoundParams p = round_params(x, arg);
      if (phase == MTMC_PH_ROUND_A) mtmc::launch_pass_a(p, s);
      else if (phase == MTMC_PH_ROUND_B) mtmc::launch_pass_b(p, s);
      else mtmc::launch_pass_c(p, s);
      break;
    }
    case MTMC_PH_ROUND_STAT: {     // few-edge lists: nothing (the statistics came out of MTMC_PH_ROUND_PROJ + MTMC_PH_ROUND_B)
      if (arg < 0 || arg >= L) return fail(MTMC_E_ARG, "round %d out of range", arg);
      if (x.plan.fold_node_stat) break;
      mtmc::NodeStatParams p;
      p.Q = round_Q(x, arg); p.deg = x.at<int>(x.lo.pub.deg_off); p.seg = x.at<double>(x.lo.pub.seg_off);
      p.un_w = m->upd_node.weight; p.un_b = m->upd_node.bias; p.un_ld = m->upd_node.in_dim;
      p.un_eoff = node_in_width(m);
      p.stats = x.at<double>(x.lo.pub.stat_round_off) + (size_t)arg * mtmc::kRoundBlock;
      p.n_nodes = c->n_nodes;
      p.node_begin = proj_lo(c); p.node_end = proj_hi(c);
      mtmc::launch_node_stat(p, s);
      break;
    }
    case MTMC_PH_END: {
      const float* src = round_h_src(x, L);
      if (L == 0 || m->agg == MTMC_AGG_MEAN || x.lo.training)   // otherwise the last round aggregated into h_out
        mtmc::launch_h_final(src, scale_deg(x), (m->agg == MTMC_AGG_MEAN && L > 0) ? 1 : 0, c->n_nodes, c->h_out, s);
      if (L == 0 && c->n_edges > 0)
        mtmc::launch_classify_e0(enc_params(x), c->edge_attr, c->n_edges, (double)c->n_edges_total, m->cls.weight,
                                 m->cls.bias, m->cls.out_dim, c->logits, s);
      break;
    }
    default:
      return fail(MTMC_E_ARG, "unknown phase %d", phase);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MTMC_E_HIP, "kernel launch failed in phase %d: %s", phase, hipGetErrorString(e));
  return MTMC_OK;
}

}  // namespace

extern "C" {

int32_t mtmc_mpn_abi_version(void) { return MTMC_MPN_ABI_VERSION; }
const char* mtmc_mpn_last_error(void) { return g_err; }

size_t mtmc_mpn_train_workspace_bytes(const mtmc_mpn_model* model, int64_t n_nodes, int64_t n_edges) {
  if (check_model(model) != MTMC_OK || n_nodes < 0 || n_edges < 0) return 0;
  Layout lo;
  make_layout(model, n_nodes, n_edges, &lo, true);
  return lo.pub.total_bytes;
}

size_t mtmc_mpn_workspace_bytes(const mtmc_mpn_model* model, int64_t n_nodes, int64_t n_edges) {
  if (check_model(model) != MTMC_OK || n_nodes < 0 || n_edges < 0) return 0;
  Layout lo;
  make_layout(model, n_nodes, n_edges, &lo);
  return lo.pub.total_bytes;
}

size_t mtmc_mpn_weight_cache_bytes(const mtmc_mpn_model* model) {
  if (check_model(model) != MTMC_OK) return 0;
  CacheLayout cl;
  make_cache_layout(model, &cl);
  return cl.total > 0 ? cl.total : 256;
}

int32_t mtmc_mpn_workspace_layout(const mtmc_mpn_model* model, int64_t n_nodes, int64_t n_edges, mtmc_ws_layout* out) {
  if (int rc = check_model(model)) return rc;
  if (!out || n_nodes < 0 || n_edges < 0) return fail(MTMC_E_ARG, "bad layout arguments");
  Layout lo;
  make_layout(model, n_nodes, n_edges, &lo);
  *out = lo.pub;
  return MTMC_OK;
}

// Diagnostics: time every layer-0 GEMM launch (row panels) of the many-row forwards that follow with HIP events on the call's
// stream; mtmc_dbg_panel_times synchronises the LAST forward's events and returns their number (elapsed ms in `ms`).
int32_t mtmc_dbg_panel_timing(int32_t enable) {
  PanelTiming& pt = panel_timing();
  if (enable && !pt.created) {
    for (int i = 0; i < 2 * kMaxPanels; ++i)
      if (hipEventCreate(&pt.ev[i]) != hipSuccess) return fail(MTMC_E_HIP, "hipEventCreate failed");
    pt.created = true;
  }
  pt.on = enable != 0;
  pt.n = 0;
  return MTMC_OK;
}
int32_t mtmc_dbg_panel_times(float* ms, int32_t max) {
  PanelTiming& pt = panel_timing();
  if (!ms || !pt.created) return 0;
  int n = 0;
  for (; n < pt.n && n < max; ++n) {
    if (hipEventSynchronize(pt.ev[2 * n + 1]) != hipSuccess) break;
    if (hipEventElapsedTime(&ms[n], pt.ev[2 * n], pt.ev[2 * n + 1]) != hipSuccess) break;
  }
  return n;
}

int32_t mtmc_mpn_run_phase(const mtmc_mpn_model* model, const mtmc_mpn_call* call, int32_t phase, int32_t arg) {
  Ctx x;
  if (int rc = make_ctx(model, call, &x)) return rc;
  return run_phase(x, phase, arg);
}

int32_t mtmc_mpn_run_phases(const mtmc_mpn_model* model, const mtmc_mpn_call* call, const int32_t* phase_args, int32_t n) {
  Ctx x;
  if (int rc = make_ctx(model, call, &x)) return rc;
  if (n < 0 || (n > 0 && !phase_args)) return fail(MTMC_E_ARG, "mtmc_mpn_run_phases: bad phase list");
  for (int i = 0; i < n; ++i)
    if (int rc = run_phase(x, phase_args[2 * i], phase_args[2 * i + 1])) return rc;
  return MTMC_OK;
}

int32_t mtmc_mpn_plan_call(const mtmc_mpn_model* model, const mtmc_mpn_call* call, mtmc_mpn_plan* out) {
  if (int rc = check_model(model)) return rc;
  if (!out) return fail(MTMC_E_ARG, "mtmc_mpn_plan_call: NULL result");
  if (int rc = check_call_size(call)) return rc;
  const mtmc_mpn_call* c = call;
  if (c->n_nodes < 0 || c->n_edges < 0 || c->n_edges > c->n_edges_total || c->node_lo < 0 || c->node_hi < c->node_lo ||
      c->node_hi > c->n_nodes || c->row_lo < 0 || c->row_hi < c->row_lo || c->row_hi > c->n_nodes)
    return fail(MTMC_E_ARG, "mtmc_mpn_plan_call: sizes / ranges out of order");
  Layout lo;                   // (host-only: offsets and flags, nothing is allocated)
  CacheLayout cl;
  CallPlan p;                  // what mtmc_mpn_forward would run (make_ctx builds the same plan)
  make_layout(model, c->n_nodes, c->n_edges, &lo, c->training != 0);
  make_cache_layout(model, &cl);
  make_plan(model, c, lo, cl, &p);
  *out = mtmc_mpn_plan();
  for (int l = 0; l < model->n_enc_layers; ++l) { out->enc_kernel[l] = p.enc_kernel[l]; out->enc_split_k[l] = p.enc_split_k[l]; }
  out->edges_per_thread = p.edges_per_thread;
  out->lazy_edges = p.lazy_edges ? 1 : 0;
  out->avg_degree = p.avg_degree;
  out->pass_a_col_blocks = p.col_blocks;
  out->pass_c = p.pass_c_pub();
  out->node_stat_folded = p.fold_node_stat ? 1 : 0;
  out->layer0_panels = p.l0_panels;
  out->enc2_passenger = (p.enc2_may_ride && !(c->flags & MTMC_F_FORK)) ? 1 : 0;     // what mtmc_mpn_forward makes of it
  return MTMC_OK;
}

int32_t mtmc_mpn_forward(const mtmc_mpn_model* model, const mtmc_mpn_call* call) {
  Ctx x;
  if (int rc = make_ctx(model, call, &x)) return rc;
  int rc;
  // many-row graphs: layer 0 in row panels, the operand split one panel ahead on a side stream (MTMC_L0_PIPELINE=0: off)
  if (x.plan.l0_panels >= 2) x.pipe = pipe_for(x.stream);
  Side* sd = (call->flags & MTMC_F_FORK) ? side_for_current_device() : nullptr;
  if (sd) {
    if ((rc = run_phase(x, MTMC_PH_BEGIN, 0))) return rc;      // prep also gathers the node encoder's operand scales
    if (hipEventRecord(sd->fork, x.stream) != hipSuccess || hipStreamWaitEvent(sd->stream, sd->fork, 0) != hipSuccess)
      return fail(MTMC_E_HIP, "fork onto the side stream failed");
    Ctx xs = x;
    xs.stream = sd->stream;
    if ((rc = run_phase(xs, MTMC_PH_EDGE_ENC, 0))) return rc;
    if (hipEventRecord(sd->join, sd->stream) != hipSuccess) return fail(MTMC_E_HIP, "hipEventRecord failed");
  } else {
    // (round 5 tried the edge part of prep_kernel as passenger of encoder layer 0, with the statistics head cleared by the operand
    //  jobs' launch instead of a memset: layer 0 took 6 us longer, the jobs alone 8.0 us against prep_kernel's 8.8 -- DESIGN.md A.5)
    if ((rc = run_phase(x, MTMC_PH_BEGIN, 0))) return rc;
    x.enc2_rides = x.plan.enc2_may_ride;          // few-row graphs: enc2 as passenger of the last encoder layer's launch
    if (!x.enc2_rides && (rc = run_phase(x, MTMC_PH_EDGE_ENC, 0))) return rc;
  }
  for (int l = 0; l < model->n_enc_layers; ++l) {
    if ((rc = run_phase(x, MTMC_PH_NODE_ENC, l))) return rc;
    if ((rc = run_phase(x, MTMC_PH_NODE_COMBINE, l))) return rc;
  }
  if (sd && hipStreamWaitEvent(x.stream, sd->join, 0) != hipSuccess) return fail(MTMC_E_HIP, "join failed");
  // single shard: h0 = relu(bn(Y_last)) is produced inside the first round's projection kernel
  const bool fused_h0 = model->num_enc_steps > 0 && call->node_lo == 0 && call->node_hi == call->n_nodes;
  if (!fused_h0 && (rc = run_phase(x, MTMC_PH_NODE_H0, 0))) return rc;
  for (int r = 0; r < model->num_enc_steps; ++r) {
    if ((rc = run_phase(x, MTMC_PH_ROUND_PROJ, r, fused_h0))) return rc;
    if ((rc = run_phase(x, MTMC_PH_ROUND_A, r))) return rc;
    if ((rc = run_phase(x, MTMC_PH_ROUND_B, r))) return rc;
    if ((rc = run_phase(x, MTMC_PH_ROUND_STAT, r))) return rc;
    if ((rc = run_phase(x, MTMC_PH_ROUND_C, r))) return rc;
  }
  return run_phase(x, MTMC_PH_END, 0);
}

}  // extern "C"
