// C-ABI entry point of the backward pass (include/mtmc_mpn.h: mtmc_mpn_backward).  Launch-only, like the forward.
// Order: rounds L-1..0 (node-update MLP, edge-update MLP + classifier, node projections), then the edge encoder,
// then the node encoder (BatchNorm backward + two fp32-MFMA GEMMs per layer on transposed operands).
#include "api_internal.h"

using namespace mtmc_api;

namespace {

#define HIP_OK(call)                                                                                   \
  do {                                                                                                 \
    if ((call) != hipSuccess) return fail(MTMC_E_HIP, "%s failed in mtmc_mpn_backward", #call);        \
  } while (0)

// the gradient tensors are written: `grads` reuses mtmc_mpn_model, whose parameter pointers are const
float* wr(const float* p) { return const_cast<float*>(p); }
mtmc::LayerGrad layer_grad(const mtmc_layer& g) { return {wr(g.weight), wr(g.bias), wr(g.gamma), wr(g.beta)}; }

// where every layer's gradients go, under the names the layers have in mtmc_mpn_model: for_each_layer walks either
struct Grads { int n_enc_layers; mtmc::LayerGrad enc_node[MTMC_MAX_ENC_LAYERS], enc_edge[2], upd_edge, upd_node, cls; };

// every layer in struct order and whether it has a BatchNorm: the order of the pieces of the flat gradient buffer.
// Two structs side by side (the model and the caller's `grads`, or a Grads) walk by the FIRST one's n_enc_layers.
template <typename A, typename B, typename F>
void for_each_layer(A& a, B& b, F f) {
  for (int l = 0; l < a.n_enc_layers; ++l) f(a.enc_node[l], b.enc_node[l], true);
  f(a.enc_edge[0], b.enc_edge[0], true); f(a.enc_edge[1], b.enc_edge[1], true);
  f(a.upd_edge, b.upd_edge, true); f(a.upd_node, b.upd_node, true);
  f(a.cls, b.cls, false);
}
template <typename Model, typename F>
void for_each_layer(Model& m, F f) {
  for_each_layer(m, m, [&](auto& l, auto&, bool bn) { f(l, bn); });
}

int check_grads(const mtmc_mpn_model* m, const mtmc_mpn_model* g) {
  if (!g) return fail(MTMC_E_ARG, "grads is NULL");
  if (g->struct_bytes != sizeof(mtmc_mpn_model)) return fail(MTMC_E_ARG, "grads.struct_bytes is %u, expected %zu", g->struct_bytes, sizeof(mtmc_mpn_model));
  bool ok = true;
  for_each_layer(*m, *g, [&](const mtmc_layer&, const mtmc_layer& l, bool bn) {
    ok = ok && l.weight && l.bias && (!bn || (l.gamma && l.beta));
  });
  return ok ? MTMC_OK : fail(MTMC_E_ARG, "grads: NULL gradient buffer");
}

// One backward: what every stage below works on.
struct Bwd {
  Ctx x;
  Grads gr;                                            // the caller's `grads`, resolved once
  const float* const* d_logits_steps; const float* d_h;
  void* grads_flat; size_t grads_flat_bytes;
  float* d_x; float* d_edge_attr;
  int cur = 0, cur_e = 0;                              // ping-pong: g_h[cur] / g_e[cur_e] hold the gradient the next round consumes
  double* bst;                                         // backward statistics blocks: per round node, edge; then the edge encoder
  float* tX; float* tWl[MTMC_MAX_ENC_LAYERS] = {};     // x^T [in_0][npad], W_l^T [in_l][out_l] (null: not needed)
  int64_t npad;                                        // the node rows rounded up to 32
  float* gA; float* gB;                                // node encoder: this layer's dA, the next one's

  float* g_e(int i) const { return x.at<float>(x.lo.g_e[i]); }
  float* g_h(int i) const { return x.at<float>(x.lo.g_h[i]); }
  float* g_e0() const { return x.at<float>(x.lo.g_e0); }
  float* g_h0() const { return x.at<float>(x.lo.g_h0); }
  double* bst_block(int i) const { return bst + (size_t)i * mtmc::kStatRep * mtmc::kBwdStride; }
};

// Gradient buffers are accumulated into with atomics: clear them first (the caller only provides storage).  x^T and every
// W_l^T the node encoder's backward multiplies by depend on nothing the backward computes: they are made here as well -- by
// the backward's FIRST launch, beside the clearing, when the caller carved all gradients out of one buffer (grads_flat).
int bwd_clear_and_transpose(Bwd& b) {
  const Ctx& x = b.x;
  const mtmc_mpn_model* m = b.x.m;
  const Layout& lo = x.lo;
  hipStream_t s = x.stream;
  mtmc::TransposeJobs tj;
  mtmc::transpose_jobs_add(tj, x.c->x, x.c->n_nodes, m->enc_node[0].in_dim, x.c->x_row_stride, b.tX, b.npad);
  float* w = x.at<float>(lo.tW);
  for (int l = 0; l < m->n_enc_layers; ++l) {
    const mtmc_layer& Lr = m->enc_node[l];
    if (l > 0 || b.d_x) { b.tWl[l] = w; mtmc::transpose_jobs_add(tj, Lr.weight, Lr.out_dim, Lr.in_dim, Lr.in_dim, w, Lr.out_dim); }
    w += (size_t)Lr.in_dim * Lr.out_dim;
  }
  if (b.grads_flat) {
    // one launch for the flat buffer's accumulated pieces (everything but the encoder's weight gradients, which must lie in it
    // in layer order, as mtmc_mpn_grad_layout lays them out) and the workspace's range; anything else: plain memsets
    mtmc::ZeroRanges z;
    auto range = [&](char* from, char* to) { z.r[z.n].p = reinterpret_cast<uint4*>(from); z.r[z.n].n16 = (size_t)(to - from) / 16; ++z.n; };
    char* at = static_cast<char*>(b.grads_flat);
    char* const end = at + b.grads_flat_bytes;
    bool ok = ((uintptr_t)at & 15) == 0 && (b.grads_flat_bytes & 15) == 0;
    for (int l = 0; ok && l < m->n_enc_layers; ++l) {
      char* w = reinterpret_cast<char*>(b.gr.enc_node[l].w);
      const size_t wb = (size_t)m->enc_node[l].in_dim * m->enc_node[l].out_dim * sizeof(float);
      ok = w >= at && w + wb <= end && ((uintptr_t)w & 15) == 0 && (wb & 15) == 0;
      if (ok && w > at) range(at, w);
      at = w + wb;
    }
    if (ok) {
      if (end > at) range(at, end);
      ok = ((uintptr_t)(x.ws + lo.bwd_zero) & 15) == 0 && ((lo.bwd_zero_end - lo.bwd_zero) & 15) == 0;
    }
    if (ok) {
      range(x.ws + lo.bwd_zero, x.ws + lo.bwd_zero_end);
      mtmc::launch_bwd_begin(z, tj, s);
      return MTMC_OK;
    }
    HIP_OK(hipMemsetAsync(b.grads_flat, 0, b.grads_flat_bytes, s));
  } else {
    // one memset per tensor; the node encoder's weight gradients are plain GEMM outputs and need none
    bool ok = true;
    int i = 0;
    auto zero = [&](float* p, size_t n) { ok = ok && hipMemsetAsync(p, 0, n * sizeof(float), s) == hipSuccess; };
    for_each_layer(*m, b.gr, [&](const mtmc_layer& ml, const mtmc::LayerGrad& g, bool bn) {
      const size_t o = ml.out_dim;
      if (i++ >= m->n_enc_layers) zero(g.w, o * ml.in_dim);
      zero(g.b, o);
      if (bn) { zero(g.g, o); zero(g.bt, o); }
    });
    if (!ok) return fail(MTMC_E_HIP, "hipMemsetAsync failed in mtmc_mpn_backward");
  }
  // the workspace side: statistics blocks, per-round dP/dQ, dh0, de0, the first de / dh buffers -- one range
  HIP_OK(hipMemsetAsync(x.ws + lo.bwd_zero, 0, lo.bwd_zero_end - lo.bwd_zero, s));
  mtmc::launch_transpose_multi(tj, s);
  return MTMC_OK;
}

// the incoming d_h, and without rounds the classifier on the encoded edges
int bwd_seed(Bwd& b) {
  const Ctx& x = b.x;
  const mtmc_mpn_model* m = b.x.m;
  const int64_t N = x.c->n_nodes, E = x.c->n_edges;
  const bool rounds = m->num_enc_steps > 0;
  if (b.d_h)
    HIP_OK(hipMemcpyAsync(rounds ? b.g_h(b.cur) : b.g_h0(), b.d_h, (size_t)N * 32 * sizeof(float), hipMemcpyDeviceToDevice, x.stream));
  if (!rounds && b.d_logits_steps && b.d_logits_steps[0] && E > 0)
    mtmc::launch_bwd_classify_e0(enc_params(x), x.c->edge_attr, E, (double)E, m->cls.weight, m->cls.out_dim,
                                 b.d_logits_steps[0], b.g_e0(), b.gr.cls.w, b.gr.cls.b, x.stream);
  return MTMC_OK;
}

// message-passing round r: node-update MLP, edge-update MLP + classifier, node projections
int bwd_round(Bwd& b, int r) {
  const Ctx& x = b.x;
  const mtmc_mpn_model* m = b.x.m;
  const Layout& lo = x.lo;
  hipStream_t s = x.stream;
  const int64_t N = x.c->n_nodes;
  const int hn = node_in_width(m);

  mtmc::BwdRoundParams bp;
  bp.f = round_params(x, r);
  bp.g_h = b.g_h(b.cur); bp.h_agg = x.at<float>(lo.h_tr[r]); bp.deg = x.at<int>(lo.pub.deg_off);
  bp.arg = x.at<int>(lo.g_arg);
  const int step = r + 1, first_cls = first_cls_step(m);
  bp.d_logits = (b.d_logits_steps && step >= first_cls) ? b.d_logits_steps[step - first_cls] : nullptr;
  bp.g_de2 = x.at<float>(lo.g_de2);
  bp.g_Q = x.at<float>(lo.g_Q) + (size_t)r * N * 32; bp.g_P = x.at<float>(lo.g_P) + (size_t)r * mtmc::kGradRep * N * 8;
  bp.g_e = b.g_e(b.cur_e); bp.g_e_prev = b.g_e(b.cur_e ^ 1); bp.g_e0 = b.g_e0(); bp.bst = b.bst_block(2 * r);
  bp.un = b.gr.upd_node; bp.ue = b.gr.upd_edge; bp.cls = b.gr.cls;
  bp.gacc = x.at<float>(lo.gacc);

  if (m->agg == MTMC_AGG_MAX) {
    HIP_OK(hipMemsetAsync(bp.arg, 0x7f, (size_t)N * 32 * sizeof(int32_t), s));
    mtmc::launch_bwd_node_upd(bp, 2, s);
  }
  mtmc::launch_bwd_node_upd(bp, 0, s);
  mtmc::launch_bwd_node_upd(bp, 1, s);
  bp.bst = b.bst_block(2 * r + 1);
  mtmc::launch_bwd_edge_upd(bp, 0, s);
  mtmc::launch_bwd_edge_upd(bp, 1, s);

  // P, Q of this round are on the tape (Layout::P_tr / Q_tr); what bwd_node_proj needs of the forward's node_proj:
  mtmc::BwdProjParams pp;
  pp.g_P = bp.g_P; pp.g_Q = bp.g_Q; pp.h_src = round_h_src(x, r);
  pp.h0 = m->reattach_nodes ? x.at<float>(lo.pub.h0_off) : nullptr;
  pp.deg = (m->agg == MTMC_AGG_MEAN && r > 0) ? x.at<int>(lo.pub.deg_off) : nullptr;
  pp.ue_w = m->upd_edge.weight; pp.ue_ld = m->upd_edge.in_dim; pp.un_w = m->upd_node.weight; pp.un_ld = m->upd_node.in_dim;
  pp.hn = hn;
  pp.g_h_prev = b.g_h(b.cur ^ 1); pp.g_h0 = b.g_h0(); pp.src_is_h0 = r == 0;
  pp.gr_ue_w = b.gr.upd_edge.w; pp.gr_un_w = b.gr.upd_node.w; pp.n_nodes = N;
  mtmc::launch_bwd_node_proj(pp, s);
  b.cur ^= 1;
  b.cur_e ^= 1;
  return MTMC_OK;
}

void bwd_edge_encoder(Bwd& b) {
  const Ctx& x = b.x;
  const int64_t E = x.c->n_edges;
  mtmc::BwdEncParams ep;
  ep.enc = enc_params(x); ep.attr = x.c->edge_attr; ep.n_edges = E; ep.e_total = (double)E; ep.g_e0 = b.g_e0();
  ep.bst = b.bst_block(2 * x.m->num_enc_steps); ep.d_attr = b.d_edge_attr;
  ep.gacc = x.at<float>(x.lo.gacc);
  ep.l1 = b.gr.enc_edge[0]; ep.l2 = b.gr.enc_edge[1];
  for (int pass = 0; pass < 3; ++pass) mtmc::launch_bwd_edge_enc(ep, pass, x.stream);
}

// node-encoder layer l: BatchNorm backward (+ the recomputation of the layer's input activation), then two fp32-MFMA GEMMs on
// transposed operands
int bwd_node_encoder_layer(Bwd& b, int l) {
  const Ctx& x = b.x;
  const mtmc_mpn_model* m = b.x.m;
  const Layout& lo = x.lo;
  hipStream_t s = x.stream;
  const int64_t N = x.c->n_nodes, npad = b.npad;
  const mtmc_layer& Lr = m->enc_node[l];
  const int d = Lr.out_dim, in = Lr.in_dim;
  float* tA = x.at<float>(lo.tA);
  float* tB = x.at<float>(lo.tB);
  float* zeros = x.at<float>(lo.zeros);
  // dh0 is the last layer's dA: bn_bwd turns it into dY in place, where the edge rounds' backward left it
  float* dY = (l == m->n_enc_layers - 1) ? b.g_h0() : b.gA;
  size_t sb_off = 0;
  for (int j = 0; j < l; ++j) sb_off += 2 * (size_t)m->enc_node[j].out_dim;
  mtmc::BnBwdParams bb;
  bb.Y = x.at<float>(lo.Y[l]); bb.dA = dY; bb.rows = N; bb.dim = d;
  bb.stats_fwd = x.at<double>(lo.pub.stat_enc_layer_off[l]); bb.stats_bwd = x.at<double>(lo.bst_n) + sb_off; bb.count = (double)N;
  bb.gamma = Lr.gamma; bb.beta = Lr.beta; bb.drop = make_drop(x, m->dropout_enc); bb.drop_stream = mtmc::kDropEncNode + l;
  bb.gr = b.gr.enc_node[l];
  // |.|max of the three GEMM operands of this layer: dY_l (written by bn_bwd's apply pass), a_{l-1} (x: the forward's
  // value; else from the recomputation below) and W_l (the forward's) -> the fp16 three-product kernel applies
  unsigned* amax_dy = x.at<unsigned>(lo.amax_bwd) + (size_t)l * mtmc::kAmaxRep;
  unsigned* amax_act = x.at<unsigned>(lo.amax_bwd) + (size_t)(MTMC_MAX_ENC_LAYERS + l) * mtmc::kAmaxRep;
  bb.amax_out = amax_dy;
  bb.dT = tA; bb.ldt = npad;                                       // dY_l^T comes out of the apply pass directly
  // the layer's input activation a_{l-1}: x itself, or relu(bn(Y_{l-1})) with its dropout mask -- recomputed, with its
  // transpose and its |.|max.  Nothing of it depends on dY_l: where the 16x64 transposing form takes the shape, the job rides
  // as the z = 1 workgroups of the apply launch; else it is a launch of its own behind it
  const float* aT = b.tX;                                          // a_{l-1}^T [in][npad]
  if (l > 0) {
    const mtmc_layer& Pv = m->enc_node[l - 1];
    bb.rc = {x.at<float>(lo.Y[l - 1]), Pv.out_dim, N, Pv.out_dim, x.at<double>(lo.pub.stat_enc_layer_off[l - 1]), Pv.gamma, Pv.beta,
             (double)N, b.gB, make_drop(x, m->dropout_enc), mtmc::kDropEncNode + l - 1, 0, amax_act, tB, npad};
    bb.rc_on = mtmc::rows_t_form_takes(bb.rc) ? 1 : 0;
    aT = tB;
  }
  mtmc::launch_bn_bwd(bb, 0, s);
  mtmc::launch_bn_bwd(bb, 1, s);                                   // dY now holds dY_l (+ a_{l-1}, a_{l-1}^T)
  if (l > 0 && !bb.rc_on) mtmc::launch_bn_relu_rows(bb.rc, s);
  // dW_l [d][in] = dY^T . a  -> NT GEMM on the transposes (reduction over the node rows, padded to 32)
  mtmc::GemmParams g = mtmc::plain_gemm(tA, npad, aT, zeros, b.gr.enc_node[l].w, in, d, (int)npad, in, amax_dy,
                                        l > 0 ? amax_act : amax_x(x));
  if (int rc = mtmc::launch_gemm_bn(g, s)) return fail(rc, "backward: weight-gradient GEMM shape");
  // dA_{l-1} [N][in] = dY . W_l  -> NT GEMM against W^T
  if (l > 0 || b.d_x) {
    g = mtmc::plain_gemm(dY, d, b.tWl[l], zeros, l > 0 ? b.gB : b.d_x, in, N, d, in, amax_dy, amax_w(x, l));    // W_l^T [in][d]
    if (int rc = mtmc::launch_gemm_bn(g, s)) return fail(rc, "backward: input-gradient GEMM shape");
    std::swap(b.gA, b.gB);
  }
  return MTMC_OK;
}

// the replicated small-gradient sums of the edge kernels -> the caller's tensors
void bwd_fold(Bwd& b) {
  const mtmc_mpn_model* m = b.x.m;
  const int hn = node_in_width(m);
  mtmc::GradFoldParams fp;
  fp.gacc = b.x.at<float>(b.x.lo.gacc);
  fp.un = b.gr.upd_node; fp.ue = b.gr.upd_edge; fp.cls = b.gr.cls; fp.l1 = b.gr.enc_edge[0]; fp.l2 = b.gr.enc_edge[1];
  fp.un_ld = m->upd_node.in_dim; fp.un_eoff = hn;
  fp.ue_ld = m->upd_edge.in_dim; fp.ue_eoff = 2 * hn; fp.nin = m->reattach_edges ? 8 : 4;
  fp.n_classes = m->cls.out_dim;
  fp.fe = m->enc_edge[0].in_dim;
  mtmc::launch_grad_fold(fp, b.x.stream);
}

}  // namespace

static int backward_impl(const mtmc_mpn_model* model, const mtmc_mpn_call* call, const float* const* d_logits_steps,
                         const float* d_h, const mtmc_mpn_model* grads, void* grads_flat, size_t grads_flat_bytes,
                         float* d_x, float* d_edge_attr) {
  Bwd b;
  Ctx& x = b.x;
  if (int rc = make_ctx(model, call, &x)) return rc;
  if (!call->training) return fail(MTMC_E_ARG, "mtmc_mpn_backward needs the call of a training-mode forward");
  if (int rc = check_grads(model, grads)) return rc;
  b.gr.n_enc_layers = model->n_enc_layers;
  for_each_layer(b.gr, *grads, [](mtmc::LayerGrad& to, const mtmc_layer& from, bool) { to = layer_grad(from); });
  b.d_logits_steps = d_logits_steps; b.d_h = d_h;
  b.grads_flat = grads_flat; b.grads_flat_bytes = grads_flat_bytes;
  b.d_x = d_x; b.d_edge_attr = d_edge_attr;
  b.bst = x.at<double>(x.lo.bst);
  b.tX = x.at<float>(x.lo.tX);
  b.npad = (call->n_nodes + 31) / 32 * 32;
  b.gA = x.at<float>(x.lo.gA); b.gB = x.at<float>(x.lo.gB);

  if (int rc = bwd_clear_and_transpose(b)) return rc;
  if (int rc = bwd_seed(b)) return rc;
  for (int r = model->num_enc_steps - 1; r >= 0; --r)
    if (int rc = bwd_round(b, r)) return rc;
  bwd_edge_encoder(b);
  for (int l = model->n_enc_layers - 1; l >= 0; --l)
    if (int rc = bwd_node_encoder_layer(b, l)) return rc;
  bwd_fold(b);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MTMC_E_HIP, "kernel launch failed in backward: %s", hipGetErrorString(e));
  return MTMC_OK;
}

extern "C" int32_t mtmc_mpn_backward(const mtmc_mpn_model* model, const mtmc_mpn_call* call, const float* d_logits,
                                     const float* d_h, const mtmc_mpn_model* grads, float* d_x, float* d_edge_attr) {
  const float* steps[64];
  int n_out = 0;
  if (int rc = check_model(model)) return rc;          // (incl. the struct-size guards, before any field is trusted)
  if (int rc = check_call_size(call)) return rc;
  if (d_logits) {
    n_out = model->num_enc_steps > 0 ? std::min(model->num_class_steps, model->num_enc_steps) : 1;
    if (n_out > 64) return fail(MTMC_E_ARG, "more than 64 classified steps");
    for (int i = 0; i < n_out; ++i) steps[i] = d_logits + (size_t)i * call->n_edges * model->cls.out_dim;
  }
  return backward_impl(model, call, d_logits ? steps : nullptr, d_h, grads, nullptr, 0, d_x, d_edge_attr);
}

extern "C" int32_t mtmc_mpn_backward_steps(const mtmc_mpn_model* model, const mtmc_mpn_call* call,
                                           const float* const* d_logits_steps, const float* d_h,
                                           const mtmc_mpn_model* grads, void* grads_flat, size_t grads_flat_bytes,
                                           float* d_x, float* d_edge_attr) {
  return backward_impl(model, call, d_logits_steps, d_h, grads, grads_flat, grads_flat_bytes, d_x, d_edge_attr);
}

// The same with the gradient carving done here: `flat` (fp32, flat_floats long) receives every parameter gradient in
// struct order -- node encoder layers, edge encoder, edge update, node update, classifier; weight, bias, then gamma, beta
// where the layer has a BatchNorm -- each piece starting on a 64-float (256-byte) boundary.  The host makes ONE allocation
// and views it with the same rule (mtmc_mpn_grad_layout: offsets in floats, returns the total), instead of filling a
// second 34-pointer struct per call.
extern "C" int64_t mtmc_mpn_grad_layout(const mtmc_mpn_model* m, int64_t* offsets, int32_t max_offsets) {
  if (!m || m->struct_bytes != sizeof(mtmc_mpn_model) || m->n_enc_layers < 1 || m->n_enc_layers > MTMC_MAX_ENC_LAYERS)
    return 0;                                                                           // (0 = no layout: bad model)
  int64_t total = 0;
  int n = 0;
  auto piece = [&](int64_t numel) {
    if (offsets && n < max_offsets) offsets[n] = total;
    ++n;
    total += (numel + 63) / 64 * 64;
  };
  for_each_layer(*m, [&](const mtmc_layer& l, bool bn) {
    piece((int64_t)l.out_dim * l.in_dim);
    piece(l.out_dim);
    if (bn) { piece(l.out_dim); piece(l.out_dim); }
  });
  return total;
}

extern "C" int32_t mtmc_mpn_backward_flat(const mtmc_mpn_model* model, const mtmc_mpn_call* call,
                                          const float* const* d_logits_steps, const float* d_h, float* flat,
                                          int64_t flat_floats, float* d_x, float* d_edge_attr) {
  if (!model || !flat) return fail(MTMC_E_ARG, "mtmc_mpn_backward_flat: NULL model or gradient buffer");
  if (int rc = check_model(model)) return rc;          // before anything indexes enc_node[] / off[] by n_enc_layers
  int64_t off[4 * (MTMC_MAX_ENC_LAYERS + 4) + 2];
  const int64_t need = mtmc_mpn_grad_layout(model, off, (int32_t)(sizeof(off) / sizeof(off[0])));
  if (flat_floats < need) return fail(MTMC_E_ARG, "mtmc_mpn_backward_flat: gradient buffer too small");
  mtmc_mpn_model g = *model;
  int n = 0;
  for_each_layer(g, [&](mtmc_layer& l, bool bn) {
    l.weight = flat + off[n++];
    l.bias = flat + off[n++];
    l.gamma = bn ? flat + off[n++] : nullptr;
    l.beta = bn ? flat + off[n++] : nullptr;
  });
  return backward_impl(model, call, d_logits_steps, d_h, &g, flat, (size_t)need * sizeof(float), d_x, d_edge_attr);
}

