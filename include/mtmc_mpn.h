/*
 * mtmc_mpn.h -- C ABI of the MI355X (gfx950) message-passing-network forward.
 *
 * This is the drop-in boundary for ONE hot path of
 * elun15/Graph-Convolutional-Network-for-Multi-Camera-Vehicle-Tracking: `MOTMPNet.forward`
 * (reference models/mpn.py:250-299).  Every pointer is a plain device pointer into HBM, every
 * size a plain integer; there are no torch (or any other framework) types in the signatures.
 * The host side that mirrors the reference's nn.Module interface (mtmc_mpn/modules.py) binds
 * these entry points with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Reference interface each entry point replaces:
 *   mtmc_mpn_forward           <- MOTMPNet.forward              models/mpn.py:250-299
 *     (node/edge encoders       MLPGraphIndependent.forward      models/mpn.py:128-142,
 *      MLP = Linear+BN+ReLU     MLP.forward                      models/mlp.py:11-33,
 *      one round                MetaLayer.forward                models/mpn.py:32-54,
 *      edge update              EdgeModel.forward                models/mpn.py:67-69,
 *      node update + aggregate  NodeModel.forward                models/mpn.py:97-99,
 *      classifier               MLPGraphIndependent.forward      models/mpn.py:291-292)
 *   mtmc_mpn_run_phase         <- the same, cut at the points where a multi-GPU run exchanges
 *                                 BatchNorm statistics / node states (no reference counterpart:
 *                                 the reference is single-GPU)
 *   mtmc_scatter_{add,mean,max}<- torch_scatter.scatter_{add,mean,max}(src, index, dim=0, dim_size)
 *                                 (third-party pytorch-scatter 2.0.8; call sites models/mpn.py:196,199,202);
 *                                 mtmc_scatter_grouped: the same three as a repeatable segmented reduction over a
 *                                 grouping of the rows, mtmc_group_by_index: that grouping (a stable radix sort)
 *   mtmc_mlp_forward           <- MLP.forward as a stand-alone op  models/mlp.py:32-33
 *   mtmc_build_graph           <- graph construction around the call  inference.py:402-456, train.py:316-342
 *   mtmc_postprocess           <- softmax/argmax + post_processing    inference.py:475-489, :70-169; utils.py:30-339
 *   mtmc_pool_tracklets        <- per-tracklet mean of the detections' embeddings  train.py:305-316,
 *                                 libs/reid_feature_extraction.py:177-178 (mtmc_pool_tracklets_weighted: rows in any order, a weight per
 *                                 detection, libs/filter_mtmc.py's filters as weights)
 *   mtmc_id_filter / _overlap / _cells / _assign <- IDF1 / IDP / IDR of a result  main.py:166-213, eval/eval.py::eval
 *   mtmc_mot_pairs / _walk     <- the CLEAR MOT columns of that result (MOTA, MOTP, switches, ...)  eval/eval.py:409-411
 *
 * All floating tensors are fp32, row-major, contiguous unless a stride argument says otherwise;
 * BatchNorm statistics are accumulated in fp64.  All work is enqueued on `stream` (a hipStream_t
 * passed as void*; NULL = the default stream); no entry point synchronises or allocates.
 * Return value: 0 on success, a negative MTMC_E_* code otherwise.  Every entry point that returns a code then leaves its
 * reason in mtmc_mpn_last_error() (one text per host thread); the stand-alone operators start it with their own name
 * without `mtmc_`, as in "edge_loss_forward: ...".
 */
#ifndef MTMC_MPN_H
#define MTMC_MPN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTMC_MPN_ABI_VERSION 6

#define MTMC_MAX_ENC_LAYERS 8   /* hidden layers of the node encoder MLP          */
#define MTMC_NODE_DIM 32        /* H : width of the node state the kernels are built for */
#define MTMC_EDGE_DIM 4         /* He: width of the edge state                    */
#define MTMC_MAX_CLASSES 4      /* classifier outputs per edge (reference: 2)     */

enum { MTMC_AGG_SUM = 0, MTMC_AGG_MEAN = 1, MTMC_AGG_MAX = 2 };

enum {
  MTMC_OK = 0,
  MTMC_E_ARG = -1,        /* bad dimension / NULL pointer / unsupported shape      */
  MTMC_E_WORKSPACE = -2,  /* workspace too small or misaligned                     */
  MTMC_E_HIP = -3,        /* a HIP runtime call failed                             */
  MTMC_E_ROWS = -4        /* fewer than 2 rows under a BatchNorm (the reference raises ValueError) */
};

/* One Linear(+BatchNorm affine) group: weight [out,in] row-major, bias [out], gamma/beta [out]. */
typedef struct mtmc_layer {
  const float* weight;
  const float* bias;
  const float* gamma;   /* BatchNorm1d.weight */
  const float* beta;    /* BatchNorm1d.bias   */
  int32_t in_dim;
  int32_t out_dim;
} mtmc_layer;

/* The 34 parameter tensors of the reference model + its structural flags. */
typedef struct mtmc_mpn_model {
  uint32_t struct_bytes;                        /* = sizeof(mtmc_mpn_model) of the header the CALLER was compiled against;
                                                   every entry point returns MTMC_E_ARG unless it equals the library's
                                                   (a binding written for an older, shorter struct fails loudly instead
                                                   of being read past its end) */
  int32_t n_enc_layers;                         /* node encoder: 2048->1024->512->128->32 => 4 */
  mtmc_layer enc_node[MTMC_MAX_ENC_LAYERS];     /* encoder.node_mlp.fc_layers.{0,4,8,12}(+1)   */
  mtmc_layer enc_edge[2];                       /* encoder.edge_mlp: in(1|2)->4->4              */
  mtmc_layer upd_edge;                          /* MPNet.edge_model.edge_mlp: [4, nf*64+ef*4]   */
  mtmc_layer upd_node;                          /* MPNet.node_model.node_mlp: [32, nf*32+4]     */
  mtmc_layer cls;                               /* classifier.edge_mlp.fc_layers.0: [C,4], no BN */
  int32_t agg;                                  /* MTMC_AGG_*  (node_agg_fn)                    */
  int32_t num_enc_steps;                        /* L                                            */
  int32_t num_class_steps;                      /* Cs                                           */
  int32_t reattach_nodes;                       /* reattach_initial_nodes                       */
  int32_t reattach_edges;                       /* reattach_initial_edges                       */
  float dropout_enc;                            /* Dropout p of both encoder MLPs (training only) */
  float dropout_upd_edge;                       /* ... of the edge-update MLP                     */
  float dropout_upd_node;                       /* ... of the node-update MLP                     */
} mtmc_mpn_model;

/* One forward call.  For a single GPU: node_lo=0, node_hi=n_nodes, n_edges_total=n_edges. */
typedef struct mtmc_mpn_call {
  uint32_t struct_bytes;     /* = sizeof(mtmc_mpn_call), checked like mtmc_mpn_model::struct_bytes */
  const float* x;            /* [node_hi-node_lo, F] rows node_lo.. of data.x           */
  int64_t x_row_stride;      /* elements between consecutive rows of x                  */
  const int64_t* row;        /* data.edge_index[0]: element e at row[e*idx_stride]      */
  const int64_t* col;        /* data.edge_index[1]                                      */
  int64_t idx_stride;        /* 1 for a contiguous [2,E]; 2 for the callers' [E,2].T view */
  const float* edge_attr;    /* [n_edges, edge_in_dim] contiguous                       */
  int64_t n_nodes;           /* N (global)                                              */
  int64_t n_edges;           /* E held by this call (the local shard)                   */
  int64_t n_edges_total;     /* E over all shards: the BatchNorm row count              */
  int64_t node_lo, node_hi;  /* node rows this call encodes                             */
  float* logits;             /* out [n_outputs][n_edges][C]; n_outputs = Cs, or 1 if L==0 */
  float* h_out;              /* out [n_nodes][32] = latent_node_feats                   */
  void* workspace;           /* >= mtmc_mpn_workspace_bytes(), 256-byte aligned         */
  size_t workspace_bytes;
  int32_t training;          /* 0: eval (Dropout = identity).  1: train: counter-based Dropout masks from `seed`,
                                every round keeps its own buffers so the workspace doubles as the backward tape
                                (size it with mtmc_mpn_train_workspace_bytes)                              */
  int32_t flags;             /* MTMC_F_*                                                */
  uint64_t seed;
  void* stream;              /* hipStream_t                                             */
  int64_t row_lo, row_hi;    /* multi-GPU, row-complete edge shards: MTMC_PH_ROUND_PROJ / _STAT work on node rows
                                [row_lo,row_hi) only -- the source rows of this call's edges; the host then exchanges
                                the column projections (mtmc_ws_layout.P_off) instead of the node state.  0,0 = all */
  void* weight_cache;        /* eval mode, optional (NULL = none): >= mtmc_mpn_weight_cache_bytes() of device memory, 256-byte
                                aligned, ZERO-FILLED once by the caller and then left alone between calls.  The library keeps
                                what it derives from the node-encoder WEIGHTS alone in it (fp16 operand planes, row scales) and
                                verifies it against the weights' CONTENT on every call -- a 64-bit fingerprint per 8 weight rows,
                                taken on the device -- so the caller promises nothing about the weights: a single changed word
                                is always seen, a change of several words is missed with probability about 2^-64 per 8 rows;
                                a changed chunk is split again, an unchanged one is not.  One cache per stream that runs forwards concurrently.
                                Few-row graphs need it for the kernels of csrc/gemm_few.hip (without: the split-K kernels).   */
  size_t weight_cache_bytes;
} mtmc_mpn_call;

#define MTMC_F_DETERMINISTIC 1   /* row-sorted edge lists: sum/mean aggregation through per-chunk partials added in
                                    a fixed order instead of float atomics (bitwise run-to-run reproducible h) */
#define MTMC_F_GLOBAL_DEG 4      /* mean aggregation divides by workspace deg_global (multi-GPU) instead of deg */
/* (8 was MTMC_F_WEIGHTS_CACHED in ABI v5: a host-side promise that the weights had not changed.  Gone: the weight-plane
 * cache verifies itself, mtmc_mpn_call::weight_cache.) */
#define MTMC_F_FORK 2            /* run the edge branch (prep, edge-encoder moments) on an internal side stream
                                    beside the node-encoder GEMMs, joined by events (default: one stream) */
#define MTMC_F_SEED_ON_DEVICE 16 /* training: `seed` holds the ADDRESS of a uint64 counter in device memory (8-byte aligned).  The
                                    forward takes the counter's value as this call's Dropout seed, stores it in the workspace
                                    (= the tape: the backward of the same tape reads it there) and moves the counter on by one --
                                    on the stream, so a HIP graph that holds a whole training step (forward, loss, backward,
                                    optimizer) draws new masks on every replay.  Additive in ABI v6: calls without the bit are
                                    as before (`seed` by value).  Reference: nn.Dropout's generator state, models/mlp.py:20-21 */

/* Byte offsets inside the workspace of the regions a multi-GPU host exchanges between phases.
 * Every statistics block is kept in MTMC_STAT_REPLICAS replicas (consumers add them up), so a host simply
 * all-reduces the whole replicated block.  Strides are in doubles. */
#define MTMC_STAT_REPLICAS 16
#define MTMC_ATTR_STRIDE 16      /* edge_attr moments : m1[2] | m2 packed upper triangle[3]                */
#define MTMC_ENC2_STRIDE 16      /* hidden edge-encoder moments : m1[4] | m2 packed[10]                     */
#define MTMC_Z1_STRIDE 16        /* edge-update pre-activation : sum[4] | sumsq[4]                          */
#define MTMC_M_STRIDE 16         /* updated edge state e' : m1[4] | m2 packed[10]                           */
#define MTMC_Z2_STRIDE 64        /* node-update pre-activation : sum[32] | sumsq[32] (without the A M A^T term) */
#define MTMC_ROUND_BLOCK (MTMC_STAT_REPLICAS * (MTMC_Z1_STRIDE + MTMC_M_STRIDE + MTMC_Z2_STRIDE))
typedef struct mtmc_ws_layout {
  size_t total_bytes;
  size_t zero_bytes;         /* the leading region [0, zero_bytes) is cleared by MTMC_PH_BEGIN           */
  size_t flags_off;          /* int32[8]: [0] rows out of order, [1] indices out of range                */
  size_t stat_attr_off;      /* f64[REPLICAS][ATTR_STRIDE]; DIRECTLY followed by encoder layer 0's block: a multi-GPU
                                host all-reduces [stat_attr_off, stat_enc_layer_off[0] + 16 * out_dim_0) as ONE message
                                after MTMC_PH_NODE_COMBINE 0 (the edge branch's statistics ride with the node encoder's) */
  size_t stat_enc2_off;      /* f64[REPLICAS][ENC2_STRIDE]; directly followed by encoder layer 1's block (if there is one) */
  size_t stat_enc_layer_off[MTMC_MAX_ENC_LAYERS];  /* per encoder layer l: f64[2][out_dim_l] column sum | sumsq    */
  size_t stat_round_off;     /* f64[L][ROUND_BLOCK]: per round the z1, e'-moment and z2 blocks in order   */
  size_t deg_off;            /* i32[N]  out-degree of the LOCAL edges (row histogram)                     */
  size_t seg_off;            /* f64[N][4] per-node segment sums of e' over the LOCAL edges (many-edge lists; zero bytes
                                on few-edge lists, whose pass B adds the statistics' edge part itself)            */
  size_t h0_off;             /* f32[N][32] encoded node state (rows node_lo..node_hi written locally)      */
  size_t h_acc_off[2];       /* f32[N][32] x2 aggregation ping-pong: round r aggregates into [r & 1],
                                except that the last round of a sum/max model aggregates into h_out       */
  size_t deg_global_off;     /* i32[N]  degree over all shards; read instead of deg for mean aggregation
                                when MTMC_F_GLOBAL_DEG is set (the host fills it)                         */
  size_t P_off;              /* f32[2][N][4] the round's edge-update projections: Pr rows, then Pc rows (gathered
                                by column: every shard needs ALL of Pc, 16 B per node, and only its own Pr / Q)   */
} mtmc_ws_layout;

enum {                       /* phases in forward order; `arg` = encoder layer or round (0-based) */
  MTMC_PH_BEGIN = 0,         /* clear statistics; int64 -> int32 indices; degree; attr moments   */
  MTMC_PH_EDGE_ENC = 1,      /* moments of the edge-encoder hidden layer                         */
  MTMC_PH_NODE_ENC = 2,      /* arg = layer: GEMM (+ column statistics unless split along K)      */
  MTMC_PH_NODE_H0 = 3,       /* h0 = relu(bn(Y_last)) for rows [node_lo,node_hi)                 */
  MTMC_PH_ROUND_PROJ = 4,    /* arg = round: per-node projections Pr|Pc|Q, clear next h buffer   */
  MTMC_PH_ROUND_A = 5,       /* statistics of the edge-update pre-activation                     */
  MTMC_PH_ROUND_B = 6,       /* e' (stored), its moments and per-node segment sums               */
  MTMC_PH_ROUND_STAT = 7,    /* statistics of the node-update pre-activation by moments (many-edge lists; a no-op on
                                few-edge lists: complete after MTMC_PH_ROUND_PROJ + MTMC_PH_ROUND_B there)      */
  MTMC_PH_ROUND_C = 8,       /* messages, aggregation into h, classifier logits                  */
  MTMC_PH_END = 9,           /* mean scaling / copy of the final node state to h_out             */
  MTMC_PH_NODE_COMBINE = 10  /* arg = layer, right after MTMC_PH_NODE_ENC: sums the split-K slabs of a few-row
                                layer and takes its column statistics (no-op when the layer was not split) */
};

int32_t mtmc_mpn_abi_version(void);
const char* mtmc_mpn_last_error(void);
size_t mtmc_mpn_workspace_bytes(const mtmc_mpn_model* model, int64_t n_nodes, int64_t n_edges);
size_t mtmc_mpn_weight_cache_bytes(const mtmc_mpn_model* model);   /* size of mtmc_mpn_call::weight_cache (0: bad model) */
int32_t mtmc_mpn_workspace_layout(const mtmc_mpn_model* model, int64_t n_nodes, int64_t n_edges,
                                  mtmc_ws_layout* out);
int32_t mtmc_mpn_forward(const mtmc_mpn_model* model, const mtmc_mpn_call* call);

/* Training (reference train.py:356,424: outputs, _ = model(data); loss.backward()).
 * Forward: mtmc_mpn_forward with call->training = 1 and a workspace of mtmc_mpn_train_workspace_bytes().
 * Backward: the SAME model/call (same workspace, untouched since the forward) plus the incoming gradients
 *   d_logits [n_outputs][E][C] and d_h [N][32] (either may be NULL = zero).  `grads` has the layout of the model
 *   struct; its weight/bias/gamma/beta pointers name the buffers that RECEIVE the 34 parameter gradients
 *   (overwritten, fp32).  d_x [N][F] / d_edge_attr [E][Fe] are written if non-NULL. */
size_t mtmc_mpn_train_workspace_bytes(const mtmc_mpn_model* model, int64_t n_nodes, int64_t n_edges);
int32_t mtmc_mpn_backward(const mtmc_mpn_model* model, const mtmc_mpn_call* call, const float* d_logits,
                          const float* d_h, const mtmc_mpn_model* grads, float* d_x, float* d_edge_attr);
/* The same with one gradient pointer per classified step (host array of min(Cs, L) device pointers, NULL entries =
 * no gradient for that step; what torch.autograd hands over) and, optionally, the ONE buffer all gradient tensors
 * of `grads` were carved from: it is cleared with a single memset instead of one per tensor. */
int32_t mtmc_mpn_backward_steps(const mtmc_mpn_model* model, const mtmc_mpn_call* call,
                                const float* const* d_logits_steps, const float* d_h, const mtmc_mpn_model* grads,
                                void* grads_flat, size_t grads_flat_bytes, float* d_x, float* d_edge_attr);
/* The same with the gradient carving done by the library: `flat` receives every parameter gradient in struct order
 * (node encoder layers, edge encoder, edge update, node update, classifier; weight, bias, then gamma, beta where the layer
 * has a BatchNorm), each piece on a 64-float boundary; mtmc_mpn_grad_layout writes the piece offsets (in floats, up to
 * max_offsets of them) and returns the total length.  One allocation and no second pointer struct per call. */
int64_t mtmc_mpn_grad_layout(const mtmc_mpn_model* model, int64_t* offsets, int32_t max_offsets);
int32_t mtmc_mpn_backward_flat(const mtmc_mpn_model* model, const mtmc_mpn_call* call,
                               const float* const* d_logits_steps, const float* d_h, float* flat, int64_t flat_floats,
                               float* d_x, float* d_edge_attr);
int32_t mtmc_mpn_run_phase(const mtmc_mpn_model* model, const mtmc_mpn_call* call, int32_t phase, int32_t arg);
/* n consecutive (phase, arg) pairs in ONE call (phase_args[2*i], phase_args[2*i+1]): what a multi-GPU host runs between two
 * of its collectives, without one library call (and one argument check) per phase. */
int32_t mtmc_mpn_run_phases(const mtmc_mpn_model* model, const mtmc_mpn_call* call, const int32_t* phase_args, int32_t n);

/* Which kernels a call would run -- a host-only query (nothing is launched, no pointer of `call` is read: only its
 * sizes, ranges, flags and `training`), so that a multi-GPU host or a test can check that a SHARD takes the kernels the
 * whole graph would.  Encoder layers are planned for the node_hi - node_lo rows the call encodes. */
enum { MTMC_GEMM_GENERIC = 0, MTMC_GEMM_INLOOP_64 = 1, MTMC_GEMM_INLOOP_128 = 2, MTMC_GEMM_PRESPLIT_256 = 3,
       MTMC_GEMM_STAGED_128 = 4, MTMC_GEMM_ROWS_16 = 5, MTMC_GEMM_FEW_L0 = 6, MTMC_GEMM_FEW_WAVE = 7 };
enum { MTMC_PASS_C_WALK = 0, MTMC_PASS_C_MFMA_SORTED = 1, MTMC_PASS_C_MFMA_ANY = 2 };
typedef struct mtmc_mpn_plan {
  int32_t enc_kernel[MTMC_MAX_ENC_LAYERS];   /* MTMC_GEMM_*: one-thread-per-output fallback / in-loop operand split on
                                                64x64 or 128x128 tiles / pre-split fp16 planes + 256x256 tiles / (layers
                                                >= 1 of many-row graphs) 128 x 256 or 256 x 128 tiles staged by producer waves /
                                                (narrow last layers of many-row graphs) one wave per 16 rows /
                                                (few-row graphs with a weight-plane cache: the call's weight_cache pointer is
                                                tested for NULL, never read) layer 0 on pre-split operands in 64 x 32 tiles over
                                                all of K / later layers with K cut between the waves of a workgroup   */
  int32_t enc_split_k[MTMC_MAX_ENC_LAYERS];  /* K slices (few-row layers; > 1 => MTMC_PH_NODE_COMBINE does work)    */
  int32_t edges_per_thread;                  /* passes A / B                                                        */
  int32_t lazy_edges;                        /* 1: e' is never stored, consumers recompute it from z1               */
  int32_t pass_c;                            /* MTMC_PASS_C_*: half-wave walk / pass_c_sorted_kernel (many-edge lists; it
                                                returns at once on unsorted rows and the walk behind it does the round) /
                                                the any-order matrix-core kernel (few-edge lists: alone; many-edge lists
                                                of >= 2^24 global node rows: returns on unsorted rows like the sorted one) */
  double avg_degree;                         /* edges per source row the pass-C choice was made on                  */
  int32_t pass_a_col_blocks;                 /* 0: pass A walks the edges in order; B > 0: by B column blocks, so that the
                                                gathered projections Pc of a block stay in an XCD's L2 (graphs whose 16 B / node
                                                table outgrows it; row-sorted lists with ascending columns -- decided on the
                                                device, the in-order kernel is launched behind it)                     */
  int32_t layer0_panels;                     /* mtmc_mpn_forward only: row panels of the pre-split layer 0 (the operand split of
                                                panel i + 1 runs on a side stream beside panel i's GEMM); 1 = one split pass, one
                                                GEMM (also what mtmc_mpn_run_phase(s) does)                              */
  int32_t enc2_passenger;                    /* mtmc_mpn_forward only: 1 = MTMC_PH_EDGE_ENC's work rides as passenger workgroups
                                                in the last node-encoder layer's launch (few-row, few-edge graphs)       */
  int32_t node_stat_folded;                  /* 1 = few-edge list: the node-update statistics come out of MTMC_PH_ROUND_PROJ +
                                                MTMC_PH_ROUND_B, MTMC_PH_ROUND_STAT launches nothing                     */
} mtmc_mpn_plan;
int32_t mtmc_mpn_plan_call(const mtmc_mpn_model* model, const mtmc_mpn_call* call, mtmc_mpn_plan* out);

/* out[dim_size, C] (fp32) <- scatter of src[E, C] by index[E] along dim 0; rows nobody writes are 0.
 * mean divides by max(count,1); max also writes arg_out[dim_size, C] (int64, E where untouched) if non-NULL. */
int32_t mtmc_scatter_add(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                         int64_t dim_size, float* out, void* stream);
/* the integer call form of the reference's post-processing, scatter_add(int64 [E], index, dim_size=N)
 * (reference utils.py:173-174, :308-309): int64 in, int64 out, exact */
int32_t mtmc_scatter_add_i64(const int64_t* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                             int64_t dim_size, int64_t* out, void* stream);
int32_t mtmc_scatter_mean(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                          int64_t dim_size, float* out, float* count_scratch, void* stream);
int32_t mtmc_scatter_max(const float* src, const int64_t* index, int64_t n_src, int64_t n_cols,
                         int64_t dim_size, float* out, int64_t* arg_out, void* stream);

/* The backward passes of the three float scatters with respect to src: grad_src[n_src, C] from grad_out[dim_size, C], r = index[e]:
 *   add : grad_src[e, c] = grad_out[r, c]
 *   mean: grad_src[e, c] = grad_out[r, c] / (float)max(count[r], 1), a true division; count[r] = the rows with index r inside
 *         [0, dim_size), as the forward counts them, recounted into count_scratch (int32 [dim_size]: one memset, one pass
 *         of integer atomics)
 *   max : grad_src[e, c] = grad_out[r, c] if arg[r, c] == e, else 0; arg [dim_size, C] is what the forward wrote to arg_out
 *         (the smallest e attaining the maximum; n_src where nobody wrote, so that gradient goes nowhere)
 * A row whose index lies outside [0, dim_size) gets zeros: the forward skips it.  Every element of grad_src is written
 * exactly once (no memset, no atomics on floats), so the result is the same bits on every run.  n_src == 0 or n_cols == 0:
 * success, nothing enqueued.  Rows of 16 bytes per lane when C % 4 == 0 and grad_out, grad_src (and arg) are 16-byte
 * aligned, one column per lane otherwise.  With dim_size == 0 grad_out, arg and count_scratch are not read and may be NULL. */
int32_t mtmc_scatter_add_backward(const float* grad_out, const int64_t* index, int64_t n_src, int64_t n_cols,
                                  int64_t dim_size, float* grad_src, void* stream);
int32_t mtmc_scatter_mean_backward(const float* grad_out, const int64_t* index, int64_t n_src, int64_t n_cols,
                                   int64_t dim_size, int32_t* count_scratch, float* grad_src, void* stream);
int32_t mtmc_scatter_max_backward(const float* grad_out, const int64_t* arg, const int64_t* index, int64_t n_src,
                                  int64_t n_cols, int64_t dim_size, float* grad_src, void* stream);

/* The repeatable forward of the three float scatters: a segmented reduction over a grouping of the rows (mtmc_group_by_index
 * below, or any perm / offsets pair of that form): out[g] reduces the rows perm[j], offsets[g] <= j < offsets[g + 1].
 * mode 0 add, 1 mean, 2 max (arg_out as above, may be NULL).  Semantics of the three entries above: rows behind
 * offsets[dim_size] count for nothing, a row nobody writes is 0, mean divides by (float)max(offsets[g + 1] - offsets[g], 1),
 * max compares as mtmc_scatter_max does and arg_out is the smallest source row of the maximum (n_src where none).
 * No fill launch, no float atomic, no count buffer: every output element has one writer, and every sum one order that is a
 * function of (n_src, n_cols, offsets) alone -- chunks of 64 positions, per chunk strided sub-row sums folded in a fixed
 * butterfly, chunk partials of a group that crosses chunks folded by the same rule in chunk order (csrc/scatter_ops.hip
 * writes it out) -- so the result has the same bits on every run, on every grid and however the grouping was made.  A
 * group of one row is a bit-exact copy of that row.  perm entries outside [0, n_src) name no row; offsets are clamped into
 * [0, n_src] before use.  16-byte loads when n_cols % 4 == 0 and src, out and workspace are 16-byte aligned (the order does
 * not depend on it).  Two launches (one when n_src == 0; none when dim_size == 0).  The size query is host-only and
 * returns 0 for sizes the entry refuses (n_src outside [0, 2^31), n_cols < 1). */
size_t mtmc_scatter_grouped_workspace_bytes(int64_t n_src, int64_t n_cols);
int32_t mtmc_scatter_grouped(const float* src, int64_t n_src, int64_t n_cols, const int64_t* perm, const int64_t* offsets,
                             int64_t dim_size, int32_t mode, float* out, int64_t* arg_out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* y[rows, out] = relu(batchnorm_batchstats(x[rows,in] . W^T + b)) for one Linear+BN+ReLU group
 * (gamma == NULL: bare Linear).  stats_scratch: f64[2*out], y_raw aliases y. */
int32_t mtmc_mlp_layer_forward(const mtmc_layer* layer, const float* x, int64_t x_row_stride, int64_t rows,
                               float* y, double* stats_scratch, void* stream);

/* Diagnostics / unit tests: Y[M][N] = A[M][K] . W[N][K]^T + bias through the node encoder's GEMM dispatch exactly as the
 * forward runs its first layer (operand scales gathered on the device, fp16 two-piece kernel where it applies);
 * K a multiple of 32.  scratch: u32[48]; stats: f64[2*N] column sum / sum of squares of Y, or NULL. */
int32_t mtmc_linear_raw(const float* A, int64_t lda, const float* W, const float* bias, float* Y, int64_t M, int32_t K,
                        int32_t N, uint32_t* scratch, double* stats, void* stream);

/* One encoder layer as the forward runs it on FEW-ROW graphs (csrc/gemm_few.hip): stats_in == NULL: layer 0,
 * Y = A . W^T + bias with both operands split into fp16 planes first (K a multiple of 64, <= 2048; N a multiple of 32);
 * else a later layer, Y = relu(bn(A)) . W^T + bias as in mtmc_linear_staged_raw (K a multiple of 32; N a multiple of 16).
 * work: >= 4*M*K + 4*N*K + 4*(M+N) + 1024 bytes; stats: f64[2*N] or NULL. */
int32_t mtmc_linear_few_raw(const float* A, int64_t lda, const double* stats_in, const float* gamma_in, const float* beta_in,
                            double count, const float* W, const float* bias, float* Y, int64_t M, int32_t K, int32_t N,
                            void* work, uint64_t work_bytes, double* stats, void* stream);

/* One encoder layer >= 1 as the forward runs it on many-row graphs (csrc/gemm_staged.hip: role-split kernel, N a multiple
 * of 256 or N = 128; csrc/gemm_rows.hip: row-streaming kernel for the narrow last layer, K = 128 and N = 32):
 * Y[M][N] = relu(bn(A))[M][K] . W[N][K]^T + bias, bn = BatchNorm1d with batch statistics given as stats_in = f64 column
 * sum[K] | sum of squares[K] over `count` rows, and gamma_in / beta_in [K] (reference models/mlp.py:14-27: the previous
 * group's BatchNorm + ReLU fused into this Linear).  K a multiple of 32 in [64, 2048].
 * work: >= 4*N*K + 4*N + 256 bytes; scratch: u32[48]; stats: f64[2*N] column sum / sum of squares of Y, or NULL. */
int32_t mtmc_linear_staged_raw(const float* A, int64_t lda, const double* stats_in, const float* gamma_in,
                               const float* beta_in, double count, const float* W, const float* bias, float* Y, int64_t M,
                               int32_t K, int32_t N, void* work, uint64_t work_bytes, uint32_t* scratch, double* stats,
                               void* stream);

/* The pre-split twin of mtmc_linear_raw (csrc/gemm_presplit.hip; what the forward runs for encoder layer 0 of graphs
 * with >= 4096 nodes): A and W are first split into fp16 pairs with one power-of-two scale per row, stored k-tile-major
 * (work: >= 4*M*K + 4*N*K + 4*(M+N) + 1024 bytes of device memory), then multiplied by a plain fp16 MFMA GEMM fed by
 * LDS-DMA.  K a multiple of 64, K <= 2048.  reuse_planes != 0: the planes a previous call left in `work` are multiplied
 * again (times the GEMM alone).  (The kernels this one was chosen against are not in this library: csrc/lab/.) */
int32_t mtmc_linear_presplit_raw(const float* A, int64_t lda, const float* W, const float* bias, float* Y, int64_t M,
                                 int32_t K, int32_t N, void* work, uint64_t work_bytes, uint32_t* scratch,
                                 double* stats, int32_t reuse_planes, void* stream);

/* ---- graph construction (SURVEY.md 8(f)-1,2; replaces reference inference.py:402-456 / train.py:316-342) ----
 * feats [N][F] raw per-tracklet features -> x_out [N][F] (column-normalised like F.normalize(dim=0) if l2norm),
 * edge_index_out [E][2] int64 (row, col) in the reference's order (per camera, ascending: nodes of the camera x nodes
 * outside it; its transpose view is the [2,E] tensor the callers pass on), edge_attr_out [E][2] =
 * [pairwise_distance, 1 - cosine_similarity], edge_labels_out [E] (1.0 iff node_labels match; NULL to skip).
 * The camera structure comes as small device arrays the host derives from the camera ids:
 *   in_list/in_off[n_cams+1]: nodes of camera c;  out_list/out_off[n_cams+1]: nodes not in c (ascending);
 *   block_off[n_cams+1]: first edge of camera c's block, block_off[n_cams] = E.
 * Uses one N x N Gram matrix on the matrix cores instead of per-edge 2048-d gathers; N <= 46000. */
size_t mtmc_graph_workspace_bytes(int64_t n_nodes, int32_t feat_dim);
int32_t mtmc_build_graph(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                         const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                         const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                         float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same construction thinned to a symmetric k-nearest list (the reference leaves the idea as a commented-out block
 * between its edge list and its attributes, inference.py:407-456): with key(i, j) = the cosine distance edge_attr[e][1]
 * that mtmc_build_graph writes for the directed edge (i, j), row i ranks its cross-camera nodes by (key, j) ascending,
 * top_i = the first min(k, n_out(i)) of them, and edge (i, j) is kept iff j is in top_i or i is in top_j -- a union, so
 * the list is symmetric by construction.  The kept edges come in the dense list's order and with the dense call's bits;
 * edge_pos_out [edge_capacity] int64 receives each kept edge's index in the dense list.  Arguments as mtmc_build_graph
 * (n_edges = the DENSE list's length, block_off[n_cams]), plus k >= 1, edge_capacity = the number of edges the four
 * edge outputs can hold (min(n_edges, 2 k n_nodes) always suffices) and n_kept_out = one int64 in device memory that
 * receives the number of kept edges E_k.  Status: n_kept_out[0] > edge_capacity reports a capacity error -- the outputs
 * then hold the first edge_capacity kept edges and nothing at or past edge_capacity was written.  Only the Gram matrix and
 * a bit matrix of n_nodes^2 / 8 bytes are N^2-sized: no dense-sized edge array is formed.  Nothing synchronises; the
 * result is bitwise repeatable for a given Gram matrix.  MTMC_E_ARG / MTMC_E_WORKSPACE as mtmc_build_graph, and for
 * k < 1, edge_capacity < 0 or a NULL n_kept_out.  The workspace query returns 0 outside 1 <= n_nodes <= 46000 or for
 * feat_dim < 32, and at least mtmc_graph_workspace_bytes otherwise. */
size_t mtmc_graph_knn_workspace_bytes(int64_t n_nodes, int32_t feat_dim);
int32_t mtmc_build_graph_knn(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                             const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                             const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                             float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                             int32_t k, int64_t edge_capacity, int64_t* edge_pos_out, int64_t* n_kept_out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The other thinning of that commented-out block, a temporal gate (inference.py:420-441), alone or before the k-nearest
 * rule: with start_frames [n_nodes] int64 in device memory (each tracklet's first frame; any int64, the difference does not overflow) and
 * max_gap >= 1, (i, j) is a candidate iff the two nodes are in different cameras and |start_i - start_j| < max_gap --
 * strict, the reference's comparison: equal starts pass, a difference of max_gap does not.  k == 0: the kept edges are
 * exactly the candidates.  k >= 1: row i ranks its CANDIDATES by (key, j) ascending, top_i = the first
 * min(k, candidates of i) of them, and (i, j) is kept iff j is in top_i or i is in top_j -- "gate, then k", which is not
 * the k list filtered afterwards.  A row without candidates has no edges; no candidates at all gives n_kept_out[0] = 0.
 * Order, bits, edge_pos_out, edge_capacity and the n_kept_out status as mtmc_build_graph_knn, whose body this shares
 * (the exact length of the gated list always suffices as capacity; with k, the smaller of it and 2 k n_nodes).  The
 * workspace is that of mtmc_graph_knn_workspace_bytes; its bit matrix goes unused when k == 0.  MTMC_E_ARG also for a
 * NULL start_frames, max_gap < 1 or k < 0. */
int32_t mtmc_build_graph_gated(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                               const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                               const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                               float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                               const int64_t* start_frames, int64_t max_gap, int32_t k,
                               int64_t edge_capacity, int64_t* edge_pos_out, int64_t* n_kept_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The two thinned lists without anything N^2-sized, for 1 <= n_nodes <= 262144: the rule, the order, the
 * bits, edge_pos_out, edge_capacity and the n_kept_out status of mtmc_build_graph_knn / mtmc_build_graph_gated, but the Gram
 * matrix is formed in row panels of P node rows ([P][n_nodes] fp32), twice -- once to pick every row's top, once to write
 * the kept edges -- and the picks live in per-row lists.  With the same input the outputs are those of the unpaneled entry
 * bit for bit at every P (a panel's product is planned as the whole product is).  start_frames may be NULL (no gate;
 * max_gap is then ignored); k >= 1 or a gate is needed, k == 0 with a gate keeps the candidates.  k above n_nodes counts
 * as n_nodes, and min(k, n_nodes) <= 4096.  panel_rows = P >= 1 (clipped to n_nodes), or 0: the library chooses.
 * mtmc_graph_panel_rows returns the P a call will use: min(panel_rows, n_nodes), and for 0 the largest multiple of 128 with
 * P * n_nodes * 4 <= 1 GiB, at least 128, clipped to n_nodes.  Workspace: P * n_nodes * 4 bytes for the panel, split times
 * as much again where the whole product's plan cuts K, 2 * n_nodes * min(k, n_nodes) * 4 for the picks and their
 * transpose, O(n_nodes + feat_dim) words besides.  Both queries return 0 outside 1 <= n_nodes <= 262144, for a feat_dim
 * that is no positive multiple of 32, min(k, n_nodes) > 4096, k < 0 or panel_rows < 0, and the entry refuses the same with
 * MTMC_E_ARG before anything is enqueued.  Nothing synchronises; the result is bitwise repeatable. */
int64_t mtmc_graph_panel_rows(int64_t n_nodes, int32_t feat_dim, int64_t panel_rows);
size_t mtmc_graph_paneled_workspace_bytes(int64_t n_nodes, int32_t feat_dim, int32_t k, int64_t panel_rows);
int32_t mtmc_build_graph_paneled(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                                 const int32_t* in_list, const int32_t* in_off, const int32_t* out_list, const int64_t* out_off,
                                 const int64_t* block_off, int32_t n_cams, int64_t n_edges, const int64_t* node_labels,
                                 float* x_out, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                                 const int64_t* start_frames, int64_t max_gap, int32_t k, int64_t panel_rows,
                                 int64_t edge_capacity, int64_t* edge_pos_out, int64_t* n_kept_out,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the construction to the node features (the reference's CNN_MODEL.finetune chain, train.py:304-342:
 * autograd through F.normalize(dim=0), F.pairwise_distance and 1 - F.cosine_similarity along the edge list).
 * feats, l2norm and the five camera tables as in the forward call (in_list per camera and out_list per camera
 * ascending, as graph_build.camera_tables writes them); x [N][F] and edge_attr [E][2] as the forward produced them;
 * d_x [N][F] and d_edge_attr [E][2]: incoming gradients, either may be NULL (= zero), both only when n_edges == 0;
 * d_feats_out [N][F] contiguous, distinct from x and d_x.  One dense product (M + M^T) . x on the fp32 matrix cores
 * with M [N][N] filled from 16 bytes per edge -- no [E][F] intermediate; workspace O(N^2 + N + F).  Everything is
 * enqueued on `stream`, nothing synchronises.  MTMC_E_ARG on null / misaligned pointers (16 bytes for the matrices,
 * 8 for the edge arrays, 256 for the workspace) or sizes outside the forward's, MTMC_E_WORKSPACE on a short workspace.
 * The workspace query returns 0 outside 1 <= n_nodes <= 46000 or for a feat_dim that is no multiple of 32. */
size_t mtmc_graph_backward_workspace_bytes(int64_t n_nodes, int32_t feat_dim);
int32_t mtmc_build_graph_backward(const float* feats, int64_t feat_row_stride, int64_t n_nodes, int32_t feat_dim, int32_t l2norm,
                                  const int32_t* in_list, const int32_t* in_off, const int32_t* out_list,
                                  const int64_t* out_off, const int64_t* block_off, int32_t n_cams, int64_t n_edges,
                                  const float* x, const float* edge_attr, const float* d_x, const float* d_edge_attr,
                                  float* d_feats_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the training callers' loss: F.cross_entropy / nn.CrossEntropyLoss(weight, reduction) on [n][n_classes<=4]
 * logits (reference train.py:88-93, :109-142, :178-186).  mode 0 = mean, 1 = sum, 2 = none.
 * forward: per_sample[i] = w[y_i] * (logsumexp(x_i) - x_i[y_i]) (NULL to skip); sums = f64[2*MTMC_STAT_REPLICAS]
 * scratch, on return sums[0] = sum_i per_sample[i], sums[1] = sum_i w[y_i]; loss_out[0] = sums[0]/sums[1] (mean) or
 * sums[0] (NULL to skip).  Rows with y_i == ignore_index count for nothing.
 * backward: d_logits[i][c] = g_i * w[y_i] * (softmax(x_i)[c] - [c == y_i]) with g_i = grad[0]/sums[1] (mean, needs the
 * forward's sums), grad[0] (sum) or grad[i] (none).  All pointers are device pointers. */
int32_t mtmc_cross_entropy_forward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                   int32_t n_classes, int64_t ignore_index, int32_t mode, float* per_sample,
                                   double* sums, float* loss_out, void* stream);
int32_t mtmc_cross_entropy_backward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                    int32_t n_classes, int64_t ignore_index, int32_t mode, const float* grad,
                                    const double* sums, float* d_logits, void* stream);

/* sum over the classified steps of cross_entropy(step, labels) in one pass (the training loop's loss, reference
 * train.py:118-138): logits = the contiguous [n_steps][n][n_classes] block of one forward, labels [n] shared by the steps.
 * mode 0 = mean per step, 1 = sum; sums as above (of all steps together); loss_out[0] = the summed loss.
 * backward: d_logits [n_steps][n][n_classes] for grad[0] = d loss. */
int32_t mtmc_cross_entropy_steps_forward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                         int32_t n_classes, int32_t n_steps, int64_t ignore_index, int32_t mode,
                                         double* sums, float* loss_out, void* stream);
int32_t mtmc_cross_entropy_steps_backward(const float* logits, const int64_t* labels, const float* weight, int64_t n,
                                          int32_t n_classes, int32_t n_steps, int64_t ignore_index, int32_t mode,
                                          const float* grad, const double* sums, float* d_logits, void* stream);

/* counts[4] (int64, device) = {TP, FP, TN, FN} of argmax(logits [n][n_classes]) against 0/1 labels [n], in one pass:
 * the confusion counts the training / validation loops compute with boolean-mask indexing (reference train.py:98-107,
 * inference.py:20-67).  Labels other than 0 / 1 are skipped; prediction = (argmax == 1), first maximum on ties. */
int32_t mtmc_edge_confusion(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int64_t* counts,
                            void* stream);

/* ---- loss and metrics of the training / validation loops in one pass: everything compute_loss_acc returns (reference
 * train.py:36-245) for every classified step, without a host read.  logits = the contiguous [n_steps][n][n_classes] block
 * of one forward, n_classes 1 (one logit x, the BCE / BCE_weighted losses) or 2 (CE / CE_weighted); labels [n] shared by
 * the steps; rows whose label is neither 0 nor 1 count for nothing anywhere.  n0 / n1 = the numbers of label-0 / label-1
 * rows.  With z = the margin of the true class (x[y] - x[1-y]; for one logit x if y = 1, -x if y = 0):
 *   row loss l = softplus(-z) (= logsumexp(x) - x[y], resp. the BCE-with-logits term), true-class probability = sigmoid(z);
 *   prediction = (argmax == 1), first maximum on ties, resp. x >= 0.
 * forward: one memset of `scratch`, ONE launch over all steps (fp64 sums L0 L1 P0 P1 and the integer counts TP FP TN FN
 * per step, in MTMC_STAT_REPLICAS replicas), one single-workgroup finalize that writes
 *   record [MTMC_EDGE_LOSS_RECORD] f64 : w0, w1, the denominator D, n0 + n1   (what the backward reads)
 *   out    [3 + 5*n_steps] f32         : loss | w0 w1 | class_loss [n_steps][2] | class_prob [n_steps][2] | fpr [n_steps]
 *   confusion [n_steps][4] int64       : TP, FP, TN, FN
 * weight_mode MTMC_EDGE_W_ONE: (w0, w1) = (1, 1); _GIVEN: weight[0..1] (n_classes 2) resp. (1, weight[0]) (one logit: the
 * pos_weight); _BALANCED: (1, n0/n1), the reference's w_0b/w_0b, w_1b/w_0b (train.py:127-130) -- (1, 1) if either class is
 * empty, where the reference divides by zero.
 *   loss = sum_s (w0 L0_s + w1 L1_s) / D + fpr_alpha * sum_s fpr_s,  D = w0 n0 + w1 n1 (n_classes 2: torch's weighted-mean
 *   cross entropy per step) resp. n0 + n1 (one logit: BCEWithLogitsLoss with pos_weight w1, reduction 'mean');
 *   fpr_s = FP_s / (FP_s + TN_s), 0 without label-0 rows (the reference's FPR term, train.py:194-195);
 *   class_loss = L_c / n_c (0 where the class is empty), class_prob = P_c / n_c (0.5 where empty: the reference's filler,
 *   train.py:378-385).  Without any counted row the loss is 0/0 = NaN, as in torch.
 * backward: one launch, d_logits [n_steps][n][n_classes] = grad[0] * w[y] / D * d l / d x (softmax(x) - onehot(y), resp.
 * (1-y) sigmoid(x) - y (1 - sigmoid(x))), 0 on skipped rows; w and D are read from `record` on the device.  The FPR term
 * has no gradient (none in the reference either).
 * All pointers are device pointers; nothing is allocated or synchronised.  MTMC_E_ARG: n_classes outside {1, 2},
 * n_steps < 1, n < 0, an unknown weight_mode, a NULL pointer (weight only with _GIVEN), a two-class block (logits,
 * d_logits) that is not 8-byte aligned, scratch_bytes short of the query's answer. */
enum { MTMC_EDGE_W_ONE = 0, MTMC_EDGE_W_GIVEN = 1, MTMC_EDGE_W_BALANCED = 2 };
#define MTMC_EDGE_LOSS_RECORD 4
size_t mtmc_edge_loss_scratch_bytes(int32_t n_steps);
int32_t mtmc_edge_loss_forward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                               int32_t weight_mode, const float* weight, float fpr_alpha, void* scratch,
                               size_t scratch_bytes, double* record, float* out, int64_t* confusion, void* stream);
int32_t mtmc_edge_loss_backward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                                const float* grad, const double* record, float* d_logits, void* stream);

/* ---- focal loss (Lin et al., "Focal Loss for Dense Object Detection") for both classifier forms: the fourth entry of
 * the reference's `loss_name: CE_weighted # CE_weighted Focal BCE_weighted BCE` (config/config_training.yaml:37), whose
 * callers (main_training.py:273-276, train.py:144-181) name a class that is commented out; only the one-logit
 * utils.FocalLoss_binary (utils.py:695-724) is live there.  Everything of mtmc_edge_loss_* holds (arguments, scratch size,
 * record and out layout, weights, D, FPR term, class_prob, confusion, refusals) with one change: with z, l, p = sigmoid(z),
 * q = 1 - p as above, the row loss is
 *   f = q^gamma * l,          loss = sum_s (w0 F0_s + w1 F1_s) / D + fpr_alpha * sum_s fpr_s,   class_loss = F_c / n_c
 *   d f / d z = -q^gamma * (gamma * p * l + q)
 * (F_c = the sum of f over the rows of class c; D as above, not modulated).  q^(gamma - 1) is never formed: the factored
 * gradient is finite for every gamma >= 0 at q = 0 (loss 0, gradient 0 there for gamma > 0) and is -q at gamma = 0, which
 * is mtmc_edge_loss_*.  On softmax outputs f = (1 - p_t)^gamma * CE; balance * f is FocalLoss_binary(reduction='none').
 * (FocalLoss_binary with reduction='mean' modulates the mean BCE, one scalar, not the rows: it is not reproduced.)
 * forward: per_row, if not NULL, receives [n_steps][n] f32 = w[y] * f (0 on skipped rows) from one more launch after the
 * finalize.  backward: grad_per_row == 0: grad[0] is the gradient of the loss, as above; != 0: grad [n_steps][n] is the
 * gradient of per_row, d_logits = grad[s][i] * w[y] * d f / d x (no division by D).
 * MTMC_E_ARG as mtmc_edge_loss_*, and for a gamma that is negative, NaN or infinite. */
int32_t mtmc_edge_focal_forward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                                int32_t weight_mode, const float* weight, float fpr_alpha, void* scratch,
                                size_t scratch_bytes, double* record, float* out, int64_t* confusion, float gamma,
                                float* per_row, void* stream);
int32_t mtmc_edge_focal_backward(const float* logits, const int64_t* labels, int64_t n, int32_t n_classes, int32_t n_steps,
                                 const float* grad, const double* record, float* d_logits, float gamma, int32_t grad_per_row,
                                 void* stream);

/* ---- post-processing of the last logits (replaces reference inference.py:475-489, post_processing
 * inference.py:70-169 and utils.py compute_SCC_and_Clusters :30-52, splitting :54-123, remove_edges_single_direction
 * :125-142, pruning :144-339) ----
 * logits [E][2] -> prob1 [E] = softmax(logits)[:,1] and predictions [E] = argmax (both written); then, per `flags`,
 * symmetric cut, flow pruning (at most num_cameras-1 active out-/in-edges per node), second cut, splitting of clusters
 * with more than num_cameras nodes; predictions is updated in place and id_pred [N] receives the cluster number of
 * every node in the reference's numbering (networkx SCC emission order, stably sorted by size, isolated nodes last).
 * logits == NULL: prob1 and predictions are INPUTS (reproduces a run from given probabilities exactly).
 * info [8] (int32, device): active edges in, active edges out, clusters, status (0 ok, 1 = more than max_active
 * active edges: predictions left at argmax, 2 = over-sized cluster without an active edge, 3 = splitting iteration cap
 * reached, 4 = an active edge named a node outside [0, n_nodes): clamped), splitting iterations,
 * component walks, pruning rounds, 100 MHz ticks spent in the walks.  max_active <= 0: size the workspace for E active edges.
 * row/col: int64 with element stride idx_stride, as in struct mtmc_mpn_call.  Nothing is synchronised or allocated. */
enum { MTMC_PP_CUTTING = 1, MTMC_PP_PRUNING = 2, MTMC_PP_SPLITTING = 4 };
size_t mtmc_postprocess_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t max_active);
int32_t mtmc_postprocess(const float* logits, const int64_t* row, const int64_t* col, int64_t idx_stride,
                         int64_t n_nodes, int64_t n_edges, int32_t num_cameras, int32_t flags, int64_t max_active,
                         float* prob1, int64_t* predictions, int64_t* id_pred, int32_t* info,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- how good a tracking result is (the input_test == 'gt' branch of reference inference.py:501-526) ----
 * mtmc_cluster_scores replaces the five scikit-learn calls on (ID_GT, ID_pred) at inference.py:509 and :516-519
 * (adjusted_rand_score, adjusted_mutual_info_score, homogeneity_score, completeness_score, v_measure_score), with
 * scikit-learn's definitions and special cases, natural logarithms, fp64 throughout.  labels_true / labels_pred: n int64
 * labels each, element strides stride_true / stride_pred >= 0; the values are arbitrary (negative, not compact, INT64_MIN
 * and INT64_MAX included) and are not modified.  With a_i / b_j the cluster sizes of either side and n_ij the cell counts:
 *   scores [MTMC_CLUSTER_SCORES] f64 : ARI, AMI, homogeneity, completeness, V-measure, H_true, H_pred, MI, EMI
 *   counts [MTMC_CLUSTER_COUNTS] i64 : R, C (clusters of either side), non-empty cells, then the pair confusion
 *       tp = sum n_ij^2 - n, fp = sum b_j^2 - sum n_ij^2, fn = sum a_i^2 - sum n_ij^2, tn = n (n - 1) - tp - fp - fn
 *       (ordered pairs of distinct nodes, scikit-learn's pair_confusion_matrix)
 *   ARI = 1 if fn == fp == 0, else 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)), products in 128 bits;
 *   MI is clamped at 0; homogeneity = 1 if H_true == 0 else MI / H_true, completeness likewise with H_pred, V their
 *   harmonic mean (0 if both are 0); AMI = 1 if R == C == 1, else (MI - EMI) / den, den = (H_true + H_pred) / 2 - EMI
 *   kept at least DBL_EPSILON away from 0 with its sign.  Identical partitions give exactly 1.0 everywhere.
 * Labels and cells are kept in open-addressing tables of O(n) slots (no R x C table), EMI is summed over pairs of distinct
 * cluster sizes; the sums are integer (fixed point), so the result does not depend on the order of the insertions.
 * The workspace (8-byte aligned) is the caller's: at most 256 n + 64 KiB bytes; the size query is host-only and returns 0
 * for n < 1 or n > 1 048 576, sizes the entry point refuses with MTMC_E_ARG, as it does a NULL pointer, a negative
 * stride and a workspace short of the query's answer.  One memset and five launches; nothing is allocated or synchronised.
 *
 * mtmc_edge_prf replaces compute_P_R_F (inference.py:23-68, called at :511) on the post-processed int64 predictions
 * (mtmc_edge_confusion takes logits): one pass over predictions [n_edges] and labels [n_edges] (element strides >= 0).
 *   counts [4] i64 : TP, FP, TN, FN; rows whose label or prediction is neither 0 nor 1 count for nothing
 *   out    [MTMC_EDGE_PRF] f64 : P = TP / (TP + FP), R = TP / (TP + FN), F = 2 P R / (P + R), each 0 on a zero denominator;
 *       then the reference's precision_class0 = 100 TN / (TN + FP) and precision_class1 = 100 TP / (TP + FN) (0 without
 *       a success of that class)
 * n_edges == 0 is legal (all zeros; the row pointers may be NULL then). */
#define MTMC_CLUSTER_SCORES 9
#define MTMC_CLUSTER_COUNTS 7
#define MTMC_EDGE_PRF 5
size_t mtmc_cluster_scores_workspace_bytes(int64_t n);
int32_t mtmc_cluster_scores(const int64_t* labels_true, int64_t stride_true, const int64_t* labels_pred, int64_t stride_pred,
                            int64_t n, double* scores, int64_t* counts, void* workspace, size_t workspace_bytes,
                            void* stream);
int32_t mtmc_edge_prf(const int64_t* predictions, int64_t stride_pred, const int64_t* labels, int64_t stride_labels,
                      int64_t n_edges, int64_t* counts, double* out, void* stream);

/* ---- from detections to node features: the mean of each tracklet's ReID embeddings ----
 * mtmc_pool_tracklets replaces the reference's Python loop with one torch.mean(bboxes_embeds, 0) per tracklet and the
 * torch.stack behind it (train.py:305-316), and the same mean taken once per tracklet at feature extraction
 * (libs/reid_feature_extraction.py:177-178); mtmc_pool_tracklets_backward is what autograd runs through that loop when the
 * CNN is fine-tuned (train.py:305-316 again, under loss.backward()).
 *   embeds  [n_rows][feat_dim] fp32, element stride row_stride between rows (a multiple of 4, >= feat_dim), 16-byte aligned
 *   offsets [n_tracklets + 1] int64 IN DEVICE MEMORY: tracklet s owns rows [offsets[s], offsets[s+1]); offsets[0] = 0,
 *           offsets[n_tracklets] = n_rows, strictly increasing
 *   out     [n_tracklets][feat_dim] fp32, contiguous, 16-byte aligned: out[s] = mean of the rows of s
 *   info    [MTMC_POOL_INFO] int32 in device memory (may be NULL): status, tracklets with a bad range, 0, 0.
 *           status 0 = ok; 1 = offsets not strictly increasing, or outside [0, n_rows]; 2 = offsets[0] != 0 or
 *           offsets[n_tracklets] != n_rows (the larger one if both).  The host never reads the offsets: every value is
 *           clamped into [0, n_rows] before it is used, an empty or inverted range gives a zero row, and with a nonzero
 *           status the other rows of out hold sums over the clamped ranges (unspecified where ranges overlap).
 * The rows are cut into chunks of mtmc_pool_chunk_rows() rows, one wave per chunk and 256 columns, so no wave's work grows
 * with the longest tracklet; a tracklet that crosses chunk boundaries is summed from per-chunk partial sums in chunk order.
 * No atomics on floats: the same bits on every run.  The partial sums live in the caller's workspace (16-byte aligned):
 * 2 * ceil(n_rows / chunk_rows) * feat_dim * 4 bytes, rounded up; the size query is host-only and returns 0 for sizes the
 * entry points refuse: feat_dim not a multiple of 4 or outside [4, 16384], n_rows < 0 or >= 2^31.
 * mtmc_pool_tracklets_backward: grad_out [n_tracklets][feat_dim] contiguous -> grad_embeds [n_rows][feat_dim] with element
 * stride grad_row_stride: grad_embeds[r] = grad_out[s] / (offsets[s+1] - offsets[s]) for every row r of s, each row written
 * exactly once (rows that no tracklet owns -- bad offsets only -- get zeros); needs no workspace.
 * n_tracklets == 0 or n_rows == 0: success, nothing is enqueued.  Everything else is enqueued on `stream`; nothing is
 * allocated or synchronised.  MTMC_E_ARG (with text) on bad sizes, NULL or misaligned pointers, a short workspace. */
#define MTMC_POOL_INFO 4
int32_t mtmc_pool_chunk_rows(void);
size_t mtmc_pool_tracklets_workspace_bytes(int64_t n_rows, int32_t feat_dim);
int32_t mtmc_pool_tracklets(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim,
                            const int64_t* offsets, int64_t n_tracklets, float* out, int32_t* info,
                            void* workspace, size_t workspace_bytes, void* stream);
int32_t mtmc_pool_tracklets_backward(const float* grad_out, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                                     int64_t n_tracklets, float* grad_embeds, int64_t grad_row_stride, void* stream);

/* ---- the same for detections in any order and with per-detection weights ----
 * out[s] = (sum_r w_r x_r) / (sum_r w_r) over the rows of tracklet s: box area, ROI and confidence filters
 * (libs/filter_mtmc.py) as a weight in the mean, and rows that arrive frame by frame instead of tracklet by tracklet.
 * The three entry points above keep their signatures and their kernels; these take two optional arrays in device memory:
 *   perm    [n_rows] int64 or NULL: position j of the grouped order holds detection row perm[j], and offsets cut the
 *           POSITIONS: tracklet s owns positions [offsets[s], offsets[s+1]).  NULL: position j is row j.  With perm,
 *           offsets[n_tracklets] may be less than n_rows (the positions behind it belong to no tracklet) and an empty
 *           range is legal.  Every row is to be named once; the sums run in position order.
 *   weights [n_rows] fp32 or NULL (all 1), indexed by the detection ROW: finite and >= 0.
 *   wsum    [n_tracklets] fp32, written by the forward: the denominators sum_r w_r, which the two backwards read.
 *   info    [MTMC_POOL_INFO] int32 (may be NULL), cleared by the first kernel as above:
 *           info[0] a set of bits: 1 = offsets decrease (without perm: do not strictly increase) or leave [0, n_rows];
 *                   2 = offsets[0] != 0, or without perm offsets[n_tracklets] != n_rows; 4 = a perm entry outside
 *                   [0, n_rows); 8 = a weight that is negative, infinite or NaN
 *           info[1] tracklets with a bad range (bits 1, 2)
 *           info[2] tracklets that got a zero row: an empty range, or weights that add up to 0 (wsum[s] = 0)
 *           info[3] positions that count for nothing: a perm entry outside [0, n_rows), or behind offsets[n_tracklets]
 *           Nothing read from device memory becomes an address unclamped: a bad perm entry names no row (weight 0, no
 *           gradient row written), a bad weight counts as 0.  A row with weight 0 adds nothing, whatever it holds.
 * The sums keep the decomposition above (chunks of mtmc_pool_chunk_rows() positions, head and tail partial sums added in
 * chunk order, fmaf(w, x, acc) per row; no atomics on floats), the weight sums beside the row sums: with every weight 1
 * the result has the bits of mtmc_pool_tracklets.  Workspace: the partial rows plus 3 words a chunk.
 * mtmc_pool_tracklets_weighted_backward: grad_embeds[perm[j]] = w * grad_out[s] / wsum[s] for every position j of s, zeros
 * for positions of no tracklet and where wsum[s] = 0; each named row is written exactly once.
 * mtmc_pool_tracklets_weight_grad: grad_weights[perm[j]] = grad_out[s] . (embeds[perm[j]] - out[s]) / wsum[s] (0 where the
 * backward writes zeros); embeds is read once, each dot product is summed in one fixed order.  out is the forward's result.
 * Sizes, alignment, the empty cases and the error codes are those of the entry points above. */
size_t mtmc_pool_tracklets_weighted_workspace_bytes(int64_t n_rows, int32_t feat_dim);
int32_t mtmc_pool_tracklets_weighted(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim,
                                     const int64_t* offsets, int64_t n_tracklets, const int64_t* perm, const float* weights,
                                     float* out, float* wsum, int32_t* info, void* workspace, size_t workspace_bytes,
                                     void* stream);
int32_t mtmc_pool_tracklets_weighted_backward(const float* grad_out, int64_t n_rows, int32_t feat_dim, const int64_t* offsets,
                                              int64_t n_tracklets, const int64_t* perm, const float* weights,
                                              const float* wsum, float* grad_embeds, int64_t grad_row_stride, void* stream);
int32_t mtmc_pool_tracklets_weight_grad(const float* embeds, int64_t row_stride, int64_t n_rows, int32_t feat_dim,
                                        const int64_t* offsets, int64_t n_tracklets, const int64_t* perm,
                                        const float* grad_out, const float* out, const float* wsum, float* grad_weights,
                                        void* stream);

/* ---- stable grouping of int64 keys: the perm / offsets pair of mtmc_pool_tracklets_weighted and mtmc_scatter_grouped ----
 * index [n_rows] int64 in device memory, n_groups a host int.  The key of row r is index[r] if it lies in [0, n_groups), else
 * n_groups.  perm [n_rows] int64 lists the rows by key, rows with equal keys in increasing row order (a stable sort: there
 * is one answer); offsets [n_groups + 1] int64: group g owns perm[offsets[g] : offsets[g + 1]], and the rows keyed n_groups
 * lie behind offsets[n_groups], in row order.  info (may be NULL): one int32, the number of rows keyed n_groups.
 * An LSD radix sort over ceil(bits(n_groups) / digit_bits) passes on tiles of mtmc_group_tile_rows() rows (per pass a
 * per-tile digit histogram, an exclusive scan over (digit, tile), and a placement whose ranks are computed with wave ballots
 * and prefixed in wave order, never drawn from an atomic); digit_bits = 0 lets the library choose, 1 .. 11 forces the width.
 * One pass when n_groups + 1 <= 2^digit_bits.  Nothing is read back, allocated or synchronised; nothing read from index
 * becomes an address unclamped.  n_rows == 0 or n_groups == 0: an all-zero offsets and perm in row order, one launch, no
 * workspace.  Limits: n_rows, n_groups < 2^31.  The size query is host-only and returns 0 for sizes the entry refuses. */
int32_t mtmc_group_tile_rows(void);
size_t mtmc_group_by_index_workspace_bytes(int64_t n_rows, int64_t n_groups, int32_t digit_bits);
int32_t mtmc_group_by_index(const int64_t* index, int64_t n_rows, int64_t n_groups, int32_t digit_bits, int64_t* perm,
                            int64_t* offsets, int32_t* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the score the reference reports: IDF1 / IDP / IDR of a tracking result (main.py:166-213, eval/eval.py::eval) ----
 * The definition is DESIGN.md 3.11.  Two tables of detections (ground truth, predictions), each already GROUPED by the
 * caller: rows stably sorted by ((camera, frame) group, identity), with per row
 *   boxes [n][4] fp64 = x, y, width, height; camera [n] int32 in [0, n_cameras); identity [n] int32 in [0, n_identities);
 *   group [n] int32, equal for the rows of one (camera, frame)
 * mtmc_id_filter (both tables; the ground truth takes step 1 only) writes which rows survive, in this order:
 *   1. border != 0: keep iff x_lo <= x + width / 2 <= x_hi and y_lo <= y + height <= y_hi          (main.py:171-204)
 *   2. roi != NULL, [n_planes][roi_height][roi_width] uint8, plane_of_camera [n_cameras] int32 (-1: none, no lookup): the
 *      corners x, x + width, y, y + height in fp64, truncated to int64; a row goes iff a corner column inside [0, roi_width)
 *      and a corner row inside [0, roi_height) meet a mask value < 255; a corner outside the mask is never looked up
 *   3. min_cameras > 0: an identity whose rows, after 1-2, come from fewer distinct cameras goes     (removeOutliersSingleCam)
 *   4. drop_repeats != 0: of the rows of one (group, identity) that are left, the first stays       (removeRepetition)
 *   stage [n] uint8: after steps 1-2; keep [n] uint8: after all four; cameras [n_identities] uint64: the camera bits of
 *   step 3; n_kept [1] int64: the rows kept.  All four in device memory, written by the call (one memset, two launches).
 * mtmc_id_overlap: C[o][h] = the number of (ground-truth row, prediction row) pairs of one group, both kept (gt_keep may be
 *   NULL: all), with identities o and h, whose boxes have 1 - I / U <= max_dist, I = iw ih, U = aw ah + bw bh - I in fp64
 *   without fused multiply-adds (U = 0: NaN, does not count).  gt_offsets / pred_offsets [n_groups + 1] int64 in device
 *   memory cut the two tables over the UNION of their group keys (either side of a group may be empty).  C is int32
 *   [n_obj][n_hyp] at the start of the workspace, cleared by the call; integer atomic adds, the same bits on every run.
 *   Lanes walk the linearised pair index (a prefix sum over the groups, kept in the workspace), so there is no limit on a
 *   group's size and no loop over groups on the host.  Every offset and identity is checked against its array before use.
 * mtmc_id_cells: the non-zero cells of C as (o, h, count) int32 triples in no particular order, at most max_cells of them
 *   written; n_cells [1] int64 in device memory gets their number (which may exceed max_cells: call again).
 * The three run on `stream`, allocate nothing and synchronise nothing.  MTMC_E_ARG (with text): n_obj * n_hyp above
 * MTMC_ID_MAX_CELLS, more than MTMC_ID_MAX_CAMERAS cameras, a row count >= 2^31, a NULL pointer, a workspace short of
 * mtmc_id_overlap_workspace_bytes (host-only; 0 for sizes that are refused).  Zero rows on either side are legal.
 * mtmc_id_assign is HOST-ONLY and touches no GPU: cells [n_cells][3] int32 in host memory (count 0 is ignored) ->
 *   idtp = the largest sum of C over one-to-one partial matchings of objects and hypotheses, match_of_obj [n_obj] = the
 *   hypothesis of each object in one such matching (-1: none; only pairs with C > 0 are reported).  The support graph of
 *   C is split into connected components (union-find) and each is solved exactly by shortest augmenting paths in integer
 *   arithmetic, O(n^3) of the component.  stats [3] (may be NULL): components, then the rows and columns of the component
 *   with the largest rows x columns (ties: more rows). */
#define MTMC_ID_MAX_CELLS 67108864
#define MTMC_ID_MAX_CAMERAS 64
int32_t mtmc_id_filter(const double* boxes, const int32_t* camera, const int32_t* identity, const int32_t* group, int64_t n_rows,
                       int64_t n_identities, int32_t n_cameras, int32_t border, double x_lo, double x_hi, double y_lo,
                       double y_hi, const uint8_t* roi, const int32_t* plane_of_camera, int32_t n_planes, int32_t roi_height,
                       int32_t roi_width, int32_t min_cameras, int32_t drop_repeats, uint8_t* stage, uint8_t* keep,
                       uint64_t* cameras, int64_t* n_kept, void* stream);
size_t mtmc_id_overlap_workspace_bytes(int64_t n_obj, int64_t n_hyp, int64_t n_groups);
int32_t mtmc_id_overlap(const double* gt_boxes, const int64_t* gt_offsets, const int32_t* gt_identity, const uint8_t* gt_keep,
                        int64_t n_gt, const double* pred_boxes, const int64_t* pred_offsets, const int32_t* pred_identity,
                        const uint8_t* pred_keep, int64_t n_pred, int64_t n_groups, int64_t n_obj, int64_t n_hyp,
                        double max_dist, void* workspace, size_t workspace_bytes, void* stream);
int32_t mtmc_id_cells(const void* workspace, int64_t n_obj, int64_t n_hyp, int32_t* cells, int64_t max_cells, int64_t* n_cells,
                      void* stream);
int32_t mtmc_id_assign(const int32_t* cells, int64_t n_cells, int64_t n_obj, int64_t n_hyp, int64_t* idtp, int32_t* match_of_obj,
                       int64_t* stats);

/* ---- the CLEAR MOT columns of the same result row: MOTA, MOTP, recall, precision, switches, ... (eval/eval.py:409-411) ----
 * The definition is DESIGN.md 3.12.  The tables are the GROUPED ones of mtmc_id_filter / mtmc_id_overlap above, with their
 * offsets and keep bytes; the groups are numbered in ascending (camera, frame).
 * mtmc_mot_pairs: every CANDIDATE, a (ground-truth row, prediction row) pair of one group, both kept (gt_keep may be NULL:
 *   all), with d = 1 - I / U <= max_dist -- the very test of mtmc_id_overlap, so a pair is listed exactly when it counts
 *   there.  pairs [max_pairs][3] int32 = (group, ground-truth row, prediction row) and dist [max_pairs] fp64 = d, both in
 *   device memory, filled behind the counter n_pairs [1] int64 (device memory, cleared by the call) in NO PARTICULAR ORDER:
 *   sort by (group, ground-truth row, prediction row), which is the order of (ground-truth row, prediction row) alone.
 *   n_pairs may exceed max_pairs: nothing is written past the list, call again with a larger one.  A lane counts the
 *   candidates among its pairs, one integer atomic add per wave reserves their slots, the lane writes them; there are no
 *   floating-point atomics: the sorted list is the same bits on every run.  The work split is
 *   mtmc_id_overlap's (a prefix sum over the groups in the workspace; no limit on a group's size); every offset and row is
 *   checked against its array before use.  Runs on `stream`, allocates nothing, synchronises nothing.  MTMC_E_ARG (with
 *   text): a row or group count >= 2^31, a NULL pointer, a workspace short of mtmc_mot_pairs_workspace_bytes (host-only;
 *   0 for sizes that are refused).  Zero rows on either side are legal.
 * mtmc_mot_walk is HOST-ONLY and touches no GPU: the sorted candidates and, per row of either grouped table, its group,
 *   its compact identity and its keep byte (NULL: all kept), for ground-truth rows also the position in the input (any
 *   strictly increasing numbering of the input order).  Ground-truth rows are sorted by (group, identity), prediction rows
 *   by group.  It visits the groups in ascending order and does what MOTAccumulator.update does with an infinite
 *   max_switch_time: first every identity keeps the prediction it was last matched to while the two are candidates (in
 *   input order), then the rows not taken are assigned -- the most pairs, among those the smallest fp64 sum of d, exactly,
 *   by shortest augmenting paths per connected component of the group's candidates (a group in which no row has two
 *   candidates needs no solver) -- a pair whose identity was last matched to another predicted identity being a SWITCH.
 *   counts [MTMC_MOT_COUNTS] int64 = matches, switches, misses, false positives, fragmentations, mostly tracked, partially
 *   tracked, mostly lost, unique objects, kept ground-truth rows, kept prediction rows, frames (groups with a kept row);
 *   dist_sum = the sum of d over matches and switches, added sequentially in the order of the ground-truth rows;
 *   match_of_row [n_gt] int32 = the prediction row of each ground-truth row, -1: a miss, -2: not kept; stats [3] (may be
 *   NULL) = the groups that needed the solver, then the rows and columns of the largest component solved (rows x columns,
 *   ties: more rows).  MTMC_E_ARG (with text): candidates not sorted or listed twice, a row outside its table, a pair
 *   across groups or of a row not kept, a NaN distance, rows not sorted, a predicted identity kept twice in one group. */
#define MTMC_MOT_COUNTS 12
size_t mtmc_mot_pairs_workspace_bytes(int64_t n_groups);
int32_t mtmc_mot_pairs(const double* gt_boxes, const int64_t* gt_offsets, const uint8_t* gt_keep, int64_t n_gt,
                       const double* pred_boxes, const int64_t* pred_offsets, const uint8_t* pred_keep, int64_t n_pred,
                       int64_t n_groups, double max_dist, int32_t* pairs, double* dist, int64_t max_pairs, int64_t* n_pairs,
                       void* workspace, size_t workspace_bytes, void* stream);
int32_t mtmc_mot_walk(const int32_t* pairs, const double* dist, int64_t n_pairs, const int32_t* gt_group,
                      const int32_t* gt_identity, const int64_t* gt_position, const uint8_t* gt_keep, int64_t n_gt,
                      const int32_t* pred_group, const int32_t* pred_identity, const uint8_t* pred_keep, int64_t n_pred,
                      int64_t n_groups, int64_t n_obj, int64_t n_hyp, int64_t* counts, double* dist_sum, int32_t* match_of_row,
                      int64_t* stats);

#ifdef __cplusplus
}
#endif
#endif /* MTMC_MPN_H */
