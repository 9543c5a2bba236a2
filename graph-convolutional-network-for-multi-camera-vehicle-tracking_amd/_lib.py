"""ctypes binding of the C ABI in include/mtmc_mpn.h (csrc/libmtmc_mpn.so, built for gfx950).

The library is built in-tree (`python -m mtmc_mpn.build`, or `__graft_entry__.build()`).  If it is
missing, loading fails loudly: there is no other implementation behind the module.
Everything here mirrors the header by hand; tests/test_abi_exports.py parses the header and compares the
constants and every entry of SIGNATURES with it.
"""
from __future__ import annotations

import ctypes as C
import os

ABI_VERSION = 6
MAX_ENC_LAYERS = 8
NODE_DIM, EDGE_DIM, MAX_CLASSES = 32, 4, 4
AGG = {"sum": 0, "mean": 1, "max": 2}

(PH_BEGIN, PH_EDGE_ENC, PH_NODE_ENC, PH_NODE_H0, PH_ROUND_PROJ, PH_ROUND_A, PH_ROUND_B, PH_ROUND_STAT,
 PH_ROUND_C, PH_END, PH_NODE_COMBINE) = range(11)

E_ARG, E_WORKSPACE, E_HIP, E_ROWS = -1, -2, -3, -4

_f32p = C.c_void_p


class Layer(C.Structure):
    _fields_ = [("weight", _f32p), ("bias", _f32p), ("gamma", _f32p), ("beta", _f32p),
                ("in_dim", C.c_int32), ("out_dim", C.c_int32)]


class Model(C.Structure):
    """mtmc_mpn_model.  struct_bytes (since ABI v5) is filled in on construction: the library refuses any other size."""
    _fields_ = [("struct_bytes", C.c_uint32), ("n_enc_layers", C.c_int32), ("enc_node", Layer * MAX_ENC_LAYERS), ("enc_edge", Layer * 2),
                ("upd_edge", Layer), ("upd_node", Layer), ("cls", Layer),
                ("agg", C.c_int32), ("num_enc_steps", C.c_int32), ("num_class_steps", C.c_int32),
                ("reattach_nodes", C.c_int32), ("reattach_edges", C.c_int32),
                ("dropout_enc", C.c_float), ("dropout_upd_edge", C.c_float), ("dropout_upd_node", C.c_float)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_bytes = C.sizeof(type(self))


class Call(C.Structure):
    """mtmc_mpn_call.  struct_bytes is filled in on construction, as in Model."""
    _fields_ = [("struct_bytes", C.c_uint32), ("x", C.c_void_p), ("x_row_stride", C.c_int64), ("row", C.c_void_p), ("col", C.c_void_p),
                ("idx_stride", C.c_int64), ("edge_attr", C.c_void_p), ("n_nodes", C.c_int64), ("n_edges", C.c_int64),
                ("n_edges_total", C.c_int64), ("node_lo", C.c_int64), ("node_hi", C.c_int64),
                ("logits", C.c_void_p), ("h_out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("training", C.c_int32), ("flags", C.c_int32),
                ("seed", C.c_uint64), ("stream", C.c_void_p), ("row_lo", C.c_int64), ("row_hi", C.c_int64),
                ("weight_cache", C.c_void_p), ("weight_cache_bytes", C.c_size_t)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_bytes = C.sizeof(type(self))


class WsLayout(C.Structure):
    _fields_ = [("total_bytes", C.c_size_t), ("zero_bytes", C.c_size_t), ("flags_off", C.c_size_t),
                ("stat_attr_off", C.c_size_t), ("stat_enc2_off", C.c_size_t), ("stat_enc_layer_off", C.c_size_t * MAX_ENC_LAYERS),
                ("stat_round_off", C.c_size_t), ("deg_off", C.c_size_t), ("seg_off", C.c_size_t),
                ("h0_off", C.c_size_t), ("h_acc_off", C.c_size_t * 2), ("deg_global_off", C.c_size_t),
                ("P_off", C.c_size_t)]


class Plan(C.Structure):
    """mtmc_mpn_plan: which kernels a call would run (host-only query)."""
    _fields_ = [("enc_kernel", C.c_int32 * MAX_ENC_LAYERS), ("enc_split_k", C.c_int32 * MAX_ENC_LAYERS),
                ("edges_per_thread", C.c_int32), ("lazy_edges", C.c_int32), ("pass_c", C.c_int32),
                ("avg_degree", C.c_double), ("pass_a_col_blocks", C.c_int32), ("layer0_panels", C.c_int32),
                ("enc2_passenger", C.c_int32), ("node_stat_folded", C.c_int32)]


(GEMM_GENERIC, GEMM_INLOOP_64, GEMM_INLOOP_128, GEMM_PRESPLIT_256, GEMM_STAGED_128, GEMM_ROWS_16, GEMM_FEW_L0,
 GEMM_FEW_WAVE) = range(8)
PASS_C_WALK, PASS_C_MFMA_SORTED, PASS_C_MFMA_ANY = range(3)

# statistics blocks (include/mtmc_mpn.h): replicas x stride doubles each
STAT_REPLICAS, ATTR_STRIDE, ENC2_STRIDE, Z1_STRIDE, M_STRIDE, Z2_STRIDE = 16, 16, 16, 16, 16, 64
ROUND_BLOCK = STAT_REPLICAS * (Z1_STRIDE + M_STRIDE + Z2_STRIDE)
F_DETERMINISTIC, F_GLOBAL_DEG, F_FORK, F_SEED_ON_DEVICE = 1, 4, 2, 16
EDGE_W_ONE, EDGE_W_GIVEN, EDGE_W_BALANCED = range(3)      # mtmc_edge_loss_forward: weight_mode
EDGE_LOSS_RECORD = 4
CLUSTER_SCORES, CLUSTER_COUNTS, EDGE_PRF = 9, 7, 5        # mtmc_cluster_scores: scores / counts; mtmc_edge_prf: out
CLUSTER_SCORES_MAX_N = 1048576
POOL_INFO = 4                                             # mtmc_pool_tracklets: info words
ID_MAX_CELLS, ID_MAX_CAMERAS = 1 << 26, 64                # mtmc_id_overlap: n_obj * n_hyp; mtmc_id_filter: cameras
MOT_COUNTS = 12                                           # mtmc_mot_walk: count words

# MTMC_MPN_LIB: another build of the same ABI (same-box A/B of two library versions, tools/lib_ab.sh); default: the in-tree build
LIB_PATH = os.environ.get("MTMC_MPN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmtmc_mpn.so")

# Every entry point of the header: name -> (return type, argument types), in the header's order.  A pointer to one of the
# structs above is typed as such; every other pointer (device or host memory, a stream) is a c_void_p.
_p, _i32, _i64, _sz, _u64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_uint64, C.c_float, C.c_double
_Layer, _Model, _Call, _WsLayout, _Plan = (C.POINTER(s) for s in (Layer, Model, Call, WsLayout, Plan))
_graph_head = [_p, _i64, _i64, _i32, _i32, _p, _p, _p, _p, _p, _i32, _i64]     # feats ... max_edges of the build_graph family
SIGNATURES = {
    "mtmc_mpn_abi_version": (_i32, []),
    "mtmc_mpn_last_error": (C.c_char_p, []),
    "mtmc_mpn_workspace_bytes": (_sz, [_Model, _i64, _i64]),
    "mtmc_mpn_weight_cache_bytes": (_sz, [_Model]),
    "mtmc_mpn_workspace_layout": (_i32, [_Model, _i64, _i64, _WsLayout]),
    "mtmc_mpn_forward": (_i32, [_Model, _Call]),
    "mtmc_mpn_train_workspace_bytes": (_sz, [_Model, _i64, _i64]),
    "mtmc_mpn_backward": (_i32, [_Model, _Call, _p, _p, _Model, _p, _p]),
    "mtmc_mpn_backward_steps": (_i32, [_Model, _Call, _p, _p, _Model, _p, _sz, _p, _p]),
    "mtmc_mpn_grad_layout": (_i64, [_Model, _p, _i32]),
    "mtmc_mpn_backward_flat": (_i32, [_Model, _Call, _p, _p, _p, _i64, _p, _p]),
    "mtmc_mpn_run_phase": (_i32, [_Model, _Call, _i32, _i32]),
    "mtmc_mpn_run_phases": (_i32, [_Model, _Call, _p, _i32]),
    "mtmc_mpn_plan_call": (_i32, [_Model, _Call, _Plan]),
    "mtmc_scatter_add": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "mtmc_scatter_add_i64": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "mtmc_scatter_mean": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "mtmc_scatter_max": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "mtmc_scatter_add_backward": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "mtmc_scatter_mean_backward": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "mtmc_scatter_max_backward": (_i32, [_p, _p, _p, _i64, _i64, _i64, _p, _p]),
    "mtmc_scatter_grouped_workspace_bytes": (_sz, [_i64, _i64]),
    "mtmc_scatter_grouped": (_i32, [_p, _i64, _i64, _p, _p, _i64, _i32, _p, _p, _p, _sz, _p]),
    "mtmc_mlp_layer_forward": (_i32, [_Layer, _p, _i64, _i64, _p, _p, _p]),
    "mtmc_linear_raw": (_i32, [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _p, _p, _p]),
    "mtmc_linear_few_raw": (_i32, [_p, _i64, _p, _p, _p, _f64, _p, _p, _p, _i64, _i32, _i32, _p, _u64, _p, _p]),
    "mtmc_linear_staged_raw": (_i32, [_p, _i64, _p, _p, _p, _f64, _p, _p, _p, _i64, _i32, _i32, _p, _u64, _p, _p, _p]),
    "mtmc_linear_presplit_raw": (_i32, [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _p, _u64, _p, _p, _i32, _p]),
    "mtmc_graph_workspace_bytes": (_sz, [_i64, _i32]),
    "mtmc_build_graph": (_i32, _graph_head + [_p, _p, _p, _p, _p, _p, _sz, _p]),
    "mtmc_graph_knn_workspace_bytes": (_sz, [_i64, _i32]),
    "mtmc_build_graph_knn": (_i32, _graph_head + [_p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _sz, _p]),
    "mtmc_build_graph_gated": (_i32, _graph_head + [_p, _p, _p, _p, _p, _p, _i64, _i32, _i64, _p, _p, _p, _sz, _p]),
    "mtmc_graph_panel_rows": (_i64, [_i64, _i32, _i64]),
    "mtmc_graph_paneled_workspace_bytes": (_sz, [_i64, _i32, _i32, _i64]),
    "mtmc_build_graph_paneled": (_i32, _graph_head + [_p, _p, _p, _p, _p, _p, _i64, _i32, _i64, _i64, _p, _p, _p, _sz, _p]),
    "mtmc_graph_backward_workspace_bytes": (_sz, [_i64, _i32]),
    "mtmc_build_graph_backward": (_i32, _graph_head + [_p, _p, _p, _p, _p, _p, _sz, _p]),
    "mtmc_cross_entropy_forward": (_i32, [_p, _p, _p, _i64, _i32, _i64, _i32, _p, _p, _p, _p]),
    "mtmc_cross_entropy_backward": (_i32, [_p, _p, _p, _i64, _i32, _i64, _i32, _p, _p, _p, _p]),
    "mtmc_cross_entropy_steps_forward": (_i32, [_p, _p, _p, _i64, _i32, _i32, _i64, _i32, _p, _p, _p]),
    "mtmc_cross_entropy_steps_backward": (_i32, [_p, _p, _p, _i64, _i32, _i32, _i64, _i32, _p, _p, _p, _p]),
    "mtmc_edge_confusion": (_i32, [_p, _p, _i64, _i32, _p, _p]),
    "mtmc_edge_loss_scratch_bytes": (_sz, [_i32]),
    "mtmc_edge_loss_forward": (_i32, [_p, _p, _i64, _i32, _i32, _i32, _p, _f32, _p, _sz, _p, _p, _p, _p]),
    "mtmc_edge_loss_backward": (_i32, [_p, _p, _i64, _i32, _i32, _p, _p, _p, _p]),
    "mtmc_edge_focal_forward": (_i32, [_p, _p, _i64, _i32, _i32, _i32, _p, _f32, _p, _sz, _p, _p, _p, _f32, _p, _p]),
    "mtmc_edge_focal_backward": (_i32, [_p, _p, _i64, _i32, _i32, _p, _p, _p, _f32, _i32, _p]),
    "mtmc_postprocess_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mtmc_postprocess": (_i32, [_p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "mtmc_cluster_scores_workspace_bytes": (_sz, [_i64]),
    "mtmc_cluster_scores": (_i32, [_p, _i64, _p, _i64, _i64, _p, _p, _p, _sz, _p]),
    "mtmc_edge_prf": (_i32, [_p, _i64, _p, _i64, _i64, _p, _p, _p]),
    "mtmc_pool_chunk_rows": (_i32, []),
    "mtmc_pool_tracklets_workspace_bytes": (_sz, [_i64, _i32]),
    "mtmc_pool_tracklets": (_i32, [_p, _i64, _i64, _i32, _p, _i64, _p, _p, _p, _sz, _p]),
    "mtmc_pool_tracklets_backward": (_i32, [_p, _i64, _i32, _p, _i64, _p, _i64, _p]),
    "mtmc_pool_tracklets_weighted_workspace_bytes": (_sz, [_i64, _i32]),
    "mtmc_pool_tracklets_weighted": (_i32, [_p, _i64, _i64, _i32, _p, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "mtmc_pool_tracklets_weighted_backward": (_i32, [_p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "mtmc_pool_tracklets_weight_grad": (_i32, [_p, _i64, _i64, _i32, _p, _i64, _p, _p, _p, _p, _p, _p]),
    "mtmc_group_tile_rows": (_i32, []),
    "mtmc_group_by_index_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "mtmc_group_by_index": (_i32, [_p, _i64, _i64, _i32, _p, _p, _p, _p, _sz, _p]),
    "mtmc_id_filter": (_i32, [_p, _p, _p, _p, _i64, _i64, _i32, _i32, _f64, _f64, _f64, _f64, _p, _p, _i32, _i32, _i32, _i32, _i32,
                              _p, _p, _p, _p, _p]),
    "mtmc_id_overlap_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mtmc_id_overlap": (_i32, [_p, _p, _p, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _f64, _p, _sz, _p]),
    "mtmc_id_cells": (_i32, [_p, _i64, _i64, _p, _i64, _p, _p]),
    "mtmc_id_assign": (_i32, [_p, _i64, _i64, _i64, _p, _p, _p]),
    "mtmc_mot_pairs_workspace_bytes": (_sz, [_i64]),
    "mtmc_mot_pairs": (_i32, [_p, _p, _p, _i64, _p, _p, _p, _i64, _i64, _f64, _p, _p, _i64, _p, _p, _sz, _p]),
    "mtmc_mot_walk": (_i32, [_p, _p, _i64, _p, _p, _p, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def load() -> C.CDLL:
    """dlopen the HIP library (after torch, so both share torch's libamdhip64) and type its entry points."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"mtmc_mpn: HIP extension not built ({LIB_PATH} missing); run `python -m mtmc_mpn.build` "
                           "-- there is no fallback implementation")
    import torch  # noqa: F401  (loads the ROCm runtime the library links against)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.mtmc_mpn_abi_version() != ABI_VERSION:
        raise RuntimeError("mtmc_mpn: ABI version mismatch between _lib.py and libmtmc_mpn.so")
    _lib = lib
    return lib


def check(rc: int):
    """Map a negative return code to the exception the reference's path would raise."""
    if rc == 0:
        return
    msg = load().mtmc_mpn_last_error().decode()
    if rc == E_ROWS:
        raise ValueError(msg)
    raise RuntimeError(f"mtmc_mpn: {msg} (code {rc})")
