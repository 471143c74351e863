"""ctypes binding of libstdadk.so (C ABI: include/stdadk.h).

The library is the product: there is NO CPU fallback.  If the shared object is missing, or a
tensor is not a contiguous fp32 tensor on a HIP device, the call raises — loudly.
torch is used here only for device memory and the current HIP stream.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STDADK_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libstdadk.so"))

MAX_HIDDEN = 8
BASIS_KIND = {"wendland": 0, "gaussian": 1, "triangular": 2}


class NativeLibraryError(RuntimeError):
    pass


class MlpDesc(C.Structure):
    _fields_ = [("n_hidden", C.c_int32), ("in_dim", C.c_int32), ("hidden", C.c_int32 * MAX_HIDDEN),
                ("out_dim", C.c_int32), ("layernorm", C.c_int32), ("ln_eps", C.c_float),
                ("dropout_p", C.c_float)]


class MlpTensors(C.Structure):
    _fields_ = [("W", C.c_void_p * (MAX_HIDDEN + 1)), ("b", C.c_void_p * (MAX_HIDDEN + 1)),
                ("ln_g", C.c_void_p * MAX_HIDDEN), ("ln_b", C.c_void_p * MAX_HIDDEN),
                ("W_bf16", C.c_void_p * (MAX_HIDDEN + 1)), ("WT_bf16", C.c_void_p * (MAX_HIDDEN + 1))]


class BF16Region(C.Structure):
    _fields_ = [("off", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("dst", C.c_void_p),
                ("dst_t", C.c_void_p)]


class BF16Shadow(C.Structure):
    _fields_ = [("n", C.c_int32), ("r", BF16Region * MAX_HIDDEN)]


class BasisDesc(C.Structure):
    _fields_ = [("p", C.c_int32), ("basis", C.c_int32), ("n_levels", C.c_int32),
                ("side", C.c_int32 * 8), ("Ks", C.c_int64), ("Kt", C.c_int64),
                ("s_centers", C.c_void_p), ("s_bw", C.c_void_p), ("t_centers", C.c_void_p),
                ("t_bw", C.c_void_p)]


ABI_VERSION = 10           # STDADK_ABI_VERSION of include/stdadk.h this binding was written against
MAX_Q = 8
LOSS_MSE, LOSS_PINBALL = 0, 1


class LossDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("y_cols", C.c_int32), ("tau", C.c_float * MAX_Q),
                ("nc_weight", C.c_float), ("nc_power", C.c_int32)]


GRADSQ_PARTS = 512


class OptimDesc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p),
                ("n", C.c_int64), ("lr", C.c_float), ("lr_dev", C.c_void_p), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("step_dev", C.c_void_p),
                ("max_norm", C.c_float), ("sumsq_parts", C.c_void_p), ("ema_decay", C.c_float),
                ("shadow", C.POINTER(BF16Shadow)), ("nonfinite_step", C.c_void_p)]


class AdamGroup(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p),
                ("n", C.c_int64), ("lr", C.c_float), ("lr_dev", C.c_void_p), ("max_norm", C.c_float),
                ("sumsq_parts", C.c_void_p), ("n_parts", C.c_int32), ("shadow", C.POINTER(BF16Shadow))]


SPARSITY_KINDS = {"none": 0, "element": 1, "group": 2, "sparse_group": 3}


class SparsityDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lambda_l1", C.c_float), ("lambda_group", C.c_float),
                ("apply_spatial", C.c_int32), ("apply_temporal", C.c_int32)]


class KnotTrain(C.Structure):
    _fields_ = [("centers_init", C.c_void_p), ("gradient_damping", C.c_int32),
                ("damping_threshold", C.c_float), ("damping_strength", C.c_float),
                ("domain_weight", C.c_float), ("movement_weight", C.c_float),
                ("penalty_grad_scale", C.c_float), ("penalty_loss_scale", C.c_float)]


class DeltaStep(C.Structure):
    """stdadk_delta_step: the head of the one-call delta step (stdadk_train_step_delta_f32)."""
    _fields_ = [("delta", C.c_void_p), ("ldd", C.c_int64), ("d_delta", C.c_void_p), ("ldg", C.c_int64),
                ("lambda_grad", C.c_float), ("lambda_loss", C.c_float)]


FLAG_DENSE = 1
FLAG_W0_T = 2
FLAG_LOG_BW = 4
FLAG_WINDOW = 8
FLAG_PREBINNED = 16
FLAG_BF16 = 32
FLAG_SCATTERED = 64
FLAG_PACK_F32 = 128        # fragment-order fp32 copies of the hidden weights in the W_bf16 / WT_bf16 slots
KNOT_CELLS = 32          # cells per axis of the knot cell lists (csrc/window.h)

_lib = None

_SIGNATURES = {
    "stdadk_abi_version": (C.c_int, []),
    "stdadk_last_error": (C.c_char_p, []),
    "stdadk_rbf_build_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_void_p]),
    "stdadk_mlp_workspace_bytes": (C.c_size_t, [C.POINTER(MlpDesc), C.c_int64]),
    "stdadk_mlp_forward_f32": (C.c_int, [C.POINTER(MlpDesc), C.POINTER(MlpTensors), C.c_void_p,
                                         C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_int32, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p]),
    "stdadk_mlp_backward_f32": (C.c_int, [C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                          C.POINTER(MlpTensors), C.c_void_p, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                                          C.POINTER(C.c_void_p), C.c_void_p]),
    "stdadk_mse_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "stdadk_loss_f32": (C.c_int, [C.POINTER(LossDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_delta_head_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "stdadk_delta_head_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.c_int32, C.c_int32, C.c_float, C.c_float,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_sparsity_f32": (C.c_int, [C.POINTER(SparsityDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_spatial_partial_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                             C.c_void_p]),
    "stdadk_temporal_partial_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "stdadk_forward_parts_f32": (C.c_int, [C.POINTER(MlpDesc), C.POINTER(MlpTensors), C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "stdadk_forward_parts_supported": (C.c_int32, [C.POINTER(MlpDesc)]),
    "stdadk_train_step_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                        C.POINTER(MlpTensors), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_float, C.POINTER(LossDesc),
                                        C.POINTER(SparsityDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                                        C.c_int32, C.POINTER(OptimDesc), C.c_void_p]),
    "stdadk_train_step_next_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                             C.POINTER(MlpTensors), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int64, C.c_float, C.POINTER(LossDesc),
                                             C.POINTER(SparsityDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                                             C.c_int32, C.POINTER(OptimDesc), C.c_void_p, C.c_int64, C.c_int32,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.c_void_p]),
    "stdadk_train_step_knots_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                              C.POINTER(MlpTensors), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int64, C.c_float, C.POINTER(LossDesc),
                                              C.POINTER(SparsityDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                                              C.c_int32, C.POINTER(OptimDesc), C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(KnotTrain),
                                              C.c_void_p, C.c_void_p, C.POINTER(AdamGroup), C.c_void_p]),
    "stdadk_train_step_delta_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                              C.POINTER(MlpTensors), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int64, C.c_float, C.POINTER(LossDesc),
                                              C.POINTER(SparsityDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                                              C.c_int32, C.POINTER(OptimDesc), C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(KnotTrain),
                                              C.c_void_p, C.c_void_p, C.POINTER(AdamGroup), C.POINTER(DeltaStep),
                                              C.c_void_p]),
    "stdadk_sumsq2_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "stdadk_adamw_ema2_f32": (C.c_int, [C.POINTER(AdamGroup), C.POINTER(AdamGroup), C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_float, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_step_uses_window": (C.c_int32, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.c_int32]),
    "stdadk_step_workspace_bytes": (C.c_size_t, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.c_int64,
                                                 C.c_int32]),
    "stdadk_forward_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64, C.c_void_p,
                                     C.c_int32, C.c_void_p]),
    "stdadk_backward_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                      C.POINTER(MlpTensors), C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p]),
    "stdadk_knot_backward_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int32,
                                           C.POINTER(KnotTrain), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "stdadk_knot_grad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "stdadk_knot_grad_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "stdadk_train_fwd_bwd_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc),
                                           C.POINTER(MlpTensors), C.POINTER(MlpTensors), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                           C.POINTER(LossDesc),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "stdadk_train_fwd_bwd_indexed_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc),
                                                   C.POINTER(MlpTensors), C.POINTER(MlpTensors), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                   C.c_float, C.POINTER(LossDesc), C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_int32,
                                                   C.c_void_p, C.c_void_p]),
    "stdadk_eval_workspace_bytes": (C.c_size_t, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.c_int64, C.c_int32]),
    "stdadk_eval_indexed_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.POINTER(MlpTensors),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.POINTER(LossDesc), C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    "stdadk_grid_score_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "stdadk_grid_score_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_quantile_diag_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "stdadk_quantile_diag_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                           C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_variogram_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "stdadk_variogram_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_int64, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "stdadk_basis_diag_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "stdadk_basis_diag_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_int32,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_group_norms_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_void_p]),
    "stdadk_conformal_scores_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "stdadk_conformal_scores_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                              C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p]),
    "stdadk_select_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "stdadk_select_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_knn_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "stdadk_knn_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_knn_apply_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_knn_cells_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "stdadk_knn_cells_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_krige_weights_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "stdadk_krige_apply_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_int32, C.c_void_p,
                                         C.c_int64, C.c_void_p]),
    "stdadk_gmm_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "stdadk_gmm_em_f64": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "stdadk_kmeans_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "stdadk_kmeans_balanced_iter_f64": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p]),
    "stdadk_kmeanspp_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "stdadk_kmeanspp_f64": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_bin_batch_f32": (C.c_int, [C.POINTER(BasisDesc), C.POINTER(MlpDesc), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_size_t, C.c_int32, C.c_void_p]),
    "stdadk_gather_batch_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_bin_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "stdadk_bin_obs_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_knot_windows_i32": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_profile_enable": (C.c_int, [C.c_int32]),
    "stdadk_profile_collect": (C.c_int64, [C.c_char_p, C.c_int64]),
    "stdadk_gemm_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "stdadk_gemm_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "stdadk_sumsq_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_step_advance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "stdadk_adamw_ema_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_float, C.c_void_p, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_float,
                                       C.c_void_p, C.c_int32, C.c_float, C.c_float, C.POINTER(BF16Shadow),
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "stdadk_bf16_shadow_refresh": (C.c_int, [C.c_void_p, C.POINTER(BF16Shadow), C.c_void_p]),
    "stdadk_f32_pack_refresh": (C.c_int, [C.c_void_p, C.POINTER(BF16Shadow), C.c_void_p]),
}


def lib():
    """Load libstdadk.so once; raise NativeLibraryError (never fall back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"libstdadk.so not found at {LIB_PATH}: build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'` (st-dadk_amd/csrc/build.sh). "
                f"This package has no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            if name in _OWN_UNIT and not hasattr(handle, name):
                continue                    # (calling it raises AttributeError: there is no fallback)
            fn = getattr(handle, name)      # AttributeError => the .so is stale
            fn.restype, fn.argtypes = res, args
        if handle.stdadk_abi_version() != ABI_VERSION:
            raise NativeLibraryError("libstdadk.so ABI version mismatch")
        _lib = handle
    return _lib


# The entry points of csrc/conformal.hip, csrc/knn.hip, csrc/knn_cells.hip and csrc/krige.hip.  A library linked without those translation units still
# loads -- the host sanitizer build (tools/build_asan.sh) names its translation units itself and lists none of them -- and a
# call of one of these then raises AttributeError.
_OWN_UNIT = frozenset(("stdadk_conformal_scores_workspace_bytes", "stdadk_conformal_scores_f32",
                       "stdadk_select_workspace_bytes", "stdadk_select_f32",
                       "stdadk_knn_workspace_bytes", "stdadk_knn_f32", "stdadk_knn_apply_f32",
                       "stdadk_knn_cells_workspace_bytes", "stdadk_knn_cells_f32",
                       "stdadk_krige_weights_f64", "stdadk_krige_apply_f32"))


def exported_symbols():
    return list(_SIGNATURES)


def _check(rc, what):
    if rc != 0:
        msg = lib().stdadk_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def dry_run():
    """STDADK_DRY_RUN=1 (read by the library when it is loaded): every entry point validates and plans but launches
    NOTHING -- the hook of the host-side sanitizer pass (tools/build_asan.sh, tests/test_host_sanitizer.py), which runs
    without a GPU.  Host tensors are then accepted as stand-ins for device buffers (the host never dereferences
    them); whatever comes out is meaningless.  Not a CPU path: without the variable host tensors raise.  With
    profile_enable() on, profile_collect() still lists the names of the launches a call would make, at 0 ms each."""
    return _DRY_RUN


# read once, as the library does (api.cpp reads it when it is loaded): a lookup in os.environ per tensor argument was
# a fifth of the host time of a learnable-knot step (38 tensors per step)
_DRY_RUN = os.environ.get("STDADK_DRY_RUN", "") == "1"


def _on_device(tensor):
    return tensor.is_cuda or _DRY_RUN


def _dev(tensor, name, cur=None):
    """Validate a device tensor and return its address (`cur`: the current device, when the caller has asked)."""
    if tensor is None:
        return None
    if _DRY_RUN and not tensor.is_cuda:
        if not tensor.is_contiguous():
            raise RuntimeError(f"{name}: tensor must be contiguous")
        return tensor.data_ptr()
    if not tensor.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on a HIP device (cuda:N), got {tensor.device}; "
                           f"the MI355X build of stnf has no CPU path")
    if tensor.dtype not in (torch.float32, torch.uint8, torch.int32, torch.bfloat16):
        raise RuntimeError(f"{name}: unsupported dtype {tensor.dtype}")
    if not tensor.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")
    if tensor.get_device() != (_current_device() if cur is None else cur):
        # the launch stream is the CURRENT device's current stream (_stream below)
        raise RuntimeError(f"{name}: tensor lives on {tensor.device} but the current device is cuda:"
                           f"{torch.cuda.current_device()}; call under torch.cuda.device({tensor.device.index})")
    return tensor.data_ptr()


# the raw accessors of torch (a tensor on a HIP device exists, so the runtime is initialised): current_device() and
# current_stream() go through lazy initialisation checks and build a Stream object per call -- per tensor argument
# and per native call that is tens of microseconds of a 0.11 ms step
_current_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(cur=None):
    """The current HIP stream of the current device (every tensor of a call is checked to live there); `cur`: that
    device, when the caller has asked already."""
    if _DRY_RUN and not torch.cuda.is_available():
        return None
    if _raw_stream is not None:
        return _raw_stream(_current_device() if cur is None else cur)
    return torch.cuda.current_stream().cuda_stream


def _ref(x):
    """byref of an optional descriptor."""
    return C.byref(x) if x is not None else None


def _ws(t):
    """Address and size in bytes of a workspace tensor."""
    return t.data_ptr(), t.numel() * t.element_size()


def _contig(idx):
    """`idx` itself when it is contiguous, else a contiguous copy (the library reads index tensors as plain arrays)."""
    return idx if idx.is_contiguous() else idx.contiguous()


def _idx(t, what):
    """Address and count of an index tensor (`what` names it in the error)."""
    if t.dtype != torch.int64 or not (t.is_cuda or _DRY_RUN) or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous int64 tensor on the device")
    return t.data_ptr(), t.numel()


def _typed(what, tensor, name, dtype, shape):
    """Address of a contiguous tensor of `dtype` and `shape` (None: any) on the current HIP device, for the wrappers of
    the float64 side kernels; `what` names the calling wrapper in the error."""
    if tensor.dtype != dtype or not _on_device(tensor) or not tensor.is_contiguous() \
            or (shape is not None and tuple(tensor.shape) != shape):
        of_shape = "" if shape is None else f" of shape {shape}"
        raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} tensor{of_shape} on the device, got "
                           f"{tensor.dtype} {tuple(tensor.shape)} on {tensor.device}")
    if tensor.is_cuda and tensor.device.index != _current_device():
        raise RuntimeError(f"{what}: {name} lives on {tensor.device} but the current device is cuda:"
                           f"{torch.cuda.current_device()}; call under torch.cuda.device({tensor.device.index})")
    return tensor.data_ptr()


def _workspace_bytes(symbol, why, *args):
    """What the library's `symbol` answers for `args`; 0 means that it refuses them, `why` says what it accepts."""
    n = getattr(lib(), symbol)(*args)
    if n == 0:
        raise RuntimeError(f"{symbol}: {why}")
    return n


# --------------------------------------------------------------------------------------------
def rbf_build(coords, t, X, s_centers, s_bw, basis, t_centers, t_bw, out):
    """out[b,:] = [X | phi | psi]; `out` is (B, ld) fp32 with ld >= p+Ks+Kt.  Any of the three
    column groups may be absent (X None/p==0, s_centers None, t_centers None)."""
    B = out.shape[0]
    ld = out.stride(0) if out.dim() == 2 else 0
    if out.dim() != 2 or out.stride(1) != 1:
        raise RuntimeError("rbf_build: out must be 2-D with unit column stride")
    p = 0 if X is None or X.numel() == 0 else X.shape[1]
    Ks = 0 if s_centers is None else s_centers.shape[0]
    Kt = 0 if t_centers is None else t_centers.shape[0]
    if Ks and (coords.shape[0] != B or coords.shape[1] != 2):
        raise RuntimeError(f"rbf_build: coords must be ({B}, 2), got {tuple(coords.shape)}")
    if Kt and t.numel() != B:
        raise RuntimeError(f"rbf_build: t must have {B} elements, got {t.numel()}")
    if p and X.shape[0] != B:
        raise RuntimeError("rbf_build: X row count mismatch")
    if not _on_device(out):
        raise RuntimeError("rbf_build: expected tensors on a HIP device; this build has no CPU path")
    rc = lib().stdadk_rbf_build_f32(
        _dev(coords, "coords") if Ks else None, _dev(t, "t") if Kt else None,
        _dev(X, "X") if p else None, B, p,
        _dev(s_centers, "s_centers") if Ks else None, _dev(s_bw, "s_bw") if Ks else None, Ks,
        BASIS_KIND[basis], _dev(t_centers, "t_centers") if Kt else None,
        _dev(t_bw, "t_bw") if Kt else None, Kt, out.data_ptr(), ld, _stream())
    _check(rc, "stdadk_rbf_build_f32")
    return out


def make_desc(in_dim, hidden, out_dim, layernorm, dropout_p, ln_eps=1e-5):
    if len(hidden) > MAX_HIDDEN:
        raise RuntimeError(f"at most {MAX_HIDDEN} hidden layers are supported")
    d = MlpDesc()
    d.n_hidden, d.in_dim, d.out_dim = len(hidden), in_dim, out_dim
    for i, h in enumerate(hidden):
        d.hidden[i] = h
    d.layernorm, d.ln_eps, d.dropout_p = int(bool(layernorm)), ln_eps, float(dropout_p)
    return d


def make_tensors(Ws, bs, gs, betas, bf16=None, packed=None):
    """Pack per-layer tensors (lists; gs/betas may be None) into the ABI struct.  `bf16`: per Linear index
    None or the pair (W_bf16 (out,in), WT_bf16 (in,out)) of torch.bfloat16 operand copies (FLAG_BF16).  `packed`
    (instead): per Linear index None or the pair (PF, PB) of float32 fragment-order copies (FLAG_PACK_F32), which
    travel in the same slots."""
    s = MlpTensors()
    for i, (w, b) in enumerate(zip(Ws, bs)):
        s.W[i], s.b[i] = _dev(w, f"W[{i}]"), _dev(b, f"b[{i}]")
    if gs is not None:
        for i, (g, be) in enumerate(zip(gs, betas)):
            s.ln_g[i], s.ln_b[i] = _dev(g, f"ln_g[{i}]"), _dev(be, f"ln_b[{i}]")
    if bf16 is not None:
        for i, pair in enumerate(bf16):
            if pair is not None:
                if pair[0].dtype != torch.bfloat16 or pair[1].dtype != torch.bfloat16:
                    raise RuntimeError("make_tensors: the operand copies must be torch.bfloat16")
                s.W_bf16[i], s.WT_bf16[i] = _dev(pair[0], f"W_bf16[{i}]"), _dev(pair[1], f"WT_bf16[{i}]")
    if packed is not None:
        if bf16 is not None:
            raise RuntimeError("make_tensors: bf16 operand copies and packed fp32 copies share their slots")
        for i, pair in enumerate(packed):
            if pair is not None:
                if pair[0].dtype != torch.float32 or pair[1].dtype != torch.float32:
                    raise RuntimeError("make_tensors: the packed copies must be torch.float32")
                s.W_bf16[i], s.WT_bf16[i] = _dev(pair[0], f"PF[{i}]"), _dev(pair[1], f"PB[{i}]")
    return s


def make_bf16_shadow(regions):
    """stdadk_bf16_shadow from [(element offset into the flat fp32 buffer, rows, cols, dst, dst_t)]."""
    if len(regions) > MAX_HIDDEN:
        raise RuntimeError(f"at most {MAX_HIDDEN} bf16 shadow regions")
    sh = BF16Shadow()
    sh.n = len(regions)
    for i, (off, rows, cols, dst, dst_t) in enumerate(regions):
        sh.r[i].off, sh.r[i].rows, sh.r[i].cols = int(off), int(rows), int(cols)
        sh.r[i].dst, sh.r[i].dst_t = _dev(dst, "shadow dst"), _dev(dst_t, "shadow dst_t")
    return sh


def bf16_shadow_refresh(p, shadow):
    """Rewrite every region's bf16 copies from the fp32 buffer `p` (stdadk_bf16_shadow_refresh)."""
    rc = lib().stdadk_bf16_shadow_refresh(_dev(p, "p"), C.byref(shadow), _stream())
    _check(rc, "stdadk_bf16_shadow_refresh")


def pack_f32_sizes(rows, cols):
    """Floats of the packed forward / backward copy (PF, PB of stdadk.h) of a (rows, cols) weight."""
    return 32 * rows * ((cols + 31) // 32), 32 * cols * ((rows + 31) // 32)


def f32_pack_refresh(p, table):
    """Rebuild every region's packed fp32 copies (dst = PF, dst_t = PB, float32 tensors in a make_bf16_shadow table)
    from the fp32 buffer `p` (stdadk_f32_pack_refresh)."""
    rc = lib().stdadk_f32_pack_refresh(_dev(p, "p"), C.byref(table), _stream())
    _check(rc, "stdadk_f32_pack_refresh")


def mlp_workspace_bytes(desc, B):
    return _workspace_bytes("stdadk_mlp_workspace_bytes", "invalid descriptor", C.byref(desc), B)


def _mask_array(masks):
    if masks is None:
        return None
    arr = (C.c_void_p * MAX_HIDDEN)()
    for i, m in enumerate(masks):
        arr[i] = _dev(m, f"drop_mask[{i}]") if m is not None else None
    return arr


def mlp_forward(desc, params, features, B, y_pred, workspace, training, seed=0, masks=None):
    rc = lib().stdadk_mlp_forward_f32(C.byref(desc), C.byref(params), _dev(features, "features"),
                                      features.stride(0), B, _dev(y_pred, "y_pred"), *_ws(workspace),
                                      int(training), seed, _mask_array(masks), _stream())
    _check(rc, "stdadk_mlp_forward_f32")


def mlp_backward(desc, params, grads, features, B, dY, workspace, seed=0, masks=None):
    rc = lib().stdadk_mlp_backward_f32(C.byref(desc), C.byref(params), C.byref(grads),
                                       _dev(features, "features"), features.stride(0), B,
                                       _dev(dY, "dY"), *_ws(workspace), seed, _mask_array(masks), _stream())
    _check(rc, "stdadk_mlp_backward_f32")


def gemm(A, a_km, Bm, b_km, M, N, K, bias=None, out=None, workspace=None):
    """C[M,N] = Aop Bop (+bias) with the MLP's fp32 MFMA GEMM (layouts: include/stdadk.h)."""
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    need = lib().stdadk_gemm_workspace_bytes(M, N, K)
    if workspace is None and need:
        workspace = torch.empty(need // 4, device=A.device, dtype=torch.float32)
    rc = lib().stdadk_gemm_f32(_dev(A, "A"), A.stride(0), int(a_km), _dev(Bm, "B"), Bm.stride(0),
                               int(b_km), M, N, K, _dev(bias, "bias"), _dev(out, "C"), out.stride(0),
                               workspace.data_ptr() if workspace is not None else None,
                               workspace.numel() * 4 if workspace is not None else 0, _stream())
    _check(rc, "stdadk_gemm_f32")
    return out


def make_basis(p, basis, sides, s_centers, s_bw, t_centers, t_bw):
    """ABI descriptor of the knot tables; `sides` = level side lengths of a uniform grid, or (with FLAG_SCATTERED)
    the knot COUNT of every level of a scattered table, or None."""
    b = BasisDesc()
    b.p, b.basis = int(p), BASIS_KIND[basis]
    b.n_levels = len(sides) if sides else 0
    if b.n_levels > 8:
        b.n_levels = 0          # more levels than the window path tracks: dense path only
    for i in range(b.n_levels):
        b.side[i] = int(sides[i])
    b.Ks, b.Kt = s_centers.shape[0], t_centers.shape[0]
    b.s_centers, b.s_bw = _dev(s_centers, "s_centers"), _dev(s_bw, "s_bw")
    b.t_centers, b.t_bw = _dev(t_centers, "t_centers"), _dev(t_bw, "t_bw")
    return b


def step_uses_window(basis, desc, flags):
    return bool(lib().stdadk_step_uses_window(C.byref(basis), C.byref(desc), flags))


def step_workspace_bytes(basis, desc, B, flags):
    return _workspace_bytes("stdadk_step_workspace_bytes", "invalid descriptors", C.byref(basis), C.byref(desc), B, flags)


def forward(basis, desc, params, coords, t, X, B, y_pred, workspace, flags, training=False, seed=0,
            step_dev=None):
    rc = lib().stdadk_forward_f32(C.byref(basis), C.byref(desc), C.byref(params), _dev(coords, "coords"),
                                  _dev(t, "t"), _dev(X, "X"), B, _dev(y_pred, "y_pred"), *_ws(workspace),
                                  int(training), seed, _dev(step_dev, "step_dev"), flags, _stream())
    _check(rc, "stdadk_forward_f32")


def backward(basis, desc, params, grads, B, dY, workspace, flags, seed=0, step_dev=None):
    rc = lib().stdadk_backward_f32(C.byref(basis), C.byref(desc), C.byref(params), C.byref(grads), B,
                                   _dev(dY, "dY"), *_ws(workspace), seed, _dev(step_dev, "step_dev"), flags,
                                   _stream())
    _check(rc, "stdadk_backward_f32")


def make_loss(kind="mse", Q=1, y_cols=None, taus=None, nc_weight=0.0, nc_power=1):
    """stdadk_loss_desc for an objective on (B,Q) predictions: kind "mse" or "pinball" (check loss
    with levels `taus`, optional prediction-level non-crossing penalty)."""
    if kind not in ("mse", "pinball"):
        raise ValueError(f"unknown loss kind '{kind}'; use 'mse' or 'pinball'")
    if Q < 1 or Q > MAX_Q:
        raise ValueError(f"Q={Q} outside 1..{MAX_Q}")
    ld = LossDesc()
    ld.kind = LOSS_MSE if kind == "mse" else LOSS_PINBALL
    ld.y_cols = Q if y_cols is None else int(y_cols)
    if kind == "pinball":
        taus = list(taus if taus is not None else [])
        if len(taus) != Q:
            raise ValueError(f"pinball loss needs {Q} quantile levels, got {len(taus)}")
        for i, q in enumerate(taus):
            ld.tau[i] = float(q)
        if nc_weight and int(nc_power) not in (1, 2):
            raise ValueError(f"Unsupported power={nc_power}; use 1 or 2.")
        ld.nc_weight = float(nc_weight)
        ld.nc_power = int(nc_power)
    return ld


def loss(desc, y_pred, y, grad_scale, dY=None, loss_sum=None):
    """stdadk_loss_f32 on y_pred (B,Q), y (B,y_cols); desc None = MSE."""
    B, Q = y_pred.shape
    rc = lib().stdadk_loss_f32(_ref(desc), _dev(y_pred, "y_pred"), _dev(y, "y"), B, Q, grad_scale, _dev(dY, "dY"),
                               _dev(loss_sum, "loss_sum"), _stream())
    _check(rc, "stdadk_loss_f32")


def _rows(tensor, name, cols):
    """Address + row stride of a (Q, cols) fp32 device matrix whose rows are contiguous."""
    if not _on_device(tensor) or tensor.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected a float32 tensor on a HIP device, got {tensor.dtype} on "
                           f"{tensor.device}; the MI355X build of stnf has no CPU path")
    if tensor.dim() != 2 or tensor.shape[1] != cols or (cols > 1 and tensor.stride(1) != 1):
        raise RuntimeError(f"{name}: expected shape (Q, {cols}) with contiguous rows, got {tuple(tensor.shape)}")
    return tensor.data_ptr(), tensor.stride(0)


def delta_head(delta, Wo, bo):
    """delta (Q, d+1) rows (any row stride) -> Wo (Q,d), bo (Q): cumulative sums over quantiles."""
    Q, d = Wo.shape
    ptr, ldd = _rows(delta, "delta", d + 1)
    rc = lib().stdadk_delta_head_f32(ptr, ldd, Q, d, _dev(Wo, "Wo"), _dev(bo, "bo"), _stream())
    _check(rc, "stdadk_delta_head_f32")


def delta_head_backward(delta, dWo, dbo, lambda_grad, lambda_loss, d_delta, loss_sum=None):
    Q, d = dWo.shape
    ptr, ldd = _rows(delta, "delta", d + 1)
    gptr, ldg = _rows(d_delta, "d_delta", d + 1)
    if ldg != ldd:
        raise RuntimeError("delta_head_backward: delta and d_delta must share the row stride")
    rc = lib().stdadk_delta_head_backward_f32(ptr, _dev(dWo, "dWo"), _dev(dbo, "dbo"), ldd, Q, d,
                                              lambda_grad, lambda_loss, gptr, _dev(loss_sum, "loss_sum"),
                                              _stream())
    _check(rc, "stdadk_delta_head_backward_f32")


def spatial_partial(basis, desc, params, coords, out, workspace, flags):
    """stdadk_spatial_partial_f32: out (S, h0) = the per-site half of layer 0's pre-activation."""
    S = coords.shape[0]
    if tuple(out.shape) != (S, desc.hidden[0]):
        raise RuntimeError(f"spatial_partial: out has shape {tuple(out.shape)}")
    rc = lib().stdadk_spatial_partial_f32(C.byref(basis), C.byref(desc), C.byref(params), _dev(coords, "coords"), S,
                                          _dev(out, "out"), *_ws(workspace), flags, _stream())
    _check(rc, "stdadk_spatial_partial_f32")


def temporal_partial(basis, desc, params, t_values, out, flags):
    """stdadk_temporal_partial_f32: out (T, h0) = the per-time half of layer 0's pre-activation."""
    T = t_values.numel()
    if tuple(out.shape) != (T, desc.hidden[0]):
        raise RuntimeError(f"temporal_partial: out has shape {tuple(out.shape)}")
    rc = lib().stdadk_temporal_partial_f32(C.byref(basis), C.byref(desc), C.byref(params), _dev(t_values, "t_values"),
                                           T, _dev(out, "out"), flags, _stream())
    _check(rc, "stdadk_temporal_partial_f32")


def forward_parts_supported(desc):
    """stdadk_forward_parts_supported: whether forward_parts runs this MLP (the fused tail's widths and head)."""
    return bool(lib().stdadk_forward_parts_supported(C.byref(desc)))


def forward_parts(desc, params, sp, tp, y_pred):
    """stdadk_forward_parts_f32: y_pred (T*S, Q), rows time-major, from the two halves of layer 0."""
    S, T = sp.shape[0], tp.shape[0]
    if y_pred.shape[0] != S * T:
        raise RuntimeError("forward_parts: y_pred must have T*S rows")
    rc = lib().stdadk_forward_parts_f32(C.byref(desc), C.byref(params), _dev(sp, "sp"), S, _dev(tp, "tp"), T,
                                        _dev(y_pred, "y_pred"), _stream())
    _check(rc, "stdadk_forward_parts_f32")


def make_sparsity(kind, lambda_l1=0.01, lambda_group=0.01, apply_spatial=True, apply_temporal=True):
    if kind not in SPARSITY_KINDS:
        raise ValueError(f"Unknown penalty_type: {kind}")
    s = SparsityDesc()
    s.kind, s.lambda_l1, s.lambda_group = SPARSITY_KINDS[kind], float(lambda_l1), float(lambda_group)
    s.apply_spatial, s.apply_temporal = int(bool(apply_spatial)), int(bool(apply_temporal))
    return s


def sparsity(sp, W0, dW0, w0_t, p, Ks, Kt, grad_scale=1.0, loss_scale=0.0, loss_sum=None, penalties=None):
    """stdadk_sparsity_f32: W0 / dW0 are (D, H0) with w0_t, else (H0, D); penalties (2,) accumulates
    (spatial, temporal)."""
    D = p + Ks + Kt
    H0 = W0.shape[1] if w0_t else W0.shape[0]
    if tuple(W0.shape) != ((D, H0) if w0_t else (H0, D)):
        raise RuntimeError(f"sparsity: W0 has shape {tuple(W0.shape)}, D = {D}")
    if dW0 is not None and (dW0.shape != W0.shape or dW0.stride() != W0.stride()):
        raise RuntimeError("sparsity: dW0 must have the shape and strides of W0")
    if penalties is not None and penalties.numel() != 2:
        raise RuntimeError("sparsity: penalties must hold 2 floats")
    rc = lib().stdadk_sparsity_f32(C.byref(sp), _dev(W0, "W0"), _dev(dW0, "dW0"), W0.stride(0), int(bool(w0_t)),
                                   H0, p, Ks, Kt, grad_scale, loss_scale, _dev(loss_sum, "loss_sum"),
                                   _dev(penalties, "penalties"), _stream())
    _check(rc, "stdadk_sparsity_f32")


def _train(name, basis, desc, params, grads, coords, t, X, y, rows, grad_scale, loss_desc, loss_sum, workspace, seed,
           flags, optim=None, sparsity_desc=None, tail=(), y_pred=None, step_dev=None, aux_stream=None):
    """The call behind the five training doors: what they share, in the order the library takes it.  `rows` stands
    between the arrays and the gradient scale: (B,), or (address, count) of the index tensor.  With `optim` it is a
    one-call door (sparsity descriptor before the accumulator, optimiser descriptor and the door's own `tail` after the
    flags); without, a split door (`y_pred` after the accumulator, the device step counter, the auxiliary stream)."""
    cur = None if _DRY_RUN else _current_device()           # asked once for the call's tensors
    stream = _stream(cur)
    fn = getattr(lib(), name)
    # (the hot call of every step: `_ref` and `_ws` written out, a Python frame each otherwise)
    loss_ref = C.byref(loss_desc) if loss_desc is not None else None
    ws_ptr, ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if optim is not None:
        rc = fn(C.byref(basis), C.byref(desc), C.byref(params), C.byref(grads), _dev(coords, "coords", cur),
                _dev(t, "t", cur), _dev(X, "X", cur), _dev(y, "y", cur), *rows, grad_scale, loss_ref,
                C.byref(sparsity_desc) if sparsity_desc is not None else None, _dev(loss_sum, "loss_sum", cur),
                ws_ptr, ws_bytes, seed, flags, C.byref(optim), *tail, stream)
    else:
        rc = fn(C.byref(basis), C.byref(desc), C.byref(params), C.byref(grads), _dev(coords, "coords", cur),
                _dev(t, "t", cur), _dev(X, "X", cur), _dev(y, "y", cur), *rows, grad_scale, loss_ref,
                _dev(loss_sum, "loss_sum", cur), _dev(y_pred, "y_pred", cur), ws_ptr, ws_bytes, seed,
                _dev(step_dev, "step_dev", cur), flags, stream,
                aux_stream.cuda_stream if aux_stream is not None else None)
    _check(rc, name)


def train_fwd_bwd(basis, desc, params, grads, coords, t, X, y, B, grad_scale, loss_sum, y_pred,
                  workspace, flags, seed=0, step_dev=None, aux_stream=None, loss_desc=None):
    _train("stdadk_train_fwd_bwd_f32", basis, desc, params, grads, coords, t, X, y, (B,), grad_scale, loss_desc,
           loss_sum, workspace, seed, flags, y_pred=y_pred, step_dev=step_dev, aux_stream=aux_stream)


def train_fwd_bwd_indexed(basis, desc, params, grads, coords_all, t_all, X_all, y_all, idx, grad_scale,
                          loss_sum, y_pred, workspace, flags, seed=0, step_dev=None, aux_stream=None,
                          loss_desc=None):
    """The fused step on rows `idx` (contiguous int64 device tensor) of the resident arrays (window path)."""
    _train("stdadk_train_fwd_bwd_indexed_f32", basis, desc, params, grads, coords_all, t_all, X_all, y_all,
           _idx(idx, "train_fwd_bwd_indexed: idx"), grad_scale, loss_desc, loss_sum, workspace, seed, flags,
           y_pred=y_pred, step_dev=step_dev, aux_stream=aux_stream)


def bin_batch(basis, desc, coords_all, t_all, X_all, y_all, idx, workspace, flags):
    """Batch preparation of the window path on its own (rows `idx` of the resident arrays binned into
    `workspace`) on the current stream; the step then runs with FLAG_PREBINNED."""
    rc = lib().stdadk_bin_batch_f32(C.byref(basis), C.byref(desc), _dev(coords_all, "coords"), _dev(t_all, "t"),
                                    _dev(X_all, "X"), _dev(y_all, "y"), *_idx(idx, "bin_batch: idx"),
                                    y_all.shape[1] if y_all is not None else 0, *_ws(workspace), flags, _stream())
    _check(rc, "stdadk_bin_batch_f32")


# slots of the float64 accumulator stdadk_eval_indexed_f32 adds into (include/stdadk.h)
EVAL_OBJECTIVE, EVAL_SSE, EVAL_SAE, EVAL_ROWS, EVAL_BATCHES, EVAL_CHECK, EVAL_SLOTS = 0, 1, 2, 3, 4, 5, 16


def eval_workspace_bytes(basis, desc, B, flags):
    return _workspace_bytes("stdadk_eval_workspace_bytes", "invalid descriptors", C.byref(basis), C.byref(desc), B, flags)


def eval_indexed(basis, desc, params, coords_all, t_all, X_all, y_all, idx, loss_desc, metric_col, batch_weight, acc,
                 y_pred, workspace, flags):
    """Forward-only pass on rows `idx` (contiguous int64 device tensor) of the resident arrays; the batch's metric
    sums are ADDED into `acc` (EVAL_SLOTS float64 on the device); `y_pred` (B,Q) or None."""
    if acc.dtype != torch.float64 or not _on_device(acc) or not acc.is_contiguous() or acc.numel() < EVAL_SLOTS:
        raise RuntimeError(f"eval_indexed: acc must be {EVAL_SLOTS} contiguous float64 on the device")
    rc = lib().stdadk_eval_indexed_f32(
        C.byref(basis), C.byref(desc), C.byref(params), _dev(coords_all, "coords"), _dev(t_all, "t"),
        _dev(X_all, "X"), _dev(y_all, "y"), *_idx(idx, "eval_indexed: idx"), _ref(loss_desc), int(metric_col),
        float(batch_weight), acc.data_ptr(), _dev(y_pred, "y_pred"), *_ws(workspace), flags, _stream())
    _check(rc, "stdadk_eval_indexed_f32")


# slots per split of the float64 accumulator stdadk_grid_score_f32 adds into (include/stdadk.h)
GRID_N, GRID_SSE, GRID_SAE, GRID_COVER, GRID_WIDTH, GRID_CHECK, GRID_SLOTS = 0, 1, 2, 3, 4, 5, 16


def grid_score_workspace_bytes(S, nT):
    return _workspace_bytes("stdadk_grid_score_workspace_bytes", f"bad grid {S} x {nT} (S*nT must stay below 2^31)", S, nT)


def _grid_args(what, y_pred, z, split, taus, workspace):
    """The checks grid_score and quantile_diag share; returns nT, S, Q and the levels as a c_float array (or None)."""
    if z.dim() != 2 or y_pred.dim() != 2:
        raise RuntimeError(f"{what}: z must be (nT, S) and y_pred (nT*S, Q)")
    nT, S = z.shape
    Q = y_pred.shape[1]
    if y_pred.shape[0] != nT * S:
        raise RuntimeError(f"{what}: y_pred has {y_pred.shape[0]} rows, z is {nT} x {S}")
    for name, x in (("y_pred", y_pred), ("z", z)):
        if x.dtype != torch.float32:
            raise RuntimeError(f"{what}: {name} must be float32, got {x.dtype}")
    if split is not None and (split.dtype != torch.uint8 or tuple(split.shape) != (nT, S)):
        raise RuntimeError(f"{what}: split must be uint8 of shape {(nT, S)}, got {split.dtype} {tuple(split.shape)}")
    if taus is not None and len(taus) != Q:
        raise RuntimeError(f"{what}: {Q} quantile levels expected, got {len(taus)}")
    if workspace.dtype != torch.float64 or not _on_device(workspace) or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: workspace must be a contiguous float64 tensor on the device")
    return nT, S, Q, (C.c_float * Q)(*[float(q) for q in taus]) if taus is not None else None


def grid_score(y_pred, z, split, metric_col, taus, lo_col, hi_col, split_acc, site_acc, time_acc, workspace):
    """stdadk_grid_score_f32 on one chunk of time slices: y_pred (nT*S, Q) time-major, z (nT, S) float32 with NaN = no
    value, split (nT, S) uint8 codes 0..3 or None; sums are ADDED into split_acc (4, GRID_SLOTS) and site_acc
    (4, S, 3) and ASSIGNED to time_acc (4, nT, 3), all float64 on the device.  taus: Q levels or None (0.5 each);
    lo_col / hi_col: the interval's columns or -1 / -1."""
    nT, S, Q, arr = _grid_args("grid_score", y_pred, z, split, taus, workspace)
    acc = lambda t, name, shape: _typed("grid_score", t, name, torch.float64, shape)      # noqa: E731
    rc = lib().stdadk_grid_score_f32(
        _dev(y_pred, "y_pred"), _dev(z, "z"), _dev(split, "split"), S, nT, Q, int(metric_col), arr, int(lo_col),
        int(hi_col), acc(split_acc, "split_acc", (4, GRID_SLOTS)), acc(site_acc, "site_acc", (4, S, 3)),
        acc(time_acc, "time_acc", (4, nT, 3)), workspace.data_ptr(), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_grid_score_f32")


# slots per split of the float64 accumulator stdadk_quantile_diag_f32 adds into (include/stdadk.h)
QD_N, QD_BELOW, QD_PIT, QD_CROSS_ROWS, QD_PAIR, QD_DEPTH1, QD_DEPTH2, QD_CRPS, QD_INSIDE, QD_SLOTS = \
    0, 1, 9, 18, 19, 26, 27, 28, 29, 32


def quantile_diag_workspace_bytes(S, nT):
    return _workspace_bytes("stdadk_quantile_diag_workspace_bytes", f"bad grid {S} x {nT} (S*nT must stay below 2^31)",
                            S, nT)


def quantile_diag(y_pred, z, split, taus, lo_col, hi_col, split_acc, site_acc, time_acc, workspace):
    """stdadk_quantile_diag_f32 on one chunk of time slices, laid out as grid_score's: y_pred (nT*S, Q) time-major,
    z (nT, S) float32 with NaN = no value, split (nT, S) uint8 codes 0..3 or None; the quantile diagnostics are ADDED
    into split_acc (4, QD_SLOTS) and site_acc (4, S, 4) and ASSIGNED to time_acc (4, nT, 4), all float64 on the
    device; site_acc and time_acc may each be None (skipped).  taus: Q levels or None (0.5 each); lo_col / hi_col: the
    interval's columns or -1 / -1."""
    nT, S, Q, arr = _grid_args("quantile_diag", y_pred, z, split, taus, workspace)
    acc = lambda t, name, shape: _typed("quantile_diag", t, name, torch.float64, shape)      # noqa: E731
    rc = lib().stdadk_quantile_diag_f32(
        _dev(y_pred, "y_pred"), _dev(z, "z"), _dev(split, "split"), S, nT, Q, arr, int(lo_col), int(hi_col),
        acc(split_acc, "split_acc", (4, QD_SLOTS)), None if site_acc is None else acc(site_acc, "site_acc", (4, S, 4)),
        None if time_acc is None else acc(time_acc, "time_acc", (4, nT, 4)), workspace.data_ptr(), workspace.numel() * 8,
        _stream())
    _check(rc, "stdadk_quantile_diag_f32")


# slots per (split, lag, bin) of the float64 accumulator stdadk_variogram_f32 assigns (include/stdadk.h)
VG_N, VG_SZ, VG_SP, VG_SR, VG_MAX_BINS, VG_MAX_LAGS = 0, 1, 2, 3, 64, 16


def variogram_workspace_bytes(S, nT, n_bins, n_lags):
    return _workspace_bytes("stdadk_variogram_workspace_bytes",
                            f"bad sizes: grid {S} x {nT} (S*nT must stay below 2^31), n_bins={n_bins} (1..{VG_MAX_BINS}), "
                            f"n_lags={n_lags} (1..{VG_MAX_LAGS})", S, nT, n_bins, n_lags)


def variogram(y_pred, col, z, split, coords, edges2, n_lags, acc, workspace):
    """stdadk_variogram_f32 on one whole grid: y_pred (nT*S, ld) float32 time-major whose column `col` is the
    prediction, or None (the field only: SP = SR = 0); z (nT, S) float32 with NaN = no value; split (nT, S) uint8 codes
    0..3 or None; coords (S, 2) float32; edges2: the n_bins + 1 SQUARED bin edges, host floats.  The pair counts and
    sums of lags 0 .. n_lags - 1 are ASSIGNED to acc (4, n_lags, n_bins, 4), float64 on the device."""
    if z.dim() != 2:
        raise RuntimeError("variogram: z must be (nT, S)")
    nT, S = z.shape
    f32 = lambda t, name, shape: _typed("variogram", t, name, torch.float32, shape)      # noqa: E731
    f64 = lambda t, name, shape: _typed("variogram", t, name, torch.float64, shape)      # noqa: E731
    ldy = 0
    if y_pred is not None:
        if y_pred.dim() != 2 or y_pred.shape[0] != nT * S:
            raise RuntimeError(f"variogram: y_pred must be (nT*S, ld) = ({nT * S}, ld), got {tuple(y_pred.shape)}")
        ldy = y_pred.shape[1]
    edges2 = [float(e) for e in edges2]
    n_bins = len(edges2) - 1
    rc = lib().stdadk_variogram_f32(
        None if y_pred is None else f32(y_pred, "y_pred", None), ldy, int(col), f32(z, "z", (nT, S)),
        None if split is None else _typed("variogram", split, "split", torch.uint8, (nT, S)),
        f32(coords, "coords", (S, 2)), S, nT, (C.c_double * len(edges2))(*edges2), n_bins, int(n_lags),
        f64(acc, "acc", (4, int(n_lags), n_bins, 4)), f64(workspace, "workspace", None), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_variogram_f32")


# slots of the float64 accumulators stdadk_basis_diag_f32 assigns (include/stdadk.h): per knot and per (site, level)
BD_K_N, BD_K_W, BD_K_SPHI, BD_K_SPHI2, BD_K_SV, BD_K_WV, BD_K_NEAR2, BD_KNOT_SLOTS = 0, 1, 2, 3, 4, 5, 6, 7
BD_S_COVER, BD_S_SPHI, BD_S_NEAR2, BD_SITE_SLOTS = 0, 1, 2, 3
MAX_LEVELS = 8


def basis_diag_workspace_bytes(S, Ks):
    return _workspace_bytes("stdadk_basis_diag_workspace_bytes", f"bad sizes: S={S}, Ks={Ks} (each 0 .. 2^31-1)", S, Ks)


def basis_diag(s_centers, s_bw, basis, level_sizes, coords, w, v, rho, knot_acc, site_acc, workspace):
    """stdadk_basis_diag_f32: the sites x knots pair reduction on the knot tables s_centers (Ks, 2), s_bw (Ks,) float32
    (bandwidths, not their logarithms) of kind `basis` ('wendland' / 'gaussian' / 'triangular'), `level_sizes` the knot
    counts per level (host integers summing to Ks), coords (S, 2) float32, w / v (S,) float64 or None, `rho` the
    support radius in units of the scaled radius.  ASSIGNS knot_acc (Ks, 7) and site_acc (S, n_levels, 3), float64 on
    the device."""
    f32 = lambda t, name, shape: _typed("basis_diag", t, name, torch.float32, shape)      # noqa: E731
    f64 = lambda t, name, shape: _typed("basis_diag", t, name, torch.float64, shape)      # noqa: E731
    if s_centers.dim() != 2 or coords.dim() != 2:
        raise RuntimeError("basis_diag: s_centers must be (Ks, 2) and coords (S, 2)")
    Ks, S = s_centers.shape[0], coords.shape[0]
    sizes = [int(n) for n in level_sizes]
    L = len(sizes)
    rc = lib().stdadk_basis_diag_f32(
        f32(s_centers, "s_centers", (Ks, 2)), f32(s_bw, "s_bw", (Ks,)), Ks, BASIS_KIND[basis],
        (C.c_int64 * max(L, 1))(*sizes), L, f32(coords, "coords", (S, 2)), S,
        None if w is None else f64(w, "w", (S,)), None if v is None else f64(v, "v", (S,)), float(rho),
        f64(knot_acc, "knot_acc", (Ks, BD_KNOT_SLOTS)), f64(site_acc, "site_acc", (S, L, BD_SITE_SLOTS)),
        f64(workspace, "workspace", None), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_basis_diag_f32")


def group_norms(W0, transposed, H, col0, n, out):
    """stdadk_group_norms_f32: out (n,) float64 = the sum of squares of the first Linear's group of H weights of the
    basis functions col0 .. col0 + n - 1.  W0: the weight as stored, float32 with unit column stride: (H, D) with
    transposed False (a group is a column), (D, H) with transposed True (a group is a row); its row stride is ld."""
    if W0.dim() != 2 or (W0.stride(1) != 1 and W0.shape[1] > 1) or W0.dtype != torch.float32 or not _on_device(W0):
        raise RuntimeError("group_norms: W0 must be a 2-D float32 tensor with unit column stride on the device")
    if W0.shape[1 if transposed else 0] != H or not 0 <= col0 <= col0 + n <= W0.shape[0 if transposed else 1]:
        raise RuntimeError(f"group_norms: columns {col0}..{col0 + n - 1} of H={H} do not fit W0 {tuple(W0.shape)} "
                           f"(transposed={bool(transposed)})")
    ld = W0.stride(0) if W0.shape[0] > 1 else max(W0.stride(0), W0.shape[1])      # (one row: its stride means nothing)
    rc = lib().stdadk_group_norms_f32(W0.data_ptr(), ld, int(bool(transposed)), int(H), int(col0), int(n),
                                      _typed("group_norms", out, "out", torch.float64, (int(n),)), _stream())
    _check(rc, "stdadk_group_norms_f32")


# the score kinds and limits of stdadk_conformal_scores_f32 / stdadk_select_f32 (include/stdadk.h)
CONFORMAL_RESID, CONFORMAL_CQR, CONFORMAL_ABS, CONFORMAL_MAX_COLS, CONFORMAL_MAX_SEGMENTS, SELECT_MAX = 0, 1, 2, 8, 2, 16


def conformal_scores_workspace_bytes(S, nT):
    return _workspace_bytes("stdadk_conformal_scores_workspace_bytes",
                            f"bad grid {S} x {nT} (S*nT must stay below 2^31)", S, nT)


def conformal_scores(y_pred, z, split, cols, codes, scores, count, overflow, workspace):
    """stdadk_conformal_scores_f32 on one chunk of time slices, laid out as grid_score's: y_pred (nT*S, Q) time-major,
    z (nT, S) float32 with NaN = no value, split (nT, S) uint8 or None (all 0).  cols: C triples (kind, col_a, col_b),
    codes: G split codes.  The C scores of every entry with a finite z and split == codes[g] are appended to
    scores[g] (scores (G, C, cap) float32) in time-major then site order, from position count[g] on (count (G,) int64
    on the device, advanced by the call, saturating at cap); overflow (G,) int32 is set where members were dropped."""
    what = "conformal_scores"
    nT, S, Q, _ = _grid_args(what, y_pred, z, split, None, workspace)
    Cn, G = len(cols), len(codes)
    if scores.dim() != 3 or tuple(scores.shape[:2]) != (G, Cn):
        raise RuntimeError(f"{what}: scores must be (G, C, cap) = ({G}, {Cn}, cap), got {tuple(scores.shape)}")
    flat = [int(v) for col in cols for v in col]
    if len(flat) != 3 * Cn:
        raise RuntimeError(f"{what}: every score column is (kind, col_a, col_b)")
    rc = lib().stdadk_conformal_scores_f32(
        _dev(y_pred, "y_pred"), _dev(z, "z"), _dev(split, "split"), S, nT, Q, (C.c_int32 * len(flat))(*flat), Cn,
        (C.c_int32 * G)(*[int(c) for c in codes]), G, _typed(what, scores, "scores", torch.float32, None),
        scores.shape[2], _typed(what, count, "count", torch.int64, (G,)),
        _typed(what, overflow, "overflow", torch.int32, (G,)), workspace.data_ptr(), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_conformal_scores_f32")


def select_workspace_bytes(n_sel):
    return _workspace_bytes("stdadk_select_workspace_bytes", f"n_sel={n_sel} outside 1..{SELECT_MAX}", n_sel)


def select(keys, n, selections, value, rank_used, workspace, n_max=None):
    """stdadk_select_f32: exact order statistics of the columns of keys (C, stride) float32, of which the first n
    (a 1-element int64 tensor on the device; n_max bounds it on the host, default the stride) are the data.
    selections: (column, rank, beta) each -- a 0-based rank, or a negative rank (or None) and the level beta, for the
    1-based rank ceil((n + 1) * beta).  value (n_sel,) float32 and rank_used (n_sel,) int64 on the device; a rank
    beyond n gives +inf and -1."""
    what = "select"
    if keys.dim() != 2:
        raise RuntimeError(f"{what}: keys must be (C, stride), got {tuple(keys.shape)}")
    Cn, stride = keys.shape
    k = len(selections)
    cols = (C.c_int32 * k)(*[int(s[0]) for s in selections])
    ranks = (C.c_int64 * k)(*[-1 if s[1] is None else int(s[1]) for s in selections])
    betas = (C.c_double * k)(*[0.0 if s[2] is None else float(s[2]) for s in selections])
    if workspace.dtype != torch.float64 or not _on_device(workspace) or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: workspace must be a contiguous float64 tensor on the device")
    rc = lib().stdadk_select_f32(
        _typed(what, keys, "keys", torch.float32, None), stride, Cn, _typed(what, n, "n", torch.int64, (1,)),
        stride if n_max is None else int(n_max), cols, ranks, betas, k,
        _typed(what, value, "value", torch.float32, (k,)), _typed(what, rank_used, "rank_used", torch.int64, (k,)),
        workspace.data_ptr(), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_select_f32")


KNN_MAX_K = 16      # STDADK_KNN_MAX_K of include/stdadk.h


def knn_workspace_bytes(M, S, nM, k):
    return _workspace_bytes("stdadk_knn_workspace_bytes",
                            f"bad sizes: M={M}, S={S}, nM={nM} (each 0 .. 2^31-1, nM*M*k below 2^31), k={k} "
                            f"(1..{KNN_MAX_K})", M, S, nM, k)


def _knn_call(what, symbol, q, coords, src, k, exclude_self, nbr_idx, nbr_d2, workspace):
    """The one parameter list of the two searches, checked and passed to `symbol`."""
    if q.dim() != 2 or coords.dim() != 2:
        raise RuntimeError(f"{what}: q must be (M, 2) and coords (S, 2)")
    M, S = q.shape[0], coords.shape[0]
    nM = 1 if src is None else src.shape[0]
    k = int(k)
    rc = getattr(lib(), symbol)(
        _typed(what, q, "q", torch.float32, (M, 2)), M, _typed(what, coords, "coords", torch.float32, (S, 2)), S,
        None if src is None else _typed(what, src, "src", torch.uint8, (nM, S)), nM, k, int(bool(exclude_self)),
        _typed(what, nbr_idx, "nbr_idx", torch.int32, (nM, M, k)), _typed(what, nbr_d2, "nbr_d2", torch.float64, (nM, M, k)),
        _typed(what, workspace, "workspace", torch.float64, None), workspace.numel() * 8, _stream())
    _check(rc, symbol)


def knn(q, coords, src, k, exclude_self, nbr_idx, nbr_d2, workspace):
    """stdadk_knn_f32: for every target of q (M, 2) float32 the k nearest sources among coords (S, 2) float32 in the
    total order (d2, index), d2 in float64.  src: (nM, S) uint8, slice m's sources are the sites with src != 0, or None
    (every site, one slice).  exclude_self (needs M == S) skips source j for target j.  ASSIGNS nbr_idx (nM, M, k) int32
    and nbr_d2 (nM, M, k) float64 on the device; a row short of k sources ends in -1 / +inf."""
    _knn_call("knn", "stdadk_knn_f32", q, coords, src, k, exclude_self, nbr_idx, nbr_d2, workspace)


def knn_cells_workspace_bytes(M, S, nM, k):
    return _workspace_bytes("stdadk_knn_cells_workspace_bytes",
                            f"bad sizes: M={M}, S={S}, nM={nM} (each 0 .. 2^31-1, nM*M*k below 2^31), k={k} "
                            f"(1..{KNN_MAX_K})", M, S, nM, k)


def knn_cells(q, coords, src, k, exclude_self, nbr_idx, nbr_d2, workspace):
    """stdadk_knn_cells_f32: knn's arguments and knn's table, bit for bit, by a cell-binned search (the sites binned
    into a uniform grid, a wave of cell-adjacent targets walking rings of cells until no neighbour can be gained); the
    workspace is knn_cells_workspace_bytes'."""
    _knn_call("knn_cells", "stdadk_knn_cells_f32", q, coords, src, k, exclude_self, nbr_idx, nbr_d2, workspace)


def knn_apply(nbr_idx, nbr_d2, k, z, power, nearest, idw):
    """stdadk_knn_apply_f32: the table nbr_idx / nbr_d2 (nM, M, k_tab) of knn, nM == 1 or nM == nT, applied to the
    slices z (nT, S) float32 with the first k entries of every row: ASSIGNS nearest (nT, M) (the nearest source's value)
    and idw (nT, M) (inverse-distance weighting with w = d^-power, power 0..4; the mean over zero distances where there
    are any), float32 on the device; either may be None.  NaN where a row holds no source."""
    what = "knn_apply"
    if nbr_idx.dim() != 3 or z.dim() != 2:
        raise RuntimeError(f"{what}: the table must be (nM, M, k_tab) and z (nT, S)")
    nM, M, k_tab = nbr_idx.shape
    nT, S = z.shape
    out = lambda t, name: None if t is None else _typed(what, t, name, torch.float32, (nT, M))      # noqa: E731
    rc = lib().stdadk_knn_apply_f32(
        _typed(what, nbr_idx, "nbr_idx", torch.int32, (nM, M, k_tab)),
        _typed(what, nbr_d2, "nbr_d2", torch.float64, (nM, M, k_tab)), nM, M, k_tab, int(k),
        _typed(what, z, "z", torch.float32, (nT, S)), nT, S, int(power), out(nearest, "nearest"), out(idw, "idw"),
        _stream())
    _check(rc, "stdadk_knn_apply_f32")


# the variogram models and the column limit of stdadk_krige_weights_f64 / stdadk_krige_apply_f32 (include/stdadk.h)
KRIGE_EXPONENTIAL, KRIGE_SPHERICAL, KRIGE_GAUSSIAN, KRIGE_MAX_COLS = 0, 1, 2, 8


def krige_weights(nbr_idx, nbr_d2, k, coords, model, nugget, psill, range_, w, var):
    """stdadk_krige_weights_f64: for every row of the table nbr_idx / nbr_d2 (nM, M, k_tab) of knn the local
    ordinary-kriging weights of its first k entries under the variogram model (KRIGE_*; nugget, psill, range) and the
    kriging variance of a new noisy observation; coords (S, 2) float32 are the sites the indices name.  ASSIGNS
    w (nM, M, k) and var (nM, M) float64 on the device: 0 / NaN where a row holds no source, all NaN where it is
    singular."""
    what = "krige_weights"
    if nbr_idx.dim() != 3 or coords.dim() != 2:
        raise RuntimeError(f"{what}: the table must be (nM, M, k_tab) and coords (S, 2)")
    nM, M, k_tab = nbr_idx.shape
    S, k = coords.shape[0], int(k)
    rc = lib().stdadk_krige_weights_f64(
        _typed(what, nbr_idx, "nbr_idx", torch.int32, (nM, M, k_tab)),
        _typed(what, nbr_d2, "nbr_d2", torch.float64, (nM, M, k_tab)), nM, M, k_tab, k,
        _typed(what, coords, "coords", torch.float32, (S, 2)), S, int(model), float(nugget), float(psill), float(range_),
        _typed(what, w, "w", torch.float64, (nM, M, k)), _typed(what, var, "var", torch.float64, (nM, M)), _stream())
    _check(rc, "stdadk_krige_weights_f64")


def krige_apply(nbr_idx, w, var, k, z, zq, out):
    """stdadk_krige_apply_f32: the weights w (nM, M, k) and variances var (nM, M) of krige_weights on the table nbr_idx
    (nM, M, k_tab), nM == 1 or nM == nT, applied to the slices z (nT, S) float32.  zq: Q standard-normal quantiles (0 for
    the mean).  ASSIGNS the first Q columns of out (nT*M, ldo) float32 on the device, grid_score's y_pred layout:
    prediction + zq * sqrt(max(var, 0)); NaN where a row has no prediction."""
    what = "krige_apply"
    if nbr_idx.dim() != 3 or z.dim() != 2 or out.dim() != 2:
        raise RuntimeError(f"{what}: the table must be (nM, M, k_tab), z (nT, S) and out (nT*M, ldo)")
    nM, M, k_tab = nbr_idx.shape
    nT, S = z.shape
    k, Q = int(k), len(zq)
    rc = lib().stdadk_krige_apply_f32(
        _typed(what, nbr_idx, "nbr_idx", torch.int32, (nM, M, k_tab)), _typed(what, w, "w", torch.float64, (nM, M, k)),
        _typed(what, var, "var", torch.float64, (nM, M)), nM, M, k_tab, k, _typed(what, z, "z", torch.float32, (nT, S)),
        nT, S, (C.c_double * max(Q, 1))(*[float(v) for v in zq]), Q,
        _typed(what, out, "out", torch.float32, (nT * M, out.shape[1])), out.shape[1], _stream())
    _check(rc, "stdadk_krige_apply_f32")


def gmm_workspace_bytes(n, k):
    return _workspace_bytes("stdadk_gmm_workspace_bytes", f"bad sizes n={n}, k={k} (1 <= n < 2^31, 1 <= k <= 65536)", n, k)


def gmm_em(X, w, mu, var, reg_covar, w_out, mu_out, var_out, lower_bound, workspace):
    """stdadk_gmm_em_f64: one EM iteration of the spherical two-dimensional mixture in float64 -- the E-step on
    (w (k,), mu (k, 2), var (k,)) over the samples X (n, 2), the M-step into (w_out, mu_out, var_out), the mean
    log-likelihood of the E-step into lower_bound (1,).  Outputs must not alias inputs (ping-pong two sets)."""
    if X.dim() != 2 or X.shape[1] != 2:
        raise RuntimeError(f"gmm_em: X must be (n, 2), got {tuple(X.shape)}")
    n, k = X.shape[0], w.shape[0] if w.dim() == 1 else -1
    f64 = lambda t, name, shape: _typed("gmm_em", t, name, torch.float64, shape)      # noqa: E731
    rc = lib().stdadk_gmm_em_f64(
        f64(X, "X", (n, 2)), n, k, f64(w, "w", (k,)), f64(mu, "mu", (k, 2)), f64(var, "var", (k,)),
        float(reg_covar), f64(w_out, "w_out", (k,)), f64(mu_out, "mu_out", (k, 2)), f64(var_out, "var_out", (k,)),
        f64(lower_bound, "lower_bound", (1,)), f64(workspace, "workspace", None), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_gmm_em_f64")


KMEANS_MAX_K = 1023        # KM_MAX_K of csrc/kmeans.hip
KMEANS_STATUS = {1: "more augmentations than points", 2: "Bellman-Ford did not settle in k + 1 rounds",
                 3: "no deficit node reachable", 4: "the predecessors form a cycle", 5: "a path arc without a point"}


def kmeans_workspace_bytes(n, k):
    return _workspace_bytes("stdadk_kmeans_workspace_bytes",
                            f"bad sizes n={n}, k={k} (n >= 1, 1 <= k <= {KMEANS_MAX_K}, n k < 2^31)", n, k)


def kmeans_balanced_iter(X, mu, lo, hi, mu_out, labels, stats, status, workspace):
    """stdadk_kmeans_balanced_iter_f64: one iteration of size-constrained k-means in float64 -- the exact assignment
    of the points X (n, 2) to the centres mu (k, 2) with lo <= |cluster| <= hi into labels (n,) int32, the clusters'
    means into mu_out (k, 2), {inertia, shift} into stats (2,) float64, {stop code, augmentations} into status (2,)
    int32.  Nothing is read back here: the caller reads stats and status.  Outputs must not alias inputs."""
    if X.dim() != 2 or X.shape[1] != 2:
        raise RuntimeError(f"kmeans_balanced_iter: X must be (n, 2), got {tuple(X.shape)}")
    n, k = X.shape[0], mu.shape[0] if mu.dim() == 2 else -1
    f64 = lambda t, name, shape: _typed("kmeans_balanced_iter", t, name, torch.float64, shape)      # noqa: E731
    i32 = lambda t, name, shape: _typed("kmeans_balanced_iter", t, name, torch.int32, shape)        # noqa: E731
    rc = lib().stdadk_kmeans_balanced_iter_f64(
        f64(X, "X", (n, 2)), n, k, f64(mu, "mu", (k, 2)), int(lo), int(hi), f64(mu_out, "mu_out", (k, 2)),
        i32(labels, "labels", (n,)), f64(stats, "stats", (2,)), i32(status, "status", (2,)),
        f64(workspace, "workspace", None), workspace.numel() * 8, _stream())
    _check(rc, "stdadk_kmeans_balanced_iter_f64")


KMEANSPP_MAX_K, KMEANSPP_MAX_RUNS, KMEANSPP_MAX_L = 65536, 64, 16        # KPP_MAX_* of csrc/kmeanspp.hip


def kmeanspp_workspace_bytes(n, k, runs):
    return _workspace_bytes("stdadk_kmeanspp_workspace_bytes",
                            f"bad sizes n={n}, k={k}, runs={runs} (1 <= n < 2^31, 1 <= k <= min(n, {KMEANSPP_MAX_K}), "
                            f"1 <= runs <= {KMEANSPP_MAX_RUNS})", n, k, runs)


def kmeanspp(X, first, u, idx_out, pot_out, workspace):
    """stdadk_kmeanspp_f64: `runs` independent greedy k-means++ runs in float64 on the points X (n, 2) -- first (runs,)
    int32 the first seed rows, u (runs, k - 1, L) float64 the uniforms behind the L candidates of every further centre
    (both drawn by the caller), the chosen rows into idx_out (runs, k) int32, the final potentials into pot_out (runs,).
    Nothing is read back here.  Outputs must not alias inputs."""
    if X.dim() != 2 or X.shape[1] != 2:
        raise RuntimeError(f"kmeanspp: X must be (n, 2), got {tuple(X.shape)}")
    if idx_out.dim() != 2 or u.dim() != 3:
        raise RuntimeError(f"kmeanspp: idx_out must be (runs, k) and u (runs, k - 1, L), got {tuple(idx_out.shape)} and "
                           f"{tuple(u.shape)}")
    n, (runs, k), L = X.shape[0], idx_out.shape, u.shape[2]
    f64 = lambda t, name, shape: _typed("kmeanspp", t, name, torch.float64, shape)      # noqa: E731
    i32 = lambda t, name, shape: _typed("kmeanspp", t, name, torch.int32, shape)        # noqa: E731
    rc = lib().stdadk_kmeanspp_f64(
        f64(X, "X", (n, 2)), n, k, runs, L, i32(first, "first", (runs,)), f64(u, "u", (runs, k - 1, L)),
        i32(idx_out, "idx_out", (runs, k)), f64(pot_out, "pot_out", (runs,)), f64(workspace, "workspace", None),
        workspace.numel() * 8, _stream())
    _check(rc, "stdadk_kmeanspp_f64")


def make_knot_train(centers_init, gradient_damping=False, damping_threshold=0.3, damping_strength=1.0,
                    domain_weight=0.0, movement_weight=0.0, penalty_grad_scale=1.0, penalty_loss_scale=0.0):
    kt = KnotTrain()
    kt.centers_init = _dev(centers_init, "centers_init")
    kt.gradient_damping = 1 if gradient_damping else 0
    kt.damping_threshold, kt.damping_strength = float(damping_threshold), float(damping_strength)
    kt.domain_weight, kt.movement_weight = float(domain_weight), float(movement_weight)
    kt.penalty_grad_scale, kt.penalty_loss_scale = float(penalty_grad_scale), float(penalty_loss_scale)
    return kt


def knot_backward(basis, desc, params, coords, B, workspace, flags, knot_train, d_centers, d_log_bw,
                  loss_sum=None):
    """Gradients w.r.t. the learnable knots for the batch whose backward just ran on `workspace`."""
    rc = lib().stdadk_knot_backward_f32(C.byref(basis), C.byref(desc), C.byref(params), _dev(coords, "coords"),
                                        B, *_ws(workspace), flags, _ref(knot_train), _dev(d_centers, "d_centers"),
                                        _dev(d_log_bw, "d_log_bw"), _dev(loss_sum, "loss_sum"), _stream())
    _check(rc, "stdadk_knot_backward_f32")


def knot_grad(coords, d_phi, centers, log_bw, basis, d_centers, d_log_bw):
    """stdadk_knot_grad_f32: dL/dphi (B, Ks) -> gradients w.r.t. the centres (Ks,2) and log-bandwidths (Ks,)."""
    B, Ks = d_phi.shape
    if d_phi.stride(1) != 1:
        raise RuntimeError("knot_grad: d_phi must have unit column stride")
    need = lib().stdadk_knot_grad_workspace_bytes(B, Ks)
    ws = torch.empty(max(need // 4, 1), device=d_phi.device, dtype=torch.float32)
    rc = lib().stdadk_knot_grad_f32(_dev(coords, "coords"), B, d_phi.data_ptr(), d_phi.stride(0),
                                    _dev(centers, "centers"), _dev(log_bw, "log_bw"), Ks, BASIS_KIND[basis],
                                    _dev(d_centers, "d_centers"), _dev(d_log_bw, "d_log_bw"), ws.data_ptr(),
                                    ws.numel() * 4, _stream())
    _check(rc, "stdadk_knot_grad_f32")


def gather_batch(coords, t, y, X, idx, coords_out, t_out, y_out, X_out):
    """Rows idx (int64 device tensor) of the resident observation arrays -> contiguous batch buffers."""
    ip, B = _idx(idx, "gather_batch: idx")
    Q = y.shape[1] if y is not None else 0
    p = X.shape[1] if X is not None else 0
    rc = lib().stdadk_gather_batch_f32(_dev(coords, "coords"), _dev(t, "t"), _dev(y, "y"), _dev(X, "X"),
                                       ip, B, Q, p, _dev(coords_out, "coords_out"),
                                       _dev(t_out, "t_out"), _dev(y_out, "y_out"), _dev(X_out, "X_out"),
                                       _stream())
    _check(rc, "stdadk_gather_batch_f32")


def bin_obs(coords, G):
    """(keys[B], cell_start[G*G+1], perm[B]) int32 device tensors of the window path's binning."""
    B = coords.shape[0]
    dev = coords.device
    keys = torch.empty(B, dtype=torch.int32, device=dev)
    cell_start = torch.empty(G * G + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(max(lib().stdadk_bin_workspace_bytes(B, G) // 4, 1), dtype=torch.float32, device=dev)
    rc = lib().stdadk_bin_obs_f32(_dev(coords, "coords"), B, G, keys.data_ptr(), cell_start.data_ptr(),
                                  perm.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream())
    _check(rc, "stdadk_bin_obs_f32")
    return keys, cell_start, perm


def knot_windows(coords, sides, p):
    B, L = coords.shape[0], len(sides)
    dev = coords.device
    out = [torch.empty(B, L, dtype=torch.int32, device=dev) for _ in range(3)]
    arr = (C.c_int32 * L)(*sides)
    rc = lib().stdadk_knot_windows_i32(_dev(coords, "coords"), B, arr, L, p, out[0].data_ptr(),
                                       out[1].data_ptr(), out[2].data_ptr(), _stream())
    _check(rc, "stdadk_knot_windows_i32")
    return out


def mse(y_pred, y, grad_scale, dY=None, loss_sum=None):
    rc = lib().stdadk_mse_f32(_dev(y_pred, "y_pred"), _dev(y, "y"), y_pred.numel(), grad_scale,
                              _dev(dY, "dY"), _dev(loss_sum, "loss_sum"), _stream())
    _check(rc, "stdadk_mse_f32")


SUMSQ_PARTS = 256


def sumsq(g, parts, step_inc=None):
    """parts[0:256] = partial sums of g^2 (`parts` is a 256-float slice, fully overwritten);
    step_inc (device int32) is advanced by one when given."""
    if parts.numel() != SUMSQ_PARTS:
        raise RuntimeError(f"sumsq: parts must hold {SUMSQ_PARTS} floats")
    rc = lib().stdadk_sumsq_f32(_dev(g, "g"), g.numel(), _dev(parts, "parts"), _dev(step_inc, "step_inc"),
                                _stream())
    _check(rc, "stdadk_sumsq_f32")


def step_advance(step_dev):
    _check(lib().stdadk_step_advance(_dev(step_dev, "step_dev"), _stream()), "stdadk_step_advance")


def adamw_ema(p, g, m, v, ema, lr, betas, eps, weight_decay, step, max_norm=0.0, sumsq_parts=None,
              grad_mul=1.0, ema_decay=0.0, lr_dev=None, step_dev=None, shadow=None, loss_watch=None,
              nonfinite_step=None):
    """`loss_watch` / `nonfinite_step`: the non-finite guard of include/stdadk.h (both or neither)."""
    rc = lib().stdadk_adamw_ema_f32(_dev(p, "p"), _dev(g, "g"), _dev(m, "m"), _dev(v, "v"),
                                    _dev(ema, "ema"), p.numel(), lr, _dev(lr_dev, "lr_dev"),
                                    betas[0], betas[1], eps, weight_decay, int(step),
                                    _dev(step_dev, "step_dev"), max_norm, _dev(sumsq_parts, "sumsq"),
                                    0 if sumsq_parts is None else sumsq_parts.numel(),
                                    grad_mul, ema_decay, _ref(shadow), _dev(loss_watch, "loss_watch"),
                                    _dev(nonfinite_step, "nonfinite_step"), _stream())
    _check(rc, "stdadk_adamw_ema_f32")


def make_optim(p, g, m, v, ema, lr, lr_dev, betas, eps, weight_decay, step_dev, max_norm, sumsq_parts, ema_decay,
               shadow=None, nonfinite_step=None):
    if sumsq_parts is not None and sumsq_parts.numel() != GRADSQ_PARTS:
        raise RuntimeError(f"make_optim: sumsq_parts must hold {GRADSQ_PARTS} floats")
    o = _fill_group(OptimDesc(), p, g, m, v, ema, lr, lr_dev, max_norm, sumsq_parts, shadow)
    o.nonfinite_step = _dev(nonfinite_step, "nonfinite_step")
    o.beta1, o.beta2, o.eps, o.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    o.step_dev = _dev(step_dev, "step_dev")
    o.ema_decay = float(ema_decay)
    return o


def _fill_group(d, p, g, m, v, ema, lr, lr_dev, max_norm, sumsq_parts, shadow):
    """The fields an OptimDesc and an AdamGroup share: buffers, rate, clip norm and its partials, operand copies."""
    d._keep = shadow                 # the descriptor points at it
    d.shadow = C.pointer(shadow) if shadow is not None else None
    d.p, d.g, d.m, d.v, d.ema = _dev(p, "p"), _dev(g, "g"), _dev(m, "m"), _dev(v, "v"), _dev(ema, "ema")
    d.n = p.numel()
    d.lr, d.lr_dev = float(lr), _dev(lr_dev, "lr_dev")
    d.max_norm = float(max_norm)
    d.sumsq_parts = _dev(sumsq_parts, "sumsq_parts")
    return d


def train_step(basis, desc, params, grads, coords, t, X, y, idx, B, grad_scale, loss_sum, workspace, flags, optim,
               seed=0, loss_desc=None, sparsity_desc=None):
    """The whole single-GPU step in one call: forward, objective (+ first-layer sparsity penalties), backward,
    clip + AdamW + EMA."""
    _train("stdadk_train_step_f32", basis, desc, params, grads, coords, t, X, y,
           (_idx(idx, "train_step: idx")[0] if idx is not None else None, B), grad_scale, loss_desc, loss_sum,
           workspace, seed, flags, optim, sparsity_desc)


def _next_batch(nxt, y, workspace, what):
    """Trailing arguments of the doors that may bin the next batch, `nxt` = (next_idx, next_workspace) or None: its
    rows, the target columns, its workspace and the word the library answers in; returns (them, that word)."""
    done = C.c_int32(0)
    if nxt is None:
        return (None, 0, 0, None, 0, C.byref(done)), done
    if nxt[1].data_ptr() == workspace.data_ptr():
        raise RuntimeError(f"{what}: the next batch needs a workspace of its own")
    return _idx(nxt[0], f"{what}: next_idx") + (y.shape[1] if y is not None else 0,) + _ws(nxt[1]) \
        + (C.byref(done),), done


def train_step_next(basis, desc, params, grads, coords_all, t_all, X_all, y_all, idx, grad_scale, loss_sum, workspace,
                    flags, optim, next_idx, next_workspace, seed=0, loss_desc=None, sparsity_desc=None):
    """train_step on rows `idx` of the resident arrays whose optimiser launch also bins rows `next_idx` into
    `next_workspace` (stdadk_train_step_next_f32).  Returns True when the next batch was binned (step on
    next_workspace with FLAG_PREBINNED then), False when nothing was prepared."""
    rows = _idx(idx, "train_step_next: idx")
    tail, done = _next_batch((next_idx, next_workspace), y_all, workspace, "train_step_next")
    _train("stdadk_train_step_next_f32", basis, desc, params, grads, coords_all, t_all, X_all, y_all, rows, grad_scale,
           loss_desc, loss_sum, workspace, seed, flags, optim, sparsity_desc, tail)
    return bool(done.value)


def train_step_knots(basis, desc, params, grads, coords, t, X, y, idx, B, grad_scale, loss_sum, workspace, flags, optim,
                     knot_train, d_centers, d_log_bw, knots, nxt=None, seed=0, loss_desc=None, sparsity_desc=None):
    """The whole single-GPU step of a learnable-knot model in one call (stdadk_train_step_knots_f32): forward, objective,
    backward, knot gradients + penalties, both clip norms, AdamW + EMA of both parameter groups.  `optim` (make_optim)
    describes the MLP group and the shared hyper-parameters, `knots` (make_adam_group) the knot group; `idx` may be None
    (rows 0..B-1 of the given arrays).  `nxt` = (next_idx, next_workspace): the rows of the following step, binned by
    this step's weight-gradient launch when it can carry them.  Returns True when it did (step on next_workspace with
    FLAG_PREBINNED then), False when nothing was prepared."""
    rows = (_idx(idx, "train_step_knots: idx")[0] if idx is not None else None, B)
    tail, done = _next_batch(nxt, y, workspace, "train_step_knots")
    tail += (_ref(knot_train), _dev(d_centers, "d_centers"), _dev(d_log_bw, "d_log_bw"), C.byref(knots))
    _train("stdadk_train_step_knots_f32", basis, desc, params, grads, coords, t, X, y, rows, grad_scale, loss_desc,
           loss_sum, workspace, seed, flags, optim, sparsity_desc, tail)
    return bool(done.value)


def make_delta_step(delta, d_delta, lambda_grad, lambda_loss):
    """stdadk_delta_step for the delta matrix [Q, ldd] and its rows of the flat gradient (same stride)."""
    h = DeltaStep()
    h.delta, h.ldd = _rows(delta, "delta", delta.shape[1])
    h.d_delta, h.ldg = _rows(d_delta, "d_delta", delta.shape[1])
    h.lambda_grad, h.lambda_loss = float(lambda_grad), float(lambda_loss)
    return h


def train_step_delta(basis, desc, params, grads, coords, t, X, y, idx, B, grad_scale, loss_sum, workspace, flags, optim,
                     head, knot_train=None, d_centers=None, d_log_bw=None, knots=None, nxt=None, seed=0, loss_desc=None,
                     sparsity_desc=None):
    """The whole single-GPU step of a model with the delta head in one call (stdadk_train_step_delta_f32): derived
    output layer, forward, objective, backward, the head's fold with P_nc(delta), [knot gradients + penalties,] clip
    norm(s), AdamW + EMA.  `head` (make_delta_step); `knots` None: fixed knots, one parameter group, else the two-group
    form of train_step_knots.  `nxt` and the return value as there."""
    rows = (_idx(idx, "train_step_delta: idx")[0] if idx is not None else None, B)
    tail, done = _next_batch(nxt, y, workspace, "train_step_delta")
    tail += (_ref(knot_train), _dev(d_centers, "d_centers"), _dev(d_log_bw, "d_log_bw"),
             C.byref(knots) if knots is not None else None, _ref(head))
    _train("stdadk_train_step_delta_f32", basis, desc, params, grads, coords, t, X, y, rows, grad_scale, loss_desc,
           loss_sum, workspace, seed, flags, optim, sparsity_desc, tail)
    return bool(done.value)


def sumsq2(g0, parts0, g1, parts1, step_inc=None):
    """stdadk_sumsq_f32 on two gradient buffers in one launch (step_inc advanced once)."""
    if parts0.numel() != SUMSQ_PARTS or parts1.numel() != SUMSQ_PARTS:
        raise RuntimeError(f"sumsq2: parts must hold {SUMSQ_PARTS} floats each")
    rc = lib().stdadk_sumsq2_f32(_dev(g0, "g0"), g0.numel(), _dev(parts0, "parts0"), _dev(g1, "g1"), g1.numel(),
                                 _dev(parts1, "parts1"), _dev(step_inc, "step_inc"), _stream())
    _check(rc, "stdadk_sumsq2_f32")


def make_adam_group(p, g, m, v, ema, lr, lr_dev=None, max_norm=0.0, sumsq_parts=None, shadow=None):
    gr = _fill_group(AdamGroup(), p, g, m, v, ema, lr, lr_dev, max_norm, sumsq_parts, shadow)
    gr.n_parts = 0 if sumsq_parts is None else sumsq_parts.numel()
    return gr


def adamw_ema2(group0, group1, betas, eps, weight_decay, step, grad_mul=1.0, ema_decay=0.0, step_dev=None,
               loss_watch=None, nonfinite_step=None):
    """stdadk_adamw_ema_f32 on two parameter groups (make_adam_group) in one launch."""
    rc = lib().stdadk_adamw_ema2_f32(C.byref(group0), C.byref(group1), betas[0], betas[1], eps, weight_decay,
                                     int(step), _dev(step_dev, "step_dev"), grad_mul, ema_decay,
                                     _dev(loss_watch, "loss_watch"), _dev(nonfinite_step, "nonfinite_step"), _stream())
    _check(rc, "stdadk_adamw_ema2_f32")


def profile_enable(on=True):
    """Bracket every kernel launch of the library with HIP events (measurement aid)."""
    lib().stdadk_profile_enable(int(on))


def profile_collect():
    """[(kernel name, milliseconds)] per launch since profile_enable(True), in launch order."""
    need = lib().stdadk_profile_collect(None, 0)
    if need < 0:
        raise RuntimeError("stdadk_profile_collect failed")
    buf = C.create_string_buffer(int(need) + 16)
    lib().stdadk_profile_collect(buf, len(buf))
    out = []
    for line in buf.value.decode().splitlines():
        name, ms = line.rsplit("\t", 1)
        out.append((name, float(ms)))
    return out
