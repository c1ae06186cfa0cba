"""ctypes binding of libbuctd_hip.so (the C ABI declared in include/buctd_hip.h).

The library is the only compute back end of the package: there is no CPU or eager
PyTorch fallback.  Importing this module without the built library, or calling an op
with tensors that are not on a ROCm device, raises.

torch is imported first on purpose: the shared object depends on libamdhip64.so.7 by
SONAME, and the dynamic loader then binds it to the HIP runtime PyTorch already loaded,
so device pointers and streams are shared with the caching allocator.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbuctd_hip.so")
# The product loader reads no environment.  Experiments that need another build of the same sources go through
# scratch/run_alt.py, which sets LIB_PATH before the first lib() call.


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "H", "W", "Ci", "Co", "R", "S", "stride", "pad", "Ho", "Wo")]


class BasicBlockDesc(C.Structure):     # mirrors buctd_basic_block
    _fields_ = ([(n, C.c_int) for n in ("N", "H", "W", "C")] +
                [(n, C.c_void_p) for n in ("x", "w1_fwd", "w2_fwd", "w1_bwd", "w2_bwd", "gamma1", "beta1", "gamma2", "beta2",
                                           "running_mean1", "running_var1", "running_mean2", "running_var2")] +
                [(n, C.c_float) for n in ("eps1", "momentum1", "eps2", "momentum2")] +
                [(n, C.c_void_p) for n in ("z1", "z2", "y", "acc", "stat")])


class BasicBlockGrads(C.Structure):    # mirrors buctd_basic_block_grads
    _fields_ = ([(n, C.c_void_p) for n in ("dy", "dz2", "dres", "dy1", "dz1", "dx", "dw1", "dw2", "dgamma1", "dbeta1",
                                           "dgamma2", "dbeta2")] +
                [(n, C.c_int) for n in ("acc_w1", "acc_w2", "acc_bn1", "acc_bn2")] +
                [("bn_acc", C.c_void_p), ("wg_ws", C.c_void_p), ("wg_ws_bytes", C.c_size_t)])


class BnAccIn(C.Structure):            # mirrors buctd_bn_acc_in
    _fields_ = [("acc", C.c_void_p), ("rows", C.c_long), ("eps", C.c_float), ("momentum", C.c_float),
                ("mean_out", C.c_void_p), ("invstd_out", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p)]


class C3Conv(C.Structure):             # mirrors buctd_c3_conv
    _fields_ = ([(n, C.c_int) for n in ("N", "H", "W", "Ci", "Co")] +
                [(n, C.c_void_p) for n in ("x", "wprep", "residual")] + [("relu", C.c_int)] +
                [(n, C.c_void_p) for n in ("y", "stats_acc")] + [("in_bn", C.POINTER(BnAccIn))] +
                [(n, C.c_void_p) for n in ("in_gamma", "in_beta")] + [("in_relu", C.c_int)] +
                [(n, C.c_void_p) for n in ("bn_z", "bn_y", "bn_mean", "bn_invstd", "bn_gamma", "bn_beta", "bn_acc")])


class C3ConvEval(C.Structure):         # mirrors buctd_c3_conv_eval
    _fields_ = ([(n, C.c_int) for n in ("N", "H", "W", "Ci", "Co")] +
                [(n, C.c_void_p) for n in ("x", "wprep", "scale", "shift", "residual")] + [("relu", C.c_int), ("y", C.c_void_p)])


class BnApplyItem(C.Structure):        # mirrors buctd_bn_apply_item
    _fields_ = [("z", C.c_void_p), ("st", BnAccIn), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("residual", C.c_void_p),
                ("relu", C.c_int), ("y", C.c_void_p), ("rows", C.c_long), ("C", C.c_int)]


class BnBwdItem(C.Structure):          # mirrors buctd_bn_bwd_item
    _fields_ = ([(n, C.c_void_p) for n in ("dy", "y", "z", "mean", "invstd", "gamma", "beta")] +
                [("relu", C.c_int), ("rows", C.c_long), ("C", C.c_int)] +
                [(n, C.c_void_p) for n in ("dz", "dres", "dgamma", "dbeta")] +
                [("accumulate", C.c_int), ("acc", C.c_void_p), ("acc_ready", C.c_int)])


class Wg3Conv(C.Structure):            # mirrors buctd_wg3_conv
    _fields_ = ([(n, C.c_int) for n in ("N", "H", "W", "Ci", "Co")] +
                [(n, C.c_void_p) for n in ("x", "dy", "dw")] + [("accumulate", C.c_int)] +
                [(n, C.c_void_p) for n in ("x_mean", "x_invstd", "x_gamma", "x_beta")] + [("x_relu", C.c_int)] +
                [("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)])


class MhaArgs(C.Structure):            # mirrors buctd_mha_args
    _fields_ = ([(n, C.c_int) for n in ("B", "T", "h", "dh")] +
                [(n, C.c_void_p) for n in ("q", "k", "v")] + [(n, C.c_int) for n in ("ldq", "ldk", "ldv")] +
                [("out", C.c_void_p), ("ldo", C.c_int), ("lse", C.c_void_p), ("scale", C.c_float), ("p_drop", C.c_float),
                 ("dout", C.c_void_p), ("lddo", C.c_int)] +
                [(n, C.c_void_p) for n in ("dq", "dk", "dv")] + [(n, C.c_int) for n in ("lddq", "lddk", "lddv")])


class AttnRowsArgs(C.Structure):       # mirrors buctd_attn_rows_args
    _fields_ = ([(n, C.c_int) for n in ("B", "T", "h", "dh", "R")] + [("q", C.c_void_p), ("k", C.c_void_p)] +
                [("ldq", C.c_int), ("ldk", C.c_int), ("rows", C.c_void_p), ("scale", C.c_float), ("out", C.c_void_p),
                 ("out_heads", C.c_void_p)])


class RefineArgs(C.Structure):          # mirrors buctd_refine_args
    _fields_ = ([(n, C.c_void_p) for n in ("coords", "maxvals", "offset", "center", "scale", "box_score", "items",
                                           "cond_trunc", "cond_joints", "status", "hist_preds", "hist_score",
                                           "hist_box_score", "hist_keypoint_score", "hist_center", "hist_scale")] +
                [(n, C.c_int) for n in ("B", "K", "pass_", "passes", "heatmap_w", "heatmap_h", "crop_w", "crop_h")] +
                [(n, C.c_double) for n in ("margin", "aspect_ratio", "in_vis_thre", "scale_thre")])


class TrackArgs(C.Structure):           # mirrors buctd_track_args
    _fields_ = ([(n, C.c_void_p) for n in ("coords", "maxvals", "offset", "ids", "misses", "next_id", "pose", "center",
                                           "scale", "items", "cond_trunc", "dets", "det_offsets", "frame_src", "sigmas",
                                           "hist_ids", "hist_preds", "hist_score", "hist_born", "hist_died")] +
                [(n, C.c_int) for n in ("M", "K", "frame", "frames", "max_dets", "max_misses", "heatmap_w", "heatmap_h",
                                        "crop_w", "crop_h")] +
                [(n, C.c_double) for n in ("margin", "aspect_ratio", "in_vis_thre", "scale_thre", "birth_oks", "merge_oks",
                                           "death_score")])


class SampleGeomArgs(C.Structure):      # mirrors buctd_sample_geom_args
    _fields_ = ([(n, C.c_void_p) for n in ("joints", "joints_vis", "cond", "cond_vis", "center", "scale", "bbox",
                                           "half_body", "draws", "bbox_draws", "flags", "pair", "items", "out_joints",
                                           "out_joints_vis", "out_cond", "out_cond_vis", "cond_trunc", "target_xy",
                                           "target_vis", "out_center", "out_scale", "out_rotation", "status")] +
                [(n, C.c_int) for n in ("B", "K", "crop_w", "crop_h", "keep_rect", "bbox_aug")] +
                [(n, C.c_double) for n in ("margin", "aspect_ratio", "scale_thre", "stride_x", "stride_y")])


class KptMatchArgs(C.Structure):        # mirrors buctd_kpt_match_args
    _fields_ = ([(n, C.c_int) for n in ("images", "K", "n_thr", "n_area")] + [(n, C.c_long) for n in ("dt_total", "gt_total")] +
                [(n, C.c_void_p) for n in ("dt_offsets", "gt_offsets", "oks_offsets", "dt_kpts", "gt_kpts", "gt_area",
                                           "gt_bbox", "gt_flags", "sigmas", "thresholds", "area_ranges", "oks",
                                           "dt_matched", "dt_ignored")])


class VisCanvas(C.Structure):           # mirrors buctd_vis_canvas (one row of the canvas table in device memory)
    _fields_ = [("base", C.c_void_p), ("row_stride", C.c_long), ("H", C.c_int), ("W", C.c_int)]


class VisPoseArgs(C.Structure):         # mirrors buctd_vis_pose_args
    _fields_ = ([(n, C.c_void_p) for n in ("canvases", "person_offsets", "persons", "joints", "skeleton", "palette",
                                           "tiles")] +
                [(n, C.c_int) for n in ("C", "P", "K", "L", "n_palette", "n_tiles", "canvas_h_max", "canvas_w_max",
                                        "style", "thickness", "radius")] +
                [("score_thresh", C.c_float), ("alpha256", C.c_int)])


# BUCTD_VIS_POSE_* of the header
VIS_POSE_PLAIN, VIS_POSE_PRETTY = 0, 1
VIS_POSE_TILE_W, VIS_POSE_TILE_H, VIS_POSE_CHUNK = 64, 16, 256


# BUCTD_GRAD_SUMSQ_CHUNK of the header: elements per partial sum of buctd_grad_sumsq
GRAD_SUMSQ_CHUNK = 8192

# BUCTD_STEP_MAX_GROUPS / BUCTD_STEP_CHUNK of the header: the grouped optimizer steps (csrc/optim_groups.hip)
STEP_MAX_GROUPS, STEP_CHUNK = 16, 16384


class StepChunk(C.Structure):           # mirrors buctd_step_chunk (16 bytes: one row of the chunk table in device memory)
    _fields_ = [("start", C.c_long), ("len", C.c_int), ("group", C.c_int)]


class AdamGroup(C.Structure):           # mirrors buctd_adam_group
    _fields_ = ([(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] +
                [("decoupled", C.c_int), ("step", C.c_int)])


class SgdGroup(C.Structure):            # mirrors buctd_sgd_group
    _fields_ = [(n, C.c_float) for n in ("lr", "momentum", "weight_decay")] + [("nesterov", C.c_int)]


class AvgItem(C.Structure):             # mirrors buctd_avg_item (24 bytes: one row of the item table in device memory)
    _fields_ = [("src", C.c_void_p), ("avg", C.c_void_p), ("n", C.c_long)]


class MatmulDesc(C.Structure):
    _fields_ = [
        ("batch", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("a_layout", C.c_int), ("b_layout", C.c_int),
        ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
        ("stride_a", C.c_long), ("stride_b", C.c_long), ("stride_c", C.c_long),
        ("Kc", C.c_int), ("group_stride_a", C.c_long), ("group_stride_bk", C.c_long),
        ("Nc", C.c_int), ("group_stride_bn", C.c_long), ("group_stride_c", C.c_long),
        ("alpha", C.c_float), ("bias_axis", C.c_int),
    ]


_P = C.c_void_p
_I = C.c_int
_L = C.c_long
_F = C.c_float
_D = C.c_double
_U64 = C.c_uint64
_SZ = C.c_size_t
_PD = C.POINTER(ConvDesc)
_PM = C.POINTER(MatmulDesc)
_PI = C.POINTER(C.c_int)
_PL = C.POINTER(C.c_long)

# name -> (restype, argtypes); mirrors include/buctd_hip.h one to one
SIGNATURES = {
    "buctd_version": (_I, []),
    "buctd_last_error": (C.c_char_p, []),
    "buctd_conv2d_fwd": (_I, [_PD, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "buctd_conv2d_fwd_thin": (_I, [_PD]),
    "buctd_conv2d_dgrad": (_I, [_PD, _P, _P, _P, _P, _P, _P]),
    "buctd_conv2d_stats_groups": (_I, [_PD, _I, _PI, _PI]),
    "buctd_conv2d_wgrad_workspace": (_SZ, [_PD]),
    "buctd_conv2d_wgrad": (_I, [_PD, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_conv2d_plan": (_I, [_PD, _I, _I, _PI]),
    "buctd_matmul_workspace": (_SZ, [_PM]),
    "buctd_matmul": (_I, [_PM, _P, _P, _P, _P, _P, _SZ, _P]),
    "buctd_matmul_plan": (_I, [_PM, _P, _P, _PI]),
    "buctd_bn_finalize": (_I, [_P, _P, _I, _I, _L, _I, _F, _F, _P, _P, _P, _P, _P]),
    "buctd_conv3x3_bf16x3_supported": (_I, [_I, _I, _I, _I, _I]),
    "buctd_conv3x3_bf16x3_stats_groups": (_I, [_I, _I, _I, _I, _I, _PI, _PI]),
    "buctd_conv3x3_bf16x3_prep_bytes": (_SZ, [_I, _I, _I]),
    "buctd_conv3x3_bf16x3_prep": (_I, [_I, _I, _P, _I, _P, _P]),
    "buctd_conv3x3_bf16x3_prep_batched": (_I, [_P, _I, _L, _P]),
    "buctd_conv3x3_bf16x3": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "buctd_conv3x3_wgrad_bf16x3_supported": (_I, [_I, _I, _I, _I, _I]),
    "buctd_conv3x3_wgrad_bf16x3_workspace": (_SZ, [_I, _I, _I, _I, _I]),
    "buctd_conv3x3_wgrad_bf16x3": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_conv3x3_bf16x6_supported": (_I, [_I, _I, _I, _I, _I]),
    "buctd_conv3x3_bf16x6_stats_groups": (_I, [_I, _I, _I, _I, _I, _PI, _PI]),
    "buctd_conv3x3_bf16x6_prep_bytes": (_SZ, [_I, _I, _I]),
    "buctd_conv3x3_bf16x6_prep": (_I, [_I, _I, _P, _I, _P, _P]),
    "buctd_conv3x3_bf16x6": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "buctd_bn_bwd_from_partials": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _P, _I, _P, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_conv3x3_wgrad_bf16x6_bnin": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_conv3x3_wgrad_bf16x6_supported": (_I, [_I, _I, _I, _I, _I]),
    "buctd_conv3x3_wgrad_bf16x6_workspace": (_SZ, [_I, _I, _I, _I, _I]),
    "buctd_conv3x3_wgrad_bf16x6": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_bn_stats": (_I, [_P, _L, _I, _P, _PI, _PI, _P]),
    "buctd_bn_stats_groups": (_I, [_L, _I, _PI, _PI]),
    "buctd_bn_apply": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _L, _I, _P]),
    "buctd_bn_bwd_workspace": (_SZ, [_L, _I]),
    "buctd_bn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _P, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_bn_fold": (_I, [_P, _P, _P, _P, _F, _I, _P, _P, _P]),
    "buctd_bn_acc_bytes": (_SZ, [_I]),
    "buctd_bn_apply_acc": (_I, [_P, C.POINTER(BnAccIn), _P, _P, _P, _I, _P, _L, _I, _P]),
    "buctd_bn_bwd_acc": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _P, _P, _P, _P, _I, _P, _I, _P]),
    "buctd_conv3x3_bf16x6_acc": (_I, [_I] * 5 + [_P, _P, _P, _I, _P, _P, C.POINTER(BnAccIn), _P, _P, _I, _P]),
    "buctd_conv3x3_bf16x6_bnstat_acc": (_I, [_I] * 5 + [_P] * 12),
    "buctd_gconv_x6_fwd_acc": (_I, [_I] * 6 + [_P] * 6),
    "buctd_conv3x3_bf16x6_group": (_I, [_I, C.POINTER(C3Conv), _P]),
    "buctd_conv3x3_bf16x6_group_eval": (_I, [_I, C.POINTER(C3ConvEval), _P]),
    "buctd_conv3x3_bf16x6_group_workgroups": (_I, [_I, C.POINTER(C3Conv)]),
    "buctd_conv3x3_bf16x6_group_plan": (_I, [_I, C.POINTER(C3Conv), C.POINTER(C.c_int)]),     # out[30]
    "buctd_conv3x3_bf16x6_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_int)]),
    "buctd_conv3x3_wgrad_bf16x6_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int)]),
    "buctd_gconv_wgrad_x6_supported": (_I, [_I] * 6),
    "buctd_gconv_wgrad_x6_plan": (_I, [_I] * 6 + [C.POINTER(C.c_int)]),
    "buctd_gconv_wgrad_x6_workspace": (_SZ, [_I] * 6),
    "buctd_gconv_wgrad_x6": (_I, [_I] * 6 + [_P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_bn_apply_acc_group": (_I, [_I, C.POINTER(BnApplyItem), _P]),
    "buctd_bn_bwd_acc_group": (_I, [_I, C.POINTER(BnBwdItem), _P]),
    "buctd_conv3x3_wgrad_bf16x6_group_workspace": (_SZ, [_I] * 6),
    "buctd_conv3x3_wgrad_bf16x6_group": (_I, [_I, C.POINTER(Wg3Conv), _P]),
    "buctd_conv3x3_wgrad_bf16x6_group_workgroups": (_I, [_I, C.POINTER(Wg3Conv)]),
    "buctd_conv3x3_wgrad_bf16x6_group_plan": (_I, [_I, C.POINTER(Wg3Conv), C.POINTER(C.c_int)]),  # out[34]
    "buctd_stream_fork": (_I, [_P, _P]),
    "buctd_basic_branches_fwd_train": (_I, [_I, _I, C.POINTER(BasicBlockDesc), _P]),
    "buctd_basic_branches_bwd": (_I, [_I, _I, C.POINTER(BasicBlockDesc), C.POINTER(BasicBlockGrads), _P, _P]),
    "buctd_basic_chain_fwd_train": (_I, [_I, C.POINTER(BasicBlockDesc), _P]),
    "buctd_basic_chain_bwd": (_I, [_I, C.POINTER(BasicBlockDesc), C.POINTER(BasicBlockGrads), _P, _P]),
    "buctd_x6_image_dims": (_I, [_I, _I, _I, _P, _P]),
    "buctd_x6_image_bytes": (C.c_size_t, [_I, _I, _I]),
    "buctd_x6_image": (_I, [_P, _I, _I, _I, _L, _L, _I, _L, _L, _I, _P, _P]),
    "buctd_x6_gemm": (_I, [_I, _I, _I, _P, _P, _P, _I, _F, _P, _L, _I, _L, _P]),
    "buctd_x6_gemm_plan": (_I, [_I, _I, _I, _PI]),
    "buctd_x6_gemm_tile": (_I, [_I, _I, _I, _I, _PI, _PI]),
    "buctd_x6_image_path": (_I, [_P, _I, _I, _I, _L, _L, _I, _L, _L, _I, _I, _I, _PI]),
    "buctd_add": (_I, [_P, _P, _P, _L, _I, _P]),
    "buctd_add_n": (_I, [C.POINTER(_P), _I, _P, _L, _P]),
    "buctd_mul": (_I, [_P, _P, _P, _L, _P]),
    "buctd_scale": (_I, [_P, _P, _F, _P, _L, _P]),
    "buctd_copy_channels": (_I, [_P, _L, _I, _I, _P, _I, _I, _I, _P]),
    "buctd_add_bcast": (_I, [_P, _P, _P, _L, _L, _P]),
    "buctd_batch_sum": (_I, [_P, _L, _L, _P, _I, _P]),
    "buctd_relu_bwd": (_I, [_P, _P, _P, _L, _P]),
    "buctd_colsum_workspace": (_SZ, [_L, _I]),
    "buctd_colsum": (_I, [_P, _L, _I, _P, _I, _P, _SZ, _P]),
    "buctd_nchw_to_nhwc": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "buctd_nhwc_to_nchw": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "buctd_fuse_sum": (_I, [C.POINTER(_P), _PI, _I, _I, _I, _I, _I, _I, _P, _P]),
    "buctd_fuse_sum_bwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "buctd_resize_bilinear": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "buctd_maxpool3x3s2_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "buctd_maxpool3x3s2_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "buctd_softmax_dropout_fwd": (_I, [_P, _L, _I, _F, _F, _U64, _P, _P, _P]),
    "buctd_softmax_dropout_bwd": (_I, [_P, _P, _L, _I, _F, _F, _U64, _P, _P]),
    "buctd_softmax_dropout_fwd_dseed": (_I, [_P, _L, _I, _F, _F, _P, _P, _P, _P]),
    "buctd_softmax_dropout_bwd_dseed": (_I, [_P, _P, _L, _I, _F, _F, _P, _P, _P]),
    "buctd_dropout": (_I, [_P, _P, _L, _F, _U64, _P]),
    "buctd_dropout_dseed": (_I, [_P, _P, _L, _F, _P, _P]),
    "buctd_dropout_seed_fill": (_I, [_P, _I, _U64, _U64, _P]),
    "buctd_attn_smallqk_supported": (_I, [_I, _I, _I]),
    "buctd_attn_smallqk_plan": (_I, [_I, _I, _I, _I, _F, _I, _PI]),
    "buctd_attn_smallqk_fwd": (_I, [_I, _I, _I, _I, _P, _P, _P, _F, _F, _U64, _I, _P, _P, _P, _P]),
    "buctd_attn_smallqk_bwd": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _U64, _I, _P, _P, _P, _P, _P]),
    "buctd_attn_smallqk_fwd_dseed": (_I, [_I, _I, _I, _I, _P, _P, _P, _F, _F, _P, _I, _P, _P, _P, _P]),
    "buctd_attn_smallqk_bwd_dseed": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, _I, _P, _P, _P, _P, _P]),
    "buctd_layernorm_fwd": (_I, [_P, _P, _P, _L, _I, _F, _P, _P, _P, _P]),
    "buctd_add_layernorm_fwd": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, _P]),
    "buctd_layernorm_bwd_workspace": (_SZ, [_L, _I]),
    "buctd_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _I, _P, _SZ, _P]),
    "buctd_joints_mse": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _F, _P, _SZ, _P]),
    "buctd_joints_ohkm_mse_workspace": (_SZ, [_I, _I]),
    "buctd_joints_ohkm_mse": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _F, _P, _SZ, _P]),
    "buctd_argmax_decode": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "buctd_warp_affine_norm": (_I, [_P, _I, _I, _I, _P, _P, _P, _L, _P, _P]),
    "buctd_cond_render_into": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P, _SZ, _P]),
    "buctd_cond_geometry": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "buctd_cond_mirror": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P]),
    "buctd_mirror_rows": (_I, [_P, _L, _P, _L, _P, _I, _I, _I, _I, _I, _P]),
    "buctd_refine_step": (_I, [C.POINTER(RefineArgs), _P]),
    "buctd_track_step": (_I, [C.POINTER(TrackArgs), _P]),
    "buctd_sample_geometry": (_I, [C.POINTER(SampleGeomArgs), _P]),
    "buctd_synthesize_pose": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, C.c_ulonglong, _P, _P]),
    "buctd_pose_error_types": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "buctd_gconv_x6_supported": (_I, [_I] * 7),
    "buctd_gconv_x6_prep_bytes": (_SZ, [_I, _I, _I, _I]),
    "buctd_gconv_x6_prep": (_I, [_I, _I, _I, _P, _I, _P, _P]),
    "buctd_gconv_x6_prep_item_bytes": (_SZ, []),
    "buctd_gconv_x6_prep_item": (_I, [_I, _I, _I, _P, _I, _P, _P]),
    "buctd_gconv_x6_prep_batched": (_I, [_P, _I, _P]),
    "buctd_gconv_x6_stats_groups": (_I, [_I] * 6 + [_PI, _PI]),
    "buctd_gconv_x6_fwd": (_I, [_I] * 6 + [_P] * 6 + [_I, _P, _P, _P, _P]),
    "buctd_gconv_x6_dgrad": (_I, [_I] * 6 + [_P] * 4 + [_P]),
    "buctd_gconv_x6_plan": (_I, [_I] * 8 + [C.POINTER(C.c_int)]),
    "buctd_mha_fwd_bf16x6_workspace": (_SZ, [_I, _I, _I]),
    "buctd_mha_heads_fwd_bf16x6_ws": (_I, [C.POINTER(MhaArgs), _P, _SZ, _P]),
    "buctd_mha_heads_fwd_supported": (_I, [_I, _I, _I]),
    "buctd_mha_heads_fwd": (_I, [C.POINTER(MhaArgs), _P]),
    "buctd_mha_heads_fwd_bf16x6": (_I, [C.POINTER(MhaArgs), _P]),
    "buctd_mha_heads_train_supported": (_I, [_I, _I, _I]),
    "buctd_mha_heads_fwd_train": (_I, [C.POINTER(MhaArgs), _U64, _P]),
    "buctd_mha_heads_bwd_workspace": (_SZ, [_I, _I, _I]),
    "buctd_mha_heads_bwd": (_I, [C.POINTER(MhaArgs), _U64, _P, _SZ, _P]),
    "buctd_mha_heads_fwd_train_dseed": (_I, [C.POINTER(MhaArgs), _P, _P]),
    "buctd_mha_heads_bwd_dseed": (_I, [C.POINTER(MhaArgs), _P, _P, _SZ, _P]),
    "buctd_attn_rows_supported": (_I, [_I, _I, _I]),
    "buctd_attn_rows": (_I, [C.POINTER(AttnRowsArgs), _P]),
    "buctd_nms_workspace": (_SZ, [_I]),
    "buctd_nms": (_I, [_P, _P, _P, _I, _I, _F, _P, _SZ, _P]),
    "buctd_cpu_nms": (_I, [_P, _I, _P, _F, _P, _P]),
    "buctd_kpt_rescore": (_I, [_P, _P, _I, _I, _D, _P, _P, _P, _P]),
    "buctd_oks_nms_grouped": (_I, [_P, _I, _I, _P, _P, _P, _I, _D, _I, _D, _P, _P]),
    "buctd_soft_oks_nms_grouped": (_I, [_P, _I, _P, _P, _P, _P, _I, _D, _I, _I, _D, _I, _P, _P, _P]),
    "buctd_oks_merge_grouped": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _D, _I, _D, _P, _P, _P, _P]),
    "buctd_coco_kpt_match_workspace": (_SZ, [_L, _I, _I]),
    "buctd_coco_kpt_match": (_I, [C.POINTER(KptMatchArgs), _P, _SZ, _P]),
    "buctd_kpt_crowding": (_I, [_P, _I, _L, _I, _P, _P, _P, _P, _D, _P, _P, _P]),
    "buctd_kpt_segment_ap": (_I, [_P, _I, _I, _L, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P]),
    # condition records (csrc/conditions.hip)
    "buctd_pose_boxes": (_I, [_P, _I, _I, _I, _P, _D, _P, _P, _P]),
    "buctd_match_boxes": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "buctd_group_max_iou": (_I, [_P, _I, _P, _I, _P, _P, _P, _P]),
    "buctd_group_near_list": (_I, [_P, _I, _P, _P, _P, _P]),
    # debug pictures (csrc/vis.hip)
    "buctd_vis_minmax": (_I, [_P, _I, _I, _I, _L, _L, _L, _L, _P, _P]),
    "buctd_vis_heatmap_grid": (_I, [_P, _I, _I, _I, _L, _L, _L, _L, _P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "buctd_vis_joint_grid": (_I, [_P, _I, _I, _I, _L, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    # pose overlays (csrc/vis_pose.hip)
    "buctd_vis_pose_overlay": (_I, [C.POINTER(VisPoseArgs), _P]),
    "buctd_argmax_decode_refined": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "buctd_argmax_decode_dark": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "buctd_gaussian_target": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _F, _P, _P, _P]),
    "buctd_cond_render_workspace": (_SZ, [_I, _I, _I, _I]),
    "buctd_cond_render": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    "buctd_flipback_avg": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "buctd_sgd_step": (_I, [_P, _P, _P, _L, _F, _F, _F, _I, _I, _F, _P]),
    "buctd_adam_step": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _I, _F, _P]),
    "buctd_sgd_step_dscale": (_I, [_P, _P, _P, _L, _F, _F, _F, _I, _I, _F, _P, _P]),
    "buctd_adam_step_dscale": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _I, _F, _P, _P]),
    # parameter groups (csrc/optim_groups.hip); runs, run groups and the group table are host arrays, the chunk table is
    # a host array for buctd_step_chunks and device memory for the two steps
    "buctd_step_chunks": (_L, [_PL, _PI, _I, C.POINTER(StepChunk)]),
    "buctd_adam_step_groups": (_I, [_P, _P, _P, _P, _P, _L, C.POINTER(AdamGroup), _I, _F, _P, _P]),
    "buctd_sgd_step_groups": (_I, [_P, _P, _P, _P, _L, C.POINTER(SgdGroup), _I, _F, _P, _P]),
    # gradient-norm clipping (csrc/grad_norm.hip); runs: a host array of longs, spans: a device one
    "buctd_grad_sumsq_workspace": (_SZ, [_PL, _I]),
    "buctd_grad_sumsq": (_I, [_P, _PL, _I, _P, _P, _SZ, _P]),
    "buctd_grad_clip_coef": (_I, [_P, _D, _D, _P, _P, _P]),
    "buctd_grad_segment_stats": (_I, [_P, _P, _I, _P, _P, _P]),
    # weight averaging (csrc/weight_avg.hip); the item table of buctd_ema_update_tensors is device memory
    "buctd_ema_update": (_I, [_P, _P, _L, _F, _P]),
    "buctd_ema_update_tensors": (_I, [_P, _I, _F, _P]),
    "buctd_swap": (_I, [_P, _P, _L, _P]),
    # bf16 inference mode (csrc/conv_bf16.hip)
    "buctd_bf16_pack_conv": (_I, [_P, _L, _L, _L, _L, _I, _I, _I, _P, _P, _P, _P, _P, _F, _P, _P, _P]),
    "buctd_bf16_conv": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _SZ, _P]),
    "buctd_bf16_fuse_sum": (_I, [C.POINTER(_P), _PI, _I, _I, _I, _I, _I, _I, _P, _P]),
    "buctd_bf16_from_f32": (_I, [_P, _L, _P, _P]),
}

_lib = None


class BuctdHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise BuctdHipError(
                f"{LIB_PATH} is missing - build it with `make` (or __graft_entry__.build()); "
                "buctd_amd has no CPU / eager fallback")
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().buctd_last_error()
        raise BuctdHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def current_stream_handle():
    """Raw hipStream_t of torch's current stream as an int.  torch.cuda.current_stream() builds a Stream object through
    several Python layers (~8 us); with ~4000 kernel launches per train step that alone was a third of the host time."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def stream_ptr():
    """hipStream_t of the current stream as a plain int (every bound function declares c_void_p argtypes: ctypes converts
    an int itself; building a c_void_p object per argument cost ~2 ms of host time per train step)."""
    return current_stream_handle()


def ptr(t):
    """Device pointer (plain int) of a contiguous fp32 (or int32) ROCm tensor, None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise BuctdHipError("buctd_amd ops need tensors on the ROCm device (no CPU path)")
    return t.data_ptr()
