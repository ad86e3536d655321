"""ctypes binding of libpbd_hip.so (include/pbd_c.h).

The library is the product; this module only marshals numpy arrays / device
pointers into it.  There is NO CPU fallback: if the shared object is missing
the import of `lib()` raises, and `pbd_create` fails on a box without a GPU.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
import weakref

import numpy as np

from .model import pbd_model_desc

_HERE = os.path.dirname(os.path.abspath(__file__))
# PBD_LIBRARY: load another build of the same ABI (tests/tools_*.py point it at libpbd_hip_probes.so, the
# `make probes` build with per-phase stamps and environment tuning knobs compiled in)
LIB_PATH = os.environ.get("PBD_LIBRARY") or os.path.join(_HERE, "libpbd_hip.so")

PBD_OK, PBD_ERR_ARG, PBD_ERR_UNSUPPORTED, PBD_ERR_CAPACITY, PBD_ERR_HIP, PBD_ERR_STATE, PBD_ERR_RCCL = range(7)
PBD_GATHER_AUTO, PBD_GATHER_HOST, PBD_GATHER_RCCL = 0, 1, 2
PBD_CONV_AUTO, PBD_CONV_EXACT, PBD_CONV_MFMA, PBD_CONV_SPLIT, PBD_CONV_SPLIT_F16 = 0, 1, 2, 3, 4
PBD_SCALAR_F32, PBD_SCALAR_F64 = 0, 1
PBD_CAND_RAW, PBD_CAND_SORT, PBD_CAND_SORT_NMS = 0, 1, 2   # pbd_set_candidate_filter: detect's output / Candidate::sort / sort + NMS
PBD_NMS_PAINTED, PBD_NMS_PARTS = 0, 1   # pbd_set_candidate_nms: the NMS of PBD_CAND_SORT_NMS — Candidate::nonMaximaSuppression / nms.m's part-wise rule
PBD_DEPTH_8U, PBD_DEPTH_16U, PBD_DEPTH_32F, PBD_DEPTH_64F = 0, 2, 5, 6          # cv::Mat::depth() (src/HOGFeatures.cpp:136-146)
PBD_GT_MAX = 64   # gt boxes per frame of the pbd_detect_gtbox_* entries and the pbd_candidates_best_overlap / _select_gt primitives
PBD_PYRAMID_OPENCV, PBD_PYRAMID_MATLAB = 0, 1   # pbd_set_pyramid_kind: HOGFeatures<T>::pyramid (cv::resize / cv::pyrDown) / matlab/detection/featpyramid.m
DEPTH_OF = {np.dtype(np.uint8): PBD_DEPTH_8U, np.dtype(np.uint16): PBD_DEPTH_16U, np.dtype(np.float32): PBD_DEPTH_32F,
            np.dtype(np.float64): PBD_DEPTH_64F}

EXPORTS = [
    "pbd_create", "pbd_destroy", "pbd_last_error", "pbd_max_parts", "pbd_set_stream",
    "pbd_detect_u8", "pbd_detect_dev_u8", "pbd_detect_enqueue_dev_u8", "pbd_detect_collect",
    "pbd_pyramid_geometry", "pbd_pyramid_u8", "pbd_get_level_image", "pbd_get_level_features",
    "pbd_set_level_features", "pbd_begin_frame", "pbd_pdf", "pbd_get_level_response",
    "pbd_set_level_response", "pbd_dp_min", "pbd_get_dp_pointers", "pbd_get_root", "pbd_dp_argmin",
    "pbd_dt2d", "pbd_hog_u8", "pbd_resize_u8", "pbd_pyrdown_u8", "pbd_nms_map",
    "pbd_set_levels", "pbd_get_level_features_f64", "pbd_set_level_features_f64", "pbd_get_level_response_f64",
    "pbd_set_level_response_f64", "pbd_get_root_f64", "pbd_dt2d_f64", "pbd_hog_u8_f64",
    "pbd_candidates_sort", "pbd_candidates_nms", "pbd_get_stage_ms", "pbd_set_profiling",
    "pbd_detect_enqueue_u8", "pbd_group_create", "pbd_group_destroy", "pbd_group_last_error", "pbd_group_size",
    "pbd_group_gather_mode", "pbd_group_member", "pbd_group_detect_batch_u8", "pbd_group_detect_u8",
    "pbd_get_work", "pbd_dp_timer", "pbd_debug_dt_stamps", "pbd_debug_dt_counters", "pbd_debug_hog_stamps", "pbd_debug_conv_stamps",
    "pbd_set_root", "pbd_set_root_f64", "pbd_set_dp_pointers", "pbd_get_footprint", "pbd_abi_version",
    "pbd_detect_batch_u8", "pbd_detect_batch_enqueue_u8", "pbd_detect_batch_enqueue_dev_u8", "pbd_detect_batch_collect",
    "pbd_get_stage_state", "pbd_get_conv_mode", "pbd_group_comm_size",
    "pbd_detect_image", "pbd_pyramid_image", "pbd_get_level_image_raw", "pbd_tune_plan",
    "pbd_create_sized", "pbd_group_create_sized", "pbd_get_filter_size",
    "pbd_set_candidate_filter", "pbd_group_set_candidate_filter", "pbd_candidates_filter",
    "pbd_set_depth_filter", "pbd_detect_rgbd_u8", "pbd_detect_rgbd_enqueue_dev_u8", "pbd_detect_batch_rgbd_u8",
    "pbd_detect_batch_rgbd_enqueue_dev_u8", "pbd_candidates_depth_filter",
    "pbd_set_box3d", "pbd_get_box3d", "pbd_candidates_box3d",
    "pbd_set_cluster3d", "pbd_get_cluster3d", "pbd_candidates_cluster3d",
    "pbd_set_part_scores", "pbd_get_part_scores", "pbd_candidates_part_scores",
    "pbd_set_boundary_pad", "pbd_get_boundary_pad", "pbd_group_set_boundary_pad",
    "pbd_get_frame_level_image_raw", "pbd_get_frame_level_features", "pbd_get_frame_level_features_f64",
    "pbd_get_frame_dp_pointers",
    "pbd_latent_mask", "pbd_dp_argbest", "pbd_detect_latent_u8", "pbd_detect_latent_dev_u8", "pbd_detect_batch_latent_u8",
    "pbd_feature_window_max", "pbd_candidates_features", "pbd_candidates_features_f64", "pbd_candidates_features_dev",
    "pbd_candidates_nms_parts", "pbd_set_candidate_nms", "pbd_group_set_candidate_nms", "pbd_candidates_filter_parts",
    "pbd_set_pyramid_kind", "pbd_get_pyramid_kind", "pbd_resize_area_f64", "pbd_reduce_f64",
    "pbd_candidates_best_overlap", "pbd_candidates_select_gt", "pbd_detect_gtbox_u8", "pbd_detect_gtbox_dev_u8",
    "pbd_detect_batch_gtbox_u8",
    "pbd_qp_create", "pbd_qp_destroy", "pbd_qp_dims", "pbd_qp_footprint", "pbd_qp_write", "pbd_qp_score", "pbd_qp_score_dev",
    "pbd_qp_lincomb", "pbd_qp_lincomb_dev", "pbd_qp_keep", "pbd_qp_get", "pbd_qp_put",
    "pbd_qp_noneg", "pbd_qp_fix", "pbd_qp_state_put", "pbd_qp_state_get", "pbd_qp_pass", "pbd_qp_one", "pbd_qp_refresh",
    "pbd_qp_loss", "pbd_qp_opt", "pbd_qp_prune", "pbd_qp_weights",
    "pbd_warp_geometry", "pbd_warp_taps", "pbd_warp_windows_u8", "pbd_warp_windows_u8_f64", "pbd_qp_write_warped_u8",
    "pbd_debug_warp_ms",
    "pbd_set_weights", "pbd_set_weights_dev", "pbd_get_weights", "pbd_qp_apply_weights", "pbd_set_threshold", "pbd_get_threshold",
    "pbd_qp_mine_u8", "pbd_qp_mine_dev_u8", "pbd_qp_mine_batch_u8",
    "pbd_qp_write_latent_u8", "pbd_qp_write_latent_dev_u8", "pbd_qp_write_latent_batch_u8", "pbd_croppos",
    "pbd_eval_keypoint_dist", "pbd_eval_pck_host", "pbd_eval_apk_match_host", "pbd_eval_ap_host",
    "pbd_eval_create", "pbd_eval_destroy", "pbd_eval_reset", "pbd_eval_dims", "pbd_eval_get", "pbd_eval_add_pck_records",
    "pbd_eval_add_apk_records", "pbd_eval_pck_frame_u8", "pbd_eval_pck_frame_batch_u8", "pbd_eval_apk_frame_u8",
    "pbd_eval_apk_frame_batch_u8", "pbd_eval_pck", "pbd_eval_apk",
    "pbd_kmeans_host", "pbd_cluster_parts_host", "pbd_cluster_parts",
    "pbd_set_interval", "pbd_get_interval", "pbd_qp_clear", "pbd_qp_positive_threshold",
    "pbd_pyrstore_create", "pbd_pyrstore_destroy", "pbd_pyrstore_dims", "pbd_pyrstore_slot", "pbd_pyrstore_layout",
    "pbd_pyrstore_put_u8", "pbd_pyrstore_put_dev_u8", "pbd_pyrstore_put_batch_u8", "pbd_pyrstore_get_level",
    "pbd_detect_stored", "pbd_detect_batch_stored", "pbd_qp_mine_stored", "pbd_qp_mine_batch_stored",
    "pbd_rotate_geometry", "pbd_map_rotate_points", "pbd_flip_points", "pbd_augment_host_u8", "pbd_augment_u8", "pbd_augment_dev_u8",
    "pbd_augment_last_error", "pbd_qp_write_warped_dev_u8",
    "pbd_debug_live_allocs",
]
# include/pbd_c.h "virtual positives"
PBD_ROT_ORI2NEW, PBD_ROT_NEW2ORI = 0, 1
PBD_ROT_NEAREST, PBD_ROT_BILINEAR = 0, 1
PBD_AUGMENT_MAX_OPS, PBD_AUGMENT_MAX_SIDE = 64, 16384
PBD_PYRSTORE_MAX_LEVELS = 128   # room pbd_pyrstore_layout's level_off needs
PBD_CLUSTER_MAX_K, PBD_CLUSTER_MAX_ITER, PBD_CLUSTER_MAX_TRIALS, PBD_CLUSTER_MAX_LABELS = 32, 10000, 2 ** 20, 2 ** 31 - 1   # include/pbd_c.h "part mixtures"
PBD_EVAL_SCALE_LAST, PBD_EVAL_SCALE_OWN = 0, 1   # pbd_eval_pck's scale rule: eval_pck.m:13 literally (the last instance's scale) / each instance's own
PBD_MINE_NONE, PBD_MINE_ONE, PBD_MINE_OPT = 0, 1, 2   # pbd_qp_mine_*'s action (detect.m:148-149, 315-324)
PBD_WARP_SKIPPED, PBD_WARP_WRITTEN, PBD_WARP_FULL = 0, 1, 2   # pbd_qp_write_warped_u8's status per box
QP_THRESH_BLOCK = 256   # lanes of a workgroup of k_qp_thresh.hip (QT_NT): pbd_qp_positive_threshold ranks that many scores per round
PBD_ABI_VERSION = 5


class pbd_options(C.Structure):
    _fields_ = [("device", C.c_int32), ("conv_mode", C.c_int32), ("max_candidates", C.c_int32),
                ("dt_correct_ptr", C.c_int32), ("level_begin", C.c_int32), ("level_end", C.c_int32),
                ("scalar_type", C.c_int32), ("graph", C.c_int32), ("reserved", C.c_int32 * 2)]


class pbd_augment_op(C.Structure):
    """one virtual copy of a frame (include/pbd_c.h "virtual positives"): the mirror first, then the rotation by `deg`"""
    _fields_ = [("flip", C.c_int32), ("method", C.c_int32), ("deg", C.c_double), ("rotate", C.c_int32), ("reserved", C.c_int32)]


class pbd_candidate_head(C.Structure):
    _fields_ = [("score", C.c_float), ("component", C.c_int32), ("level", C.c_int32), ("nparts", C.c_int32)]


class pbd_camera(C.Structure):
    """image_geometry::PinholeCameraModel's fx(), fy(), cx(), cy(), Tx(), Ty()"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("tx", C.c_double),
                ("ty", C.c_double)]


class pbd_box3d(C.Structure):
    _fields_ = [("valid", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("zmin", C.c_float), ("zmax", C.c_float), ("reserved", C.c_int32), ("x3d", C.c_double), ("y3d", C.c_double),
                ("z3d", C.c_double), ("width3d", C.c_double), ("height3d", C.c_double), ("depth3d", C.c_double)]


BOX3D_DTYPE = np.dtype([("valid", np.int32), ("x", np.int32), ("y", np.int32), ("width", np.int32), ("height", np.int32),
                        ("zmin", np.float32), ("zmax", np.float32), ("reserved", np.int32), ("x3d", np.float64),
                        ("y3d", np.float64), ("z3d", np.float64), ("width3d", np.float64), ("height3d", np.float64),
                        ("depth3d", np.float64)])


class pbd_feature_block(C.Structure):
    """one part of a detection's feature vector (include/pbd_c.h): the ids of its bias / deformation / filter blocks, the filter's
    size and the deformation block -(dx^2, dx, dy^2, dy)"""
    _fields_ = [("bias_id", C.c_int32), ("def_id", C.c_int32), ("filter_id", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("reserved", C.c_int32), ("def", C.c_double * 4)]


FEATURE_BLOCK_DTYPE = np.dtype([("bias_id", np.int32), ("def_id", np.int32), ("filter_id", np.int32), ("kh", np.int32),
                                ("kw", np.int32), ("reserved", np.int32), ("def", np.float64, (4,))])
PBD_FEATVEC_STAGING_BYTES = 16 << 20


# pbd_latent_example (include/pbd_c.h "latent positives"): one fixed block of 32 bytes per frame
LATENT_EXAMPLE_DTYPE = np.dtype([("found", np.int32), ("written", np.int32), ("component", np.int32), ("level", np.int32),
                                 ("x", np.int32), ("y", np.int32), ("score", np.float64)])


CLUSTER3D_DTYPE = np.dtype([("cropped", np.int32), ("nclusters", np.int32), ("size", np.int32), ("first", np.int32),
                            ("cx", np.float64), ("cy", np.float64), ("cz", np.float64)])


def camera(cam) -> pbd_camera:
    """a pbd_camera from one, or from (fx, fy, cx, cy[, tx, ty])"""
    if isinstance(cam, pbd_camera):
        return cam
    v = [float(x) for x in cam]
    return pbd_camera(*(v + [0.0] * (6 - len(v))))


HEAD_DTYPE = np.dtype([("score", np.float32), ("component", np.int32), ("level", np.int32), ("nparts", np.int32)])

_lib = None


class PbdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pbd error {code}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    """Load libpbd_hip.so; fail loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.pbd_last_error.restype = C.c_char_p
        L.pbd_last_error.argtypes = [C.c_void_p]
        L.pbd_group_last_error.restype = C.c_char_p
        L.pbd_group_last_error.argtypes = [C.c_void_p]
        L.pbd_group_member.restype = C.c_void_p
        L.pbd_group_member.argtypes = [C.c_void_p, C.c_int]
        for name in EXPORTS:
            getattr(L, name)  # every declared symbol must be exported
        L.pbd_qp_create.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pbd_qp_destroy.restype = None
        L.pbd_qp_destroy.argtypes = [C.c_void_p]
        L.pbd_qp_dims.argtypes = [C.c_void_p] * 5
        L.pbd_qp_footprint.argtypes = [C.c_void_p, C.c_void_p]
        L.pbd_qp_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        for name in ("pbd_qp_score", "pbd_qp_score_dev", "pbd_qp_lincomb", "pbd_qp_lincomb_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.pbd_qp_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pbd_qp_get.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pbd_qp_put.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pbd_qp_noneg.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pbd_qp_fix.argtypes = [C.c_void_p, C.c_int]
        L.pbd_qp_state_put.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.pbd_qp_state_get.argtypes = [C.c_void_p] * 5
        L.pbd_qp_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.pbd_qp_one.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pbd_qp_refresh.argtypes = [C.c_void_p]
        L.pbd_qp_loss.argtypes = [C.c_void_p, C.c_void_p]
        L.pbd_qp_opt.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pbd_qp_prune.argtypes = [C.c_void_p, C.c_void_p]
        L.pbd_qp_weights.argtypes = [C.c_void_p, C.c_void_p]
        L.pbd_warp_geometry.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pbd_warp_taps.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        for name in ("pbd_warp_windows_u8", "pbd_warp_windows_u8_f64"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]
        L.pbd_qp_write_warped_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        for name in ("pbd_set_weights", "pbd_set_weights_dev", "pbd_get_weights"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pbd_qp_apply_weights.argtypes = [C.c_void_p]
        L.pbd_set_threshold.argtypes = [C.c_void_p, C.c_float]
        L.pbd_get_threshold.argtypes = [C.c_void_p, C.c_void_p]
        for name in ("pbd_qp_mine_u8", "pbd_qp_mine_dev_u8"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        L.pbd_qp_mine_batch_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        for name in ("pbd_qp_write_latent_u8", "pbd_qp_write_latent_dev_u8"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_double, C.c_int, C.c_void_p]
        L.pbd_qp_write_latent_batch_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        L.pbd_croppos.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        V, I, D = C.c_void_p, C.c_int, C.c_double
        L.pbd_eval_keypoint_dist.argtypes = [V, I, V, V]
        L.pbd_eval_pck_host.argtypes = [V, V, I, I, D, I, V]
        L.pbd_eval_apk_match_host.argtypes = [V, V, I, I, I, V, V, I, D, V]
        L.pbd_eval_ap_host.argtypes = [V, V, I, I, C.c_longlong, V, V, V]
        L.pbd_eval_create.argtypes = [V, I, I, I, D, V]
        L.pbd_eval_destroy.restype = None
        L.pbd_eval_destroy.argtypes = [V]
        L.pbd_eval_reset.argtypes = [V]
        L.pbd_eval_dims.argtypes = [V] * 6
        L.pbd_eval_get.argtypes = [V] * 5
        L.pbd_eval_add_pck_records.argtypes = [V, V, V, V, V, V, I, V]
        L.pbd_eval_add_apk_records.argtypes = [V, V, V, I, V, V, I, V]
        L.pbd_eval_pck_frame_u8.argtypes = [V, V, I, I, I, I, V, V, I, D, V, V, V]
        L.pbd_eval_pck_frame_batch_u8.argtypes = [V, V, I, I, I, I, I, V, V, V, D, V, V, V]
        L.pbd_eval_apk_frame_u8.argtypes = [V, V, I, I, I, I, V, V, I, V, V]
        L.pbd_eval_apk_frame_batch_u8.argtypes = [V, V, I, I, I, I, I, V, V, V, V, V]
        L.pbd_eval_pck.argtypes = [V, D, I, V]
        L.pbd_eval_apk.argtypes = [V, V, V, V]
        L.pbd_kmeans_host.argtypes = [V, I, I, I, V, C.c_uint64, I, V, V, V, V]
        L.pbd_cluster_parts_host.argtypes = [V, I, I, V, V, I, C.c_uint64, I, V, V, V, V, V, V, V]
        L.pbd_cluster_parts.argtypes = [I, V, I, I, V, V, I, C.c_uint64, I, V, V, V, V, V, V, V]
        L.pbd_set_interval.argtypes = [V, I]
        L.pbd_get_interval.argtypes = [V]
        L.pbd_qp_clear.argtypes = [V]
        L.pbd_qp_positive_threshold.argtypes = [V, D, V, V]
        L.pbd_pyrstore_create.argtypes = [V, I, I, I, V]
        L.pbd_pyrstore_destroy.restype = None
        L.pbd_pyrstore_destroy.argtypes = [V]
        L.pbd_pyrstore_dims.argtypes = [V] * 8
        L.pbd_pyrstore_slot.argtypes = [V, I, V, V, V, V]
        L.pbd_pyrstore_layout.argtypes = [I, I, I, I, I, I, V, V, V]
        for name in ("pbd_pyrstore_put_u8", "pbd_pyrstore_put_dev_u8"):
            getattr(L, name).argtypes = [V, I, V, I, I, I, I]
        L.pbd_pyrstore_put_batch_u8.argtypes = [V, V, V, I, I, I, I, I]
        L.pbd_pyrstore_get_level.argtypes = [V, I, I, V, C.c_size_t]
        L.pbd_detect_stored.argtypes = [V, V, I, V, V, V, I, V]
        L.pbd_detect_batch_stored.argtypes = [V, V, V, I, V, V, V, I, V]
        L.pbd_qp_mine_stored.argtypes = [V, V, I, I, V, V, V]
        L.pbd_qp_mine_batch_stored.argtypes = [V, V, V, I, V, V, V, V]
        L.pbd_rotate_geometry.argtypes = [I, I, D, V, V, V]
        L.pbd_map_rotate_points.argtypes = [V, I, I, I, D, I, V]
        L.pbd_flip_points.argtypes = [V, I, I, V, V]
        L.pbd_augment_host_u8.argtypes = [V, I, I, I, I, V, I, V, V]
        for name in ("pbd_augment_u8", "pbd_augment_dev_u8"):
            getattr(L, name).argtypes = [I, V, I, I, I, I, V, I, V, V]
        L.pbd_augment_last_error.restype = C.c_char_p
        L.pbd_augment_last_error.argtypes = []
        L.pbd_qp_write_warped_dev_u8.argtypes = L.pbd_qp_write_warped_u8.argtypes
        L.pbd_debug_live_allocs.argtypes = [V, V]
        if L.pbd_abi_version() != PBD_ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI version {L.pbd_abi_version()}, this binding is for {PBD_ABI_VERSION}")
        _lib = L
    return _lib


def live_allocs():
    """pbd_debug_live_allocs: (buffers, bytes) of device and pinned host memory the library holds in this process right now"""
    n, b = C.c_longlong(0), C.c_longlong(0)
    lib().pbd_debug_live_allocs(C.byref(n), C.byref(b))
    return n.value, b.value


def _p(a, ct):
    return None if a is None else a.ctypes.data_as(C.POINTER(ct))


def _strided_ok(a) -> bool:
    """an HxW or HxWxcn array whose rows the library can read in place: dense inner axes, rows strides[0] >= w * cn * itemsize bytes
    apart (a multiple of the itemsize).  An ROI of a larger frame, a pitched buffer and a contiguous array all are."""
    if a.ndim not in (2, 3):
        return False
    isz = a.itemsize
    cn = 1 if a.ndim == 2 else a.shape[2]
    if a.strides[-1] != isz or (a.ndim == 3 and a.strides[1] != cn * isz):
        return False
    return a.strides[0] >= a.shape[1] * cn * isz and a.strides[0] % isz == 0


def _frame(im, dtype=np.uint8):
    """(array, w, hgt, cn, stride in bytes) of an HxW or HxWxcn frame; dtype=None: the array's own.  A strided view (_strided_ok) of the
    right dtype is passed as it is — pointer array.ctypes.data, stride strides[0]; only the first w * cn * itemsize bytes of a row are
    read —, anything else is copied contiguous.  A contiguous array gives stride w * cn * itemsize."""
    a = np.asarray(im)
    if (dtype is not None and a.dtype != np.dtype(dtype)) or a.flags["C_CONTIGUOUS"] or not _strided_ok(a):
        a = np.ascontiguousarray(im, dtype)
    hgt, w = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    return a, w, hgt, cn, (w * cn * a.itemsize if a.flags["C_CONTIGUOUS"] else a.strides[0])


def _frames(frames, dtype=np.uint8):
    """([arrays], stride) of the frames of a batch, which share one stride argument: strided views are passed as they are only when
    all frames have one strides[0], else every frame is copied contiguous"""
    fr = [_frame(f, dtype) for f in frames]
    if len({f[4] for f in fr}) > 1:
        fr = [_frame(np.ascontiguousarray(f[0]), dtype) for f in fr]
    return [f[0] for f in fr], (fr[0][4] if fr else 0)


def _depth_image(depth, dtype):
    """(array, stride in bytes) of an HxW depth image of element type dtype, by _frame's rule"""
    a, _, _, _, stride = _frame(depth, dtype)
    return a, stride


class Handle:
    """Owns one pbd_handle (one GPU, one stream)."""

    def __init__(self, model, device=0, conv_mode=PBD_CONV_AUTO, max_candidates=4096, dt_correct_ptr=0,
                 level_begin=0, level_end=0, dp_groups=0, dtype=np.float32, graph=0, dp_mode=0, nms_sz=0, sized=False,
                 cand_filter=None, cand_nms=None):
        """dtype: np.float32 = PartsBasedDetector<float>, np.float64 = PartsBasedDetector<double>.
        nms_sz > 0: score-map NMS of the root planes on the device in front of the back-tracking (pbd_options.reserved[0]).
        dp_mode: 0 = messages folded by the parent's x pass where the model allows it (default), 1 = the
        three-kernel structure (x pass, y pass, reduce) for every model.  dp_groups: ignored (kept for callers).
        A model whose filters differ in size is created through pbd_create_sized, a uniform one through pbd_create
        (sized=True: pbd_create_sized for any model).
        cand_filter=(mode, overlap): pbd_set_candidate_filter — every detect returns Candidate::sort (PBD_CAND_SORT) or sort +
        nonMaximaSuppression(overlap) (PBD_CAND_SORT_NMS) of its output, computed on the GPU.
        cand_nms=(kind, top): pbd_set_candidate_nms — what that NMS is (PBD_NMS_PARTS: matlab/detection/nms.m after a cut to `top`)."""
        self.L = lib()
        self.model = model
        # a size per filter (pbd_create_sized) only where the bank is mixed: uniform banks keep pbd_create
        self.fsize = None
        if model.is_uniform() and not sized:
            self.desc = model.to_desc()
        else:
            self.desc, self.fsize = model.to_desc_sized()
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        self._f64 = self.dtype == np.dtype(np.float64)
        self._ct = C.c_double if self._f64 else C.c_float
        opt = pbd_options(device, conv_mode, max_candidates, dt_correct_ptr, level_begin, level_end,
                          PBD_SCALAR_F64 if self._f64 else PBD_SCALAR_F32, graph, (C.c_int32 * 2)(nms_sz, dp_mode))
        self.h = C.c_void_p()
        if self.fsize is None:
            rc = self.L.pbd_create(C.byref(self.desc), C.byref(opt), C.byref(self.h))
        else:
            rc = self.L.pbd_create_sized(C.byref(self.desc), _p(self.fsize, C.c_int32), C.byref(opt), C.byref(self.h))
        if rc != PBD_OK:
            msg = self.L.pbd_last_error(self.h).decode() if self.h else "allocation failed"
            if self.h:
                self.L.pbd_destroy(self.h)
            self.h = None
            raise PbdError(rc, msg)
        self.max_parts = self.L.pbd_max_parts(self.h)
        self.conv_mode = self.L.pbd_get_conv_mode(self.h)      # what PBD_CONV_AUTO resolved to
        if cand_filter is not None:
            self.set_candidate_filter(*cand_filter)
        if cand_nms is not None:
            self.set_candidate_nms(*cand_nms)

    # ---- weight and threshold updates (include/pbd_c.h "weight and threshold updates": vec2model.m on a live handle) ----
    def set_weights(self, w):
        """pbd_set_weights / pbd_set_weights_dev: the handle's weights replaced by `w` (Model.feature_layout() order, rounded to float32) —
        a numpy vector, or a contiguous float64 torch tensor on the handle's device, which is read in place.  The handle then behaves
        like one freshly created from model.with_weight_vector(w), which self.model becomes."""
        if hasattr(w, "data_ptr"):
            import torch
            if w.dtype != torch.float64 or not w.is_cuda or not w.is_contiguous():
                raise ValueError("a device weight vector must be a contiguous float64 tensor on the handle's device")
            torch.cuda.current_stream(w.device).synchronize()   # the library reads it on the handle's own stream
            self._chk(self.L.pbd_set_weights_dev(self.h, C.c_void_p(w.data_ptr()), int(w.numel())))
        else:
            w = np.ascontiguousarray(w, np.float64).ravel()
            self._chk(self.L.pbd_set_weights(self.h, _vp(w), int(w.size)))
        self._model_follows()

    def _model_follows(self):
        self.model = self.model.with_weight_vector(self.weights())

    def weights(self) -> np.ndarray:
        """pbd_get_weights: the handle's current float32 weights as float64, in Model.feature_layout() order"""
        out = np.zeros(self.model.feature_layout()["size"], np.float64)
        self._chk(self.L.pbd_get_weights(self.h, _vp(out), int(out.size)))
        return out

    def set_threshold(self, t: float):
        """pbd_set_threshold: the model's thresh for every detect from now on (any value but NaN)"""
        self._chk(self.L.pbd_set_threshold(self.h, float(t)))
        self.model = copy.copy(self.model)
        self.model.thresh = self.threshold

    @property
    def threshold(self) -> float:
        """pbd_get_threshold"""
        t = C.c_float()
        self._chk(self.L.pbd_get_threshold(self.h, C.byref(t)))
        return t.value

    # ---- the interval (include/pbd_c.h "one training round": train.m:95-96,121) ----
    def set_interval(self, interval: int):
        """pbd_set_interval: the pyramid's levels per octave from the next frame on (1..16).  The handle then behaves like one freshly
        created from the same model with that interval, which self.model gets; a bound QpCache or Eval stays valid."""
        self._chk(self.L.pbd_set_interval(self.h, int(interval)))
        self.model = copy.copy(self.model)
        self.model.interval = self.interval

    @property
    def interval(self) -> int:
        """pbd_get_interval"""
        return int(self.L.pbd_get_interval(self.h))

    def set_candidate_nms(self, kind, top=0):
        """pbd_set_candidate_nms: PBD_NMS_PAINTED / PBD_NMS_PARTS (top: 1000 = nms.m's cut, 0 = none) for the frames enqueued from now on."""
        self._chk(self.L.pbd_set_candidate_nms(self.h, int(kind), int(top)))

    def candidates_filter_parts(self, heads, boxes, locs, overlap=0.3, top=1000):
        """pbd_candidates_filter_parts: sort + nms.m's part-wise NMS of the records through the device kernels; returns the kept
        (heads, boxes, locs)."""
        heads = np.ascontiguousarray(heads, HEAD_DTYPE).copy()
        boxes = None if boxes is None else np.ascontiguousarray(boxes, np.int32).copy()
        locs = None if locs is None else np.ascontiguousarray(locs, np.int32).copy()
        kept = C.c_int(0)
        self._chk(self.L.pbd_candidates_filter_parts(self.h, C.c_float(overlap), int(top), heads.ctypes.data_as(C.c_void_p),
                                                     _p(boxes, C.c_int32), _p(locs, C.c_int32), len(heads), C.byref(kept)))
        k = kept.value
        return heads[:k], None if boxes is None else boxes[:k], None if locs is None else locs[:k]

    def set_candidate_filter(self, mode, overlap=0.0):
        """pbd_set_candidate_filter: PBD_CAND_RAW / PBD_CAND_SORT / PBD_CAND_SORT_NMS for the frames enqueued from now on."""
        self._chk(self.L.pbd_set_candidate_filter(self.h, int(mode), C.c_float(overlap)))

    def candidates_filter(self, heads, boxes, locs, im_w, im_h, mode=PBD_CAND_SORT_NMS, overlap=0.0):
        """pbd_candidates_filter: the records through the device kernel; returns the kept (heads, boxes, locs)."""
        heads = np.ascontiguousarray(heads, HEAD_DTYPE).copy()
        boxes = None if boxes is None else np.ascontiguousarray(boxes, np.int32).copy()
        locs = None if locs is None else np.ascontiguousarray(locs, np.int32).copy()
        kept = C.c_int(0)
        self._chk(self.L.pbd_candidates_filter(self.h, int(mode), C.c_float(overlap), int(im_w), int(im_h),
                                               heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                               len(heads), C.byref(kept)))
        k = kept.value
        return heads[:k], None if boxes is None else boxes[:k], None if locs is None else locs[:k]

    # ---- depth-consistency pruning (SearchSpacePruning::filterCandidatesByDepth) -------------------------------
    def set_depth_filter(self, on=True, zfactor=0.03):
        """pbd_set_depth_filter: the *_rgbd_* detects prune their records by the depth image (0.03: the reference's commented-out call)."""
        self._chk(self.L.pbd_set_depth_filter(self.h, int(bool(on)), C.c_float(zfactor)))

    @property
    def depth_dtype(self):
        """element type of the depth images this handle takes: T"""
        return np.dtype(np.float64 if self._f64 else np.float32)

    def _zimg(self, depth, dtype=None):
        """(array, PBD_DEPTH_*, stride in bytes) of a 2-D depth image (a strided view is passed as it is); dtype=None: the handle's T"""
        if depth is None:
            return None, DEPTH_OF[self.depth_dtype], 0
        d, ds = _depth_image(depth, dtype if dtype is not None else self.depth_dtype)
        return d, DEPTH_OF.get(d.dtype, 7), ds

    def detect_rgbd(self, im: np.ndarray, depth, capacity=4096, depth_dtype=None):
        """pbd_detect_rgbd_u8: depth = an HxW array (converted to T unless depth_dtype is given), or None"""
        im, w, hgt, cn, stride = _frame(im)
        d, dt, ds = self._zimg(depth, depth_dtype)
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_detect_rgbd_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride,
                                            None if d is None else d.ctypes.data_as(C.c_void_p), dt, ds,
                                            heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                            capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    def enqueue_rgbd_dev(self, dptr: int, w, hgt, cn, d_depth: int, dstride=None, stride=None, depth_type=None):
        """pbd_detect_rgbd_enqueue_dev_u8 (device image and depth; d_depth 0: none); collect with collect()"""
        dt = DEPTH_OF[self.depth_dtype] if depth_type is None else depth_type
        self._chk(self.L.pbd_detect_rgbd_enqueue_dev_u8(self.h, C.c_void_p(dptr), w, hgt, cn, stride or w * cn,
                                                        C.c_void_p(d_depth or None), dt, dstride or w * self.depth_dtype.itemsize))

    def detect_batch_rgbd(self, frames, depths, capacity=4096, depth_dtype=None):
        """pbd_detect_batch_rgbd_u8: depths[f] an HxW array or None"""
        frames, stride = _frames(frames)
        if not frames or len(depths) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("detect_batch_rgbd: one depth (or None) per frame, frames of one shape")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        zs = [self._zimg(d, depth_dtype) for d in depths]
        if any(z[0] is not None and z[0].shape != (hgt, w) for z in zs):
            raise ValueError("detect_batch_rgbd: depth images of the frames' size")
        dt = next((z[1] for z in zs if z[0] is not None), DEPTH_OF[self.depth_dtype])
        if len({z[2] for z in zs if z[0] is not None}) > 1:   # one dstride for the batch: views of different strides are copied
            zs = [z if z[0] is None else self._zimg(np.ascontiguousarray(z[0]), depth_dtype) for z in zs]
        ds = next((z[2] for z in zs if z[0] is not None), w * np.dtype(self.depth_dtype if depth_dtype is None else depth_dtype).itemsize)
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        dptrs = (C.c_void_p * len(frames))(*[None if z[0] is None else z[0].ctypes.data for z in zs])
        return self._batch_out(len(frames), capacity, lambda hd, bx, lc, cnt: self.L.pbd_detect_batch_rgbd_u8(
            self.h, ptrs, dptrs, len(frames), w, hgt, cn, stride, dt, ds,
            hd, bx, lc, capacity, cnt))

    def enqueue_batch_rgbd_dev(self, dptr: int, d_depths: int, nframes, w, hgt, cn, depth_type=None):
        """frames and depth images back to back in device memory; collect with collect_batch"""
        self._nb = nframes
        dt = DEPTH_OF[self.depth_dtype] if depth_type is None else depth_type
        self._chk(self.L.pbd_detect_batch_rgbd_enqueue_dev_u8(self.h, C.c_void_p(dptr), C.c_void_p(d_depths or None), nframes,
                                                              w, hgt, cn, dt))

    def candidates_depth_filter(self, heads, boxes, locs, depth, zfactor=0.03, depth_dtype=None):
        """pbd_candidates_depth_filter: the records pruned by `depth` (HxW, any size; None: empty) on the device; returns the
        kept (heads, boxes, locs), stable"""
        heads = np.ascontiguousarray(heads, HEAD_DTYPE).copy()
        boxes = np.ascontiguousarray(boxes, np.int32).copy()
        locs = None if locs is None else np.ascontiguousarray(locs, np.int32).copy()
        d, dt, ds = self._zimg(depth, depth_dtype)
        dh, dw = (0, 0) if d is None else d.shape
        kept = C.c_int(0)
        self._chk(self.L.pbd_candidates_depth_filter(self.h, C.c_float(zfactor), None if d is None else d.ctypes.data_as(C.c_void_p),
                                                     dt, dw, dh, ds, heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                                     _p(locs, C.c_int32), len(heads), C.byref(kept)))
        k = kept.value
        return heads[:k], boxes[:k], None if locs is None else locs[:k]

    # ---- 3-D boxes (Candidate::boundingBox3D + PointCloudClusterer::computeBoundingBoxes) -----------------------------
    def set_box3d(self, on=True, cam=None):
        """pbd_set_box3d: the *_rgbd_* detects compute a pbd_box3d (and part centres) per returned record; cam: a pbd_camera or
        (fx, fy, cx, cy[, tx, ty])"""
        c = None if cam is None else camera(cam)
        self._chk(self.L.pbd_set_box3d(self.h, int(bool(on)), None if c is None else C.byref(c)))

    def get_box3d(self, frame=0, capacity=None):
        """pbd_get_box3d: (boxes as a BOX3D_DTYPE array, centres [n, max_parts, 3]) of frame `frame` of the last collect"""
        cnt = C.c_int(0)
        rc = self.L.pbd_get_box3d(self.h, frame, None, None, 0, C.byref(cnt))
        if rc not in (PBD_OK, PBD_ERR_CAPACITY):
            self._chk(rc)
        n = cnt.value if capacity is None else capacity
        out = np.zeros(n, BOX3D_DTYPE)
        cen = np.zeros((n, self.max_parts, 3), np.float64)
        self._chk(self.L.pbd_get_box3d(self.h, frame, out.ctypes.data_as(C.c_void_p), _p(cen, C.c_double), n, C.byref(cnt)))
        return out[:cnt.value], cen[:cnt.value]

    def candidates_box3d(self, heads, boxes, depth, im_w, im_h, cam, depth_dtype=None):
        """pbd_candidates_box3d: (boxes as a BOX3D_DTYPE array, centres [n, max_parts, 3]) of the records against `depth` (HxW, any
        size; None: empty; converted to the handle's T unless depth_dtype is given)"""
        heads = np.ascontiguousarray(heads, HEAD_DTYPE)
        bx = np.zeros((len(heads), self.max_parts, 4), np.int32)
        b = np.asarray(boxes, np.int32)
        bx[:, :b.shape[1]] = b[:, :self.max_parts]
        d, dt, ds = self._zimg(depth, depth_dtype)
        dh, dw = (0, 0) if d is None else d.shape
        out = np.zeros(len(heads), BOX3D_DTYPE)
        cen = np.zeros((len(heads), self.max_parts, 3), np.float64)
        c = camera(cam)
        self._chk(self.L.pbd_candidates_box3d(self.h, C.byref(c), None if d is None else d.ctypes.data_as(C.c_void_p), dt, dw, dh,
                                              ds, int(im_w), int(im_h), heads.ctypes.data_as(C.c_void_p), _p(bx, C.c_int32),
                                              len(heads), out.ctypes.data_as(C.c_void_p), _p(cen, C.c_double)))
        return out, cen

    # ---- object clusters (PointCloudClusterer::clusterObjects) ---------------------------------------------------------
    def set_cluster3d(self, on=True, tolerance=0.01):
        """pbd_set_cluster3d: the frames that compute 3-D boxes also compute the object cluster of every returned record"""
        self._chk(self.L.pbd_set_cluster3d(self.h, int(bool(on)), C.c_float(tolerance)))

    def get_cluster3d(self, frame=0):
        """pbd_get_cluster3d: (results as a CLUSTER3D_DTYPE array, the kept clusters' indices one after the other) of frame
        `frame` of the last collect; record i's indices start at the exclusive prefix sum of results["size"]"""
        cnt, tot = C.c_int(0), C.c_int(0)
        rc = self.L.pbd_get_cluster3d(self.h, frame, None, 0, C.byref(cnt), None, 0, C.byref(tot))
        if rc not in (PBD_OK, PBD_ERR_CAPACITY):
            self._chk(rc)
        out = np.zeros(cnt.value, CLUSTER3D_DTYPE)
        idx = np.zeros(max(tot.value, 1), np.int32)
        self._chk(self.L.pbd_get_cluster3d(self.h, frame, out.ctypes.data_as(C.c_void_p), len(out), C.byref(cnt),
                                           _p(idx, C.c_int32), len(idx), C.byref(tot)))
        return out[:cnt.value], idx[:tot.value]

    def candidates_cluster3d(self, cloud, boxes3d, tolerance=0.01):
        """pbd_candidates_cluster3d: (results as a CLUSTER3D_DTYPE array, the kept clusters' indices one after the other) of the
        pbd_box3d records `boxes3d` (BOX3D_DTYPE) against the organized cloud, an [h, w, 3] float32 array (cluster3d_raw takes
        strided buffers such as PCL's PointXYZ / PointXYZRGB)"""
        c = np.ascontiguousarray(cloud, np.float32)
        if c.ndim != 3 or c.shape[2] != 3:
            raise ValueError("cloud: [h, w, 3] float32")
        ch, cw = c.shape[:2]
        return self._cluster3d(c, cw, ch, 12, 12 * cw, np.ascontiguousarray(boxes3d, BOX3D_DTYPE), tolerance)

    def cluster3d_raw(self, buf, cw, ch, point_stride, row_stride, boxes3d, tolerance=0.01):
        """pbd_candidates_cluster3d on a raw buffer with explicit geometry (strides in bytes)"""
        return self._cluster3d(np.ascontiguousarray(buf), cw, ch, point_stride, row_stride,
                               np.ascontiguousarray(boxes3d, BOX3D_DTYPE), tolerance)

    def _cluster3d(self, c, cw, ch, ps, rs, b, tol):
        out = np.zeros(len(b), CLUSTER3D_DTYPE)
        tot = C.c_int(0)
        cp = c.ctypes.data_as(C.c_void_p) if c.size else None
        self._chk(self.L.pbd_candidates_cluster3d(self.h, cp, int(cw), int(ch), int(ps), int(rs), b.ctypes.data_as(C.c_void_p),
                                                  len(b), C.c_float(tol), out.ctypes.data_as(C.c_void_p), None, 0, C.byref(tot)))
        idx = np.zeros(max(tot.value, 1), np.int32)
        self._chk(self.L.pbd_candidates_cluster3d(self.h, cp, int(cw), int(ch), int(ps), int(rs), b.ctypes.data_as(C.c_void_p),
                                                  len(b), C.c_float(tol), out.ctypes.data_as(C.c_void_p), _p(idx, C.c_int32),
                                                  len(idx), C.byref(tot)))
        return out, idx[:tot.value]

    # ---- per-part scores (the decomposition of a detection's score) ------------------------------------------------------
    def set_boundary_pad(self, pad=3):
        """pbd_set_boundary_pad: `pad` cells of padding (0, and 1 in the last channel) around every pyramid level from the next
        frame on; 0 = off.  Planes, locs and pyramid_geometry() are then padded; boxes are shifted back by the padding."""
        self._chk(self.L.pbd_set_boundary_pad(self.h, int(pad)))

    @property
    def boundary_pad(self):
        """pbd_get_boundary_pad"""
        return int(self.L.pbd_get_boundary_pad(self.h))

    def set_pyramid_kind(self, kind=PBD_PYRAMID_MATLAB):
        """pbd_set_pyramid_kind: PBD_PYRAMID_MATLAB = the image pyramid of matlab/detection/featpyramid.m (area resize + reduce, double
        level images) for every 8-bit frame from the next one on; PBD_PYRAMID_OPENCV = the default.  geometry() answers for the kind."""
        self._chk(self.L.pbd_set_pyramid_kind(self.h, int(kind)))

    @property
    def pyramid_kind(self):
        """pbd_get_pyramid_kind"""
        return int(self.L.pbd_get_pyramid_kind(self.h))

    def set_part_scores(self, on=True):
        """pbd_set_part_scores: every detect also computes (app, def, bias) of every part of every returned record"""
        self._chk(self.L.pbd_set_part_scores(self.h, int(bool(on))))

    def part_scores(self, frame=0):
        """pbd_get_part_scores: [count, max_parts, 3] float64 (app, def, bias; zero beyond a record's nparts) of frame `frame` of
        the last detect / collect, in the order its records were returned"""
        cnt = C.c_int(0)
        rc = self.L.pbd_get_part_scores(self.h, frame, None, 0, C.byref(cnt))
        if rc not in (PBD_OK, PBD_ERR_CAPACITY):
            self._chk(rc)
        out = np.zeros((cnt.value, self.max_parts, 3), np.float64)
        self._chk(self.L.pbd_get_part_scores(self.h, frame, _p(out, C.c_double), len(out), C.byref(cnt)))
        return out[:cnt.value]

    def candidates_part_scores(self, heads, locs):
        """pbd_candidates_part_scores: [n, max_parts, 3] float64 of the caller's records against the response planes resident for
        the handle's frame (level: the plan's level; frame f of a batch plan: f * nlevels + l)"""
        heads = np.ascontiguousarray(heads, HEAD_DTYPE)
        lc = np.zeros((len(heads), self.max_parts, 3), np.int32)
        l = np.asarray(locs, np.int32).reshape(len(heads), -1, 3)
        lc[:, :l.shape[1]] = l[:, :self.max_parts]
        out = np.zeros((len(heads), self.max_parts, 3), np.float64)
        self._chk(self.L.pbd_candidates_part_scores(self.h, heads.ctypes.data_as(C.c_void_p), _p(lc, C.c_int32), len(heads),
                                                    _p(out, C.c_double)))
        return out

    # ---- feature vectors of detections (detect.m:272-308) ---------------------------------------------------------------
    def feature_window_max(self):
        """pbd_feature_window_max: elements of a window slot, the bank's largest kh * kw * flen"""
        n = int(self.L.pbd_feature_window_max(self.h))
        if n < 0:
            raise PbdError(-n, "pbd_feature_window_max")
        return n

    def _records(self, heads, locs):
        heads = np.ascontiguousarray(heads, HEAD_DTYPE)
        lc = np.zeros((len(heads), self.max_parts, 3), np.int32)
        if len(heads):   # (an empty selection has no part axis to infer)
            l = np.asarray(locs, np.int32).reshape(len(heads), -1, 3)
            lc[:, :l.shape[1]] = l[:, :self.max_parts]
        return heads, lc

    def candidates_features(self, heads, locs):
        """pbd_candidates_features[_f64]: (blocks [n, max_parts] FEATURE_BLOCK_DTYPE, windows [n, max_parts, wmax] in the handle's
        dtype) of the caller's records against the features resident for the handle's frame (level: the plan's level; frame f of
        a batch plan: f * nlevels + l).  A window is [kh][kw * 32] at the front of its slot."""
        heads, lc = self._records(heads, locs)
        blocks = np.zeros((len(heads), self.max_parts), FEATURE_BLOCK_DTYPE)
        windows = np.zeros((len(heads), self.max_parts, self.feature_window_max()), self.dtype)
        self._chk(self._fn("pbd_candidates_features")(self.h, heads.ctypes.data_as(C.c_void_p), _p(lc, C.c_int32), len(heads),
                                                      blocks.ctypes.data_as(C.c_void_p), _p(windows, self._ct)))
        return blocks, windows

    def candidates_features_dev(self, heads, locs, d_blocks: int, d_windows: int):
        """pbd_candidates_features_dev: the same into the caller's device buffers (integer device pointers: n * max_parts blocks of 56
        bytes, n * max_parts * wmax elements of the handle's dtype), on the handle's stream; returns after the launch."""
        heads, lc = self._records(heads, locs)
        self._chk(self.L.pbd_candidates_features_dev(self.h, heads.ctypes.data_as(C.c_void_p), _p(lc, C.c_int32), len(heads),
                                                     C.c_void_p(d_blocks), C.c_void_p(d_windows)))

    def close(self):
        if getattr(self, "h", None):
            for ref in getattr(self, "_caches", ()):   # the example caches and evaluation ledgers created from this handle go first: they borrow its device
                q = ref()
                if q is not None:
                    q.close()
            self._caches = []
            self.L.pbd_destroy(self.h)
            self.h = None

    def filter_size(self, n):
        """(kh, kw) of filter n (pbd_get_filter_size)."""
        kh, kw = C.c_int32(), C.c_int32()
        self._chk(self.L.pbd_get_filter_size(self.h, n, C.byref(kh), C.byref(kw)))
        return kh.value, kw.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fn(self, name):
        """Stage entry point of this handle's instantiation (name or name_f64)."""
        return getattr(self.L, name + ("_f64" if self._f64 else ""))

    def _chk(self, rc):
        if rc != PBD_OK:
            raise PbdError(rc, self.L.pbd_last_error(self.h).decode())

    # ---- detect ----------------------------------------------------------------
    def _bufs(self, capacity):
        heads = np.zeros(capacity, HEAD_DTYPE)
        boxes = np.zeros((capacity, self.max_parts, 4), np.int32)
        locs = np.zeros((capacity, self.max_parts, 3), np.int32)
        return heads, boxes, locs

    def _out(self, heads, boxes, locs, n):
        return heads[:n].copy(), boxes[:n].copy(), locs[:n].copy()

    def detect(self, im: np.ndarray, capacity=4096):
        im, w, hgt, cn, stride = _frame(im)
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_detect_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride,
                                       heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                       capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    def detect_image(self, im: np.ndarray, capacity=4096):
        """pbd_detect_image: the image in its own depth (uint8 / uint16 / float32 / float64 = CV_8U / 16U / 32F / 64F); other dtypes are refused
        by the library the way the reference refuses them (CV_Error(StsUnsupportedFormat))"""
        im, w, hgt, cn, stride = _frame(im, None)
        depth = DEPTH_OF.get(im.dtype, 1 if im.dtype == np.int8 else 3 if im.dtype == np.int16 else 4 if im.dtype == np.int32 else 7)
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_detect_image(self.h, im.ctypes.data_as(C.c_void_p), depth, w, hgt, cn, stride,
                                          heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                          capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    def tune_plan(self, im, batch=1):
        """pbd_tune_plan: (chosen geometry 1 / 2 — 0 for double handles —, [ms with 256 lanes / 40 KB, ms with 128 lanes / 25 KB]); im=None: the rule again"""
        chosen = C.c_int(0)
        ms = (C.c_double * 2)()
        if im is None:
            self._chk(self.L.pbd_tune_plan(self.h, None, 0, 0, 0, 0, 1, C.byref(chosen), ms))
            return 0, [0.0, 0.0]
        im, w, hgt, cn, stride = _frame(im)
        self._chk(self.L.pbd_tune_plan(self.h, _p(im, C.c_uint8), w, hgt, cn, stride, int(batch), C.byref(chosen), ms))
        return chosen.value, [ms[0], ms[1]]

    def detect_dev(self, dptr: int, w, hgt, cn, stride=None, capacity=4096):
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_detect_dev_u8(self.h, C.c_void_p(dptr), w, hgt, cn, stride or w * cn,
                                           heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                           _p(locs, C.c_int32), capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    def enqueue_dev(self, dptr: int, w, hgt, cn, stride=None):
        self._chk(self.L.pbd_detect_enqueue_dev_u8(self.h, C.c_void_p(dptr), w, hgt, cn, stride or w * cn))

    def enqueue(self, im: np.ndarray):
        """pbd_detect_enqueue_u8: asynchronous H2D of a host image (pinned for true asynchrony) + all kernels.
        The array (contiguous, or a strided view as _frame passes it) must stay alive until collect()."""
        assert im.dtype == np.uint8 and (im.flags["C_CONTIGUOUS"] or _strided_ok(im))   # read in place: never a copy
        im, w, hgt, cn, stride = _frame(im)
        self._inflight_im = im
        self._chk(self.L.pbd_detect_enqueue_u8(self.h, C.c_void_p(im.ctypes.data), w, hgt, cn, stride))

    def enqueue_host_ptr(self, ptr: int, w, hgt, cn, stride=None):
        """same from a raw host pointer (e.g. a torch pinned tensor's data_ptr())."""
        self._chk(self.L.pbd_detect_enqueue_u8(self.h, C.c_void_p(ptr), w, hgt, cn, stride or w * cn))

    def collect(self, capacity=4096):
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_detect_collect(self.h, heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                            _p(locs, C.c_int32), capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    # ---- frames from a pyramid store (include/pbd_c.h "pyramid store") ---------------------
    def detect_stored(self, store: "PyramidStore", slot: int, capacity=4096):
        """pbd_detect_stored: detect() on the frame that was put into `slot` of `store` — the slot's feature pyramid is loaded where the
        image pyramid and HOG ran; the result is detect(image)'s on this handle, in bits.  `slot` may be a StoredFrame."""
        store, slot = _stored(store, slot)
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_detect_stored(self.h, store.s, int(slot), heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                           _p(locs, C.c_int32), capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    def detect_batch_stored(self, store: "PyramidStore", slots, capacity=4096):
        """pbd_detect_batch_stored: detect_batch() on the frames of `slots` (same-sized; any order, repeats allowed)"""
        sl = np.ascontiguousarray([int(getattr(x, "slot", x)) for x in slots], np.int32)
        return self._batch_out(len(sl), capacity, lambda hd, bx, lc, cnt: self.L.pbd_detect_batch_stored(
            self.h, store.s, _vp(sl), len(sl), hd, bx, lc, capacity, cnt))

    # ---- a batch of same-sized frames through this handle ------------------------------------
    def detect_batch(self, frames, capacity=4096):
        """pbd_detect_batch_u8: list of HxWxC uint8 frames -> list of (heads, boxes, locs), one per frame."""
        frames, stride = _frames(frames)
        if not frames:
            raise ValueError("detect_batch: at least one frame")
        if any(f.shape != frames[0].shape for f in frames):   # the C side reads w * hgt * cn bytes behind every pointer
            raise ValueError("detect_batch: all frames of a batch must have the same shape, got "
                             f"{sorted({f.shape for f in frames})}")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        return self._batch_out(len(frames), capacity, lambda hd, bx, lc, cnt: self.L.pbd_detect_batch_u8(
            self.h, ptrs, len(frames), w, hgt, cn, stride, hd, bx, lc, capacity, cnt))

    def enqueue_batch_dev(self, dptr: int, nframes, w, hgt, cn):
        """frames back to back in device memory (tightly packed); collect with collect_batch"""
        self._nb = nframes
        self._chk(self.L.pbd_detect_batch_enqueue_dev_u8(self.h, C.c_void_p(dptr), nframes, w, hgt, cn))

    def enqueue_batch_host_ptrs(self, ptrs, w, hgt, cn, stride=None):
        """host frames (raw pointers, e.g. pinned torch tensors; one stride for all); collect with collect_batch"""
        self._nb = len(ptrs)
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._chk(self.L.pbd_detect_batch_enqueue_u8(self.h, arr, len(ptrs), w, hgt, cn, stride or w * cn))

    def collect_batch(self, capacity=4096):
        return self._batch_out(self._nb, capacity, lambda hd, bx, lc, cnt: self.L.pbd_detect_batch_collect(self.h, hd, bx, lc, capacity, cnt))

    def _batch_out(self, nb, capacity, call):
        heads = np.zeros(nb * capacity, HEAD_DTYPE)
        boxes = np.zeros((nb * capacity, self.max_parts, 4), np.int32)
        locs = np.zeros((nb * capacity, self.max_parts, 3), np.int32)
        counts = (C.c_int * nb)()
        self._chk(call(heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32), counts))
        return [self._out(heads[f * capacity:(f + 1) * capacity], boxes[f * capacity:(f + 1) * capacity],
                          locs[f * capacity:(f + 1) * capacity], counts[f]) for f in range(nb)]

    def set_levels(self, levels):
        """Process only this set of pyramid levels (empty = all): multi-GPU level sharding."""
        a = np.ascontiguousarray(list(levels), np.int32)
        self._chk(self.L.pbd_set_levels(self.h, _p(a, C.c_int32) if len(a) else None, len(a)))

    def set_stream(self, stream_ptr: int):
        self._chk(self.L.pbd_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- stages ------------------------------------------------------------------
    def geometry(self, w, hgt):
        n = C.c_int(0)
        self._chk(self.L.pbd_pyramid_geometry(self.h, w, hgt, C.byref(n), None, None, None, None, None))
        a = [np.zeros(n.value, np.int32) for _ in range(4)]
        sc = np.zeros(n.value, np.float32)
        self._chk(self.L.pbd_pyramid_geometry(self.h, w, hgt, C.byref(n), *[_p(x, C.c_int32) for x in a],
                                              _p(sc, C.c_float)))
        return dict(nlevels=n.value, img_w=a[0], img_h=a[1], cell_w=a[2], cell_h=a[3], scales=sc)

    def begin_frame(self, w, hgt, cn):
        self._chk(self.L.pbd_begin_frame(self.h, w, hgt, cn))
        self._geo = self.geometry(w, hgt)
        self._cn = cn

    def pyramid(self, im: np.ndarray):
        im, w, hgt, cn, stride = _frame(im)
        self._chk(self.L.pbd_pyramid_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride))
        self._geo = self.geometry(w, hgt)
        self._cn = cn
        self._imdtype = np.dtype(np.uint8)

    def pyramid_image(self, im: np.ndarray):
        """pbd_pyramid_image: pyramid() for an image of any accepted depth (its numpy dtype)"""
        im, w, hgt, cn, stride = _frame(im, None)
        self._chk(self.L.pbd_pyramid_image(self.h, im.ctypes.data_as(C.c_void_p), DEPTH_OF[im.dtype], w, hgt, cn, stride))
        self._geo = self.geometry(w, hgt)
        self._cn = cn
        self._imdtype = im.dtype

    def level_image_raw(self, l):
        g = self._geo
        shape = (g["img_h"][l], g["img_w"][l]) + ((self._cn,) if self._cn > 1 else ())
        dt = np.dtype(np.float64) if self.pyramid_kind == PBD_PYRAMID_MATLAB else getattr(self, "_imdtype", np.dtype(np.uint8))
        out = np.zeros(shape, dt)
        self._chk(self.L.pbd_get_level_image_raw(self.h, l, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
        return out

    def level_image(self, l):
        g = self._geo
        shape = (g["img_h"][l], g["img_w"][l]) + ((self._cn,) if self._cn > 1 else ())
        out = np.zeros(shape, np.uint8)
        self._chk(self.L.pbd_get_level_image(self.h, l, _p(out, C.c_uint8)))
        return out

    def level_features(self, l):
        g = self._geo
        out = np.zeros((g["cell_h"][l], g["cell_w"][l], 32), self.dtype)
        self._chk(self._fn("pbd_get_level_features")(self.h, l, _p(out, self._ct)))
        return out

    def frame_planes(self, frame, l, w, hgt, cn=3, imdtype=np.uint8):
        """pbd_get_frame_level_image_raw / pbd_get_frame_level_features: (level image, features) of one frame of the current plan — a batch
        plan included — for a plan of w x hgt x cn frames of pixel type imdtype.  Read-only; needs no earlier pyramid() on this object."""
        g = self.geometry(w, hgt)
        img = np.zeros((g["img_h"][l], g["img_w"][l]) + ((cn,) if cn > 1 else ()), np.dtype(imdtype))
        feat = np.zeros((g["cell_h"][l], g["cell_w"][l], 32), self.dtype)
        self._chk(self.L.pbd_get_frame_level_image_raw(self.h, int(frame), int(l), img.ctypes.data_as(C.c_void_p), C.c_size_t(img.nbytes)))
        self._chk(self._fn("pbd_get_frame_level_features")(self.h, int(frame), int(l), _p(feat, self._ct)))
        return img, feat

    def set_level_features(self, l, f):
        f = np.ascontiguousarray(f, self.dtype)
        self._chk(self._fn("pbd_set_level_features")(self.h, l, _p(f, self._ct)))

    def pdf(self):
        self._chk(self.L.pbd_pdf(self.h))

    def level_response(self, l, n):
        g = self._geo
        out = np.zeros((g["cell_h"][l], g["cell_w"][l]), self.dtype)
        self._chk(self._fn("pbd_get_level_response")(self.h, l, n, _p(out, self._ct)))
        return out

    def set_level_response(self, l, n, r):
        r = np.ascontiguousarray(r, self.dtype)
        self._chk(self._fn("pbd_set_level_response")(self.h, l, n, _p(r, self._ct)))

    def dp_min(self):
        self._chk(self.L.pbd_dp_min(self.h))

    def stage_state(self):
        """pbd_get_stage_state: dict of which stage buffers currently hold valid data"""
        st = (C.c_int32 * 4)()
        self._chk(self.L.pbd_get_stage_state(self.h, st))
        return dict(pyramid=bool(st[0]), features=bool(st[1]), responses=bool(st[2]), dp=bool(st[3]))

    def dp_pointers(self, l, c, p, m):
        g = self._geo
        sh = (g["cell_h"][l], g["cell_w"][l])
        ix, iy, ik = (np.zeros(sh, np.int32) for _ in range(3))
        self._chk(self.L.pbd_get_dp_pointers(self.h, l, c, p, m, _p(ix, C.c_int32), _p(iy, C.c_int32),
                                             _p(ik, C.c_int32)))
        return ix, iy, ik

    def frame_dp_pointers(self, frame, l, c, p, m, w, hgt):
        """pbd_get_frame_dp_pointers: (Ix, Iy, Ik) of one frame of the current plan — a batch plan included — of w x hgt frames"""
        g = self.geometry(w, hgt)
        sh = (g["cell_h"][l], g["cell_w"][l])
        ix, iy, ik = (np.zeros(sh, np.int32) for _ in range(3))
        self._chk(self.L.pbd_get_frame_dp_pointers(self.h, int(frame), int(l), c, p, m, _p(ix, C.c_int32), _p(iy, C.c_int32),
                                                   _p(ik, C.c_int32)))
        return ix, iy, ik

    def root(self, l, c):
        g = self._geo
        sh = (g["cell_h"][l], g["cell_w"][l])
        rv, ri = np.zeros(sh, self.dtype), np.zeros(sh, np.int32)
        self._chk(self._fn("pbd_get_root")(self.h, l, c, _p(rv, self._ct), _p(ri, C.c_int32)))
        return rv, ri

    def set_root(self, l, c, rootv, rooti):
        rv, ri = np.ascontiguousarray(rootv, self.dtype), np.ascontiguousarray(rooti, np.int32)
        self._chk(self._fn("pbd_set_root")(self.h, l, c, _p(rv, self._ct), _p(ri, C.c_int32)))

    def set_dp_pointers(self, l, c, p, m, ix, iy, ik):
        """hand DynamicProgram::argmin pointer tables that this handle's min() did not produce"""
        a = [np.ascontiguousarray(t, np.int32) for t in (ix, iy, ik)]
        self._chk(self.L.pbd_set_dp_pointers(self.h, l, c, p, m, *[_p(t, C.c_int32) for t in a]))

    def footprint(self):
        """(frame_bytes, model_bytes) of device memory held by the handle"""
        fb, mb = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.L.pbd_get_footprint(self.h, C.byref(fb), C.byref(mb)))
        return fb.value, mb.value

    def dp_argmin(self, capacity=4096):
        heads, boxes, locs = self._bufs(capacity)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_dp_argmin(self.h, heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                       _p(locs, C.c_int32), capacity, C.byref(cnt)))
        return self._out(heads, boxes, locs, cnt.value)

    # ---- latent detection (detect(im, model, thresh, bbox, overlap) of matlab/detection/detect.m) -------------------------
    def _latent_args(self, truth, mix, nframes=1):
        """truth [nframes, <= max_parts, 4] (x, y, width, height) and mix [nframes, <= max_parts] (-1: free) or None, padded to
        max_parts rows (zero boxes, free mixtures) -> contiguous int32 arrays"""
        t = np.asarray(truth, np.int32).reshape(nframes, -1, 4)
        tr = np.zeros((nframes, self.max_parts, 4), np.int32)
        tr[:, :t.shape[1]] = t[:, :self.max_parts]
        mx = None
        if mix is not None:
            m = np.asarray(mix, np.int32).reshape(nframes, -1)
            mx = np.full((nframes, self.max_parts), -1, np.int32)
            mx[:, :m.shape[1]] = m[:, :self.max_parts]
        return tr, mx

    def latent_mask(self, truth, overlap, mix=None, component=-1):
        """pbd_latent_mask: masks the resident response planes; returns admissible [nlevels, ncomponents] (1: the pair remains)"""
        tr, mx = self._latent_args(truth, mix)
        adm = np.zeros((self._geo["nlevels"], self.model.ncomponents), np.int32)
        self._chk(self.L.pbd_latent_mask(self.h, _p(tr, C.c_int32), _p(mx, C.c_int32), int(component), C.c_double(overlap),
                                         _p(adm, C.c_int32)))
        return adm

    def dp_argbest(self):
        """pbd_dp_argbest: (heads, boxes, locs) holding one record, or none"""
        heads, boxes, locs = self._bufs(1)
        found = C.c_int(0)
        self._chk(self.L.pbd_dp_argbest(self.h, heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                        C.byref(found)))
        return self._out(heads, boxes, locs, found.value)

    def detect_latent(self, im: np.ndarray, truth, overlap, mix=None, component=-1):
        """pbd_detect_latent_u8: (heads, boxes, locs) holding the best pose whose parts overlap `truth`, or none"""
        im, w, hgt, cn, stride = _frame(im)
        tr, mx = self._latent_args(truth, mix)
        heads, boxes, locs = self._bufs(1)
        found = C.c_int(0)
        self._chk(self.L.pbd_detect_latent_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride, _p(tr, C.c_int32), _p(mx, C.c_int32),
                                              int(component), C.c_double(overlap), heads.ctypes.data_as(C.c_void_p),
                                              _p(boxes, C.c_int32), _p(locs, C.c_int32), C.byref(found)))
        return self._out(heads, boxes, locs, found.value)

    def detect_latent_dev(self, dptr: int, w, hgt, cn, truth, overlap, mix=None, component=-1, stride=None):
        """pbd_detect_latent_dev_u8: the image already in device memory"""
        tr, mx = self._latent_args(truth, mix)
        heads, boxes, locs = self._bufs(1)
        found = C.c_int(0)
        self._chk(self.L.pbd_detect_latent_dev_u8(self.h, C.c_void_p(dptr), w, hgt, cn, stride or w * cn, _p(tr, C.c_int32),
                                                  _p(mx, C.c_int32), int(component), C.c_double(overlap),
                                                  heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                                  C.byref(found)))
        return self._out(heads, boxes, locs, found.value)

    def detect_batch_latent(self, frames, truths, overlap, mixes=None, component=-1):
        """pbd_detect_batch_latent_u8: a truth set (and mixture set) per frame -> list of (heads, boxes, locs), one record or none each"""
        frames, stride = _frames(frames)
        if not frames or len(truths) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("detect_batch_latent: one truth set per frame, frames of one shape")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        tr, mx = self._latent_args(np.stack([np.asarray(t, np.int32) for t in truths]),
                                   None if mixes is None else np.stack([np.asarray(m, np.int32) for m in mixes]), len(frames))
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        return self._batch_out(len(frames), 1, lambda hd, bx, lc, cnt: self.L.pbd_detect_batch_latent_u8(
            self.h, ptrs, len(frames), w, hgt, cn, stride, _p(tr, C.c_int32), _p(mx, C.c_int32), int(component),
            C.c_double(overlap), hd, bx, lc, cnt))

    # ---- best pose per ground-truth box (matlab/detection/testmodel_gtbox.m, bestoverlap.m) -------------------------------
    def candidates_select_gt(self, heads, boxes, gt, overlap=0.3):
        """pbd_candidates_select_gt: pbd_candidates_best_overlap of host records through the device kernels -> (best[ngt], o[ngt])"""
        heads = np.ascontiguousarray(heads, HEAD_DTYPE)
        boxes = np.ascontiguousarray(boxes, np.int32)
        gt = np.ascontiguousarray(gt, np.float64).reshape(-1, 4)
        best = np.full(len(gt), -1, np.int32)
        o = np.zeros(len(gt), np.float64)
        self._chk(self.L.pbd_candidates_select_gt(self.h, _p(gt, C.c_double), len(gt), C.c_double(overlap),
                                                  heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), len(heads),
                                                  _p(best, C.c_int32), _p(o, C.c_double)))
        return best, o

    def _gt_out(self, n):
        return self._bufs(n) + (np.zeros(n, np.int32), np.zeros(n, np.float64))

    def detect_gtbox(self, im: np.ndarray, gt, overlap=0.3):
        """pbd_detect_gtbox_u8: per gt box (x1, y1, x2, y2) the best pose of the frame on it -> (heads, boxes, locs, found, o), one
        slot per box (zeros where found is 0); self.gt_records = the frame's records in front of the selection"""
        im, w, hgt, cn, stride = _frame(im)
        gt = np.ascontiguousarray(gt, np.float64).reshape(-1, 4)
        heads, boxes, locs, found, o = self._gt_out(len(gt))
        nrec = C.c_int(0)
        rc = self.L.pbd_detect_gtbox_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride, _p(gt, C.c_double), len(gt), C.c_double(overlap),
                                        heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                        _p(found, C.c_int32), _p(o, C.c_double), C.byref(nrec))
        self.gt_records = nrec.value
        self._chk(rc)
        return heads, boxes, locs, found, o

    def detect_gtbox_dev(self, dptr: int, w, hgt, cn, gt, overlap=0.3, stride=None):
        """pbd_detect_gtbox_dev_u8: the image already in device memory"""
        gt = np.ascontiguousarray(gt, np.float64).reshape(-1, 4)
        heads, boxes, locs, found, o = self._gt_out(len(gt))
        nrec = C.c_int(0)
        rc = self.L.pbd_detect_gtbox_dev_u8(self.h, C.c_void_p(dptr), w, hgt, cn, stride or w * cn, _p(gt, C.c_double), len(gt),
                                            C.c_double(overlap), heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                            _p(locs, C.c_int32), _p(found, C.c_int32), _p(o, C.c_double), C.byref(nrec))
        self.gt_records = nrec.value
        self._chk(rc)
        return heads, boxes, locs, found, o

    def detect_batch_gtbox(self, frames, gts, overlap=0.3):
        """pbd_detect_batch_gtbox_u8: the gt boxes of every frame (any number up to PBD_GT_MAX, also none) -> per frame what
        detect_gtbox returns"""
        frames, stride = _frames(frames)
        if not frames or len(gts) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("detect_batch_gtbox: one set of gt boxes per frame, frames of one shape")
        gts = [np.asarray(g, np.float64).reshape(-1, 4) for g in gts]
        if any(len(g) > PBD_GT_MAX for g in gts):
            raise ValueError("detect_batch_gtbox: at most PBD_GT_MAX gt boxes per frame")
        nb = len(frames)
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        gt = np.zeros((nb, PBD_GT_MAX, 4), np.float64)
        ngt = np.array([len(g) for g in gts], np.int32)
        for f, g in enumerate(gts):
            gt[f, :len(g)] = g
        heads, boxes, locs, found, o = self._gt_out(nb * PBD_GT_MAX)
        ptrs = (C.c_void_p * nb)(*[f.ctypes.data for f in frames])
        nrec = C.c_int(0)
        rc = self.L.pbd_detect_batch_gtbox_u8(self.h, ptrs, nb, w, hgt, cn, stride, _p(gt, C.c_double), _p(ngt, C.c_int32),
                                              C.c_double(overlap), heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32),
                                              _p(locs, C.c_int32), _p(found, C.c_int32), _p(o, C.c_double), C.byref(nrec))
        self.gt_records = nrec.value
        self._chk(rc)
        return [tuple(a[f * PBD_GT_MAX:f * PBD_GT_MAX + ngt[f]].copy() for a in (heads, boxes, locs, found, o)) for f in range(nb)]

    # ---- primitives ----------------------------------------------------------------
    def dt2d(self, a: np.ndarray, ax, bx, ay, by, osx, osy):
        a = np.ascontiguousarray(a, self.dtype)
        out = np.zeros_like(a)
        ix, iy = np.zeros(a.shape, np.int32), np.zeros(a.shape, np.int32)
        self._chk(self._fn("pbd_dt2d")(self.h, _p(a, self._ct), a.shape[0], a.shape[1], C.c_double(ax), C.c_double(bx),
                                       C.c_double(ay), C.c_double(by), osx, osy, _p(out, self._ct), _p(ix, C.c_int32),
                                       _p(iy, C.c_int32)))
        return out, ix, iy

    def hog(self, im: np.ndarray):
        im, w, hgt, cn, stride = _frame(im)
        sb = self.model.sbin
        buf = np.zeros((hgt // sb + 2) * (w // sb + 2) * 32, self.dtype)
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self._fn("pbd_hog_u8")(self.h, _p(im, C.c_uint8), w, hgt, cn, stride, _p(buf, self._ct), C.byref(a),
                                         C.byref(b)))
        return buf[: b.value * a.value * 32].reshape(b.value, a.value, 32).copy()

    def resize(self, im: np.ndarray, ow, oh):
        im, w, hgt, cn, stride = _frame(im)
        out = np.zeros((oh, ow) + ((cn,) if cn > 1 else ()), np.uint8)
        self._chk(self.L.pbd_resize_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride, _p(out, C.c_uint8), ow, oh))
        return out

    def resize_area(self, im: np.ndarray, scale):
        """pbd_resize_area_f64: resize(im, scale) of matlab/mex/resize.cc on a double image [h, w] or [h, w, 3]"""
        im = np.ascontiguousarray(im, np.float64)
        hgt, w = im.shape[:2]
        cn = 1 if im.ndim == 2 else im.shape[2]
        out = np.zeros(max(hgt, 1) * max(w, 1) * cn, np.float64)     # scale <= 1: never larger than the source
        ow, oh = C.c_int(0), C.c_int(0)
        self._chk(self.L.pbd_resize_area_f64(self.h, _p(im, C.c_double), w, hgt, cn, C.c_double(scale), _p(out, C.c_double),
                                             C.byref(ow), C.byref(oh)))
        return out[:oh.value * ow.value * cn].reshape((oh.value, ow.value) + ((cn,) if im.ndim == 3 else ())).copy()

    def reduce(self, im: np.ndarray):
        """pbd_reduce_f64: reduce(im) of matlab/mex/reduce.cc on a double image [h, w] or [h, w, 3], both dimensions >= 5"""
        im = np.ascontiguousarray(im, np.float64)
        hgt, w = im.shape[:2]
        cn = 1 if im.ndim == 2 else im.shape[2]
        out = np.zeros(max(hgt, 1) * max(w, 1) * cn, np.float64)
        ow, oh = C.c_int(0), C.c_int(0)
        self._chk(self.L.pbd_reduce_f64(self.h, _p(im, C.c_double), w, hgt, cn, _p(out, C.c_double), C.byref(ow), C.byref(oh)))
        return out[:oh.value * ow.value * cn].reshape((oh.value, ow.value) + ((cn,) if im.ndim == 3 else ())).copy()

    def warp_windows(self, im: np.ndarray, boxes, filter: int):
        """pbd_warp_windows_u8[_f64]: warppos.m's windows of the boxes ((x1, y1, x2, y2), 1-based inclusive) for filter `filter` and
        their HOG -> (windows [n, oh, ow, 3] float64, features [n, kh, kw, 32] of the handle's dtype)"""
        im, w, hgt, cn, stride = _frame(im)
        boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4)
        kh, kw = self.filter_size(filter)
        sbin = self.model.sbin
        win = np.zeros((len(boxes), (kh + 2) * sbin, (kw + 2) * sbin, 3), np.float64)
        feat = np.zeros((len(boxes), kh, kw, 32), self.dtype)
        self._chk(self._fn("pbd_warp_windows_u8")(self.h, _vp(im), w, hgt, cn, stride, _vp(boxes), len(boxes), int(filter), _vp(win),
                                                 _vp(feat)))
        return win, feat

    def warp_ms(self):
        """pbd_debug_warp_ms: (resample, hog, write) ms of the last warped-positives call, measured while set_profiling() is on"""
        ms = (C.c_float * 3)()
        self._chk(self.L.pbd_debug_warp_ms(self.h, ms))
        return tuple(ms)

    def pyrdown(self, im: np.ndarray):
        im, w, hgt, cn, stride = _frame(im)
        out = np.zeros(((hgt + 1) // 2, (w + 1) // 2) + ((cn,) if cn > 1 else ()), np.uint8)
        self._chk(self.L.pbd_pyrdown_u8(self.h, _p(im, C.c_uint8), w, hgt, cn, stride, _p(out, C.c_uint8)))
        return out

    def nms_map(self, src: np.ndarray, sz: int):
        src = np.ascontiguousarray(src, np.float32)
        out = np.zeros(src.shape, np.uint8)
        self._chk(self.L.pbd_nms_map(self.h, _p(src, C.c_float), src.shape[0], src.shape[1], sz, _p(out, C.c_uint8)))
        return out

    # ---- instrumentation -------------------------------------------------------------
    def set_profiling(self, on=True):
        self._chk(self.L.pbd_set_profiling(self.h, int(on)))

    def stage_ms(self):
        ms = (C.c_float * 6)()
        self._chk(self.L.pbd_get_stage_ms(self.h, ms))
        return dict(zip(["image_pyramid", "hog", "pdf", "dp_min", "argmin", "total"], list(ms)))

    def work(self):
        wk = (C.c_double * 6)()
        self._chk(self.L.pbd_get_work(self.h, wk))
        return dict(zip(["B_hog", "B_pdf", "F_pdf", "B_dp", "cells", "dt_elements"], list(wk)))

    def dp_timer(self, reset=False):
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.L.pbd_dp_timer(self.h, int(reset), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class Group:
    """pbd_group: one process driving several GPUs (include/pbd_c.h).  devices may repeat an ordinal."""

    def __init__(self, model, devices, gather=PBD_GATHER_AUTO, conv_mode=PBD_CONV_AUTO, max_candidates=4096,
                 dtype=np.float32, graph=0, nms_sz=0, cand_filter=None, cand_nms=None):
        self.L = lib()
        self.model = model
        self.fsize = None
        if model.is_uniform():
            self.desc = model.to_desc()
        else:
            self.desc, self.fsize = model.to_desc_sized()
        f64 = np.dtype(dtype) == np.dtype(np.float64)
        opt = pbd_options(0, conv_mode, max_candidates, 0, 0, 0, PBD_SCALAR_F64 if f64 else PBD_SCALAR_F32, graph,
                          (C.c_int32 * 2)(int(nms_sz), 0))
        dv = np.ascontiguousarray(list(devices), np.int32)
        self.g = C.c_void_p()
        if self.fsize is None:
            rc = self.L.pbd_group_create(C.byref(self.desc), C.byref(opt), _p(dv, C.c_int32), len(dv), gather, C.byref(self.g))
        else:
            rc = self.L.pbd_group_create_sized(C.byref(self.desc), _p(self.fsize, C.c_int32), C.byref(opt), _p(dv, C.c_int32), len(dv),
                                               gather, C.byref(self.g))
        if rc != PBD_OK:
            msg = self.L.pbd_group_last_error(self.g).decode() if self.g else "allocation failed"
            if self.g:
                self.L.pbd_group_destroy(self.g)
            self.g = None
            raise PbdError(rc, msg)
        self.size = self.L.pbd_group_size(self.g)
        self.gather_mode = self.L.pbd_group_gather_mode(self.g)
        self.comm_size = self.L.pbd_group_comm_size(self.g)       # ranks of the RCCL communicator (0: host gather)
        self.max_parts = self.L.pbd_max_parts(C.c_void_p(self.L.pbd_group_member(self.g, 0)))
        if cand_filter is not None:
            self.set_candidate_filter(*cand_filter)
        if cand_nms is not None:
            self.set_candidate_nms(*cand_nms)

    def set_candidate_nms(self, kind, top=0):
        """pbd_group_set_candidate_nms: every member (Handle.set_candidate_nms); detect() applies it to the union of the members' levels."""
        self._chk(self.L.pbd_group_set_candidate_nms(self.g, int(kind), int(top)))

    def set_candidate_filter(self, mode, overlap=0.0):
        """pbd_group_set_candidate_filter: every member; detect() filters the union of the members' levels."""
        self._chk(self.L.pbd_group_set_candidate_filter(self.g, int(mode), C.c_float(overlap)))

    def set_boundary_pad(self, pad=3):
        """pbd_group_set_boundary_pad: every member (Handle.set_boundary_pad)."""
        self._chk(self.L.pbd_group_set_boundary_pad(self.g, int(pad)))

    def close(self):
        if getattr(self, "g", None):
            self.L.pbd_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != PBD_OK:
            raise PbdError(rc, self.L.pbd_group_last_error(self.g).decode())

    def detect_batch(self, frames, capacity=4096):
        """frames: list of equal-sized uint8 images -> list of (heads, boxes, locs), frame f on member f % size."""
        frames, stride = _frames(frames)
        n = len(frames)
        if not n or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("detect_batch: one or more frames, all of the same shape")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        heads = np.zeros(n * capacity, HEAD_DTYPE)
        boxes = np.zeros((n * capacity, self.max_parts, 4), np.int32)
        locs = np.zeros((n * capacity, self.max_parts, 3), np.int32)
        counts = np.zeros(n, np.int32)
        self._chk(self.L.pbd_group_detect_batch_u8(self.g, ptrs, n, w, hgt, cn, stride, heads.ctypes.data_as(C.c_void_p),
                                                   _p(boxes, C.c_int32), _p(locs, C.c_int32), capacity, _p(counts, C.c_int32)))
        return [(heads[f * capacity: f * capacity + counts[f]].copy(), boxes[f * capacity: f * capacity + counts[f]].copy(),
                 locs[f * capacity: f * capacity + counts[f]].copy()) for f in range(n)]

    def detect(self, im, capacity=4096):
        """one frame, pyramid levels LPT-sharded over the members."""
        im, w, hgt, cn, stride = _frame(im)
        heads = np.zeros(capacity, HEAD_DTYPE)
        boxes = np.zeros((capacity, self.max_parts, 4), np.int32)
        locs = np.zeros((capacity, self.max_parts, 3), np.int32)
        cnt = C.c_int(0)
        self._chk(self.L.pbd_group_detect_u8(self.g, _p(im, C.c_uint8), w, hgt, cn, stride, heads.ctypes.data_as(C.c_void_p),
                                             _p(boxes, C.c_int32), _p(locs, C.c_int32), capacity, C.byref(cnt)))
        return heads[:cnt.value].copy(), boxes[:cnt.value].copy(), locs[:cnt.value].copy()


def candidates_sort(heads, boxes, locs):
    """Candidate::sort (include/Candidate.hpp:91-99) — host code inside the library."""
    heads, boxes, locs = heads.copy(), np.ascontiguousarray(boxes).copy(), np.ascontiguousarray(locs).copy()
    mp = boxes.shape[1] if boxes.ndim == 3 else 1
    rc = lib().pbd_candidates_sort(heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                   len(heads), mp)
    if rc:
        raise PbdError(rc, "pbd_candidates_sort")
    return heads, boxes, locs


def candidates_nms(heads, boxes, locs, im_w, im_h, overlap=0.0):
    """Candidate::nonMaximaSuppression (include/Candidate.hpp:277-304)."""
    heads, boxes, locs = heads.copy(), np.ascontiguousarray(boxes).copy(), np.ascontiguousarray(locs).copy()
    mp = boxes.shape[1]
    kept = C.c_int(0)
    rc = lib().pbd_candidates_nms(heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                  len(heads), mp, im_w, im_h, C.c_float(overlap), C.byref(kept))
    if rc:
        raise PbdError(rc, "pbd_candidates_nms")
    return heads[:kept.value], boxes[:kept.value], locs[:kept.value]


def candidates_nms_parts(heads, boxes, locs, overlap=0.3, top=1000):
    """matlab/detection/nms.m on sorted records (pbd_candidates_nms_parts, include/pbd_c.h) — host code inside the library."""
    heads, boxes = heads.copy(), np.ascontiguousarray(boxes, np.int32).copy()
    locs = None if locs is None else np.ascontiguousarray(locs, np.int32).copy()
    mp = boxes.shape[1]
    kept = C.c_int(0)
    rc = lib().pbd_candidates_nms_parts(heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), _p(locs, C.c_int32),
                                        len(heads), mp, C.c_float(overlap), int(top), C.byref(kept))
    if rc:
        raise PbdError(rc, "pbd_candidates_nms_parts")
    return heads[:kept.value], boxes[:kept.value], None if locs is None else locs[:kept.value]


def candidates_best_overlap(heads, boxes, gt, overlap=0.3):
    """matlab/detection/bestoverlap.m per gt box (x1, y1, x2, y2) on records in the given order (pbd_candidates_best_overlap,
    include/pbd_c.h) — host code inside the library -> (best[ngt] record index or -1, o[ngt])."""
    heads = np.ascontiguousarray(heads, HEAD_DTYPE)
    boxes = np.ascontiguousarray(boxes, np.int32)
    gt = np.ascontiguousarray(gt, np.float64).reshape(-1, 4)
    mp = boxes.shape[1]
    best = np.full(len(gt), -1, np.int32)
    o = np.zeros(len(gt), np.float64)
    rc = lib().pbd_candidates_best_overlap(heads.ctypes.data_as(C.c_void_p), _p(boxes, C.c_int32), len(heads), mp, _p(gt, C.c_double),
                                           len(gt), C.c_double(overlap), _p(best, C.c_int32), _p(o, C.c_double))
    if rc:
        raise PbdError(rc, "pbd_candidates_best_overlap")
    return best, o


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def warp_geometry(box, kh, kw, sbin):
    """pbd_warp_geometry (host code, no GPU): the crop of warppos.m for a box (x1, y1, x2, y2), 1-based inclusive ->
    dict(rect=(X1, Y1, X2, Y2), rows_first, py, px)"""
    box = np.ascontiguousarray(box, np.float64).reshape(4)
    rect = np.zeros(4, np.int32)
    rf, py, px = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib().pbd_warp_geometry(_vp(box), int(kh), int(kw), int(sbin), _vp(rect), C.byref(rf), C.byref(py), C.byref(px))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_warp_geometry")
    return dict(rect=tuple(int(v) for v in rect), rows_first=bool(rf.value), py=py.value, px=px.value)


def warp_taps(n_in, n_out):
    """pbd_warp_taps (host code, no GPU): one axis of the bilinear resize from n_in to n_out -> (index [n_out, P] int32, 0-based inside
    the crop with the mirror resolved; weight [n_out, P] float64, normalised)"""
    P = C.c_int32()
    rc = lib().pbd_warp_taps(int(n_in), int(n_out), None, None, 0, C.byref(P))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_warp_taps")
    idx, w = np.zeros((n_out, P.value), np.int32), np.zeros((n_out, P.value), np.float64)
    rc = lib().pbd_warp_taps(int(n_in), int(n_out), _vp(idx), _vp(w), idx.size, C.byref(P))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_warp_taps")
    return idx, w


def croppos(truth, nparts, w, hgt):
    """pbd_croppos (host code, no GPU): croppos.m for the first `nparts` truth boxes ((x, y, width, height), 0-based, covering
    x .. x + width) of a w x hgt frame -> (roi (x, y, width, height) of the crop, truth_out [nparts, 4] relative to it).  The crop is
    the view im[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]]."""
    t = np.ascontiguousarray(np.asarray(truth, np.int32).reshape(-1, 4)[:int(nparts)])
    if len(t) < int(nparts):
        raise ValueError("croppos: fewer truth boxes than nparts")
    roi, out = np.zeros(4, np.int32), np.zeros_like(t)
    rc = lib().pbd_croppos(_vp(t), int(nparts), int(w), int(hgt), _vp(roi), _vp(out))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_croppos")
    return tuple(int(v) for v in roi), out


class QpCache:
    """pbd_qp (include/pbd_c.h "training example cache"): the QP's cache of block-sparse examples on the device — qp_write.m,
    matlab/mex/score.cc and lincomb.cc — and the coordinate-descent solver over it (qp_one_sparse.cc, qp_one.m, qp_refresh.m, qp_opt.m,
    qp_prune.m, qp_w.m: noneg() .. weights() below), whose columns never leave the device.  Bound to `handle`, whose close() closes
    the caches it still has."""

    def __init__(self, handle: Handle, capacity: int, cpos: float = 1.0, cneg: float = 1.0, wreg=None, w0=None):
        self.handle, self.L = handle, handle.L
        wreg = None if wreg is None else np.ascontiguousarray(wreg, np.float64)
        w0 = None if w0 is None else np.ascontiguousarray(w0, np.float64)
        size = handle.model.feature_layout()["size"]
        for v in (wreg, w0):
            if v is not None and v.size != size:
                raise ValueError(f"wreg / w0 must have Model.feature_layout()['size'] = {size} elements")
        self.q = C.c_void_p()
        handle._chk(self.L.pbd_qp_create(handle.h, int(capacity), float(cpos), float(cneg), _vp(wreg), _vp(w0), C.byref(self.q)))
        if not hasattr(handle, "_caches"):
            handle._caches = []
        handle._caches.append(weakref.ref(self))   # Handle.close() closes the caches it still has: nothing of theirs outlives it

    def dims(self):
        """(len, k, capacity, n): dense length, column length, capacity and examples held"""
        v = [C.c_int() for _ in range(4)]
        self.handle._chk(self.L.pbd_qp_dims(self.q, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def footprint(self) -> int:
        b = C.c_size_t()
        self.handle._chk(self.L.pbd_qp_footprint(self.q, C.byref(b)))
        return b.value

    def write(self, heads, locs, label: int, id: int) -> int:
        """pbd_qp_write: the records (as Handle.candidates_features takes them) appended as examples; returns how many were."""
        heads, lc = self.handle._records(heads, locs)
        written = C.c_int(-1)
        self.handle._chk(self.L.pbd_qp_write(self.q, heads.ctypes.data_as(C.c_void_p), _vp(lc), len(heads), int(label), int(id),
                                             C.byref(written)))
        return written.value

    def write_warped(self, im, boxes, filter: int, bias: int, min_area: float = 0.0, ids=None):
        """pbd_qp_write_warped_u8: train.m's poswarp — the boxes ((x1, y1, x2, y2), 1-based inclusive) of the 8-bit frame cropped, resized,
        HOGed and appended as positives [bias | window of `filter`] without leaving the device -> (written, status [n] int32:
        PBD_WARP_WRITTEN / _SKIPPED (area below min_area) / _FULL).  ids: one id per box (None: the box's index)."""
        im, w, hgt, cn, stride = _frame(im)
        boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4)
        ids = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(len(boxes))
        status = np.full(len(boxes), -1, np.int32)
        written = C.c_int(-1)
        self.handle._chk(self.L.pbd_qp_write_warped_u8(self.q, _vp(im), w, hgt, cn, stride, _vp(boxes), _vp(ids), len(boxes), int(filter),
                                                       int(bias), float(min_area), _vp(status), C.byref(written)))
        return written.value, status

    def write_warped_dev(self, dptr, w=None, hgt=None, cn=None, boxes=None, filter: int = 0, bias: int = 0, min_area: float = 0.0, ids=None,
                         stride=None):
        """pbd_qp_write_warped_dev_u8: write_warped on a frame in device memory — a DeviceFrame, or an integer device pointer with
        w, hgt, cn (stride: bytes between rows, default w * cn) —, copied device to device; the same columns, status and refusals"""
        if isinstance(dptr, DeviceFrame):
            fr = dptr
            fr.sync()
            dptr, w, hgt, cn, stride = fr.dptr, fr.w, fr.hgt, fr.cn, fr.stride
        boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4)
        ids = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(len(boxes))
        status = np.full(len(boxes), -1, np.int32)
        written = C.c_int(-1)
        self.handle._chk(self.L.pbd_qp_write_warped_dev_u8(self.q, C.c_void_p(dptr), int(w), int(hgt), int(cn),
                                                           int(w) * int(cn) if stride is None else int(stride), _vp(boxes), _vp(ids),
                                                           len(boxes), int(filter), int(bias), float(min_area), _vp(status),
                                                           C.byref(written)))
        return written.value, status

    @staticmethod
    def _inds(inds):
        return None if inds is None else np.ascontiguousarray(inds, np.int32).ravel()

    def score(self, w, inds=None) -> np.ndarray:
        """pbd_qp_score: score.cc's w . x of the examples `inds` (None: all n), float64"""
        length, _, _, n = self.dims()
        w = np.ascontiguousarray(w, np.float64).ravel()
        if w.size != length:
            raise ValueError(f"w must have {length} elements")
        inds = self._inds(inds)
        cnt = n if inds is None else len(inds)
        out = np.zeros(cnt, np.float64)
        self.handle._chk(self.L.pbd_qp_score(self.q, _vp(w), _vp(inds), cnt, _vp(out)))
        return out

    def score_dev(self, d_w: int, d_inds: int, n: int, d_out: int) -> None:
        """pbd_qp_score_dev: integer device pointers (d_inds 0: examples 0 .. n - 1); enqueued on the handle's stream"""
        self.handle._chk(self.L.pbd_qp_score_dev(self.q, C.c_void_p(d_w), C.c_void_p(d_inds or None), int(n), C.c_void_p(d_out)))

    def lincomb(self, a, inds=None) -> np.ndarray:
        """pbd_qp_lincomb: lincomb.cc's sum of a[i] * x(:, i) over `inds`, in that order (None: all n); a: one value per example of
        the capacity (shorter: padded with zeros)"""
        length, _, cap, n = self.dims()
        av = np.zeros(cap, np.float64)
        a = np.asarray(a, np.float64).ravel()
        if a.size > cap:
            raise ValueError("a has more elements than the cache's capacity")
        av[:a.size] = a
        inds = self._inds(inds)
        out = np.zeros(length, np.float64)
        self.handle._chk(self.L.pbd_qp_lincomb(self.q, _vp(av), _vp(inds), n if inds is None else len(inds), _vp(out)))
        return out

    def lincomb_dev(self, d_a: int, d_inds: int, n: int, d_w_out: int) -> None:
        self.handle._chk(self.L.pbd_qp_lincomb_dev(self.q, C.c_void_p(d_a), C.c_void_p(d_inds or None), int(n), C.c_void_p(d_w_out)))

    def keep(self, inds) -> None:
        """pbd_qp_keep: qp_prune.m's move — the examples `inds` (strictly ascending) become 0 .. len(inds) - 1"""
        inds = self._inds(inds)
        self.handle._chk(self.L.pbd_qp_keep(self.q, _vp(inds), len(inds)))

    def get(self, i0: int = 0, n=None):
        """pbd_qp_get: (x [n, k] float32, ids [n, 5] int32, b [n] float32, d [n] float64) of examples i0 .. i0 + n - 1 (None: up to
        the cache's n)"""
        _, k, _, have = self.dims()
        n = max(have - i0, 0) if n is None else int(n)
        x, ids = np.zeros((n, k), np.float32), np.zeros((n, 5), np.int32)
        b, d = np.zeros(n, np.float32), np.zeros(n, np.float64)
        self.handle._chk(self.L.pbd_qp_get(self.q, int(i0), n, _vp(x), _vp(ids), _vp(b), _vp(d)))
        return x, ids, b, d

    def put(self, x, ids=None, b=None, d=None) -> None:
        """pbd_qp_put: appends columns made elsewhere (x [n, k]; ids / b / d default to zeros)"""
        _, k, _, _ = self.dims()
        x = np.ascontiguousarray(x, np.float32).reshape(-1, k)
        n = len(x)
        ids = np.zeros((n, 5), np.int32) if ids is None else np.ascontiguousarray(ids, np.int32).reshape(n, 5)
        b = np.zeros(n, np.float32) if b is None else np.ascontiguousarray(b, np.float32).reshape(n)
        d = np.zeros(n, np.float64) if d is None else np.ascontiguousarray(d, np.float64).reshape(n)
        self.handle._chk(self.L.pbd_qp_put(self.q, n, _vp(x), _vp(ids), _vp(b), _vp(d)))

    # ---- the QP solver (include/pbd_c.h "QP solver") ----
    def noneg(self, idx) -> None:
        """pbd_qp_noneg: the dense indices clamped at zero (Model.qp_vectors()[3])"""
        idx = np.ascontiguousarray(idx, np.int32).ravel()
        self.handle._chk(self.L.pbd_qp_noneg(self.q, _vp(idx), len(idx)))

    def fix(self, nfix: int) -> None:
        """pbd_qp_fix: svfix = examples 0 .. nfix - 1"""
        self.handle._chk(self.L.pbd_qp_fix(self.q, int(nfix)))

    def state(self):
        """pbd_qp_state_get: (a [capacity] float64, sv [capacity] uint8, w [len] float64, stats [4] = l, lb, lb_old, ub)"""
        length, _, cap, _ = self.dims()
        a, sv, w, st = np.zeros(cap), np.zeros(cap, np.uint8), np.zeros(length), np.zeros(4)
        self.handle._chk(self.L.pbd_qp_state_get(self.q, _vp(a), _vp(sv), _vp(w), _vp(st)))
        return a, sv, w, st

    def support(self) -> np.ndarray:
        """pbd_qp_state_get for sv alone: the support-vector flags of the n examples held (capacity bytes over PCIe, nothing else)"""
        _, _, cap, n = self.dims()
        sv = np.zeros(cap, np.uint8)
        self.handle._chk(self.L.pbd_qp_state_get(self.q, None, _vp(sv), None, None))
        return sv[:n]

    def set_state(self, a=None, sv=None) -> None:
        """pbd_qp_state_put: a and / or sv of examples 0 .. len - 1"""
        a = None if a is None else np.ascontiguousarray(a, np.float64).ravel()
        sv = None if sv is None else np.ascontiguousarray(sv, np.uint8).ravel()
        if a is not None and sv is not None and len(a) != len(sv):
            raise ValueError("a and sv must have the same length")
        n = len(a) if a is not None else (len(sv) if sv is not None else 0)
        self.handle._chk(self.L.pbd_qp_state_put(self.q, _vp(a), _vp(sv), n))

    def solve_pass(self, order) -> float:
        """pbd_qp_pass: one qp_one_sparse.cc pass over the examples `order`; returns its loss"""
        order = self._inds(order)
        loss = C.c_double()
        self.handle._chk(self.L.pbd_qp_pass(self.q, _vp(order), len(order), C.byref(loss)))
        return loss.value

    def one(self, order) -> None:
        """pbd_qp_one: qp_one.m from its pass on — pass, refresh, sv(svfix) = 1, lb_old / lb / ub"""
        order = self._inds(order)
        self.handle._chk(self.L.pbd_qp_one(self.q, _vp(order), len(order)))

    def refresh(self) -> None:
        self.handle._chk(self.L.pbd_qp_refresh(self.q))

    def loss(self) -> float:
        """pbd_qp_loss: computeloss of qp_opt.m over all n examples"""
        v = C.c_double()
        self.handle._chk(self.L.pbd_qp_loss(self.q, C.byref(v)))
        return v.value

    def opt(self, tol: float = .05, max_iter: int = 1000, seed: int = 0):
        """pbd_qp_opt: qp_opt.m's loop -> (lb, ub, passes)"""
        lb, ub, passes = C.c_double(), C.c_double(), C.c_int()
        self.handle._chk(self.L.pbd_qp_opt(self.q, float(tol), int(max_iter), int(seed), C.byref(lb), C.byref(ub), C.byref(passes)))
        return lb.value, ub.value, passes.value

    def prune(self) -> int:
        """pbd_qp_prune: qp_prune.m -> the examples kept"""
        n = C.c_int()
        self.handle._chk(self.L.pbd_qp_prune(self.q, C.byref(n)))
        return n.value

    def weights(self) -> np.ndarray:
        """pbd_qp_weights: qp_w.m's w ./ wreg + w0"""
        out = np.zeros(self.dims()[0])
        self.handle._chk(self.L.pbd_qp_weights(self.q, _vp(out)))
        return out

    def apply_weights(self) -> None:
        """pbd_qp_apply_weights: train.m's model = vec2model(qp_w, model) — weights() into the cache's handle, without leaving the device"""
        self.handle._chk(self.L.pbd_qp_apply_weights(self.q))
        self.handle._model_follows()

    # ---- one training round (include/pbd_c.h "one training round") ----
    def clear(self) -> None:
        """pbd_qp_clear: train.m:75's qp.n = 0 — the cache keeps capacity, wreg, w0, noneg and binding and is otherwise a new cache's,
        the solver's state (a, sv, w, the bounds, nfix) included"""
        self.handle._chk(self.L.pbd_qp_clear(self.q))

    def positive_threshold(self, q: float = .05):
        """pbd_qp_positive_threshold: train.m:116-118 on the device — Model.positive_threshold(score(w + w0 * wreg, positives) / cpos,
        q) with the solver's resident w, bit for bit -> (thresh, the number of positives)"""
        t, m = C.c_double(), C.c_int()
        self.handle._chk(self.L.pbd_qp_positive_threshold(self.q, float(q), C.byref(t), C.byref(m)))
        return t.value, m.value

    # ---- hard-negative mining (include/pbd_c.h "hard-negative mining") ----
    def mine(self, im, id: int):
        """pbd_qp_mine_u8: train.m:102's detect(im, model, -1, [], 0, id, -1) on the cache's handle — the frame is detected as
        Handle.detect would detect it (the handle's threshold, candidate filter, pad and pyramid kind), its records stay on the device
        and become examples of label -1, ub grows by every record's slack -> (records, written, action): the frame's records, how many
        the cache had room for, and PBD_MINE_NONE / _ONE / _OPT: what detect.m would now run.  train.m:96's model.interval = 2 is
        Handle.set_interval."""
        im, w, hgt, cn, stride = _frame(im)
        rec, wr, act = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = self.L.pbd_qp_mine_u8(self.q, _vp(im), w, hgt, cn, stride, int(id), C.byref(rec), C.byref(wr), C.byref(act))
        self._mine_chk(rc, [rec.value])
        return rec.value, wr.value, act.value

    def mine_dev(self, dptr: int, w, hgt, cn, id: int, stride=None):
        """pbd_qp_mine_dev_u8: the same on a frame in device memory (an integer device pointer), read in place"""
        rec, wr, act = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = self.L.pbd_qp_mine_dev_u8(self.q, C.c_void_p(dptr), w, hgt, cn, w * cn if stride is None else int(stride), int(id),
                                       C.byref(rec), C.byref(wr), C.byref(act))
        self._mine_chk(rc, [rec.value])
        return rec.value, wr.value, act.value

    def mine_batch(self, ims, ids):
        """pbd_qp_mine_batch_u8: same-sized frames as one batch -> (records [n] int32, written [n] int32, action); the examples and ub
        are those of the frames mined one by one, in bits"""
        frames, stride = _frames(ims)
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        if not frames or len(ids) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("mine_batch: one id per frame, frames of one shape")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        rec, wr, act = np.full(len(frames), -1, np.int32), np.full(len(frames), -1, np.int32), C.c_int(-1)
        rc = self.L.pbd_qp_mine_batch_u8(self.q, ptrs, len(frames), w, hgt, cn, stride, _vp(ids), _vp(rec), _vp(wr), C.byref(act))
        self._mine_chk(rc, rec)
        return rec, wr, act.value

    def mine_stored(self, store: "PyramidStore", slot: int, id: int):
        """pbd_qp_mine_stored: mine() on the frame that was put into `slot` of `store` (or a StoredFrame): the same records, examples,
        ub and action as mine(image, id) on this cache's handle, in bits — only the features come from the slot"""
        store, slot = _stored(store, slot)
        rec, wr, act = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = self.L.pbd_qp_mine_stored(self.q, store.s, int(slot), int(id), C.byref(rec), C.byref(wr), C.byref(act))
        self._mine_chk(rc, [rec.value])
        return rec.value, wr.value, act.value

    def mine_batch_stored(self, store: "PyramidStore", slots, ids):
        """pbd_qp_mine_batch_stored: mine_batch() on the frames of `slots` (same-sized), one id per slot"""
        sl = np.ascontiguousarray([int(getattr(x, "slot", x)) for x in slots], np.int32)
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        if not len(sl) or len(ids) != len(sl):
            raise ValueError("mine_batch_stored: one id per slot")
        rec, wr, act = np.full(len(sl), -1, np.int32), np.full(len(sl), -1, np.int32), C.c_int(-1)
        rc = self.L.pbd_qp_mine_batch_stored(self.q, store.s, _vp(sl), len(sl), _vp(ids), _vp(rec), _vp(wr), C.byref(act))
        self._mine_chk(rc, rec)
        return rec, wr, act.value

    # ---- latent positives (include/pbd_c.h "latent positives") ----
    def write_latent(self, im, truth, overlap, id: int, mix=None, component=-1):
        """pbd_qp_write_latent_u8: train.m:187's detect(im, model, 0, bbox, overlap, id, 1) on the cache's handle — the frame is
        detected as Handle.detect_latent would detect it, its pose stays on the device and becomes one example of label +1 -> the
        frame's block, a LATENT_EXAMPLE_DTYPE record (found, written, component, level, x, y, score).  found = 0: no pose, nothing
        written; found = 1, written = 0: the cache was full.  After a refused call the block is in `last_latent`."""
        im, w, hgt, cn, stride = _frame(im)
        tr, mx = self.handle._latent_args(truth, mix)
        out = np.zeros(1, LATENT_EXAMPLE_DTYPE)
        self.last_latent = out
        self.handle._chk(self.L.pbd_qp_write_latent_u8(self.q, _vp(im), w, hgt, cn, stride, _vp(tr), _vp(mx), int(component),
                                                       C.c_double(overlap), int(id), _vp(out)))
        return out[0]

    def write_latent_dev(self, dptr: int, w, hgt, cn, truth, overlap, id: int, mix=None, component=-1, stride=None):
        """pbd_qp_write_latent_dev_u8: the same on a frame in device memory (an integer device pointer), read in place"""
        tr, mx = self.handle._latent_args(truth, mix)
        out = np.zeros(1, LATENT_EXAMPLE_DTYPE)
        self.last_latent = out
        self.handle._chk(self.L.pbd_qp_write_latent_dev_u8(self.q, C.c_void_p(dptr), w, hgt, cn, w * cn if stride is None else int(stride),
                                                           _vp(tr), _vp(mx), int(component), C.c_double(overlap), int(id), _vp(out)))
        return out[0]

    def write_latent_batch(self, ims, truths, overlap, ids, mixes=None, component=-1):
        """pbd_qp_write_latent_batch_u8: same-sized frames as one batch, a truth set (and mixture set) and an id per frame -> the
        frames' blocks [n] (LATENT_EXAMPLE_DTYPE); the examples are those of the frames written one by one, in bits"""
        frames, stride = _frames(ims)
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        if not frames or len(ids) != len(frames) or len(truths) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("write_latent_batch: one truth set and one id per frame, frames of one shape")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        tr, mx = self.handle._latent_args(np.stack([np.asarray(t, np.int32) for t in truths]),
                                          None if mixes is None else np.stack([np.asarray(m, np.int32) for m in mixes]), len(frames))
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        out = np.zeros(len(frames), LATENT_EXAMPLE_DTYPE)
        self.last_latent = out
        self.handle._chk(self.L.pbd_qp_write_latent_batch_u8(self.q, ptrs, len(frames), w, hgt, cn, stride, _vp(tr), _vp(mx),
                                                             int(component), C.c_double(overlap), _vp(ids), _vp(out)))
        return out

    def _mine_chk(self, rc, records):
        if rc == PBD_ERR_CAPACITY:   # (the needed count travels with the error, as Handle.detect's does)
            msg = self.L.pbd_last_error(self.handle.h).decode()
            err = PbdError(rc, msg)
            err.records = [int(r) for r in records]
            raise err
        self.handle._chk(rc)

    def close(self):
        if getattr(self, "q", None):   # (a live cache implies a live handle: Handle.close() closes its caches before itself)
            self.L.pbd_qp_destroy(self.q)
        self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- evaluation: eval_pck.m, eval_apk.m, VOCap.m (include/pbd_c.h "evaluation ledger") ------------------------------------------------
# ---- pyramid store (include/pbd_c.h "pyramid store") -------------------------------------------------------------------------------------
def pyrstore_layout(w, hgt, sbin, interval, kind=PBD_PYRAMID_OPENCV, pad=0):
    """pbd_pyrstore_layout (host only, no GPU): (nlevels, level_off [nlevels] int64 element offsets, total elements) of one frame's
    feature pyramid; raises PbdError(PBD_ERR_ARG) for a frame too small for `interval` levels"""
    n, total = C.c_int(0), C.c_longlong(0)
    off = np.zeros(PBD_PYRSTORE_MAX_LEVELS, np.int64)
    rc = lib().pbd_pyrstore_layout(int(w), int(hgt), int(sbin), int(interval), int(kind), int(pad), C.byref(n), _vp(off), C.byref(total))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_pyrstore_layout: no pyramid for this frame and these settings")
    return n.value, off[:n.value].copy(), total.value


class StoredFrame:
    """One slot of a PyramidStore, as an item detectStored / mineNegatives / train() take where they take an image"""

    def __init__(self, store: "PyramidStore", slot: int):
        self.store, self.slot = store, int(slot)

    def __repr__(self):
        return f"StoredFrame(slot={self.slot})"


def _stored(store, slot):
    """(store, slot) from (store, slot) or (StoredFrame, None) / (store, StoredFrame)"""
    if isinstance(store, StoredFrame):
        return store.store, store.slot
    if isinstance(slot, StoredFrame):
        return slot.store, slot.slot
    return store, slot


class PyramidStore:
    """pbd_pyrstore: `slots` device-resident feature pyramids, each of one frame as `handle` (the producer) computes it.  Any handle
    on the same device whose sbin, interval, pyramid kind, boundary pad and dtype equal the producer's at this moment detects and mines
    from a slot (Handle.detect_stored, QpCache.mine_stored) with the image entries' results, in bits.  Sized for frames of up to
    max_w x max_h.  Close the store before its producer (Handle.close() does it for the stores it still has)."""

    def __init__(self, handle: Handle, slots: int, max_w: int, max_h: int):
        self.handle, self.L = handle, handle.L
        self.s = C.c_void_p()
        handle._chk(self.L.pbd_pyrstore_create(handle.h, int(slots), int(max_w), int(max_h), C.byref(self.s)))
        if not hasattr(handle, "_caches"):
            handle._caches = []
        handle._caches.append(weakref.ref(self))   # Handle.close() closes what it still has: the store goes before its producer

    def _chk(self, rc):
        self.handle._chk(rc)

    def dims(self):
        """dict(slots, sbin, interval, kind, pad, scalar_bytes, slot_bytes): the store's size and signature"""
        v = [C.c_int() for _ in range(6)]
        b = C.c_size_t()
        self._chk(self.L.pbd_pyrstore_dims(self.s, *[C.byref(x) for x in v], C.byref(b)))
        return dict(zip(("slots", "sbin", "interval", "kind", "pad", "scalar_bytes"), (x.value for x in v)), slot_bytes=b.value)

    def slot(self, slot: int):
        """(w, hgt, cn, nlevels) of the frame in `slot`; w == 0: empty"""
        v = [C.c_int() for _ in range(4)]
        self._chk(self.L.pbd_pyrstore_slot(self.s, int(slot), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def put(self, slot: int, im) -> StoredFrame:
        """pbd_pyrstore_put_u8: the producer's pyramid of the 8-bit frame `im` into `slot` (synchronous)"""
        im, w, hgt, cn, stride = _frame(im)
        self._chk(self.L.pbd_pyrstore_put_u8(self.s, int(slot), _vp(im), w, hgt, cn, stride))
        return StoredFrame(self, slot)

    def put_dev(self, slot: int, dptr: int, w, hgt, cn, stride=None) -> StoredFrame:
        """pbd_pyrstore_put_dev_u8: the same from a frame in device memory (an integer device pointer)"""
        self._chk(self.L.pbd_pyrstore_put_dev_u8(self.s, int(slot), C.c_void_p(dptr), w, hgt, cn, w * cn if stride is None else int(stride)))
        return StoredFrame(self, slot)

    def put_batch(self, slots, ims):
        """pbd_pyrstore_put_batch_u8: same-sized frames through the producer as one batch, frame f into slots[f]"""
        frames, stride = _frames(ims)
        sl = np.ascontiguousarray([int(x) for x in slots], np.int32)
        if not frames or len(sl) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("put_batch: one slot per frame, frames of one shape")
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        self._chk(self.L.pbd_pyrstore_put_batch_u8(self.s, _vp(sl), ptrs, len(frames), w, hgt, cn, stride))
        return [StoredFrame(self, x) for x in sl]

    def level(self, slot: int, level: int) -> np.ndarray:
        """pbd_pyrstore_get_level: level `level` of the slot's pyramid, [ch][cw][32] in the producer's dtype"""
        w, hgt, _, n = self.slot(slot)
        if w == 0 or not 0 <= level < n:   # (the library words the refusal)
            self._chk(self.L.pbd_pyrstore_get_level(self.s, int(slot), int(level), _vp(np.zeros(1)), 0))
        d = self.dims()
        _, off, total = pyrstore_layout(w, hgt, d["sbin"], d["interval"], d["kind"], d["pad"])
        nel = int((off[level + 1] if level + 1 < n else total) - off[level])
        dt = np.float64 if d["scalar_bytes"] == 8 else np.float32
        g = self.handle.geometry(w, hgt)   # (the level's shape: the producer's geometry while its settings are still the store's)
        shape = (int(g["cell_h"][level]), int(g["cell_w"][level]), 32) if level < g["nlevels"] else (0, 0, 32)
        out = np.zeros(shape if shape[0] * shape[1] * 32 == nel else (nel // 32, 32), dt)
        self._chk(self.L.pbd_pyrstore_get_level(self.s, int(slot), int(level), _vp(out), C.c_size_t(out.nbytes)))
        return out

    def frames(self):
        """a StoredFrame per occupied slot, in slot order"""
        return [StoredFrame(self, i) for i in range(self.dims()["slots"]) if self.slot(i)[0] > 0]

    def close(self):
        if getattr(self, "s", None):   # (a live store implies a live producer: Handle.close() closes its stores before itself)
            self.L.pbd_pyrstore_destroy(self.s)
        self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _persons(points, scale, P=None):
    """(points [ngt, P, 2] float64, scale [ngt] float64) of one frame's annotated persons"""
    scale = np.ascontiguousarray(scale, np.float64).reshape(-1)
    points = np.ascontiguousarray(points, np.float64)
    points = points.reshape(len(scale), -1, 2) if P is None else points.reshape(len(scale), P, 2)
    return points, scale


def eval_keypoint_dist(boxes, points):
    """pbd_eval_keypoint_dist (host code, no GPU): one record's part boxes [P, 4] against points [P, 2] -> d [P]"""
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    points = np.ascontiguousarray(points, np.float64).reshape(len(boxes), 2)
    d = np.zeros(len(boxes), np.float64)
    rc = lib().pbd_eval_keypoint_dist(_vp(boxes), len(boxes), _vp(points), _vp(d))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_eval_keypoint_dist")
    return d


def eval_pck_host(dist, scale, thresh=.5, rule=PBD_EVAL_SCALE_LAST):
    """pbd_eval_pck_host (host code, no GPU): dist [N, P], scale [N] -> pck [P]"""
    dist = np.ascontiguousarray(dist, np.float64)
    scale = np.ascontiguousarray(scale, np.float64).reshape(-1)
    if dist.ndim != 2 or len(dist) != len(scale):
        raise ValueError("eval_pck_host: dist [N, P], scale [N]")
    pck = np.zeros(dist.shape[1], np.float64)
    rc = lib().pbd_eval_pck_host(_vp(dist), _vp(scale), len(scale), dist.shape[1], float(thresh), int(rule), _vp(pck))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_eval_pck_host")
    return pck


def eval_apk_match_host(heads, boxes, points, scale, nparts, thresh=.5):
    """pbd_eval_apk_match_host (host code, no GPU): one frame's records in the given order against its persons -> tp [count, nparts] uint8"""
    heads = np.ascontiguousarray(heads, HEAD_DTYPE)
    boxes = np.ascontiguousarray(boxes, np.int32)
    if boxes.ndim != 3 or boxes.shape[0] != len(heads) or boxes.shape[2] != 4:
        raise ValueError("eval_apk_match_host: boxes [count, max_parts, 4]")
    points, scale = _persons(points, scale, nparts)
    tp = np.zeros((len(heads), nparts), np.uint8)
    rc = lib().pbd_eval_apk_match_host(_vp(heads), _vp(boxes), len(heads), boxes.shape[1], int(nparts), _vp(points), _vp(scale), len(scale),
                                       float(thresh), _vp(tp))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_eval_apk_match_host")
    return tp


def eval_ap_host(score, tp, npos, curves=False):
    """pbd_eval_ap_host (host code, no GPU): score [M], tp [M, P], npos -> apk [P] (curves: also prec, rec [P, M] in sorted order)"""
    score = np.ascontiguousarray(score, np.float32).reshape(-1)
    tp = np.ascontiguousarray(tp, np.uint8)
    if tp.ndim != 2 or tp.shape[0] != len(score):
        raise ValueError("eval_ap_host: tp [M, P]")
    P = tp.shape[1]
    apk = np.zeros(P, np.float64)
    prec, rec = (np.zeros((P, len(score)), np.float64), np.zeros((P, len(score)), np.float64)) if curves else (None, None)
    rc = lib().pbd_eval_ap_host(_vp(score), _vp(tp), len(score), P, int(npos), _vp(apk), _vp(prec), _vp(rec))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_eval_ap_host")
    return (apk, prec, rec) if curves else apk


class Eval:
    """pbd_eval (include/pbd_c.h "evaluation ledger"): per-instance keypoint distances (PCK) and per-detection true-positive flags (APK)
    accumulated on the device.  Bound to `handle`, whose close() closes the ledgers it still has.  After PBD_ERR_CAPACITY the PbdError
    carries .needed (instances or detections the ledger would have had to hold) and nothing was added."""

    def __init__(self, handle: Handle, nparts: int, max_instances: int, max_detections: int, apk_thresh: float = .5):
        self.handle, self.L, self.P = handle, handle.L, int(nparts)
        self.q = C.c_void_p()
        handle._chk(self.L.pbd_eval_create(handle.h, int(nparts), int(max_instances), int(max_detections), float(apk_thresh),
                                           C.byref(self.q)))
        if not hasattr(handle, "_caches"):
            handle._caches = []
        handle._caches.append(weakref.ref(self))

    def _chk(self, rc, needed=None):
        if rc == PBD_ERR_CAPACITY:
            err = PbdError(rc, self.L.pbd_last_error(self.handle.h).decode())
            err.needed = None if needed is None else needed.value
            raise err
        self.handle._chk(rc)

    def dims(self):
        """(P, N, M, npos, frames)"""
        v = [C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), C.c_int()]
        self.handle._chk(self.L.pbd_eval_dims(self.q, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def reset(self):
        self.handle._chk(self.L.pbd_eval_reset(self.q))

    def get(self):
        """the ledger: dict(dist [N, P], scale [N], score [M], tp [M, P])"""
        P, N, M, _, _ = self.dims()
        out = dict(dist=np.zeros((N, P), np.float64), scale=np.zeros(N, np.float64), score=np.zeros(M, np.float32),
                   tp=np.zeros((M, P), np.uint8))
        self.handle._chk(self.L.pbd_eval_get(self.q, _vp(out["dist"]), _vp(out["scale"]), _vp(out["score"]), _vp(out["tp"])))
        return out

    def add_pck_records(self, heads, boxes, found, points, scale):
        """pbd_eval_add_pck_records: per person its selected pose (heads / boxes [ngt, max_parts, 4], found [ngt]) -> ngt instances"""
        points, scale = _persons(points, scale, self.P)
        heads = np.ascontiguousarray(heads, HEAD_DTYPE)
        boxes = np.ascontiguousarray(boxes, np.int32)
        found = np.ascontiguousarray(found, np.int32)
        if not (len(heads) == len(found) == len(scale)) or boxes.shape != (len(scale), self.handle.max_parts, 4):
            raise ValueError("add_pck_records: one record slot and one found flag per person, boxes [ngt, max_parts, 4]")
        need = C.c_int(0)
        self._chk(self.L.pbd_eval_add_pck_records(self.q, _vp(heads), _vp(boxes), _vp(found), _vp(points), _vp(scale), len(scale),
                                                  C.byref(need)), need)

    def add_apk_records(self, heads, boxes, points, scale):
        """pbd_eval_add_apk_records: ONE frame's records in the given order against its persons -> len(heads) rows"""
        points, scale = _persons(points, scale, self.P)
        heads = np.ascontiguousarray(heads, HEAD_DTYPE)
        boxes = np.ascontiguousarray(boxes, np.int32)
        if boxes.shape != (len(heads), self.handle.max_parts, 4):
            raise ValueError("add_apk_records: boxes [count, max_parts, 4]")
        need = C.c_int(0)
        self._chk(self.L.pbd_eval_add_apk_records(self.q, _vp(heads), _vp(boxes), len(heads), _vp(points), _vp(scale), len(scale),
                                                  C.byref(need)), need)

    def _batch_persons(self, frames, persons):
        frames, stride = _frames(frames)
        if not frames or len(persons) != len(frames) or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("evaluation batch: one (points, scale) pair per frame, frames of one shape")
        nb = len(frames)
        pts = np.zeros((nb, PBD_GT_MAX, self.P, 2), np.float64)
        sc = np.zeros((nb, PBD_GT_MAX), np.float64)
        ngt = np.zeros(nb, np.int32)
        for f, (p, s) in enumerate(persons):
            p, s = _persons(p, s, self.P)
            if len(s) > PBD_GT_MAX:
                raise ValueError("evaluation batch: at most PBD_GT_MAX persons per frame")
            pts[f, :len(s)], sc[f, :len(s)], ngt[f] = p, s, len(s)
        hgt, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        ptrs = (C.c_void_p * nb)(*[f.ctypes.data for f in frames])
        return frames, ptrs, nb, w, hgt, cn, stride, pts, sc, ngt

    def pck_frame(self, im, points, scale, overlap=0.3):
        """pbd_eval_pck_frame_u8: the frame as Handle.detect_gtbox on the persons' keypoint boxes -> found [ngt]; self.records = the
        frame's records in front of the selection"""
        im, w, hgt, cn, stride = _frame(im)
        points, scale = _persons(points, scale, self.P)
        found = np.zeros(len(scale), np.int32)
        nrec, need = C.c_int(0), C.c_int(0)
        rc = self.L.pbd_eval_pck_frame_u8(self.q, _vp(im), w, hgt, cn, stride, _vp(points), _vp(scale), len(scale), float(overlap),
                                          _vp(found), C.byref(nrec), C.byref(need))
        self.records = nrec.value
        self._chk(rc, need)
        return found

    def pck_batch(self, frames, persons, overlap=0.3):
        """pbd_eval_pck_frame_batch_u8: persons = [(points, scale)] per frame -> [found] per frame"""
        frames, ptrs, nb, w, hgt, cn, stride, pts, sc, ngt = self._batch_persons(frames, persons)
        found = np.zeros((nb, PBD_GT_MAX), np.int32)
        nrec, need = C.c_int(0), C.c_int(0)
        rc = self.L.pbd_eval_pck_frame_batch_u8(self.q, ptrs, nb, w, hgt, cn, stride, _vp(pts), _vp(sc), _vp(ngt), float(overlap),
                                                _vp(found), C.byref(nrec), C.byref(need))
        self.records = nrec.value
        self._chk(rc, need)
        return [found[f, :ngt[f]].copy() for f in range(nb)]

    def apk_frame(self, im, points, scale) -> int:
        """pbd_eval_apk_frame_u8: the frame as Handle.detect (threshold, candidate mode and NMS of the handle) -> its final records"""
        im, w, hgt, cn, stride = _frame(im)
        points, scale = _persons(points, scale, self.P)
        rec, need = C.c_int(0), C.c_int(0)
        rc = self.L.pbd_eval_apk_frame_u8(self.q, _vp(im), w, hgt, cn, stride, _vp(points), _vp(scale), len(scale), C.byref(rec),
                                          C.byref(need))
        self.records = [rec.value]
        self._chk(rc, need)
        return rec.value

    def apk_batch(self, frames, persons):
        """pbd_eval_apk_frame_batch_u8 -> records [nframes]"""
        frames, ptrs, nb, w, hgt, cn, stride, pts, sc, ngt = self._batch_persons(frames, persons)
        rec = np.zeros(nb, np.int32)
        need = C.c_int(0)
        rc = self.L.pbd_eval_apk_frame_batch_u8(self.q, ptrs, nb, w, hgt, cn, stride, _vp(pts), _vp(sc), _vp(ngt), _vp(rec), C.byref(need))
        self.records = [int(r) for r in rec]
        self._chk(rc, need)
        return rec

    def pck(self, thresh=.5, rule=PBD_EVAL_SCALE_LAST) -> np.ndarray:
        out = np.zeros(self.P, np.float64)
        self.handle._chk(self.L.pbd_eval_pck(self.q, float(thresh), int(rule), _vp(out)))
        return out

    def apk(self, curves=False):
        """apk [P]; curves: (apk, prec [P, M], rec [P, M]) in sorted order"""
        M = self.dims()[2]
        out = np.zeros(self.P, np.float64)
        prec, rec = (np.zeros((self.P, M), np.float64), np.zeros((self.P, M), np.float64)) if curves else (None, None)
        self.handle._chk(self.L.pbd_eval_apk(self.q, _vp(out), _vp(prec), _vp(rec)))
        return (out, prec, rec) if curves else out

    def close(self):
        if getattr(self, "q", None):   # (a live ledger implies a live handle: Handle.close() closes its ledgers before itself)
            self.L.pbd_eval_destroy(self.q)
        self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- part mixtures: k_means.m, clusterparts.m (include/pbd_c.h "part mixtures") ------------------------------------------------------
def kmeans_host(X, k=None, c0=None, state0=0, max_iter=1000):
    """pbd_kmeans_host (host code, no GPU): X [n, m]; c0 [k, m]: the k_means(X, C) form, else k centroids drawn from the generator at
    state0 -> dict(idx [n] int32 0-based, c [k, m] (NaN rows: empty clusters), sumdist, iters)"""
    X = np.ascontiguousarray(X, np.float64)
    if X.ndim != 2:
        raise ValueError("kmeans_host: X [n, m]")
    n, m = X.shape
    if c0 is not None:
        c0 = np.ascontiguousarray(c0, np.float64).reshape(-1, m)
        k = len(c0)
    if k is None:
        raise ValueError("kmeans_host: k or c0")
    idx, c = np.zeros(n, np.int32), np.zeros((max(int(k), 0), m), np.float64)
    sd, it = C.c_double(), C.c_int()
    rc = lib().pbd_kmeans_host(_vp(X), n, m, int(k), _vp(c0), int(state0) & (2 ** 64 - 1), int(max_iter), _vp(idx), _vp(c), C.byref(sd),
                               C.byref(it))
    if rc != PBD_OK:
        raise PbdError(rc, "pbd_kmeans_host")
    return dict(idx=idx, c=c, sumdist=sd.value, iters=it.value)


def _cluster_parts(fn, name, lead, deffeat, parents, K, R, seed, max_iter):
    deffeat = np.ascontiguousarray(deffeat, np.float64)
    if deffeat.ndim != 3 or deffeat.shape[2] != 2:
        raise ValueError(f"{name}: def [P, n, 2] (Model.data_def)")
    P, n = deffeat.shape[:2]
    parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.int32), (P,)))
    if len(parents) != P:
        raise ValueError(f"{name}: one parent per part")
    R = int(R)
    out = dict(idx=np.zeros((P, n), np.int32), centres=np.zeros((P, PBD_CLUSTER_MAX_K, 2), np.float64), sumdist=np.zeros(P, np.float64),
               best_trial=np.zeros(P, np.int32), trial_sumdist=np.zeros((P, max(R, 0)), np.float64),
               trial_iters=np.zeros((P, max(R, 0)), np.int32))
    capped = C.c_int32()
    rc = fn(*lead, _vp(deffeat), n, P, _vp(parents), _vp(K), R, int(seed) & (2 ** 64 - 1), int(max_iter), _vp(out["idx"]),
            _vp(out["centres"]), _vp(out["sumdist"]), _vp(out["best_trial"]), _vp(out["trial_sumdist"]), _vp(out["trial_iters"]),
            C.byref(capped))
    if rc != PBD_OK:
        raise PbdError(rc, name)
    out["capped"] = capped.value
    return out


def cluster_parts_host(deffeat, parents, K, R=100, seed=0, max_iter=1000):
    """pbd_cluster_parts_host (host code, no GPU): clusterparts.m.  deffeat [P, n, 2] (Model.data_def), parents 0-based with -1 at the
    root, K an int or one per part -> dict(idx [P, n] int32 0-based mixture labels, centres [P, PBD_CLUSTER_MAX_K, 2], sumdist [P],
    best_trial [P], trial_sumdist [P, R], trial_iters [P, R], capped)"""
    return _cluster_parts(lib().pbd_cluster_parts_host, "pbd_cluster_parts_host", (), deffeat, parents, K, R, seed, max_iter)


def cluster_parts(deffeat, parents, K, R=100, seed=0, max_iter=1000, device=0):
    """pbd_cluster_parts: cluster_parts_host on HIP device `device`, one wavefront per (part, trial); bit-identical outputs"""
    return _cluster_parts(lib().pbd_cluster_parts, "pbd_cluster_parts", (int(device),), deffeat, parents, K, R, seed, max_iter)


# ---- virtual positives: map_rotate_points.m and the image operation (include/pbd_c.h "virtual positives") ------------------------------
_ROT_METHODS = {"nearest": PBD_ROT_NEAREST, "bilinear": PBD_ROT_BILINEAR}


def _aug_chk(rc, name):
    if rc != PBD_OK:
        raise PbdError(rc, f"{name}: {lib().pbd_augment_last_error().decode()}")


def rotate_geometry(w, hgt, deg):
    """pbd_rotate_geometry (host code, no GPU): map_rotate_points.m:21-35 for a w x hgt frame turned by deg degrees ->
    dict(w, h: the canvas, m [6] float64 = (cos, sin, hiA_r, hiA_c, hiB_r, hiB_c))"""
    ow, oh, m = C.c_int(), C.c_int(), np.zeros(6, np.float64)
    _aug_chk(lib().pbd_rotate_geometry(int(w), int(hgt), float(deg), C.byref(ow), C.byref(oh), _vp(m)), "pbd_rotate_geometry")
    return dict(w=ow.value, h=oh.value, m=m)


def map_rotate_points(pts, w, hgt, deg, direction=PBD_ROT_ORI2NEW):
    """pbd_map_rotate_points (host code, no GPU): rows (x, y) in the 0-based frame (pixel index k at coordinate k) of a w x hgt frame
    mapped into its canvas at deg degrees (PBD_ROT_ORI2NEW) or back (PBD_ROT_NEW2ORI) -> [n, 2] float64"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    out = np.zeros_like(p)
    _aug_chk(lib().pbd_map_rotate_points(_vp(p), len(p), int(w), int(hgt), float(deg), int(direction), _vp(out)), "pbd_map_rotate_points")
    return out


def flip_points(pts, w, mirror=None):
    """pbd_flip_points (host code, no GPU): out[p] = (w - 1 - x[mirror[p]], y[mirror[p]]) in the 0-based frame; mirror: a permutation
    of the parts (the left / right swap), None: the identity"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    mr = None if mirror is None else np.ascontiguousarray(mirror, np.int32).ravel()
    if mr is not None and len(mr) != len(p):
        raise ValueError("flip_points: one mirror entry per point")
    out = np.zeros_like(p)
    _aug_chk(lib().pbd_flip_points(_vp(p), len(p), int(w), _vp(mr), _vp(out)), "pbd_flip_points")
    return out


def augment_ops(specs):
    """a pbd_augment_op array from specs (flip, deg[, method]): flip a bool, deg the angle in degrees or None for no rotation, method
    "bilinear" (default) / "nearest" or a PBD_ROT_* value.  A pbd_augment_op array passes through."""
    if isinstance(specs, C.Array) and getattr(specs, "_type_", None) is pbd_augment_op:
        return specs
    specs = list(specs)
    ops = (pbd_augment_op * max(len(specs), 1))()
    for i, sp in enumerate(specs):
        if isinstance(sp, pbd_augment_op):
            ops[i] = sp
            continue
        flip, deg = sp[0], sp[1]
        method = sp[2] if len(sp) > 2 else "bilinear"
        ops[i] = pbd_augment_op(int(bool(flip)), int(_ROT_METHODS.get(method, method)), 0.0 if deg is None else float(deg), int(deg is not None), 0)
    ops.count = len(specs)
    return ops


def augment_canvas(w, hgt, op):
    """(rows, cols) of op's output for a w x hgt frame"""
    if not op.rotate:
        return int(hgt), int(w)
    g = rotate_geometry(w, hgt, op.deg)
    return g["h"], g["w"]


def _aug_views(bufs, canvases, cn):
    return [b[:r, :c * cn].reshape((r, c) if cn == 1 else (r, c, cn)) for b, (r, c) in zip(bufs, canvases)]


def _augment_np(fn, name, lead, im, specs, outs):
    im, w, hgt, cn, stride = _frame(im)
    ops = augment_ops(specs)
    n = getattr(ops, "count", len(ops))
    canv = [augment_canvas(w, hgt, ops[i]) for i in range(n)] if 0 < n <= PBD_AUGMENT_MAX_OPS else []
    if outs is None:
        outs = [np.zeros((r, c * cn), np.uint8) for r, c in canv]
    if any(o.dtype != np.uint8 or o.ndim != 2 or not o.flags["C_CONTIGUOUS"] for o in outs):
        raise ValueError(f"{name}: outs are C-contiguous 2-D uint8 arrays [rows, stride]")
    ptrs = (C.c_void_p * max(len(outs), 1))(*[o.ctypes.data for o in outs])
    strides = np.ascontiguousarray([o.shape[1] for o in outs] or [0], np.int32)
    if any(o.shape[0] < r for o, (r, _) in zip(outs, canv)) or (canv and len(outs) != n):
        raise ValueError(f"{name}: one output per op with at least the canvas' rows")
    _aug_chk(fn(*lead, _vp(im), w, hgt, cn, stride, ops, n, ptrs, _vp(strides)), name)
    return _aug_views(outs, canv, cn)


def augment_host(im, specs, outs=None):
    """pbd_augment_host_u8 (host code, no GPU): the virtual copies of the 8-bit frame `im` (HxW or HxWxcn, a strided view is read in
    place), one per spec of augment_ops -> a list of uint8 arrays [rows, cols(, cn)].  outs: the caller's 2-D uint8 buffers
    [rows, stride bytes], written in place (bytes beyond a canvas row stay); the result is then views into them."""
    return _augment_np(lib().pbd_augment_host_u8, "pbd_augment_host_u8", (), im, specs, outs)


def augment(im, specs, device=0, outs=None):
    """pbd_augment_u8: augment_host on HIP device `device` (host in, host out, one launch for all specs); identical bytes"""
    return _augment_np(lib().pbd_augment_u8, "pbd_augment_u8", (int(device),), im, specs, outs)


class DeviceFrame:
    """An 8-bit frame in device memory: hgt rows of w pixels of cn channels, `stride` bytes apart, from device pointer `dptr` on; `owner`
    (a torch tensor, usually) is whatever keeps the allocation alive.  QpCache.write_warped_dev / write_latent_dev,
    PartsBasedDetector.writeWarped / latentPositives and train() take one where they take an array."""

    def __init__(self, dptr, w, hgt, cn, stride=None, owner=None):
        self.dptr, self.w, self.hgt, self.cn = int(dptr), int(w), int(hgt), int(cn)
        self.stride = self.w * self.cn if stride is None else int(stride)
        self.owner = owner

    @classmethod
    def from_tensor(cls, t):
        """a contiguous torch uint8 tensor [hgt, w] or [hgt, w, cn] on a GPU"""
        if str(t.dtype) != "torch.uint8" or not t.is_cuda or not t.is_contiguous() or t.dim() not in (2, 3):
            raise ValueError("DeviceFrame.from_tensor: a contiguous uint8 tensor [hgt, w(, cn)] on a GPU")
        return cls(t.data_ptr(), t.shape[1], t.shape[0], 1 if t.dim() == 2 else t.shape[2], None, t)

    @property
    def shape(self):
        return (self.hgt, self.w) if self.cn == 1 else (self.hgt, self.w, self.cn)

    def crop(self, x, y, w, h):
        """the view of columns x .. x + w - 1 and rows y .. y + h - 1: pointer arithmetic, nothing is copied"""
        if x < 0 or y < 0 or w < 1 or h < 1 or x + w > self.w or y + h > self.hgt:
            raise ValueError("DeviceFrame.crop: outside the frame")
        return DeviceFrame(self.dptr + int(y) * self.stride + int(x) * self.cn, w, h, self.cn, self.stride, self.owner)

    def sync(self):
        """the library reads the frame on streams of its own: whatever the owner's device still has queued is waited for"""
        if hasattr(self.owner, "is_cuda"):
            import torch
            torch.cuda.synchronize(self.owner.device)

    def numpy(self):
        """a host copy [hgt, w(, cn)] (the owner must be a torch tensor)"""
        flat = self.owner.reshape(-1).cpu().numpy()
        off = self.dptr - self.owner.data_ptr()
        v = np.lib.stride_tricks.as_strided(flat[off:], (self.hgt, self.w, self.cn), (self.stride, self.cn, 1))
        return np.ascontiguousarray(v if self.cn > 1 else v[:, :, 0])

    def __repr__(self):
        return f"DeviceFrame({self.w}x{self.hgt}x{self.cn}, stride={self.stride})"


def augment_dev(frame, specs, device=None, outs=None):
    """pbd_augment_dev_u8: the virtual copies of a frame that is in device memory — a DeviceFrame or a torch uint8 tensor
    [hgt, w(, cn)] —, read in place and written into torch uint8 tensors on the same device -> a list of DeviceFrame that own them.
    outs: the caller's 2-D uint8 tensors [rows, stride bytes] instead (bytes beyond a canvas row stay)."""
    import torch
    fr = frame if isinstance(frame, DeviceFrame) else DeviceFrame.from_tensor(frame)
    ops = augment_ops(specs)
    n = getattr(ops, "count", len(ops))
    canv = [augment_canvas(fr.w, fr.hgt, ops[i]) for i in range(n)] if 0 < n <= PBD_AUGMENT_MAX_OPS else []
    dev = fr.owner.device if hasattr(fr.owner, "device") else torch.device("cuda", 0 if device is None else int(device))
    if outs is None:
        outs = [torch.zeros((r, c * fr.cn), dtype=torch.uint8, device=dev) for r, c in canv]
    if any(o.dtype != torch.uint8 or o.dim() != 2 or not o.is_contiguous() or not o.is_cuda for o in outs):
        raise ValueError("augment_dev: outs are contiguous 2-D uint8 tensors [rows, stride] on the GPU")
    if any(o.shape[0] < r for o, (r, _) in zip(outs, canv)) or (canv and len(outs) != n):
        raise ValueError("augment_dev: one output per op with at least the canvas' rows")
    ptrs = (C.c_void_p * max(len(outs), 1))(*[o.data_ptr() for o in outs])
    strides = np.ascontiguousarray([o.shape[1] for o in outs] or [0], np.int32)
    torch.cuda.synchronize(dev)   # (the fills above and whatever produced the source ran on torch's streams)
    _aug_chk(lib().pbd_augment_dev_u8(dev.index or 0, C.c_void_p(fr.dptr), fr.w, fr.hgt, fr.cn, fr.stride, ops, n, ptrs, _vp(strides)),
             "pbd_augment_dev_u8")
    return [DeviceFrame(o.data_ptr(), c, r, fr.cn, o.shape[1], o) for o, (r, c) in zip(outs, canv)]
