"""ctypes binding of the C ABI in include/ebvo_hip.h (libebvo_hip.so, built in-tree by hipcc).

There is no CPU fallback: if the shared library is missing this module raises, and if no HIP
device is usable ``ebvo_ctx_create`` fails and :class:`EbvoError` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EBVO_LIB") or os.path.join(_HERE, "libebvo_hip.so")   # EBVO_LIB: another build of the same ABI (A/B runs)

EDGE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("index", "<i4"), ("pad", "<i4")])
assert EDGE_DTYPE.itemsize == 32

EBVO_OK = 0
EBVO_ERR_ARG = -1
EBVO_ERR_CAPACITY = -2
EBVO_ERR_HIP = -3
EBVO_ERR_NOMEM = -4
EBVO_ERR_STATE = -5

STAGE_EPIPOLAR = 1
STAGE_DISPARITY = 2
STAGE_ORIENTATION = 4
STAGE_ALL = 7

MAX_KERNELS = 32
TOED_STRICT, TOED_HYBRID = 0, 1

# every symbol include/ebvo_hip.h declares (checked by tests/test_abi_symbols.py)
ABI_SYMBOLS = (
    "ebvo_strerror", "ebvo_last_error", "ebvo_abi_version", "ebvo_ctx_create", "ebvo_ctx_destroy",
    "ebvo_set_toed_mode", "ebvo_get_toed_mode", "ebvo_toed_fallbacks", "ebvo_graph_launches", "ebvo_toed_stats", "ebvo_toed_screen_audit", "ebvo_stereo_upload_async", "ebvo_host_register", "ebvo_host_unregister", "ebvo_ingest_stats",
    "ebvo_stereo_fetch_compact_begin", "ebvo_stereo_fetch_compact_end", "ebvo_stereo_pushed_view",
    "ebvo_toed", "ebvo_toed_pair", "ebvo_epipolar_lines", "ebvo_epi_candidates", "ebvo_epi_candidates_staged", "ebvo_ncc_pairs",
    "ebvo_edge_patches", "ebvo_ncc_patches", "ebvo_ncc_quads", "ebvo_stereo_default_params", "ebvo_finalize_default_params",
    "ebvo_stereo_upload", "ebvo_stereo_run", "ebvo_stereo_fetch", "ebvo_stereo_set_slots",
    "ebvo_stereo_upload_slot", "ebvo_stereo_submit", "ebvo_stereo_wait", "ebvo_stereo_fetch_slot", "ebvo_profile_enable",
    "ebvo_profile_reset", "ebvo_profile_get", "ebvo_fp64_peak",
    "ebvo_gn_default_params", "ebvo_sobel_gradients", "ebvo_gn_refine_stereo", "ebvo_stereo_refine",
    "ebvo_stereo_fetch_refined", "ebvo_gn_refine_temporal", "ebvo_finalize_pairs", "ebvo_bnb_test", "ebvo_keep_best", "ebvo_epipolar_shift", "ebvo_cluster_rows", "ebvo_stereo_finalize", "ebvo_stereo_finalize_submit", "ebvo_stereo_finalize_wait", "ebvo_stereo_fetch_final",
    "ebvo_debug_set", "ebvo_stereo_fetch_begin", "ebvo_stereo_fetch_end",
    "ebvo_undistort", "ebvo_stereo_set_undistort", "ebvo_sift_descriptors", "ebvo_sift_min_distances",
    "ebvo_toed_resident", "ebvo_epi_candidates_resident", "ebvo_ncc_pairs_resident",
    "ebvo_temporal_default_params", "ebvo_temporal_set_keyframe", "ebvo_temporal_match", "ebvo_temporal_match_submit", "ebvo_temporal_match_wait", "ebvo_temporal_fetch", "ebvo_temporal_fetch_final",
    "ebvo_pose_default_params", "ebvo_temporal_estimate_pose", "ebvo_pose_from_quads", "ebvo_temporal_final_size",
    "ebvo_gt_default_params", "ebvo_stereo_set_gt", "ebvo_stereo_gt_size", "ebvo_stereo_gt_fetch", "ebvo_stereo_gt_metrics",
    "ebvo_stereo_gt_stage_rows", "ebvo_gt_locate", "ebvo_gt_evaluate_rows",
    "ebvo_tgt_default_params", "ebvo_temporal_set_gt", "ebvo_temporal_gt_size", "ebvo_temporal_gt_fetch", "ebvo_temporal_gt_metrics",
    "ebvo_temporal_gt_flags", "ebvo_tgt_veridical", "ebvo_tgt_evaluate_rows",
    "ebvo_temporal_keep_stages", "ebvo_temporal_stage_size", "ebvo_temporal_fetch_stage", "ebvo_temporal_gt_stage_rows",
    "ebvo_tgt_grid_rows",
    "ebvo_tprior_default_params", "ebvo_temporal_set_prior", "ebvo_temporal_clear_prior", "ebvo_temporal_prior_fetch",
    "ebvo_tprior_candidates",
    "ebvo_pose_from_quads_gt", "ebvo_temporal_estimate_pose_gt", "ebvo_pose_constraint_metrics",
    "ebvo_temporal_pose_constraint_metrics",
    "ebvo_pose_refine_default_params", "ebvo_pose_refine_from_quads", "ebvo_temporal_refine_pose",
    "ebvo_align_default_params", "ebvo_pose_align_edges", "ebvo_temporal_align_pose", "ebvo_temporal_align_size",
    "ebvo_depth_default_params", "ebvo_depth_refine_edges", "ebvo_temporal_refine_depth", "ebvo_temporal_depth_fetch",
    "ebvo_temporal_depth_reset", "ebvo_temporal_use_depth", "ebvo_pose_align_edges_depth",
    "ebvo_depth_carry_default_params", "ebvo_depth_carry", "ebvo_temporal_promote_keyframe", "ebvo_temporal_depth_source",
    "ebvo_cover_default_params", "ebvo_keyframe_cover_edges", "ebvo_temporal_keyframe_cover", "ebvo_temporal_cover_size",
    "ebvo_keyframe_policy_default",
    "ebvo_keyframe_decide", "ebvo_temporal_keyframe_pose", "ebvo_track_default_params", "ebvo_temporal_track_frame",
)


class StereoParams(C.Structure):
    _fields_ = [("F21", C.c_double * 9), ("epi_thr", C.c_double), ("max_disp", C.c_double),
                ("orient_thr_deg", C.c_double), ("ncc_thr", C.c_double), ("stage_mask", C.c_int),
                ("reserved", C.c_int)]


PAIR_PACK = 8                         # ... into device staging: the compact fetch is one copy
PAIR_PUSH, PAIR_PUSH_THETA = 2, 4   # ... the chain ends by writing the compact results into page-locked host memory
PAIR_NO_SIMS = 1     # StereoParams.reserved: the resident pipeline stores best + keep only (ebvo_hip.h EBVO_PAIR_NO_SIMS)


class StereoCalib(C.Structure):
    _fields_ = [("K_left", C.c_double * 9), ("K_right", C.c_double * 9), ("R21", C.c_double * 9), ("T21", C.c_double * 3)]


class GnParams(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("tol", C.c_double), ("huber_delta", C.c_double)]


class FinalizeParams(C.Structure):
    _fields_ = [("bnb_ratio", C.c_double), ("ncc_thr", C.c_double), ("gn", GnParams), ("use_sift", C.c_int),
                ("reserved", C.c_int), ("sift_thr", C.c_double), ("bnb_sift", C.c_double)]


class FinalizeCounts(C.Structure):
    _fields_ = [("n_ncc", C.c_int32), ("n_bnb", C.c_int32), ("n_clusters", C.c_int32), ("n_ncc2", C.c_int32),
                ("n_final", C.c_int32), ("n_sift", C.c_int32)]


class StereoCounts(C.Structure):
    _fields_ = [("n_left", C.c_int32), ("n_right", C.c_int32), ("n_total_left", C.c_int32),
                ("n_total_right", C.c_int32), ("n_pairs", C.c_int64), ("n_matches", C.c_int64)]


class UndistortParams(C.Structure):
    _fields_ = [("K_left", C.c_double * 4), ("K_right", C.c_double * 4), ("dist_left", C.c_double * 5),
                ("dist_right", C.c_double * 5), ("n_dist", C.c_int), ("reserved", C.c_int)]


class TemporalParams(C.Structure):
    _fields_ = [("cell_size", C.c_int), ("stages", C.c_int), ("grid_radius", C.c_double), ("orient_thr_deg", C.c_double),
                ("ncc_thr", C.c_double), ("sift_thr", C.c_double), ("bnb_ncc", C.c_double), ("bnb_sift", C.c_double),
                ("gn", GnParams)]


class TemporalCounts(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_cf", C.c_int32), ("n_candidates", C.c_int64), ("n_kept", C.c_int64),
                ("n_sift", C.c_int64), ("n_bnb_ncc", C.c_int64), ("n_bnb_sift", C.c_int64), ("n_refined_valid", C.c_int64),
                ("n_final", C.c_int64)]


class PoseParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("min_iterations", C.c_int32), ("dyn_num_trials_mult", C.c_double),
                ("success_prob", C.c_double), ("max_reproj_error", C.c_double), ("top_rank_fraction", C.c_double),
                ("tau_length", C.c_double), ("tau_t1", C.c_double), ("tau_t2", C.c_double), ("tau_tangent", C.c_double),
                ("rand_seed", C.c_uint32), ("continue_stream", C.c_int32), ("max_draws", C.c_int64)]


class PoseResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("status", C.c_int32), ("found", C.c_int32),
                ("n_quads", C.c_int64), ("top_n", C.c_int64), ("iterations", C.c_int64), ("draws", C.c_int64),
                ("hypotheses", C.c_int64), ("best_inliers", C.c_int64), ("dynamic_max_iter", C.c_int64),
                ("inlier_ratio", C.c_double), ("best_q1", C.c_int32), ("best_q2", C.c_int32)]


POSE_OK, POSE_INSUFFICIENT, POSE_DRAW_CAP = 0, 1, 2


class PoseRefineParams(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32), ("huber_px", C.c_double), ("step_eps", C.c_double),
                ("block_threads", C.c_int32), ("reserved", C.c_int32)]


class PoseRefined(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("status", C.c_int32), ("stop_reason", C.c_int32),
                ("rounds_run", C.c_int32), ("steps_kept", C.c_int32), ("n_quads", C.c_int64), ("fit_quads", C.c_int64),
                ("inliers", C.c_int64), ("cost_first", C.c_double), ("cost_last", C.c_double)]


REFINE_OK, REFINE_NOTHING, REFINE_PIVOT = 0, 1, 2


class AlignParams(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32), ("radius", C.c_double), ("cell_size", C.c_int32),
                ("min_terms", C.c_int32), ("orient_thr_deg", C.c_double), ("huber_px", C.c_double), ("inlier_px", C.c_double),
                ("step_eps", C.c_double), ("img_margin", C.c_double), ("cameras", C.c_int32), ("block_threads", C.c_int32)]


class AlignedPose(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("status", C.c_int32), ("stop_reason", C.c_int32),
                ("rounds_run", C.c_int32), ("steps_kept", C.c_int32), ("n_kf", C.c_int32), ("fit_terms", C.c_int32),
                ("n_assoc", C.c_int32 * 2), ("inliers", C.c_int64), ("cost_first", C.c_double), ("cost_last", C.c_double),
                ("rms_normal", C.c_double)]


class DepthParams(C.Structure):
    _fields_ = [("sigma_disp_px", C.c_double), ("sigma_normal_px", C.c_double), ("huber_px", C.c_double), ("gate_px", C.c_double),
                ("iterations", C.c_int32), ("cameras", C.c_int32), ("lambda_min", C.c_double), ("lambda_max", C.c_double),
                ("info_max", C.c_double), ("img_margin", C.c_double), ("block_threads", C.c_int32), ("reserved", C.c_int32)]


class DepthCarryParams(C.Structure):
    _fields_ = [("sigma_disp_px", C.c_double), ("radius", C.c_double), ("cell_size", C.c_int32), ("min_obs", C.c_int32),
                ("orient_thr_deg", C.c_double), ("carry", C.c_double), ("gate_sigmas", C.c_double), ("lambda_min", C.c_double),
                ("lambda_max", C.c_double), ("info_max", C.c_double), ("img_margin", C.c_double), ("reserved", C.c_int32),
                ("pad", C.c_int32)]


class DepthCarried(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_old", "n_sources", "n_live", "n_new", "n_dead", "n_assoc", "n_carried", "n_gated")]


class DepthRefined(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_dead", C.c_int32), ("n_updated", C.c_int32), ("n_restored", C.c_int32),
                ("n_terms", C.c_int32 * 2), ("n_gated", C.c_int32 * 2), ("rms_before", C.c_double), ("rms_after", C.c_double)]


COVER_BINS = 64
COVER_DEAD, COVER_IN_FRAME, COVER_ASSOCIATED, COVER_INLIER = 1, 2, 4, 8                          # flags of ebvo_keyframe_cover_edges
KF_LOST, KF_LOW_OVERLAP, KF_LOW_ASSOC, KF_NEW_CONTENT, KF_PARALLAX = 1, 2, 4, 8, 16              # reasons of ebvo_keyframe_decide
(TRACK_STAGE_NONE, TRACK_STAGE_ALIGN, TRACK_STAGE_DEPTH, TRACK_STAGE_COVER, TRACK_STAGE_FINALIZE, TRACK_STAGE_PROMOTE) = range(6)


class CoverParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("orient_thr_deg", C.c_double), ("img_margin", C.c_double), ("inlier_px", C.c_double),
                ("bin_px", C.c_double), ("cell_size", C.c_int32), ("cover_cell", C.c_int32), ("min_cell_edges", C.c_int32),
                ("min_cell_explained", C.c_int32), ("reserved", C.c_int32), ("pad", C.c_int32)]


class KeyframeCover(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_kf", "n_dead", "n_in_frame", "n_assoc", "n_inliers", "n_edges", "n_explained", "cw", "ch",
                                         "n_cells_cur", "n_cells_covered", "disp_median_bin")] + [("hist", C.c_int32 * COVER_BINS)]


class KeyframePolicy(C.Structure):
    _fields_ = [("min_assoc", C.c_int32), ("max_disp_bins", C.c_int32), ("min_in_frame_share", C.c_double),
                ("min_assoc_share", C.c_double), ("min_cell_cover", C.c_double)]


class TrackParams(C.Structure):
    _fields_ = [("align", AlignParams), ("depth", DepthParams), ("cover", CoverParams), ("carry", DepthCarryParams),
                ("finalize", FinalizeParams), ("policy", KeyframePolicy), ("refine_depth", C.c_int32), ("reserved", C.c_int32)]


class TrackedFrame(C.Structure):
    _fields_ = [("pose", AlignedPose), ("depth", DepthRefined), ("cover", KeyframeCover), ("carried", DepthCarried),
                ("finalized", FinalizeCounts), ("R_seq", C.c_double * 9), ("t_seq", C.c_double * 3), ("reasons", C.c_uint32),
                ("decision", C.c_int32), ("switched", C.c_int32), ("tracked", C.c_int32), ("failed_stage", C.c_int32),
                ("pad", C.c_int32)]


DEPTH_DEAD, DEPTH_UPDATED, DEPTH_RESTORED, DEPTH_GATED_LEFT, DEPTH_GATED_RIGHT = 1, 2, 4, 8, 16   # flags of one update

ALIGN_OK, ALIGN_NOTHING, ALIGN_PIVOT = 0, 1, 2   # the stop reasons are the refit's, 4 = fewer than min_terms associated terms
(REFINE_STOP_EPS, REFINE_STOP_CAP, REFINE_STOP_COST, REFINE_STOP_PIVOT, REFINE_STOP_FEW) = range(5)

# stage ids (ebvo_hip.h EBVO_PC_*) and the names of Solution_Constraints_Application (src/MotionTracker.cpp:299-378)
PC_STAGE_NAMES = ("Baseline", "Normalized Length Constraint", "T1 Angle Similarity Constraint", "T2 Angle Similarity Constraint",
                  "Tangent Angle Similarity Constraint")
(PC_BASELINE, PC_LENGTH, PC_T1, PC_T2, PC_TANGENT) = range(5)
PC_NUM_STAGES = 5
PC_MAX_DRAWS = 1 << 24   # n_runs x max_iterations of one call


class PoseCascadeStage(C.Structure):
    _fields_ = [("stage", C.c_int32), ("reserved", C.c_int32), ("surviving", C.c_int64), ("veridical", C.c_int64),
                ("recall", C.c_double), ("precision", C.c_double)]


class PoseCascadeRun(C.Structure):
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("n_quads", C.c_int64), ("top_n", C.c_int64),
                ("draws", C.c_int64), ("stages", PoseCascadeStage * PC_NUM_STAGES)]


class GtParams(C.Structure):
    _fields_ = [("orient_gate_deg", C.c_double), ("pool_epi_thr", C.c_double), ("pool_dist", C.c_double),
                ("pool_orient_deg", C.c_double), ("tp_dist", C.c_double)]


class GtStage(C.Structure):
    _fields_ = [("stage", C.c_int32), ("present", C.c_int32), ("rows", C.c_int64), ("nonempty", C.c_int64),
                ("rows_with_tp", C.c_int64), ("sum_tp", C.c_int64), ("sum_n", C.c_int64), ("recall", C.c_double),
                ("precision", C.c_double), ("precision_pair", C.c_double), ("ambiguity", C.c_double)]


# stage ids (ebvo_hip.h EBVO_GT_*) and the names the reference gives them in Frame_Evaluation_Metrics
# (src/Stereo_Matches.cpp:1382-1535; "NCC" appears twice there)
GT_STAGE_NAMES = ("Epipolar Proximity", "Location Proximity", "Orientation", "SIFT", "NCC", "BNB-NCC", "BNB-SIFT",
                  "Photometric Refinement", "Edge Clustering", "NCC", "Best", "Final")
(GT_EPIPOLAR, GT_DISPARITY, GT_ORIENTATION, GT_SIFT, GT_NCC, GT_BNB_NCC, GT_BNB_SIFT, GT_REFINE, GT_CLUSTER, GT_NCC2, GT_BEST,
 GT_FINAL) = range(12)
GT_NUM_STAGES = 12


class TgtParams(C.Structure):
    _fields_ = [("orient_thr_deg", C.c_double), ("tp_dist", C.c_double), ("search_radius", C.c_double), ("img_margin", C.c_double)]


class TpriorParams(C.Structure):
    _fields_ = [("img_margin", C.c_double), ("use_orientation", C.c_int32)]


# stage ids (ebvo_hip.h EBVO_TGT_*) and the names of src/Temporal_Matches.cpp:186-215
TGT_STAGE_NAMES = ("Location Proximity", "Orientation", "NCC", "SIFT", "BNB-NCC", "BNB-SIFT", "Photometric Refinement",
                   "Edge Clustering")
(TGT_GRID, TGT_ORIENTATION, TGT_NCC, TGT_SIFT, TGT_BNB_NCC, TGT_BNB_SIFT, TGT_REFINE, TGT_CLUSTER) = range(8)
TGT_NUM_STAGES = 8


class StereoView(C.Structure):
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p),
                ("sims", C.c_void_p), ("best", C.c_void_p), ("keep", C.c_void_p), ("n_left", C.c_int32),
                ("n_right", C.c_int32), ("n_pairs", C.c_int64)]


class ToedView(C.Structure):
    _fields_ = [("edges", C.c_void_p), ("all4", C.c_void_p), ("n_kept", C.c_int32), ("n_total", C.c_int32),
                ("tag", C.c_uint64), ("t_conv", C.c_double), ("t_nms", C.c_double)]


class CandidatesView(C.Structure):
    _fields_ = [("row_ptr", C.c_void_p), ("col_idx", C.c_void_p), ("orient_ok", C.c_void_p), ("n_pairs", C.c_int64),
                ("row_ptr_final", C.c_void_p), ("col_idx_final", C.c_void_p), ("n_final", C.c_int64)]


class NccView(C.Structure):
    _fields_ = [("left_patches", C.c_void_p), ("sims", C.c_void_p), ("best", C.c_void_p), ("keep", C.c_void_p),
                ("n_left", C.c_int32), ("n_pairs", C.c_int64)]


NCC_WANT_LEFT_PATCHES, NCC_WANT_SIMS = 1, 2

FETCH_EDGES, FETCH_CSR, FETCH_BEST, FETCH_KEEP, FETCH_SIMS, FETCH_DEFAULT, FETCH_ALL = 1, 2, 4, 8, 16, 15, 31


class CompactView(C.Structure):
    _fields_ = [("left_xy", C.c_void_p), ("right_xy", C.c_void_p), ("left_theta", C.c_void_p), ("right_theta", C.c_void_p),
                ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p), ("best", C.c_void_p), ("keep_bits", C.c_void_p),
                ("n_left", C.c_int32), ("n_right", C.c_int32), ("n_pairs", C.c_int64), ("n_matches", C.c_int64)]


COMPACT_XY, COMPACT_THETA, COMPACT_CSR, COMPACT_BEST, COMPACT_KEEP_BITS, COMPACT_DEFAULT, COMPACT_ALL = 1, 2, 4, 8, 16, 29, 31


class ScreenAudit(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("n_maxima", C.c_int32), ("n_kept", C.c_int32), ("n_neighbour_points", C.c_int32),
                ("max_err_gx", C.c_double), ("max_err_gy", C.c_double), ("max_err_mag", C.c_double),
                ("max_err_mag_neighbours", C.c_double), ("bound_g", C.c_double), ("bound_mag", C.c_double),
                ("bound_slope", C.c_double), ("tol_mag", C.c_double), ("tol_slope", C.c_double)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("launches", C.c_int64)]


class EbvoError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status}" + (f" ({detail})" if detail else ""))


_lib = None


def load_library() -> C.CDLL:
    """dlopen libebvo_hip.so (raises if it was not built) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with __graft_entry__.build() or "
            "`make -C edge_based_visual_odometry_amd/csrc` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    ssz = C.c_ssize_t
    lib.ebvo_strerror.restype = C.c_char_p
    lib.ebvo_strerror.argtypes = [i32]
    lib.ebvo_last_error.restype = C.c_char_p
    lib.ebvo_last_error.argtypes = [vp]
    lib.ebvo_abi_version.restype = i32
    lib.ebvo_ctx_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    lib.ebvo_ctx_destroy.restype = None
    lib.ebvo_ctx_destroy.argtypes = [vp]
    lib.ebvo_set_toed_mode.argtypes = [vp, i32]
    lib.ebvo_get_toed_mode.argtypes = [vp]
    lib.ebvo_toed_fallbacks.argtypes = [vp]
    lib.ebvo_toed_fallbacks.restype = i64
    lib.ebvo_graph_launches.argtypes = [vp]
    lib.ebvo_graph_launches.restype = i64
    lib.ebvo_toed_stats.argtypes = [vp, i32, vp]
    lib.ebvo_toed_screen_audit.argtypes = [vp, vp, i32, i32, ssz, C.POINTER(ScreenAudit)]
    lib.ebvo_toed.argtypes = [vp, vp, i32, i32, ssz, vp, i32, C.POINTER(i32), C.POINTER(i32), vp, i32,
                              C.POINTER(dbl), C.POINTER(dbl)]
    lib.ebvo_toed_pair.argtypes = [vp, vp, vp, i32, i32, ssz, ssz, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.ebvo_epipolar_lines.argtypes = [vp, vp, i32, vp]
    lib.ebvo_epi_candidates.argtypes = [vp, vp, i32, vp, i32, vp, dbl, dbl, dbl, i32, vp, vp, i64,
                                        C.POINTER(i64)]
    lib.ebvo_epi_candidates_staged.restype = i32
    lib.ebvo_epi_candidates_staged.argtypes = [vp, vp, i32, vp, i32, vp, dbl, dbl, dbl, vp, vp, vp, i64, C.POINTER(i64)]
    lib.ebvo_ncc_pairs.argtypes = [vp, vp, vp, i32, i32, ssz, ssz, vp, i32, vp, vp, dbl, vp, vp, vp, vp]
    lib.ebvo_edge_patches.argtypes = [vp, vp, i32, i32, ssz, vp, i32, vp]
    lib.ebvo_ncc_patches.argtypes = [vp, vp, vp, i32, vp]
    lib.ebvo_ncc_quads.argtypes = [vp, vp, vp, vp, vp, i32, dbl, vp, vp, vp]
    lib.ebvo_stereo_default_params.restype = None
    lib.ebvo_finalize_default_params.restype = None
    lib.ebvo_finalize_default_params.argtypes = [C.c_void_p]
    lib.ebvo_stereo_default_params.argtypes = [C.POINTER(StereoParams)]
    lib.ebvo_stereo_upload.argtypes = [vp, vp, vp, i32, i32, ssz, ssz]
    lib.ebvo_toed_resident.argtypes = [vp, i32, vp, i32, i32, ssz, i32, C.POINTER(ToedView)]
    lib.ebvo_epi_candidates_resident.argtypes = [vp, C.c_uint64, C.c_uint64, vp, dbl, dbl, dbl, i32, i32, C.POINTER(CandidatesView)]
    lib.ebvo_ncc_pairs_resident.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, i32, i32, ssz, ssz, vp, vp, dbl, i32,
                                            C.POINTER(NccView)]
    lib.ebvo_stereo_run.argtypes = [vp, C.POINTER(StereoParams), C.POINTER(StereoCounts)]
    lib.ebvo_stereo_fetch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ebvo_stereo_set_slots.argtypes = [vp, i32]
    lib.ebvo_stereo_upload_slot.argtypes = [vp, i32, vp, vp, i32, i32, ssz, ssz]
    lib.ebvo_stereo_submit.argtypes = [vp, i32, C.POINTER(StereoParams)]
    lib.ebvo_stereo_upload_async.argtypes = [vp, i32, vp, vp, i32, i32, ssz, ssz]
    lib.ebvo_host_register.argtypes = [vp, vp, C.c_size_t]
    lib.ebvo_host_unregister.argtypes = [vp, vp]
    lib.ebvo_ingest_stats.argtypes = [vp, vp]
    lib.ebvo_stereo_fetch_compact_begin.argtypes = [vp, i32, i32]
    lib.ebvo_stereo_fetch_compact_end.argtypes = [vp, i32, C.POINTER(CompactView)]
    lib.ebvo_stereo_pushed_view.argtypes = [vp, i32, C.POINTER(CompactView)]
    lib.ebvo_stereo_wait.argtypes = [vp, i32, C.POINTER(StereoCounts)]
    lib.ebvo_stereo_fetch_slot.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ebvo_profile_enable.argtypes = [vp, i32]
    lib.ebvo_profile_reset.argtypes = [vp]
    lib.ebvo_profile_get.argtypes = [vp, C.POINTER(KernelTime), C.POINTER(i32)]
    lib.ebvo_fp64_peak.argtypes = [vp, i32, C.POINTER(dbl), C.POINTER(dbl)]
    lib.ebvo_debug_set.argtypes = [vp, i32, i32]
    lib.ebvo_stereo_fetch_begin.argtypes = [vp, i32, i32]
    lib.ebvo_sift_descriptors.argtypes = [vp, vp, i32, i32, ssz, vp, i32, vp]
    lib.ebvo_sift_min_distances.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.ebvo_temporal_default_params.restype = None
    lib.ebvo_temporal_default_params.argtypes = [C.POINTER(TemporalParams)]
    lib.ebvo_temporal_set_keyframe.argtypes = [vp, i32]
    lib.ebvo_temporal_match.argtypes = [vp, i32, C.POINTER(TemporalParams), C.POINTER(TemporalCounts)]
    lib.ebvo_temporal_match_submit.argtypes = [vp, i32, C.POINTER(TemporalParams)]
    lib.ebvo_temporal_match_wait.argtypes = [vp, i32, C.POINTER(TemporalCounts)]
    lib.ebvo_temporal_fetch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.ebvo_temporal_fetch_final.restype = i32
    lib.ebvo_temporal_fetch_final.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ebvo_pose_default_params.restype = None
    lib.ebvo_pose_default_params.argtypes = [C.POINTER(PoseParams)]
    lib.ebvo_temporal_estimate_pose.restype = i32
    lib.ebvo_temporal_estimate_pose.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(PoseParams), C.POINTER(PoseResult), vp]
    lib.ebvo_temporal_final_size.restype = i32
    lib.ebvo_temporal_final_size.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(i64)]
    lib.ebvo_pose_from_quads.restype = i32
    lib.ebvo_pose_from_quads.argtypes = [vp, vp, vp, i32, vp, vp, vp, C.POINTER(StereoCalib), C.POINTER(PoseParams),
                                         C.POINTER(PoseResult), vp, vp, vp]
    lib.ebvo_pose_from_quads_gt.restype = i32
    lib.ebvo_pose_from_quads_gt.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, C.POINTER(StereoCalib), C.POINTER(PoseParams),
                                            C.POINTER(PoseResult), vp, vp, vp]
    lib.ebvo_temporal_estimate_pose_gt.restype = i32
    lib.ebvo_temporal_estimate_pose_gt.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(PoseParams), C.POINTER(PoseResult), vp]
    lib.ebvo_pose_constraint_metrics.restype = i32
    lib.ebvo_pose_constraint_metrics.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, C.POINTER(StereoCalib),
                                                 C.POINTER(PoseParams), i32, C.POINTER(PoseCascadeRun), vp, vp]
    lib.ebvo_temporal_pose_constraint_metrics.restype = i32
    lib.ebvo_temporal_pose_constraint_metrics.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(PoseParams), i32,
                                                          C.POINTER(PoseCascadeRun), vp, vp]
    lib.ebvo_pose_refine_default_params.restype = None
    lib.ebvo_pose_refine_default_params.argtypes = [C.POINTER(PoseRefineParams)]
    lib.ebvo_pose_refine_from_quads.restype = i32
    lib.ebvo_pose_refine_from_quads.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, C.POINTER(StereoCalib), C.POINTER(PoseParams),
                                                C.POINTER(PoseRefineParams), vp, vp, C.POINTER(PoseRefined), vp]
    lib.ebvo_temporal_refine_pose.restype = i32
    lib.ebvo_temporal_refine_pose.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(PoseParams), C.POINTER(PoseRefineParams),
                                              vp, vp, i32, C.POINTER(PoseRefined), vp]
    lib.ebvo_align_default_params.restype = None
    lib.ebvo_align_default_params.argtypes = [C.POINTER(AlignParams)]
    lib.ebvo_pose_align_edges.restype = i32
    lib.ebvo_pose_align_edges.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, C.POINTER(StereoCalib), C.POINTER(AlignParams),
                                          vp, vp, C.POINTER(AlignedPose), vp, vp]
    lib.ebvo_temporal_align_pose.restype = i32
    lib.ebvo_temporal_align_pose.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(AlignParams), vp, vp, C.POINTER(AlignedPose),
                                             vp, vp]
    lib.ebvo_temporal_align_size.restype = i32
    lib.ebvo_temporal_align_size.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ebvo_depth_default_params.restype = None
    lib.ebvo_depth_default_params.argtypes = [C.POINTER(DepthParams)]
    lib.ebvo_depth_refine_edges.restype = i32
    lib.ebvo_depth_refine_edges.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, C.POINTER(StereoCalib),
                                            C.POINTER(DepthParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(DepthRefined)]
    lib.ebvo_temporal_refine_depth.restype = i32
    lib.ebvo_temporal_refine_depth.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(AlignParams), C.POINTER(DepthParams), vp, vp,
                                               C.POINTER(DepthRefined)]
    lib.ebvo_temporal_depth_fetch.restype = i32
    lib.ebvo_temporal_depth_fetch.argtypes = [vp, vp, vp, vp, vp]
    lib.ebvo_temporal_depth_reset.restype = i32
    lib.ebvo_temporal_depth_reset.argtypes = [vp]
    lib.ebvo_temporal_use_depth.restype = i32
    lib.ebvo_temporal_use_depth.argtypes = [vp, i32]
    lib.ebvo_pose_align_edges_depth.restype = i32
    lib.ebvo_pose_align_edges_depth.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, C.POINTER(StereoCalib),
                                                C.POINTER(AlignParams), vp, vp, C.POINTER(AlignedPose), vp, vp]
    lib.ebvo_depth_carry_default_params.restype = None
    lib.ebvo_depth_carry_default_params.argtypes = [C.POINTER(DepthCarryParams)]
    lib.ebvo_depth_carry.restype = i32
    lib.ebvo_depth_carry.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StereoCalib),
                                     C.POINTER(DepthCarryParams), vp, vp, vp, vp, vp, vp, vp, C.POINTER(DepthCarried)]
    lib.ebvo_temporal_promote_keyframe.restype = i32
    lib.ebvo_temporal_promote_keyframe.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(DepthCarryParams), vp, vp,
                                                   C.POINTER(DepthCarried)]
    lib.ebvo_temporal_depth_source.restype = i32
    lib.ebvo_temporal_depth_source.argtypes = [vp, vp]
    lib.ebvo_cover_default_params.restype = None
    lib.ebvo_cover_default_params.argtypes = [C.POINTER(CoverParams)]
    lib.ebvo_keyframe_cover_edges.restype = i32
    lib.ebvo_keyframe_cover_edges.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, C.POINTER(StereoCalib), C.POINTER(CoverParams), vp, vp,
                                              C.POINTER(KeyframeCover), vp, vp, vp, vp, vp, vp]
    lib.ebvo_temporal_keyframe_cover.restype = i32
    lib.ebvo_temporal_keyframe_cover.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(CoverParams), vp, vp, C.POINTER(KeyframeCover),
                                                 vp, vp, vp, vp, vp, vp]
    lib.ebvo_temporal_cover_size.restype = i32
    lib.ebvo_temporal_cover_size.argtypes = [vp, i32, C.POINTER(CoverParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ebvo_keyframe_policy_default.restype = None
    lib.ebvo_keyframe_policy_default.argtypes = [C.POINTER(KeyframePolicy)]
    lib.ebvo_keyframe_decide.restype = i32
    lib.ebvo_keyframe_decide.argtypes = [C.POINTER(KeyframeCover), C.POINTER(KeyframePolicy), C.POINTER(C.c_uint32)]
    lib.ebvo_temporal_keyframe_pose.restype = i32
    lib.ebvo_temporal_keyframe_pose.argtypes = [vp, vp, vp]
    lib.ebvo_track_default_params.restype = None
    lib.ebvo_track_default_params.argtypes = [C.POINTER(TrackParams)]
    lib.ebvo_temporal_track_frame.restype = i32
    lib.ebvo_temporal_track_frame.argtypes = [vp, i32, C.POINTER(StereoCalib), C.POINTER(TrackParams), vp, vp, C.POINTER(TrackedFrame)]
    lib.ebvo_gt_default_params.restype = None
    lib.ebvo_gt_default_params.argtypes = [C.POINTER(GtParams)]
    lib.ebvo_stereo_set_gt.argtypes = [vp, i32, vp, i32, i32, ssz, C.POINTER(StereoCalib), C.POINTER(GtParams)]
    lib.ebvo_stereo_gt_size.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(i64)]
    lib.ebvo_stereo_gt_fetch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.ebvo_stereo_gt_metrics.argtypes = [vp, i32, C.POINTER(GtStage)]
    lib.ebvo_stereo_gt_stage_rows.argtypes = [vp, i32, i32, vp, i32]
    lib.ebvo_gt_locate.argtypes = [vp, vp, i32, vp, i32, i32, ssz, C.POINTER(StereoCalib), C.POINTER(GtParams), vp, vp, vp, vp]
    lib.ebvo_gt_evaluate_rows.argtypes = [vp, vp, vp, i32, vp, vp, dbl, vp, C.POINTER(GtStage)]
    lib.ebvo_tgt_default_params.restype = None
    lib.ebvo_tgt_default_params.argtypes = [C.POINTER(TgtParams)]
    lib.ebvo_temporal_set_gt.argtypes = [vp, i32, vp, vp, C.POINTER(StereoCalib), C.POINTER(TgtParams), vp, vp]
    lib.ebvo_temporal_gt_size.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(i64)]
    lib.ebvo_temporal_gt_fetch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ebvo_temporal_gt_metrics.argtypes = [vp, i32, C.POINTER(GtStage)]
    lib.ebvo_temporal_gt_flags.argtypes = [vp, i32, i32, vp]
    lib.ebvo_tgt_veridical.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, C.POINTER(StereoCalib),
                                       C.POINTER(TgtParams), vp, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]
    lib.ebvo_tgt_evaluate_rows.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, dbl, vp, vp, C.POINTER(GtStage)]
    lib.ebvo_temporal_keep_stages.argtypes = [vp, i32, i32]
    lib.ebvo_temporal_stage_size.argtypes = [vp, i32, i32, C.POINTER(i64)]
    lib.ebvo_temporal_fetch_stage.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.ebvo_temporal_gt_stage_rows.argtypes = [vp, i32, i32, vp, i32]
    lib.ebvo_tgt_grid_rows.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, dbl, vp, vp, vp, dbl, vp, C.POINTER(GtStage)]
    lib.ebvo_tprior_default_params.restype = None
    lib.ebvo_tprior_default_params.argtypes = [C.POINTER(TpriorParams)]
    lib.ebvo_temporal_set_prior.argtypes = [vp, i32, vp, vp, C.POINTER(StereoCalib), C.POINTER(TpriorParams)]
    lib.ebvo_temporal_clear_prior.argtypes = [vp, i32]
    lib.ebvo_temporal_prior_fetch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.ebvo_tprior_candidates.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, dbl, dbl, vp, vp, C.POINTER(StereoCalib),
                                           C.POINTER(TpriorParams), vp, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]
    lib.ebvo_undistort.argtypes = [vp, vp, i32, i32, ssz, vp, vp, i32, vp, ssz]
    lib.ebvo_stereo_set_undistort.argtypes = [vp, C.POINTER(UndistortParams)]
    lib.ebvo_stereo_fetch_end.argtypes = [vp, i32, C.POINTER(StereoView)]
    lib.ebvo_gn_default_params.restype = None
    lib.ebvo_gn_default_params.argtypes = [C.POINTER(GnParams)]
    lib.ebvo_sobel_gradients.argtypes = [vp, vp, i32, i32, ssz, vp, vp]
    lib.ebvo_gn_refine_temporal.argtypes = [vp, vp, vp, i32, i32, ssz, ssz, vp, vp, vp, i32, C.POINTER(GnParams), vp, vp, vp,
                                            vp]
    lib.ebvo_bnb_test.argtypes = [vp, vp, i32, vp, dbl, i32, vp, vp]
    lib.ebvo_keep_best.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.ebvo_epipolar_shift.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.ebvo_cluster_rows.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.ebvo_stereo_finalize.argtypes = [vp, i32, C.POINTER(FinalizeParams), C.POINTER(StereoCalib), C.POINTER(FinalizeCounts)]
    lib.ebvo_stereo_finalize_submit.argtypes = [vp, i32, C.POINTER(FinalizeParams), C.POINTER(StereoCalib)]
    lib.ebvo_stereo_finalize_wait.argtypes = [vp, i32, C.POINTER(FinalizeCounts)]
    lib.ebvo_stereo_fetch_final.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.ebvo_finalize_pairs.argtypes = [vp, C.POINTER(StereoCalib), vp, vp, i32, vp]
    lib.ebvo_stereo_refine.argtypes = [vp, i32, C.POINTER(GnParams)]
    lib.ebvo_stereo_fetch_refined.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.ebvo_gn_refine_stereo.argtypes = [vp, vp, vp, i32, i32, ssz, ssz, vp, i32, vp, vp, vp, C.POINTER(GnParams),
                                          vp, vp, vp, vp, vp, vp]
    _lib = lib
    return lib


def ptr(a):
    """void* of a numpy array (None -> NULL)."""
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)
