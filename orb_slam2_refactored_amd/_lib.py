"""Loader for liborbslam2_amd.so (the HIP kernels + C-ABI, include/orbslam2_amd.h).

There is deliberately no CPU fallback: if the library is missing or cannot be loaded this module
raises, and every op in the package fails loudly.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("ORBSLAM2_AMD_LIB", PKG / "liborbslam2_amd.so"))


class OrbxParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scaleFactor", C.c_float), ("nlevels", C.c_int32),
                ("iniThFAST", C.c_int32), ("minThFAST", C.c_int32)]


class TriFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("kp_xy", C.c_void_p), ("octave", C.c_void_p), ("uright", C.c_void_p),
                ("has_mappoint", C.c_void_p), ("desc", C.c_void_p), ("n_nodes", C.c_int32),
                ("node_id", C.c_void_p), ("node_off", C.c_void_p), ("indices", C.c_void_p)]


class TriBatch(C.Structure):
    """orbm_tri_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("cap1", C.c_int32), ("cap2", C.c_int32),
                ("kps1", C.c_void_p), ("desc1", C.c_void_p), ("counts1", C.c_void_p), ("uright1", C.c_void_p),
                ("has_mappoint1", C.c_void_p), ("kps2", C.c_void_p), ("desc2", C.c_void_p), ("counts2", C.c_void_p),
                ("uright2", C.c_void_p), ("has_mappoint2", C.c_void_p), ("frame1", C.c_void_p),
                ("frame2", C.c_void_p), ("F12", C.c_void_p), ("ep2", C.c_void_p),
                ("fv_node1", C.c_void_p), ("fv_off1", C.c_void_p), ("fv_idx1", C.c_void_p),
                ("fv_n_nodes1", C.c_void_p), ("fv_node2", C.c_void_p), ("fv_off2", C.c_void_p),
                ("fv_idx2", C.c_void_p), ("fv_n_nodes2", C.c_void_p), ("fv_cap1", C.c_int32),
                ("fv_cap2", C.c_int32), ("n_levels", C.c_int32), ("scale_factors2", C.c_void_p),
                ("sigma2", C.c_void_p), ("only_stereo", C.c_int32)]


class BowBatch(C.Structure):
    """orbm_bow_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("cap1", C.c_int32), ("cap2", C.c_int32),
                ("kps1", C.c_void_p), ("desc1", C.c_void_p), ("mp_valid1", C.c_void_p), ("frame1", C.c_void_p),
                ("kps2", C.c_void_p), ("desc2", C.c_void_p), ("counts2", C.c_void_p),
                ("fv_node1", C.c_void_p), ("fv_off1", C.c_void_p), ("fv_idx1", C.c_void_p),
                ("fv_n_nodes1", C.c_void_p), ("fv_node2", C.c_void_p), ("fv_off2", C.c_void_p),
                ("fv_idx2", C.c_void_p), ("fv_n_nodes2", C.c_void_p), ("fv_cap1", C.c_int32),
                ("fv_cap2", C.c_int32), ("nnratio", C.c_float), ("check_orientation", C.c_int32),
                ("counts1", C.c_void_p), ("mp_valid2", C.c_void_p), ("frame2", C.c_void_p)]


class StereoView(C.Structure):
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("n_levels", C.c_int32),
                ("level", C.c_void_p), ("level_rows", C.c_void_p), ("level_cols", C.c_void_p),
                ("level_step", C.c_void_p)]


class BAProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("pose_R", C.c_void_p), ("pose_t", C.c_void_p),
                ("pose_fixed", C.c_void_p), ("n_points", C.c_int32), ("points", C.c_void_p),
                ("n_edges", C.c_int32), ("edge_point", C.c_void_p), ("edge_pose", C.c_void_p),
                ("edge_obs", C.c_void_p), ("edge_inv_sigma2", C.c_void_p), ("edge_cam", C.c_void_p)]


class BAResult(C.Structure):
    _fields_ = [("pose_R", C.c_void_p), ("pose_t", C.c_void_p), ("pose_q", C.c_void_p),
                ("points", C.c_void_p), ("edge_outlier", C.c_void_p), ("edge_chi2", C.c_void_p),
                ("iterations", C.c_int32 * 2), ("chi2", C.c_double * 2), ("ran", C.c_int32)]


class GBAOptions(C.Structure):
    """orbba_gba_options (include/orbslam2_amd.h)."""
    _fields_ = [("n_iterations", C.c_int32), ("robust", C.c_int32), ("stereo_rule", C.c_int32)]


class GBAResult(C.Structure):
    """orbba_gba_result (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("pose_R", "pose_t", "pose_q", "points", "pose_f", "points_f", "point_included",
                                          "edge_chi2")] + [
        ("iterations", C.c_int32), ("trials", C.c_int32), ("chi2", C.c_double), ("ran", C.c_int32)]


class GBAMap(C.Structure):
    """orbba_gba_map (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("n_origins", C.c_int32)] + [
        (k, C.c_void_p) for k in ("origins", "kf_child_off", "kf_child_idx", "kf_in_gba", "kf_pose", "kf_pose_gba",
                                  "kf_pose_bef", "mp_bad", "mp_in_gba", "mp_pos_gba", "mp_ref_kf", "mp_xw")]


class ProjBatch(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("total_kp", C.c_int32), ("total_mp", C.c_int32),
                ("kp_begin", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_uright", C.c_void_p),
                ("kp_desc", C.c_void_p), ("kp_claimed", C.c_void_p), ("bounds", C.c_void_p),
                ("mp_begin", C.c_void_p), ("mp_valid", C.c_void_p), ("mp_proj", C.c_void_p),
                ("mp_view_cos", C.c_void_p), ("mp_level", C.c_void_p), ("mp_desc", C.c_void_p),
                ("mp_has_obs", C.c_void_p), ("n_levels", C.c_int32), ("scale_factors", C.c_void_p),
                ("th", C.c_float), ("nnratio", C.c_float)]


class MotionBatch(C.Structure):
    """orbm_motion_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_frames", C.c_int32), ("total_kp", C.c_int32), ("total_mp", C.c_int32),
                ("kp_begin", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_uright", C.c_void_p),
                ("kp_desc", C.c_void_p), ("kp_angle", C.c_void_p), ("kp_claimed", C.c_void_p), ("bounds", C.c_void_p),
                ("mp_begin", C.c_void_p), ("mp_valid", C.c_void_p), ("mp_proj", C.c_void_p), ("mp_octave", C.c_void_p),
                ("mp_desc", C.c_void_p), ("mp_has_obs", C.c_void_p), ("mp_angle", C.c_void_p), ("motion", C.c_void_p),
                ("n_levels", C.c_int32), ("scale_factors", C.c_void_p), ("th", C.c_float),
                ("check_orientation", C.c_int32)]


class RelocBatch(C.Structure):
    """orbm_reloc_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_frames", C.c_int32), ("total_kp", C.c_int32), ("total_mp", C.c_int32),
                ("kp_begin", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_desc", C.c_void_p),
                ("kp_angle", C.c_void_p), ("kp_claimed", C.c_void_p), ("bounds", C.c_void_p), ("pose", C.c_void_p),
                ("camera", C.c_void_p), ("mp_begin", C.c_void_p), ("mp_valid", C.c_void_p), ("mp_xw", C.c_void_p),
                ("mp_max_min", C.c_void_p), ("mp_desc", C.c_void_p), ("mp_angle", C.c_void_p), ("n_levels", C.c_int32),
                ("scale_factors", C.c_void_p), ("log_scale_factor", C.c_float), ("th", C.c_float),
                ("orb_dist", C.c_int32), ("check_orientation", C.c_int32)]


class FuseBatch(C.Structure):
    """orbm_fuse_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_items", C.c_int32), ("total_kp", C.c_int32), ("total_mp", C.c_int32),
                ("kp_begin", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_uright", C.c_void_p),
                ("kp_desc", C.c_void_p), ("bounds", C.c_void_p), ("pose", C.c_void_p), ("camera", C.c_void_p),
                ("mp_begin", C.c_void_p), ("mp_valid", C.c_void_p), ("mp_xw", C.c_void_p), ("mp_max_min", C.c_void_p),
                ("mp_normal", C.c_void_p), ("mp_desc", C.c_void_p), ("n_levels", C.c_int32),
                ("scale_factors", C.c_void_p), ("inv_sigma2", C.c_void_p), ("log_scale_factor", C.c_float),
                ("th", C.c_float), ("chi2_gate", C.c_int32)]


class Sim3Batch(C.Structure):
    """orbm_sim3_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("total_kp1", C.c_int32), ("total_kp2", C.c_int32),
                ("kp1_begin", C.c_void_p), ("kp2_begin", C.c_void_p),
                ("kp1_xy", C.c_void_p), ("kp1_octave", C.c_void_p), ("kp1_desc", C.c_void_p),
                ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p), ("kp2_desc", C.c_void_p),
                ("bounds1", C.c_void_p), ("pose1", C.c_void_p), ("camera1", C.c_void_p),
                ("bounds2", C.c_void_p), ("pose2", C.c_void_p), ("camera2", C.c_void_p),
                ("mp1_valid", C.c_void_p), ("mp1_xw", C.c_void_p), ("mp1_max_min", C.c_void_p), ("mp1_desc", C.c_void_p),
                ("mp2_valid", C.c_void_p), ("mp2_xw", C.c_void_p), ("mp2_max_min", C.c_void_p), ("mp2_desc", C.c_void_p),
                ("s12", C.c_void_p), ("n_levels", C.c_int32), ("scale_factors", C.c_void_p),
                ("log_scale_factor", C.c_float), ("th", C.c_float)]


class InitBatch(C.Structure):
    """orbm_init_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("total_kp", C.c_int32), ("total_q", C.c_int32),
                ("kp_begin", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_desc", C.c_void_p),
                ("kp_angle", C.c_void_p), ("bounds", C.c_void_p), ("q_begin", C.c_void_p), ("q_octave", C.c_void_p),
                ("q_desc", C.c_void_p), ("q_angle", C.c_void_p), ("prev_matched", C.c_void_p), ("window", C.c_int32),
                ("nnratio", C.c_float), ("check_orientation", C.c_int32)]


class PoseBatch(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("edge_begin", C.c_void_p), ("pose_R", C.c_void_p), ("pose_t", C.c_void_p),
                ("cam", C.c_void_p), ("xw", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p)]


class PoseResult(C.Structure):
    _fields_ = [("pose_R", C.c_void_p), ("pose_t", C.c_void_p), ("n_inliers", C.c_void_p), ("outlier", C.c_void_p)]


class OptSim3Batch(C.Structure):
    """orbba_sim3_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("total_kp1", C.c_int32), ("total_kp2", C.c_int32),
                ("kp1_begin", C.c_void_p), ("kp2_begin", C.c_void_p),
                ("kp1_xy", C.c_void_p), ("kp1_octave", C.c_void_p), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p),
                ("pose1", C.c_void_p), ("camera1", C.c_void_p), ("pose2", C.c_void_p), ("camera2", C.c_void_p),
                ("mp1_valid", C.c_void_p), ("mp1_xw", C.c_void_p), ("mp2_valid", C.c_void_p), ("mp2_xw", C.c_void_p),
                ("s12", C.c_void_p), ("match12", C.c_void_p), ("n_levels", C.c_int32),
                ("inv_level_sigma2", C.c_void_p), ("max_chi2", C.c_float), ("fix_scale", C.c_int32)]


class OptSim3Result(C.Structure):
    """orbba_sim3_result (include/orbslam2_amd.h)."""
    _fields_ = [("s12", C.c_void_p), ("s12_g2o", C.c_void_p), ("match12", C.c_void_p), ("n_inliers", C.c_void_p),
                ("iterations", C.c_void_p)]


class EssentialGraph(C.Structure):
    """orbba_essential_graph (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("vertex_sim3", C.c_void_p), ("edge_sim3", C.c_void_p),
                ("fixed_slot", C.c_int32), ("fix_scale", C.c_int32), ("n_edges", C.c_int32),
                ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("edge_table", C.c_void_p),
                ("n_points", C.c_int32), ("points", C.c_void_p), ("point_ref", C.c_void_p)]


class EssentialGraphResult(C.Structure):
    """orbba_essential_graph_result (include/orbslam2_amd.h)."""
    _fields_ = [("sim3_g2o", C.c_void_p), ("pose", C.c_void_p), ("points", C.c_void_p), ("measurement", C.c_void_p),
                ("iterations", C.c_void_p), ("chi2", C.c_void_p), ("accept", C.c_void_p)]


class EssentialGraphTables(C.Structure):
    """orbba_eg_tables (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("kf_id", C.c_void_p), ("parent", C.c_void_p),
                ("loop_begin", C.c_void_p), ("loop_slot", C.c_void_p),
                ("covis_begin", C.c_void_p), ("covis_slot", C.c_void_p), ("covis_weight", C.c_void_p),
                ("n_connections", C.c_int32), ("conn_kf", C.c_void_p), ("conn_begin", C.c_void_p),
                ("conn_slot", C.c_void_p), ("curr_slot", C.c_int32), ("loop_kf_slot", C.c_int32)]


class Sim3SolverBatch(C.Structure):
    """orb_sim3solver_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("total_kp1", C.c_int32), ("total_kp2", C.c_int32),
                ("kp1_begin", C.c_void_p), ("kp2_begin", C.c_void_p),
                ("kp1_xy", C.c_void_p), ("kp1_octave", C.c_void_p), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p),
                ("pose1", C.c_void_p), ("camera1", C.c_void_p), ("pose2", C.c_void_p), ("camera2", C.c_void_p),
                ("mp1_valid", C.c_void_p), ("mp1_xw", C.c_void_p), ("mp2_valid", C.c_void_p), ("mp2_xw", C.c_void_p),
                ("s12", C.c_void_p), ("match12", C.c_void_p), ("n_levels", C.c_int32),
                ("level_sigma2", C.c_void_p), ("fix_scale", C.c_int32), ("draws", C.c_void_p), ("rand_max", C.c_int32),
                ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
                ("maxk", C.c_int32)]


class Sim3SolverResult(C.Structure):
    """orb_sim3solver_result (include/orbslam2_amd.h)."""
    _fields_ = [("s12", C.c_void_p), ("inlier", C.c_void_p), ("match12", C.c_void_p), ("found", C.c_void_p),
                ("n_inliers", C.c_void_p), ("iterations", C.c_void_p), ("max_inliers", C.c_void_p),
                ("terminate", C.c_void_p), ("hyp_inliers", C.c_void_p)]


class PnPSolverBatch(C.Structure):
    """orb_pnpsolver_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_frames", C.c_int32), ("total_kp", C.c_int32), ("kp_begin", C.c_void_p), ("kp_xy", C.c_void_p),
                ("kp_octave", C.c_void_p), ("camera", C.c_void_p), ("mp_valid", C.c_void_p), ("mp_xw", C.c_void_p),
                ("n_levels", C.c_int32), ("level_sigma2", C.c_void_p), ("draws", C.c_void_p), ("n_draws", C.c_int32),
                ("rand_max", C.c_int32), ("probability", C.c_double), ("min_inliers", C.c_int32),
                ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float), ("th2", C.c_float),
                ("maxk", C.c_int32)]


class PnPSolverResult(C.Structure):
    """orb_pnpsolver_result (include/orbslam2_amd.h)."""
    _fields_ = [("tcw", C.c_void_p), ("inlier", C.c_void_p), ("found", C.c_void_p), ("n_inliers", C.c_void_p),
                ("terminate", C.c_void_p), ("iterations", C.c_void_p), ("best_inliers", C.c_void_p),
                ("best_mask", C.c_void_p), ("best_tcw", C.c_void_p), ("hyp_inliers", C.c_void_p)]


class InitializerBatch(C.Structure):
    """orb_initializer_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("total_kp1", C.c_int32), ("total_kp2", C.c_int32),
                ("kp1_begin", C.c_void_p), ("kp2_begin", C.c_void_p), ("kp1_xy", C.c_void_p), ("kp2_xy", C.c_void_p),
                ("matches12", C.c_void_p), ("camera", C.c_void_p), ("draws", C.c_void_p), ("rand_max", C.c_int32),
                ("sigma", C.c_float), ("max_iterations", C.c_int32), ("min_parallax", C.c_float),
                ("min_triangulated", C.c_int32), ("rh_threshold", C.c_double)]


class InitializerResult(C.Structure):
    """orb_initializer_result (include/orbslam2_amd.h)."""
    _fields_ = [("found", C.c_void_p), ("model", C.c_void_p), ("r21t21", C.c_void_p), ("p3d", C.c_void_p),
                ("triangulated", C.c_void_p), ("score_h", C.c_void_p), ("score_f", C.c_void_p), ("best_h", C.c_void_p),
                ("best_f", C.c_void_p), ("h21", C.c_void_p), ("f21", C.c_void_p), ("inlier_h", C.c_void_p),
                ("inlier_f", C.c_void_p), ("hyp_score", C.c_void_p), ("n_good", C.c_void_p), ("parallax", C.c_void_p)]


class OrblmBatch(C.Structure):
    """orblm_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("cap1", C.c_int32), ("cap2", C.c_int32), ("n_frames1", C.c_int32),
                ("n_frames2", C.c_int32), ("kps1", C.c_void_p), ("counts1", C.c_void_p), ("uright1", C.c_void_p),
                ("depth1", C.c_void_p), ("kps2", C.c_void_p), ("counts2", C.c_void_p), ("uright2", C.c_void_p),
                ("depth2", C.c_void_p), ("has_mappoint2", C.c_void_p), ("mp_xw2", C.c_void_p), ("pose1", C.c_void_p),
                ("pose2", C.c_void_p), ("camera1", C.c_void_p), ("camera2", C.c_void_p), ("frame1", C.c_void_p),
                ("frame2", C.c_void_p), ("n_levels", C.c_int32), ("scale_factors1", C.c_void_p), ("sigma2_1", C.c_void_p),
                ("scale_factors2", C.c_void_p), ("sigma2_2", C.c_void_p), ("scale_factor", C.c_float),
                ("monocular", C.c_int32)]


class OrblmPairs(C.Structure):
    """orblm_pairs (include/orbslam2_amd.h)."""
    _fields_ = [("F12", C.c_void_p), ("ep2", C.c_void_p), ("baseline", C.c_void_p), ("median", C.c_void_p),
                ("skip", C.c_void_p), ("frame1", C.c_void_p), ("frame2", C.c_void_p), ("consts", C.c_void_p)]


class OrblmPoints(C.Structure):
    """orblm_points (include/orbslam2_amd.h)."""
    _fields_ = [("status", C.c_void_p), ("branch", C.c_void_p), ("xw", C.c_void_p), ("normal", C.c_void_p),
                ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("new_idx1", C.c_void_p),
                ("new_idx2", C.c_void_p), ("n_created", C.c_void_p), ("has_mappoint1", C.c_void_p),
                ("has_mappoint2", C.c_void_p)]


class OrbdbQueryBatch(C.Structure):
    """orbdb_query_batch (include/orbslam2_amd.h)."""
    _fields_ = [("n_queries", C.c_int32), ("cap", C.c_int32), ("n_frames", C.c_int32), ("bow_word", C.c_void_p),
                ("bow_weight", C.c_void_p), ("n_words", C.c_void_p), ("frame", C.c_void_p), ("covis", C.c_void_p),
                ("conn_off", C.c_void_p), ("conn_idx", C.c_void_p), ("min_score", C.c_void_p)]


class OrbdbResult(C.Structure):
    """orbdb_result (include/orbslam2_amd.h)."""
    _fields_ = [("cand", C.c_void_p), ("n_cand", C.c_void_p), ("words", C.c_void_p), ("scored", C.c_void_p),
                ("score", C.c_void_p), ("acc", C.c_void_p), ("bestk", C.c_void_p)]


# cv::KeyPoint layout (28 bytes)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

VP = C.c_void_p
I32 = C.c_int32
SZ = C.c_size_t

# name -> (restype, argtypes); every symbol declared in include/orbslam2_amd.h
class OrbtlMap(C.Structure):
    """orbtl_map (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf_bad", "kf_covis", "kf_parent", "kf_child_off", "kf_child_idx", "kf_n", "kf_mappoint",
                                  "mp_bad", "mp_xw", "mp_normal", "mp_max_min", "mp_desc", "mp_nobs", "mp_obs_off",
                                  "mp_obs_kf", "mp_visible")]


class OrbtlFrames(C.Structure):
    """orbtl_frames (include/orbslam2_amd.h)."""
    _fields_ = [("n_frames", C.c_int32), ("kp_cap", C.c_int32), ("kf_list_cap", C.c_int32), ("mp_cap", C.c_int32),
                ("n_levels", C.c_int32), ("log_scale_factor", C.c_float), ("min_view_cos", C.c_float)] + [
        (k, C.c_void_p) for k in ("frame_n", "frame_mappoint", "pose", "camera", "bounds", "local_kf", "n_local_kf")]


class OrbtlResult(C.Structure):
    """orbtl_result (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("reference_kf", "local_mp", "n_local_mp", "n_to_match", "status", "kp_begin",
                                          "mp_begin", "kp_claimed", "mp_valid", "mp_proj", "mp_view_cos", "mp_level",
                                          "mp_desc", "mp_has_obs", "votes")]


class OrbtfFrames(C.Structure):
    """orbtf_frames (include/orbslam2_amd.h)."""
    _fields_ = [("n_frames", C.c_int32), ("kp_cap", C.c_int32)] + [
        (k, C.c_void_p) for k in ("frame_n", "frame_mappoint", "frame_outlier", "pose", "camera", "bounds", "kp_xy", "kp_octave",
                                  "kp_uright", "kp_depth", "kp_angle", "kp_desc")]


class OrbtfMap(C.Structure):
    """orbtf_map (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32)] + [
        (k, C.c_void_p) for k in ("mp_xw", "mp_bad", "mp_nobs", "mp_found", "mp_replaced", "mp_desc", "kf_n", "kf_mappoint")]


class OrbtfEdges(C.Structure):
    """orbtf_edges (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("edge_begin", "pose_R", "pose_t", "cam", "xw", "obs", "inv_sigma2", "edge_kp")]


class OrbtfMotion(C.Structure):
    """orbtf_motion (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("motion", "kp_begin", "mp_begin", "kp_claimed", "mp_valid", "mp_proj", "mp_octave",
                                          "mp_desc", "mp_has_obs", "mp_angle")]


class OrbtfCreated(C.Structure):
    """orbtf_created (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("created_kp", "created_xw", "n_created", "n_processed")]


class OrbfrInput(C.Structure):
    """orbfr_input (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_int32) for k in ("n_frames", "kp_cap", "rows", "cols", "mode", "depth_type")] + [
        (k, C.c_void_p) for k in ("kps", "counts", "camera", "dist", "depth")] + [
        ("depth_frame_stride", C.c_size_t), ("depth_step", C.c_size_t), ("depth_factor", C.c_float)]


class OrbfrFrames(C.Structure):
    """orbfr_frames (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("frame_n", "kp_xy", "kp_octave", "kp_angle", "kp_un", "kp_uright", "kp_depth", "bounds",
                                          "frame_mappoint", "frame_outlier", "kp_begin")]


class OrbmkFrames(C.Structure):
    """orbmk_frames (include/orbslam2_amd.h)."""
    _fields_ = [("n_frames", C.c_int32), ("kp_cap", C.c_int32)] + [
        (k, C.c_void_p) for k in ("frame_n", "frame_mappoint", "kp_un", "kp_octave", "kp_uright", "kp_depth", "kp_desc", "pose",
                                  "camera")]


class OrbmkKeyframes(C.Structure):
    """orbmk_keyframes (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("kf_cap", C.c_int32), ("conn_cap", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf_id", "kf_n", "kf_mappoint", "kf_keypoint", "kf_kp_octave", "kf_uright", "kf_depth", "kf_desc",
                                  "kf_pose", "kf_camera", "kf_bad", "kf_not_erase", "kf_to_be_erased", "kf_parent",
                                  "kf_first_connection", "conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord",
                                  "kf_covis")]


class OrbmkMap(C.Structure):
    """orbmk_map (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32), ("n_obs", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf_id", "kf_n", "kf_mappoint", "kf_uright", "kf_bad", "kf_desc", "mp_bad", "mp_xw", "mp_normal",
                                  "mp_max_min", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "mp_first_kf_id", "mp_ref_kf",
                                  "mp_desc", "mp_obs_off", "mp_obs_kf", "mp_obs_idx")]


class OrbmkLists(C.Structure):
    """orbmk_lists (include/orbslam2_amd.h)."""
    _fields_ = [("n_items", C.c_int32), ("list_cap", C.c_int32), ("values_by_keypoint", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf1", "kf2", "n_list", "idx1", "idx2", "xw", "normal", "max_distance", "min_distance")] + [
        ("n_frames", C.c_int32), ("kp_cap", C.c_int32), ("item_frame", C.c_void_p), ("frame_mappoint", C.c_void_p)]


class OrbmkCreated(C.Structure):
    """orbmk_created (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("alloc", "status", "needed", "created", "n_created", "recent", "n_recent")] + [
        ("recent_cap", C.c_int32)]


class OrbmmPoints(C.Structure):
    """orbmm_points (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32), ("n_obs", C.c_int32),
                ("n_levels", C.c_int32)] + [
        (k, C.c_void_p) for k in ("scale_factors", "mp_bad", "mp_xw", "mp_ref_kf", "mp_obs_off", "mp_obs_kf", "mp_obs_idx",
                                  "kf_pose", "kf_n", "kf_kp_octave")] + [
        ("n_points", C.c_int32), ("point", C.c_void_p), ("mp_normal", C.c_void_p), ("mp_max_min", C.c_void_p)]


class OrbmmGraph(C.Structure):
    """orbmm_graph (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32), ("conn_cap", C.c_int32),
                ("n_obs", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf_id", "kf_n", "kf_mappoint", "mp_bad", "mp_obs_off", "mp_obs_kf", "conn_slot",
                                  "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_first_connection",
                                  "kf_parent", "kf_covis", "status")]


class OrbmmObserve(C.Structure):
    """orbmm_observe (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32), ("n_obs", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf_n", "kf_mappoint", "kf_uright", "mp_bad", "mp_nobs", "mp_found", "mp_visible",
                                  "mp_replaced", "mp_obs_off", "mp_obs_kf", "mp_obs_idx")]


class OrbmmApply(C.Structure):
    """orbmm_apply (include/orbslam2_amd.h)."""
    _fields_ = [("mode", C.c_int32), ("n_items", C.c_int32), ("n_entries", C.c_int32)] + [
        (k, C.c_void_p) for k in ("item_kf", "mp_begin", "point", "best_idx", "replace_point", "n_fused", "touched",
                                  "n_touched", "progress", "status")]


class OrbmmCsr(C.Structure):
    """orbmm_csr (include/orbslam2_amd.h)."""
    _fields_ = [("kf_bad", C.c_void_p), ("covis_begin", C.c_void_p), ("covis_slot", C.c_void_p),
                ("covis_weight", C.c_void_p), ("n_queries", C.c_int32), ("query", C.c_void_p), ("append_self", C.c_int32),
                ("conn_off", C.c_void_p), ("conn_idx", C.c_void_p)]


class OrblcMap(C.Structure):
    """orblc_map (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32), ("conn_cap", C.c_int32),
                ("n_obs", C.c_int32), ("n_levels", C.c_int32)] + [
        (k, C.c_void_p) for k in ("scale_factors", "kf_id", "kf_n", "kf_mappoint", "mp_bad", "mp_obs_off", "mp_obs_kf", "conn_slot",
                                  "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_first_connection", "kf_parent",
                                  "kf_covis", "status", "mp_obs_idx", "mp_ref_kf", "kf_kp_octave", "mp_xw", "kf_pose", "mp_normal",
                                  "mp_max_min", "mp_corrected_by", "mp_corrected_ref")]


class OrbmmCull(C.Structure):
    """orbmm_cull (include/orbslam2_amd.h)."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32), ("kf_cap", C.c_int32), ("conn_cap", C.c_int32),
                ("n_obs", C.c_int32)] + [
        (k, C.c_void_p) for k in ("kf_id", "kf_n", "kf_mappoint", "kf_kp_octave", "kf_uright", "kf_depth", "kf_pose", "kf_bad",
                                  "kf_not_erase", "kf_to_be_erased", "kf_tcp", "mp_bad", "mp_nobs", "mp_found", "mp_visible",
                                  "mp_first_kf_id", "mp_ref_kf", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "conn_slot",
                                  "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_parent", "kf_covis")]


class OrbbaWindowMap(C.Structure):
    """orbba_window_map (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_int32) for k in ("n_keyframes", "n_mappoints", "kf_cap", "conn_cap", "n_obs", "n_levels")] + [
        (k, C.c_void_p) for k in ("inv_sigma2", "scale_factors", "kf_id", "kf_n", "kf_bad", "kf_mappoint", "kf_keypoint",
                                  "kf_kp_octave", "kf_uright", "kf_camera", "kf_pose", "ord_slot", "n_ord", "mp_bad", "mp_xw",
                                  "mp_nobs", "mp_ref_kf", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "mp_normal", "mp_max_min")]


class OrbbaWindow(C.Structure):
    """orbba_window (include/orbslam2_amd.h)."""
    _fields_ = [(k, C.c_int32) for k in ("cap_poses", "cap_points", "cap_edges")] + [
        (k, C.c_void_p) for k in ("counts", "pose_kf", "pose_fixed", "point", "edge_point", "edge_pose", "edge_kf", "edge_idx",
                                  "edge_obs", "edge_inv_sigma2", "edge_cam")]


class OrbbaMapResult(C.Structure):
    """orbba_map_result (include/orbslam2_amd.h)."""
    _fields_ = [("iterations", C.c_int32 * 2), ("chi2", C.c_double * 2), ("ran", C.c_int32), ("counts", C.c_int32 * 4),
                ("status", C.c_int32)]


SIGNATURES = {    "orbx_create": (C.c_int, [C.POINTER(OrbxParams), C.c_int, C.POINTER(VP)]),
    "orbx_destroy": (C.c_int, [VP]),
    "orbx_scale_tables": (C.c_int, [VP, VP, VP, VP, VP, VP]),
    "orbx_max_keypoints": (C.c_int, [VP, C.c_int, C.c_int, C.POINTER(I32)]),
    "orbx_set_opencv_compat": (C.c_int, [VP, C.c_int, C.c_int]),
    "orbx_get_opencv_compat": (C.c_int, [VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "orbx_extract": (C.c_int, [VP, VP, C.c_int, C.c_int, SZ, VP, VP, C.c_int, C.POINTER(C.c_int)]),
    "orbx_pyramid_level": (C.c_int, [VP, C.c_int, VP, SZ, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "orbx_extract_batch_device": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, SZ, SZ, VP, VP, VP, C.c_int, VP]),
    "orbx_batch_status": (C.c_int, [VP, VP, C.POINTER(C.c_uint32)]),
    "orbx_fault_word_device": (C.c_int, [VP, C.POINTER(VP)]),
    "orbx_pyramid_device": (C.c_int, [VP, C.c_int, C.c_int, C.POINTER(VP), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(SZ)]),
    "orbm_descriptor_distance": (C.c_int, [VP, VP]),
    "orbm_hamming_top2_device": (C.c_int, [VP, C.c_int, VP, C.c_int, VP, VP, VP, VP]),
    "orbm_bf_match_batch_device": (C.c_int, [VP, VP, C.c_int, VP, VP, C.c_int, VP, C.c_int, C.c_float, C.c_int,
                                             VP, VP, VP, VP, VP]),
    "orbm_bf_match": (C.c_int, [VP, C.c_int, VP, C.c_int, C.c_float, C.c_int, VP, VP, VP, VP]),
    "orbm_check_orientation": (C.c_int, [VP, C.c_int, VP, C.c_int, VP, C.POINTER(I32)]),
    "orbm_check_orientation_batch_device": (C.c_int, [VP, C.c_int, C.c_int, VP, VP, C.c_int, C.c_int, VP, C.c_int,
                                                      VP, C.c_int, VP, VP]),
    "orbm_search_for_triangulation": (C.c_int, [C.POINTER(TriFrame), C.POINTER(TriFrame), VP, VP, VP, VP,
                                                C.c_int, C.c_int, VP, C.POINTER(I32)]),
    "orbm_search_for_triangulation_batch_device": (C.c_int, [C.POINTER(TriBatch), VP, VP, VP]),
    "orbm_search_by_bow_batch_device": (C.c_int, [C.POINTER(BowBatch), VP, VP, VP]),
    "orbm_search_by_bow_kf_batch_device": (C.c_int, [C.POINTER(BowBatch), VP, VP, VP]),
    "orbm_compute_stereo_matches": (C.c_int, [C.POINTER(StereoView), C.POINTER(StereoView), VP, VP, C.c_float,
                                              C.c_float, VP, VP]),
    "orbx_stereo_matches_batch_device": (C.c_int, [VP, VP, C.c_int, VP, VP, VP, VP, VP, VP, C.c_int, C.c_float,
                                                   C.c_float, VP, VP, VP]),
    "orbx_stereo_matches_last": (C.c_int, [VP, VP, C.c_float, C.c_float, VP, VP, C.c_int]),
    "orbm_search_by_projection": (C.c_int, [C.POINTER(ProjBatch), VP, VP, C.c_int]),
    "orbm_search_by_projection_device": (C.c_int, [C.POINTER(ProjBatch), VP, VP, VP]),
    "orbm_search_by_projection_motion_device": (C.c_int, [C.POINTER(MotionBatch), VP, VP, VP]),
    "orbm_search_for_initialization": (C.c_int, [C.POINTER(InitBatch), VP, VP, C.c_int]),
    "orbm_search_by_projection_reloc": (C.c_int, [C.POINTER(RelocBatch), VP, VP, C.c_int]),
    "orbm_search_by_projection_reloc_device": (C.c_int, [C.POINTER(RelocBatch), VP, VP, VP]),
    "orbm_search_for_initialization_device": (C.c_int, [C.POINTER(InitBatch), VP, VP, VP]),
    "orbm_fuse": (C.c_int, [C.POINTER(FuseBatch), VP, VP, VP, C.c_int]),
    "orbm_fuse_device": (C.c_int, [C.POINTER(FuseBatch), VP, VP, VP, VP]),
    "orbm_search_by_projection_sim3": (C.c_int, [C.POINTER(FuseBatch), VP, VP, VP, C.c_int]),
    "orbm_search_by_projection_sim3_device": (C.c_int, [C.POINTER(FuseBatch), VP, VP, VP, VP]),
    "orbm_search_by_sim3": (C.c_int, [C.POINTER(Sim3Batch), VP, VP, VP, VP, C.c_int]),
    "orbm_search_by_sim3_device": (C.c_int, [C.POINTER(Sim3Batch), VP, VP, VP, VP, VP]),
    "orbm_distinctive_descriptors": (C.c_int, [VP, VP, C.c_int32, VP, VP, VP, C.c_int]),
    "orbm_distinctive_descriptors_device": (C.c_int, [VP, VP, C.c_int32, VP, VP, VP, VP]),
    "orbv_load_text": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(VP)]),
    "orbv_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP, VP, VP, C.c_int, C.POINTER(VP)]),
    "orbv_destroy": (C.c_int, [VP]),
    "orbv_info": (C.c_int, [VP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                            C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "orbv_transform": (C.c_int, [VP, VP, C.c_int, C.c_int, VP, VP, C.POINTER(C.c_int), VP, VP, VP,
                                 C.POINTER(C.c_int)]),
    "orbv_transform_batch_device": (C.c_int, [VP, VP, VP, C.c_int, C.c_int, C.c_int, VP, VP, VP, VP, VP, VP, VP, VP]),
    "orbba_local_ba": (C.c_int, [C.POINTER(BAProblem), C.POINTER(BAResult), VP, C.c_int]),
    "orbba_bundle_adjustment": (C.c_int, [C.POINTER(BAProblem), C.POINTER(GBAOptions), C.POINTER(GBAResult), VP, C.c_int]),
    "orbba_debug_ldlt_grid": (C.c_int, [VP, VP, C.c_int, VP, VP, C.c_int]),
    "orbba_debug_ldlt_lds": (C.c_int, [VP, VP, C.c_int, C.c_double, C.c_int, C.c_int, VP, VP, C.c_int]),
    "orbba_debug_ldlt_hbm": (C.c_int, [VP, VP, C.c_int, VP, VP, C.c_int]),
    "orbba_gba_update_map": (C.c_int, [C.POINTER(GBAMap), C.c_int]),
    "orbba_gba_update_map_device": (C.c_int, [C.POINTER(GBAMap), VP]),
    "orbba_pose_optimization": (C.c_int, [C.POINTER(PoseBatch), C.POINTER(PoseResult), C.c_int]),
    "orbba_pose_optimization_device": (C.c_int, [C.POINTER(PoseBatch), C.POINTER(PoseResult), VP]),
    "orbba_optimize_sim3": (C.c_int, [C.POINTER(OptSim3Batch), C.POINTER(OptSim3Result), C.c_int]),
    "orbba_optimize_sim3_device": (C.c_int, [C.POINTER(OptSim3Batch), C.POINTER(OptSim3Result), VP]),
    "orbba_optimize_essential_graph": (C.c_int, [C.POINTER(EssentialGraph), C.POINTER(EssentialGraphResult), C.c_int]),
    "orbba_optimize_essential_graph_device": (C.c_int, [C.POINTER(EssentialGraph), C.POINTER(EssentialGraphResult), VP]),
    "orbba_essential_graph_profile": (C.c_int, [C.POINTER(EssentialGraph), C.POINTER(EssentialGraphResult), C.c_int, VP]),
    "orbba_essential_graph_edges": (C.c_int, [C.POINTER(EssentialGraphTables), C.c_int32, C.c_int32, VP, VP, VP, VP]),
    "orb_sim3solver_iterate": (C.c_int, [C.POINTER(Sim3SolverBatch), C.POINTER(Sim3SolverResult), C.c_int]),
    "orb_sim3solver_iterate_device": (C.c_int, [C.POINTER(Sim3SolverBatch), C.POINTER(Sim3SolverResult), VP]),
    "orb_pnpsolver_iterate": (C.c_int, [C.POINTER(PnPSolverBatch), C.POINTER(PnPSolverResult), C.c_int]),
    "orb_pnpsolver_iterate_device": (C.c_int, [C.POINTER(PnPSolverBatch), C.POINTER(PnPSolverResult), VP]),
    "orb_initializer_initialize": (C.c_int, [C.POINTER(InitializerBatch), C.POINTER(InitializerResult), C.c_int]),
    "orb_initializer_initialize_device": (C.c_int, [C.POINTER(InitializerBatch), C.POINTER(InitializerResult), VP]),
    "orblm_prepare_pairs": (C.c_int, [C.POINTER(OrblmBatch), C.POINTER(OrblmPairs), C.c_int]),
    "orblm_prepare_pairs_device": (C.c_int, [C.POINTER(OrblmBatch), C.POINTER(OrblmPairs), VP]),
    "orblm_triangulate": (C.c_int, [C.POINTER(OrblmBatch), C.POINTER(OrblmPairs), VP, C.POINTER(OrblmPoints), C.c_int]),
    "orblm_triangulate_device": (C.c_int, [C.POINTER(OrblmBatch), C.POINTER(OrblmPairs), VP, C.POINTER(OrblmPoints), VP]),
    "orblm_create_new_map_points": (C.c_int, [C.POINTER(OrblmBatch), C.POINTER(TriBatch), C.c_int32, C.POINTER(OrblmPairs),
                                              C.POINTER(OrblmPoints), VP, VP, C.c_int]),
    "orblm_create_new_map_points_device": (C.c_int, [C.POINTER(OrblmBatch), C.POINTER(TriBatch), C.c_int32,
                                                     C.POINTER(OrblmPairs), C.POINTER(OrblmPoints), VP, VP, VP]),
    "orbdb_create": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, C.POINTER(VP)]),
    "orbdb_destroy": (C.c_int, [VP]),
    "orbdb_info": (C.c_int, [VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "orbdb_clear": (C.c_int, [VP, VP]),
    "orbdb_add_device": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, C.c_int, C.c_int, VP]),
    "orbdb_erase_device": (C.c_int, [VP, C.c_int, VP, VP]),
    "orbdb_min_score_device": (C.c_int, [VP, C.POINTER(OrbdbQueryBatch), VP, VP, VP, VP]),
    "orbdb_detect_reloc_device": (C.c_int, [VP, C.POINTER(OrbdbQueryBatch), C.POINTER(OrbdbResult), VP]),
    "orbdb_detect_loop_device": (C.c_int, [VP, C.POINTER(OrbdbQueryBatch), C.POINTER(OrbdbResult), VP]),
    "orbdb_add": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, C.c_int, C.c_int]),
    "orbdb_erase": (C.c_int, [VP, C.c_int, VP]),
    "orbdb_min_score": (C.c_int, [VP, C.POINTER(OrbdbQueryBatch), VP, VP, VP]),
    "orbdb_detect_reloc": (C.c_int, [VP, C.POINTER(OrbdbQueryBatch), C.POINTER(OrbdbResult)]),
    "orbdb_detect_loop": (C.c_int, [VP, C.POINTER(OrbdbQueryBatch), C.POINTER(OrbdbResult)]),
    "orbdb_read_slots": (C.c_int, [VP, VP, VP]),
    "orbtl_track_local_map_device": (C.c_int, [C.POINTER(OrbtlMap), C.POINTER(OrbtlFrames), C.POINTER(OrbtlResult), VP]),
    "orbtl_track_local_map": (C.c_int, [C.POINTER(OrbtlMap), C.POINTER(OrbtlFrames), C.POINTER(OrbtlResult), C.c_int]),
    "orbba_local_window_device": (C.c_int, [C.POINTER(OrbbaWindowMap), C.c_int32, C.POINTER(OrbbaWindow), VP]),
    "orbba_local_window": (C.c_int, [C.POINTER(OrbbaWindowMap), C.c_int32, C.POINTER(OrbbaWindow), C.c_int]),
    "orbba_local_ba_apply_device": (C.c_int, [C.POINTER(OrbbaWindowMap), C.POINTER(OrbbaWindow), VP, VP, VP, VP, VP]),
    "orbba_local_ba_apply": (C.c_int, [C.POINTER(OrbbaWindowMap), C.POINTER(OrbbaWindow), VP, VP, VP, VP, C.c_int]),
    "orbba_local_ba_map_device": (C.c_int, [C.POINTER(OrbbaWindowMap), C.c_int32, C.POINTER(OrbbaWindow),
                                            C.POINTER(OrbbaMapResult), VP, VP]),
    "orbba_local_ba_map": (C.c_int, [C.POINTER(OrbbaWindowMap), C.c_int32, C.POINTER(OrbbaMapResult), VP, C.c_int]),
    "orbmm_update_normal_depth_device": (C.c_int, [C.POINTER(OrbmmPoints), VP]),
    "orbmm_update_normal_depth": (C.c_int, [C.POINTER(OrbmmPoints), C.c_int]),
    "orbmm_update_connections_device": (C.c_int, [C.POINTER(OrbmmGraph), C.c_int32, VP, VP]),
    "orbmm_update_connections": (C.c_int, [C.POINTER(OrbmmGraph), C.c_int32, VP, C.c_int]),
    "orbmm_children_device": (C.c_int, [C.c_int32, VP, VP, VP, VP]),
    "orbmm_children": (C.c_int, [C.c_int32, VP, VP, VP, C.c_int]),
    "orbmm_covis_csr_device": (C.c_int, [C.POINTER(OrbmmGraph), C.POINTER(OrbmmCsr), VP]),
    "orbmm_covis_csr": (C.c_int, [C.POINTER(OrbmmGraph), C.POINTER(OrbmmCsr), C.c_int]),
    "orbmm_cull_map_points_device": (C.c_int, [C.POINTER(OrbmmCull), C.c_int32, VP, C.c_int32, C.c_int32, VP, VP]),
    "orbmm_cull_map_points": (C.c_int, [C.POINTER(OrbmmCull), C.c_int32, VP, C.c_int32, C.c_int32, VP, C.c_int]),
    "orbmm_cull_keyframes_device": (C.c_int, [C.POINTER(OrbmmCull), C.c_int32, C.c_int32, C.c_float, VP, VP, VP, VP]),
    "orbmm_cull_keyframes": (C.c_int, [C.POINTER(OrbmmCull), C.c_int32, C.c_int32, C.c_float, VP, VP, VP, C.c_int]),
    "orbmm_compact_observations_device": (C.c_int, [C.c_int32, C.c_int32, VP, VP, VP, VP, VP, VP, VP]),
    "orbmm_compact_observations": (C.c_int, [C.c_int32, C.c_int32, VP, VP, VP, VP, VP, VP, C.c_int]),
    "orbmm_children_live_device": (C.c_int, [C.c_int32, VP, VP, VP, VP, VP]),
    "orbmm_children_live": (C.c_int, [C.c_int32, VP, VP, VP, VP, C.c_int]),
    "orbmm_add_keyframe_observations_device": (C.c_int, [C.POINTER(OrbmmObserve), C.c_int32, VP, VP, VP, VP, VP]),
    "orbmm_add_keyframe_observations": (C.c_int, [C.POINTER(OrbmmObserve), C.c_int32, VP, VP, VP, VP, C.c_int]),
    "orbmm_fuse_apply_device": (C.c_int, [C.POINTER(OrbmmObserve), C.POINTER(OrbmmApply), VP]),
    "orbmm_fuse_apply": (C.c_int, [C.POINTER(OrbmmObserve), C.POINTER(OrbmmApply), C.c_int]),
    "orbmm_grow_observations_device": (C.c_int, [C.c_int32, C.c_int32, VP, VP, VP, C.c_int32, VP, C.c_int32, VP, VP, VP, VP, VP]),
    "orbmm_grow_observations": (C.c_int, [C.c_int32, C.c_int32, VP, VP, VP, C.c_int32, VP, C.c_int32, VP, VP, VP, VP, C.c_int]),
    "orblc_connected_device": (C.c_int, [C.POINTER(OrblcMap), C.c_int32, VP, VP, VP]),
    "orblc_connected": (C.c_int, [C.POINTER(OrblcMap), C.c_int32, VP, VP, C.c_int]),
    "orblc_propagate_device": (C.c_int, [C.POINTER(OrblcMap), C.c_int32, VP, VP, C.c_int32, VP, VP, VP, VP, VP]),
    "orblc_propagate": (C.c_int, [C.POINTER(OrblcMap), C.c_int32, VP, VP, C.c_int32, VP, VP, VP, VP, C.c_int]),
    "orblc_loop_connections_device": (C.c_int, [C.POINTER(OrblcMap), VP, C.c_int32, VP, VP, VP, VP, VP]),
    "orblc_loop_connections": (C.c_int, [C.POINTER(OrblcMap), VP, C.c_int32, VP, VP, VP, VP, C.c_int]),
    "orbba_essential_graph_edges_device": (C.c_int, [C.POINTER(EssentialGraphTables), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                     C.c_int32, VP, VP, VP, VP, VP]),
    "orbx_pack_descriptors": (C.c_int,[VP, C.c_int, VP, VP, C.c_int, VP, C.c_int, VP]),
    **{name + suffix: (C.c_int, args + [last]) for suffix, last in (("_device", VP), ("", C.c_int)) for name, args in {
        "orbtf_apply_matches": [C.POINTER(OrbtfFrames), C.c_int32, VP, VP, C.c_int32, C.c_int32, VP, C.c_int32],
        "orbtf_pose_edges": [C.POINTER(OrbtfFrames), C.POINTER(OrbtfMap), VP, C.c_int32, C.POINTER(OrbtfEdges)],
        "orbtf_finish_pose": [C.POINTER(OrbtfFrames), C.POINTER(OrbtfMap), C.c_int32, C.POINTER(OrbtfEdges),
                              C.POINTER(PoseResult), C.c_int32, C.c_int32, VP, VP, VP],
        "orbtf_motion_project": [C.POINTER(OrbtfFrames), C.POINTER(OrbtfFrames), C.POINTER(OrbtfMap), VP, VP, C.c_int32,
                                 C.POINTER(OrbtfMotion)],
        "orbtf_end_frame": [C.POINTER(OrbtfFrames), C.POINTER(OrbtfMap), C.c_float, VP, VP, VP, VP],
        "orbtf_drop_outliers": [C.POINTER(OrbtfFrames)],
        "orbtf_stereo_points": [C.POINTER(OrbtfFrames), C.POINTER(OrbtfMap), C.c_int32, C.c_float, C.POINTER(OrbtfCreated)],
    }.items()},
    "orbfr_build_frames_device": (C.c_int, [C.POINTER(OrbfrInput), C.POINTER(OrbfrFrames), VP]),
    "orbfr_build_frames": (C.c_int, [C.POINTER(OrbfrInput), C.POINTER(OrbfrFrames), C.c_int]),
    "orbfr_image_bounds": (C.c_int, [C.c_int32, C.c_int32, VP, VP, VP]),
    "orbfr_undistort_points": (C.c_int, [VP, VP, VP, C.c_int32, VP]),
    "orbmk_insert_keyframes_device": (C.c_int, [C.POINTER(OrbmkFrames), C.POINTER(OrbmkKeyframes), C.c_int32, VP, VP, VP, VP, VP]),
    "orbmk_insert_keyframes": (C.c_int, [C.POINTER(OrbmkFrames), C.POINTER(OrbmkKeyframes), C.c_int32, VP, VP, VP, VP, C.c_int]),
    "orbmk_create_points_device": (C.c_int, [C.POINTER(OrbmkMap), C.POINTER(OrbmkLists), C.POINTER(OrbmkCreated), VP]),
    "orbmk_create_points": (C.c_int, [C.POINTER(OrbmkMap), C.POINTER(OrbmkLists), C.POINTER(OrbmkCreated), C.c_int]),
    "orbx_profile_enable": (C.c_int, [VP, C.c_int]),
    "orbx_profile_read": (C.c_int, [VP, VP, VP]),
    "orbx_debug_level_candidates": (C.c_int, [VP, C.c_int, C.c_int, VP, C.c_int, C.POINTER(C.c_int)]),
    "orbx_debug_qt_sort": (C.c_int, [VP, C.c_int, VP]),
    "orbba_debug_po_wave": (C.c_int, [VP, VP, VP]),
    "orbx_debug_level_selected": (C.c_int, [VP, C.c_int, C.c_int, VP, C.c_int, C.POINTER(C.c_int)]),
    "orbx_debug_describe": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, SZ, VP, C.c_int, VP, VP]),
    "orb_last_error": (C.c_char_p, []),
    "orb_device_count": (C.c_int, []),
}

_lib = None


class OrbError(RuntimeError):
    pass


def lib():
    """Load the native library (raises if absent: no fallback path exists)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OrbError(f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        l = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            # an A/B build named by ORBSLAM2_AMD_LIB may predate newer entry points: those stay
            # unbound (calling one fails); the in-tree library must export every symbol
            if os.environ.get("ORBSLAM2_AMD_LIB") and not hasattr(l, name):
                continue
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().orb_last_error().decode(errors="replace")
        raise OrbError(f"{what} failed with status {rc}: {msg}")
    return rc


def ptr(a: np.ndarray):
    # The buffer protocol is the cheapest address (~1 us; a.ctypes.data_as(VP) builds numpy's ctypes
    # helper, ~3 us, per array per call); read-only or empty arrays take the helper.
    try:
        return VP(C.addressof(C.c_char.from_buffer(a)))
    except (TypeError, ValueError, BufferError):
        return VP(a.ctypes.data)


def tptr(t):
    """Device pointer of a torch tensor."""
    return VP(t.data_ptr())


def stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return VP(s.cuda_stream)
