"""MI355X-native RGB-D front-end (ORB + LSD/LBD + PEAC planes + Hamming matching).

Thin ctypes binding over libhvo.so (csrc/, C ABI in include/hvo.h) plus host-side mirrors
of the reference's operator interfaces so parity tests read like the reference's call sites:

    ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)(image)
        -> reference include/ORBextractor.h:53-61, src/ORBextractor.cc:1041
    LINEextractor(numOctaves, scale, nLSDFeature)(image)
        -> reference include/LineExtractor.h:186-193, src/LineExtractor.cpp:329
    PlaneDetection(K, depthMapFactor).run(depth_u16)
        -> reference include/PlaneExtractor.h:36-56, src/PlaneExtractor.cpp:26-66
    ORBmatcher.DescriptorDistance / LSDmatcher.match
        -> reference src/ORBmatcher.cc:1676, src/LSDmatcher.cpp:828

There is no CPU path: if libhvo.so is missing or no gfx950 device is present every call
raises HvoError.  This package never imports the oracle.
"""
import ctypes as C
import os
import subprocess
import numpy as np

from . import _marshal as _m

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# HVO_LIB: developer knob, points the binding at an experimental build of the same library (A/B measurements)
_LIBPATH = os.environ.get("HVO_LIB") or os.path.join(_CSRC, "libhvo.so")
_LIB = None
# Load-order rule (multi-GPU path): torch's wheel carries its own HIP runtime; whichever of torch / libhvo.so is loaded first decides
# which libamdhip64 the process runs on, and a process that loaded libhvo.so first cannot initialise torch.cuda afterwards.  lib()
# records the order and torch_order_check() (called by every entry point that hands device memory to torch, dist.py) raises a clear
# error instead of the runtime's obscure one.
_LOADED_BEFORE_TORCH = False

HVO_OK = 0
STAGE_ORB, STAGE_LSD, STAGE_PLANES, STAGE_ALL = 1, 2, 4, 7
SLAB_LABELS = 1            # hvo_batch_pack_results_ex: the int8 label image at the end of every slab
STAGE_LSD_CULL = 8        # STAGE_LSD followed by Frame::cullingLine (merged lines replace the extractor's)
# the rest of the Frame constructor as pipeline stages (include/hvo.h): isLineGood, vanishing points, ComputePlanes' tail, the two grids
STAGE_LINES3D, STAGE_VP, STAGE_PLANE_TAIL, STAGE_GRIDS = 16, 32, 64, 128
STAGE_FRAME = 1 | 2 | 8 | 4 | 16 | 32 | 64 | 128
LINE_MATCH_NNR, LINE_MATCH_BF, LINE_MATCH_DOUBLE = 0, 1, 2

KEYPOINT_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                        ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KEYLINE_DT = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"),
                       ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                       ("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"),
                       ("sox", "<f4"), ("soy", "<f4"), ("eox", "<f4"), ("eoy", "<f4"),
                       ("length", "<f4"), ("num_pixels", "<i4")])
PLANE_DT = np.dtype([("normal", "<f8", 3), ("center", "<f8", 3), ("mse", "<f8"),
                     ("n_points", "<i4"), ("rid", "<i4")])
class VpResult(C.Structure):
    _fields_ = [("vps", (C.c_double * 3) * 3), ("score", C.c_double), ("best", C.c_int32), ("n_hypotheses", C.c_int32)]


LINE3D_DT = np.dtype([("A", "<f8", 3), ("B", "<f8", 3), ("line_nor", "<f8", 3), ("line_eq", "<f4", 3), ("good", "<i4"),
                      ("n_samples", "<i4"), ("n_inliers", "<i4"), ("inlier_mask", "<u4"), ("pad", "<i4")])
PLANE_CLOUD_DT = np.dtype([("coef", "<f4", 4), ("valid", "<i4"), ("gate_ok", "<i4"), ("first", "<i4"), ("n_points", "<i4"), ("n_pixels", "<i4"), ("n_inliers", "<i4")])
SURFACE_NORMAL_DT = np.dtype([("normal", "<f4", 3), ("position", "<f4", 3), ("frame_x", "<i4"), ("frame_y", "<i4")])
READING_BLUR_FLOAT, READING_LSD_8U = 1, 2

EXPORTS = [
    "hvo_abi_version", "hvo_default_params", "hvo_create", "hvo_destroy", "hvo_strerror", "hvo_last_error",
    "hvo_extract_orb", "hvo_extract_lsd", "hvo_compute_planes",
    "hvo_hamming_matrix", "hvo_hamming_knn2", "hvo_match_nnr", "hvo_match_lines_geom", "hvo_search_lines_by_projection", "hvo_stream_match_lines_geom", "hvo_stream_search_lines_by_projection", "hvo_search_lines_by_projection_map", "hvo_stream_search_lines_by_projection_map", "hvo_search_by_projection", "hvo_stereo_from_rgbd",
    "hvo_undistort_keypoints", "hvo_image_bounds", "hvo_assign_features_to_grid", "hvo_assign_lines_to_grid",
    "hvo_extract_lsd_culled", "hvo_set_line_culling", "hvo_lines_3d", "hvo_vanishing_points", "hvo_plane_clouds", "hvo_surface_normals", "hvo_search_by_projection_map", "hvo_frame_bf_match", "hvo_search_double",
    "hvo_batch_upload", "hvo_batch_run", "hvo_batch_download", "hvo_extract_batch", "hvo_batch_slab_layout", "hvo_batch_pack_results", "hvo_batch_slab_layout_ex", "hvo_batch_pack_results_ex", "hvo_batch_stage_upload", "hvo_batch_commit_staged", "hvo_batch_results_async", "hvo_batch_results_wait",
    "hvo_profile_last", "hvo_profile_enable", "hvo_lsd_async_report", "hvo_set_readings", "hvo_stream_set_readings", "hvo_pin_host", "hvo_unpin_host",
    "hvo_stream_create", "hvo_stream_destroy", "hvo_stream_last_error", "hvo_stream_capacity", "hvo_stream_image_bounds",
    "hvo_stream_submit", "hvo_stream_poll", "hvo_stream_collect", "hvo_stream_stage_ms",
    "hvo_stream_search_by_projection", "hvo_stream_match_lines", "hvo_stream_project_last", "hvo_search_by_projection_tracked",
    "hvo_tail_capacity", "hvo_set_tail_params", "hvo_batch_download_tail", "hvo_stream_collect_tail", "hvo_normals_lpvo",
    "hvo_track_manhattan", "hvo_stream_track_manhattan", "hvo_batch_track_manhattan",
    "hvo_plane_map_create", "hvo_plane_map_destroy", "hvo_plane_map_set", "hvo_plane_map_set_bad", "hvo_plane_map_counts", "hvo_plane_map_slot",
    "hvo_plane_map_last_error", "hvo_match_planes", "hvo_stream_match_planes", "hvo_batch_match_planes", "hvo_pose_optimize", "hvo_stream_pose_optimize", "hvo_batch_pose_optimize", "hvo_pose_last_kernel_ms", "hvo_stream_pose_last_kernel_ms",
    "hvo_line_struct_default_params", "hvo_line_struct_optimize", "hvo_stream_line_struct_optimize", "hvo_batch_line_struct_optimize",
    "hvo_line_opt_last_kernel_ms", "hvo_stream_line_opt_last_kernel_ms",
    "hvo_line_map_create", "hvo_line_map_destroy", "hvo_line_map_set", "hvo_line_map_set_many", "hvo_line_map_set_bad", "hvo_line_map_set_observed",
    "hvo_line_map_counts", "hvo_line_map_slot", "hvo_line_map_last_error",
    "hvo_search_local_lines", "hvo_stream_search_local_lines", "hvo_batch_search_local_lines",
    "hvo_point_map_create", "hvo_point_map_destroy", "hvo_point_map_set", "hvo_point_map_set_many", "hvo_point_map_set_bad", "hvo_point_map_set_observed",
    "hvo_point_map_counts", "hvo_point_map_slot", "hvo_point_map_last_error",
    "hvo_search_local_points", "hvo_stream_search_local_points", "hvo_batch_search_local_points",
    "hvo_vocabulary_create", "hvo_vocabulary_load_text", "hvo_vocabulary_destroy", "hvo_vocabulary_info",
    "hvo_compute_bow", "hvo_stream_compute_bow", "hvo_batch_compute_bow", "hvo_search_by_bow", "hvo_stream_search_by_bow",
    "hvo_bow_last_kernel_ms", "hvo_stream_bow_last_kernel_ms",
    "hvo_keyframe_db_create", "hvo_keyframe_db_destroy", "hvo_keyframe_db_last_error", "hvo_keyframe_db_add", "hvo_stream_keyframe_db_add",
    "hvo_keyframe_db_erase", "hvo_keyframe_db_clear", "hvo_keyframe_db_set_covisible", "hvo_keyframe_db_get", "hvo_keyframe_db_info",
    "hvo_keyframe_db_query", "hvo_stream_keyframe_db_query", "hvo_batch_keyframe_db_query", "hvo_keyframe_db_last_kernel_ms",
    "hvo_pnp_default_params", "hvo_pnp_ransac", "hvo_stream_pnp_ransac", "hvo_pnp_last_kernel_ms", "hvo_stream_pnp_last_kernel_ms",
    "hvo_search_by_projection_keyframe", "hvo_stream_search_by_projection_keyframe",
    "hvo_fuse_points", "hvo_fuse_points_slots", "hvo_stream_fuse_points",
    "hvo_fuse_lines", "hvo_fuse_lines_slots", "hvo_stream_fuse_lines",
    "hvo_create_new_map_points", "hvo_stream_create_new_map_points", "hvo_create_new_map_lines", "hvo_stream_create_new_map_lines",
    "hvo_refresh_map_points", "hvo_refresh_map_lines", "hvo_point_map_refresh", "hvo_line_map_refresh",
    "hvo_update_map_planes", "hvo_stream_update_map_planes", "hvo_plane_map_get_points", "hvo_plane_update_transform",
    "hvo_local_ba_create", "hvo_local_ba_destroy", "hvo_local_ba_last_error", "hvo_local_ba_last_ms", "hvo_local_ba_last_profile", "hvo_local_ba_default_params", "hvo_local_ba_optimize",
    "hvo_kfi_default_params", "hvo_kf_insert_create", "hvo_kf_insert_destroy", "hvo_kf_insert_last_error", "hvo_create_keyframe_features", "hvo_stream_create_keyframe_features",
]


class HvoError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = _LIB.hvo_strerror(status).decode() if _LIB is not None else "libhvo.so unavailable"
        super().__init__("hvo status %d (%s) %s" % (status, msg, what))


class Params(C.Structure):
    _fields_ = [("orb_nfeatures", C.c_int32), ("orb_scale_factor", C.c_float), ("orb_nlevels", C.c_int32),
                ("orb_ini_th_fast", C.c_int32), ("orb_min_th_fast", C.c_int32),
                ("lsd_num_octaves", C.c_int32), ("lsd_scale", C.c_float), ("lsd_nfeatures", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("depth_map_factor", C.c_float), ("device", C.c_int32), ("max_batch", C.c_int32)]


class FrameIn(C.Structure):
    _fields_ = [("gray", C.c_void_p), ("gray_stride", C.c_int),
                ("depth", C.c_void_p), ("depth_stride", C.c_int)]


class FrameOut(C.Structure):
    _fields_ = [("kp", C.c_void_p), ("desc", C.c_void_p), ("kp_cap", C.c_int), ("n_kp", C.c_int),
                ("kl", C.c_void_p), ("ldesc", C.c_void_p), ("linefn", C.c_void_p), ("kl_cap", C.c_int), ("n_kl", C.c_int),
                ("labels", C.c_void_p), ("planes", C.c_void_p), ("pl_cap", C.c_int), ("n_planes", C.c_int),
                ("status", C.c_int), ("labels8", C.c_void_p)]


class StreamParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth", C.c_int32), ("stages", C.c_uint32),
                ("dist5", C.c_float * 5), ("bf", C.c_float), ("seed", C.c_uint32), ("plane_dist_th", C.c_float), ("vp_th_angle", C.c_float)]


class FrameTail(C.Structure):
    _fields_ = [("lines3d", C.c_void_p), ("vp", C.c_void_p), ("vp_idx", C.c_void_p),
                ("plane_clouds", C.c_void_p), ("cloud_xyz", C.c_void_p), ("cloud_cap", C.c_int), ("n_cloud", C.c_int),
                ("normals", C.c_void_p), ("normals_cap", C.c_int), ("n_normals", C.c_int),
                ("pt_cell_start", C.c_void_p), ("pt_cell_items", C.c_void_p), ("pt_items_cap", C.c_int), ("n_pt_items", C.c_int),
                ("ln_cell_start", C.c_void_p), ("ln_cell_items", C.c_void_p), ("ln_items_cap", C.c_int), ("n_ln_items", C.c_int),
                ("status", C.c_int)]


class MfResult(C.Structure):
    """hvo_mf_result: one Tracking::TrackManhattanFrame call (R row-major)"""
    _fields_ = [("R", C.c_float * 9), ("axis_vec", (C.c_float * 3) * 3), ("density", C.c_float * 3),
                ("found", C.c_int32 * 3), ("n_found", C.c_int32), ("n_in_cone", C.c_int32 * 3), ("n_selected", C.c_int32 * 3),
                ("min_num_sn", C.c_int32), ("tracked", C.c_int32), ("status", C.c_int32)]

    def to_dict(self):
        return dict(R=np.array(self.R[:], np.float32).reshape(3, 3), axis_vec=np.array([r[:] for r in self.axis_vec], np.float32),
                    density=np.array(self.density[:], np.float32), found=list(self.found), n_found=self.n_found, n_in_cone=list(self.n_in_cone),
                    n_selected=list(self.n_selected), min_num_sn=self.min_num_sn, tracked=self.tracked, status=self.status)

class PlaneMatch(C.Structure):
    """hvo_plane_match: one PlaneMatcher::SearchMapByCoefficients call (slots, -1 = none)"""
    _fields_ = [("n_planes", C.c_int32), ("n_matches", C.c_int32), ("match", C.c_int32 * 64), ("vertical", C.c_int32 * 64),
                ("parallel", C.c_int32 * 64), ("plane_idx", C.c_int32 * 64), ("dist", C.c_float * 64), ("pM", (C.c_float * 4) * 64)]

    def to_dict(self):
        n = self.n_planes
        return dict(n_planes=n, n_matches=self.n_matches, match=np.array(self.match[:n], np.int32), vertical=np.array(self.vertical[:n], np.int32),
                    parallel=np.array(self.parallel[:n], np.int32), plane_idx=np.array(self.plane_idx[:n], np.int32),
                    dist=np.array(self.dist[:n], np.float32), pM=np.array([r[:] for r in self.pM], np.float32).reshape(64, 4)[:n])

PLANE_UPDATE_MERGE, PLANE_UPDATE_INSERT, PLANE_UPDATE_MAX_POINTS = 0, 1, 1 << 20


class PlaneUpdate(C.Structure):
    """hvo_plane_update: up to 64 operations (frame plane, slot, PLANE_UPDATE_MERGE / _INSERT), applied in list order"""
    _fields_ = [("n", C.c_int32), ("plane", C.c_int32 * 64), ("slot", C.c_int32 * 64), ("op", C.c_int32 * 64)]


class PlaneUpdateResult(C.Structure):
    _fields_ = [("status", C.c_int32 * 64), ("n_frame", C.c_int32 * 64), ("n_before", C.c_int32 * 64), ("n_after", C.c_int32 * 64), ("n_done", C.c_int32)]

    def to_dict(self, n):
        return dict(n_done=self.n_done, **{k: np.array(getattr(self, k)[:n], np.int32) for k in ("status", "n_frame", "n_before", "n_after")})


def _plane_update_arg(ops):
    """ops: a PlaneUpdate, or a sequence of (plane, slot, op)"""
    if isinstance(ops, PlaneUpdate):
        return ops, max(0, min(ops.n, 64))
    ops = list(ops)
    if len(ops) > 64:
        raise ValueError("at most 64 plane updates per call")
    u = PlaneUpdate(); u.n = len(ops)
    for k, (p, s_, o) in enumerate(ops):
        u.plane[k] = p; u.slot[k] = s_; u.op[k] = o
    return u, len(ops)


def plane_update_transform(Tcw):
    """the matrix a MERGE applies to the frame's cloud: rows 0..2 of inverse(toSE3Quat(Tcw)) as (3, 4) doubles (host arithmetic, no device)"""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(12); M = np.zeros(12, np.float64)
    rc = lib().hvo_plane_update_transform(_p(T), _p(M))
    if rc != HVO_OK:
        raise HvoError(rc, "plane_update_transform")
    return M.reshape(3, 4)


PLANE_MATCH_DEFAULT_TH = (0.1, 0.86, 0.08716, 0.9962)       # PlaneMatcher's constructor defaults (include/PlaneMatcher.h:17)


class PosePlaneParams(C.Structure):
    """hvo_pose_plane_params: Plane.AngleInfo, DistanceInfo, ParallelInfo, VerticalInfo, Chi, VPChi of the settings file"""
    _fields_ = [(k, C.c_double) for k in ("angle_info", "distance_info", "parallel_info", "vertical_info", "chi", "vp_chi")]


class PoseCamera(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "bf", "b")]


class PoseProblem(C.Structure):
    """hvo_pose_problem: one frame's Optimizer::PoseOptimization input (include/hvo.h)"""
    _fields_ = [("Tcw", C.c_float * 12), ("n_points", C.c_int32), ("n_lines", C.c_int32), ("n_planes", C.c_int32), ("reserved", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("kp_un", "uright", "inv_sigma2", "linefn", "lines3d", "plane_coef",
                                          "pt_has", "pt_xyz", "ln_has", "ln_xyz", "pl_has", "pl_coef_w",
                                          "plane_map", "slot_match", "slot_parallel", "slot_vertical")]


class PoseFlags(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier")]


class PoseResult(C.Structure):
    """hvo_pose_result; after a call through the binding the outlier flags hang on it as numpy arrays (pt_outlier, ln_outlier, pl_outlier
    (n_planes x 3: plane, parallel, vertical), vp_outlier)"""
    _fields_ = [("Tcw_d", C.c_double * 12), ("Tcw", C.c_float * 12), ("ret", C.c_int32), ("n_initial", C.c_int32), ("n_bad", C.c_int32),
                ("n_line_bad", C.c_int32), ("n_edges", C.c_int32), ("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4),
                ("status", C.c_int32), ("reserved", C.c_int32), ("lam", C.c_double * 4), ("chi2", C.c_double * 4)]

    def to_dict(self):
        d = {k: (np.array(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}
        d["Tcw_d"] = d["Tcw_d"].reshape(3, 4); d["Tcw"] = d["Tcw"].reshape(3, 4)
        for k in ("pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier"):
            if hasattr(self, k): d[k] = getattr(self, k)
        return d


LINE_STRUCT_CONSTRAINTS, LINE_STRUCT_OPTIMIZE = 1, 2
LINE_STRUCT_ROW_UNSET, LINE_STRUCT_ROW_Z0 = 0, 1


class LineStructParams(C.Structure):
    """hvo_line_struct_params: the thresholds of Manhattan::computeStructConstrains and the constants of Optimizer::LineOptStruct"""
    _fields_ = [("cos_par", C.c_double), ("cos_perp", C.c_double), ("huber_delta", C.c_double), ("chi2_reject", C.c_double),
                ("chi2_round", C.c_float * 2), ("min_constraints", C.c_int32), ("iterations", C.c_int32), ("row_rule", C.c_int32), ("mode", C.c_uint32)]


class LineStructProblem(C.Structure):
    _fields_ = [("n_lines", C.c_int32), ("reserved", C.c_int32), ("linefn", C.c_void_p), ("lines3d", C.c_void_p)]


class LineOptResult(C.Structure):
    """hvo_line_opt_result; the binding hangs rel (n x n int8) and lines (n x 6 doubles: A, B after the call) on it"""
    _fields_ = [("n_lines", C.c_int32), ("n_lines_to_opt", C.c_int32), ("n_edges", C.c_int32), ("n_par_edges", C.c_int32), ("n_perp_edges", C.c_int32),
                ("rounds", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("n_flagged", C.c_int32 * 2),
                ("written_back", C.c_int32), ("status", C.c_int32), ("lam", C.c_double * 2), ("chi2", C.c_double * 2)]

LINE_MAP_MAX_QUERIES = 16384      # lines in view per call (the search core's limit)


class LocalLinesParams(C.Structure):
    """hvo_local_lines_params"""
    _fields_ = [("bounds", C.c_float * 4), ("log_scale_factor", C.c_float), ("th", C.c_float), ("nn_ratio", C.c_float)]


class LocalLinesFrame(C.Structure):
    """hvo_local_lines_frame: the frame side on host arrays"""
    _fields_ = [("kl", C.c_void_p), ("linefn", C.c_void_p), ("l3d", C.c_void_p), ("desc", C.c_void_p), ("n_kl", C.c_int32),
                ("cell_start", C.c_void_p), ("cell_items", C.c_void_p)]


class LocalLinesIO(C.Structure):
    """hvo_local_lines_io: one frame's inputs and outputs"""
    _fields_ = [("n_kl", C.c_int32), ("held", C.c_void_p), ("seen_extra", C.c_void_p), ("n_seen_extra", C.c_int32), ("in_view_slot", C.c_void_p),
                ("proj", C.c_void_p), ("view_cos", C.c_void_p), ("level", C.c_void_p), ("match_idx", C.c_void_p), ("match_dist", C.c_void_p),
                ("n_par", C.c_void_p), ("n_perp", C.c_void_p), ("rel_map", C.c_void_p)]


class LocalLinesResult(C.Structure):
    """hvo_local_lines_result: one Tracking::SearchLocalLines + computeStructConstInMap call.  The arrays (held, in_view_slot, proj, view_cos,
    level, match_idx, match_dist, n_par, n_perp, rel_map or None) are attached as attributes by the calls that return it."""
    _fields_ = [("n_slots_tested", C.c_int32), ("n_in_view", C.c_int32), ("n_matches", C.c_int32), ("n_gated", C.c_int32), ("status", C.c_int32),
                ("kernel_ms", C.c_float * 3)]

    def to_dict(self):
        d = dict(n_slots_tested=self.n_slots_tested, n_in_view=self.n_in_view, n_matches=self.n_matches, n_gated=self.n_gated, status=self.status,
                 kernel_ms=tuple(self.kernel_ms))
        for k in ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist", "n_par", "n_perp", "rel_map"):
            d[k] = getattr(self, k, None)
        return d

# ---------------------------------------------------------------------------------------
# the binding records (_marshal): each call family's arrays declared once, and the argument building its Context and Stream forms share
# ---------------------------------------------------------------------------------------
_i8, _u8, _i32, _f32, _f64 = np.int8, np.uint8, np.int32, np.float32, np.float64
REQ, OPT = _m.REQ, _m.OPT


def _ret(obj, rc, name, finish, check=True):
    """the return path of a Context or Stream call: obj._chk raises, obj._last_error is its handle's message"""
    return _m.returned(rc, obj._last_error, name, obj._chk, finish, check, HVO_OK)


def _results(table, R, lens):
    """one result record of R per entry of lens (the table's lengths) -> (R, what _finished needs)"""
    return R, [(table.alloc(R[j], **l), l) for j, l in enumerate(lens)]


def _finished(table, R, keep, ok=True):
    return [table.finish(R[j], a, ok, **l) for j, (a, l) in enumerate(keep)]


def _entry(f, dt, cols=1, length="n"):
    return (f, dt, cols, length, None)


# ---- the local-map searches: held per key feature, everything else per slot in view; 0 / -1 / 256 before the call
def _map_out(proj_cols, per_key=()):
    q = lambda f, dt, cols=1: (f, dt, cols, "capq", "n_in_view")
    return _m.Outputs([_entry("held", _i32, 1, "n_key"), q("in_view_slot", _i32), q("proj", _f32, proj_cols), q("view_cos", _f32), q("level", _i32),
                       q("match_idx", _i32), q("match_dist", _i32)] + [_entry(f, _i32, 1, "n_key") for f in per_key], 0,
                      fill=dict(held=-1, match_idx=-1, match_dist=256))


LL_OUT, LP_OUT = _map_out(4, ("n_par", "n_perp")), _map_out(3)


def _ll_params(bounds4, log_scale_factor, th, nn_ratio):
    p = LocalLinesParams(); _m.bounds(p.bounds, bounds4)
    p.log_scale_factor = log_scale_factor; p.th = th; p.nn_ratio = nn_ratio
    return p


def _lp_params(bounds4, log_scale_factor, n_levels, bf, th, th_high, nn_ratio, view_cos_limit):
    p = LocalPointsParams(); _m.bounds(p.bounds, bounds4)
    p.log_scale_factor = log_scale_factor; p.n_levels = n_levels; p.bf = bf; p.th = th; p.th_high = th_high; p.nn_ratio = nn_ratio
    p.view_cos_limit = view_cos_limit
    return p


def _map_io(io, table, n_key, what, n_slots, max_queries, held, seen_extra):
    """fills io (n_kl / n_kp already set) -> (io, the arrays it points at).  held stays -1 beyond the given entries"""
    a = table.alloc(io, n_key=n_key, capq=max(1, min(n_slots, max_queries)))
    if held is not None:
        hh = np.asarray(held, np.int32).reshape(-1)
        if len(hh) != n_key:
            raise ValueError("held must have one entry per key %s (%d)" % (what, n_key))
        a["held"][:n_key] = hh
    a["seen_extra"] = ex = np.ascontiguousarray([] if seen_extra is None else seen_extra, np.int32).reshape(-1)
    io.seen_extra = _m.ptr(ex); io.n_seen_extra = len(ex)
    return io, a


def _map_finish(r, table, a, n_key):
    """attaches held and the in-view arrays, cut to the counts (nothing in view after a refusal) -> the in-view count"""
    ok = r.status == HVO_OK
    for k, v in table.cut(r, a, n_key=n_key, capq=len(a["in_view_slot"]) if ok else 0).items():
        setattr(r, k, v)
    return r.n_in_view if ok else 0


def _ll_io(n_kl, n_slots, held, seen_extra, want_rel):
    """-> (LocalLinesIO, dict of the arrays it points at)"""
    io = LocalLinesIO(); io.n_kl = n_kl
    io, a = _map_io(io, LL_OUT, n_kl, "line", n_slots, LINE_MAP_MAX_QUERIES, held, seen_extra)
    a["rel_map"] = np.zeros(max(n_kl, 1) * len(a["in_view_slot"]), np.int8) if want_rel else None
    io.rel_map = _m.ptr(a["rel_map"])
    return io, a


def _ll_finish(r, a, n_kl):
    nq = _map_finish(r, LL_OUT, a, n_kl)
    r.rel_map = None if a["rel_map"] is None else a["rel_map"][: n_kl * nq].reshape(n_kl, nq)
    return r


def _lp_io(n_kp, n_slots, held, seen_extra):
    """-> (LocalPointsIO, dict of the arrays it points at)"""
    io = LocalPointsIO(); io.n_kp = n_kp
    return _map_io(io, LP_OUT, n_kp, "point", n_slots, POINT_MAP_MAX_QUERIES, held, seen_extra)


def _lp_finish(r, a, n_kp):
    _map_finish(r, LP_OUT, a, n_kp)
    return r


LP_FRAME = _m.Inputs([("kp_un", KEYPOINT_DT, (), REQ, "n"), ("uright", _f32, (), OPT, "n"), ("desc", _u8, (32,), REQ, "n")])


def _lp_frame(kp_un, uright, desc):
    """a frame on host arrays (mvKeysUn, mvuRight or None, mDescriptors) -> (LocalPointsFrame, the arrays, its key-point count)"""
    F = LocalPointsFrame()
    return (F,) + LP_FRAME.fill(F, dict(kp_un=kp_un, uright=uright, desc=desc))


POINT_MAP_MAX_SLOTS = 1 << 20
POINT_MAP_MAX_QUERIES = 16384     # points in view per call (the search core's limit)
HELD_FOREIGN_OBSERVED, HELD_FOREIGN_UNOBSERVED = -2, -3     # values of held besides a slot and -1: a map point that is not in the point map


class LocalPointsParams(C.Structure):
    """hvo_local_points_params"""
    _fields_ = [("bounds", C.c_float * 4), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32), ("bf", C.c_float), ("th", C.c_float),
                ("th_high", C.c_int32), ("nn_ratio", C.c_float), ("view_cos_limit", C.c_float)]


class LocalPointsFrame(C.Structure):
    """hvo_local_points_frame: the frame side on host arrays"""
    _fields_ = [("kp_un", C.c_void_p), ("uright", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int32)]


class LocalPointsIO(C.Structure):
    """hvo_local_points_io: one frame's inputs and outputs"""
    _fields_ = [("n_kp", C.c_int32), ("held", C.c_void_p), ("seen_extra", C.c_void_p), ("n_seen_extra", C.c_int32), ("in_view_slot", C.c_void_p),
                ("proj", C.c_void_p), ("view_cos", C.c_void_p), ("level", C.c_void_p), ("match_idx", C.c_void_p), ("match_dist", C.c_void_p)]


class LocalPointsResult(C.Structure):
    """hvo_local_points_result: one Tracking::SearchLocalPoints call.  The arrays (held, in_view_slot, proj, view_cos, level, match_idx,
    match_dist) are attached as attributes by the calls that return it."""
    _fields_ = [("n_slots_tested", C.c_int32), ("n_in_view", C.c_int32), ("n_matches", C.c_int32), ("status", C.c_int32), ("kernel_ms", C.c_float * 3)]

    def to_dict(self):
        d = dict(n_slots_tested=self.n_slots_tested, n_in_view=self.n_in_view, n_matches=self.n_matches, status=self.status, kernel_ms=tuple(self.kernel_ms))
        for k in ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist"):
            d[k] = getattr(self, k, None)
        return d

VOC_TF_IDF, VOC_TF, VOC_IDF, VOC_BINARY = 0, 1, 2, 3                                                  # DBoW2::WeightingType
VOC_L1_NORM, VOC_L2_NORM, VOC_CHI_SQUARE, VOC_KL, VOC_BHATTACHARYYA, VOC_DOT_PRODUCT = 0, 1, 2, 3, 4, 5    # DBoW2::ScoringType
BOW_MAX_FEATURES = 4096


class VocabularyDesc(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("k", "L", "n_nodes", "n_words", "scoring", "weighting", "device")]


class Bow(C.Structure):
    _fields_ = [("cap", C.c_int32), ("word_id", C.c_void_p), ("node_id", C.c_void_p), ("bow_word", C.c_void_p), ("bow_value", C.c_void_p),
                ("fv_node", C.c_void_p), ("fv_start", C.c_void_p), ("fv_index", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("n_features", "n_words", "n_nodes", "n_valid", "n_short", "computed", "status")]


class BowKeyframe(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("node_id", C.c_void_p), ("has_map_point", C.c_void_p), ("angle", C.c_void_p), ("n", C.c_int32)]


class BowSearchParams(C.Structure):
    _fields_ = [("nnratio", C.c_float), ("check_orientation", C.c_int32), ("th_low", C.c_int32)]


class BowMatches(C.Structure):
    _fields_ = [("match_kf", C.c_void_p), ("n_matches", C.c_int32), ("status", C.c_int32)]


KFDB_MAX_SLOTS, KFDB_MAX_COVISIBLE = 16384, 10
KFDB_RELOC, KFDB_LOOP = 0, 1


class KeyframeDbDesc(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("n_live", C.c_int32), ("scoring", C.c_int32), ("device", C.c_int32),
                ("pooled_words", C.c_int64), ("pool_capacity", C.c_int64), ("next_sequence", C.c_int64)]


class LocalBAParams(C.Structure):
    _fields_ = [("iterations", C.c_int32 * 2), ("max_trials", C.c_int32), ("stop_at_poll", C.c_int32), ("huber_delta", C.c_double * 3),
                ("chi2_gate", C.c_double * 3), ("inv_sigma", C.c_double * 3)]


LOCAL_BA_GRAPH_ARRAYS = (("Tcw", np.float32), ("fixed", np.uint8), ("cam", np.float32), ("pt_pos", np.float32), ("pt_obs_start", np.int32),
                         ("pt_obs_kf", np.int32), ("pt_obs_uv", np.float32), ("pt_obs_inv_sigma2", np.float32), ("ln_pos", np.float64),
                         ("ln_manh_idx", np.int32), ("ln_obs_start", np.int32), ("ln_obs_kf", np.int32), ("ln_obs_fn", np.float64),
                         ("par_start", np.int32), ("par_kf", np.int32), ("par_idx", np.int32), ("par_fn", np.float64), ("par_map_size", np.int32),
                         ("perp_start", np.int32), ("perp_kf", np.int32), ("perp_idx", np.int32), ("perp_fn", np.float64), ("perp_map_size", np.int32),
                         ("manh_axis", np.float64))


class LocalBAGraph(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_points", C.c_int32), ("n_lines", C.c_int32), ("manh_available", C.c_int32)] + \
               [(n, C.c_void_p) for n, _ in LOCAL_BA_GRAPH_ARRAYS]


LOCAL_BA_RESULT_ARRAYS = ("Tcw_f", "Tcw_d", "pt_f", "pt_d", "ln_f", "ln_d", "pt_erase", "ln_erase", "manh_erase", "par_erase", "perp_erase",
                          "par_made", "perp_made", "line_made")


class LocalBAResult(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LOCAL_BA_RESULT_ARRAYS] + \
               [("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("lam", C.c_double * 2), ("chi2", C.c_double * 2),
                ("n_free_kf", C.c_int32), ("n_pt_edges", C.c_int32), ("n_line_obs", C.c_int32), ("n_manh_edges", C.c_int32),
                ("n_par_edges", C.c_int32), ("n_perp_edges", C.c_int32), ("n_lines_made", C.c_int32), ("rounds", C.c_int32),
                ("stopped_at", C.c_int32), ("status", C.c_int32)]


LBA_OPTIMISED, LBA_NOTHING, LBA_STOPPED = 0, 1, 2
LBA_LIMITS = dict(free_kf=64, kf=1024, points=65536, lines=16384, pt_obs=1 << 20, ln_obs=1 << 18, struct=1 << 18)


KFI_KEYFRAME, KFI_INIT, KFI_TEMPORAL = 0, 1, 2
KFI_CREATED, KFI_BAD_LEVEL = 0, 1
KFI_MAX_FEATURES, KFI_MAX_LINES = 16384, 2048


class KfiParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("th_depth", C.c_float), ("n_levels", C.c_int32), ("line_n_levels", C.c_int32), ("line_scale_factor", C.c_float),
                ("line_geometry", C.c_int32), ("cos_par", C.c_double), ("cos_perp", C.c_double), ("first_point_slot", C.c_int32), ("first_line_slot", C.c_int32)]


class KfiFrame(C.Structure):
    _fields_ = [("kp_un", C.c_void_p), ("depth", C.c_void_p), ("desc", C.c_void_p), ("n_kp", C.c_int32),
                ("keylines", C.c_void_p), ("ldesc", C.c_void_p), ("lines3d", C.c_void_p), ("n_kl", C.c_int32)]


_KFI_IO = (("held_points", np.int32, 1, 0), ("held_lines", np.int32, 1, 1),
           ("pt_index", np.int32, 1, 0), ("pt_slot", np.int32, 1, 0), ("pt_status", np.uint8, 1, 0), ("pt_pos", np.float32, 3, 0), ("pt_normal", np.float32, 3, 0),
           ("pt_max_dist", np.float32, 1, 0), ("pt_min_dist", np.float32, 1, 0),
           ("ln_index", np.int32, 1, 1), ("ln_slot", np.int32, 1, 1), ("ln_status", np.uint8, 1, 1), ("ln_pos", np.float64, 6, 1), ("ln_wvec", np.float64, 3, 1),
           ("ln_normal", np.float64, 3, 1), ("ln_max_dist", np.float32, 1, 1), ("ln_min_dist", np.float32, 1, 1))


class KfiIO(C.Structure):
    _fields_ = [("n_kp", C.c_int32), ("n_kl", C.c_int32)] + [(k, C.c_void_p) for k, _, _, _ in _KFI_IO] + [("ln_rel", C.c_void_p)]


class KfiResult(C.Structure):
    _fields_ = [("n_kp", C.c_int32), ("n_kl", C.c_int32), ("n_point_entries", C.c_int32), ("n_points_created", C.c_int32), ("n_line_entries", C.c_int32),
                ("n_lines_created", C.c_int32), ("n_point_candidates", C.c_int32), ("n_line_candidates", C.c_int32), ("kernel_ms", C.c_float), ("status", C.c_int32)]


KFI_UNTOUCHED = 119                # the byte the binding fills its output arrays with: an entry the call did not write keeps it


# ---- CreateNewKeyFrame: KFI_UNTOUCHED before the call, but held_* start at -1 (the call's own "holds nothing")
KFI_OUT = _m.Outputs([(k, dt, c, ("n_kp", "n_kl")[s], None if k.startswith("held") else ("n_point_entries", "n_line_entries")[s]) for k, dt, c, s in _KFI_IO],
                     KFI_UNTOUCHED, fill=dict(held_points=-1, held_lines=-1), scalars=[f for f, _ in KfiResult._fields_])


def _kfi_args(n_kp, n_kl, mode, th_depth, n_levels, line_n_levels, line_scale_factor, line_geometry, cos_par, cos_perp, first_point_slot, first_line_slot,
              held_points, held_lines):
    p = KfiParams(); lib().hvo_kfi_default_params(C.byref(p))
    p.mode = mode; p.th_depth = th_depth; p.n_levels = n_levels; p.line_n_levels = line_n_levels; p.line_scale_factor = line_scale_factor
    p.line_geometry = 1 if line_geometry else 0; p.first_point_slot = first_point_slot; p.first_line_slot = first_line_slot
    if cos_par is not None: p.cos_par = cos_par
    if cos_perp is not None: p.cos_perp = cos_perp
    n_kp, n_kl = int(n_kp), int(n_kl)
    io = KfiIO(); io.n_kp, io.n_kl = n_kp, n_kl
    a = KFI_OUT.alloc(io, n_kp=n_kp, n_kl=n_kl)
    for k, given, n in (("held_points", held_points, n_kp), ("held_lines", held_lines, n_kl)):
        if given is not None: a[k][:n] = np.asarray(given, np.int32).reshape(-1)[:n]
    a["ln_rel"] = np.full((max(n_kl, 1), max(n_kl, 1)), KFI_UNTOUCHED, np.uint8); io.ln_rel = a["ln_rel"].ctypes.data
    return p, io, a


class KfiOutput:
    """what create_keyframe_features returns: .held_points / .held_lines after the call; per selected point, in creation order, .pt_index,
    .pt_slot, .pt_status, .pt_pos, .pt_normal, .pt_max_dist, .pt_min_dist; per selected line .ln_index .. .ln_min_dist with .ln_wvec, and
    .ln_rel (entries x key lines; HVO_KFI_KEYFRAME only); the counts of hvo_kfi_result and .kernel_ms"""


def _kfi_finish(r, a, n_kp, n_kl, mode):
    o = KfiOutput()
    for k, v in KFI_OUT.finish(r, a, n_kp=n_kp, n_kl=n_kl).items(): setattr(o, k, v)
    ne = r.n_line_entries
    o.ln_rel = a["ln_rel"].reshape(-1)[:ne * n_kl].reshape(ne, n_kl) if mode == KFI_KEYFRAME and n_kl else np.zeros((0, n_kl), np.uint8)
    return o


class KfdbParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_score", C.c_float), ("connected", C.c_void_p), ("n_connected", C.c_int32)]


class KfdbResult(C.Structure):
    _fields_ = [("cap", C.c_int32), ("candidate", C.c_void_p), ("n_candidates", C.c_int32),
                ("slot_cap", C.c_int32), ("words", C.c_void_p), ("score", C.c_void_p), ("acc", C.c_void_p), ("best", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("n_sharing", "max_common", "min_common", "n_scored")] + [("best_acc_score", C.c_float), ("status", C.c_int32)]


# ---- the key-frame database and the bag of words: zeros (-1 for the per-feature ids) before the call, copies afterwards
KFDB_OUT = _m.Outputs([("candidate", _i32, 1, "cap", "n_candidates")], 0, scalars=("n_sharing", "max_common", "min_common", "n_scored"), copy=True)
KFDB_VIEWS = _m.Outputs([_entry(k, dt, 1, "n_slots") for k, dt in (("words", _i32), ("score", _f32), ("acc", _f32), ("best", _i32))], 0, copy=True)


def _kfdb_args(n_slots, mode, min_score, connected, views, cap=None):
    """(hvo_kfdb_params, hvo_kfdb_result, the arrays behind them) for a database of n_slots slots"""
    conn = np.ascontiguousarray([] if connected is None else connected, np.int32).reshape(-1)
    P = KfdbParams(); P.mode = mode; P.min_score = float(min_score); P.connected = _m.ptr(conn); P.n_connected = len(conn)
    R = KfdbResult(); R.cap = max(n_slots, 1) if cap is None else int(cap); R.slot_cap = n_slots if views else 0
    a = dict(KFDB_OUT.alloc(R, cap=R.cap), connected=conn)
    if views:
        a.update(KFDB_VIEWS.alloc(R, n_slots=n_slots))
    return P, R, a


def _kfdb_finish(R, a, n_slots, views):
    """dict(candidates (slots, the reference's order), n_sharing, max_common, min_common, n_scored, best_acc_score; with views: words, score, acc,
    best per slot)"""
    r = KFDB_OUT.finish(R, a, cap=len(a["candidate"])); r["candidates"] = r.pop("candidate"); r["best_acc_score"] = np.float32(R.best_acc_score)
    if views:
        r.update(KFDB_VIEWS.cut(R, a, n_slots=n_slots))
    return r


BOW_OUT = _m.Outputs([("word_id", _i32, 1, "cap", "n_features"), ("node_id", _i32, 1, "cap", "n_features"), ("bow_word", _i32, 1, "cap", "n_words"),
                      ("bow_value", _f64, 1, "cap", "n_words"), ("fv_node", _i32, 1, "cap", "n_nodes"), ("fv_start", _i32, 1, "cap1", ("n_nodes", 1)),
                      ("fv_index", _i32, 1, "cap", "n_valid")], 0, fill=dict(word_id=-1, node_id=-1), scalars=("n_short", "computed"), copy=True)
BOW_SIDE = _m.Inputs([("desc", _u8, (32,), REQ, "n"), ("node_id", _i32, (), REQ, "n"), ("has_map_point", bool, (), OPT, "n"), ("angle", _f32, (), OPT, "n")])


def _bow_out(cap):
    """an hvo_bow with room for `cap` features and the arrays behind it"""
    b = Bow(); b.cap = max(int(cap), 1)
    return b, BOW_OUT.alloc(b, cap=b.cap, cap1=b.cap + 1)


def _bow_finish(b, a):
    """dict(word_id, node_id per feature; bow_word, bow_value; fv_node, fv_start, fv_index; n_short, computed)"""
    d = BOW_OUT.finish(b, a, cap=b.cap, cap1=b.cap + 1); d["computed"] = bool(d["computed"])
    return d


def _bow_side(desc, node_id, has_map_point=None, angle=None):
    k = BowKeyframe()
    a, n = BOW_SIDE.fill(k, dict(desc=desc, node_id=node_id, has_map_point=has_map_point, angle=angle))
    if has_map_point is None: a["has_map_point"] = np.ones(n, np.uint8); k.has_map_point = _m.ptr(a["has_map_point"])     # every feature holds a map point
    if angle is None: a["angle"] = np.zeros(n, np.float32); k.angle = _m.ptr(a["angle"])
    return k, a


def _bow_search_args(n_frame, kfs, nnratio, check_orientation, th_low):
    """kfs: a list of dict(desc, node_id, has_map_point, angle) or of tuples in that order"""
    keep = []; K = (BowKeyframe * len(kfs))()
    for j, kf in enumerate(kfs):
        k, kp = _bow_side(**kf) if isinstance(kf, dict) else _bow_side(*kf)
        K[j] = k; keep.append(kp)
    P = BowSearchParams(float(nnratio), 1 if check_orientation else 0, int(th_low))
    R = (BowMatches * len(kfs))(); m = np.full((len(kfs), max(n_frame, 1)), -1, np.int32)
    for j in range(len(kfs)):
        R[j].match_kf = m[j].ctypes.data
    return K, P, R, m, keep


class PnpParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float), ("th2", C.c_float),
                ("seed", C.c_uint32), ("extra_iterations", C.c_int32), ("max_events", C.c_int32)]


class PnpProblem(C.Structure):
    _fields_ = [("p3d", C.c_void_p), ("p2d", C.c_void_p), ("sigma2", C.c_void_p), ("feature_index", C.c_void_p), ("n", C.c_int32), ("n_features", C.c_int32)]


class PnpEvent(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("n_inliers", C.c_int32), ("success", C.c_int32), ("hyp_n_inliers", C.c_int32), ("Tcw", C.c_float * 12), ("hyp_Tcw", C.c_float * 12),
                ("inliers", C.c_void_p), ("hyp_inliers", C.c_void_p)]


class PnpResult(C.Structure):
    _fields_ = [("cap_hyp", C.c_int32), ("cap_events", C.c_int32), ("hyp_inliers", C.c_void_p), ("hyp_event", C.c_void_p), ("hyp_sample", C.c_void_p),
                ("events", C.POINTER(PnpEvent)), ("best_inliers", C.c_void_p), ("best_Tcw", C.c_float * 12)] + \
               [(k, C.c_int32) for k in ("best_n_inliers", "best_valid", "best_iteration", "n", "n_features", "min_inliers", "max_its")] + [("epsilon", C.c_float)] + \
               [(k, C.c_int32) for k in ("n_hyp", "n_events", "no_more", "status")]


class PnpKeyframeSide(C.Structure):
    _fields_ = [("match_kf", C.c_void_p), ("pos", C.c_void_p), ("bad", C.c_void_p), ("n", C.c_int32)]


PNP_MAX_HYP = 1024


# ---- the relocalisation PnP: its result block stays written out (_pnp_results / _pnp_finish): the sentinel is a byte pattern read through three
# dtypes, hyp_sample's width is a parameter of the call, and the events are records whose two inlier rows are wired one by one
PNP_PROBLEM = _m.Inputs([("p3d", _f32, (3,), REQ, "n"), ("p2d", _f32, (2,), REQ, "n"), ("sigma2", _f32, (), REQ, "n"), ("feature_index", _i32, (), REQ, "n")],
                        differ="pnp_ransac: a problem's arrays differ in length")
PNP_KF_SIDE = _m.Inputs([("match_kf", _i32, (), REQ, None), ("pos", _f32, (3,), REQ, "n"), ("bad", bool, (), REQ, "n")],
                        differ="pnp_ransac: pos and bad differ in length")


def pnp_params(**kw):
    """hvo_pnp_default_params (SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), seed 1, 8 extra iterations, 8 events) with fields overridden"""
    P = PnpParams()
    lib().hvo_pnp_default_params(C.byref(P))
    for k, v in kw.items():
        if not hasattr(P, k):
            raise TypeError("unknown PnP parameter " + k)
        setattr(P, k, v)
    return P


PNP_SENTINEL = 0xA5                  # what the result arrays hold where the call writes nothing: past T, past n_events, past n_features


def _pnp_results(n_kf, n_features, P, want_sample, spare_events=0):
    """hvo_pnp_result x n_kf with their arrays: room for max_iterations + extra_iterations hypotheses (at most 1024) and max_events (+ spare_events)
    events, every byte PNP_SENTINEL (iteration = -99 in the event records) before the call"""
    cap = max(1, min(PNP_MAX_HYP, P.max_iterations + P.extra_iterations)); E = max(int(P.max_events), 1) + int(spare_events)
    sent32 = np.frombuffer(bytes([PNP_SENTINEL] * 4), np.int32)[0]
    R = (PnpResult * n_kf)(); keep = []
    for j in range(n_kf):
        nf = max(int(n_features[j]), 1)
        a = dict(hyp_inliers=np.full(cap, sent32, np.int32), hyp_event=np.full(cap, sent32, np.int32),
                 hyp_sample=np.full((cap, max(P.min_set, 1)), sent32, np.int32) if want_sample else None,
                 ev_inliers=np.full((E, nf), PNP_SENTINEL, np.uint8), ev_hyp_inliers=np.full((E, nf), PNP_SENTINEL, np.uint8),
                 best_inliers=np.full(nf, PNP_SENTINEL, np.uint8), events=(PnpEvent * E)())
        for e in range(E):
            a["events"][e].iteration = -99
            a["events"][e].inliers = a["ev_inliers"][e].ctypes.data; a["events"][e].hyp_inliers = a["ev_hyp_inliers"][e].ctypes.data
        R[j].cap_hyp = cap; R[j].cap_events = E
        R[j].hyp_inliers = a["hyp_inliers"].ctypes.data; R[j].hyp_event = a["hyp_event"].ctypes.data
        R[j].hyp_sample = a["hyp_sample"].ctypes.data if want_sample else None
        R[j].events = a["events"]; R[j].best_inliers = a["best_inliers"].ctypes.data
        keep.append(a)
    return R, keep


def _pnp_finish(R, keep, min_set):
    out = []
    for r, a in zip(R, keep):
        T, nf = r.n_hyp, r.n_features
        ev = [dict(iteration=a["events"][e].iteration, n_inliers=a["events"][e].n_inliers, success=bool(a["events"][e].success),
                   Tcw=np.array(a["events"][e].Tcw, np.float32), inliers=a["ev_inliers"][e, :nf].copy(), hyp_n_inliers=a["events"][e].hyp_n_inliers,
                   hyp_Tcw=np.array(a["events"][e].hyp_Tcw, np.float32), hyp_inliers=a["ev_hyp_inliers"][e, :nf].copy()) for e in range(r.n_events)]
        out.append(dict(N=r.n, n_features=nf, min_inliers=r.min_inliers, max_its=r.max_its, epsilon=np.float32(r.epsilon), T=T, no_more=bool(r.no_more), status=r.status,
                        hyp_inliers=a["hyp_inliers"][:T].copy(), hyp_event=a["hyp_event"][:T].copy(),
                        hyp_sample=None if a["hyp_sample"] is None else a["hyp_sample"][:T, :min_set].copy(), events=ev,
                        best_n_inliers=r.best_n_inliers, best_valid=bool(r.best_valid), best_iteration=r.best_iteration, best_Tcw=np.array(r.best_Tcw, np.float32),
                        best_inliers=a["best_inliers"][:nf].copy() if r.best_iteration > 0 else np.zeros(nf, np.uint8), raw=a))
    return out


def pnp_iterate(res, state, n_iterations):
    """PnPsolver::iterate(nIterations, bNoMore, vbInliers, nInliers) (src/PnPsolver.cc:165-258) replayed over one candidate's result `res`
    of pnp_ransac.  state: a dict that keeps mnIterations between calls (start with {}).  Returns (Tcw (12 floats) or None, bNoMore,
    vbInliers or None, nInliers).  A replay that would need a hypothesis past the T evaluated ones reports bNoMore."""
    it = state.get("mnIterations", 0)
    if res["N"] < res["min_inliers"]:
        return None, True, None, 0
    cur = 0
    while it < res["max_its"] or cur < n_iterations:
        cur += 1; it += 1
        state["mnIterations"] = it
        if it > res["T"]:
            return None, True, None, 0
        e = int(res["hyp_event"][it - 1])
        if e >= 0:
            ev = res["events"][e]
            return ev["Tcw"], False, ev["inliers"], ev["n_inliers"]
    state["mnIterations"] = it
    if it >= res["max_its"]:
        last = None                                              # the best after `it` iterations: the latest record at or before it
        for ev in res["events"]:
            if ev["iteration"] <= it:
                last = ev
        if last is not None:
            return last["hyp_Tcw"], True, last["hyp_inliers"], last["hyp_n_inliers"]
        return None, True, None, 0
    return None, False, None, 0


KF_SEARCH_MAX_ENTRIES, KF_SEARCH_MAX_FEATURES = 16384, 65535
KF_GATES = ("searched", "skip", "u < minX", "u > maxX", "v < minY", "v > maxY", "dist < 0.8 min", "dist > 1.2 max")     # hvo_kf_search_result.gate


class KfSearchCandidate(C.Structure):
    """hvo_kf_search_candidate: one candidate key frame's map points, the frame's pose for it and the frame's occupancy at entry"""
    _fields_ = [("n", C.c_int32), ("pos", C.c_void_p), ("skip", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("desc", C.c_void_p),
                ("angle", C.c_void_p), ("Tcw", C.c_float * 12), ("occupied", C.c_void_p)]


class KfSearchParams(C.Structure):
    """hvo_kf_search_params"""
    _fields_ = [("th", C.c_float), ("orb_dist", C.c_int32), ("check_orientation", C.c_int32), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("bounds", C.c_float * 4)]


class KfSearchResult(C.Structure):
    """hvo_kf_search_result"""
    _fields_ = [("match_idx", C.c_void_p), ("match_dist", C.c_void_p), ("feature_kf", C.c_void_p), ("proj", C.c_void_p), ("level", C.c_void_p),
                ("gate", C.c_void_p), ("n_matches", C.c_int32), ("n_searched", C.c_int32), ("status", C.c_int32), ("kernel_ms", C.c_float * 2)]

KF_UNTOUCHED = -7           # what the outputs hold before the call: a refusal leaves them so


# ---- SearchByProjection(Frame, KeyFrame): KF_UNTOUCHED before the call
KFS_IN = _m.Inputs([("pos", _f32, (3,), REQ, "n"), ("skip", _u8, (), REQ, "n"), ("max_dist", _f32, (), REQ, "n"), ("min_dist", _f32, (), REQ, "n"),
                    ("desc", _u8, (32,), REQ, "n"), ("angle", _f32, (), OPT, "n"), ("occupied", _u8, (), OPT, "n_frame")],
                   differ="search_by_projection_keyframe: a candidate's arrays differ in length")
KFS_OUT = _m.Outputs([_entry("match_idx", _i32), _entry("match_dist", _i32), _entry("feature_kf", _i32, 1, "n_frame"), _entry("proj", _f32, 2), _entry("level", _i32),
                      _entry("gate", _i8)], KF_UNTOUCHED, counts=("n_matches", "n_searched", "status"), scalars=("n_matches", "n_searched", "status", "kernel_ms"))


def _kfs_args(n_frame, kfs, bounds4, th, orb_dist, check_orientation, log_scale_factor, n_levels):
    """-> (KfSearchParams, candidates, results, the arrays they point at).  kfs: one dict per candidate with pos (n x 3), skip (n), max_dist,
    min_dist (n, raw), desc (n x 32), angle (n, or None), Tcw (3 x 4), occupied (frame features, or None)"""
    P = KfSearchParams(); P.th = th; P.orb_dist = orb_dist; P.check_orientation = 1 if check_orientation else 0
    P.log_scale_factor = log_scale_factor; P.n_levels = n_levels; _m.bounds(P.bounds, bounds4)
    K = (KfSearchCandidate * len(kfs))(); keep = []; lens = []
    for j, kf in enumerate(kfs):
        a, n = KFS_IN.fill(K[j], kf, n_frame=n_frame)      # (a candidate without entries passes NULL for all its arrays; the call reads nothing)
        _m.vec(K[j].Tcw, kf["Tcw"])
        keep.append(a); lens.append(dict(n=n, n_frame=n_frame))
    R, rk = _results(KFS_OUT, (KfSearchResult * len(kfs))(), lens)
    return P, K, R, (keep, rk)


def _kfs_finish(R, keep):
    """one dict per candidate, cut to its entries and the frame's features even after a refusal (every entry is then KF_UNTOUCHED)"""
    return _finished(KFS_OUT, R, keep[1], True)


FUSE_MAX_FEATURES, FUSE_MAX_ENTRIES = 65535, 1 << 20
FUSE_GATES = ("searched", "skip", "behind", "out of image", "dist < 0.8 min", "dist > 1.2 max", "view angle")     # hvo_fuse_result.gate
FUSE_UNTOUCHED = -7         # what the outputs hold before the call: a refusal leaves them so


class FuseKeyframe(C.Structure):
    """hvo_fuse_keyframe: a key frame's features, its pose and the skip bytes of its map entries"""
    _fields_ = [("n", C.c_int32), ("kp_un", C.c_void_p), ("uright", C.c_void_p), ("desc", C.c_void_p), ("Tcw", C.c_float * 12), ("skip", C.c_void_p)]


class FuseMap(C.Structure):
    """hvo_fuse_map: a map side on host arrays"""
    _fields_ = [("n", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("desc", C.c_void_p)]


class FuseParams(C.Structure):
    """hvo_fuse_params"""
    _fields_ = [("th", C.c_float), ("th_low", C.c_int32), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32), ("bf", C.c_float),
                ("bounds", C.c_float * 4), ("map_per_keyframe", C.c_int32)]


class FuseResult(C.Structure):
    """hvo_fuse_result"""
    _fields_ = [("best_idx", C.c_void_p), ("best_dist", C.c_void_p), ("gate", C.c_void_p), ("level", C.c_void_p), ("proj", C.c_void_p),
                ("fused_entry", C.c_void_p), ("fused_idx", C.c_void_p), ("n_fused", C.c_int32), ("n_searched", C.c_int32), ("status", C.c_int32),
                ("kernel_ms", C.c_float * 3)]

LF_MAX_LINES, LF_MAX_ENTRIES, LF_MAX_PAIRS = 2048, 65536, 1 << 24
LF_GATES = ("searched", "skip", "behind", "out of image", "dist < 0.8 min", "dist > 1.2 max", "view angle", "level")      # hvo_lf_result.gate
LF_LEVEL_RULES = ("clamped", "as written")                         # HVO_LF_LEVEL_*


class LfKeyframe(C.Structure):
    """hvo_lf_keyframe: a key frame's key lines, the rows its candidates are compared with, its pose, bounds, camera and skip bytes"""
    _fields_ = [("n", C.c_int32), ("kl", C.c_void_p), ("desc_rows", C.c_void_p), ("n_desc_rows", C.c_int32), ("Tcw", C.c_float * 12), ("bounds", C.c_float * 4),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("skip", C.c_void_p)]


class LfMap(C.Structure):
    """hvo_lf_map: a map side on host arrays"""
    _fields_ = [("n", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("desc", C.c_void_p)]


class LfParams(C.Structure):
    """hvo_lf_params"""
    _fields_ = [("th", C.c_float), ("th_low", C.c_int32), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32), ("scale_factor", C.c_float),
                ("level_rule", C.c_int32), ("map_per_keyframe", C.c_int32)]


class LfResult(C.Structure):
    """hvo_lf_result"""
    _fields_ = [("best_idx", C.c_void_p), ("best_dist", C.c_void_p), ("gate", C.c_void_p), ("level", C.c_void_p), ("proj", C.c_void_p),
                ("fused_entry", C.c_void_p), ("fused_idx", C.c_void_p), ("behind_entry", C.c_void_p), ("n_fused", C.c_int32), ("n_behind", C.c_int32),
                ("n_searched", C.c_int32), ("status", C.c_int32), ("kernel_ms", C.c_float * 3)]

# ---- Fuse, points and lines: FUSE_UNTOUCHED before the call, whole arrays after a refusal
def _fuse_out(proj_cols, lists, counts):
    return _m.Outputs([_entry("best_idx", _i32), _entry("best_dist", _i32), _entry("gate", _i8), _entry("level", _i32), _entry("proj", _f32, proj_cols)] +
                      [(f, _i32, 1, "n", c) for f, c in lists], FUSE_UNTOUCHED, counts=counts, scalars=counts + ("kernel_ms",))


FUSE_OUT = _fuse_out(3, (("fused_entry", "n_fused"), ("fused_idx", "n_fused")), ("n_fused", "n_searched", "status"))
LF_OUT = _fuse_out(4, (("fused_entry", "n_fused"), ("fused_idx", "n_fused"), ("behind_entry", "n_behind")), ("n_fused", "n_behind", "n_searched", "status"))
FUSE_MAP = _m.Inputs([("pos", _f32, (3,), REQ, "n"), ("normal", _f32, (3,), REQ, "n"), ("max_dist", _f32, (), REQ, "n"), ("min_dist", _f32, (), REQ, "n"),
                      ("desc", _u8, (32,), REQ, "n")], differ="fuse_points: a map side's arrays differ in length")
LF_MAP = _m.Inputs([("pos", _f64, (6,), REQ, "n"), ("normal", _f64, (3,), REQ, "n"), ("max_distance", _f32, (), REQ, "n"), ("min_distance", _f32, (), REQ, "n"),
                    ("desc", _u8, (32,), REQ, "n")], differ="fuse_lines: a map side's arrays differ in length")
FUSE_KF = _m.Inputs([("kp_un", KEYPOINT_DT, (), REQ, "n"), ("desc", _u8, (32,), REQ, "n"), ("uright", _f32, (), OPT, "n"), ("skip", bool, (), OPT, "entries")])
LF_KF = _m.Inputs([("kl", KEYLINE_DT, (), OPT, None), ("desc_rows", _u8, (32,), OPT, None), ("skip", bool, (), OPT, "entries")], count_from="kl")


def _fuse_params(cam, bounds4, th, th_low, log_scale_factor, n_levels, per_keyframe):
    P = FuseParams(); P.th = th; P.th_low = th_low; P.log_scale_factor = log_scale_factor; P.n_levels = n_levels; P.bf = float(cam[4])
    _m.bounds(P.bounds, bounds4); P.map_per_keyframe = 1 if per_keyframe else 0
    return P


def _lf_params(th, th_low, log_scale_factor, n_levels, scale_factor, level_rule, per_keyframe):
    P = LfParams(); P.th = th; P.th_low = th_low; P.log_scale_factor = log_scale_factor; P.n_levels = n_levels; P.scale_factor = scale_factor
    P.level_rule = LF_LEVEL_RULES.index(level_rule) if isinstance(level_rule, str) else int(level_rule)
    P.map_per_keyframe = 1 if per_keyframe else 0
    return P


def _map_sides(table, M, maps):
    """the map sides (dicts of the table's arrays) -> (the records M, the arrays, the entries of each)"""
    keep = [table.fill(M[s], mp)[0] for s, mp in enumerate(maps)]
    return M, keep, [M[s].n for s in range(len(maps))]


def _lf_maps(maps):
    """dicts of pos (n x 6 doubles), normal (n x 3 doubles), max_distance, min_distance (n, raw), desc (n x 32)"""
    return _map_sides(LF_MAP, (LfMap * len(maps))(), maps)


def _fuse_keyframes(kfs, n_entries, resident=False):
    """kfs: dicts of kp_un, uright (or None), desc, Tcw, skip (or None); n_entries[j]: the entries of key frame j's map side.  resident: the
    features are the resident frame's, only skip and Tcw are read"""
    K = (FuseKeyframe * len(kfs))(); keep = []
    for j, kf in enumerate(kfs):
        keep.append(FUSE_KF.fill(K[j], kf, only=("skip",) if resident else None, entries=n_entries[j])[0])
        _m.vec(K[j].Tcw, kf["Tcw"])
    return K, keep


def _lf_keyframes(kfs, n_entries, resident=False):
    """kfs: dicts of kl, desc_rows, Tcw, cam (fx, fy, cx, cy), bounds, skip (or None); n_entries[j]: the entries of key frame j's map side"""
    K = (LfKeyframe * len(kfs))(); keep = []
    for j, kf in enumerate(kfs):
        # (an array given as None with a count "n" / "n_desc_rows" beside it reaches the library as a missing array: its refusal is tested)
        a, _ = LF_KF.fill(K[j], kf, n=int(kf.get("n", 0)) if kf.get("kl") is None else None, only=("skip",) if resident else None, entries=n_entries[j])
        if not resident:
            K[j].n_desc_rows = len(a["desc_rows"]) if a["desc_rows"] is not None else int(kf.get("n_desc_rows", 0))
            _m.vec(K[j].bounds, kf["bounds"])
            K[j].fx, K[j].fy, K[j].cx, K[j].cy = (float(v) for v in kf["cam"][:4])
        _m.vec(K[j].Tcw, kf["Tcw"])
        keep.append(a)
    return K, keep


class _FuseFamily:
    """what fuse_points and fuse_lines differ in: the records, their tables and the key-frame builder"""
    def __init__(self, name, Map, Result, map_in, out, keyframes):
        self.name, self.Map, self.Result, self.map_in, self.out, self.keyframes = name, Map, Result, map_in, out, keyframes

    def build(self, kfs, maps=None, slots=None, resident=False):
        """the arguments the three forms of a fuse call share.  maps: ONE dict for all key frames or a list with one per key frame; else slots
        of a resident map -> (key frames K, map sides M or None, slot array or None, per_keyframe, results R, finish(ok), what must stay alive)"""
        per_kf = maps is not None and not isinstance(maps, dict)
        if per_kf and len(maps) != len(kfs):
            raise ValueError("%s: one map side per key frame, or one dict for all" % self.name)
        if maps is not None:
            sides = list(maps) if per_kf else [maps]
            M, mk, ns = _map_sides(self.map_in, (self.Map * len(sides))(), sides); sl = None
            ne = ns if per_kf else ns * len(kfs)
        else:
            M = mk = None; sl = np.ascontiguousarray(slots, np.int32).reshape(-1); ne = [len(sl)] * len(kfs)
        K, kk = self.keyframes(kfs, ne, resident)
        R, rk = _results(self.out, (self.Result * len(ne))(), [dict(n=n) for n in ne])
        return K, M, sl, per_kf, R, lambda ok: _finished(self.out, R, rk, ok), (mk, kk)


_FUSE = _FuseFamily("fuse_points", FuseMap, FuseResult, FUSE_MAP, FUSE_OUT, _fuse_keyframes)
_LF = _FuseFamily("fuse_lines", LfMap, LfResult, LF_MAP, LF_OUT, _lf_keyframes)


NP_MAX_FEATURES, NP_MAX_NEIGHBOURS = 4096, 64
NP_OUTCOMES = ("created", "occupied", "no match", "low parallax", "w == 0", "no depth", "behind 1", "behind 2", "reproj 1", "reproj 2", "zero dist", "scale")
NP_UNTOUCHED = -7           # what the outputs hold before the call: a refusal leaves them so


class NpKeyframe(C.Structure):
    """hvo_np_keyframe: the current key frame, and each neighbour"""
    _fields_ = [("n", C.c_int32), ("kp_un", C.c_void_p), ("kp", C.c_void_p), ("uright", C.c_void_p), ("depth", C.c_void_p), ("desc", C.c_void_p),
                ("node_id", C.c_void_p), ("has_map_point", C.c_void_p), ("Tcw", C.c_float * 12), ("mb", C.c_float), ("skip", C.c_uint8)]


class NpParams(C.Structure):
    """hvo_np_params"""
    _fields_ = [("th_low", C.c_int32), ("n_levels", C.c_int32), ("scale_factor", C.c_float), ("bf", C.c_float)]


class NpResult(C.Structure):
    """hvo_np_result"""
    _fields_ = [("match_idx2", C.c_void_p), ("match_dist", C.c_void_p), ("outcome", C.c_void_p), ("branch", C.c_void_p), ("x3d", C.c_void_p),
                ("created_idx1", C.c_void_p), ("created_idx2", C.c_void_p), ("n_created", C.c_int32), ("gate", C.c_int32), ("status", C.c_int32)]


class NpSummary(C.Structure):
    """hvo_np_summary"""
    _fields_ = [("owner", C.c_void_p), ("n_new", C.c_int32), ("kernel_ms", C.c_float * 3)]

NL_MAX_LINES, NL_MAX_NEIGHBOURS = 2048, 16
NL_PAIR_AS_WRITTEN, NL_PAIR_ALIGNED = 0, 1
NL_OUTCOMES = ("created", "no match", "idx range", "occupied 1", "occupied 2", "occupied 3", "bad octave", "epipolar parallel", "norm zero 23", "norm zero 1",
               "not coplanar", "w == 0 start", "w == 0 end", "parallax start", "parallax end", "ratio 1", "ratio 2", "ratio 3",
               "behind 1s", "behind 1e", "behind 2s", "behind 2e", "behind 3s", "behind 3e", "reproj 1s", "reproj 1e", "reproj 2s", "reproj 2e", "reproj 3s", "reproj 3e",
               "disjoint 1", "overlap 1", "disjoint 2", "overlap 2", "disjoint 3", "overlap 3")
NL_UNTOUCHED = -7           # what the outputs hold before the call: a refusal leaves them so


class NlKeyframe(C.Structure):
    """hvo_nl_keyframe: the current key frame, and each neighbour"""
    _fields_ = [("n", C.c_int32), ("kl", C.c_void_p), ("linefn", C.c_void_p), ("desc", C.c_void_p), ("has_map_line", C.c_void_p), ("Tcw", C.c_float * 12),
                ("cam", C.c_float * 6), ("mb", C.c_float), ("median_depth", C.c_float), ("skip", C.c_uint8)]


class NlParams(C.Structure):
    """hvo_nl_params"""
    _fields_ = [("th_high", C.c_int32), ("nn_ratio", C.c_float), ("n_levels", C.c_int32), ("scale_factor", C.c_float), ("pairing", C.c_int32)]


class NlMatch(C.Structure):
    """hvo_nl_match"""
    _fields_ = [("match_idx", C.c_void_p), ("n_matched", C.c_int32), ("gate", C.c_int32)]


class NlResult(C.Structure):
    """hvo_nl_result"""
    _fields_ = [("kf2", C.c_int32), ("kf3", C.c_int32), ("mv2", C.c_int32), ("mv3", C.c_int32), ("outcome", C.c_void_p), ("line3d", C.c_void_p),
                ("created_idx0", C.c_void_p), ("created_idx1", C.c_void_p), ("created_idx2", C.c_void_p), ("n_created", C.c_int32), ("status", C.c_int32)]


class NlSummary(C.Structure):
    """hvo_nl_summary"""
    _fields_ = [("owner_pair", C.c_void_p), ("n_new", C.c_int32), ("n_pairs", C.c_int32), ("kernel_ms", C.c_float * 3)]

# ---- CreateNewMapPoints / CreateNewMapLinesConstraint: NP_UNTOUCHED / NL_UNTOUCHED before the call, whole arrays after a refusal.  A key
# frame's arrays may all be missing (they stay NULL and are the library's to refuse) and an explicit "n" beside them is honoured
NP_KF = _m.Inputs([("kp_un", KEYPOINT_DT, (), OPT, None), ("kp", KEYPOINT_DT, (), OPT, None), ("uright", _f32, (), OPT, None), ("depth", _f32, (), OPT, None),
                   ("node_id", _i32, (), OPT, None), ("desc", _u8, (32,), OPT, None), ("has_map_point", bool, (), OPT, None)], count_from="kp_un")
NP_OUT = _m.Outputs([_entry("match_idx2", _i32), _entry("match_dist", _i32), _entry("outcome", _i8), _entry("branch", _i8), _entry("x3d", _f32, 3),
                     ("created_idx1", _i32, 1, "n", "n_created"), ("created_idx2", _i32, 1, "n", "n_created")], NP_UNTOUCHED,
                    counts=("n_created", "gate", "status"), scalars=("n_created", "gate", "status"))
NP_SUMMARY = _m.Outputs([_entry("owner", _i32)], NP_UNTOUCHED, counts=("n_new",), scalars=("n_new", "kernel_ms"))
NL_KF = _m.Inputs([("kl", KEYLINE_DT, (), OPT, None), ("linefn", _f64, (3,), OPT, None), ("desc", _u8, (32,), OPT, None), ("has_map_line", bool, (), OPT, None)],
                  count_from="kl")
NL_MATCH = _m.Outputs([_entry("match_idx", _i32)], NL_UNTOUCHED, counts=("n_matched", "gate"), scalars=("n_matched", "gate"))
NL_OUT = _m.Outputs([_entry("outcome", _i8), _entry("line3d", _f32, 6)] + [("created_idx%d" % k, _i32, 1, "n", "n_created") for k in range(3)], NL_UNTOUCHED,
                    counts=("kf2", "kf3", "mv2", "mv3", "n_created", "status"), scalars=("kf2", "kf3", "mv2", "mv3", "n_created", "status"))
NL_SUMMARY = _m.Outputs([_entry("owner_pair", _i32)], NL_UNTOUCHED, counts=("n_new", "n_pairs"), scalars=("n_new", "n_pairs", "kernel_ms"))


def _np_keyframe(K, kf, resident=False):
    """kf: dict of kp_un, kp (or None), uright, depth (both or None), desc, node_id, has_map_point, Tcw, mb, skip.  resident: only
    has_map_point, Tcw and mb are read"""
    a, _ = NP_KF.fill(K, kf, n=int(kf["n"]) if "n" in kf else None, only=("has_map_point",) if resident else None)
    _m.vec(K.Tcw, kf["Tcw"])
    K.mb = float(kf.get("mb", 0.0)); K.skip = 1 if kf.get("skip") else 0
    return a


def _np_args(m, kfs, th_low, n_levels, scale_factor, bf):
    """room for m features per neighbour -> (K, R, S, P, finish(n1) -> what _ret calls, what must stay alive).  finish(n1)(ok): (one dict per
    neighbour, the summary), cut to the n1 features the caller named"""
    nk = len(kfs)
    K = (NpKeyframe * max(nk, 1))(); R = (NpResult * max(nk, 1))()
    keep = [_np_keyframe(K[j], kf) for j, kf in enumerate(kfs)]
    outs = [NP_OUT.alloc(R[j], n=m) for j in range(nk)]
    S = NpSummary(); owner = NP_SUMMARY.alloc(S, n=m)
    P = NpParams(); P.th_low = th_low; P.n_levels = n_levels; P.scale_factor = scale_factor; P.bf = bf
    finish = lambda n1: lambda ok: ([NP_OUT.finish(R[j], o, ok, n=n1) for j, o in enumerate(outs)], NP_SUMMARY.finish(S, owner, ok, n=n1))
    return K, R, S, P, finish, keep


def _nl_keyframe(K, kf, resident=False):
    """kf: dict of kl, linefn, desc, has_map_line, Tcw, cam (fx, fy, cx, cy), mb, median_depth, skip.  resident: only has_map_line, Tcw and cam
    are read"""
    a, _ = NL_KF.fill(K, kf, n=int(kf["n"]) if "n" in kf else None, only=("has_map_line",) if resident else None)
    _m.vec(K.Tcw, kf["Tcw"]); _m.vec(K.cam, kf["cam"], 4)
    K.mb = float(kf.get("mb", 0.0)); K.median_depth = float(kf.get("median_depth", 1.0)); K.skip = 1 if kf.get("skip") else 0
    return a


def _nl_args(m, kfs, th_high, nn_ratio, n_levels, scale_factor, pairing, n_pairs_cap):
    """room for m lines per neighbour and per pair -> (K, M, R, S, P, the pair capacity, finish(n1), what must stay alive).  finish(n1)(ok):
    (one dict per neighbour, one per pair, the summary); after a refusal every result record the caller made room for is listed"""
    nk = len(kfs); cap = nk * (nk - 1) // 2 if n_pairs_cap is None else int(n_pairs_cap)
    K = (NlKeyframe * max(nk, 1))(); M = (NlMatch * max(nk, 1))(); R = (NlResult * max(cap, 1))()
    keep = [_nl_keyframe(K[j], kf) for j, kf in enumerate(kfs)]
    mouts = [NL_MATCH.alloc(M[j], n=m) for j in range(nk)]
    outs = [NL_OUT.alloc(R[p], n=m) for p in range(cap)]
    S = NlSummary(); owner = NL_SUMMARY.alloc(S, n=m)
    P = NlParams(); P.th_high = th_high; P.nn_ratio = nn_ratio; P.n_levels = n_levels; P.scale_factor = scale_factor; P.pairing = pairing

    def finish(n1):
        return lambda ok: ([NL_MATCH.finish(M[j], mo, ok, n=n1) for j, mo in enumerate(mouts)],
                           [NL_OUT.finish(R[p], o, ok, n=n1) for p, o in enumerate(outs[:max(S.n_pairs, 0)] if ok else outs)],
                           NL_SUMMARY.finish(S, owner, ok, n=n1))
    return K, M, R, S, P, cap, finish, keep


MR_DESCRIPTOR, MR_GEOMETRY = 1, 2
MR_MAX_OBS, MR_MAX_FEATURES, MR_MAX_OBS_TOTAL = 256, 65536, 1 << 20
MR_REFRESHED, MR_SKIPPED, MR_NO_OBS, MR_DESC_KEPT, MR_BAD_LEVEL = range(5)
MR_STATUS = ("refreshed", "skipped", "no observations", "descriptor kept", "bad level")
MR_UNTOUCHED = 119          # what the outputs hold before the call: an entry that is not written stays so


class MrParams(C.Structure):
    """hvo_mr_params"""
    _fields_ = [("n_levels", C.c_int32), ("scale_factor", C.c_float), ("what", C.c_int32)]


class MrInput(C.Structure):
    """hvo_mr_input"""
    _fields_ = [("n", C.c_int32), ("obs_start", C.c_void_p), ("obs_desc", C.c_void_p), ("obs_Ow", C.c_void_p), ("kf_bad", C.c_void_p), ("ref_Ow", C.c_void_p),
                ("ref_level", C.c_void_p), ("skip", C.c_void_p)]


class MrPointOut(C.Structure):
    """hvo_mr_point_out"""
    _fields_ = [("best_obs", C.c_void_p), ("best_median", C.c_void_p), ("desc", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p),
                ("status", C.c_void_p), ("kernel_ms", C.c_float)]


class MrLineOut(C.Structure):
    """hvo_mr_line_out"""
    _fields_ = [("best_obs", C.c_void_p), ("best_median", C.c_void_p), ("desc", C.c_void_p), ("normal", C.c_void_p), ("wvec", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("status", C.c_void_p), ("kernel_ms", C.c_float)]

# ---- the map refresh: MR_UNTOUCHED before the call; every input may be missing (NULL, the library's to refuse)
MR_IN = _m.Inputs([("obs_start", _i32, (), REQ, None), ("obs_desc", _u8, (32,), OPT, None), ("obs_Ow", _f32, (3,), OPT, None), ("kf_bad", bool, (), OPT, None),
                   ("ref_Ow", _f32, (3,), OPT, None), ("ref_level", _i32, (), OPT, None), ("skip", bool, (), OPT, None)], count=None)
MR_OUT = tuple(_m.Outputs([_entry("best_obs", _i32), _entry("best_median", _i32), _entry("desc", _u8, 32), _entry("normal", rdt, 3), _entry("max_dist", _f32),
                           _entry("min_dist", _f32), _entry("status", _u8)] + more, MR_UNTOUCHED, scalars=("kernel_ms",))
               for rdt, more in ((_f32, []), (_f64, [_entry("wvec", _f64, 3)])))            # [line]: points, lines


def map_refresh_check(obs_start):
    """the limits of one refresh call, refused here as the library refuses them (HvoError, HVO_ERR_UNSUPPORTED): needs no device"""
    st = np.asarray(obs_start, np.int64).reshape(-1)
    n = len(st) - 1
    if n > MR_MAX_FEATURES:
        raise HvoError(-4, "map refresh: %d features (limit %d)" % (n, MR_MAX_FEATURES))
    if n > 0:
        most = int(np.diff(st).max())
        if most > MR_MAX_OBS:
            raise HvoError(-4, "map refresh: %d observations of one feature (limit %d)" % (most, MR_MAX_OBS))
        if int(st[-1]) > MR_MAX_OBS_TOTAL:
            raise HvoError(-4, "map refresh: %d observations (limit %d)" % (int(st[-1]), MR_MAX_OBS_TOTAL))


def _mr_args(line, obs_start, obs_desc, obs_Ow, ref_Ow, ref_level, kf_bad, skip, n_levels, scale_factor, what, want):
    """(params, input, output struct, the output arrays, n, what must stay alive).  want: the outputs to hand to the call; the others are
    passed as NULL, and their arrays come back untouched"""
    I = MrInput()
    a, _ = MR_IN.fill(I, dict(obs_start=obs_start, obs_desc=obs_desc, obs_Ow=obs_Ow, kf_bad=kf_bad, ref_Ow=ref_Ow, ref_level=ref_level, skip=skip))
    n = I.n = max(len(a["obs_start"]) - 1, 0)
    O = MrLineOut() if line else MrPointOut()
    o = MR_OUT[line].alloc(O, want, n=n)
    P = MrParams(); P.n_levels = n_levels; P.scale_factor = scale_factor; P.what = what
    return P, I, O, o, n, a


def _mr_call(ctx, name, line, pre, post, obs, n_levels, scale_factor, what, want, check):
    map_refresh_check(obs["obs_start"])
    P, I, O, o, n, keep = _mr_args(line, obs["obs_start"], obs.get("obs_desc"), obs.get("obs_Ow"), obs.get("ref_Ow"), obs.get("ref_level"), obs.get("kf_bad"),
                                   obs.get("skip"), n_levels, scale_factor, what, want)
    rc = getattr(lib(), name)(ctx.h, *pre, C.addressof(P), C.addressof(I), *post, C.addressof(O))
    del keep
    return _ret(ctx, rc, name[4:], lambda ok: MR_OUT[line].finish(O, o, n=n), check)


def line_struct_params(**kw):
    """the reference's values (hvo_line_struct_default_params) with the given fields replaced (mode, row_rule, ...)"""
    p = LineStructParams()
    lib().hvo_line_struct_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "chi2_round": p.chi2_round[0], p.chi2_round[1] = v
        else: setattr(p, k, v)
    return p


def _ls_params(params, mode, row_rule):
    p = line_struct_params() if params is None else (params if isinstance(params, LineStructParams) else line_struct_params(**params))
    if mode is not None: p.mode = mode
    if row_rule is not None: p.row_rule = row_rule
    return p


def rel_lists(rel_row):
    """(mvParLinesIdx[k], mvPerpLinesIdx[k]) of one row of the relation matrix: partner indices in ascending order, -1 where LineOptStruct
    rejected the constraint (the slot is kept)"""
    r = np.asarray(rel_row)
    ip, iq = np.nonzero(np.abs(r) == 1)[0], np.nonzero(np.abs(r) == 2)[0]
    return np.where(r[ip] > 0, ip, -1).tolist(), np.where(r[iq] > 0, iq, -1).tolist()


def _pose_problem(Tcw, kp_un=None, uright=None, inv_sigma2=None, linefn=None, lines3d=None, plane_coef=None,
                  pt_has=None, pt_xyz=None, ln_has=None, ln_xyz=None, pl_has=None, pl_coef_w=None, counts=None, plane_map=None, plane_match=None):
    """(PoseProblem, PoseFlags, the arrays that must stay alive).  counts = (n_points, n_lines, n_planes) when the frame side is resident.
    plane_map + plane_match (a PlaneMatch, or a dict with match / parallel / vertical slot arrays): the plane side as slots of a PlaneMap."""
    keep = {}
    def arr(k, a, dt, shape):
        if a is None: return None
        keep[k] = np.ascontiguousarray(a, dt).reshape(shape); return keep[k]
    kp = arr("kp_un", kp_un, KEYPOINT_DT, -1); fn = arr("linefn", linefn, np.float64, (-1, 3)); pc = arr("plane_coef", plane_coef, np.float32, (-1, 4))
    px = arr("pt_xyz", pt_xyz, np.float32, (-1, 3)); lx = arr("ln_xyz", ln_xyz, np.float64, (-1, 6)); pw = arr("pl_coef_w", pl_coef_w, np.float32, (-1, 3, 4))
    n = counts[0] if counts else (0 if kp is None else len(kp))
    nl = counts[1] if counts else (0 if fn is None else len(fn))
    m = counts[2] if counts else (0 if pc is None else len(pc))
    arr("uright", uright, np.float32, n); arr("inv_sigma2", inv_sigma2, np.float32, n); arr("lines3d", lines3d, LINE3D_DT, nl)
    if n and px is None: raise ValueError("pt_xyz is needed with points")
    keep["pt_has"] = np.ones(n, np.uint8) if pt_has is None else np.ascontiguousarray(pt_has, np.uint8).reshape(n)
    keep["ln_has"] = np.ones(nl, np.uint8) if ln_has is None else np.ascontiguousarray(ln_has, np.uint8).reshape(nl)
    keep["pl_has"] = (np.ones((m, 3), np.uint8) if pw is not None else np.zeros((m, 3), np.uint8)) if pl_has is None else np.ascontiguousarray(pl_has, np.uint8).reshape(m, 3)
    if pw is None: keep["pl_coef_w"] = np.zeros((m, 3, 4), np.float32)
    if px is None: keep["pt_xyz"] = np.zeros((n, 3), np.float32)
    if lx is None: keep["ln_xyz"] = np.zeros((nl, 6), np.float64)
    for k, cnt in (("pt_xyz", n), ("ln_xyz", nl), ("pl_coef_w", m)):
        if len(keep[k]) != cnt: raise ValueError("%s: %d rows for %d features" % (k, len(keep[k]), cnt))
    P = PoseProblem()
    P.Tcw[:] = np.ascontiguousarray(Tcw, np.float32).reshape(12).tolist()
    P.n_points, P.n_lines, P.n_planes = n, nl, m
    if plane_map is not None:
        g = (lambda k: plane_match[k]) if isinstance(plane_match, dict) else (lambda k: getattr(plane_match, k))
        for k in ("match", "parallel", "vertical"):
            keep["slot_" + k] = np.ascontiguousarray(np.array(g(k), np.int32)[:m]) if m else np.zeros(0, np.int32)
        P.plane_map = plane_map.h
        keep["pl_has"] = np.stack([keep["slot_" + k] >= 0 for k in ("match", "parallel", "vertical")], axis=1).astype(np.uint8).reshape(m, 3)
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data if a.size else None)
    fl = dict(pt_outlier=np.zeros(n, np.uint8), ln_outlier=np.zeros(nl, np.uint8), pl_outlier=np.zeros((m, 3), np.uint8), vp_outlier=np.zeros(nl, np.uint8))
    F = PoseFlags()
    for k, a in fl.items():
        setattr(F, k, a.ctypes.data if a.size else None)
    return P, F, keep, fl


def _pose_cam(cam):
    c = PoseCamera()
    c.fx, c.fy, c.cx, c.cy, c.bf = [float(v) for v in cam[:5]]
    c.b = float(cam[5]) if len(cam) > 5 else 0.0
    return c


def _pose_pp(pp):
    if pp is None: return None
    return C.byref(pp if isinstance(pp, PosePlaneParams) else PosePlaneParams(**pp))


def _th_arg(th):
    return None if th is None else np.ascontiguousarray(th, np.float32).reshape(4)


def _normals_arg(normals):
    """SURFACE_NORMAL_DT array, or (N, 3) floats taken as the normals"""
    a = np.asarray(normals)
    if a.dtype == SURFACE_NORMAL_DT:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.asarray(a, np.float32).reshape(-1, 3)
    out = np.zeros(len(a), SURFACE_NORMAL_DT); out["normal"] = a
    return out


def _tail_buffers(kp_cap, kl_cap, w, h):
    """numpy result arrays of one frame's tail stages + the FrameTail that points at them"""
    cc = C.c_int(0); nn = C.c_int(0); lc = C.c_int(0)
    lib().hvo_tail_capacity(kl_cap, w, h, C.byref(cc), C.byref(nn), C.byref(lc))
    b = dict(lines3d=np.zeros(kl_cap, LINE3D_DT), vp=VpResult(), vp_idx=np.full(kl_cap, 3, np.int32), plane_clouds=np.zeros(64, PLANE_CLOUD_DT),
             cloud_xyz=np.zeros((cc.value, 3), np.float32), normals=np.zeros(max(nn.value, 1), SURFACE_NORMAL_DT),
             pt_cell_start=np.zeros(64 * 48 + 1, np.int32), pt_cell_items=np.zeros(max(kp_cap, 1), np.int32),
             ln_cell_start=np.zeros(64 * 48 + 1, np.int32), ln_cell_items=np.zeros(max(lc.value, 1), np.int32))
    t = FrameTail()
    t.lines3d = b["lines3d"].ctypes.data; t.vp = C.addressof(b["vp"]); t.vp_idx = b["vp_idx"].ctypes.data
    t.plane_clouds = b["plane_clouds"].ctypes.data; t.cloud_xyz = b["cloud_xyz"].ctypes.data; t.cloud_cap = cc.value
    t.normals = b["normals"].ctypes.data; t.normals_cap = nn.value
    t.pt_cell_start = b["pt_cell_start"].ctypes.data; t.pt_cell_items = b["pt_cell_items"].ctypes.data; t.pt_items_cap = kp_cap
    t.ln_cell_start = b["ln_cell_start"].ctypes.data; t.ln_cell_items = b["ln_cell_items"].ctypes.data; t.ln_items_cap = lc.value
    return b, t


def _tail_result(b, t, n_kl, n_planes, stages):
    r = {"tail_status": t.status}
    if stages & STAGE_LINES3D: r["lines3d"] = b["lines3d"][:n_kl]
    if stages & STAGE_VP:
        v = b["vp"]
        r["vp"] = dict(vps=np.array([[v.vps[i][j] for j in range(3)] for i in range(3)]), score=v.score, best=v.best, n_hypotheses=v.n_hypotheses, vp_idx=b["vp_idx"][:n_kl])
    if stages & STAGE_PLANE_TAIL:
        r["plane_clouds"] = b["plane_clouds"][:n_planes]; r["cloud_xyz"] = b["cloud_xyz"][: t.n_cloud]; r["normals"] = b["normals"][: t.n_normals]
    if stages & STAGE_GRIDS:
        r["pt_grid"] = (b["pt_cell_start"], b["pt_cell_items"][: t.n_pt_items]); r["ln_grid"] = (b["ln_cell_start"], b["ln_cell_items"][: t.n_ln_items])
    return r
def build(force=False):
    """compile libhvo.so in-tree with hipcc --offload-arch=gfx950 (cross-compiles without a GPU)"""
    if force:
        subprocess.check_call(["make", "-s", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", _CSRC])


def torch_order_check():
    """raise if libhvo.so was loaded into this process before torch (see _LOADED_BEFORE_TORCH): `import torch` must come first
    in every process that shares device memory between the two (dist.device_slabs, dist.gather_device_slabs, bench.py --gpus N)"""
    if _LIB is not None and _LOADED_BEFORE_TORCH:
        raise RuntimeError("libhvo.so was loaded before torch in this process: torch.cuda cannot be initialised on top of it. "
                           "Import torch (and call torch.cuda.init()) BEFORE the first hvo call in processes that use hvo_amd.dist.")


# argtypes / restype of every hvo_* function the binding calls, applied once by lib(); name -> (restype, argtypes)
SIGNATURES = {
    "hvo_strerror": (C.c_char_p, [C.c_int]),
    "hvo_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_default_params": (None, [C.POINTER(Params)]),
    "hvo_create": (C.c_int, [C.POINTER(Params), C.POINTER(C.c_void_p)]),
    "hvo_destroy": (None, [C.c_void_p]),
    "hvo_extract_orb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_extract_lsd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_compute_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_hamming_matrix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "hvo_hamming_knn2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hvo_match_nnr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_search_by_projection": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p] * 4 + [C.c_int] + [C.c_float] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_frame_bf_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_match_lines_geom": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_search_lines_by_projection": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_stream_match_lines_geom": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hvo_stream_search_lines_by_projection": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_pose_optimize": (C.c_int, [C.c_void_p, C.POINTER(PoseCamera), C.c_void_p, C.c_int, C.POINTER(PoseProblem), C.POINTER(PoseResult), C.POINTER(PoseFlags)]),
    "hvo_pose_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hvo_stream_pose_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_float)]),
    "hvo_stream_pose_optimize": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(PoseProblem), C.POINTER(PoseResult), C.POINTER(PoseFlags)]),
    "hvo_line_struct_default_params": (C.c_int, [C.POINTER(LineStructParams)]),
    "hvo_line_struct_optimize": (C.c_int, [C.c_void_p, C.POINTER(LineStructParams), C.c_int, C.POINTER(LineStructProblem), C.c_void_p, C.c_void_p, C.POINTER(LineOptResult)]),
    "hvo_batch_line_struct_optimize": (C.c_int, [C.c_void_p, C.POINTER(LineStructParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LineOptResult)]),
    "hvo_stream_line_struct_optimize": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(LineStructParams), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(LineOptResult)]),
    "hvo_line_opt_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hvo_stream_line_opt_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_float)]),
    "hvo_track_manhattan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MfResult), C.c_void_p, C.c_void_p]),
    "hvo_stream_track_manhattan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(MfResult), C.c_void_p, C.c_void_p]),
    "hvo_batch_track_manhattan": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hvo_plane_map_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int64]),
    "hvo_plane_map_destroy": (None, [C.c_void_p]),
    "hvo_plane_map_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "hvo_plane_map_set_bad": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hvo_plane_map_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "hvo_plane_map_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hvo_plane_map_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_match_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PlaneMatch), C.c_void_p, C.c_void_p]),
    "hvo_stream_match_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(PlaneMatch)]),
    "hvo_batch_match_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvo_update_map_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PlaneUpdate), C.POINTER(PlaneUpdateResult)]),
    "hvo_stream_update_map_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(PlaneUpdate), C.POINTER(PlaneUpdateResult)]),
    "hvo_plane_map_get_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_plane_update_transform": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hvo_local_ba_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "hvo_local_ba_destroy": (None, [C.c_void_p]),
    "hvo_local_ba_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_local_ba_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hvo_local_ba_last_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_float * 4), C.POINTER(C.c_int32 * 2)]),
    "hvo_local_ba_default_params": (None, [C.POINTER(LocalBAParams)]),
    "hvo_local_ba_optimize": (C.c_int, [C.c_void_p, C.POINTER(LocalBAParams), C.POINTER(LocalBAGraph), C.c_void_p, C.POINTER(LocalBAResult)]),
    "hvo_line_map_create": (C.c_void_p, [C.c_int, C.c_int]),
    "hvo_line_map_destroy": (None, [C.c_void_p]),
    "hvo_line_map_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int]),
    "hvo_line_map_set_many": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8),
    "hvo_line_map_set_bad": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hvo_line_map_set_observed": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hvo_line_map_counts": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3),
    "hvo_line_map_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hvo_line_map_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_search_local_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(LocalLinesParams), C.POINTER(LocalLinesFrame), C.POINTER(LocalLinesIO), C.POINTER(LocalLinesResult)]),
    "hvo_stream_search_local_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(LocalLinesParams), C.POINTER(LocalLinesIO), C.POINTER(LocalLinesResult)]),
    "hvo_batch_search_local_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(LocalLinesParams), C.POINTER(LocalLinesIO), C.POINTER(LocalLinesResult)]),
    "hvo_point_map_create": (C.c_void_p, [C.c_int, C.c_int]),
    "hvo_point_map_destroy": (None, [C.c_void_p]),
    "hvo_point_map_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int]),
    "hvo_point_map_set_many": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7),
    "hvo_point_map_set_bad": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hvo_point_map_set_observed": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hvo_point_map_counts": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3),
    "hvo_point_map_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hvo_point_map_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_search_local_points": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(LocalPointsParams), C.POINTER(LocalPointsFrame), C.POINTER(LocalPointsIO), C.POINTER(LocalPointsResult)]),
    "hvo_stream_search_local_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(LocalPointsParams), C.POINTER(LocalPointsIO), C.POINTER(LocalPointsResult)]),
    "hvo_batch_search_local_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(LocalPointsParams), C.POINTER(LocalPointsIO), C.POINTER(LocalPointsResult)]),
    "hvo_kfi_default_params": (None, [C.POINTER(KfiParams)]),
    "hvo_kf_insert_create": (C.c_void_p, [C.c_int]),
    "hvo_kf_insert_destroy": (None, [C.c_void_p]),
    "hvo_kf_insert_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_create_keyframe_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(KfiParams), C.POINTER(KfiFrame), C.POINTER(KfiIO), C.POINTER(KfiResult)]),
    "hvo_stream_create_keyframe_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.c_void_p, C.POINTER(KfiParams), C.POINTER(KfiIO), C.POINTER(KfiResult)]),
    "hvo_vocabulary_create": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 4 + [C.POINTER(C.c_void_p)]),
    "hvo_vocabulary_load_text": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "hvo_vocabulary_destroy": (None, [C.c_void_p]),
    "hvo_vocabulary_info": (C.c_int, [C.c_void_p, C.POINTER(VocabularyDesc)]),
    "hvo_compute_bow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Bow)]),
    "hvo_stream_compute_bow": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(Bow)]),
    "hvo_batch_compute_bow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Bow)]),
    "hvo_search_by_bow": (C.c_int, [C.c_void_p, C.POINTER(BowKeyframe), C.c_int, C.POINTER(BowKeyframe), C.POINTER(BowSearchParams), C.POINTER(BowMatches)]),
    "hvo_stream_search_by_bow": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(BowKeyframe), C.POINTER(BowSearchParams), C.POINTER(BowMatches)]),
    "hvo_bow_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hvo_stream_bow_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "hvo_keyframe_db_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "hvo_keyframe_db_destroy": (None, [C.c_void_p]),
    "hvo_keyframe_db_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_keyframe_db_add": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hvo_stream_keyframe_db_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]),
    "hvo_keyframe_db_erase": (C.c_int, [C.c_void_p, C.c_int]),
    "hvo_keyframe_db_clear": (C.c_int, [C.c_void_p]),
    "hvo_keyframe_db_set_covisible": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hvo_keyframe_db_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "hvo_keyframe_db_info": (C.c_int, [C.c_void_p, C.POINTER(KeyframeDbDesc)]),
    "hvo_keyframe_db_query": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(KfdbParams), C.POINTER(KfdbResult)]),
    "hvo_stream_keyframe_db_query": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(KfdbParams), C.POINTER(KfdbResult)]),
    "hvo_batch_keyframe_db_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(KfdbParams), C.POINTER(KfdbResult)]),
    "hvo_keyframe_db_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hvo_pnp_default_params": (None, [C.POINTER(PnpParams)]),
    "hvo_pnp_ransac": (C.c_int, [C.c_void_p, C.POINTER(PoseCamera), C.POINTER(PnpParams), C.c_int, C.POINTER(PnpProblem), C.POINTER(PnpResult)]),
    "hvo_stream_pnp_ransac": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.POINTER(PnpParams), C.c_int, C.POINTER(PnpKeyframeSide), C.POINTER(PnpResult)]),
    "hvo_pnp_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hvo_search_by_projection_keyframe": (C.c_int, [C.c_void_p, C.POINTER(PoseCamera), C.POINTER(KfSearchParams), C.POINTER(LocalPointsFrame), C.c_int, C.POINTER(KfSearchCandidate), C.POINTER(KfSearchResult)]),
    "hvo_stream_search_by_projection_keyframe": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.POINTER(KfSearchParams), C.c_int, C.POINTER(KfSearchCandidate), C.POINTER(KfSearchResult)]),
    "hvo_fuse_points": (C.c_int, [C.c_void_p, C.POINTER(PoseCamera), C.POINTER(FuseParams), C.POINTER(FuseMap), C.c_int, C.POINTER(FuseKeyframe), C.POINTER(FuseResult)]),
    "hvo_fuse_points_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PoseCamera), C.POINTER(FuseParams), C.c_int, C.POINTER(FuseKeyframe), C.POINTER(FuseResult)]),
    "hvo_create_new_map_points": (C.c_int, [C.c_void_p, C.POINTER(PoseCamera), C.POINTER(NpParams), C.POINTER(NpKeyframe), C.c_int, C.POINTER(NpKeyframe), C.POINTER(NpResult), C.POINTER(NpSummary)]),
    "hvo_stream_create_new_map_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(PoseCamera), C.POINTER(NpParams), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(NpKeyframe), C.POINTER(NpResult), C.POINTER(NpSummary)]),
    "hvo_fuse_lines": (C.c_int, [C.c_void_p, C.POINTER(LfParams), C.POINTER(LfMap), C.c_int, C.POINTER(LfKeyframe), C.POINTER(LfResult)]),
    "hvo_fuse_lines_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(LfParams), C.c_int, C.POINTER(LfKeyframe), C.POINTER(LfResult)]),
    "hvo_stream_fuse_lines": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.POINTER(LfParams), C.c_void_p, C.c_void_p, C.POINTER(LfMap), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(LfResult)]),
    "hvo_stream_fuse_points": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(PoseCamera), C.POINTER(FuseParams), C.c_void_p, C.c_void_p, C.POINTER(FuseMap), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(FuseResult)]),
    "hvo_stream_pnp_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "hvo_search_lines_by_projection_map": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_stream_search_lines_by_projection_map": (C.c_int, [C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_search_by_projection_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 4 + [C.c_int] + [C.c_float] * 4 + [C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_stereo_from_rgbd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "hvo_set_line_culling": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "hvo_vanishing_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvo_lines_3d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "hvo_plane_clouds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_surface_normals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_undistort_keypoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hvo_image_bounds": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hvo_assign_features_to_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_assign_lines_to_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_batch_upload": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FrameIn), C.c_int, C.c_int]),
    "hvo_batch_run": (C.c_int, [C.c_void_p, C.c_uint]),
    "hvo_batch_download": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FrameOut)]),
    "hvo_extract_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FrameIn), C.POINTER(FrameOut), C.c_int, C.c_int, C.c_uint]),
    "hvo_batch_slab_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "hvo_batch_pack_results": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hvo_profile_last": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "hvo_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "hvo_pin_host": (C.c_int, [C.c_void_p, C.c_size_t]),
    "hvo_unpin_host": (C.c_int, [C.c_void_p]),
    "hvo_stream_create": (C.c_int, [C.POINTER(Params), C.POINTER(StreamParams), C.POINTER(C.c_void_p)]),
    "hvo_stream_destroy": (None, [C.c_void_p]),
    "hvo_stream_last_error": (C.c_char_p, [C.c_void_p]),
    "hvo_stream_capacity": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3),
    "hvo_stream_image_bounds": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hvo_stream_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "hvo_stream_poll": (C.c_int, [C.c_void_p, C.c_int64]),
    "hvo_stream_collect": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(FrameOut), C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvo_stream_stage_ms": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "hvo_stream_search_by_projection": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "hvo_stream_match_lines": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hvo_normals_lpvo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hvo_tail_capacity": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3),
    "hvo_set_tail_params": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_double]),
    "hvo_batch_download_tail": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FrameTail)]),
    "hvo_stream_collect_tail": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(FrameTail)]),
}
SIGNATURES["hvo_search_double"] = SIGNATURES["hvo_frame_bf_match"]
SIGNATURES["hvo_batch_pose_optimize"] = SIGNATURES["hvo_pose_optimize"]
SIGNATURES["hvo_extract_lsd_culled"] = SIGNATURES["hvo_extract_lsd"]
SIGNATURES["hvo_batch_stage_upload"] = SIGNATURES["hvo_batch_upload"]
SIGNATURES.update({
    "hvo_batch_commit_staged": (C.c_int, [C.c_void_p]),
    "hvo_batch_results_wait": (C.c_int, [C.c_void_p]),
    "hvo_batch_results_async": (C.c_int, [C.c_void_p, C.c_int, C.c_uint, C.c_void_p]),
    "hvo_batch_slab_layout_ex": (C.c_int, [C.c_void_p, C.c_uint] + [C.c_void_p] * 5),
    "hvo_batch_pack_results_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint]),
    "hvo_lsd_async_report": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3),
    "hvo_set_readings": (C.c_int, [C.c_void_p, C.c_uint]),
    "hvo_stream_set_readings": (C.c_int, [C.c_void_p, C.c_uint]),
    "hvo_stream_project_last": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 +
                                [C.c_float, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "hvo_search_by_projection_tracked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 4 + [C.c_int] +
                                         [C.c_float] * 4 + [C.c_int, C.c_float] + [C.c_void_p] * 3),
    # (ctx, params, current, n, neighbours, matches, pair capacity, results, summary); the stream form: (s, cur, cam[6], params, Tcw, has, n, ...)
    "hvo_create_new_map_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hvo_stream_create_new_map_lines": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_void_p]),
    # (ctx, params, input, positions, output) and (ctx, map, slots, params, input, output)
    "hvo_refresh_map_points": (C.c_int, [C.c_void_p] * 5), "hvo_refresh_map_lines": (C.c_int, [C.c_void_p] * 5),
    "hvo_point_map_refresh": (C.c_int, [C.c_void_p] * 6), "hvo_line_map_refresh": (C.c_int, [C.c_void_p] * 6),
})
# the test doors: exported by the library, not declared in include/hvo.h, so outside EXPORTS
DEBUG_SIGNATURES = {
    "hvo_debug_plan_select": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]),
    "hvo_debug_frame_perm": (C.c_int, [C.c_int, C.c_void_p]),
    "hvo_debug_kf_insert_fill": (C.c_int, [C.c_void_p, C.c_int]),
    "hvo_debug_line_map_scratch": (C.c_int, [C.c_void_p, C.c_int]), "hvo_debug_point_map_scratch": (C.c_int, [C.c_void_p, C.c_int]),
    "hvo_debug_call_arena": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hvo_debug_call_arena_peek": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "hvo_debug_stream_call_arena": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hvo_debug_stream_call_arena_peek": (C.c_int, [C.c_void_p, C.c_int64, C.c_size_t, C.c_size_t, C.c_void_p]),
    "hvo_debug_lsd_images": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_longlong,
                                       C.POINTER(C.c_longlong), C.c_void_p]),
    "hvo_debug_lbd_desc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "hvo_debug_peac_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hvo_debug_launch_report": (C.c_int, [C.c_void_p, C.c_void_p]),
}

# every mirror and the include/hvo.h type it mirrors.  Field names are the header's, except those Python cannot spell (HEADER_NAMES)
HEADER_NAMES = {"lam": "lambda"}
RECORDS = {
    "hvo_keypoint": KEYPOINT_DT, "hvo_keyline": KEYLINE_DT, "hvo_plane": PLANE_DT, "hvo_line3d": LINE3D_DT, "hvo_plane_cloud": PLANE_CLOUD_DT,
    "hvo_surface_normal": SURFACE_NORMAL_DT, "hvo_vp_result": VpResult, "hvo_params": Params, "hvo_frame_in": FrameIn, "hvo_frame_out": FrameOut,
    "hvo_stream_params": StreamParams, "hvo_frame_tail": FrameTail, "hvo_mf_result": MfResult, "hvo_plane_match": PlaneMatch,
    "hvo_plane_update": PlaneUpdate, "hvo_plane_update_result": PlaneUpdateResult, "hvo_pose_plane_params": PosePlaneParams, "hvo_camera": PoseCamera,
    "hvo_pose_problem": PoseProblem, "hvo_pose_flags": PoseFlags, "hvo_pose_result": PoseResult, "hvo_line_struct_params": LineStructParams,
    "hvo_line_struct_problem": LineStructProblem, "hvo_line_opt_result": LineOptResult, "hvo_local_lines_params": LocalLinesParams,
    "hvo_local_lines_frame": LocalLinesFrame, "hvo_local_lines_io": LocalLinesIO, "hvo_local_lines_result": LocalLinesResult,
    "hvo_local_points_params": LocalPointsParams, "hvo_local_points_frame": LocalPointsFrame, "hvo_local_points_io": LocalPointsIO,
    "hvo_local_points_result": LocalPointsResult, "hvo_vocabulary_desc": VocabularyDesc, "hvo_bow": Bow, "hvo_bow_keyframe": BowKeyframe,
    "hvo_bow_search_params": BowSearchParams, "hvo_bow_matches": BowMatches, "hvo_keyframe_db_desc": KeyframeDbDesc, "hvo_kfdb_params": KfdbParams,
    "hvo_kfdb_result": KfdbResult, "hvo_local_ba_params": LocalBAParams, "hvo_local_ba_graph": LocalBAGraph, "hvo_local_ba_result": LocalBAResult,
    "hvo_kfi_params": KfiParams, "hvo_kfi_frame": KfiFrame, "hvo_kfi_io": KfiIO, "hvo_kfi_result": KfiResult, "hvo_pnp_params": PnpParams,
    "hvo_pnp_problem": PnpProblem, "hvo_pnp_event": PnpEvent, "hvo_pnp_result": PnpResult, "hvo_pnp_keyframe_side": PnpKeyframeSide,
    "hvo_kf_search_candidate": KfSearchCandidate, "hvo_kf_search_params": KfSearchParams, "hvo_kf_search_result": KfSearchResult,
    "hvo_fuse_keyframe": FuseKeyframe, "hvo_fuse_map": FuseMap, "hvo_fuse_params": FuseParams, "hvo_fuse_result": FuseResult,
    "hvo_lf_keyframe": LfKeyframe, "hvo_lf_map": LfMap, "hvo_lf_params": LfParams, "hvo_lf_result": LfResult,
    "hvo_np_keyframe": NpKeyframe, "hvo_np_params": NpParams, "hvo_np_result": NpResult, "hvo_np_summary": NpSummary,
    "hvo_nl_keyframe": NlKeyframe, "hvo_nl_params": NlParams, "hvo_nl_match": NlMatch, "hvo_nl_result": NlResult, "hvo_nl_summary": NlSummary,
    "hvo_mr_params": MrParams, "hvo_mr_input": MrInput, "hvo_mr_point_out": MrPointOut, "hvo_mr_line_out": MrLineOut,
}


def lib():
    """libhvo.so, loaded on first use, every function with the signature SIGNATURES / DEBUG_SIGNATURES gives it"""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIBPATH):
            raise HvoError(-3, "libhvo.so not built (run __graft_entry__.build())")
        import sys
        global _LOADED_BEFORE_TORCH
        _LOADED_BEFORE_TORCH = "torch" not in sys.modules
        L = C.CDLL(_LIBPATH)
        for name, (restype, argtypes) in list(SIGNATURES.items()) + [kv for kv in DEBUG_SIGNATURES.items() if hasattr(L, kv[0])]:
            f = getattr(L, name); f.restype = restype; f.argtypes = argtypes
        _LIB = L
    return _LIB


PEAC_CLUSTER_FORMS = ("heads", "c64", "c32", "c16", "c16_lend", "slots")
LSD_GROW_FORMS = ("async", "lat", "grow", "dense", "grow_c", "dense_c")
LSD_PRE_FORMS = ("fused", "split", "u8")
LBD_GRADIENT_FORMS = ("fused", "split", "float")
_PEAC_REPORT_FIELDS = ("cluster", "heads", "heads_big", "ldsq", "edges_done", "poolcap", "group", "cluster_wgs", "perm_items", "blkmap_y",
                       "flood_t", "flood_epl", "flood_slim", "flood_perm_items", "n", "slots_fit")
_LSD_REPORT_FIELDS = ("pre", "compact", "chunk", "chunks", "grow", "async_w", "async_fallback", "async_lds", "lat_lds", "lbd_gradient", "lbd_desc",
                      "perm_items", "n", "cull", "plan_batch", "async_early")
_BATCH_REPORT_FIELDS = ("sched", "orb_first", "lsd_first", "peac_last", "prio_orb", "prio_lsd", "prio_peac", "stages")


def _launch_report_dict(m):
    """the 48 ints of hvo_debug_launch_report / hvo_debug_plan_select as {"peac": {...}, "lsd": {...}, "batch": {...}}; a part that was
    not filled (a stage that has not run, or refuses the geometry) is None.  Forms are named (PEAC_CLUSTER_FORMS, LSD_GROW_FORMS, ...)"""
    m = [int(v) for v in m]
    r = {"peac": None, "lsd": None, "batch": None}
    if m[40] & 1:
        d = dict(zip(_PEAC_REPORT_FIELDS, m[0:16])); d["cluster"] = PEAC_CLUSTER_FORMS[d["cluster"]]; r["peac"] = d
    if m[40] & 2:
        d = dict(zip(_LSD_REPORT_FIELDS, m[16:32])); d["pre"] = LSD_PRE_FORMS[d["pre"]]; d["grow"] = LSD_GROW_FORMS[d["grow"]]
        d["lbd_gradient"] = LBD_GRADIENT_FORMS[d["lbd_gradient"]]; r["lsd"] = d
    if m[40] & 4:
        d = dict(zip(_BATCH_REPORT_FIELDS, m[32:40])); d["n"] = m[41]; r["batch"] = d
    return r


def plan_select(w, h, n, max_batch=None, stages=STAGE_ALL):
    """diagnostics: the kernels a batch of n frames of w x h would take in a context of max_batch frames (default: n) under the current
    environment -- the selection functions the launches use, evaluated on the host: no context, no device"""
    L = lib()
    m = np.zeros(48, np.int32)
    rc = L.hvo_debug_plan_select(int(w), int(h), int(n), int(max_batch if max_batch is not None else n), int(stages), _p(m))
    if rc:
        raise HvoError(rc, "plan_select")
    return _launch_report_dict(m)


def frame_perm(n):
    """diagnostics: the launch order of n items (the bit-reversal order the one-wave-per-frame kernels take their frames in), host only"""
    L = lib()
    m = np.zeros(int(n), np.int32)
    rc = L.hvo_debug_frame_perm(int(n), _p(m))
    if rc:
        raise HvoError(rc, "frame_perm")
    return m


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pin(a):
    """page-lock a numpy array (hvo_pin_host); returns the array.  Unpin with unpin(a) before it is freed."""
    rc = lib().hvo_pin_host(a.ctypes.data, a.nbytes)
    if rc != HVO_OK:
        raise HvoError(rc, "hvo_pin_host")
    return a


def unpin(a):
    lib().hvo_unpin_host(a.ctypes.data)


def default_params(**kw):
    p = Params()
    lib().hvo_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown hvo_params field " + k)
        setattr(p, k, v)
    return p


def local_ba_graph_arrays(graph, limits=True):
    """the graph dict of LocalBA.optimize as contiguous arrays of the C ABI's types, with the counts; refuses what can be refused without
    a device (the limits of include/hvo.h) by raising HvoError(HVO_ERR_UNSUPPORTED) with the reason.  limits=False leaves the limits to
    the library (tests of its own refusals)."""
    a = {}
    for name, dt in LOCAL_BA_GRAPH_ARRAYS:
        v = graph.get(name)
        a[name] = np.ascontiguousarray(np.zeros(0, dt) if v is None else v, dt)
    n_kf = a["Tcw"].size // 12; n_pts = a["pt_pos"].size // 3; n_ln = a["ln_pos"].size // 6
    if a["fixed"].size != n_kf or a["cam"].size != 4 * n_kf:
        raise ValueError("fixed / cam do not match Tcw")
    for start, n in (("pt_obs_start", n_pts), ("ln_obs_start", n_ln), ("par_start", n_ln), ("perp_start", n_ln)):
        if a[start].size == 0 and n == 0:
            a[start] = np.zeros(1, np.int32)
        if a[start].size != n + 1:
            raise ValueError(start + " needs one entry more than its landmarks")
    for name in ("ln_manh_idx", "par_map_size", "perp_map_size"):
        if a[name].size != n_ln:
            raise ValueError(name + " needs one entry per line")
    for kf, other, per in (("pt_obs_kf", ("pt_obs_uv", "pt_obs_inv_sigma2"), (2, 1)), ("ln_obs_kf", ("ln_obs_fn",), (3,)),
                           ("par_kf", ("par_idx", "par_fn"), (1, 3)), ("perp_kf", ("perp_idx", "perp_fn"), (1, 3))):
        start = {"pt_obs_kf": "pt_obs_start", "ln_obs_kf": "ln_obs_start", "par_kf": "par_start", "perp_kf": "perp_start"}[kf]
        if a[kf].size != int(a[start][-1]) or any(a[o].size != k * a[kf].size for o, k in zip(other, per)):
            raise ValueError(kf + " and its companions do not match " + start)
    if int(graph.get("manh_available", 0)) and a["manh_axis"].size != 9:
        raise ValueError("manh_axis must be 3 x 3")

    def no(why):
        raise HvoError(-4, "local_ba_optimize: " + why)
    L = LBA_LIMITS
    if not limits:
        return a, n_kf, n_pts, n_ln
    if n_kf > L["kf"]: no("more than 1024 key frames")
    if n_pts > L["points"]: no("more than 65536 points")
    if n_ln > L["lines"]: no("more than 16384 lines")
    if a["pt_obs_kf"].size > L["pt_obs"]: no("more than 2^20 point observations")
    if a["ln_obs_kf"].size > L["ln_obs"]: no("more than 2^18 line observations")
    if a["par_kf"].size + a["perp_kf"].size > L["struct"]: no("more than 2^18 par plus perp entries")
    if int((a["fixed"] == 0).sum()) > L["free_kf"]: no("more than 64 free key frames")
    for kf in ("pt_obs_kf", "ln_obs_kf", "par_kf", "perp_kf"):
        if a[kf].size and (int(a[kf].min()) < 0 or int(a[kf].max()) >= n_kf): no("a key-frame index outside the call's list")
    for start, kf, what in (("pt_obs_start", "pt_obs_kf", "point"), ("ln_obs_start", "ln_obs_kf", "line")):
        if a[kf].size:
            owner = np.repeat(np.arange(a[start].size - 1, dtype=np.int64), np.diff(a[start]))
            if np.unique(owner * max(n_kf, 1) + a[kf]).size != a[kf].size: no("a key frame observes one %s twice" % what)
    return a, n_kf, n_pts, n_ln


class LocalBA:
    """hvo_local_ba: Optimizer::LocalMapOptimization on the device (reference src/Optimizer.cc:3014-3940).  The object owns a grow-only
    workspace on its device; create it once beside the map and reuse it for every key frame.  Not thread-safe.

    optimize(graph, params=None, stop=None) -> LocalBAOutput.  graph: a dict of the arrays of hvo_local_ba_graph (include/hvo.h;
    key frame 0 is the current key frame, observations are CSR lists naming their observer by its index) plus manh_available; params: a
    dict of changes to the defaults (iterations, max_trials, stop_at_poll, huber_delta, chi2_gate, inv_sigma); stop: None or a
    ctypes.c_int the caller may set from another thread (mbAbortBA)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        rc = lib().hvo_local_ba_create(device, C.byref(h))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_local_ba_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().hvo_local_ba_destroy(self.h)
            self.h = None

    __del__ = close

    def last_error(self):
        return lib().hvo_local_ba_last_error(self.h).decode()

    def last_ms(self):
        ms = C.c_float(0)
        lib().hvo_local_ba_last_ms(self.h, C.byref(ms))
        return ms.value

    def last_profile(self):
        """dict(linearise_ms, trials_ms, factor_ms, call_ms, linearisations, trials) of the last call (hvo_local_ba_last_profile)"""
        ms = (C.c_float * 4)(); n = (C.c_int32 * 2)()
        lib().hvo_local_ba_last_profile(self.h, C.byref(ms), C.byref(n))
        return dict(linearise_ms=ms[0], trials_ms=ms[1], factor_ms=ms[2], call_ms=ms[3], linearisations=n[0], trials=n[1])

    @staticmethod
    def default_params():
        p = LocalBAParams()
        lib().hvo_local_ba_default_params(C.byref(p))
        return p

    def optimize(self, graph, params=None, stop=None, limits=True):
        a, n_kf, n_pts, n_ln = local_ba_graph_arrays(graph, limits)
        p = self.default_params()
        for k, v in (params or {}).items():
            if k in ("iterations", "huber_delta", "chi2_gate", "inv_sigma"):
                for i, x in enumerate(v):
                    getattr(p, k)[i] = x
            else:
                setattr(p, k, v)
        G = LocalBAGraph(n_kf=n_kf, n_points=n_pts, n_lines=n_ln, manh_available=int(graph.get("manh_available", 0)))
        for name, _ in LOCAL_BA_GRAPH_ARRAYS:
            setattr(G, name, _p(a[name]) if a[name].size else None)
        n_po, n_lo, n_pa, n_pe = a["pt_obs_kf"].size, a["ln_obs_kf"].size, a["par_kf"].size, a["perp_kf"].size
        out = LocalBAOutput()
        shapes = dict(Tcw_f=((n_kf, 3, 4), np.float32), Tcw_d=((n_kf, 3, 4), np.float64), pt_f=((n_pts, 3), np.float32), pt_d=((n_pts, 3), np.float64),
                      ln_f=((n_ln, 6), np.float32), ln_d=((n_ln, 6), np.float64), pt_erase=((n_po,), np.uint8), ln_erase=((n_lo,), np.uint8),
                      manh_erase=((n_ln,), np.uint8), par_erase=((n_pa,), np.uint8), perp_erase=((n_pe,), np.uint8), par_made=((n_pa,), np.uint8),
                      perp_made=((n_pe,), np.uint8), line_made=((n_ln,), np.uint8))
        R = LocalBAResult()
        for name in LOCAL_BA_RESULT_ARRAYS:
            shp, dt = shapes[name]
            arr = np.full(shp, 0xEE, dt) if dt == np.uint8 else np.full(shp, np.nan, dt)       # a refusal leaves them as they are
            setattr(out, name, arr)
            setattr(R, name, _p(arr) if arr.size else None)
        rc = lib().hvo_local_ba_optimize(self.h, C.byref(p), C.byref(G), C.byref(stop) if stop is not None else None, C.byref(R))
        out.rc = rc
        if rc != HVO_OK:
            err = HvoError(rc, "local_ba_optimize: " + self.last_error())
            err.output = out                                                  # the arrays as the library left them
            raise err
        for k in ("iterations", "trials", "lam", "chi2"):
            setattr(out, k, list(getattr(R, k)))
        for k in ("n_free_kf", "n_pt_edges", "n_line_obs", "n_manh_edges", "n_par_edges", "n_perp_edges", "n_lines_made", "rounds", "stopped_at", "status"):
            setattr(out, k, getattr(R, k))
        out.ms = self.last_ms()
        return out


class LocalBAOutput:
    """what LocalBA.optimize returns: the arrays and fields of hvo_local_ba_result (lambda is `lam`) and `ms`"""


class PlaneMap:
    """hvo_plane_map: the map's planes resident on one device (world coefficients, bad flag, cloud per slot).  Slot index = position in the
    vector PlaneMatcher::SearchMapByCoefficients would have received.  Not thread-safe; usable from any Context / Stream of its device."""

    def __init__(self, device=0, slots=0, points=0):
        self.h = lib().hvo_plane_map_create(device, slots, points)
        if not self.h:
            raise HvoError(-3, "hvo_plane_map_create")

    def close(self):
        if getattr(self, "h", None):
            lib().hvo_plane_map_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, what):
        if rc != HVO_OK:
            raise HvoError(rc, what + ": " + lib().hvo_plane_map_last_error(self.h).decode())

    def set(self, slot, coef, xyz):
        """set or replace a slot: coef = GetWorldPos() (4 floats), xyz = mvPlanePoints as (n, 3) floats (n may be 0)"""
        c = np.ascontiguousarray(coef, np.float32).reshape(4)
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._chk(lib().hvo_plane_map_set(self.h, slot, _p(c), _p(x) if len(x) else None, len(x)), "plane_map_set")

    def set_bad(self, slot, bad=True):
        self._chk(lib().hvo_plane_map_set_bad(self.h, slot, 1 if bad else 0), "plane_map_set_bad")

    def counts(self):
        """(slots, good slots, points of all slots)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(lib().hvo_plane_map_counts(self.h, C.byref(a), C.byref(b), C.byref(c)), "plane_map_counts")
        return a.value, b.value, c.value

    def slot(self, slot):
        """(coef, n_points, bad) of one slot"""
        c = np.zeros(4, np.float32); n, b = C.c_int(0), C.c_int(0)
        self._chk(lib().hvo_plane_map_slot(self.h, slot, _p(c), C.byref(n), C.byref(b)), "plane_map_slot")
        return c, n.value, bool(b.value)

    def points(self, slot):
        """the slot's cloud as the map holds it -> (n, 3) float32"""
        n = self.slot(slot)[1]
        x = np.zeros((n, 3), np.float32); m = C.c_int(0)
        self._chk(lib().hvo_plane_map_get_points(self.h, slot, _p(x) if n else None, n, C.byref(m)), "plane_map_get_points")
        return x


class KeyFrameInsert:
    """hvo_kf_insert: the workspace of Context.create_keyframe_features / Stream.create_keyframe_features (a device block, a pinned block,
    events; grow-only).  Create it once beside the maps and reuse it for every key frame.  Not thread-safe."""

    def __init__(self, device=0):
        self.h = lib().hvo_kf_insert_create(device)
        if not self.h:
            raise HvoError(-3, "hvo_kf_insert_create")

    def close(self):
        if getattr(self, "h", None):
            lib().hvo_kf_insert_destroy(self.h)
            self.h = None

    __del__ = close

    def last_error(self):
        return lib().hvo_kf_insert_last_error(self.h).decode()

    def _chk(self, rc, what):
        if rc != HVO_OK:
            raise HvoError(rc, "%s: %s" % (what, self.last_error()))

    def debug_fill(self, byte):
        """test door, not product API: the workspace's two blocks, at the sizes they have, set to `byte`"""
        f = lib().hvo_debug_kf_insert_fill
        self._chk(f(self.h, int(byte)), "debug_fill")


class _SlotMap:
    """what LineMap and PointMap share.  A subclass names its C prefix (_c), the dtype of its geometry (_dt) and the geometry's arrays as
    (name, components) (_geo); distance range, descriptor and the two flags are the same for both"""

    def __init__(self, device=0, slots=0):
        self.h = self._f("create")(device, slots)
        if not self.h:
            raise HvoError(-3, "hvo_%s_create" % self._c)

    def _f(self, name):
        return getattr(lib(), "hvo_%s_%s" % (self._c, name))

    def close(self):
        if getattr(self, "h", None):
            self._f("destroy")(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, what):
        if rc != HVO_OK:
            raise HvoError(rc, "%s_%s: %s" % (self._c, what, self._f("last_error")(self.h).decode()))

    def _set(self, slot, geo, max_dist, min_dist, desc, observed):
        a = [np.ascontiguousarray(v, self._dt).reshape(c) for v, (_, c) in zip(geo, self._geo)] + [np.ascontiguousarray(desc, np.uint8).reshape(32)]
        self._chk(self._f("set")(self.h, slot, *[_p(v) for v in a[:-1]], float(max_dist), float(min_dist), _p(a[-1]), 1 if observed else 0), "set")

    def _set_many(self, first, geo, max_dist, min_dist, desc, observed, bad):
        n = len(np.ascontiguousarray(geo[0], self._dt).reshape(-1, self._geo[0][1]))
        a = [np.ascontiguousarray(v, self._dt).reshape(n, c) for v, (_, c) in zip(geo, self._geo)]
        a += [np.ascontiguousarray(max_dist, np.float32).reshape(n), np.ascontiguousarray(min_dist, np.float32).reshape(n), np.ascontiguousarray(desc, np.uint8).reshape(n, 32)]
        a += [None if v is None else np.ascontiguousarray(np.asarray(v).astype(bool), np.uint8).reshape(n) for v in (observed, bad)]
        self._chk(self._f("set_many")(self.h, first, n, *[None if v is None or v.size == 0 else _p(v) for v in a]), "set_many")

    def refresh(self, ctx, slots, obs, n_levels=8, scale_factor=1.2, what=MR_DESCRIPTOR | MR_GEOMETRY, want=None, check=True):
        """Context.refresh_map_points / refresh_map_lines on slots of this map: the position is the slot's, and descriptor, normal, distance range
        (and world vector) are rewritten in place; observed and bad are never touched.  Returns what the array form returns"""
        sl = None if slots is None else np.ascontiguousarray(slots, np.int32).reshape(-1)
        line = self._c == "line_map"
        return _mr_call(ctx, "hvo_%s_refresh" % self._c, line, (self.h, _m.ptr(sl)), (), obs, n_levels, scale_factor, what, want, check)

    def set_bad(self, slot, bad=True):
        self._chk(self._f("set_bad")(self.h, slot, 1 if bad else 0), "set_bad")

    def debug_fill_scratch(self, byte):
        """test door, not product API: the map's two call-scratch buffers, at the sizes they have, set to `byte`"""
        f = getattr(lib(), "hvo_debug_%s_scratch" % self._c)
        self._chk(f(self.h, int(byte)), "debug_fill_scratch")

    def set_observed(self, slot, observed=True):
        self._chk(self._f("set_observed")(self.h, slot, 1 if observed else 0), "set_observed")

    def counts(self):
        """(slots, good slots, slots with observations)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self._f("counts")(self.h, C.byref(a), C.byref(b), C.byref(c)), "counts")
        return a.value, b.value, c.value

    def slot(self, slot):
        """dict(pos, wvec (LineMap only), normal, max_dist, min_dist, desc, bad, observed) of one slot"""
        g = {k: np.zeros(c, self._dt) for k, c in self._geo}; d = np.zeros(32, np.uint8)
        mx, mn, b, o = C.c_float(0), C.c_float(0), C.c_int(0), C.c_int(0)
        self._chk(self._f("slot")(self.h, slot, *[_p(v) for v in g.values()], C.byref(mx), C.byref(mn), _p(d), C.byref(b), C.byref(o)), "slot")
        return dict(g, max_dist=mx.value, min_dist=mn.value, desc=d, bad=bool(b.value), observed=bool(o.value))


class LineMap(_SlotMap):
    """hvo_line_map: mvpLocalMapLines resident on one device (world end points, world vector, normal, distance range, descriptor, bad and
    has-observations flags per slot).  Slot index = position in the vector Tracking::SearchLocalLines walks.  Not thread-safe; usable from
    any Context / Stream of its device."""
    _c, _dt, _geo = "line_map", np.float64, (("pos", 6), ("wvec", 3), ("normal", 3))

    def set(self, slot, pos, wvec, normal, max_dist, min_dist, desc, observed=True):
        """set or replace a slot: pos = GetWorldPos() (6), wvec = GetWorldVector(), normal = GetNormal(), the raw mfMaxDistance / mfMinDistance,
        desc = GetDescriptor() (32 bytes), observed = Observations() > 0"""
        self._set(slot, (pos, wvec, normal), max_dist, min_dist, desc, observed)

    def set_many(self, first, pos, wvec, normal, max_dist, min_dist, desc, observed=None, bad=None):
        """slots first .. first + n - 1 in one upload: pos (n, 6), wvec / normal (n, 3), max_dist / min_dist (n), desc (n, 32), observed / bad (n) or None"""
        self._set_many(first, (pos, wvec, normal), max_dist, min_dist, desc, observed, bad)


class PointMap(_SlotMap):
    """hvo_point_map: mvpLocalMapPoints resident on one device (world position, normal, distance range, descriptor, bad and has-observations
    flags per slot).  Slot index = position in the vector Tracking::SearchLocalPoints walks.  Not thread-safe; usable from any Context /
    Stream of its device."""
    _c, _dt, _geo = "point_map", np.float32, (("pos", 3), ("normal", 3))

    def set(self, slot, pos, normal, max_dist, min_dist, desc, observed=True):
        """set or replace a slot: pos = GetWorldPos() (3), normal = GetNormal() (3), the raw mfMaxDistance / mfMinDistance, desc = GetDescriptor()
        (32 bytes), observed = Observations() > 0"""
        self._set(slot, (pos, normal), max_dist, min_dist, desc, observed)

    def set_many(self, first, pos, normal, max_dist, min_dist, desc, observed=None, bad=None):
        """slots first .. first + n - 1 in one upload: pos / normal (n, 3), max_dist / min_dist (n), desc (n, 32), observed / bad (n) or None"""
        self._set_many(first, (pos, normal), max_dist, min_dist, desc, observed, bad)


class Vocabulary:
    """hvo_vocabulary: the ORB vocabulary (a k-ary tree of 32-byte descriptors) resident on one device, read-only.  The arrays are in the order
    of the reference's text format: row i is node i + 1 (node 0, the root, has no row).  device=-1 makes a host-only vocabulary (validated,
    answers info(), computes nothing)."""

    def __init__(self, k, L, parent, is_leaf, desc, weight, scoring=VOC_L1_NORM, weighting=VOC_TF_IDF, device=0):
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1); n = len(parent)
        a = [parent, np.ascontiguousarray(np.asarray(is_leaf).astype(bool), np.uint8).reshape(n), np.ascontiguousarray(desc, np.uint8).reshape(n, 32),
             np.ascontiguousarray(weight, np.float64).reshape(n)]
        h = C.c_void_p()
        rc = lib().hvo_vocabulary_create(device, k, L, scoring, weighting, n, *[_p(v) if n else None for v in a], C.byref(h))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_vocabulary_create")
        self.h = h

    @classmethod
    def load_text(cls, path, device=0):
        """the reference's text format (ORBvoc.txt); the binary format is not read"""
        h = C.c_void_p()
        rc = lib().hvo_vocabulary_load_text(os.fsencode(path), device, C.byref(h))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_vocabulary_load_text")
        v = cls.__new__(cls); v.h = h
        return v

    def close(self):
        if getattr(self, "h", None):
            lib().hvo_vocabulary_destroy(self.h)
            self.h = None

    __del__ = close

    def info(self):
        """dict(k, L, n_nodes (the root included), n_words, scoring, weighting, device)"""
        d = VocabularyDesc()
        rc = lib().hvo_vocabulary_info(self.h, C.byref(d))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_vocabulary_info")
        return {k: getattr(d, k) for k, _ in VocabularyDesc._fields_}


class KeyFrameDatabase:
    """hvo_keyframe_db: the key-frame database resident on the vocabulary's device.  A key frame is a slot (0 <= slot < 16384) the caller
    numbers; it holds the key frame's bag of words, up to 10 covisible slots and the scores the last queries left on it.  Both detections
    return the slots of the candidates in the reference's order.  Not thread-safe."""

    def __init__(self, voc):
        h = C.c_void_p()
        rc = lib().hvo_keyframe_db_create(voc.h, C.byref(h))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_keyframe_db_create")
        self.h = h; self.voc = voc

    def close(self):
        if getattr(self, "h", None):
            lib().hvo_keyframe_db_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, what):
        if rc != HVO_OK:
            raise HvoError(rc, what + ": " + lib().hvo_keyframe_db_last_error(self.h).decode())

    def last_error(self):
        return lib().hvo_keyframe_db_last_error(self.h).decode()

    def info(self):
        """dict(n_slots, n_live, scoring, device, pooled_words, pool_capacity, next_sequence)"""
        d = KeyframeDbDesc()
        self._chk(lib().hvo_keyframe_db_info(self.h, C.byref(d)), "keyframe_db_info")
        return {k: getattr(d, k) for k, _ in KeyframeDbDesc._fields_}

    def add(self, slot, bow_word, bow_value=None, ticket=None):
        """KeyFrameDatabase::add: add(slot, bow_word, bow_value) with the bag as compute_bow returns it, or add(slot, stream, ticket=t) with the
        bag Stream.compute_bow left on the resident frame t (device to device)"""
        if ticket is not None:
            return bow_word.keyframe_db_add(ticket, self, slot)
        w = np.ascontiguousarray(bow_word, np.int32).reshape(-1); v = np.ascontiguousarray(bow_value, np.float64).reshape(-1)
        if len(w) != len(v):
            raise ValueError("bow_word and bow_value differ in length")
        self._chk(lib().hvo_keyframe_db_add(self.h, slot, len(w), _p(w) if len(w) else None, _p(v) if len(v) else None), "keyframe_db_add")

    def erase(self, slot):
        self._chk(lib().hvo_keyframe_db_erase(self.h, slot), "keyframe_db_erase")

    def clear(self):
        self._chk(lib().hvo_keyframe_db_clear(self.h), "keyframe_db_clear")

    def set_covisible(self, slot, slots):
        """the slot's GetBestCovisibilityKeyFrames(10), in that order"""
        a = np.ascontiguousarray(slots, np.int32).reshape(-1)
        self._chk(lib().hvo_keyframe_db_set_covisible(self.h, slot, len(a), _p(a) if len(a) else None), "keyframe_db_set_covisible")

    setCovisible = set_covisible

    def get(self, slot):
        """(bow_word, bow_value, (kept reloc score, kept loop score)) of a live slot as the device holds them"""
        n = C.c_int32(0); sc = np.zeros(2, np.float32)
        self._chk(lib().hvo_keyframe_db_get(self.h, slot, 0, None, None, C.byref(n), _p(sc)), "keyframe_db_get")
        w = np.zeros(max(n.value, 1), np.int32); v = np.zeros(max(n.value, 1), np.float64)
        self._chk(lib().hvo_keyframe_db_get(self.h, slot, len(w), _p(w), _p(v), C.byref(n), _p(sc)), "keyframe_db_get")
        return w[:n.value].copy(), v[:n.value].copy(), sc

    def query(self, bow_word, bow_value, mode=KFDB_RELOC, min_score=0.0, connected=None, views=False, cap=None):
        """either detection with the bag on the host; see _kfdb_finish for the result"""
        w = np.ascontiguousarray(bow_word, np.int32).reshape(-1); v = np.ascontiguousarray(bow_value, np.float64).reshape(-1)
        if len(w) != len(v):
            raise ValueError("bow_word and bow_value differ in length")
        ns = self.info()["n_slots"]
        P, R, a = _kfdb_args(ns, mode, min_score, connected, views, cap)
        self._chk(lib().hvo_keyframe_db_query(self.h, len(w), _p(w) if len(w) else None, _p(v) if len(v) else None, C.byref(P), C.byref(R)), "keyframe_db_query")
        return _kfdb_finish(R, a, ns, views)

    def DetectRelocalizationCandidates(self, stream, ticket):
        """the candidates' slots for the resident frame `ticket` (Stream.compute_bow first)"""
        return stream.keyframe_db_query(ticket, self)["candidates"].tolist()

    def DetectLoopCandidates(self, bow, connected, minScore):
        """bow: (bow_word, bow_value) of the query key frame or the dict compute_bow returned; connected: the slots of its connected key frames"""
        w, v = (bow["bow_word"], bow["bow_value"]) if isinstance(bow, dict) else bow
        return self.query(w, v, KFDB_LOOP, minScore, connected)["candidates"].tolist()

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._chk(lib().hvo_keyframe_db_last_kernel_ms(self.h, C.byref(ms)), "keyframe_db_last_kernel_ms")
        return ms.value


class Context:
    """One hvo_ctx: one HIP stream + device slabs.  Not thread-safe (like ORBextractor)."""

    def __init__(self, params=None, **kw):
        self.params = params if params is not None else default_params(**kw)
        h = C.c_void_p()
        rc = lib().hvo_create(C.byref(self.params), C.byref(h))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            for a in getattr(self, "_pinned", []):
                unpin(a)
            self._pinned = []
            lib().hvo_destroy(self.h)
            self.h = None

    __del__ = close

    def _last_error(self):
        return lib().hvo_last_error(self.h)

    def _chk(self, rc, what):
        if rc != HVO_OK:
            raise HvoError(rc, what + ": " + self._last_error().decode())

    def debug_call_arena(self, fill=None, min_bytes=0):
        """test door, not product API: grow the context's call arena to at least min_bytes the way a call would, set its whole capacity to the byte
        `fill` (None: leave it) and return the capacity in bytes"""
        L = lib(); f = L.hvo_debug_call_arena
        cap = C.c_size_t(0)
        self._chk(f(self.h, -1 if fill is None else int(fill), int(min_bytes), C.byref(cap)), "debug_call_arena")
        return cap.value

    def debug_call_arena_peek(self, offset, n):
        """test door, not product API: n bytes of the call arena from `offset` -> uint8 array"""
        L = lib(); f = L.hvo_debug_call_arena_peek
        out = np.zeros(int(n), np.uint8)
        self._chk(f(self.h, int(offset), int(n), _p(out)), "debug_call_arena_peek")
        return out

    # ---- single frame ----
    def extract_orb(self, gray):
        if gray is None or gray.size == 0:
            return np.zeros(0, KEYPOINT_DT), np.zeros((0, 32), np.uint8)
        if gray.dtype != np.uint8 or gray.ndim != 2:
            raise HvoError(-6, "ORB input must be CV_8UC1 (ORBextractor.cc:1048)")
        gray = np.ascontiguousarray(gray)
        h, w = gray.shape
        cap = self.params.orb_nfeatures + 8 * self.params.orb_nlevels + 64
        kp = np.zeros(cap, KEYPOINT_DT); desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._chk(lib().hvo_extract_orb(self.h, _p(gray), w, h, gray.strides[0], _p(kp), _p(desc), cap, C.byref(n)), "extract_orb")
        return kp[: n.value].copy(), desc[: n.value].copy()

    def extract_lsd(self, gray, cap=None, culled=False):
        """LINEextractor::operator(); culled=True: Frame::ExtractLSD up to and including cullingLine (Frame.cc:895-934)"""
        if gray is None or gray.size == 0:
            return np.zeros(0, KEYLINE_DT), np.zeros((0, 32), np.uint8), np.zeros((0, 3))
        if gray.dtype != np.uint8 or gray.ndim != 2:
            raise HvoError(-6, "LSD input must be CV_8UC1 (LineExtractor.cpp:335)")
        gray = np.ascontiguousarray(gray)
        h, w = gray.shape
        cap = cap or max(self.params.lsd_nfeatures, 1)
        kl = np.zeros(cap, KEYLINE_DT); desc = np.zeros((cap, 32), np.uint8); fn = np.zeros((cap, 3), np.float64)
        n = C.c_int(0)
        fnc = lib().hvo_extract_lsd_culled if culled else lib().hvo_extract_lsd
        self._chk(fnc(self.h, _p(gray), w, h, gray.strides[0], _p(kl), _p(desc), _p(fn), cap, C.byref(n)), "extract_lsd")
        return kl[: n.value].copy(), desc[: n.value].copy(), fn[: n.value].copy()

    def set_line_culling(self, dis=5.0, angle_deg=2.5, endpoint_dis=15.0):
        """parameters of Frame::cullingLine (Frame.cc:934)"""
        self._chk(lib().hvo_set_line_culling(self.h, dis, angle_deg, endpoint_dis), "set_line_culling")

    def lines_3d(self, kl, depth, seed=1):
        """Frame::isLineGood (src/Frame.cc:1205-1322): mvLines3D / mvLineEq / mvLineNor of every key line -> LINE3D_DT array"""
        kl = np.ascontiguousarray(kl); depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        out = np.zeros(len(kl), LINE3D_DT)
        self._chk(lib().hvo_lines_3d(self.h, _p(kl), len(kl), _p(depth), w, h, depth.strides[0], seed, _p(out)), "lines_3d")
        return out

    def vanishing_points(self, kl, seed=1, th_angle=None, want_grid=False):
        """Frame::getVPHypVia2Lines .. line2Vps (src/Frame.cc:442-778) -> dict(vps (3,3), best, score, n_hypotheses, vp_idx (n)[, grid (90,360)])"""
        kl = np.ascontiguousarray(kl); n = len(kl)
        if th_angle is None:
            th_angle = 1.0 / 180.0 * 3.1415926535897932384626433832795          # Frame.h:365
        res = VpResult(); idx = np.full(n, 3, np.int32); grid = np.zeros((90, 360)) if want_grid else None
        self._chk(lib().hvo_vanishing_points(self.h, _p(kl), n, seed, th_angle, C.byref(res), _p(idx), _p(grid) if want_grid else None), "vanishing_points")
        out = dict(vps=np.array([[res.vps[i][j] for j in range(3)] for i in range(3)]), best=res.best, score=res.score, n_hypotheses=res.n_hypotheses, vp_idx=idx)
        if want_grid:
            out["grid"] = grid
        return out

    def compute_planes(self, depth, cap=64):
        if depth.dtype != np.uint16 or depth.ndim != 2:
            raise HvoError(-6, "depth must be CV_16UC1 (PlaneExtractor.cpp:34-38)")
        depth = np.ascontiguousarray(depth)
        h, w = depth.shape
        labels = np.zeros((h, w), np.int32); planes = np.zeros(cap, PLANE_DT)
        n = C.c_int(0)
        self._chk(lib().hvo_compute_planes(self.h, _p(depth), w, h, depth.strides[0], _p(labels), _p(planes), cap, C.byref(n)), "compute_planes")
        return labels, planes[: n.value].copy()

    def plane_clouds(self, depth, labels, planes, dist_th=0.05, cap=200000):
        """the per-plane tail of Frame::ComputePlanes (src/Frame.cc:2110-2154, 2214-2274) -> (PLANE_CLOUD_DT array, cloud (n, 3) f32)"""
        depth = np.ascontiguousarray(depth, np.uint16); labels = np.ascontiguousarray(labels, np.int32); planes = np.ascontiguousarray(planes)
        h, w = depth.shape
        out = np.zeros(len(planes), PLANE_CLOUD_DT); cloud = np.zeros((cap, 3), np.float32); n = C.c_int(0)
        self._chk(lib().hvo_plane_clouds(self.h, _p(depth), w, h, depth.strides[0], _p(labels), _p(planes), len(planes), dist_th, _p(cloud), cap, _p(out), C.byref(n)), "plane_clouds")
        return out, cloud[: n.value].copy()

    def normals_lpvo(self, depth):
        """Manhattan::computeNormalsLPVO (src/Manhattan.cpp:237-393), the CV_32F reading -> (normals (n,3) f64, depth (n) f32, pixel (n,2) i32)"""
        depth = np.ascontiguousarray(depth, np.uint16); h, w = depth.shape
        cap = ((h + 14) // 15) * ((w + 14) // 15)
        nrm = np.zeros((cap, 3)); dz = np.zeros(cap, np.float32); px = np.zeros((cap, 2), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_normals_lpvo(self.h, _p(depth), w, h, depth.strides[0], _p(nrm), _p(dz), _p(px), cap, C.byref(n)), "normals_lpvo")
        return nrm[: n.value], dz[: n.value], px[: n.value]

    def surface_normals(self, depth):
        """vSurfaceNormal of Frame::ComputePlanes (src/Frame.cc:2157-2212) -> SURFACE_NORMAL_DT array"""
        depth = np.ascontiguousarray(depth, np.uint16); h, w = depth.shape
        cap = (((h + 2) // 3) // 2) * (((w + 2) // 3) // 2)
        out = np.zeros(max(cap, 1), SURFACE_NORMAL_DT); n = C.c_int(0)
        self._chk(lib().hvo_surface_normals(self.h, _p(depth), w, h, depth.strides[0], _p(out), cap, C.byref(n)), "surface_normals")
        return out[: n.value].copy()

    def lsd_images(self, frame=0):
        """diagnostics (not part of the reference interface): what the streaming line kernels of the last batch_run(STAGE_LSD) left for
        `frame` -- the defined mask (sh x words u32, a bit per scaled pixel), the 32-byte records {angle, cos, sin, modgrad} of the defined
        pixels in raster order (n x 4 f64) and the LBD gradient image (h x w x 2 i16).  Only for a batch of at most one chunk."""
        L = lib()
        w, h = self._w, self._h
        sw, sh = int(round(w * 0.8)), int(round(h * 0.8))
        mask = np.zeros((sh, (sw + 31) // 32), np.uint32); rec = np.zeros((sw * sh, 4), np.float64); dxy = np.zeros((h, w, 2), np.int16)
        n = C.c_longlong(0); csw = C.c_int(0); csh = C.c_int(0)
        self._chk(L.hvo_debug_lsd_images(self.h, frame, C.byref(csw), C.byref(csh), _p(mask), _p(rec), len(rec), C.byref(n), _p(dxy)), "lsd_images")
        if (csw.value, csh.value) != (sw, sh):
            raise HvoError(-1, "lsd_images: the plan's scaled size is %d x %d" % (csw.value, csh.value))
        return {"mask": mask, "records": rec[:n.value].copy(), "dxy": dxy}

    def lbd_desc(self, gray, keylines):
        """diagnostics (not part of the reference interface): the 32-byte LBD descriptors of caller-supplied key lines (KEYLINE_DT) on one
        image, by the plan's blur / Sobel and the descriptor kernels HVO_LBD_DESC selected when the plan was built.  The image is uploaded
        as a batch of one: the resident batch and the results of the last batch_run are gone afterwards (upload and run again)"""
        L = lib()
        gray = np.ascontiguousarray(gray, np.uint8); h, w = gray.shape
        kl = np.ascontiguousarray(keylines, KEYLINE_DT)
        desc = np.zeros((len(kl), 32), np.uint8)
        self._chk(L.hvo_debug_lbd_desc(self.h, _p(gray), w, h, gray.strides[0], _p(kl), len(kl), _p(desc)), "lbd_desc")
        return desc

    def peac_stats(self, frame=0):
        """diagnostics (not part of the reference interface): bookkeeping words of the last plane run of `frame`"""
        L = lib()
        m = np.zeros(16, np.int32)
        self._chk(L.hvo_debug_peac_stats(self.h, frame, _p(m)), "peac_stats")
        return {"segments": int(m[0]), "coarse_planes": int(m[2]), "flags": int(m[3]), "planes": int(m[4]), "queue_entries": int(m[5]),
                "flood_rounds": int(m[8]), "flood_ranked_rounds": int(m[9]), "flood_serial_rounds": int(m[10]), "ahc_rounds": int(m[11]), "ahc_stops_no_head": int(m[12]), "ahc_stops_conflict": int(m[13]), "ahc_stops_key_order": int(m[14])}

    def launch_report(self):
        """diagnostics (not part of the reference interface): which kernels the last batch_run / compute_planes / extract_lsd of this
        context launched, as _launch_report_dict lays them out; the same record plan_select() gives without a device"""
        L = lib()
        m = np.zeros(48, np.int32)
        self._chk(L.hvo_debug_launch_report(self.h, _p(m)), "launch_report")
        return _launch_report_dict(m)

    # ---- matching ----
    def hamming_matrix(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        d = np.zeros((len(q), len(t)), np.uint16)
        self._chk(lib().hvo_hamming_matrix(self.h, _p(q), len(q), _p(t), len(t), _p(d)), "hamming_matrix")
        return d

    def hamming_knn2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.zeros((len(q), 2), np.int32); dist = np.zeros((len(q), 2), np.int32)
        self._chk(lib().hvo_hamming_knn2(self.h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist)), "hamming_knn2")
        return idx, dist

    def match_nnr(self, d1, d2, nnr):
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        m = np.full(len(d1), -1, np.int32); n = C.c_int(0)
        self._chk(lib().hvo_match_nnr(self.h, _p(d1), len(d1), _p(d2), len(d2), nnr, _p(m), C.byref(n)), "match_nnr")
        return n.value, m

    def search_by_projection(self, q_desc, q_u, q_v, q_radius, q_min_level, q_max_level, q_ur, q_angle, q_blocks,
                             t_kp, t_uright, t_occupied, t_desc, bounds, th_high=100, check_orientation=True):
        """ORBmatcher::SearchByProjection(Cur, Last) core (src/ORBmatcher.cc:1353-1497) -> (nmatches, idx, dist)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        q_desc = np.ascontiguousarray(q_desc, np.uint8); t_desc = np.ascontiguousarray(t_desc, np.uint8)
        nq, nt = len(q_desc), len(t_desc)
        q_u, q_v, q_radius, q_ur, q_angle, t_uright = map(f32, (q_u, q_v, q_radius, q_ur, q_angle, t_uright))
        q_min_level = np.ascontiguousarray(q_min_level, np.int32); q_max_level = np.ascontiguousarray(q_max_level, np.int32)
        q_blocks = np.ascontiguousarray(q_blocks, np.uint8); t_occupied = np.ascontiguousarray(t_occupied, np.uint8)
        t_kp = np.ascontiguousarray(t_kp)
        mi = np.zeros(nq, np.int32); md = np.zeros(nq, np.int32); n = C.c_int(0)
        self._chk(lib().hvo_search_by_projection(self.h, _p(q_desc), nq, _p(q_u), _p(q_v), _p(q_radius), _p(q_min_level), _p(q_max_level),
                                                 _p(q_ur), _p(q_angle), _p(q_blocks), _p(t_kp), _p(t_uright), _p(t_occupied), _p(t_desc), nt,
                                                 bounds[0], bounds[1], bounds[2], bounds[3], th_high, 1 if check_orientation else 0,
                                                 _p(mi), _p(md), C.byref(n)), "search_by_projection")
        return n.value, mi, md

    def frame_bf_match(self, d1, d2, TH=50.0, nnratio=0.9, mutual=False):
        """LSDmatcher::FrameBFMatch (LSDmatcher.cpp:942-966); mutual=True: SearchDouble's two-way check (902-939)"""
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        m = np.full(max(len(d1), 1), -1, np.int32); n = C.c_int(0)
        fn = lib().hvo_search_double if mutual else lib().hvo_frame_bf_match
        self._chk(fn(self.h, _p(d1), len(d1), _p(d2), len(d2), TH, nnratio, _p(m), C.byref(n)), "frame_bf_match")
        return n.value, m[: len(d1)]

    def match_lines_geom(self, d_last, kl_last, d_cur, kl_cur, bounds4, desc_th=0.9, last_has_mapline=None):
        """LSDmatcher::SearchByGeomNApearance (src/LSDmatcher.cpp:36-108) -> (lmatches, matches12, accepted)"""
        d_last = np.ascontiguousarray(d_last, np.uint8); d_cur = np.ascontiguousarray(d_cur, np.uint8)
        kl_last = np.ascontiguousarray(kl_last); kl_cur = np.ascontiguousarray(kl_cur); b = np.ascontiguousarray(bounds4, np.float32)
        n1, n2 = len(kl_last), len(kl_cur)
        hm = None if last_has_mapline is None else np.ascontiguousarray(last_has_mapline, np.uint8)
        m = np.zeros(max(n1, 1), np.int32); acc = np.zeros(max(n1, 1), np.uint8); n = C.c_int(0)
        self._chk(lib().hvo_match_lines_geom(self.h, _p(d_last), _p(kl_last), None if hm is None else _p(hm), n1, _p(d_cur), _p(kl_cur), n2, desc_th, _p(b),
                                             _p(m), _p(acc), C.byref(n)), "match_lines_geom")
        return n.value, m[:n1], acc[:n1]

    def search_lines_by_projection(self, q_xyxy, q_kl, q_desc, q_blocks, t_kl, t_linefn, t_desc, t_occupied, cell_start, cell_items, bounds4, th):
        """LSDmatcher::SearchByProjection(Cur, Last, th) core (src/LSDmatcher.cpp:561-662) -> (nmatches, match_idx, match_dist)"""
        q_xyxy = np.ascontiguousarray(q_xyxy, np.float32).reshape(-1, 4); nq = len(q_xyxy)
        q_kl = np.ascontiguousarray(q_kl); t_kl = np.ascontiguousarray(t_kl); nt = len(t_kl)
        q_desc = np.ascontiguousarray(q_desc, np.uint8); t_desc = np.ascontiguousarray(t_desc, np.uint8)
        q_blocks = np.ascontiguousarray(q_blocks, np.uint8); t_occupied = np.ascontiguousarray(t_occupied, np.uint8)
        t_linefn = np.ascontiguousarray(t_linefn, np.float64); b = np.ascontiguousarray(bounds4, np.float32)
        cs = np.ascontiguousarray(cell_start, np.int32); ci = np.ascontiguousarray(cell_items, np.int32)
        if len(ci) == 0: ci = np.zeros(1, np.int32)
        mi = np.zeros(max(nq, 1), np.int32); md = np.zeros(max(nq, 1), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_search_lines_by_projection(self.h, nq, _p(q_xyxy), _p(q_kl), _p(q_desc), _p(q_blocks), _p(t_kl), _p(t_linefn), _p(t_desc), _p(t_occupied), nt,
                                                       _p(cs), _p(ci), _p(b), th, _p(mi), _p(md), C.byref(n)), "search_lines_by_projection")
        return n.value, mi[:nq], md[:nq]

    def search_lines_by_projection_map(self, q_xyxy, q_view_cos, q_wvec, q_desc, q_blocks, t_kl, t_linefn, t_l3d, t_desc, t_occupied, cell_start, cell_items,
                                       bounds4, th=1.0, nn_ratio=0.95):
        """LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th), the local-map line search (src/LSDmatcher.cpp:709-801) -> (nmatches, match_idx,
        match_dist).  q_blocks / t_occupied may be None; t_l3d: LINE3D_DT (mvLines3D of the current frame)"""
        q_xyxy = np.ascontiguousarray(q_xyxy, np.float32).reshape(-1, 4); nq = len(q_xyxy)
        q_view_cos = np.ascontiguousarray(q_view_cos, np.float32).reshape(-1); q_wvec = np.ascontiguousarray(q_wvec, np.float64).reshape(-1, 3)
        q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        t_kl = np.ascontiguousarray(t_kl); nt = len(t_kl); t_l3d = np.ascontiguousarray(t_l3d, LINE3D_DT)
        t_linefn = np.ascontiguousarray(t_linefn, np.float64); t_desc = np.ascontiguousarray(t_desc, np.uint8); b = np.ascontiguousarray(bounds4, np.float32)
        assert len(q_view_cos) == nq and len(q_wvec) == nq and len(q_desc) == nq and len(t_l3d) == nt and len(t_desc) == nt
        keep = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (q_blocks, t_occupied)]
        cs = np.ascontiguousarray(cell_start, np.int32); ci = np.ascontiguousarray(cell_items, np.int32)
        if len(ci) == 0: ci = np.zeros(1, np.int32)
        pp = lambda a: None if a is None else _p(a)
        mi = np.zeros(max(nq, 1), np.int32); md = np.zeros(max(nq, 1), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_search_lines_by_projection_map(self.h, nq, pp(q_xyxy), pp(q_view_cos), pp(q_wvec), pp(q_desc), pp(keep[0]), pp(t_kl), pp(t_linefn),
                                                           pp(t_l3d), pp(t_desc), pp(keep[1]), nt, _p(cs), _p(ci), _p(b), th, nn_ratio, _p(mi), _p(md), C.byref(n)),
                  "search_lines_by_projection_map")
        return n.value, mi[:nq], md[:nq]

    def track_manhattan(self, normals, l3d, R_last, axes=False):
        """Tracking::TrackManhattanFrame(R_last, vSurfaceNormal, mVF3DLines) (src/Tracking.cc:1172-1348) -> MfResult, or (MfResult,
        normal_axes, line_axes) with axes=True.  normals: SURFACE_NORMAL_DT or (N, 3) floats; l3d: LINE3D_DT of every key line (None: no
        lines); R_last: 3 x 3 (R_cm of the last frame)."""
        sn = _normals_arg(normals)
        l3d = np.zeros(0, LINE3D_DT) if l3d is None else np.ascontiguousarray(l3d, LINE3D_DT).reshape(-1)
        R = np.ascontiguousarray(R_last, np.float32).reshape(9)
        res = MfResult()
        na = np.zeros(max(len(sn), 1), np.uint8); la = np.zeros(max(len(l3d), 1), np.uint8)
        self._chk(lib().hvo_track_manhattan(self.h, _p(sn) if len(sn) else None, len(sn), _p(l3d) if len(l3d) else None, len(l3d), _p(R), C.byref(res),
                                            _p(na) if axes else None, _p(la) if axes else None), "track_manhattan")
        return (res, na[:len(sn)], la[:len(l3d)]) if axes else res

    def batch_track_manhattan(self, R0, n=None):
        """the first n (default all) frames of the resident batch as a sequence, frame k from frame k-1's R (needs STAGE_PLANE_TAIL |
        STAGE_LINES3D in the last batch_run) -> list of MfResult"""
        n = self._B if n is None else n
        R = np.ascontiguousarray(R0, np.float32).reshape(9)
        res = (MfResult * n)()
        self._chk(lib().hvo_batch_track_manhattan(self.h, n, _p(R), res), "batch_track_manhattan")
        return list(res)

    def _pose_call(self, fn, what, cam, probs, plane_params, resident):
        built = [_pose_problem(**p) for p in probs]
        n = len(built)
        P = (PoseProblem * n)(*[b[0] for b in built]); F = (PoseFlags * n)(*[b[1] for b in built]); R = (PoseResult * n)()
        c = _pose_cam(cam)
        self._chk(fn(self.h, C.byref(c), _pose_pp(plane_params), n, P, R, F), what)
        out = []
        for i in range(n):
            r = PoseResult.from_buffer_copy(R[i])
            for k, a in built[i][3].items(): setattr(r, k, a)
            out.append(r)
        return out

    def pose_optimize(self, cam, problems, plane_params=None):
        """Optimizer::PoseOptimization (src/Optimizer.cc:590-1478) of one problem (a dict of _pose_problem's keywords: Tcw, kp_un, uright,
        inv_sigma2, linefn, lines3d, plane_coef, pt_has, pt_xyz, ln_has, ln_xyz, pl_has, pl_coef_w or plane_map + plane_match) or of a list of
        them in one launch, one workgroup each -> PoseResult or list of PoseResult.  cam = (fx, fy, cx, cy, bf); plane_params: PosePlaneParams,
        dict or None (TUM3.yaml)."""
        single = isinstance(problems, dict)
        out = self._pose_call(lib().hvo_pose_optimize, "pose_optimize", cam, [problems] if single else list(problems), plane_params, False)
        return out[0] if single else out

    def batch_pose_optimize(self, cam, problems, plane_params=None):
        """the first len(problems) frames of the resident batch (needs STAGE_ORB, an LSD stage, STAGE_LINES3D, STAGE_PLANE_TAIL and depth), frame
        k under problems[k]: a dict with Tcw, counts = (n_points, n_lines, n_planes) and the map side -> list of PoseResult"""
        return self._pose_call(lib().hvo_batch_pose_optimize, "batch_pose_optimize", cam, list(problems), plane_params, True)

    def _ls_call(self, fn, what, p, sizes, probs, rels):
        n = len(sizes)
        rel = [np.zeros((c, c), np.int8) if r is None else np.ascontiguousarray(r, np.int8).reshape(c, c).copy() for c, r in zip(sizes, rels)]
        out = [np.zeros((c, 6), np.float64) for c in sizes]
        RP = (C.c_void_p * n)(*[r.ctypes.data for r in rel]); OP = (C.c_void_p * n)(*[o.ctypes.data for o in out]); R = (LineOptResult * n)()
        if probs is None:
            nl = np.array(sizes, np.int32)
            self._chk(fn(self.h, C.byref(p), n, _p(nl), RP, OP, R), what)
        else:
            self._chk(fn(self.h, C.byref(p), n, probs, RP, OP, R), what)
        res = []
        for i in range(n):
            r = LineOptResult.from_buffer_copy(R[i]); r.rel = rel[i]; r.lines = out[i]; res.append(r)
        return res

    def line_struct_optimize(self, problems, params=None, mode=None, row_rule=None):
        """Manhattan::computeStructConstrains for every key line and Optimizer::LineOptStruct (src/Tracking.cc:270-335) of one problem or a list
        of problems in one launch sequence.  A problem is a dict: linefn (n x 3 doubles, mvKeyLineFunctions; needed for part 1), lines3d
        (LINE3D_DT: A, B, line_eq are read), rel (n x n int8; needed when mode is LINE_STRUCT_OPTIMIZE alone).  mode: LINE_STRUCT_CONSTRAINTS,
        LINE_STRUCT_OPTIMIZE or both (default); row_rule: LINE_STRUCT_ROW_UNSET (default) / LINE_STRUCT_ROW_Z0 -> LineOptResult (or a list) with
        .rel (0 none, 1 parallel, 2 perpendicular, negative = rejected) and .lines (n x 6: A, B after the call)."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        p = _ls_params(params, mode, row_rule)
        keep, P = [], (LineStructProblem * len(probs))()
        for i, d in enumerate(probs):
            l3 = np.ascontiguousarray(d["lines3d"], LINE3D_DT).reshape(-1)
            fn = None if d.get("linefn") is None else np.ascontiguousarray(d["linefn"], np.float64).reshape(-1, 3)
            if fn is not None and len(fn) != len(l3): raise ValueError("linefn: %d rows for %d lines" % (len(fn), len(l3)))
            if not (p.mode & LINE_STRUCT_CONSTRAINTS) and d.get("rel") is None: raise ValueError("rel is needed without LINE_STRUCT_CONSTRAINTS")
            keep += [l3, fn]
            P[i].n_lines = len(l3); P[i].lines3d = _m.ptr(l3); P[i].linefn = _m.ptr(fn)
        out = self._ls_call(lib().hvo_line_struct_optimize, "line_struct_optimize", p, [int(q.n_lines) for q in P], P, [d.get("rel") for d in probs])
        return out[0] if single else out

    def batch_line_struct_optimize(self, n_lines, params=None, mode=None, row_rule=None, rel=None):
        """the same on the first len(n_lines) frames of the resident batch (needs an LSD stage, STAGE_LINES3D and depth): n_lines[k] is frame
        k's key-line count; A, B of the resident 3-D line records are rewritten -> list of LineOptResult"""
        sizes = [int(v) for v in n_lines]
        return self._ls_call(lib().hvo_batch_line_struct_optimize, "batch_line_struct_optimize", _ls_params(params, mode, row_rule), sizes, None,
                             rel if rel is not None else [None] * len(sizes))

    def line_opt_last_kernel_ms(self):
        """(pair pass, optimisation) device time of the last line_struct_optimize / batch_line_struct_optimize in ms"""
        ms = (C.c_float * 2)()
        self._chk(lib().hvo_line_opt_last_kernel_ms(self.h, ms), "line_opt_last_kernel_ms")
        return ms[0], ms[1]

    def pose_last_kernel_ms(self):
        ms = C.c_float(0)
        self._chk(lib().hvo_pose_last_kernel_ms(self.h, C.byref(ms)), "pose_last_kernel_ms")
        return ms.value

    def match_planes(self, pmap, coef, Tcw, th=None, matrices=False):
        """PlaneMatcher::SearchMapByCoefficients (src/PlaneMatcher.cpp:10-68) of the frame planes coef ((n, 4) floats, camera frame) under the pose
        Tcw (3 x 4) against the resident PlaneMap -> PlaneMatch, or (PlaneMatch, dist (n, slots), angle (n, slots)) with matrices=True.
        th = (dTh, aTh, verTh, parTh), None for the constructor's defaults."""
        c = np.ascontiguousarray(coef, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        t = _th_arg(th)
        res = PlaneMatch()
        ns = pmap.counts()[0]
        dm = np.zeros((len(c), ns), np.float32); am = np.zeros((len(c), ns), np.float32)
        self._chk(lib().hvo_match_planes(self.h, pmap.h, _p(c) if len(c) else None, len(c), _p(T), None if t is None else _p(t), C.byref(res),
                                         _p(dm) if matrices and dm.size else None, _p(am) if matrices and am.size else None), "match_planes")
        return (res, dm, am) if matrices else res

    def update_map_planes(self, pmap, records, cloud, Tcw, ops, Twc=None):
        """MapPlane::UpdateCoefficientsAndPoints (src/MapPlane.cc:300-368) on the resident PlaneMap from host arrays: records (PLANE_CLOUD_DT) and
        cloud ((n, 3) floats) as plane_clouds / collect_tail return them; ops = (frame plane as match_planes numbers them, slot,
        PLANE_UPDATE_MERGE / _INSERT) in list order; Twc (3 x 4, GetPoseInverse()) for an INSERT -> dict(status, n_frame, n_before, n_after, n_done)"""
        r = np.ascontiguousarray(records, PLANE_CLOUD_DT).reshape(-1)
        c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        W = None if Twc is None else np.ascontiguousarray(Twc, np.float32).reshape(12)
        u, n = _plane_update_arg(ops)
        res = PlaneUpdateResult()
        self._chk(lib().hvo_update_map_planes(self.h, pmap.h, _p(r) if len(r) else None, len(r), _p(c) if len(c) else None, len(c), _p(T),
                                              None if W is None else _p(W), C.byref(u), C.byref(res)), "update_map_planes")
        return res.to_dict(n)

    def batch_match_planes(self, pmap, Tcw, th=None):
        """the first len(Tcw) frames of the resident batch (needs STAGE_PLANE_TAIL in the last batch_run), frame k under Tcw[k] (3 x 4), every
        frame against the same PlaneMap in one launch sequence -> list of PlaneMatch"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 12)
        t = _th_arg(th)
        res = (PlaneMatch * len(T))()
        self._chk(lib().hvo_batch_match_planes(self.h, pmap.h, len(T), _p(T), None if t is None else _p(t), res), "batch_match_planes")
        return list(res)

    def search_local_lines(self, lmap, cam, Tcw, t_kl, t_linefn, t_l3d, t_desc, cell_start, cell_items, bounds4, held=None, seen_extra=None,
                           log_scale_factor=float(np.log(np.float32(1.2))), th=1.0, nn_ratio=0.95, rel_map=False):
        """Tracking::SearchLocalLines + Manhattan::computeStructConstInMap (src/Tracking.cc:3279-3392, src/Manhattan.cpp:163-224) of a frame on
        host arrays against the resident LineMap under the pose Tcw (3 x 4): frustum test of every slot, the local-map line search on the
        lines in view, the CosSita post-gate, the map constraints.  held: the slot each key line holds at entry (-1 = none) ->
        LocalLinesResult with .held, .in_view_slot, .proj, .view_cos, .level, .match_idx, .match_dist, .n_par, .n_perp, .rel_map"""
        nt = len(t_kl)
        keep = [np.ascontiguousarray(t_kl), np.ascontiguousarray(t_linefn, np.float64), np.ascontiguousarray(t_l3d), np.ascontiguousarray(t_desc, np.uint8),
                np.ascontiguousarray(cell_start, np.int32), np.ascontiguousarray(cell_items, np.int32)]
        F = LocalLinesFrame(); F.n_kl = nt
        for k, v in zip(("kl", "linefn", "l3d", "desc", "cell_start", "cell_items"), keep):
            setattr(F, k, _m.ptr(v))
        io, a = _ll_io(nt, lmap.counts()[0], held, seen_extra, rel_map)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); c = _pose_cam(cam); p = _ll_params(bounds4, log_scale_factor, th, nn_ratio)
        r = LocalLinesResult()
        self._chk(lib().hvo_search_local_lines(self.h, lmap.h, C.byref(c), _p(T), C.byref(p), C.byref(F), C.byref(io), C.byref(r)), "search_local_lines")
        return _ll_finish(r, a, nt)

    def batch_search_local_lines(self, lmap, cam, Tcw, n_kl, held=None, seen_extra=None, log_scale_factor=float(np.log(np.float32(1.2))), th=1.0,
                                 nn_ratio=0.95, rel_map=False):
        """the first len(Tcw) frames of the resident batch (needs an LSD stage, STAGE_GRIDS | STAGE_LINES3D and depth), frame k under Tcw[k] with
        n_kl[k] key lines, held[k] and seen_extra[k]; the map is read once for all frames -> list of LocalLinesResult"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 12); n = len(T)
        ns = lmap.counts()[0]
        ios = (LocalLinesIO * n)(); arrs = []
        for k in range(n):
            io, a = _ll_io(int(n_kl[k]), ns, None if held is None else held[k], None if seen_extra is None else seen_extra[k], rel_map)
            ios[k] = io; arrs.append(a)
        c = _pose_cam(cam); p = _ll_params(None, log_scale_factor, th, nn_ratio)
        res = (LocalLinesResult * n)()
        self._chk(lib().hvo_batch_search_local_lines(self.h, lmap.h, n, C.byref(c), _p(T), C.byref(p), ios, res), "batch_search_local_lines")
        return [_ll_finish(res[k], arrs[k], int(n_kl[k])) for k in range(n)]

    def search_local_points(self, pmap, cam, Tcw, t_kp_un, t_uright, t_desc, bounds4, held=None, seen_extra=None,
                            log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8, bf=None, th=1.0, th_high=100, nn_ratio=0.8, view_cos_limit=0.5):
        """Tracking::SearchLocalPoints (src/Tracking.cc:3227-3277) of a frame on host arrays (mvKeysUn, mvuRight or None, mDescriptors) against
        the resident PointMap under the pose Tcw (3 x 4): frustum test of every slot, SearchByProjection(F, vpMapPoints, th) on the points in
        view, the assignment.  held: what each key point holds at entry (a slot, -1, HELD_FOREIGN_OBSERVED, HELD_FOREIGN_UNOBSERVED) ->
        LocalPointsResult with .held, .in_view_slot, .proj (u, v, ur), .view_cos, .level, .match_idx, .match_dist"""
        F, keep, nt = _lp_frame(t_kp_un, t_uright, t_desc)
        io, a = _lp_io(nt, pmap.counts()[0], held, seen_extra)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); c = _pose_cam(cam)
        p = _lp_params(bounds4, log_scale_factor, n_levels, float(cam[4]) if bf is None else bf, th, th_high, nn_ratio, view_cos_limit)
        r = LocalPointsResult()
        self._chk(lib().hvo_search_local_points(self.h, pmap.h, C.byref(c), _p(T), C.byref(p), C.byref(F), C.byref(io), C.byref(r)), "search_local_points")
        return _lp_finish(r, a, nt)

    def create_keyframe_features(self, kfi, pmap, lmap, cam, Tcw, kp_un=None, depth=None, desc=None, keylines=None, ldesc=None, lines3d=None, mode=KFI_KEYFRAME,
                                 th_depth=3.0, held_points=None, held_lines=None, first_point_slot=-1, first_line_slot=-1, n_levels=8, line_n_levels=1,
                                 line_scale_factor=1.2, line_geometry=1, cos_par=None, cos_perp=None):
        """The new map points and map lines of Tracking::CreateNewKeyFrame (src/Tracking.cc:3032-3187; mode KFI_KEYFRAME), StereoInitialization
        (KFI_INIT) or the temporal points of UpdateLastFrame (KFI_TEMPORAL) from a frame on host arrays (mvKeysUn, mvDepth, mDescriptors;
        mvKeylinesUn, mLdesc, mvLines3D), written into the resident PointMap / LineMap from first_*_slot on (-1: returned only; the map may
        then be None).  kfi: a KeyFrameInsert.  held_*: what each feature holds at entry -> KfiOutput"""
        n_kp = 0 if kp_un is None else len(kp_un); n_kl = 0 if keylines is None else len(keylines)
        F = KfiFrame(); F.n_kp = n_kp; F.n_kl = n_kl; keep = []
        for name, v, dt, n in (("kp_un", kp_un, KEYPOINT_DT, n_kp), ("depth", depth, np.float32, n_kp), ("desc", desc, np.uint8, n_kp),
                               ("keylines", keylines, KEYLINE_DT, n_kl), ("ldesc", ldesc, np.uint8, n_kl), ("lines3d", lines3d, LINE3D_DT, n_kl)):
            if n:
                keep.append(np.ascontiguousarray(v, dt)); setattr(F, name, keep[-1].ctypes.data)
                assert keep[-1].size == n * (32 if dt is np.uint8 else 1), name
        p, io, a = _kfi_args(n_kp, n_kl, mode, th_depth, n_levels, line_n_levels, line_scale_factor, line_geometry, cos_par, cos_perp, first_point_slot,
                             first_line_slot, held_points, held_lines)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); c = _pose_cam(cam); r = KfiResult()
        kfi._chk(lib().hvo_create_keyframe_features(kfi.h, self.h, pmap.h if pmap is not None else None, lmap.h if lmap is not None else None, C.byref(c), _p(T),
                                                    C.byref(p), C.byref(F), C.byref(io), C.byref(r)), "create_keyframe_features")
        return _kfi_finish(r, a, n_kp, 0 if mode == KFI_TEMPORAL else n_kl, mode)

    def batch_search_local_points(self, pmap, cam, Tcw, n_kp, held=None, seen_extra=None, log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8,
                                  bf=None, th=1.0, th_high=100, nn_ratio=0.8, view_cos_limit=0.5):
        """the first len(Tcw) frames of the resident batch (needs STAGE_ORB), frame k under Tcw[k] with n_kp[k] key points, held[k] and
        seen_extra[k]; the map is read once for all frames; mvuRight is formed from the resident depth when bf (None: cam's) > 0 -> list of LocalPointsResult"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 12); n = len(T)
        ns = pmap.counts()[0]
        ios = (LocalPointsIO * n)(); arrs = []
        for k in range(n):
            io, a = _lp_io(int(n_kp[k]), ns, None if held is None else held[k], None if seen_extra is None else seen_extra[k])
            ios[k] = io; arrs.append(a)
        c = _pose_cam(cam); p = _lp_params(None, log_scale_factor, n_levels, float(cam[4]) if bf is None else bf, th, th_high, nn_ratio, view_cos_limit)
        res = (LocalPointsResult * n)()
        self._chk(lib().hvo_batch_search_local_points(self.h, pmap.h, n, C.byref(c), _p(T), C.byref(p), ios, res), "batch_search_local_points")
        return [_lp_finish(res[k], arrs[k], int(n_kp[k])) for k in range(n)]

    def compute_bow(self, voc, descs, levelsup=4):
        """Frame::ComputeBoW on host descriptors: descs is one (n, 32) array or a list of them (all frames in one launch sequence)"""
        single = not isinstance(descs, (list, tuple))
        ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in ([descs] if single else descs)]
        nf = len(ds); B = (Bow * nf)(); keep = []
        for f, d in enumerate(ds):
            B[f], a = _bow_out(len(d)); keep.append(a)
        ptr = (C.c_void_p * nf)(*[_m.ptr(d) for d in ds]); nd = np.array([len(d) for d in ds], np.int32)
        self._chk(lib().hvo_compute_bow(self.h, voc.h, levelsup, nf, ptr, _p(nd), B), "compute_bow")
        r = [_bow_finish(B[f], keep[f]) for f in range(nf)]
        return r[0] if single else r

    def batch_compute_bow(self, voc, n, levelsup=4, cap=None):
        """the same on the first n frames of the resident batch; the result stays with the batch until the next batch_run"""
        cap = cap or BOW_MAX_FEATURES
        B = (Bow * n)(); keep = []
        for f in range(n):
            B[f], a = _bow_out(cap); keep.append(a)
        self._chk(lib().hvo_batch_compute_bow(self.h, voc.h, n, levelsup, B), "batch_compute_bow")
        return [_bow_finish(B[f], keep[f]) for f in range(n)]

    def bow_last_kernel_ms(self):
        """(ComputeBoW kernels, SearchByBoW kernels): device ms of the last calls"""
        ms = np.zeros(2, np.float32)
        self._chk(lib().hvo_bow_last_kernel_ms(self.h, _p(ms)), "bow_last_kernel_ms")
        return float(ms[0]), float(ms[1])

    def keyframe_db_query(self, db, bow_word, bow_value, mode=KFDB_RELOC, min_score=0.0, connected=None, views=False):
        """KeyFrameDatabase.query (the database has its own stream; the context only names the call like its siblings)"""
        return db.query(bow_word, bow_value, mode, min_score, connected, views)

    def batch_keyframe_db_query(self, voc, db, n, mode=KFDB_RELOC, min_score=0.0, connected=None, views=False):
        """frames 0 .. n-1 of the resident batch (batch_compute_bow first), queried one after the other; a list of n results"""
        ns = db.info()["n_slots"]
        P = (KfdbParams * n)(); R = (KfdbResult * n)(); keep = []
        for f in range(n):
            P[f], R[f], a = _kfdb_args(ns, mode, min_score, connected, views); keep.append(a)
        rc = lib().hvo_batch_keyframe_db_query(self.h, voc.h, db.h, n, P, R)
        if rc != HVO_OK:
            raise HvoError(rc, "batch_keyframe_db_query: " + db.last_error())
        return [_kfdb_finish(R[f], keep[f], ns, views) for f in range(n)]

    def pnp_ransac(self, cam, problems, params=None, want_sample=False, check=True, spare_events=0):
        """PnPsolver's EPnP RANSAC of every candidate in one call.  cam = (fx, fy, cx, cy); problems: a list of dict(p3d (n x 3), p2d (n x 2),
        sigma2 (n), feature_index (n), n_features); params: pnp_params(...).  Returns one dict per candidate (hyp_inliers, hyp_event, events,
        best_*, the effective N / min_inliers / max_its / epsilon, T, no_more, status); pnp_iterate replays iterate() over it.  check=False:
        a candidate with more records than max_events does not raise, its status is -5.  spare_events: room for that many events beyond max_events
        (cap_events > max_events; the call leaves them alone).  Each dict's "raw" holds the whole arrays as the call left them."""
        P = params or pnp_params()
        Q = (PnpProblem * len(problems))(); keep = []
        for j, pr in enumerate(problems):
            keep.append(PNP_PROBLEM.fill(Q[j], pr)[0]); Q[j].n_features = int(pr["n_features"])
        R, rk = _pnp_results(len(problems), [pr["n_features"] for pr in problems], P, want_sample, spare_events)
        cm = _pose_cam(tuple(cam[:4]) + (0.0,))
        rc = lib().hvo_pnp_ransac(self.h, C.byref(cm), C.byref(P), len(problems), Q, R)
        if rc != -5 or check:
            self._chk(rc, "pnp_ransac")
        return _pnp_finish(R, rk, P.min_set)

    def search_by_projection_keyframe(self, cam, t_kp_un, t_desc, bounds4, kfs, th=10.0, orb_dist=100, check_orientation=True,
                                      log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8, check=True):
        """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1499-1628) of a frame on host arrays
        (mvKeysUn, mDescriptors) for every candidate of kfs (dicts: pos, skip, max_dist, min_dist, desc, angle, Tcw, occupied) in one call.
        Returns one dict per candidate: match_idx, match_dist (per key-frame entry), feature_kf (per frame feature), proj, level, gate,
        n_matches, n_searched, status, kernel_ms.  check=False: (return code, message, the dicts) instead of an exception; a refused call
        leaves every output at KF_UNTOUCHED."""
        F, fkeep, nt = _lp_frame(t_kp_un, None, t_desc)
        P, K, R, keep = _kfs_args(nt, kfs, bounds4, th, orb_dist, check_orientation, log_scale_factor, n_levels)
        cm = _pose_cam(cam)
        rc = lib().hvo_search_by_projection_keyframe(self.h, C.byref(cm), C.byref(P), C.byref(F), len(kfs), K, R)
        return _ret(self, rc, "search_by_projection_keyframe", lambda ok: _kfs_finish(R, keep), check)

    def fuse_points(self, cam, kfs, maps, bounds4, th=3.0, th_low=50, log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8, check=True):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:838-994) for every key frame of kfs (dicts: kp_un, uright or None, desc, Tcw,
        skip or None) in one call.  maps: ONE dict (pos, normal, max_dist, min_dist, desc), shared by all key frames and uploaded once, or a
        list with one dict per key frame.  cam: (fx, fy, cx, cy, bf).  Returns one dict per key frame: best_idx, best_dist, gate, level, proj
        (n x 3), fused_entry, fused_idx (the list the caller walks), n_fused, n_searched, status, kernel_ms.  check=False: (return code,
        message, the dicts) instead of an exception; a refused call leaves every output at FUSE_UNTOUCHED."""
        K, M, _, per_kf, R, finish, keep = _FUSE.build(kfs, maps)
        P = _fuse_params(cam, bounds4, th, th_low, log_scale_factor, n_levels, per_kf); cm = _pose_cam(cam)
        rc = lib().hvo_fuse_points(self.h, C.byref(cm), C.byref(P), M, len(kfs), K, R)
        return _ret(self, rc, "fuse_points", finish, check)

    def fuse_points_slots(self, point_map, slots, cam, kfs, bounds4, th=3.0, th_low=50, log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8, check=True):
        """fuse_points with the map side given as slots of a resident PointMap, shared by all key frames: the map's device arrays are read in
        place, only the slot list and the skip bytes go up.  A bad slot counts as skipped; a slot outside the map refuses the whole call."""
        K, _, sl, _, R, finish, keep = _FUSE.build(kfs, slots=slots)
        P = _fuse_params(cam, bounds4, th, th_low, log_scale_factor, n_levels, False); cm = _pose_cam(cam)
        rc = lib().hvo_fuse_points_slots(self.h, point_map.h, len(sl), _m.ptr(sl), C.byref(cm), C.byref(P), len(kfs), K, R)
        return _ret(self, rc, "fuse_points_slots", finish, check)

    def fuse_lines(self, kfs, maps, th=3.0, th_low=50, log_scale_factor=float(np.log(np.float32(1.2))), n_levels=1, scale_factor=1.2, level_rule="clamped", check=True):
        """LSDmatcher::Fuse(pKF, vpMapLines, th) (src/LSDmatcher.cpp:1297-1434) for every key frame of kfs (dicts: kl, desc_rows, Tcw, cam
        (fx, fy, cx, cy), bounds, skip or None) in one call.  desc_rows are the rows the candidates are compared with: mLineDescriptors, or
        mDescriptors for the text as written.  maps: ONE dict (pos n x 6, normal n x 3, max_distance, min_distance, desc), shared by all key
        frames, or a list with one dict per key frame.  n_levels / scale_factor: the line extractor's octaves (mvScaleFactorsLine).  level_rule:
        "clamped" or "as written".  Returns one dict per key frame: best_idx,
        best_dist, gate (LF_GATES), level, proj (n x 4), fused_entry, fused_idx, behind_entry, n_fused, n_behind, n_searched, status,
        kernel_ms.  check=False: (return code, message, the dicts); a refused call leaves every output at FUSE_UNTOUCHED."""
        K, M, _, per_kf, R, finish, keep = _LF.build(kfs, maps)
        P = _lf_params(th, th_low, log_scale_factor, n_levels, scale_factor, level_rule, per_kf)
        rc = lib().hvo_fuse_lines(self.h, C.byref(P), M, len(kfs), K, R)
        return _ret(self, rc, "fuse_lines", finish, check)

    def fuse_lines_slots(self, line_map, slots, kfs, th=3.0, th_low=50, log_scale_factor=float(np.log(np.float32(1.2))), n_levels=1, scale_factor=1.2,
                         level_rule="clamped", check=True):
        """fuse_lines with the map side given as slots of a resident LineMap, shared by all key frames: the map's device arrays are read in
        place, only the slot list and the skip bytes go up.  A bad slot counts as skipped; a slot outside the map refuses the whole call."""
        K, _, sl, _, R, finish, keep = _LF.build(kfs, slots=slots)
        P = _lf_params(th, th_low, log_scale_factor, n_levels, scale_factor, level_rule, False)
        rc = lib().hvo_fuse_lines_slots(self.h, line_map.h, len(sl), _m.ptr(sl), C.byref(P), len(kfs), K, R)
        return _ret(self, rc, "fuse_lines_slots", finish, check)

    def create_new_map_points(self, cam, cur, kfs, th_low=50, n_levels=8, scale_factor=1.2, check=True):
        """LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:335-580): the epipolar search and the triangulation of the current key frame
        `cur` against every neighbour of kfs in one call.  cur and each neighbour: dict(kp_un, kp or None, uright, depth (both or None), desc,
        node_id, has_map_point, Tcw, mb; a neighbour also skip).  cam: fx, fy, cx, cy, bf.  Returns (one dict per neighbour: match_idx2, match_dist,
        outcome (NP_OUTCOMES), branch, x3d, created_idx1, created_idx2 (the list the caller walks), n_created, gate, status; the summary:
        owner, n_new, kernel_ms).  check=False: (return code, message, the two) instead of an exception; a refused call leaves every output
        at NP_UNTOUCHED."""
        ck = NpKeyframe(); keep1 = _np_keyframe(ck, cur); n1 = ck.n
        K, R, S, P, finish, keep = _np_args(n1, kfs, th_low, n_levels, scale_factor, float(cam[4]))
        cm = _pose_cam(cam)
        rc = lib().hvo_create_new_map_points(self.h, C.byref(cm), C.byref(P), C.byref(ck), len(kfs), K, R, C.byref(S))
        del keep1, keep
        return _ret(self, rc, "create_new_map_points", finish(n1), check)

    def create_new_map_lines(self, cur, kfs, th_high=80, nn_ratio=0.85, n_levels=8, scale_factor=1.2, pairing=NL_PAIR_AS_WRITTEN, n_pairs_cap=None, check=True):
        """LocalMapping::CreateNewMapLinesConstraint (src/LocalMapping.cc:1064-1565): SearchForTriangulation of the current key frame `cur` against
        every neighbour of kfs that passes the baseline gate, and the three-view triangulation of every pair of searched neighbours, in one call.
        cur and each neighbour: dict(kl, linefn, desc, has_map_line, Tcw, cam (fx, fy, cx, cy); a neighbour also mb, median_depth, skip).
        n_levels / scale_factor: the LINE pyramid.  Returns (one dict per neighbour: match_idx, n_matched, gate; one dict per pair: kf2, kf3, mv2, mv3,
        outcome (NL_OUTCOMES), line3d, created_idx0 / idx1 / idx2 (the list the caller walks), n_created, status; the summary: owner_pair, n_new,
        n_pairs, kernel_ms).  check=False: (return code, message, the three) instead of an exception; a refused call leaves every output at
        NL_UNTOUCHED."""
        ck = NlKeyframe(); keep1 = _nl_keyframe(ck, cur); n1 = ck.n
        K, M, R, S, P, cap, finish, keep = _nl_args(n1, kfs, th_high, nn_ratio, n_levels, scale_factor, pairing, n_pairs_cap)
        rc = lib().hvo_create_new_map_lines(self.h, C.addressof(P), C.addressof(ck), len(kfs), C.addressof(K), C.addressof(M), cap, C.addressof(R), C.addressof(S))
        del keep1, keep
        return _ret(self, rc, "create_new_map_lines", finish(n1), check)

    def refresh_map_points(self, pos, obs, n_levels=8, what=MR_DESCRIPTOR | MR_GEOMETRY, want=None, check=True):
        """MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (src/MapPoint.cc:240-305, 328-369) for n points in one call.  pos (n, 3);
        obs: dict(obs_start (n + 1, CSR), obs_desc (n_obs, 32), obs_Ow (n_obs, 3), kf_bad (n_obs) or None, ref_Ow (n, 3), ref_level (n), skip (n) or
        None), the observations in mObservations' order.  The scale table is the context's.  Returns dict(best_obs, best_median, desc, normal,
        max_dist, min_dist, status (MR_STATUS), kernel_ms); an entry the status says was not written holds MR_UNTOUCHED.  want: the outputs to
        ask for (None: all).  check=False: (return code, message, the dict); the limits of map_refresh_check raise either way, before the library is called"""
        p = None if pos is None else np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        return _mr_call(self, "hvo_refresh_map_points", False, (), (_m.ptr(p),), obs, n_levels, 1.2, what, want, check)

    def refresh_map_lines(self, pos, obs, n_levels=8, scale_factor=1.2, what=MR_DESCRIPTOR | MR_GEOMETRY, want=None, check=True):
        """MapLine::ComputeDistinctiveDescriptors + UpdateAverageDir (src/MapLine.cpp:331-396, 404-455) for n lines in one call.  pos (n, 6) doubles;
        obs as for refresh_map_points (LBD rows, mvKeyLines octaves); n_levels / scale_factor: the LINE pyramid.  Returns the same dict with
        normal in float64 and wvec"""
        p = None if pos is None else np.ascontiguousarray(pos, np.float64).reshape(-1, 6)
        return _mr_call(self, "hvo_refresh_map_lines", True, (), (_m.ptr(p),), obs, n_levels, scale_factor, what, want, check)

    def pnp_last_kernel_ms(self):
        """(hypothesis kernels, refine kernels): device ms of the last pnp_ransac"""
        ms = np.zeros(2, np.float32)
        self._chk(lib().hvo_pnp_last_kernel_ms(self.h, _p(ms)), "pnp_last_kernel_ms")
        return float(ms[0]), float(ms[1])

    def search_by_bow(self, frame, kfs, nnratio=0.7, check_orientation=True, th_low=50):
        """ORBmatcher::SearchByBoW on host arrays: frame = dict(desc, node_id, angle), kfs = list of dict(desc, node_id, has_map_point, angle).
        Returns a list of (match_kf, n_matches), one per key frame."""
        F, fkeep = _bow_side(frame["desc"], frame["node_id"], None, frame.get("angle"))
        K, P, R, m, keep = _bow_search_args(F.n, kfs, nnratio, check_orientation, th_low)
        self._chk(lib().hvo_search_by_bow(self.h, C.byref(F), len(kfs), K, C.byref(P), R), "search_by_bow")
        return [(m[j, :F.n].copy(), R[j].n_matches) for j in range(len(kfs))]

    def set_readings(self, blur_float=False, lsd_8u=False):
        """the alternative readings of cv::GaussianBlur / cv::LineSegmentDetector (include/hvo.h HVO_READING_*); the next extraction uses them"""
        self._chk(lib().hvo_set_readings(self.h, (READING_BLUR_FLOAT if blur_float else 0) | (READING_LSD_8U if lsd_8u else 0)), "set_readings")

    def lsd_async_report(self):
        """(frames grown again by the one-wave kernel, workers that sat on a foreign XCD, workers per frame) of the last async line growing"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(lib().hvo_lsd_async_report(self.h, C.byref(a), C.byref(b), C.byref(c)), "lsd_async_report")
        return a.value, b.value, c.value

    def search_by_projection_map(self, q_desc, q_u, q_v, q_radius, q_min_level, q_max_level, q_ur, q_blocks,
                                 t_kp, t_uright, t_occupied, t_desc, bounds, th_high=100, nn_ratio=0.8):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th) core (src/ORBmatcher.cc:45-132) -> (nmatches, match_idx, match_dist)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        q_desc = np.ascontiguousarray(q_desc, np.uint8); t_desc = np.ascontiguousarray(t_desc, np.uint8)
        nq, nt = len(q_desc), len(t_desc)
        q_u, q_v, q_radius, q_ur = map(f32, (q_u, q_v, q_radius, q_ur))
        q_min_level = np.ascontiguousarray(q_min_level, np.int32); q_max_level = np.ascontiguousarray(q_max_level, np.int32)
        q_blocks = np.ascontiguousarray(q_blocks, np.uint8); t_occupied = np.ascontiguousarray(t_occupied, np.uint8)
        t_kp = np.ascontiguousarray(t_kp); t_uright = f32(t_uright)
        mi = np.zeros(nq, np.int32); md = np.zeros(nq, np.int32); n = C.c_int(0)
        self._chk(lib().hvo_search_by_projection_map(self.h, _p(q_desc), nq, _p(q_u), _p(q_v), _p(q_radius), _p(q_min_level), _p(q_max_level), _p(q_ur),
                                                     _p(q_blocks), _p(t_kp), _p(t_uright), _p(t_occupied), _p(t_desc), nt,
                                                     bounds[0], bounds[1], bounds[2], bounds[3], th_high, nn_ratio, _p(mi), _p(md), C.byref(n)),
                  "search_by_projection_map")
        return n.value, mi, md

    def search_by_projection_tracked(self, q_desc, proj_x, proj_y, proj_xr, level, view_cos, q_blocks, th,
                                     t_kp, t_uright, t_occupied, t_desc, bounds, th_high=100, nn_ratio=0.8):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th) from mTrackProjX/Y/XR, mnTrackScaleLevel, mTrackViewCos: the window
        prologue (src/ORBmatcher.cc:55-70, 134-140) runs on the device -> (nmatches, match_idx, match_dist)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        q_desc = np.ascontiguousarray(q_desc, np.uint8); t_desc = np.ascontiguousarray(t_desc, np.uint8)
        nq, nt = len(q_desc), len(t_desc)
        proj_x, proj_y, view_cos = map(f32, (proj_x, proj_y, view_cos)); proj_xr = f32(proj_xr) if proj_xr is not None else None
        level = np.ascontiguousarray(level, np.int32)
        q_blocks = np.ascontiguousarray(q_blocks, np.uint8); t_occupied = np.ascontiguousarray(t_occupied, np.uint8)
        t_kp = np.ascontiguousarray(t_kp); t_uright = f32(t_uright)
        mi = np.zeros(nq, np.int32); md = np.zeros(nq, np.int32); n = C.c_int(0)
        fn = lib().hvo_search_by_projection_tracked
        self._chk(fn(self.h, _p(q_desc), nq, _p(proj_x), _p(proj_y), _p(proj_xr) if proj_xr is not None else None, _p(level), _p(view_cos), _p(q_blocks), float(th),
                     _p(t_kp), _p(t_uright), _p(t_occupied), _p(t_desc), nt, bounds[0], bounds[1], bounds[2], bounds[3], th_high, nn_ratio,
                     _p(mi), _p(md), C.byref(n)), "search_by_projection_tracked")
        return n.value, mi, md

    def stereo_from_rgbd(self, kp, kp_un, depth, bf):
        """Frame::ComputeStereoFromRGBD (src/Frame.cc:1940-1961) -> (mvuRight, mvDepth)"""
        kp = np.ascontiguousarray(kp); kp_un = np.ascontiguousarray(kp_un); depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        ur = np.zeros(len(kp), np.float32); z = np.zeros(len(kp), np.float32)
        self._chk(lib().hvo_stereo_from_rgbd(self.h, _p(kp), _p(kp_un), len(kp), _p(depth), w, h, depth.strides[0], bf, _p(ur), _p(z)), "stereo_from_rgbd")
        return ur, z

    # ---- Frame post-processing ----
    def undistort_keypoints(self, kp, dist5):
        """Frame::UndistortKeyPoints (src/Frame.cc:1701-1731); dist5 = (k1, k2, p1, p2, k3)"""
        kp = np.ascontiguousarray(kp); out = np.zeros_like(kp); d = np.ascontiguousarray(dist5, np.float32)
        assert d.shape == (5,)
        self._chk(lib().hvo_undistort_keypoints(self.h, _p(kp), len(kp), _p(d), _p(out)), "undistort_keypoints")
        return out

    def image_bounds(self, w, h, dist5):
        """Frame::ComputeImageBounds (src/Frame.cc:1733-1762) -> (mnMinX, mnMaxX, mnMinY, mnMaxY)"""
        d = np.ascontiguousarray(dist5, np.float32); b = np.zeros(4, np.float32)
        self._chk(lib().hvo_image_bounds(self.h, w, h, _p(d), _p(b)), "image_bounds")
        return b

    def assign_features_to_grid(self, kp_un, bounds4):
        """Frame::AssignFeaturesToGrid (src/Frame.cc:832-847) as CSR (cell = col*48 + row)"""
        kp_un = np.ascontiguousarray(kp_un); b = np.ascontiguousarray(bounds4, np.float32)
        start = np.zeros(64 * 48 + 1, np.int32); items = np.zeros(max(len(kp_un), 1), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_assign_features_to_grid(self.h, _p(kp_un), len(kp_un), _p(b), _p(start), _p(items), C.byref(n)), "assign_features_to_grid")
        return start, items[: n.value]

    def assign_lines_to_grid(self, kl, bounds4, cap=None):
        """Frame::AssignFeaturesToGridForLine (src/Frame.cc:849-872) as CSR"""
        kl = np.ascontiguousarray(kl); b = np.ascontiguousarray(bounds4, np.float32)
        cap = cap if cap is not None else max(len(kl), 1) * 128
        start = np.zeros(64 * 48 + 1, np.int32); items = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_assign_lines_to_grid(self.h, _p(kl), len(kl), _p(b), _p(start), _p(items), cap, C.byref(n)), "assign_lines_to_grid")
        return start, items[: n.value]

    # ---- batch ----
    def batch_upload(self, gray, depth=None, repeat=1, n=None):
        """gray: (B,H,W) u8; depth: (B,H,W) u16 or None.  repeat > 1 uploads the B frames cyclically
        B*repeat times (frames are passed by pointer, host memory is not replicated); n: only the first n of them
        (a batch size that is no multiple of B: frame f is gray[f % B])."""
        gray = np.ascontiguousarray(gray, np.uint8)
        B0, h, w = gray.shape
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
        B = B0 * repeat
        if n is not None:
            if not 1 <= n <= B: raise ValueError("n = %r outside 1 .. %d" % (n, B))
            B = int(n)
        fi = (FrameIn * B)()
        for b in range(B):
            s = b % B0
            fi[b].gray = gray[s].ctypes.data; fi[b].gray_stride = gray.strides[1]
            if depth is not None:
                fi[b].depth = depth[s].ctypes.data; fi[b].depth_stride = depth.strides[1]
        self._chk(lib().hvo_batch_upload(self.h, B, fi, w, h), "batch_upload")
        self._B, self._w, self._h = B, w, h

    def _frames_in(self, gray, depth, repeat):
        gray = np.ascontiguousarray(gray, np.uint8)
        B0, h, w = gray.shape
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
        B = B0 * repeat
        fi = (FrameIn * B)()
        for b in range(B):
            s = b % B0
            fi[b].gray = gray[s].ctypes.data; fi[b].gray_stride = gray.strides[1]
            if depth is not None:
                fi[b].depth = depth[s].ctypes.data; fi[b].depth_stride = depth.strides[1]
        return fi, B, w, h, (gray, depth)

    def batch_stage_upload(self, gray, depth=None, repeat=1, frames_in=None):
        """the NEXT batch's images into the staging slabs, enqueued on a copy stream of its own (returns at once; the host arrays must
        stay alive and unchanged until batch_commit_staged).  frames_in: a tuple from a previous call (the FrameIn table is reused)."""
        fr = frames_in if frames_in is not None else self._frames_in(gray, depth, repeat)
        fi, B, w, h, _keep = fr
        self._chk(lib().hvo_batch_stage_upload(self.h, B, fi, w, h), "batch_stage_upload")
        self._staged = fr
        return fr

    def batch_commit_staged(self):
        """wait for the staged upload and make it the resident batch (device-to-device)"""
        self._chk(lib().hvo_batch_commit_staged(self.h), "batch_commit_staged")
        _, self._B, self._w, self._h, _ = self._staged

    def batch_results_async(self, n, host_slabs, labels=True):
        """pack the first n frames' results (hvo_batch_pack_results_ex) and start ONE copy of the slabs into `host_slabs` (a page-locked
        uint8 array of n * slab_bytes); batch_results_wait() waits for it.  The resident batch may run again at once."""
        fn = lib().hvo_batch_results_async
        self._chk(fn(self.h, n, SLAB_LABELS if labels else 0, host_slabs.ctypes.data), "batch_results_async")

    def batch_results_wait(self):
        self._chk(lib().hvo_batch_results_wait(self.h), "batch_results_wait")

    def batch_run(self, stages=STAGE_ALL):
        self._chk(lib().hvo_batch_run(self.h, stages), "batch_run")

    def set_tail_params(self, seed=1, plane_dist_th=0.05, vp_th_angle=0.0):
        """seed (frame f draws with seed + f), Plane.DistanceThreshold and line2Vps' angle for the tail stages of batch_run"""
        self._chk(lib().hvo_set_tail_params(self.h, seed, plane_dist_th, vp_th_angle), "set_tail_params")

    def batch_download_tail(self, stages, results):
        """results of the tail stages (STAGE_LINES3D | STAGE_VP | STAGE_PLANE_TAIL | STAGE_GRIDS) of the resident batch, merged into the
        per-frame dicts `results` of batch_download (their line / plane counts size the arrays)"""
        n = len(results)
        kc, lc, _, _ = self.slab_layout()
        bufs = []; arr = (FrameTail * n)()
        for f in range(n):
            b, t = _tail_buffers(kc, lc, self._w, self._h)
            bufs.append(b); arr[f] = t
        self._chk(lib().hvo_batch_download_tail(self.h, n, arr), "batch_download_tail")
        for f in range(n):
            results[f].update(_tail_result(bufs[f], arr[f], len(results[f].get("kl", ())), len(results[f].get("planes", ())), stages))
        return results

    def batch_download(self, stages=STAGE_ALL, pl_cap=64, n=None, reuse=False, labels8=False, pinned=False):
        """results of the first n (default all) frames of the resident batch.  reuse=True keeps the host result arrays of the
        previous call with the same shape (a caller that consumes the results before the next download avoids re-faulting
        ~1.4 MB of fresh pages per frame)."""
        B, w, h = self._B, self._w, self._h
        B = B if n is None else min(B, n)
        kcap = self.params.orb_nfeatures + 8 * self.params.orb_nlevels + 64
        lcap = max(self.params.lsd_nfeatures, 1)
        key = (B, w, h, stages, pl_cap, labels8)
        if reuse and getattr(self, "_dl_key", None) == key:
            fo, res_proto = self._dl_fo, self._dl_res
            self._chk(lib().hvo_batch_download(self.h, B, fo), "batch_download")
            return self._dl_finish(fo, [dict(r) for r in res_proto])
        fo = (FrameOut * B)()
        res = [dict() for _ in range(B)]
        # one slab per output kind for the whole batch (per-frame results are views): 8 allocations, not 8 per frame
        if stages & STAGE_ORB:
            kp = np.zeros((B, kcap), KEYPOINT_DT); desc = np.zeros((B, kcap, 32), np.uint8)
            for b in range(B):
                res[b]["kp"] = kp[b]; res[b]["desc"] = desc[b]
                fo[b].kp = kp[b].ctypes.data; fo[b].desc = desc[b].ctypes.data; fo[b].kp_cap = kcap
        if stages & (STAGE_LSD | STAGE_LSD_CULL):
            kl = np.zeros((B, lcap), KEYLINE_DT); ldesc = np.zeros((B, lcap, 32), np.uint8); linefn = np.zeros((B, lcap, 3))
            for b in range(B):
                res[b]["kl"] = kl[b]; res[b]["ldesc"] = ldesc[b]; res[b]["linefn"] = linefn[b]
                fo[b].kl = kl[b].ctypes.data; fo[b].ldesc = ldesc[b].ctypes.data; fo[b].linefn = linefn[b].ctypes.data
                fo[b].kl_cap = lcap
        if stages & STAGE_PLANES:
            # labels are always written in full; labels8=True: as int8, the way they cross PCIe (no widening to CV_32S)
            labels = np.empty((B, h, w), np.int8 if labels8 else np.int32); planes = np.zeros((B, pl_cap), PLANE_DT)
            if pinned and reuse:
                pin(labels); self._pinned = getattr(self, "_pinned", []) + [labels]
            for b in range(B):
                res[b]["labels"] = labels[b]; res[b]["planes"] = planes[b]
                if labels8: fo[b].labels8 = labels[b].ctypes.data
                else: fo[b].labels = labels[b].ctypes.data
                fo[b].planes = planes[b].ctypes.data; fo[b].pl_cap = pl_cap
        if reuse:
            self._dl_key, self._dl_fo, self._dl_res = key, fo, [dict(r) for r in res]
        self._chk(lib().hvo_batch_download(self.h, B, fo), "batch_download")
        return self._dl_finish(fo, res)

    @staticmethod
    def _dl_finish(fo, res):
        for b, r in enumerate(res):
            r["status"] = fo[b].status
            if "kp" in r:
                r["kp"] = r["kp"][: fo[b].n_kp]; r["desc"] = r["desc"][: fo[b].n_kp]
            if "kl" in r:
                r["kl"] = r["kl"][: fo[b].n_kl]; r["ldesc"] = r["ldesc"][: fo[b].n_kl]; r["linefn"] = r["linefn"][: fo[b].n_kl]
            if "planes" in r:
                r["planes"] = r["planes"][: fo[b].n_planes]
        return res

    def slab_layout(self, labels=False):
        """(kp_cap, kl_cap, pl_cap, slab_bytes) of the resident batch's device result slabs; labels=True: with the int8 label image at
        the end of every slab (HVO_SLAB_LABELS) -> (kp_cap, kl_cap, pl_cap, slab_bytes, labels_off)"""
        a, b, c, d, e = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        fn = lib().hvo_batch_slab_layout_ex
        self._chk(fn(self.h, SLAB_LABELS if labels else 0, C.byref(a), C.byref(b), C.byref(c), C.byref(e), C.byref(d)), "batch_slab_layout")
        return (a.value, b.value, c.value, d.value, e.value) if labels else (a.value, b.value, c.value, d.value)

    def pack_results(self, n, device_ptr, labels=False):
        """write the first n frames' result slabs to device memory at `device_ptr` (n * slab_bytes bytes)"""
        fn = lib().hvo_batch_pack_results_ex
        self._chk(fn(self.h, n, C.c_void_p(device_ptr), SLAB_LABELS if labels else 0), "batch_pack_results")

    def profile_enable(self, mode=1):
        """0 off, 1 hipEvents around each kernel group, 2 events + stages serialised on one stream"""
        self._chk(lib().hvo_profile_enable(self.h, int(mode)), "profile_enable")

    def profile_last(self):
        names = (C.c_char_p * 32)(); ms = (C.c_float * 32)()
        n = lib().hvo_profile_last(self.h, names, ms, 32)
        return {names[i].decode(): ms[i] for i in range(n)}


class BatchPipeline:
    """Consecutive batches with upload, run and download overlapped: `nctx` contexts on `nctx` host threads, each looping
    upload -> run -> download over its own resident batch, with one lock per stage so that only one context at a time
    uploads (the link), runs (the GPU) or downloads -- the three stages of different batches overlap, a stage never competes
    with itself.  (Different contexts may be driven from different threads, include/hvo.h.)  Measured on MI355X with pinned
    host buffers and int8 labels: 3 x 2048 frames sustain 72 % of the resident-batch rate, unlocked threads 50 %."""

    def __init__(self, nctx=3, batch=2048, stages=STAGE_ALL, make_context=None, **ctx_kw):
        import threading
        self.stages = stages; self.batch = batch
        self.ctxs = [make_context(batch) if make_context else Context(max_batch=batch, **ctx_kw) for _ in range(nctx)]
        self.locks = [threading.Lock() for _ in range(3)]

    def run(self, gray, depth, repeat=1, rounds=1, on_result=None, pinned=True):
        """every context processes `rounds` batches of gray/depth (cyclic `repeat`); on_result(ctx_index, results) is called
        with each downloaded batch (result arrays are reused by the next batch of that context).  Returns frames processed."""
        import threading
        def loop(i):
            c = self.ctxs[i]
            for _ in range(rounds):
                with self.locks[0]:
                    c.batch_upload(gray, depth, repeat=repeat)
                with self.locks[1]:
                    c.batch_run(self.stages)
                with self.locks[2]:
                    res = c.batch_download(self.stages, reuse=True, labels8=True, pinned=pinned)
                if on_result:
                    on_result(i, res)
        thr = [threading.Thread(target=loop, args=(i,)) for i in range(len(self.ctxs))]
        for t in thr: t.start()
        for t in thr: t.join()
        return len(self.ctxs) * rounds * len(gray) * repeat

    def close(self):
        for c in self.ctxs:
            c.close()
        self.ctxs = []


class Stream:
    """hvo_stream: the streamed-sequence mode (one Frame construction per camera image, src/Tracking.cc:262, with `depth`
    frames in flight and the last `depth` frames' results resident in HBM for frame-to-frame matching)."""

    def __init__(self, width=640, height=480, depth=4, stages=STAGE_ALL, dist5=(0, 0, 0, 0, 0), bf=40.0, params=None, seed=1, plane_dist_th=0.05, vp_th_angle=0.0, **kw):
        self.params = params if params is not None else default_params(**kw)
        sp = StreamParams(); sp.width = width; sp.height = height; sp.depth = depth; sp.stages = stages; sp.bf = bf
        sp.seed = seed; sp.plane_dist_th = plane_dist_th; sp.vp_th_angle = vp_th_angle; self.seed = seed
        for k in range(5):
            sp.dist5[k] = dist5[k]
        h = C.c_void_p()
        rc = lib().hvo_stream_create(C.byref(self.params), C.byref(sp), C.byref(h))
        if rc != HVO_OK:
            raise HvoError(rc, "hvo_stream_create")
        self.h = h; self.w = width; self.hgt = height; self.stages = stages; self.depth = depth
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        lib().hvo_stream_capacity(self.h, C.byref(a), C.byref(b), C.byref(c))
        self.kp_cap, self.kl_cap, self.pl_cap = a.value, b.value, c.value
        bb = np.zeros(4, np.float32); lib().hvo_stream_image_bounds(self.h, _p(bb)); self.bounds = bb      # mnMinX, mnMaxX, mnMinY, mnMaxY

    def close(self):
        if getattr(self, "h", None):
            lib().hvo_stream_destroy(self.h)
            self.h = None

    __del__ = close

    def _last_error(self):
        return lib().hvo_stream_last_error(self.h)

    def _chk(self, rc, what):
        if rc != HVO_OK:
            raise HvoError(rc, what + ": " + self._last_error().decode())

    def debug_call_arena(self, ticket, fill=None, min_bytes=0):
        """test door, not product API: Context.debug_call_arena on the context of the ring slot that holds frame `ticket`, the arena the
        stream forms of the matching, fusing and solving calls stage through"""
        L = lib(); f = L.hvo_debug_stream_call_arena
        cap = C.c_size_t(0)
        self._chk(f(self.h, int(ticket), -1 if fill is None else int(fill), int(min_bytes), C.byref(cap)), "debug_call_arena")
        return cap.value

    def debug_call_arena_peek(self, ticket, offset, n):
        """test door, not product API: n bytes of that arena from `offset` -> uint8 array"""
        L = lib(); f = L.hvo_debug_stream_call_arena_peek
        out = np.zeros(int(n), np.uint8)
        self._chk(f(self.h, int(ticket), int(offset), int(n), _p(out)), "debug_call_arena_peek")
        return out

    def submit(self, gray, depth=None):
        assert gray.dtype == np.uint8 and gray.shape == (self.hgt, self.w) and gray.strides[1] == 1
        t = C.c_int64(-1)
        if depth is not None:
            assert depth.dtype == np.uint16 and depth.shape == (self.hgt, self.w) and depth.strides[1] == 2
            rc = lib().hvo_stream_submit(self.h, gray.ctypes.data, gray.strides[0], depth.ctypes.data, depth.strides[0], C.byref(t))
        else:
            rc = lib().hvo_stream_submit(self.h, gray.ctypes.data, gray.strides[0], None, 0, C.byref(t))
        self._chk(rc, "stream_submit")
        return t.value

    def poll(self, ticket):
        r = lib().hvo_stream_poll(self.h, ticket)
        if r < 0:
            raise HvoError(r, "stream_poll")
        return r == 1

    def collect(self, ticket, labels=True):
        fo = FrameOut(); r = {}
        tail_stages = self.stages & (STAGE_LINES3D | STAGE_VP | STAGE_PLANE_TAIL | STAGE_GRIDS)
        if tail_stages:                                   # the tail block is read before hvo_stream_collect releases the slot
            tb, tt = _tail_buffers(self.kp_cap, self.kl_cap, self.w, self.hgt)
            self._chk(lib().hvo_stream_collect_tail(self.h, ticket, C.byref(tt)), "stream_collect_tail")
        if self.stages & STAGE_ORB:
            kp = np.zeros(self.kp_cap, KEYPOINT_DT); desc = np.zeros((self.kp_cap, 32), np.uint8); kpu = np.zeros(self.kp_cap, KEYPOINT_DT)
            ur = np.zeros(self.kp_cap, np.float32); zd = np.zeros(self.kp_cap, np.float32)
            fo.kp = kp.ctypes.data; fo.desc = desc.ctypes.data; fo.kp_cap = self.kp_cap
        if self.stages & (STAGE_LSD | STAGE_LSD_CULL):
            kl = np.zeros(self.kl_cap, KEYLINE_DT); ldesc = np.zeros((self.kl_cap, 32), np.uint8); fn = np.zeros((self.kl_cap, 3))
            fo.kl = kl.ctypes.data; fo.ldesc = ldesc.ctypes.data; fo.linefn = fn.ctypes.data; fo.kl_cap = self.kl_cap
        if self.stages & STAGE_PLANES:
            planes = np.zeros(self.pl_cap, PLANE_DT); fo.planes = planes.ctypes.data; fo.pl_cap = self.pl_cap
            if labels:
                lab = np.empty((self.hgt, self.w), np.int32); fo.labels = lab.ctypes.data
        if self.stages & STAGE_ORB:
            self._chk(lib().hvo_stream_collect(self.h, ticket, C.byref(fo), _p(kpu), _p(ur), _p(zd)), "stream_collect")
            n = fo.n_kp
            r.update(kp=kp[:n], desc=desc[:n], kp_un=kpu[:n], uright=ur[:n], zdepth=zd[:n])
        else:
            self._chk(lib().hvo_stream_collect(self.h, ticket, C.byref(fo), None, None, None), "stream_collect")
        if self.stages & (STAGE_LSD | STAGE_LSD_CULL):
            n = fo.n_kl
            r.update(kl=kl[:n], ldesc=ldesc[:n], linefn=fn[:n])
        if self.stages & STAGE_PLANES:
            r["planes"] = planes[: fo.n_planes]
            if labels:
                r["labels"] = lab
        r["status"] = fo.status
        if tail_stages:
            r.update(_tail_result(tb, tt, fo.n_kl, fo.n_planes, tail_stages))
        return r

    def stage_ms(self, ticket):
        ms = np.zeros(3, np.float32)
        self._chk(lib().hvo_stream_stage_ms(self.h, ticket, _p(ms)), "stream_stage_ms")
        return {"orb": float(ms[0]), "lsd": float(ms[1]), "planes": float(ms[2])}

    def project_last(self, cur, last, cam, Tcw, Tlw, q_index, x3Dw, q_blocks, th, mono=False, t_occupied=None, q_desc=None,
                     th_high=100, check_orientation=True, want_uv=False):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) whole between two resident frames: projection prologue
        (src/ORBmatcher.cc:1364-1405) + search core on the device.  cam = (fx, fy, cx, cy, mbf, mb); Tcw / Tlw: 3 x 4 row-major.
        -> (nmatches, idx, dist[, uv])"""
        q_index = np.ascontiguousarray(q_index, np.int32); nq = len(q_index)
        x3Dw = np.ascontiguousarray(x3Dw, np.float32).reshape(-1, 3); assert len(x3Dw) == nq
        Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(12); Tlw = np.ascontiguousarray(Tlw, np.float32).reshape(12)
        q_blocks = np.ascontiguousarray(q_blocks, np.uint8)
        t_occupied = np.ascontiguousarray(t_occupied, np.uint8) if t_occupied is not None else None
        q_desc = np.ascontiguousarray(q_desc, np.uint8) if q_desc is not None else None
        mi = np.zeros(max(nq, 1), np.int32); md = np.zeros(max(nq, 1), np.int32); n = C.c_int(0)
        uv = np.zeros((max(nq, 1), 2), np.float32) if want_uv else None
        pp = lambda a: _p(a) if a is not None else None
        c = PoseCamera(*[float(v) for v in cam])
        fn = lib().hvo_stream_project_last
        self._chk(fn(self.h, cur, last, C.byref(c), _p(Tcw), _p(Tlw), nq, _p(q_index), _p(x3Dw), _p(q_blocks), pp(q_desc), pp(t_occupied),
                     float(th), 1 if mono else 0, th_high, 1 if check_orientation else 0, _p(mi), _p(md), C.byref(n), pp(uv)), "stream_project_last")
        return (n.value, mi[:nq], md[:nq], uv[:nq]) if want_uv else (n.value, mi[:nq], md[:nq])

    def search_by_projection(self, cur, last, q_index, q_u, q_v, q_radius, q_min_level, q_max_level, q_ur, q_blocks,
                             t_occupied=None, q_desc=None, th_high=100, check_orientation=True):
        """ORBmatcher::SearchByProjection(Cur, Last) core between two resident frames -> (nmatches, idx, dist)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        q_index = np.ascontiguousarray(q_index, np.int32); nq = len(q_index)
        q_u, q_v, q_radius = map(f32, (q_u, q_v, q_radius))
        q_ur = f32(q_ur) if q_ur is not None else None
        q_min_level = np.ascontiguousarray(q_min_level, np.int32); q_max_level = np.ascontiguousarray(q_max_level, np.int32)
        q_blocks = np.ascontiguousarray(q_blocks, np.uint8)
        t_occupied = np.ascontiguousarray(t_occupied, np.uint8) if t_occupied is not None else None
        q_desc = np.ascontiguousarray(q_desc, np.uint8) if q_desc is not None else None
        mi = np.zeros(max(nq, 1), np.int32); md = np.zeros(max(nq, 1), np.int32); n = C.c_int(0)
        pp = lambda a: _p(a) if a is not None else None
        self._chk(lib().hvo_stream_search_by_projection(self.h, cur, last, nq, _p(q_index), pp(q_desc), _p(q_u), _p(q_v), _p(q_radius), _p(q_min_level),
                                                        _p(q_max_level), pp(q_ur), _p(q_blocks), pp(t_occupied), th_high, 1 if check_orientation else 0,
                                                        _p(mi), _p(md), C.byref(n)), "stream_search_by_projection")
        return n.value, mi[:nq], md[:nq]

    def compute_bow(self, ticket, voc, levelsup=4):
        """Frame::ComputeBoW on the resident frame `ticket`; kept with the frame (a second call with the same arguments returns computed=False)"""
        b, a = _bow_out(self.kp_cap)
        self._chk(lib().hvo_stream_compute_bow(self.h, ticket, voc.h, levelsup, C.byref(b)), "stream_compute_bow")
        return _bow_finish(b, a)

    def bow_last_kernel_ms(self, cur):
        """(ComputeBoW kernels, SearchByBoW kernels): device ms of the last calls on the resident frame `cur`"""
        ms = np.zeros(2, np.float32)
        self._chk(lib().hvo_stream_bow_last_kernel_ms(self.h, cur, _p(ms)), "stream_bow_last_kernel_ms")
        return float(ms[0]), float(ms[1])

    def keyframe_db_add(self, ticket, db, slot):
        """KeyFrameDatabase::add with the bag compute_bow left on the resident frame `ticket`: device to device"""
        rc = lib().hvo_stream_keyframe_db_add(self.h, ticket, db.voc.h, db.h, slot)
        if rc != HVO_OK:
            raise HvoError(rc, "stream_keyframe_db_add: " + db.last_error())

    def keyframe_db_query(self, ticket, db, mode=KFDB_RELOC, min_score=0.0, connected=None, views=False, voc=None):
        """either detection with the bag compute_bow left on the resident frame `ticket`; nothing of the bag crosses the bus"""
        ns = db.info()["n_slots"]
        P, R, a = _kfdb_args(ns, mode, min_score, connected, views)
        rc = lib().hvo_stream_keyframe_db_query(self.h, ticket, (voc or db.voc).h, db.h, C.byref(P), C.byref(R))
        if rc != HVO_OK:
            raise HvoError(rc, "stream_keyframe_db_query: " + db.last_error())
        return _kfdb_finish(R, a, ns, views)

    def pnp_ransac(self, cur, cam, kf_sides, params=None, want_sample=False, check=True):
        """PnPsolver's RANSAC of every candidate against the resident frame `cur`: kf_sides is a list of dict(match_kf (as search_by_bow returned
        it), pos (key-frame features x 3 world positions), bad (a byte per key-frame feature)).  Returns what Context.pnp_ransac returns."""
        P = params or pnp_params()
        K = (PnpKeyframeSide * len(kf_sides))(); keep = []
        for j, kf in enumerate(kf_sides):
            mk = np.ascontiguousarray(kf["match_kf"], np.int32).reshape(-1)
            if len(mk) < self.kp_cap:                                   # (the call reads one entry per feature the frame can hold: -1 past the given ones)
                mk = np.concatenate([mk, np.full(self.kp_cap - len(mk), -1, np.int32)])
            keep.append(PNP_KF_SIDE.fill(K[j], dict(kf, match_kf=mk))[0])
        R, rk = _pnp_results(len(kf_sides), [self.kp_cap] * len(kf_sides), P, want_sample)
        cm = _pose_cam(tuple(cam[:4]) + (0.0,))
        rc = lib().hvo_stream_pnp_ransac(self.h, cur, C.byref(cm), C.byref(P), len(kf_sides), K, R)
        if rc != -5 or check:
            self._chk(rc, "stream_pnp_ransac")
        return _pnp_finish(R, rk, P.min_set)

    def search_by_projection_keyframe(self, cur, cam, n_kp, kfs, th=10.0, orb_dist=100, check_orientation=True,
                                      log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8, check=True):
        """Context.search_by_projection_keyframe on the resident frame `cur` (needs STAGE_ORB): key points and descriptors stay on the
        device, the bounds are the frame grid's, only the candidates go up.  n_kp: the frame's key-point count (the length of occupied and
        feature_kf)."""
        P, K, R, keep = _kfs_args(int(n_kp), kfs, None, th, orb_dist, check_orientation, log_scale_factor, n_levels)
        cm = _pose_cam(cam)
        rc = lib().hvo_stream_search_by_projection_keyframe(self.h, cur, C.byref(cm), C.byref(P), len(kfs), K, R)
        return _ret(self, rc, "stream_search_by_projection_keyframe", lambda ok: _kfs_finish(R, keep), check)

    def fuse_points(self, cur, cam, Tcw, maps=None, point_map=None, slots=None, skip=None, th=3.0, th_low=50,
                    log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8, check=True):
        """ORBmatcher::Fuse(mpCurrentKeyFrame, vpFuseCandidates) with the resident frame `cur` as the key frame under Tcw (needs STAGE_ORB):
        its undistorted key points, mvuRight and descriptors stay on the device, the bounds are the frame grid's.  The map side is `maps`
        (one dict of host arrays) or `slots` of `point_map`.  Returns one dict as Context.fuse_points does per key frame."""
        K, M, sl, _, R, finish, keep = _FUSE.build([dict(Tcw=Tcw, skip=skip)], maps, slots, resident=True)
        P = _fuse_params(cam, None, th, th_low, log_scale_factor, n_levels, False); cm = _pose_cam(cam)
        rc = lib().hvo_stream_fuse_points(self.h, cur, C.byref(cm), C.byref(P), C.addressof(K[0].Tcw), K[0].skip, M, point_map.h if point_map is not None else None,
                                          M[0].n if sl is None else len(sl), _m.ptr(sl), R)
        return _ret(self, rc, "stream_fuse_points", lambda ok: finish(ok)[0], check)

    def fuse_lines(self, cur, cam, Tcw, maps=None, line_map=None, slots=None, skip=None, th=3.0, th_low=50, log_scale_factor=float(np.log(np.float32(1.2))),
                   n_levels=1, scale_factor=1.2, level_rule="clamped", check=True):
        """LSDmatcher::Fuse(mpCurrentKeyFrame, vpFuseCandidates) with the resident frame `cur` as the key frame under Tcw and cam (needs an LSD
        stage): its key lines and LBD descriptors stay on the device, the bounds are the frame grid's.  The map side is `maps` (one dict of
        host arrays) or `slots` of `line_map`.  Returns one dict as Context.fuse_lines does per key frame."""
        K, M, sl, _, R, finish, keep = _LF.build([dict(Tcw=Tcw, skip=skip)], maps, slots, resident=True)
        P = _lf_params(th, th_low, log_scale_factor, n_levels, scale_factor, level_rule, False); cm = _pose_cam(cam)
        rc = lib().hvo_stream_fuse_lines(self.h, cur, C.byref(cm), C.byref(P), C.addressof(K[0].Tcw), K[0].skip, M, line_map.h if line_map is not None else None,
                                         M[0].n if sl is None else len(sl), _m.ptr(sl), R)
        return _ret(self, rc, "stream_fuse_lines", lambda ok: finish(ok)[0], check)

    def pnp_last_kernel_ms(self, cur):
        ms = np.zeros(2, np.float32)
        self._chk(lib().hvo_stream_pnp_last_kernel_ms(self.h, cur, _p(ms)), "stream_pnp_last_kernel_ms")
        return float(ms[0]), float(ms[1])

    def create_new_map_points(self, cur, voc, cam, Tcw, has_map_point, kfs, th_low=50, n_levels=8, scale_factor=1.2, check=True):
        """LocalMapping::CreateNewMapPoints with the resident frame `cur` as the current key frame under Tcw (needs STAGE_ORB and the bag of words
        compute_bow left on it for voc): key points, mvuRight, mvDepth, descriptors and node ids are read where the stages left them; only the
        occupancy bytes (one per feature of the frame), the pose and the neighbours go up.  cam: fx, fy, cx, cy, bf, b (the current key frame's
        mb).  Returns what Context.create_new_map_points returns."""
        hm = np.asarray(has_map_point).astype(bool).reshape(-1); n1 = len(hm)
        has = np.zeros(max(n1, self.kp_cap, 1), np.uint8); has[:n1] = hm          # (a frame with more features than bytes given reads zeros, not past the end)
        K, R, S, P, finish, keep = _np_args(max(n1, self.kp_cap), kfs, th_low, n_levels, scale_factor, float(cam[4]))
        cm = _pose_cam(cam)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        rc = lib().hvo_stream_create_new_map_points(self.h, cur, voc.h, C.byref(cm), C.byref(P), T.ctypes.data, has.ctypes.data, len(kfs), K, R, C.byref(S))
        del keep
        return _ret(self, rc, "stream_create_new_map_points", finish(n1), check)

    def create_new_map_lines(self, cur, cam, Tcw, has_map_line, kfs, th_high=80, nn_ratio=0.85, n_levels=8, scale_factor=1.2, pairing=NL_PAIR_AS_WRITTEN,
                             n_pairs_cap=None, check=True):
        """LocalMapping::CreateNewMapLinesConstraint with the resident frame `cur` (either LSD stage) as the current key frame under Tcw with camera
        cam (fx, fy, cx, cy): key lines, line functions and descriptors are read where the stage left them; only the occupancy bytes (one per
        line of the frame), the pose and the neighbours go up.  Returns what Context.create_new_map_lines returns."""
        hm = np.asarray(has_map_line).astype(bool).reshape(-1); n1 = len(hm)
        has = np.zeros(max(n1, self.kl_cap, 1), np.uint8); has[:n1] = hm           # (a frame with more lines than bytes given reads zeros, not past the end)
        K, M, R, S, P, cap, finish, keep = _nl_args(max(n1, self.kl_cap), kfs, th_high, nn_ratio, n_levels, scale_factor, pairing, n_pairs_cap)
        cm = (C.c_float * 6)(*([float(v) for v in cam[:4]] + [0.0, 0.0]))
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        rc = lib().hvo_stream_create_new_map_lines(self.h, cur, C.addressof(cm), C.addressof(P), T.ctypes.data, has.ctypes.data, len(kfs), C.addressof(K), C.addressof(M), cap,
                                                   C.addressof(R), C.addressof(S))
        del keep
        return _ret(self, rc, "stream_create_new_map_lines", finish(n1), check)

    def search_by_bow(self, cur, voc, kfs, nnratio=0.7, check_orientation=True, th_low=50):
        """SearchByBoW of the key frames kfs (dicts of desc, node_id, has_map_point, angle) against the resident frame `cur`, which holds its bag
        of words.  Returns a list of (match_kf, n_matches); match_kf has the stream's key-point capacity, entries past the frame's count are -1."""
        K, P, R, m, keep = _bow_search_args(self.kp_cap, kfs, nnratio, check_orientation, th_low)
        self._chk(lib().hvo_stream_search_by_bow(self.h, cur, voc.h, len(kfs), K, C.byref(P), R), "stream_search_by_bow")
        return [(m[j].copy(), R[j].n_matches) for j in range(len(kfs))]

    def set_readings(self, blur_float=False, lsd_8u=False):
        self._chk(lib().hvo_stream_set_readings(self.h, (READING_BLUR_FLOAT if blur_float else 0) | (READING_LSD_8U if lsd_8u else 0)), "stream_set_readings")

    def match_lines_geom(self, cur, last, desc_th=0.9, last_has_mapline=None):
        """LSDmatcher::SearchByGeomNApearance(Cur, Last) between two resident frames -> (lmatches, matches12, accepted)"""
        m = np.full(self.kl_cap, -1, np.int32); acc = np.zeros(self.kl_cap, np.uint8); n1 = C.c_int(0); n = C.c_int(0)
        hm = None if last_has_mapline is None else np.ascontiguousarray(last_has_mapline, np.uint8)
        self._chk(lib().hvo_stream_match_lines_geom(self.h, cur, last, desc_th, None if hm is None else _p(hm), _p(m), _p(acc), C.byref(n1), C.byref(n)), "stream_match_lines_geom")
        return n.value, m[: n1.value], acc[: n1.value]

    def search_lines_by_projection(self, cur, last, q_index, q_xyxy, th, q_blocks=None, t_occupied=None, q_desc=None):
        """LSDmatcher::SearchByProjection(Cur, Last, th) core between two resident frames -> (nmatches, match_idx, match_dist)"""
        q_index = np.ascontiguousarray(q_index, np.int32); nq = len(q_index)
        q_xyxy = np.ascontiguousarray(q_xyxy, np.float32).reshape(-1, 4)
        pp = lambda a, t: _p(np.ascontiguousarray(a, t)) if a is not None else None
        keep = [np.ascontiguousarray(a, t) if a is not None else None for a, t in ((q_desc, np.uint8), (q_blocks, np.uint8), (t_occupied, np.uint8))]
        mi = np.zeros(max(nq, 1), np.int32); md = np.zeros(max(nq, 1), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_stream_search_lines_by_projection(self.h, cur, last, nq, _p(q_index), _p(q_xyxy), None if keep[0] is None else _p(keep[0]),
                                                              None if keep[1] is None else _p(keep[1]), None if keep[2] is None else _p(keep[2]), th,
                                                              _p(mi), _p(md), C.byref(n)), "stream_search_lines_by_projection")
        return n.value, mi[:nq], md[:nq]

    def search_lines_by_projection_map(self, cur, q_xyxy, q_view_cos, q_wvec, q_desc, q_blocks=None, t_occupied=None, th=1.0, nn_ratio=0.95):
        """LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) on the resident frame `cur` (needs STAGE_GRIDS | STAGE_LINES3D and depth)
        -> (nmatches, match_idx, match_dist)"""
        q_xyxy = np.ascontiguousarray(q_xyxy, np.float32).reshape(-1, 4); nq = len(q_xyxy)
        q_view_cos = np.ascontiguousarray(q_view_cos, np.float32).reshape(-1); q_wvec = np.ascontiguousarray(q_wvec, np.float64).reshape(-1, 3)
        q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        assert len(q_view_cos) == nq and len(q_wvec) == nq and len(q_desc) == nq
        keep = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (q_blocks, t_occupied)]
        pp = lambda a: None if a is None else _p(a)
        mi = np.zeros(max(nq, 1), np.int32); md = np.zeros(max(nq, 1), np.int32); n = C.c_int(0)
        self._chk(lib().hvo_stream_search_lines_by_projection_map(self.h, cur, nq, pp(q_xyxy), pp(q_view_cos), pp(q_wvec), pp(q_desc), pp(keep[0]), pp(keep[1]),
                                                                  th, nn_ratio, _p(mi), _p(md), C.byref(n)), "stream_search_lines_by_projection_map")
        return n.value, mi[:nq], md[:nq]

    def search_local_lines(self, lmap, cur, cam, Tcw, n_kl, held=None, seen_extra=None, log_scale_factor=float(np.log(np.float32(1.2))), th=1.0,
                           nn_ratio=0.95, rel_map=False):
        """Tracking::SearchLocalLines + Manhattan::computeStructConstInMap on the resident frame `cur` (needs an LSD stage, STAGE_GRIDS |
        STAGE_LINES3D and depth) against the resident LineMap: only the pose, held and seen_extra go up.  n_kl: the frame's key-line count
        -> LocalLinesResult as Context.search_local_lines"""
        io, a = _ll_io(int(n_kl), lmap.counts()[0], held, seen_extra, rel_map)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); c = _pose_cam(cam); p = _ll_params(None, log_scale_factor, th, nn_ratio)
        r = LocalLinesResult()
        self._chk(lib().hvo_stream_search_local_lines(self.h, lmap.h, cur, C.byref(c), _p(T), C.byref(p), C.byref(io), C.byref(r)), "stream_search_local_lines")
        return _ll_finish(r, a, int(n_kl))

    def search_local_points(self, pmap, cur, cam, Tcw, n_kp, held=None, seen_extra=None, log_scale_factor=float(np.log(np.float32(1.2))), n_levels=8,
                            bf=None, th=1.0, th_high=100, nn_ratio=0.8, view_cos_limit=0.5):
        """Tracking::SearchLocalPoints on the resident frame `cur` (needs STAGE_ORB) against the resident PointMap: only the pose, held and
        seen_extra go up.  n_kp: the frame's key-point count -> LocalPointsResult as Context.search_local_points"""
        io, a = _lp_io(int(n_kp), pmap.counts()[0], held, seen_extra)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); c = _pose_cam(cam)
        p = _lp_params(None, log_scale_factor, n_levels, float(cam[4]) if bf is None else bf, th, th_high, nn_ratio, view_cos_limit)
        r = LocalPointsResult()
        self._chk(lib().hvo_stream_search_local_points(self.h, pmap.h, cur, C.byref(c), _p(T), C.byref(p), C.byref(io), C.byref(r)), "stream_search_local_points")
        return _lp_finish(r, a, int(n_kp))

    def create_keyframe_features(self, kfi, pmap, lmap, cur, cam, Tcw, n_kp, n_kl, mode=KFI_KEYFRAME, th_depth=3.0, held_points=None, held_lines=None,
                                 first_point_slot=-1, first_line_slot=-1, n_levels=8, line_n_levels=1, line_scale_factor=1.2, line_geometry=1,
                                 cos_par=None, cos_perp=None):
        """Context.create_keyframe_features on the resident frame `cur` (needs STAGE_ORB, an LSD stage, STAGE_LINES3D, bf > 0 and depth): the
        frame's arrays are read where they lie (after line_struct_optimize: the optimised 3-D lines), only held goes up.  n_kp / n_kl: the
        frame's counts (the lengths of held_points / held_lines) -> KfiOutput"""
        p, io, a = _kfi_args(n_kp, n_kl, mode, th_depth, n_levels, line_n_levels, line_scale_factor, line_geometry, cos_par, cos_perp, first_point_slot,
                             first_line_slot, held_points, held_lines)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); c = _pose_cam(cam); r = KfiResult()
        rc = lib().hvo_stream_create_keyframe_features(kfi.h, self.h, pmap.h if pmap is not None else None, lmap.h if lmap is not None else None, cur, C.byref(c), _p(T),
                                                       C.byref(p), C.byref(io), C.byref(r))
        kfi._chk(rc, "stream_create_keyframe_features")
        return _kfi_finish(r, a, r.n_kp, r.n_kl, mode)

    def track_manhattan(self, cur, R_last, axes=False):
        """Tracking::TrackManhattanFrame on the resident frame `cur` (needs STAGE_PLANE_TAIL | STAGE_LINES3D and depth): its normals and 3-D
        lines stay on the device -> MfResult, or (MfResult, normal_axes, line_axes over the key lines) with axes=True"""
        R = np.ascontiguousarray(R_last, np.float32).reshape(9)
        res = MfResult()
        nn = C.c_int(0); lib().hvo_tail_capacity(self.kl_cap, self.w, self.hgt, None, C.byref(nn), None)
        na = np.zeros(max(nn.value, 1), np.uint8); la = np.zeros(max(self.kl_cap, 1), np.uint8)
        self._chk(lib().hvo_stream_track_manhattan(self.h, cur, _p(R), C.byref(res), _p(na) if axes else None, _p(la) if axes else None),
                  "stream_track_manhattan")
        return (res, na[:nn.value], la) if axes else res

    def pose_optimize(self, cur, cam, Tcw, counts, plane_params=None, **map_side):
        """Optimizer::PoseOptimization on the resident frame `cur` (needs STAGE_LINES3D, STAGE_PLANE_TAIL, bf > 0 and depth): only the pose and
        the map side (pt_has, pt_xyz, ln_has, ln_xyz, pl_has, pl_coef_w, indexed by feature) go up.  counts = (n_points, n_lines, n_planes)
        of those arrays -> PoseResult with the flag arrays."""
        P, F, keep, fl = _pose_problem(Tcw, counts=tuple(int(v) for v in counts), **map_side)
        c = _pose_cam(cam); r = PoseResult()
        self._chk(lib().hvo_stream_pose_optimize(self.h, cur, C.byref(c), _pose_pp(plane_params), C.byref(P), C.byref(r), C.byref(F)), "stream_pose_optimize")
        for k, a in fl.items(): setattr(r, k, a)
        return r

    def line_struct_optimize(self, cur, n_lines, params=None, mode=None, row_rule=None, rel=None):
        """Manhattan::computeStructConstrains + Optimizer::LineOptStruct on the resident frame `cur` (needs an LSD stage, STAGE_LINES3D and
        depth): n_lines is the frame's key-line count; A, B of the resident 3-D line records are rewritten, so a following pose_optimize or
        search_lines_by_projection_map on the frame sees the optimised lines -> LineOptResult with .rel and .lines"""
        c = int(n_lines); p = _ls_params(params, mode, row_rule)
        r_ = np.zeros((c, c), np.int8) if rel is None else np.ascontiguousarray(rel, np.int8).reshape(c, c).copy()
        out = np.zeros((c, 6), np.float64); r = LineOptResult()
        self._chk(lib().hvo_stream_line_struct_optimize(self.h, cur, C.byref(p), c, _p(r_), _p(out), C.byref(r)), "stream_line_struct_optimize")
        r.rel = r_; r.lines = out
        return r

    def line_opt_last_kernel_ms(self, cur):
        ms = (C.c_float * 2)()
        self._chk(lib().hvo_stream_line_opt_last_kernel_ms(self.h, cur, ms), "stream_line_opt_last_kernel_ms")
        return ms[0], ms[1]

    def pose_last_kernel_ms(self, cur):
        ms = C.c_float(0)
        self._chk(lib().hvo_stream_pose_last_kernel_ms(self.h, cur, C.byref(ms)), "stream_pose_last_kernel_ms")
        return ms.value

    def match_planes(self, pmap, cur, Tcw, th=None):
        """PlaneMatcher::SearchMapByCoefficients on the resident frame `cur` (needs STAGE_PLANE_TAIL and depth): the valid planes of its plane
        tail stay on the device -> PlaneMatch (plane_idx: each frame plane's index among the 64 plane_clouds records)"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        t = _th_arg(th)
        res = PlaneMatch()
        self._chk(lib().hvo_stream_match_planes(self.h, pmap.h, cur, _p(T), None if t is None else _p(t), C.byref(res)), "stream_match_planes")
        return res

    def update_map_planes(self, pmap, cur, Tcw, ops, Twc=None):
        """MapPlane::UpdateCoefficientsAndPoints on the resident frame `cur` (needs STAGE_PLANES | STAGE_PLANE_TAIL and depth): the frame's plane
        clouds stay on the device; ops and the result as Context.update_map_planes"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        W = None if Twc is None else np.ascontiguousarray(Twc, np.float32).reshape(12)
        u, n = _plane_update_arg(ops)
        res = PlaneUpdateResult()
        self._chk(lib().hvo_stream_update_map_planes(self.h, pmap.h, cur, _p(T), None if W is None else _p(W), C.byref(u), C.byref(res)), "stream_update_map_planes")
        return res.to_dict(n)

    def match_lines(self, frm, to, mode=LINE_MATCH_NNR, th=50.0, nnratio=0.95):
        m = np.full(self.kl_cap, -1, np.int32); n1 = C.c_int(0); n = C.c_int(0)
        self._chk(lib().hvo_stream_match_lines(self.h, frm, to, mode, th, nnratio, _p(m), C.byref(n1), C.byref(n)), "stream_match_lines")
        return n.value, m[: n1.value]


# ---------------------------------------------------------------------------------------
# host-side mirrors of the reference's operator interfaces
# ---------------------------------------------------------------------------------------


class ORBextractor:
    """ORB_SLAM2::ORBextractor (include/ORBextractor.h:53-61).  operator()(image) -> (keypoints, descriptors)."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device=0):
        self.ctx = Context(orb_nfeatures=nfeatures, orb_scale_factor=scaleFactor, orb_nlevels=nlevels,
                           orb_ini_th_fast=iniThFAST, orb_min_th_fast=minThFAST, device=device)

    def __call__(self, image, mask=None):
        return self.ctx.extract_orb(image)     # mask is ignored, as in the reference (ORBextractor.h:58)


class LINEextractor:
    """ORB_SLAM2::LINEextractor (include/LineExtractor.h:186-193)."""

    def __init__(self, numOctaves=1, scale=1.2, nLSDFeature=200, min_line_length=0, device=0):
        self.ctx = Context(lsd_num_octaves=numOctaves, lsd_scale=scale, lsd_nfeatures=nLSDFeature, device=device)

    def __call__(self, image, mask=None):
        return self.ctx.extract_lsd(image)


class PlaneDetection:
    """PlaneDetection (include/PlaneExtractor.h:36-56): readDepthImage + runPlaneDetection."""

    def __init__(self, K=None, depthMapFactor=1.0 / 5000.0, device=0):
        kw = dict(depth_map_factor=depthMapFactor, device=device)
        if K is not None:
            kw.update(fx=K[0][0], fy=K[1][1], cx=K[0][2], cy=K[1][2])
        self.ctx = Context(**kw)

    def run(self, depth_u16):
        return self.ctx.compute_planes(depth_u16)


class ORBmatcher:
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30      # src/ORBmatcher.cc:37-39

    def __init__(self, ctx=None):
        self.ctx = ctx or Context()

    def DescriptorDistance(self, a, b):
        return int(self.ctx.hamming_matrix(np.asarray(a).reshape(1, 32), np.asarray(b).reshape(1, 32))[0, 0])


class LSDmatcher:
    TH_HIGH, TH_LOW = 80, 50                          # src/LSDmatcher.cpp:12-14

    def __init__(self, ctx=None):
        self.ctx = ctx or Context()

    def match(self, desc1, desc2, nnr):
        """LSDmatcher::match -> matchNNR (src/LSDmatcher.cpp:828-863, 803-826): (n, matches_12)"""
        return self.ctx.match_nnr(desc1, desc2, nnr)
