"""ctypes binding of libvmm_ba.so (include/vmm_ba.h).

There is no CPU fallback: if the library is missing or no MI355X is visible the calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VMM_BA_LIB selects another build of the same ABI (A/B timing of kernel variants)
LIB_PATH = os.environ.get("VMM_BA_LIB") or os.path.join(_HERE, "libvmm_ba.so")

ABI_VERSION = 6          # VMM_BA_ABI_VERSION of include/vmm_ba.h
RCCL_ID_BYTES = 128      # VMM_BA_RCCL_ID_BYTES
PRECISION_F64, PRECISION_F32_ACCUM = 0, 1
LANDMARK_TAG_POSES, LANDMARK_POINTS = 0, 1
RIG_MAX_CAMS = 8         # VMM_BA_RIG_MAX_CAMS
SMALL_MAX_KEPT = 24      # VMM_BA_SMALL_MAX_KEPT
OK, ERR_ARGUMENT, ERR_HIP, ERR_COLLECTIVE, ERR_STATE, ERR_NUMERIC = 0, 1, 2, 3, 4, 5
ELIM_AUTO, ELIM_TAGS, ELIM_CAMERAS = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
# VMM_BA_LOC_*: status of one image of vmm_ba_localize (of one frame of vmm_ba_rig_localize, one tag of vmm_ba_locate_tags)
LOC_OK, LOC_NO_OBSERVATIONS, LOC_NO_CANDIDATE, LOC_TOO_FEW_INLIERS, LOC_SINGULAR = 0, 1, 2, 3, 4
LOC_STATUS_NAMES = ("ok", "no_observations", "no_candidate", "too_few_inliers", "singular")
# VMM_BA_TRI_*: status of one point of vmm_ba_triangulate
TRI_OK, TRI_TOO_FEW_VIEWS, TRI_NO_CANDIDATE, TRI_TOO_FEW_INLIERS, TRI_SINGULAR = 0, 1, 2, 3, 4
TRI_STATUS_NAMES = ("ok", "too_few_views", "no_candidate", "too_few_inliers", "singular")
# VMM_BA_CAL_*: status of vmm_ba_calibrate
CAL_OK, CAL_NO_IMAGES, CAL_SINGULAR, CAL_NO_CONVERGENCE = 0, 1, 2, 3
CAL_STATUS_NAMES = ("ok", "no_images", "singular", "no_convergence")
# VMM_BA_PRED_*: status of one pose of vmm_ba_predict_localization
PRED_OK, PRED_NO_VISIBLE_TAG, PRED_TOO_FEW_TAGS, PRED_SINGULAR = 0, 1, 2, 3
PRED_STATUS_NAMES = ("ok", "no_visible_tag", "too_few_tags", "singular")


class Problem(C.Structure):
    _fields_ = [("intr", C.c_double * 4), ("dist", C.c_double * 5), ("n_cams", C.c_int32),
                ("n_tags", C.c_int32), ("cam_qt", C.POINTER(C.c_double)),
                ("tag_qt", C.POINTER(C.c_double)), ("tag_wh", C.POINTER(C.c_double)),
                ("fixed_tag", C.c_int32), ("n_obs", C.c_int64), ("obs_cam", C.POINTER(C.c_int32)),
                ("obs_tag", C.POINTER(C.c_int32)), ("obs_px", C.POINTER(C.c_double))]


class CreateOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("elimination", C.c_int32), ("rank", C.c_int32),
                ("world_size", C.c_int32), ("precision", C.c_int32), ("landmarks", C.c_int32),
                ("n_structure_obs", C.c_int64), ("structure_obs_cam", C.POINTER(C.c_int32)),
                ("structure_obs_tag", C.POINTER(C.c_int32))]


class Options(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("robustify", C.c_int32), ("huber_a", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("max_num_consecutive_invalid_steps", C.c_int32),
                ("jacobi_scaling", C.c_int32), ("num_threads", C.c_int32), ("poll_interval", C.c_int32)]


class Iteration(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("step_is_valid", C.c_int32),
                ("step_is_successful", C.c_int32), ("reserved", C.c_int32), ("cost", C.c_double),
                ("cost_change", C.c_double), ("gradient_max_norm", C.c_double),
                ("step_norm", C.c_double), ("relative_decrease", C.c_double),
                ("trust_region_radius", C.c_double), ("model_cost_change", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("termination_type", C.c_int32), ("iterations", C.c_int32),
                ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
                ("num_lm_iterations", C.c_int32), ("num_jacobian_evals", C.c_int32),
                ("num_cost_evals", C.c_int32), ("elimination", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("time_solve_s", C.c_double),
                ("trace", C.POINTER(Iteration)), ("trace_capacity", C.c_int32), ("reserved", C.c_int32),
                ("time_eval_s", C.c_double), ("time_eliminate_s", C.c_double), ("time_factor_solve_s", C.c_double),
                ("time_step_s", C.c_double), ("time_control_s", C.c_double),
                ("num_sync_timeouts", C.c_int32), ("sync_timeout_kernels", C.c_int32),
                ("block_sparse", C.c_int32), ("tree_ordering", C.c_int32)]


class KernelTimes(C.Structure):
    _fields_ = [("eval_elim_ms", C.c_double), ("eval_keep_ms", C.c_double), ("cost_ms", C.c_double),
                ("form_z_ms", C.c_double), ("syrk_ms", C.c_double), ("cholesky_ms", C.c_double),
                ("backsub_ms", C.c_double), ("lm_iteration_ms", C.c_double), ("n_obs", C.c_int64),
                ("reduced_dim", C.c_int32), ("elim_dim", C.c_int32), ("schur_sparse", C.c_int32),
                ("syrk_wide", C.c_int32), ("schur_flops", C.c_double), ("chol_flops", C.c_double)]


class InitOptions(C.Structure):
    _fields_ = [("sweeps", C.c_int32), ("min_tag_observations", C.c_int32), ("score_cap_px", C.c_double),
                ("refine_iterations", C.c_int32), ("reserved", C.c_int32)]


class InitReport(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("cams_reached", C.c_int32), ("tags_reached", C.c_int32),
                ("reserved", C.c_int32), ("avg_reprojection_px", C.c_double), ("time_s", C.c_double)]


class LocalizeOptions(C.Structure):
    _fields_ = [("refine_iterations", C.c_int32), ("robustify", C.c_int32), ("huber_a", C.c_double),
                ("score_cap_px", C.c_double), ("inlier_px", C.c_double), ("reclassify_passes", C.c_int32),
                ("min_inlier_tags", C.c_int32)]


class LocalizeResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_obs", C.c_int32), ("n_inlier_obs", C.c_int32), ("trials", C.c_int32),
                ("rms_px", C.c_double), ("cost", C.c_double)]


class TriangulateOptions(C.Structure):
    _fields_ = [("refine_iterations", C.c_int32), ("robustify", C.c_int32), ("huber_a", C.c_double),
                ("score_cap_px", C.c_double), ("inlier_px", C.c_double), ("reclassify_passes", C.c_int32),
                ("min_inlier_views", C.c_int32), ("max_pair_views", C.c_int32), ("reserved", C.c_int32)]


class TriangulateResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_obs", C.c_int32), ("n_inlier_obs", C.c_int32), ("trials", C.c_int32),
                ("rms_px", C.c_double), ("cost", C.c_double)]


class PredictOptions(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("sigma_px", C.c_double), ("margin_px", C.c_double),
                ("min_depth", C.c_double), ("max_view_angle_deg", C.c_double), ("min_side_px", C.c_double),
                ("min_tags", C.c_int32), ("reserved", C.c_int32)]


class PredictResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_visible", C.c_int32), ("sigma_pos_m", C.c_double), ("sigma_rot_rad", C.c_double)]


class CalibrateOptions(C.Structure):
    _fields_ = [("loc", LocalizeOptions), ("max_trials", C.c_int32), ("refine_mask", C.c_int32),
                ("robustify", C.c_int32), ("reclassify_passes", C.c_int32), ("min_inlier_tags", C.c_int32),
                ("reserved", C.c_int32), ("huber_a", C.c_double), ("inlier_px", C.c_double)]


class CalibrateReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("trials", C.c_int32), ("accepted", C.c_int32), ("passes", C.c_int32),
                ("n_images_used", C.c_int32), ("n_obs_used", C.c_int32), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("initial_rms_px", C.c_double), ("final_rms_px", C.c_double),
                ("time_s", C.c_double)]


class RigCalibrateOptions(C.Structure):
    _fields_ = [("loc", LocalizeOptions), ("max_trials", C.c_int32), ("refine_mask", C.c_int32),
                ("robustify", C.c_int32), ("reclassify_passes", C.c_int32), ("min_inlier_tags", C.c_int32),
                ("reserved", C.c_int32), ("huber_a", C.c_double), ("inlier_px", C.c_double)]


class RigCalibrateReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("trials", C.c_int32), ("accepted", C.c_int32), ("passes", C.c_int32),
                ("n_frames_used", C.c_int32), ("n_obs_used", C.c_int32), ("cams_refined", C.c_int32),
                ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("initial_rms_px", C.c_double), ("final_rms_px", C.c_double), ("time_s", C.c_double)]


class SelfcalOptions(C.Structure):
    _fields_ = [("max_outer_iterations", C.c_int32), ("refine_mask", C.c_int32), ("parameter_tolerance", C.c_double),
                ("function_tolerance", C.c_double)]


class SelfcalReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("outer_iterations", C.c_int32), ("accepted", C.c_int32),
                ("inner_lm_iterations", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("time_s", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

# One line per export of include/vmm_ba.h, in its order: name -> (restype, argtypes).  A handle and every array travel as
# void pointers (numpy's .ctypes.data_as), structs as typed pointers.
_h = _a = C.c_void_p
_i, _i32, _i64, _d, _P = C.c_int, C.c_int32, C.c_int64, C.c_double, C.POINTER
_MAP = [_i32, _a, _a]                   # n_tags, tag_qt, tag_wh
_BATCH = [_i32, _a, _a, _a]             # n_imgs / n_frames, img_start, obs_tag, obs_px
SIGNATURES = {
    "vmm_ba_last_error": (C.c_char_p, []),
    "vmm_ba_abi_version": (_i, []),
    "vmm_ba_default_options": (None, [_P(Options)]),
    "vmm_ba_default_create_options": (None, [_P(CreateOptions)]),
    "vmm_ba_create": (_i, [_P(Problem), _P(CreateOptions), _P(C.c_void_p)]),
    "vmm_ba_destroy": (None, [_h]),
    "vmm_ba_set_state": (_i, [_h, _a, _a]),
    "vmm_ba_get_state": (_i, [_h, _a, _a]),
    "vmm_ba_get_points": (_i, [_h, _a]),
    "vmm_ba_set_allreduce": (_i, [_h, ALLREDUCE_FN, C.c_void_p]),
    "vmm_ba_rccl_available": (_i, []),
    "vmm_ba_rccl_unique_id": (_i, [_a]),
    "vmm_ba_enable_rccl": (_i, [_h, _a]),
    "vmm_ba_set_observation_mask": (_i, [_h, _a]),
    "vmm_ba_set_constant_poses": (_i, [_h, _a, _a]),
    "vmm_ba_solve": (_i, [_h, _P(Options), _P(Summary)]),
    "vmm_ba_solve_small": (_i, [_i32, _P(Problem), _a, _a, _P(Options), _i32, _a, _a, _P(Summary), _i]),
    "vmm_ba_cost": (_i, [_h, _i, _d, _P(_d)]),
    "vmm_ba_reprojection_stats": (_i, [_h, _a, _a, _P(_d), _a]),
    "vmm_ba_tag_translation_covariance": (_i, [_h, _i, _d, _a]),
    "vmm_ba_covariance_blocks": (_i, [_h, _i, _d, _i64, _a, _a, _a]),
    "vmm_ba_project_points": (_i, [_a, _a, _i64, _a, _a, _i]),
    "vmm_ba_quad_poses": (_i, [_a, _a, _i64, _a, _a, _a, _a, _i]),
    "vmm_ba_default_init_options": (None, [_P(InitOptions)]),
    "vmm_ba_initialize": (_i, [_h, _P(InitOptions), _P(InitReport), _a, _a]),
    "vmm_ba_default_localize_options": (None, [_P(LocalizeOptions)]),
    "vmm_ba_localize": (_i, [_a, _a] + _MAP + _BATCH + [_P(LocalizeOptions), _a, _a, _a, _a, _i]),
    "vmm_ba_rig_localize": (_i, [_i32, _a, _a, _a] + _MAP + _BATCH + [_P(LocalizeOptions), _a, _a, _a, _a, _i]),
    "vmm_ba_default_rig_calibrate_options": (None, [_P(RigCalibrateOptions)]),
    "vmm_ba_rig_calibrate": (_i, [_i32, _a, _a, _a] + _MAP + _BATCH + [_P(RigCalibrateOptions), _a, _a, _a, _a, _a, _a,
                                  _P(RigCalibrateReport), _i]),
    "vmm_ba_default_triangulate_options": (None, [_P(TriangulateOptions)]),
    "vmm_ba_triangulate": (_i, [_a, _a, _i32, _a, _a] + _BATCH + [_P(TriangulateOptions), _a, _a, _a, _a, _a, _i]),
    "vmm_ba_locate_tags": (_i, [_a, _a, _i32, _a, _a, _i32, _a, _a, _a, _a, _P(LocalizeOptions), _a, _a, _a, _a, _a, _i]),
    "vmm_ba_default_predict_options": (None, [_P(PredictOptions)]),
    "vmm_ba_predict_localization": (_i, [_a, _a] + _MAP + [_a, _i32, _a, _P(PredictOptions), _a, _a, _a, _a, _i]),
    "vmm_ba_predict_localization_joint": (_i, [_a, _a] + _MAP + [_a, _i32, _a, _a, _P(PredictOptions), _a, _a, _a, _a, _i]),
    "vmm_ba_default_calibrate_options": (None, [_P(CalibrateOptions)]),
    "vmm_ba_calibrate": (_i, [_a, _a] + _MAP + _BATCH + [_P(CalibrateOptions), _a, _a, _a, _a, _a, _a, _a,
                              _P(CalibrateReport), _i]),
    "vmm_ba_set_intrinsics": (_i, [_h, _a, _a]),
    "vmm_ba_get_intrinsics": (_i, [_h, _a, _a]),
    "vmm_ba_intrinsics_system": (_i, [_h, _i, _d, _P(_d), _a, _a, _a, _a]),
    "vmm_ba_default_selfcal_options": (None, [_P(SelfcalOptions)]),
    "vmm_ba_solve_selfcal": (_i, [_h, _P(Options), _P(SelfcalOptions), _P(Summary), _P(SelfcalReport), _a, _a, _a]),
    "vmm_ba_eval_blocks": (_i, [_h, _i, _d, _P(_d), _a, _a, _a, _a, _a]),
    "vmm_ba_dense_spd_solve": (_i, [_i, _i, _a, _a, _a, _P(_i)]),
    "vmm_ba_dense_syrk": (_i, [_i, _i, _i, _a, _a]),
    "vmm_ba_pose_plus": (_i, [_i64, _a, _a, _a, _i]),
    "vmm_ba_debug_overlap": (_i, [_h, _i, _a]),
    "vmm_ba_debug_chol_schedule": (_i, [_i, _i, _i, _a, _i, _a, _a]),
    "vmm_ba_debug_chol_tile": (_i, [_i, _a, _i, _a, _a]),
    "vmm_ba_time_kernels": (_i, [_h, _P(Options), _i, _P(KernelTimes)]),
}
EXPORTS = list(SIGNATURES)   # every symbol include/vmm_ba.h declares
# Additive within ABI 6: a library built before these entries (VMM_BA_LIB; tools/bench_covariance.py times the parent
# commit's build) still loads, and calling the missing entry raises AttributeError.
OPTIONAL = {"vmm_ba_covariance_blocks", "vmm_ba_rig_localize", "vmm_ba_default_rig_calibrate_options", "vmm_ba_rig_calibrate",
            "vmm_ba_default_calibrate_options", "vmm_ba_calibrate", "vmm_ba_default_triangulate_options",
            "vmm_ba_triangulate", "vmm_ba_locate_tags", "vmm_ba_default_predict_options", "vmm_ba_predict_localization",
            "vmm_ba_predict_localization_joint",
            "vmm_ba_set_intrinsics", "vmm_ba_get_intrinsics", "vmm_ba_intrinsics_system",
            "vmm_ba_default_selfcal_options", "vmm_ba_solve_selfcal", "vmm_ba_solve_small"}

_LIB = None


class VmmBaError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("libvmm_ba status %d: %s" % (status, message))
        self.status = status


def lib():
    """Loads libvmm_ba.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with __graft_entry__.build() or "
                              "make -C visual_marker_mapping_amd/csrc" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.vmm_ba_abi_version.restype = C.c_int
        if L.vmm_ba_abi_version() != ABI_VERSION:
            raise ImportError("%s has ABI version %d, this binding needs %d: rebuild it"
                              % (LIB_PATH, L.vmm_ba_abi_version(), ABI_VERSION))
        for name, (restype, argtypes) in SIGNATURES.items():
            if name in OPTIONAL and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def check(status):
    if status != OK:
        raise VmmBaError(status, lib().vmm_ba_last_error().decode("utf-8", "replace"))
