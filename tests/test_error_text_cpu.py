"""CPU-only: the return code and the exact vmm_ba_last_error() text of every argument error that an entry point of
csrc/covariance.hip, selfcal.hip, initialize.hip, standalone.hip and diagnostics.hip (and the state readers of
vmm_ba.hip) reports before its first device call.  The library loads without a GPU; no handle can be created here, so
the handle entries are reached with a null handle, or -- for the checks that come before the handle is looked at --
with a pointer to zeroed memory that stands in for one.  The texts were recorded from the library before its host
source was split by entry family: a move must keep every one of them."""
import ctypes as C

import numpy as np
import pytest

from visual_marker_mapping_amd import _lib

ARG = _lib.ERR_ARGUMENT
_zeros = np.zeros(1 << 16, np.uint8)           # never read: every case below returns before the handle is dereferenced
H = _zeros.ctypes.data_as(C.c_void_p)
D = lambda n=1: np.zeros(max(n, 1))            # a double array the entry may name but never touches
I32 = lambda n=1: np.zeros(max(n, 1), np.int32)
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
INTR, DIST = np.array([1000.0, 1000.0, 500.0, 400.0]), np.zeros(5)


def _selfcal(**kw):
    """The defaults (checked against the library below) with `kw` over them; the library is not loaded for this: the case
    table is built when the module is imported."""
    o = _lib.SelfcalOptions(max_outer_iterations=30, refine_mask=0x1FF, parameter_tolerance=1e-10, function_tolerance=1e-12)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _cases():
    """(id, entry, arguments, text)"""
    d, i32 = P(D(64)), P(I32(8))
    intr, dist = P(INTR), P(DIST)
    c = C.byref(C.c_double(0))
    ci = C.byref(C.c_int(0))
    nan_intr = P(np.array([1000.0, np.nan, 500.0, 400.0]))
    inf_dist = P(np.array([0.0, 0.0, np.inf, 0.0, 0.0]))
    opts, summ, rep = C.byref(_lib.Options()), C.byref(_lib.Summary()), C.byref(_lib.SelfcalReport())
    kt = C.byref(_lib.KernelTimes())
    out = []
    add = lambda name, fn, args, text: out.append(pytest.param(fn, args, text, id=name))
    # ---- covariance.hip
    add("ttc_null_handle", "vmm_ba_tag_translation_covariance", (None, 0, 1.0, d), "bad argument")
    add("ttc_null_cov", "vmm_ba_tag_translation_covariance", (H, 0, 1.0, None), "bad argument")
    add("cb_null_handle", "vmm_ba_covariance_blocks", (None, 0, 1.0, 1, i32, i32, d), "bad argument")
    add("cb_negative_pairs", "vmm_ba_covariance_blocks", (H, 0, 1.0, -1, i32, i32, d), "bad argument")
    add("cb_too_many_pairs", "vmm_ba_covariance_blocks", (H, 0, 1.0, (2 ** 31 - 1) // 4 + 1, i32, i32, d), "bad argument")
    add("cb_null_pose_a", "vmm_ba_covariance_blocks", (H, 0, 1.0, 1, None, i32, d), "bad argument")
    add("cb_null_pose_b", "vmm_ba_covariance_blocks", (H, 0, 1.0, 1, i32, None, d), "bad argument")
    add("cb_null_cov", "vmm_ba_covariance_blocks", (H, 0, 1.0, 1, i32, i32, None), "bad argument")
    add("is_null_handle", "vmm_ba_intrinsics_system", (None, 1, 1.0, c, d, d, d, d), "intrinsics_system: null handle")
    # ---- selfcal.hip
    add("si_null_handle", "vmm_ba_set_intrinsics", (None, intr, dist), "set_intrinsics: null argument")
    add("si_null_intr", "vmm_ba_set_intrinsics", (H, None, dist), "set_intrinsics: null argument")
    add("si_null_dist", "vmm_ba_set_intrinsics", (H, intr, None), "set_intrinsics: null argument")
    add("si_nan_intr", "vmm_ba_set_intrinsics", (H, nan_intr, dist), "set_intrinsics: the camera model is not finite")
    add("si_inf_dist", "vmm_ba_set_intrinsics", (H, intr, inf_dist), "set_intrinsics: the camera model is not finite")
    add("gi_null_handle", "vmm_ba_get_intrinsics", (None, d, d), "get_intrinsics: null argument")
    add("gi_null_intr", "vmm_ba_get_intrinsics", (H, None, d), "get_intrinsics: null argument")
    add("gi_null_dist", "vmm_ba_get_intrinsics", (H, d, None), "get_intrinsics: null argument")
    sc = lambda **kw: (H, opts, C.byref(_selfcal(**kw)), summ, rep, d, d, d)
    add("ss_null_handle", "vmm_ba_solve_selfcal", (None, opts, None, summ, rep, d, d, d), "solve_selfcal: null argument")
    add("ss_null_report", "vmm_ba_solve_selfcal", (H, opts, None, summ, None, d, d, d), "solve_selfcal: null argument")
    add("ss_null_intr", "vmm_ba_solve_selfcal", (H, opts, None, summ, rep, None, d, d), "solve_selfcal: null argument")
    add("ss_null_dist", "vmm_ba_solve_selfcal", (H, opts, None, summ, rep, d, None, d), "solve_selfcal: null argument")
    for name, kw in (("negative_outer", dict(max_outer_iterations=-1)), ("negative_mask", dict(refine_mask=-1)),
                     ("mask_too_wide", dict(refine_mask=0x200)), ("negative_ptol", dict(parameter_tolerance=-1.0)),
                     ("nan_ptol", dict(parameter_tolerance=float("nan"))), ("negative_ftol", dict(function_tolerance=-1.0)),
                     ("nan_ftol", dict(function_tolerance=float("nan")))):
        add("ss_" + name, "vmm_ba_solve_selfcal", sc(**kw), "solve_selfcal: bad options")
    # ---- initialize.hip
    add("init_null_handle", "vmm_ba_initialize", (None, None, None, None, None), "null handle")
    # ---- standalone.hip
    add("pp_null_intr", "vmm_ba_project_points", (None, dist, 1, d, d, 0), "bad argument")
    add("pp_null_dist", "vmm_ba_project_points", (intr, None, 1, d, d, 0), "bad argument")
    add("pp_negative_n", "vmm_ba_project_points", (intr, dist, -1, d, d, 0), "bad argument")
    add("pp_null_points", "vmm_ba_project_points", (intr, dist, 1, None, d, 0), "bad argument")
    add("pp_null_uv", "vmm_ba_project_points", (intr, dist, 1, d, None, 0), "bad argument")
    add("plus_negative_n", "vmm_ba_pose_plus", (-1, d, d, d, 0), "bad argument")
    add("plus_null_qt", "vmm_ba_pose_plus", (1, None, d, d, 0), "bad argument")
    add("plus_null_delta", "vmm_ba_pose_plus", (1, d, None, d, 0), "bad argument")
    add("plus_null_out", "vmm_ba_pose_plus", (1, d, d, None, 0), "bad argument")
    add("quad_null_intr", "vmm_ba_quad_poses", (None, dist, 1, d, d, d, d, 0), "bad argument")
    add("quad_null_dist", "vmm_ba_quad_poses", (intr, None, 1, d, d, d, d, 0), "bad argument")
    add("quad_negative_n", "vmm_ba_quad_poses", (intr, dist, -1, d, d, d, d, 0), "bad argument")
    for k, name in enumerate(("tag_wh", "obs_px", "qt2", "rms2")):
        args = [intr, dist, 1, d, d, d, d, 0]
        args[3 + k] = None
        add("quad_null_" + name, "vmm_ba_quad_poses", tuple(args), "bad argument")
    add("spd_zero_n", "vmm_ba_dense_spd_solve", (0, 0, d, d, d, ci), "bad argument")
    add("spd_negative_n", "vmm_ba_dense_spd_solve", (0, -3, d, d, d, ci), "bad argument")
    add("spd_null_A", "vmm_ba_dense_spd_solve", (0, 2, None, d, d, ci), "bad argument")
    add("spd_null_b", "vmm_ba_dense_spd_solve", (0, 2, d, None, d, ci), "bad argument")
    add("spd_null_x", "vmm_ba_dense_spd_solve", (0, 2, d, d, None, ci), "bad argument")
    add("syrk_zero_k", "vmm_ba_dense_syrk", (0, 0, 2, d, d), "bad argument")
    add("syrk_zero_n", "vmm_ba_dense_syrk", (0, 2, 0, d, d), "bad argument")
    add("syrk_null_Z", "vmm_ba_dense_syrk", (0, 2, 2, None, d), "bad argument")
    add("syrk_null_C", "vmm_ba_dense_syrk", (0, 2, 2, d, None), "bad argument")
    # ---- diagnostics.hip
    add("tk_null_handle", "vmm_ba_time_kernels", (None, opts, 1, kt), "bad argument")
    add("tk_null_out", "vmm_ba_time_kernels", (H, opts, 1, None), "bad argument")
    add("tk_zero_reps", "vmm_ba_time_kernels", (H, opts, 0, kt), "bad argument")
    add("ov_null_handle", "vmm_ba_debug_overlap", (None, 1, d), "bad argument")
    add("ov_null_ms", "vmm_ba_debug_overlap", (H, 1, None), "bad argument")
    add("ov_zero_reps", "vmm_ba_debug_overlap", (H, 0, d), "bad argument")
    add("sched_zero_blocks", "vmm_ba_debug_chol_schedule", (0, 0, 256, i32, 1, ci, ci), "bad argument")
    add("sched_zero_cus", "vmm_ba_debug_chol_schedule", (4, 0, 0, i32, 1, ci, ci), "bad argument")
    add("sched_negative_cap", "vmm_ba_debug_chol_schedule", (4, 0, 256, i32, -1, ci, ci), "bad argument")
    add("sched_null_launches", "vmm_ba_debug_chol_schedule", (4, 0, 256, None, 1, ci, ci), "bad argument")
    add("sched_null_count", "vmm_ba_debug_chol_schedule", (4, 0, 256, i32, 1, None, ci), "bad argument")
    add("sched_df_too_large", "vmm_ba_debug_chol_schedule", (4, 3, 256, i32, 1, ci, ci), "bad argument")
    launch = np.array([0, -1, -1, -1, -1, 0, 0, 2], np.int32)
    add("tile_null_launch", "vmm_ba_debug_chol_tile", (4, None, 0, ci, ci), "bad argument")
    add("tile_null_bi", "vmm_ba_debug_chol_tile", (4, P(launch), 0, None, ci), "bad argument")
    add("tile_null_bj", "vmm_ba_debug_chol_tile", (4, P(launch), 0, ci, None), "bad argument")
    add("tile_negative_t", "vmm_ba_debug_chol_tile", (4, P(launch), -1, ci, ci), "bad argument")
    add("tile_t_past_the_end", "vmm_ba_debug_chol_tile", (4, P(launch), 2, ci, ci), "bad argument")
    # ---- vmm_ba.hip: the entries whose flush_state block was rewritten
    add("get_points_null_handle", "vmm_ba_get_points", (None, d), "null argument")
    add("get_points_null_points", "vmm_ba_get_points", (H, None), "null argument")
    add("get_state_null_handle", "vmm_ba_get_state", (None, d, d), "null handle")
    add("cost_null_handle", "vmm_ba_cost", (None, 1, 1.0, c), "null argument")
    add("cost_null_cost", "vmm_ba_cost", (H, 1, 1.0, None), "null argument")
    add("stats_null_handle", "vmm_ba_reprojection_stats", (None, d, d, c, d), "null handle")
    add("eval_null_handle", "vmm_ba_eval_blocks", (None, 1, 1.0, c, d, d, d, d, d), "null handle")
    return out   # (data_as and byref keep what they point to alive)


_CASES = _cases()


@pytest.mark.parametrize("entry, args, text", _CASES)
def test_argument_error_keeps_its_code_and_text(entry, args, text):
    L = _lib.lib()
    # a text left behind by this call, not by an earlier one
    assert L.vmm_ba_get_state(None, None, None) == ARG and L.vmm_ba_last_error() == b"null handle"
    if entry == "vmm_ba_get_state":
        assert L.vmm_ba_cost(None, 0, 1.0, None) == ARG and L.vmm_ba_last_error() == b"null argument"
    assert getattr(L, entry)(*args) == ARG
    assert L.vmm_ba_last_error().decode() == text


def test_default_option_entries_accept_null_and_keep_their_defaults():
    L = _lib.lib()
    L.vmm_ba_default_selfcal_options(None)
    L.vmm_ba_default_init_options(None)
    so = _lib.SelfcalOptions()
    L.vmm_ba_default_selfcal_options(C.byref(so))
    assert bytes(so) == bytes(_selfcal())
    assert (so.max_outer_iterations, so.refine_mask, so.parameter_tolerance, so.function_tolerance) == (30, 0x1FF, 1e-10, 1e-12)
    io = _lib.InitOptions()
    L.vmm_ba_default_init_options(C.byref(io))
    assert (io.sweeps, io.min_tag_observations, io.score_cap_px, io.refine_iterations) == (1, 2, 100.0, 30)


def test_an_empty_batch_of_a_handle_free_entry_is_answered_without_a_device():
    L = _lib.lib()
    assert L.vmm_ba_project_points(P(INTR), P(DIST), 0, None, None, 0) == _lib.OK
    assert L.vmm_ba_pose_plus(0, None, None, None, 0) == _lib.OK
    assert L.vmm_ba_quad_poses(P(INTR), P(DIST), 0, None, None, None, None, 0) == _lib.OK
