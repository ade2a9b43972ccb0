#!/usr/bin/env python3
"""Bit comparison of two builds of libvmm_ba.so.  --cases pose (default): the single-pose solver's three entries,
vmm_ba_quad_poses, vmm_ba_initialize and vmm_ba_localize.  --cases chol: every Cholesky and back-substitution kernel
(csrc/kernels_chol*.hip, kernels_backsolve.hip) through vmm_ba_dense_spd_solve and a tree-ordered bundle adjustment.
--cases calibrate: vmm_ba_calibrate (csrc/kernels_calibrate.hip behind the localisation's three kernels).
--cases rig: vmm_ba_rig_localize and vmm_ba_rig_calibrate (csrc/kernels_rig.hip, rig.hip) at 3 and 8 cameras.
--cases cov: vmm_ba_tag_translation_covariance (csrc/kernels_cov.hip) after a solve.
--cases handle: the other entries that work on a handle after a solve (csrc/covariance.hip, selfcal.hip, initialize.hip
and the evaluation entries of vmm_ba.hip).
--cases triangulate: vmm_ba_triangulate (csrc/kernels_triangulate.hip, point_lm.hpp).
--cases locate: vmm_ba_locate_tags (csrc/kernels_locate.hip behind k_quad_pose).

    python tools/ab_bits.py --a <libvmm_ba.so> --b <libvmm_ba.so> [--cases pose|chol|calibrate|rig|cov|handle|triangulate|locate] [--keep DIR]

Each library runs in a fresh child process of its own (VMM_BA_LIB is read when the package is imported); the child
writes every array the entries return to an .npz.  The parent compares them byte for byte and prints one JSON line:
{"equal": ..., "outputs": {name: {"equal": ..., "sha256": [a, b]}}}; the exit status is 1 on any difference.  A float
output of 3 x 3 blocks that differs also gets "max_gap_3x3", the largest |a - b| over the largest |a| of its block.  The
scenes are the smallest that reach every loop trip and both variants of every kernel; all of
them are generated here from fixed seeds.  The wall times in the initialisation, calibration and self-calibration
reports and in the solver's summary are the fields left out."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = (8075.29, 8083.17, 3016.39, 1996.29)
DIST = (-0.18618, 0.37018, -2.939e-4, 4.153e-4, 0.05704)


def _quad_cases(eng, out):
    """65 and 200 observations (one wave plus a lane; four workgroups), with and without distortion; observation 3 has
    four equal corners (RMS = +inf)."""
    from visual_marker_mapping_amd import pnp
    w = 0.1285
    quad = np.array([[-w / 2, -w / 2, 0], [w / 2, -w / 2, 0], [w / 2, w / 2, 0], [-w / 2, w / 2, 0]])
    for n in (65, 200):
        for name, dist in (("plain", (0.0,) * 5), ("dist", DIST)):
            rng = np.random.default_rng(1000 + n)
            px = np.zeros((n, 8))
            for i in range(n):
                R = pnp.rodrigues(rng.normal(size=3) * 0.4)
                t = np.array([rng.normal() * 0.2, rng.normal() * 0.2, 3.0 + 3.0 * rng.random()])
                px[i] = eng.project_points(INTR, dist, quad @ R.T + t).reshape(8) + rng.normal(size=8) * 0.3
            px[3] = np.tile(px[3, :2], 4)
            qt2, rms2 = eng.quad_poses(INTR, dist, np.full((n, 2), w), px)
            out["quad_%d_%s_qt2" % (n, name)], out["quad_%d_%s_rms2" % (n, name)] = qt2, rms2


def _init_cases(eng, make_scene, out):
    """70 x 12: 70 > 64 observations per tag, the second trip of the lane-strided sums.  520 x 4: 1040 candidates per
    tag, the second trip of k_init_score's candidate loop.  100 x 60 at visibility 0.3: several growth rounds."""
    for name, kw in (("70x12", dict(n_cams=70, n_tags=12)), ("520x4", dict(n_cams=520, n_tags=4)),
                     ("100x60_vis0.30", dict(n_cams=100, n_tags=60, visibility=0.30))):
        s = make_scene(1, seed=4242, **kw)
        cam = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 1.0]), (len(s.cam_gt), 1))
        tag = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0.0]), (len(s.tag_gt), 1))
        tag[s.fixed_tag] = s.tag_gt[s.fixed_tag]
        with eng.BundleAdjuster(s.intr, s.dist, cam, tag, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px) as ba:
            report, cam_ok, tag_ok = ba.initialize(sweeps=1)
            cam_qt, tag_qt = ba.get_state()
        out["init_%s_cam_qt" % name], out["init_%s_tag_qt" % name] = cam_qt, tag_qt
        out["init_%s_cam_reached" % name], out["init_%s_tag_reached" % name] = cam_ok, tag_ok
        out["init_%s_counts" % name] = np.array([report["rounds"], report["cams_reached"], report["tags_reached"]], np.int64)
        out["init_%s_avg_px" % name] = np.array([report["avg_reprojection_px"]])


def _localize_cases(eng, make_scene, out):
    """One batch of images with 1, 2, 64, 256 (the last staged size) and 257 (the first unstaged; second trip of the
    256-thread stride) observations, a tenth of the 64-observation image's pixel coordinates displaced by up to 60 px; robust and plain,
    with 0 and 2 reclassification passes."""
    s = make_scene(1, seed=4243, n_cams=5, n_tags=260)
    sizes, tags, pxs = (1, 2, 64, 256, 257), [], []
    for c, m in enumerate(sizes):
        idx = np.flatnonzero(s.obs_cam == c)[:m]
        assert len(idx) == m, (c, len(idx))
        tags.append(s.obs_tag[idx])
        pxs.append(s.obs_px[idx].copy())
    rng = np.random.default_rng(4244)
    hit = rng.random(pxs[2].shape) < 0.1
    pxs[2][hit] += rng.uniform(-60.0, 60.0, int(hit.sum()))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for robust in (1, 0):
        for passes in (0, 2):
            cam, cov, inl, res = eng.localize(s.intr, s.dist, s.tag_gt, s.tag_wh, start, np.concatenate(tags),
                                              np.concatenate(pxs), robustify=robust, reclassify_passes=passes)
            key = "loc_%s_p%d_" % ("robust" if robust else "plain", passes)
            out[key + "cam_qt"], out[key + "cam_cov"], out[key + "inlier"] = cam, cov, inl
            out[key + "res_int"] = np.array([[r[k] for k in ("status", "n_obs", "n_inlier_obs", "trials")] for r in res], np.int32)
            out[key + "res_f64"] = np.array([[r["rms_px"], r["cost"]] for r in res])


def _calibrate_cases(eng, make_scene, out):
    """258 images of a map of 260 tags, so that the 64-thread kernels (k_calib_begin, k_calib_cov_pose), k_calib_solve's
    four chains and k_calib_control's 256-stride all wrap.  Image 0 has 257 observations (the second trip of the
    256-thread stride, and the unstaged k_localize), image 1 none, image 2's detections are displaced so far that it
    fails min_inlier_tags, a tenth of image 3's pixel coordinates are displaced by up to 60 px; the others have 4 to 12
    observations.  The model starts off the truth.  Robust and plain, with 0 and 2 reclassification passes, all nine
    parameters free and the distortion held; max_trials 8 keeps each call at a few dozen launches."""
    s = make_scene(5, seed=4245, n_cams=258, n_tags=260, visibility=1.0)
    rng = np.random.default_rng(4246)
    sizes = rng.integers(4, 13, len(s.cam_gt))
    sizes[0], sizes[1] = 257, 0
    tags, pxs = [], []
    for c, m in enumerate(sizes):
        idx = np.flatnonzero(s.obs_cam == c)[:m]
        assert len(idx) == m, (c, len(idx))
        tags.append(s.obs_tag[idx])
        pxs.append(s.obs_px[idx].copy())
    pxs[2] += rng.uniform(-400.0, 400.0, pxs[2].shape)
    hit = rng.random(pxs[3].shape) < 0.1
    pxs[3][hit] += rng.uniform(-60.0, 60.0, int(hit.sum()))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    k0 = np.concatenate([s.intr, s.dist]) + 0.25 * np.array([200.0, -150.0, 30.0, -25.0, 0.02, -0.05, 1e-3, -1e-3, 0.02])
    names = ("intr", "dist", "intr_cov", "cam_qt", "cam_cov", "inlier")
    for robust in (1, 0):
        for passes in (0, 2):
            for mask in (0x1FF, 0x00F):
                got = eng.calibrate(k0[:4], k0[4:], s.tag_gt, s.tag_wh, start, np.concatenate(tags), np.concatenate(pxs),
                                    robustify=robust, reclassify_passes=passes, refine_mask=mask, max_trials=8)
                res, rep = got[6], got[7]
                # else the scene does not do what the text above says: pick another one
                assert rep["n_images_used"] == len(sizes) - 2 and not got[4][2].any() and got[4][3].any(), rep
                key = "cal_%s_p%d_m%03x_" % ("robust" if robust else "plain", passes, mask)
                for name, value in zip(names, got):
                    out[key + name] = value
                out[key + "res_int"] = np.array([[r[k] for k in ("status", "n_obs", "n_inlier_obs", "trials")] for r in res], np.int32)
                out[key + "res_f64"] = np.array([[r["rms_px"], r["cost"]] for r in res])
                ints = ("status", "trials", "accepted", "passes", "n_images_used", "n_obs_used")
                floats = ("initial_cost", "final_cost", "initial_rms_px", "final_rms_px")
                assert sorted(ints + floats + ("time_s",)) == sorted(rep), sorted(rep)   # a new field belongs in one of them
                out[key + "report_int"] = np.array([rep[k] for k in ints], np.int64)
                out[key + "report_f64"] = np.array([rep[k] for k in floats], np.float64)


def _rig_cases(eng, make_rig_scene, out):
    """258 frames of a rig of K = 3 (120 tags) and K = 8 cameras (50 tags), so that the 64-thread k_rigcal_begin,
    k_rigcal_solve's four chains and k_rigcal_control's 256-stride all wrap; at K = 8 a record has 1277 doubles and every
    256-strided loop over a record or the 48 x 48 system takes several trips, at K = 3 one.  Frame 0 has 257 observations
    spread over its cameras (the second trip of the 256-thread stride), frame 1 none, frame 2 no image of camera 0, frame
    3's detections are displaced so far that it fails min_inlier_tags, a tenth of frame 4's pixel coordinates (12
    observations per image) are displaced by up to 60 px; the other images have 2 to 6 observations, the first m of their
    slot.  The extrinsics start off the truth.  vmm_ba_rig_localize robust and plain, with 0 and 2 passes;
    vmm_ba_rig_calibrate robust and plain, with 0 and 2 reclassification passes, under the default mask and with a
    middle camera held, and once (K = 3) with the default mask on a batch in which camera 2 has no observation in any
    frame (its unit rows); max_trials 8 keeps each call at a few dozen launches."""
    def yaw(deg, t):
        a = np.radians(deg) / 2
        return [np.cos(a), 0.0, np.sin(a), 0.0, t[0], t[1], t[2]]

    def batch(s, sizes, rng):
        K = s.n_rig_cams
        tags, pxs = [], []
        for slot, m in enumerate(sizes.reshape(-1)):
            idx = np.arange(s.img_start[slot], s.img_start[slot + 1])[:m]
            assert len(idx) == m, (slot, len(idx))
            tags.append(s.obs_tag[idx])
            px = s.obs_px[idx].copy()
            if slot // K == 3:
                px += rng.uniform(-400.0, 400.0, px.shape)
            if slot // K == 4:
                hit = rng.random(px.shape) < 0.1
                px[hit] += rng.uniform(-60.0, 60.0, int(hit.sum()))
            pxs.append(px)
        start = np.concatenate([[0], np.cumsum(sizes.reshape(-1))]).astype(np.int64)
        return start, np.concatenate(tags), np.concatenate(pxs)

    for K, n_tags in ((3, 120), (8, 50)):
        ext = np.array([yaw(a, (0.1 * (k - (K - 1) / 2), 0.02 * (k % 3), 0.0)) for k, a in enumerate(np.linspace(-15.0, 15.0, K))])
        s = make_rig_scene(5, ext, seed=4247 + K, n_cams=258, n_tags=n_tags, visibility=1.0)
        F = s.n_frames
        rng = np.random.default_rng(4250 + K)
        avail = np.diff(s.img_start).reshape(F, K)
        sizes = rng.integers(2, 7, (F, K))
        sizes[0] = avail[0]
        while sizes[0].sum() > 257:
            sizes[0, sizes[0].argmax()] -= 1
        assert sizes[0].sum() == 257 and (sizes[0] > 0).all(), sizes[0]
        sizes[1] = 0
        sizes[2, 0] = 0
        sizes[4] = 12
        ext0 = ext.copy()   # off the truth: a few pixels, so that the default inlier_px still localises the frames
        ext0[1:, :4] += 2e-4 * np.array([0.0, 1.0, -1.0, 0.5]) * (1 + np.arange(1, K))[:, None] / K
        ext0[1:, :4] /= np.linalg.norm(ext0[1:, :4], axis=1)[:, None]
        ext0[1:, 4:] += 1e-3 * np.array([1.0, -0.5, 0.5])
        start, tags, pxs = batch(s, sizes, np.random.default_rng(4260 + K))
        for robust in (1, 0):
            for passes in (0, 2):
                rig, cov, inl, res = eng.rig_localize(s.intr, s.dist, ext0, s.tag_gt, s.tag_wh, start, tags, pxs,
                                                      robustify=robust, reclassify_passes=passes)
                key = "rigloc_k%d_%s_p%d_" % (K, "robust" if robust else "plain", passes)
                out[key + "rig_qt"], out[key + "rig_cov"], out[key + "inlier"] = rig, cov, inl
                out[key + "res_int"] = np.array([[r[k] for k in ("status", "n_obs", "n_inlier_obs", "trials")] for r in res], np.int32)
                out[key + "res_f64"] = np.array([[r["rms_px"], r["cost"]] for r in res])
        held = 1 << (K // 2)
        default = (1 << K) - 2
        runs = [(name, mask, start, tags, pxs, 2) for name, mask in (("default", default), ("held", default & ~held))]
        if K == 3:
            blind = sizes.copy()
            blind[:, 2] = 0
            runs.append(("blind", default) + batch(s, blind, np.random.default_rng(4260 + K)) + (2,))
        names = ("ext_qt", "ext_cov", "rig_qt", "rig_cov", "inlier")
        for name, mask, st, tg, px, lost in runs:
            for robust in (1, 0):
                for passes in (0, 2):
                    got = eng.rig_calibrate(s.intr, s.dist, ext0, s.tag_gt, s.tag_wh, st, tg, px, robustify=robust,
                                            reclassify_passes=passes, refine_mask=mask, max_trials=8)
                    res, rep = got[5], got[6]
                    flags = lambda f: got[4][st[f * K]:st[(f + 1) * K]]
                    # else the scene does not do what the text above says: pick another one
                    assert rep["n_frames_used"] == F - lost and not flags(3).any() and flags(4).any(), rep
                    if name == "blind":
                        assert got[0][2].tobytes() == ext0[2].tobytes() and not rep["cams_refined"] & 4, rep
                    key = "rigcal_k%d_%s_%s_p%d_" % (K, name, "robust" if robust else "plain", passes)
                    for n, value in zip(names, got):
                        out[key + n] = value
                    out[key + "res_int"] = np.array([[r[k] for k in ("status", "n_obs", "n_inlier_obs", "trials")] for r in res], np.int32)
                    out[key + "res_f64"] = np.array([[r["rms_px"], r["cost"]] for r in res])
                    ints = ("status", "trials", "accepted", "passes", "n_frames_used", "n_obs_used", "cams_refined")   # the binding leaves `reserved` out
                    floats = ("initial_cost", "final_cost", "initial_rms_px", "final_rms_px")
                    assert sorted(ints + floats + ("time_s",)) == sorted(rep), sorted(rep)   # a new field belongs in one of them
                    out[key + "report_int"] = np.array([rep[k] for k in ints], np.int64)
                    out[key + "report_f64"] = np.array([rep[k] for k in floats], np.float64)


class _Env:
    """Switches of the engine for one case (a handle and vmm_ba_dense_spd_solve read them when they are created / called)."""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _chol_dense_cases(eng, out):
    """vmm_ba_dense_spd_solve on seeded SPD systems, the smallest orders that reach every kernel and loop trip: 40 (one
    block: the chain's single-block exit), 130 (3 blocks: one hop, one trip behind it), 300 (5: several trips with the
    next tile requested ahead), 1200 (19: the benchmark's size), 3136 (49: launch-per-column steps with paired rank-128
    updates, the hand-over launch, the dataflow tail, the chain over 49 blocks); 300 without the dataflow kernel
    (k_chol_step all the way, rank-64 updates) and without the chain (k_backsolve_step); 1200 on the bulk kernel; an
    indefinite 70 x 70 matrix (info on the failure path)."""
    def system(n):
        rng = np.random.default_rng(7000 + n)
        M = rng.normal(size=(n, n))
        return M @ M.T + n * np.eye(n), rng.normal(size=n)

    cases = [("n40", 40, {}), ("n130", 130, {}), ("n300", 300, {}), ("n1200", 1200, {}), ("n3136", 3136, {}),
             ("n300_no_dataflow", 300, dict(VMM_BA_NO_DATAFLOW=1)), ("n300_no_chain", 300, dict(VMM_BA_NO_CHAIN=1)),
             ("n1200_df_bulk", 1200, dict(VMM_BA_DF_BULK=1))]
    for name, n, env in cases:
        A, b = system(n)
        with _Env(**env):
            x, info = eng.dense_spd_solve(A, b)
        out["dense_%s_x" % name], out["dense_%s_info" % name] = x, np.array([info], np.int32)
    A, b = system(70)
    A[35, 35] = -1.0
    x, info = eng.dense_spd_solve(A, b)
    out["dense_indefinite70_x"], out["dense_indefinite70_info"] = x, np.array([info], np.int32)


def _chol_tree_cases(eng, make_scene, out):
    """A close-up scene whose kept family gets a tree ordering (tree_ordering >= 3): k_chol_dataflow_tree and
    k_backsolve_chain_tree; the same with helper waves; the same with every chain giving up and its pass redone."""
    s = make_scene(1, n_cams=60, n_tags=70, neighbors_min=3, neighbors_max=6)
    base = dict(VMM_BA_ORDER="nd", VMM_BA_SCHUR="sparse")
    for name, env in (("tree", {}), ("tree_help", dict(VMM_BA_DF_HELP=1)),
                      ("tree_chain_redone", dict(VMM_BA_DEBUG_SPIN_LIMIT=1, VMM_BA_DEBUG_SPIN_KERNEL="chain",
                                                 VMM_BA_DEBUG_SPIN_ONCE=0))):
        with _Env(**base, **env):
            with eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                    s.obs_px) as ba:
                res = ba.solve(eng.default_options(max_num_iterations=6), trace_capacity=16)
                cam_qt, tag_qt = ba.get_state()
        assert res["tree_ordering"] >= 3, res["tree_ordering"]   # else the tree kernels did not run: pick another scene
        out["%s_costs" % name] = np.array([it["cost"] for it in res["trace"]])
        out["%s_cam_qt" % name], out["%s_tag_qt" % name] = cam_qt, tag_qt
        out["%s_tree_ordering" % name] = np.array([res["tree_ordering"], res["block_sparse"]], np.int32)
        out["%s_redone" % name] = np.array([res["num_sync_timeouts"] > 0], np.int32)


def _cov_cases(eng, make_scene, out):
    """The scenes of tests/test_gpu_pose_covariance.py (each configuration's own fixed seed): 30 x 14 under both eliminations, plain and robust (a reduced
    system of two or three blocks, a right-hand side of 84 columns: not a multiple of 64); 20 x 10 with the cameras
    eliminated (one block: no update launch); 12 x 24 (tags eliminated by ELIM_AUTO); a 60 x 80 close-up handle on the
    block-sparse path, which switches to the dense system for the call.  The state after the solve is an output too: a
    difference there is not the covariance's."""
    def run(name, s, robust, **kw):
        with eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                s.obs_px, **kw) as ba:
            res = ba.solve(eng.default_options(robustify=robust))
            assert res["termination_type"] == eng.CONVERGENCE, (name, res["termination_type"])
            out["cov_%s_cam_qt" % name], out["cov_%s_tag_qt" % name] = ba.get_state()
            out["cov_%s_tag_translation" % name] = ba.tag_translation_covariance(robustify=bool(robust))
        return res

    for elim, mode in (("cams", eng.ELIM_CAMERAS), ("tags", eng.ELIM_TAGS)):
        for robust in (0, 1):
            s = make_scene(5 if robust else 1, n_cams=30, n_tags=14, visibility=0.7)
            run("30x14_elim_%s_%s" % (elim, "robust" if robust else "plain"), s, robust, elimination=mode)
    run("20x10_elim_cams", make_scene(1), 0, elimination=eng.ELIM_CAMERAS)
    run("12x24_auto", make_scene(1, n_cams=12, n_tags=24, visibility=0.5), 0, elimination=eng.ELIM_AUTO)
    with _Env(VMM_BA_SCHUR="sparse"):
        res = run("60x80_block_sparse", make_scene(2, n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10), 0)
    assert res["block_sparse"] == 1, res["block_sparse"]   # else the handle was dense all along: pick another scene


def _handle_cases(eng, make_scene, out):
    """The two smallest scenes of tests/test_gpu_selfcal.py with a non-zero distortion (12 x 8) and a k_dim above 64 (the
    12 x 30 close-up), under both eliminations.  After a solve from the initial guess: vmm_ba_covariance_blocks for pairs
    that mix eliminated and kept poses (6 distinct poses: a right-hand side of 36 columns, not a multiple of 64),
    vmm_ba_intrinsics_system, vmm_ba_eval_blocks, vmm_ba_reprojection_stats and vmm_ba_cost, robust and plain; then
    vmm_ba_solve_selfcal from the true poses and a camera model off the truth (that test file's start), with every
    parameter free and with the distortion held, on a handle of its own each; vmm_ba_initialize from poses that say
    nothing."""
    scenes = (("distortion_12x8", 5, dict(n_cams=12, n_tags=8, visibility=0.6)),
              ("closeup_12x30", 2, dict(n_cams=12, n_tags=30, neighbors_min=6, neighbors_max=10)))
    perturb = np.array([200.0, -150.0, 30.0, -25.0, 0.02, -0.05, 1e-3, -1e-3, 0.02])
    for name, cfg, kw in scenes:
        s = make_scene(cfg, **kw)
        nc, nt = len(s.cam_init), len(s.tag_init)
        pairs = np.array([[0, 0], [0, nc], [nc + 1, 1], [nc + nt - 1, nc + nt - 1], [nc - 1, 0], [nc, nc + 1]])
        assert len(np.unique(pairs)) == 6
        for elim, mode in (("tags", eng.ELIM_TAGS), ("cams", eng.ELIM_CAMERAS)):
            key = "handle_%s_elim_%s_" % (name, elim)
            new = lambda intr, dist, cam, tag: eng.BundleAdjuster(intr, dist, cam, tag, s.tag_wh, s.fixed_tag, s.obs_cam,
                                                                  s.obs_tag, s.obs_px, elimination=mode)
            with new(s.intr, s.dist, s.cam_init, s.tag_init) as ba:
                res = ba.solve(eng.default_options(robustify=1))
                out[key + "solve"] = np.array([res["termination_type"], res["iterations"]], np.int64)
                out[key + "cam_qt"], out[key + "tag_qt"] = ba.get_state()
                for robust in (0, 1):
                    r = key + ("robust_" if robust else "plain_")
                    out[r + "covariance_blocks"] = ba.covariance_blocks(pairs, robustify=bool(robust))
                    for k, v in ba.intrinsics_system(robustify=bool(robust)).items():
                        out[r + "system_" + k] = np.asarray(v)
                    for k, v in ba.eval_blocks(robustify=bool(robust)).items():
                        out[r + "eval_" + k] = np.asarray(v)
                    out[r + "cost"] = np.array([ba.cost(robustify=bool(robust))])
                pc, pt, avg, corner = ba.reprojection_stats()
                out[key + "stats_per_cam"], out[key + "stats_per_tag"], out[key + "stats_corner"] = pc, pt, corner
                out[key + "stats_avg"] = np.array([avg])
            k0 = np.concatenate([s.intr, s.dist]) + perturb
            for mask in (0x1FF, 0x00F):
                m = key + "selfcal_m%03x_" % mask
                with new(k0[:4], k0[4:], s.cam_gt, s.tag_gt) as ba:
                    intr, dist, cov, rep, summ = ba.solve_selfcal(eng.default_options(robustify=1), refine_mask=mask)
                    out[m + "intr"], out[m + "dist"], out[m + "intr_cov"] = intr, dist, cov
                    out[m + "cam_qt"], out[m + "tag_qt"] = ba.get_state()
                ints, floats = ("status", "outer_iterations", "accepted", "inner_lm_iterations"), ("initial_cost", "final_cost")
                assert sorted(ints + floats + ("time_s",)) == sorted(rep), sorted(rep)   # a new field belongs in one of them
                out[m + "report_int"] = np.array([rep[k] for k in ints], np.int64)
                out[m + "report_f64"] = np.array([rep[k] for k in floats])
                out[m + "last_inner"] = np.array([summ[k] for k in ("termination_type", "iterations", "num_lm_iterations")], np.int64)
                out[m + "last_inner_cost"] = np.array([summ["initial_cost"], summ["final_cost"]])
            cam = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 1.0]), (nc, 1))
            tag = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0.0]), (nt, 1))
            tag[s.fixed_tag] = s.tag_gt[s.fixed_tag]
            with new(s.intr, s.dist, cam, tag) as ba:
                report, cam_ok, tag_ok = ba.initialize(sweeps=1)
                out[key + "init_cam_qt"], out[key + "init_tag_qt"] = ba.get_state()
            out[key + "init_cam_reached"], out[key + "init_tag_reached"] = cam_ok, tag_ok
            out[key + "init_counts"] = np.array([report["rounds"], report["cams_reached"], report["tags_reached"]], np.int64)
            out[key + "init_avg_px"] = np.array([report["avg_reprojection_px"]])


def _triangulate_cases(eng, out):
    """Nine points in one batch against 70 cameras on an arc: in k_triangulate a wave is a point, a workgroup has four
    and the lanes stride a point's views by 64, so nine points make three workgroups, the last with one wave at work.
    Views per point: 1 (TOO_FEW_VIEWS), 2, 3, 64, 65 and 70 (the second trip of the stride), 70 with a third of its
    pixels displaced by up to 60 px, 2 along parallel rays (cameras 68 and 69 share their rotation and the point has the
    same pixel in both: spd3_solve's floor), 3.  max_pair_views 2 and 16, with and without cam_cov, robust and plain, 0
    and 2 reclassification passes."""
    from visual_marker_mapping_amd import _lib
    n_cams = 70
    rng = np.random.default_rng(4270)
    phi = np.radians(np.linspace(-60.0, 60.0, n_cams))
    phi[69] = phi[68]
    cam_qt = np.zeros((n_cams, 7))
    R = np.zeros((n_cams, 3, 3))
    for i, a in enumerate(phi):
        R[i] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        centre = -4.0 * R[i, 2] + np.array([0.0, 0.3 * np.sin(7.0 * i), 0.0]) + (i == 69) * 0.5 * R[i, 0]
        cam_qt[i] = [np.cos(a / 2), 0.0, np.sin(a / 2), 0.0, *(-R[i] @ centre)]
    views = (1, 2, 3, 64, 65, 70, 70, 2, 3)
    X = rng.uniform(-0.5, 0.5, (len(views), 3))
    cams, uvs = [], []
    for p, m in enumerate(views):
        c = np.sort(rng.choice(n_cams, m, replace=False)).astype(np.int32)
        if p == 7:
            c = np.array([68, 69], np.int32)
        uv = np.stack([eng.project_points(INTR, DIST, (R[k] @ X[p] + cam_qt[k, 4:])[None])[0] for k in c])
        uv += rng.normal(size=uv.shape) * 0.3
        if p == 6:
            hit = rng.random(uv.shape) < 1.0 / 3.0
            uv[hit] += rng.uniform(-60.0, 60.0, int(hit.sum()))
        if p == 7:
            uv[1] = uv[0]
        cams.append(c)
        uvs.append(uv)
    start = np.concatenate([[0], np.cumsum(views)]).astype(np.int64)
    cams, uvs = np.concatenate(cams), np.concatenate(uvs)
    cov_in = np.zeros((n_cams, 6, 6))
    for i in range(n_cams):
        m = rng.normal(size=(6, 6)) * 1e-4
        cov_in[i] = m @ m.T + 1e-8 * np.eye(6)
    for pair in (2, 16):
        for with_cov in (0, 1):
            for robust in (1, 0):
                for passes in (0, 2):
                    xyz, cov, cov_cams, inl, res = eng.triangulate(INTR, DIST, cam_qt, start, cams, uvs,
                                                                   cam_cov=cov_in if with_cov else None, max_pair_views=pair,
                                                                   robustify=robust, reclassify_passes=passes)
                    status = [r["status"] for r in res]
                    # else the scene does not do what the text above says: pick another one
                    assert status[0] == _lib.TRI_TOO_FEW_VIEWS and status[7] not in (_lib.TRI_OK, _lib.TRI_TOO_FEW_VIEWS), status
                    assert all(st == _lib.TRI_OK for k, st in enumerate(status) if k not in (0, 7)), status
                    assert passes == 0 or not inl[start[6]:start[7]].all(), "the displaced pixels of point 6 are all inliers"
                    key = "tri_pair%d_%s_%s_p%d_" % (pair, "cov" if with_cov else "nocov", "robust" if robust else "plain", passes)
                    out[key + "xyz"], out[key + "xyz_cov"], out[key + "xyz_cov_cams"], out[key + "inlier"] = xyz, cov, cov_cams, inl
                    out[key + "res_int"] = np.array([[r[k] for k in ("status", "n_obs", "n_inlier_obs", "trials")] for r in res], np.int32)
                    out[key + "res_f64"] = np.array([[r["rms_px"], r["cost"]] for r in res])


def _locate_cases(eng, make_scene, out):
    """Nine tags in one batch against 260 cameras, each the first m of its observations in camera order: 0
    (NO_OBSERVATIONS), 1 (TOO_FEW_INLIERS under min_inlier_tags 2), 2, 64, 65 (one wave plus a lane), 256 (the last
    staged size), 257 (the first unstaged; second trip of the 256-thread stride), 64 with a tenth of its pixel
    coordinates displaced by up to 60 px, 1 collapsed to a point (NO_CANDIDATE).  With and without cam_cov, robust and
    plain, 0 and 2 reclassification passes."""
    from visual_marker_mapping_amd import _lib
    sizes = (0, 1, 2, 64, 65, 256, 257, 64, 1)
    s = make_scene(1, seed=4280, n_cams=260, n_tags=len(sizes))
    order = np.lexsort((s.obs_cam, s.obs_tag))
    first = np.concatenate([[0], np.cumsum(np.bincount(s.obs_tag, minlength=len(sizes)))])
    cams, pxs = [], []
    for t, m in enumerate(sizes):
        idx = order[first[t]:first[t + 1]][:m]
        assert len(idx) == m, (t, len(idx))
        cams.append(s.obs_cam[idx].astype(np.int32))
        pxs.append(s.obs_px[idx].copy())
    rng = np.random.default_rng(4281)
    hit = rng.random(pxs[7].shape) < 0.1
    pxs[7][hit] += rng.uniform(-60.0, 60.0, int(hit.sum()))
    pxs[8][0] = np.tile(pxs[8][0, :2], 4)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cams, pxs = np.concatenate(cams), np.concatenate(pxs)
    cov_in = np.zeros((len(s.cam_gt), 6, 6))
    for i in range(len(cov_in)):
        m = rng.normal(size=(6, 6)) * 1e-4
        cov_in[i] = m @ m.T + 1e-8 * np.eye(6)
    expected = [_lib.LOC_NO_OBSERVATIONS, _lib.LOC_TOO_FEW_INLIERS] + [_lib.LOC_OK] * 6 + [_lib.LOC_NO_CANDIDATE]
    for with_cov in (0, 1):
        for robust in (1, 0):
            for passes in (0, 2):
                tag, cov, cov_cams, inl, res = eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh, start, cams, pxs,
                                                               cam_cov=cov_in if with_cov else None, min_inlier_tags=2,
                                                               robustify=robust, reclassify_passes=passes)
                status = [r["status"] for r in res]
                # else the scene does not do what the text above says: pick another one
                assert status == expected, status
                assert np.isfinite(tag).all() and np.isfinite(cov).all() and np.isfinite(cov_cams).all()
                assert all(np.isfinite([r["rms_px"], r["cost"]]).all() for r in res)
                for t in (0, 8):   # zero flags, the identity pose, zero covariances
                    assert not inl[start[t]:start[t + 1]].any() and tag[t].tolist() == [1, 0, 0, 0, 0, 0, 0], t
                    assert not cov[t].any() and not cov_cams[t].any(), t
                assert not cov[1].any() and not cov_cams[1].any()
                assert with_cov or not cov_cams.any()
                assert passes == 0 or not inl[start[7]:start[8]].all(), "the displaced pixels of tag 7 are all inliers"
                key = "locate_%s_%s_p%d_" % ("cov" if with_cov else "nocov", "robust" if robust else "plain", passes)
                out[key + "tag_qt"], out[key + "tag_cov"], out[key + "tag_cov_cams"], out[key + "inlier"] = tag, cov, cov_cams, inl
                out[key + "res_int"] = np.array([[r[k] for k in ("status", "n_obs", "n_inlier_obs", "trials")] for r in res], np.int32)
                out[key + "res_f64"] = np.array([[r["rms_px"], r["cost"]] for r in res])


def child(path, cases):
    sys.path.insert(0, ROOT)
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    out = {}
    if cases == "pose":
        _quad_cases(eng, out)
        _init_cases(eng, make_scene, out)
        _localize_cases(eng, make_scene, out)
    elif cases == "calibrate":
        _calibrate_cases(eng, make_scene, out)
    elif cases == "rig":
        from visual_marker_mapping_amd.synthetic import make_rig_scene
        _rig_cases(eng, make_rig_scene, out)
    elif cases == "cov":
        _cov_cases(eng, make_scene, out)
    elif cases == "handle":
        _handle_cases(eng, make_scene, out)
    elif cases == "triangulate":
        _triangulate_cases(eng, out)
    elif cases == "locate":
        _locate_cases(eng, make_scene, out)
    else:
        _chol_dense_cases(eng, out)
        _chol_tree_cases(eng, make_scene, out)
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--a", help="first library")
    ap.add_argument("--b", help="second library")
    ap.add_argument("--cases", choices=("pose", "chol", "calibrate", "rig", "cov", "handle", "triangulate", "locate"), default="pose", help="which set of cases (default: pose)")
    ap.add_argument("--keep", help="directory that receives a.npz and b.npz (default: a temporary one)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cases)
    if not args.a or not args.b:
        ap.error("--a and --b are required")
    keep = args.keep or tempfile.mkdtemp(prefix="ab_bits_")
    os.makedirs(keep, exist_ok=True)
    data = {}
    for side, lib in (("a", args.a), ("b", args.b)):
        path = os.path.join(keep, side + ".npz")
        env = dict(os.environ, VMM_BA_LIB=os.path.abspath(lib), PYTHONPATH=ROOT)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--cases", args.cases], env=env, timeout=600)
        if run.returncode != 0:   # nothing more is started on the GPU after a child that failed
            print(json.dumps({"equal": False, "error": "child %s exited with %d" % (side, run.returncode)}))
            return 2
        with np.load(path) as z:
            data[side] = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
    outputs, equal = {}, sorted(data["a"]) == sorted(data["b"])
    for k in sorted(set(data["a"]) | set(data["b"])):
        same = k in data["a"] and k in data["b"] and data["a"][k] == data["b"][k]
        equal = equal and same
        outputs[k] = {"equal": same, "sha256": [hashlib.sha256(data[x][k][2]).hexdigest() if k in data[x] else None
                                                for x in ("a", "b")]}
        if not same and k in data["a"] and k in data["b"] and data["a"][k][:2] == data["b"][k][:2] \
                and data["a"][k][0] == "<f8" and data["a"][k][1][-2:] == (3, 3):
            a, b = (np.frombuffer(data[x][k][2]).reshape(-1, 9) for x in ("a", "b"))
            scale = np.abs(a).max(axis=1)
            outputs[k]["max_gap_3x3"] = float((np.abs(a - b).max(axis=1)[scale > 0] / scale[scale > 0]).max(initial=0.0))
            outputs[k]["blocks_differing"] = int((a != b).any(axis=1).sum())
    print(json.dumps({"equal": equal, "cases": args.cases, "a": args.a, "b": args.b, "n_outputs": len(outputs), "outputs": outputs}))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
