"""GPU tests of the bundle adjustment that refines the camera model (vmm_ba_set_intrinsics, vmm_ba_intrinsics_system,
vmm_ba_solve_selfcal, BundleAdjuster's members, TagReconstructor.doBundleAdjustment(refineCameraModel=True) and the
selfcalibration command line).

Yardstick: tests/yardstick.py -- joint_system / host_joint_lm / reduced_system / model_covariance, numpy around
oracle/oracle.py, proven against central differences in tests/test_yardstick_cpu.py; they never call the code under test.

Tolerances.
  C, g_k, cost   entry by entry in the metric of tests/eval_cases.py: |device - reference| over the entry's MAGNITUDE (the
                 same sum over absolute values), an entry of magnitude 0 exactly 0.  The bound is what
                 profiles/eval_accuracy.jsonl records for the blocks of the same kind on ordinary scenes (parts "widths"
                 and "task edges", f64): the largest deviation of the two CPU references from the longdouble one is
                 1.26e-12 over V, U and W (sums of J J products, as C), 2.06e-15 over g_cam and g_tag (sums of J r
                 products, as g_k) and 1.458e-13 for the cost; times eval_cases.MARGIN = 8 as tests/test_gpu_eval_accuracy.py.
  S_k, r_k       come out of a cancellation (C is about 1e4 x S_k on the principal-point entries) and are not compared
                 entry by entry: inv(S_k) to 1e-6 x max|ref| as the existing covariance tests, inv(S_k) r_k in standard
                 deviations to ten times the gap between the two host optimisers (HOST_SIGMA_GAP).
  exact data     1e-9, the bound of the calibration's exact test
  noisy data     poses to 1e-6 between two optima, cost to 1e-9 relative (second order in the gap),
                 every free parameter within 10 x HOST_SIGMA_GAP standard deviations, the covariance to 1e-6 x max|ref|
"""
import os
import shutil

import numpy as np
import pytest

from yardstick import (BOUND_C, BOUND_COST, BOUND_G, HOST_SIGMA_GAP, PERTURB, host_joint_lm, joint_system, model_covariance,
                       pose_gap, reduced_system, same_bytes, scene_args)

pytestmark = pytest.mark.gpu

SCENES = {
    "config1_20x10": (1, dict()),                                                          # the reduced system fits one 64-row block
    "closeup_12x30": (2, dict(n_cams=12, n_tags=30, neighbors_min=6, neighbors_max=10)),   # 180 / 72 kept rows, k_dim above 64
    "distortion_12x8": (5, dict(n_cams=12, n_tags=8, visibility=0.6)),                     # non-zero distortion
}
ELIMS = ("tags", "cams")
TIGHT = dict(function_tolerance=1e-16, parameter_tolerance=1e-14, max_num_iterations=200)
_cache = {}


def _scene(name, exact=False):
    from visual_marker_mapping_amd.synthetic import make_scene
    key = ("scene", name, exact)
    if key not in _cache:
        cfg, kw = SCENES[name]
        _cache[key] = make_scene(cfg, **dict(kw, noise_px=0.0, outlier_frac=0.0)) if exact else make_scene(cfg, **kw)
    return _cache[key]


def _truth(s):
    return np.concatenate([s.intr, s.dist])


def _handle(s, elim, k=None, cam=None, tag=None, obs=None):
    from visual_marker_mapping_amd import engine as eng
    k = _truth(s) if k is None else k
    oc, ot, px = (s.obs_cam, s.obs_tag, s.obs_px) if obs is None else obs
    return eng.BundleAdjuster(k[:4], k[4:], s.cam_gt if cam is None else cam, s.tag_gt if tag is None else tag, s.tag_wh,
                              s.fixed_tag, oc, ot, px, elimination=eng.ELIM_TAGS if elim == "tags" else eng.ELIM_CAMERAS)


def _options(robust, **kw):
    from visual_marker_mapping_amd import engine as eng
    return eng.default_options(robustify=int(robust), **dict(TIGHT, **kw))


def _reference(O, name, robust, mask=0x1FF, k_start=None):
    """host_joint_lm from the truth, once per case: (k, cams, tags, cost, H)."""
    key = ("ref", name, robust, mask, None if k_start is None else k_start.tobytes())
    if key not in _cache:
        s = _scene(name)
        _cache[key] = host_joint_lm(O, _truth(s) if k_start is None else k_start, s.cam_gt, s.tag_gt, *scene_args(s),
                                    robust=robust, mask=mask)
    return _cache[key]


# ---- 1. the system ---------------------------------------------------------------------------------------------------

def _variants(s):
    n, nc, nt = len(s.obs_cam), len(s.cam_gt), len(s.tag_gt)
    on = np.ones(n, bool)
    on[3::5] = False   # not from 0: in the 20 x 10 scene that would switch off every observation of the origin tag, the gauge
    cam_const, tag_const = np.zeros(nc, bool), np.zeros(nt, bool)
    cam_const[[1, nc - 1]] = True
    tag_const[nt - 1] = True
    return (("robust", True, None, None, None), ("plain", False, None, None, None), ("masked", True, on, None, None),
            ("constants", True, None, cam_const, tag_const))


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_system_matches_the_host_jacobian(oracle, monkeypatch, name, elim):
    s = _scene(name)
    k = _truth(s) + 0.01 * PERTURB   # off the optimum: r_k is a step of many standard deviations
    n6 = 6 * (len(s.cam_gt) + len(s.tag_gt))
    monkeypatch.setenv("VMM_BA_SCHUR", "dense")
    dense = _handle(s, elim, k)
    monkeypatch.setenv("VMM_BA_SCHUR", "sparse")
    monkeypatch.setenv("VMM_BA_ORDER", "nd")
    sparse = _handle(s, elim, k)
    bad = []
    try:
        assert sparse.solve(_options(True, max_num_iterations=0))["block_sparse"] == 1
        sparse.set_state(s.cam_gt, s.tag_gt)
        for label, robust, on, cam_const, tag_const in _variants(s):
            for ba in (dense, sparse):
                ba.set_observation_mask(on)
                ba.set_constant_poses(cam_const, tag_const)
            got = dense.intrinsics_system(robustify=robust)
            cost, r, J, rmag = joint_system(oracle, k, s.cam_gt, s.tag_gt, *scene_args(s), robust=robust, obs_on=on,
                                            cam_const=cam_const, tag_const=tag_const, want_magnitude=True)
            gk, Cm, rk, Sk = reduced_system(r, J, n6)
            Jk = np.abs(J[:, n6:])
            mag_C, mag_g = Jk.T @ Jk, Jk.T @ rmag
            for arr, ref, mag, bound in (("C", Cm, mag_C, BOUND_C), ("g_k", gk, mag_g, BOUND_G)):
                live = mag > 0
                dev = (np.abs(got[arr] - ref)[live] / mag[live]).max()
                zeros_ok = not got[arr][~live].any()
                print("%s %s %s %-3s deviation %.3e  bound %.3e  ratio %.3f" % (name, elim, label, arr, dev, bound, dev / bound))
                if not (dev <= bound and zeros_ok):
                    bad.append("%s %s: deviation %.3e above %.3e, or a non-zero entry of magnitude 0" % (label, arr, dev, bound))
            dev = abs(got["cost"] - cost) / cost
            print("%s %s %s cost deviation %.3e  bound %.3e" % (name, elim, label, dev, BOUND_COST))
            if not dev <= BOUND_COST:
                bad.append("%s cost: %.3e above %.3e" % (label, dev, BOUND_COST))
            H = J.T @ J
            cov_ref = model_covariance(H, n6)
            cov = np.linalg.inv(got["S_k"])
            sigma = np.sqrt(np.diag(cov_ref))
            step, step_ref = cov @ got["r_k"], np.linalg.inv(Sk) @ rk
            d_cov = np.abs(cov - cov_ref).max() / np.abs(cov_ref).max()
            d_step = (np.abs(step - step_ref) / sigma).max()
            print("%s %s %s inv(S_k) %.3e x max|ref|; step of %.3g sigma off by %.3e sigma (bound %.3e)"
                  % (name, elim, label, d_cov, (np.abs(step_ref) / sigma).max(), d_step, 10 * HOST_SIGMA_GAP))
            if not (d_cov <= 1e-6 and d_step <= 10 * HOST_SIGMA_GAP):
                bad.append("%s: inv(S_k) off by %.3e, the step by %.3e sigma" % (label, d_cov, d_step))
            if not np.array_equal(got["S_k"], got["S_k"].T):
                bad.append("%s: S_k is not symmetric in its bits" % label)
            # idempotent, and the same bits from a block-sparse, tree-ordered handle
            if not same_bytes(got, dense.intrinsics_system(robustify=robust)):
                bad.append("%s: the second call gives other bits" % label)
            if not same_bytes(got, sparse.intrinsics_system(robustify=robust)):
                bad.append("%s: the block-sparse handle gives other bits" % label)
        cam, tag = dense.get_state()
        assert cam.tobytes() == s.cam_gt.tobytes() and tag.tobytes() == s.tag_gt.tobytes()   # the state is left alone
    finally:
        dense.close()
        sparse.close()
    assert not bad, "\n".join(bad)


# ---- 2. set_intrinsics -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ELIMS)
def test_set_intrinsics_makes_the_handle_one_created_with_the_new_model(elim):
    s = _scene("distortion_12x8")
    k1, k2 = _truth(s) + 0.05 * PERTURB, _truth(s)
    used, fresh = _handle(s, elim, k1, s.cam_init, s.tag_init), _handle(s, elim, k2, s.cam_init, s.tag_init)
    try:
        used.solve(robustify=1)   # captures the iteration graph with k1
        used.set_state(s.cam_init, s.tag_init)
        used.set_intrinsics(k2[:4], k2[4:])
        gi, gd = used.get_intrinsics()
        assert gi.tobytes() == k2[:4].tobytes() and gd.tobytes() == k2[4:].tobytes()
        assert used.cost() == fresh.cost()
        a, b = used.eval_blocks(), fresh.eval_blocks()
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
        sa, sb = used.solve(robustify=1), fresh.solve(robustify=1)   # a stale captured graph would still hold k1
        for key in ("termination_type", "iterations", "initial_cost", "final_cost", "num_lm_iterations"):
            assert sa[key] == sb[key], key
        for x, y in zip(used.get_state(), fresh.get_state()):
            assert x.tobytes() == y.tobytes()
        pa, pb = used.reprojection_stats(), fresh.reprojection_stats()
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(pa, pb))
        assert same_bytes(used.intrinsics_system(), fresh.intrinsics_system())
    finally:
        used.close()
        fresh.close()


# ---- 3. exact data ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_exact_data_recovers_the_model_and_the_poses(name, elim):
    from visual_marker_mapping_amd import _lib
    s = _scene(name, exact=True)
    ba = _handle(s, elim, _truth(s) + PERTURB)
    try:
        intr, dist, cov, rep, inner = ba.solve_selfcal(_options(False))
        cam, tag = ba.get_state()
    finally:
        ba.close()
    k = np.concatenate([intr, dist])
    err = np.abs(k - _truth(s)) / np.maximum(np.abs(_truth(s)), 1.0)
    gc, gt = max(pose_gap(cam, s.cam_gt)), max(pose_gap(tag, s.tag_gt))
    print("%s %s: status %d outer %d accepted %d inner %d; cost %.3g -> %.3g; pose gaps %.3g %.3g; parameter errors %s"
          % (name, elim, rep["status"], rep["outer_iterations"], rep["accepted"], rep["inner_lm_iterations"],
             rep["initial_cost"], rep["final_cost"], gc, gt, np.array2string(err, precision=3)))
    assert rep["status"] == _lib.CAL_OK
    assert np.isfinite(cov).all() and np.isfinite(k).all() and np.isfinite(cam).all() and np.isfinite(tag).all()
    assert (err <= 1e-9).all() and gc <= 1e-9 and gt <= 1e-9


# ---- 4. noisy data against the host optimum -----------------------------------------------------------------------------

def _check_against_host(s, got, ref, label, mask=0x1FF):
    intr, dist, cov, rep, cam, tag = got
    k_ref, cams_ref, tags_ref, cost_ref, H = ref
    n6 = 6 * (len(cams_ref) + len(tags_ref))
    cov_ref = model_covariance(H, n6, mask)
    free = [j for j in range(9) if (mask >> j) & 1]
    sigma = np.sqrt(np.diag(cov_ref))[free]
    gap = np.abs(np.concatenate([intr, dist]) - k_ref)[free] / sigma
    pg = max(*pose_gap(cam, cams_ref), *pose_gap(tag, tags_ref))
    rel = (rep["final_cost"] - cost_ref) / cost_ref
    d_cov = np.abs(cov - cov_ref).max() / np.abs(cov_ref).max()
    print("%s: status %d outer %d accepted %d inner %d; pose gap %.3g; cost device %.15g host %.15g (rel %.3g); covariance "
          "%.3g x max|ref|; parameter gaps in sigma %s" % (label, rep["status"], rep["outer_iterations"], rep["accepted"],
                                                         rep["inner_lm_iterations"], pg, rep["final_cost"], cost_ref, rel,
                                                         d_cov, np.array2string(gap, precision=3)))
    assert pg <= 1e-6, (label, pg)
    assert abs(rel) <= 1e-9, (label, rel)
    assert (gap <= 10 * HOST_SIGMA_GAP).all(), (label, gap)
    assert d_cov <= 1e-6, (label, d_cov)
    for j in range(9):
        if not (mask >> j) & 1:
            assert not cov[j].any() and not cov[:, j].any()


@pytest.mark.parametrize("robust", (False, True), ids=("plain", "robust"))
@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_noisy_data_reaches_the_host_optimum(oracle, name, elim, robust):
    from visual_marker_mapping_amd import _lib
    s = _scene(name)
    ref = _reference(oracle, name, robust)
    ba = _handle(s, elim, _truth(s) + PERTURB)
    try:
        intr, dist, cov, rep, inner = ba.solve_selfcal(_options(robust))
        cam, tag = ba.get_state()
    finally:
        ba.close()
    assert rep["status"] == _lib.CAL_OK
    _check_against_host(s, (intr, dist, cov, rep, cam, tag), ref, "%s %s %s" % (name, elim, "robust" if robust else "plain"))


# ---- 5. the mask -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ELIMS)
def test_a_masked_parameter_keeps_its_bits_and_the_rest_reach_the_restricted_optimum(oracle, elim):
    from visual_marker_mapping_amd import _lib
    s = _scene("config1_20x10")
    start = _truth(s) + PERTURB * np.array([1, 1, 1, 1, 0, 0, 0, 0, 0.0])
    ref = _reference(oracle, "config1_20x10", True, mask=0x00F, k_start=_truth(s))
    ba = _handle(s, elim, start)
    try:
        intr, dist, cov, rep, inner = ba.solve_selfcal(_options(True), refine_mask=0x00F)
        cam, tag = ba.get_state()
    finally:
        ba.close()
    assert rep["status"] == _lib.CAL_OK and dist.tobytes() == start[4:].tobytes()
    _check_against_host(s, (intr, dist, cov, rep, cam, tag), ref, "mask 0x00F %s" % elim, mask=0x00F)


@pytest.mark.parametrize("elim", ELIMS)
def test_an_empty_mask_is_a_plain_solve(elim):
    from visual_marker_mapping_amd import _lib
    s = _scene("config1_20x10")
    k0 = _truth(s) + 0.1 * PERTURB
    a, b = _handle(s, elim, k0, s.cam_init, s.tag_init), _handle(s, elim, k0, s.cam_init, s.tag_init)
    try:
        plain = a.solve(_options(True), trace_capacity=64)
        intr, dist, cov, rep, inner = b.solve_selfcal(_options(True), trace_capacity=64, refine_mask=0)
        for x, y in zip(a.get_state(), b.get_state()):
            assert x.tobytes() == y.tobytes()
    finally:
        a.close()
        b.close()
    timing = {key for key in plain if key.startswith("time_")}
    assert {key: v for key, v in plain.items() if key not in timing} == {key: v for key, v in inner.items() if key not in timing}
    assert rep["status"] == _lib.CAL_OK and rep["outer_iterations"] == 0 and rep["accepted"] == 0
    assert rep["initial_cost"] == rep["final_cost"] == plain["final_cost"]
    assert np.concatenate([intr, dist]).tobytes() == k0.tobytes() and not cov.any()


# ---- 6. consistency --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ELIMS)
def test_results_are_consistent_and_repeat_bit_for_bit(elim):
    from visual_marker_mapping_amd import _lib
    s = _scene("distortion_12x8")
    k0 = _truth(s) + PERTURB
    ba = _handle(s, elim, k0)
    try:
        runs = []
        for _ in range(2):
            ba.set_state(s.cam_gt, s.tag_gt)
            ba.set_intrinsics(k0[:4], k0[4:])
            intr, dist, cov, rep, inner = ba.solve_selfcal(_options(True))
            cam, tag = ba.get_state()
            gi, gd = ba.get_intrinsics()
            assert gi.tobytes() == intr.tobytes() and gd.tobytes() == dist.tobytes()
            assert ba.intr.tobytes() == intr.tobytes() and ba.dist.tobytes() == dist.tobytes()
            assert ba.cost(robustify=True) == pytest.approx(rep["final_cost"], rel=1e-12)
            assert rep["final_cost"] == inner["final_cost"] or rep["final_cost"] < inner["final_cost"]   # the last trial may be a rejected one
            assert rep["final_cost"] <= rep["initial_cost"] and rep["accepted"] <= rep["outer_iterations"]
            for v in list(rep.values()) + [intr, dist, cov, cam, tag]:
                assert np.isfinite(v).all()
            assert np.array_equal(cov, cov.T) and (np.diag(cov) > 0).all()
            runs.append((intr, dist, cov, cam, tag, {key: v for key, v in rep.items() if key != "time_s"}))
        for x, y in zip(runs[0][:5], runs[1][:5]):
            assert x.tobytes() == y.tobytes()
        assert runs[0][5] == runs[1][5]
        # every observation switched off: nothing to refine, OK, the model unchanged
        ba.set_intrinsics(k0[:4], k0[4:])
        ba.set_observation_mask(np.zeros(len(s.obs_cam), bool))
        sys0 = ba.intrinsics_system()
        assert sys0["cost"] == 0 and not any(sys0[key].any() for key in ("g_k", "C", "r_k", "S_k"))
        intr, dist, cov, rep, inner = ba.solve_selfcal(_options(True))
        assert rep["status"] == _lib.CAL_OK and rep["accepted"] == 0 and not cov.any()
        assert np.concatenate([intr, dist]).tobytes() == k0.tobytes()
    finally:
        ba.close()
    # no observation at all
    empty = _handle(s, elim, k0, obs=([], [], np.zeros((0, 8))))
    try:
        sys0 = empty.intrinsics_system()
        assert sys0["cost"] == 0 and not any(sys0[key].any() for key in ("g_k", "C", "r_k", "S_k"))
        intr, dist, cov, rep, inner = empty.solve_selfcal(_options(True))
        cam, tag = empty.get_state()
        assert rep["status"] == _lib.CAL_OK and np.concatenate([intr, dist]).tobytes() == k0.tobytes() and not cov.any()
        assert cam.tobytes() == s.cam_gt.tobytes() and tag.tobytes() == s.tag_gt.tobytes()
    finally:
        empty.close()


def test_state_errors_and_an_unidentifiable_model():
    """Point-landmark handles are refused like the covariance entries refuse them; a model that the data cannot
    determine (one camera, one fronto-parallel tag: focal length against distance) is SINGULAR, the state that of the
    first solve, the covariance zeros."""
    from visual_marker_mapping_amd import _lib, engine as eng
    s = _scene("config1_20x10")
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px,
                            landmarks=eng.LANDMARK_POINTS)
    try:
        for call in (lambda: ba.set_intrinsics(s.intr, s.dist), ba.intrinsics_system, ba.solve_selfcal):
            with pytest.raises(_lib.VmmBaError) as ei:
                call()
            assert ei.value.status == _lib.ERR_STATE
        gi, gd = ba.get_intrinsics()
        assert gi.tobytes() == s.intr.tobytes() and gd.tobytes() == s.dist.tobytes()
    finally:
        ba.close()
    first = np.flatnonzero(s.obs_tag == s.fixed_tag)[:1]
    cam = s.cam_gt[s.obs_cam[first]]
    one = eng.BundleAdjuster(s.intr, s.dist, cam, s.tag_gt[:1], s.tag_wh[:1], 0, [0], [0], s.obs_px[first])
    try:
        plain = one.solve(_options(False))
        state = one.get_state()
        one.set_state(cam, s.tag_gt[:1])
        intr, dist, cov, rep, inner = one.solve_selfcal(_options(False))
        assert rep["status"] == _lib.CAL_SINGULAR and not cov.any() and rep["accepted"] == 0
        assert np.concatenate([intr, dist]).tobytes() == _truth(s).tobytes()
        assert rep["final_cost"] == plain["final_cost"]
        for x, y in zip(one.get_state(), state):
            assert x.tobytes() == y.tobytes()
    finally:
        one.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------

def test_reconstructor_member_and_command_line_recover_the_truth(tmp_path):
    """Exact data through the files.  The model and the poses travel with 17 significant digits, so nothing is lost on the
    way, and the member tightens the inner solves itself: the bound is the 1e-9 of the exact tests above, on parameters
    (relative to max(|k_j|, 1)) and poses."""
    from visual_marker_mapping_amd import _lib, io as vio, selfcalibration
    from visual_marker_mapping_amd.synthetic import write_project
    from visual_marker_mapping_amd.tag_reconstructor import CameraModel, TagReconstructor
    s = _scene("config1_20x10", exact=True)
    proj = str(tmp_path / "proj")
    model, det = write_project(s, proj)
    shutil.copy(os.path.join(proj, "ground_truth.json"), os.path.join(proj, "reconstruction.json"))
    k0 = _truth(s) + PERTURB
    start_file = str(tmp_path / "start.json")
    start_model = CameraModel(*k0[:4], distortionCoefficients=k0[4:], verticalResolution=model.verticalResolution,
                              horizontalResolution=model.horizontalResolution)
    vio.writeCameraModel(start_model, start_file)

    def errors(m, tags, cams):
        k = np.concatenate([[m.fx, m.fy, m.cx, m.cy], m.distortionCoefficients])
        err = np.abs(k - _truth(s)) / np.maximum(np.abs(_truth(s)), 1.0)
        gt = max(pose_gap(np.array([np.r_[tags[t].q, tags[t].t] for t in range(len(s.tag_gt))]), s.tag_gt))
        gc = max(pose_gap(np.array([np.r_[cams[c].q, cams[c].t] for c in range(len(s.cam_gt))]), s.cam_gt))
        return k, err, max(gt, gc)

    assert selfcalibration.main(["--project_path", proj, "--intrinsics", start_file]) == 0
    tags, cams, m = vio.parseReconstructions(os.path.join(proj, "reconstruction_selfcalibrated.json"))
    k, err, pg = errors(m, tags, cams)
    print("command line: pose gap %.3g, parameter errors %s" % (pg, np.array2string(err, precision=3)))
    assert (err <= 1e-9).all() and pg <= 1e-9
    m2 = vio.readCameraModel(os.path.join(proj, "camera_intrinsics_calibrated.json"))
    assert np.concatenate([[m2.fx, m2.fy, m2.cx, m2.cy], m2.distortionCoefficients]).tobytes() == k.tobytes()
    assert (m2.verticalResolution, m2.horizontalResolution) == (model.verticalResolution, model.horizontalResolution)
    side = vio.read_json(os.path.join(proj, "selfcalibration.json"))
    assert side["status"] == "ok" and int(side["accepted"]) >= 1 and int(side["outer_iterations"]) >= int(side["accepted"])
    assert [float(v) for v in side["parameters"]] == k.tolist()
    cov = np.array([float(v) for v in side["covariance"]["coefficents"]]).reshape(9, 9)
    assert np.allclose(np.sqrt(np.diag(cov)), [float(v) for v in side["standard_deviations"]], rtol=1e-12)
    assert float(side["final_cost"]) <= float(side["initial_cost"])
    # the member, and its default: without refineCameraModel the model is taken as given
    rec = TagReconstructor(det)
    rec.setCameraModel(start_model)
    gt_tags, gt_cams, _ = vio.parseReconstructions(os.path.join(proj, "ground_truth.json"))
    rec.setReconstructedTags(gt_tags)
    rec.setReconstructedCameras(gt_cams)
    rec.setOriginTagId(0)
    rec.doBundleAdjustment(50, 1, False)
    assert rec.getCameraModel() is start_model and rec.lastSelfCalibrationReport is None
    rec.doBundleAdjustment(1500, 1, False, refineCameraModel=True)
    report = rec.lastSelfCalibrationReport
    k, err, pg = errors(rec.getCameraModel(), rec.getReconstructedTags(), rec.getReconstructedCameras())
    print("member: status %d, pose gap %.3g, parameter errors %s" % (report["status"], pg, np.array2string(err, precision=3)))
    assert report["status"] == _lib.CAL_OK and report["intrinsics"].tobytes() == k.tobytes()
    assert (err <= 1e-9).all() and pg <= 1e-9
    assert np.allclose(report["std"], np.sqrt(np.diag(report["covariance"])))
    rec.close()
