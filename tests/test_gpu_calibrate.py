"""GPU tests of the calibration against a finished map (vmm_ba_calibrate, engine.calibrate,
TagReconstructor.refineCameraModel and the command line).

Yardstick: tests/yardstick.py -- calib_system / host_calibration / calibration_covariance, numpy around
oracle/oracle.py, proven against central differences in tests/test_yardstick_cpu.py; they never call the code under
test.  Tolerances: 1e-9 on exact data, 1e-6 per pose between two optima, covariances to
1e-6 x max|ref| as the existing covariance tests, costs to 1e-9 relative (second order in the gap), parameters in units of their standard deviation
(yardstick.SIGMA_GAP).  Scenes come from synthetic.make_scene, the map is tag_gt.
tests/test_gpu_arrowhead_accuracy.py supersedes in strength the 1e-6 x max|ref| comparisons of intr_cov and cam_cov (under
a max-norm the rows of k1 .. k3 of intr_cov could be wrong by their whole size), the 1e-9 comparison of final_cost with the
host optimum and the finiteness checks of an image's cost, rms_px and of final_rms_px: there every entry over
sqrt(truth_ii truth_jj), every scalar and one single trial are held to float64 accuracy at the device's own state, on
images of 1 .. 513 tags and batches of 1 .. 257 images.  The tests here stay, their assertions unchanged.
"""
import os
import shutil

import numpy as np
import pytest

from yardstick import PERTURB, SIGMA_GAP, calib_system, calibration_covariance, host_calibration, pose_gap

pytestmark = pytest.mark.gpu

WIDE = dict(inlier_px=1e4, loc_inlier_px=1e4)   # the data hold no outliers: every observation is an inlier
EXACT = {
    "config1_20x10": (1, dict()),
    "distortion_12x8": (5, dict(n_cams=12, n_tags=8, visibility=0.6)),
    "closeup_12x30": (2, dict(n_cams=12, n_tags=30, neighbors_min=6, neighbors_max=10)),
}
OUTLIER_SCENE = (5, dict(n_cams=30, n_tags=40, visibility=0.5))


# ---- helpers --------------------------------------------------------------------------------------------------------

def _csr(s):
    """The scene's observations grouped by image: (img_start, obs_img, obs_tag, obs_px)."""
    start, order = s.by_image()
    return start, s.obs_cam[order].astype(np.int64), s.obs_tag[order].astype(np.int32), s.obs_px[order].copy()


def _truth(s):
    return np.concatenate([s.intr, s.dist])


def _calibrate(s, k0, start, tag, px, **kw):
    from visual_marker_mapping_amd import engine as eng
    out = eng.calibrate(k0[:4], k0[4:], s.tag_gt, s.tag_wh, start, tag, px, **kw)
    return dict(zip(("intr", "dist", "intr_cov", "cam", "cam_cov", "inl", "res", "report"), out),
                k=np.concatenate([out[0], out[1]]))


def _assert_clean(d):
    for key in ("intr", "dist", "intr_cov", "cam", "cam_cov"):
        assert np.isfinite(d[key]).all(), key
    for r in d["res"]:
        assert np.isfinite(r["rms_px"]) and np.isfinite(r["cost"]), r
    for key, v in d["report"].items():
        assert np.isfinite(v), key


def _check_against_host(O, s, d, ref, used, label, mask=0x1FF):
    """The device's result `d` against the host optimum ref = (k, cams, cost, H) over the images `used`: poses to 1e-6,
    cost to 1e-9 relative on either side, every free parameter to SIGMA_GAP standard deviations."""
    k_ref, cams_ref, cost_ref, H = ref
    icov, _ = calibration_covariance(H, len(cams_ref), mask)
    sigma = np.sqrt(np.diag(icov))
    gq, gt = pose_gap(d["cam"][used], cams_ref)
    rel = (d["report"]["final_cost"] - cost_ref) / cost_ref
    free = [j for j in range(9) if (mask >> j) & 1]
    gap = np.abs(d["k"] - k_ref)[free] / sigma[free]
    print("%s: trials %d accepted %d passes %d; |dq| %.3g |dt| %.3g; cost device %.15g host %.15g (rel %.3g); "
          "parameter gaps in sigma %s" % (label, d["report"]["trials"], d["report"]["accepted"], d["report"]["passes"], gq, gt,
                                          d["report"]["final_cost"], cost_ref, rel, np.array2string(gap, precision=3)))
    assert gq <= 1e-6 and gt <= 1e-6, (label, gq, gt)
    assert abs(rel) <= 1e-9, (label, rel)
    assert (gap <= SIGMA_GAP).all(), (label, gap)


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_data_recovers_the_camera_model_and_the_poses(name):
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = EXACT[name]
    s = make_scene(cfg, noise_px=0.0, outlier_frac=0.0, **kw)
    start, _, tag, px = _csr(s)
    d = _calibrate(s, _truth(s) + PERTURB, start, tag, px, **WIDE)
    rep = d["report"]
    gq, gt = pose_gap(d["cam"], s.cam_gt)
    err = np.abs(d["k"] - _truth(s)) / np.maximum(np.abs(_truth(s)), 1.0)
    print("%s: %d images %d observations; status %d trials %d accepted %d passes %d; rms %.3g -> %.3g px; |dq| %.3g |dt| %.3g; "
          "parameter errors %s" % (name, len(d["cam"]), len(tag), rep["status"], rep["trials"], rep["accepted"], rep["passes"],
                                   rep["initial_rms_px"], rep["final_rms_px"], gq, gt, np.array2string(err, precision=3)))
    _assert_clean(d)
    assert rep["status"] == _lib.CAL_OK
    assert rep["n_images_used"] == len(d["cam"]) and rep["n_obs_used"] == len(tag) and d["inl"].all()
    assert gq <= 1e-9 and gt <= 1e-9, (gq, gt)
    assert (err <= 1e-9).all(), err


# ---- 2.-4. noisy data against an independent optimum ---------------------------------------------------------------

@pytest.fixture(scope="module")
def noisy():
    """make_scene(1) at its own noise: the device's non-robust result from the perturbed start and the host optimum from
    the truth, shared by the tests below and left unchanged."""
    from oracle import oracle as O
    from visual_marker_mapping_amd.synthetic import make_scene
    O.build()
    s = make_scene(1)
    assert s.noise_px == 0.3
    start, img, tag, px = _csr(s)
    d = _calibrate(s, _truth(s) + PERTURB, start, tag, px, robustify=0, reclassify_passes=0, **WIDE)
    ref = host_calibration(O, _truth(s), s.cam_gt, s.tag_gt, s.tag_wh, img, tag, px, robust=False)
    return s, (start, img, tag, px), d, ref


def test_noisy_data_reaches_the_host_optimum(oracle, noisy):
    """Measured between the two host optimisers (host_calibration and scipy least_squares, see SIGMA_GAP): 1.01e-6 sigma
    at the worst parameter; the bound on the device is ten times that, 1.01e-5 sigma."""
    from visual_marker_mapping_amd import _lib
    s, (start, img, tag, px), d, ref = noisy
    _assert_clean(d)
    assert d["report"]["status"] == _lib.CAL_OK and d["report"]["passes"] == 1
    assert d["report"]["n_images_used"] == len(s.cam_gt) and d["inl"].all()
    _check_against_host(oracle, s, d, ref, np.arange(len(s.cam_gt)), "noisy non-robust")


def test_robust_loss_reaches_the_host_optimum(oracle, noisy):
    from visual_marker_mapping_amd import _lib
    s, (start, img, tag, px), _, _ = noisy
    d = _calibrate(s, _truth(s) + PERTURB, start, tag, px, robustify=1, reclassify_passes=0, **WIDE)
    _assert_clean(d)
    assert d["report"]["status"] == _lib.CAL_OK
    keep = d["inl"]
    assert keep.all()
    ref = host_calibration(oracle, _truth(s), s.cam_gt, s.tag_gt, s.tag_wh, img[keep], tag[keep], px[keep], robust=True)
    _check_against_host(oracle, s, d, ref, np.arange(len(s.cam_gt)), "noisy robust")


def test_covariances_match_the_inverse_of_the_full_normal_matrix(oracle, noisy):
    s, (start, img, tag, px), d, _ = noisy
    _, _, J = calib_system(oracle, d["k"], d["cam"], s.tag_gt, s.tag_wh, img, tag, px, robust=False)
    icov, ccov = calibration_covariance(J.T @ J, len(s.cam_gt))
    err = np.abs(d["intr_cov"] - icov).max() / np.abs(icov).max()
    print("intr_cov: error %.3g of max|ref|; sigma %s" % (err, np.array2string(np.sqrt(np.diag(icov)), precision=3)))
    assert err <= 1e-6
    assert (d["intr_cov"] == d["intr_cov"].T).all() and np.linalg.eigvalsh(d["intr_cov"]).min() > 0
    worst = 0.0
    for i in range(len(s.cam_gt)):
        e = np.abs(d["cam_cov"][i] - ccov[i]).max() / np.abs(ccov[i]).max()
        worst = max(worst, e)
        assert e <= 1e-6, (i, e)
        assert (d["cam_cov"][i] == d["cam_cov"][i].T).all() and np.linalg.eigvalsh(d["cam_cov"][i]).min() > 0
    print("cam_cov: worst error %.3g of max|ref|" % worst)


# ---- 5. mask --------------------------------------------------------------------------------------------------------

def test_masked_parameters_keep_their_bits_and_the_rest_reach_the_restricted_optimum(oracle, noisy):
    from visual_marker_mapping_amd import _lib
    s, (start, img, tag, px), _, _ = noisy
    assert (s.dist == 0).all()
    k0 = _truth(s) + PERTURB   # wrong distortion, held fixed
    d = _calibrate(s, k0, start, tag, px, refine_mask=0xF, robustify=0, reclassify_passes=0, **WIDE)
    _assert_clean(d)
    assert d["report"]["status"] == _lib.CAL_OK
    assert d["dist"].tobytes() == k0[4:].tobytes()
    assert (d["intr_cov"][4:, :] == 0).all() and (d["intr_cov"][:, 4:] == 0).all()
    assert np.linalg.eigvalsh(d["intr_cov"][:4, :4]).min() > 0
    ref = host_calibration(oracle, k0, s.cam_gt, s.tag_gt, s.tag_wh, img, tag, px, robust=False, mask=0xF)
    assert ref[0][4:].tobytes() == k0[4:].tobytes()
    _check_against_host(oracle, s, d, ref, np.arange(len(s.cam_gt)), "mask 0xF", mask=0xF)


# ---- 6. outliers and reclassification, 8. repeatability ------------------------------------------------------------

@pytest.fixture(scope="module")
def outliers():
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = OUTLIER_SCENE
    s = make_scene(cfg, **kw)
    start, img, tag, px = _csr(s)
    d = _calibrate(s, _truth(s) + 0.25 * PERTURB, start, tag, px)   # the default options
    return s, (start, img, tag, px), d


def test_outliers_are_reclassified_and_the_result_is_the_optimum_over_the_final_inliers(oracle, outliers):
    from visual_marker_mapping_amd import _lib, engine as eng
    s, (start, img, tag, px), d = outliers
    rep = d["report"]
    _assert_clean(d)
    print("outliers: status %d trials %d accepted %d passes %d; %d of %d images, %d of %d observations; rms %.4g -> %.4g px"
          % (rep["status"], rep["trials"], rep["accepted"], rep["passes"], rep["n_images_used"], len(s.cam_gt),
             rep["n_obs_used"], len(tag), rep["initial_rms_px"], rep["final_rms_px"]))
    assert rep["status"] == _lib.CAL_OK and rep["passes"] == 3
    assert rep["final_rms_px"] < rep["initial_rms_px"]
    used = np.array([i for i in range(len(s.cam_gt)) if np.any(d["cam_cov"][i])])
    assert len(used) == rep["n_images_used"] and int(d["inl"].sum()) >= rep["n_obs_used"]
    # the host optimum over the final inlier set of the images that took part
    index = {int(i): n for n, i in enumerate(used)}
    keep = d["inl"] & np.isin(img, used)
    assert int(keep.sum()) == rep["n_obs_used"]
    ref = host_calibration(oracle, _truth(s), s.cam_gt[used], s.tag_gt, s.tag_wh,
                           np.array([index[int(i)] for i in img[keep]]), tag[keep], px[keep], robust=True)
    _check_against_host(oracle, s, d, ref, used, "outliers")
    # corner-displaced observations: some corner further from its true projection than noise can put it (0.5 px noise
    # per axis: 4 px is 8 sigma)
    r = np.array([oracle.obs_eval(s.intr, s.dist, s.cam_gt[img[o]], s.tag_gt[tag[o]], s.tag_wh[tag[o]], px[o], jac=False)
                  for o in range(len(tag))])
    displaced = (np.linalg.norm(r.reshape(-1, 4, 2), axis=2) > 4.0).any(axis=1)
    _, _, loc_inl, _ = eng.localize(s.intr, s.dist, s.tag_gt, s.tag_wh, start, tag, px)
    out_cal, out_loc = int((~d["inl"] & displaced).sum()), int((~loc_inl & displaced).sum())
    print("outliers: %d displaced observations; flagged out by the calibration %d, by the localisation under the true "
          "model %d; clean observations flagged out %d" % (int(displaced.sum()), out_cal, out_loc,
                                                          int((~d["inl"] & ~displaced).sum())))
    assert displaced.sum() > 10 and out_cal >= out_loc


def test_two_calls_give_identical_bytes(outliers):
    s, (start, img, tag, px), d = outliers
    again = _calibrate(s, _truth(s) + 0.25 * PERTURB, start, tag, px)
    for key in ("intr", "dist", "intr_cov", "cam", "cam_cov", "inl"):
        assert d[key].tobytes() == again[key].tobytes(), key
    assert d["res"] == again["res"]
    assert {k: v for k, v in d["report"].items() if k != "time_s"} == {k: v for k, v in again["report"].items() if k != "time_s"}


def test_reclassification_without_a_trial_reproduces_the_localisations_flags():
    """max_trials=0: the camera model never moves and the poses stay the localisation's, so the one reclassification
    pass (k_calib_classify) must return byte for byte the flags k_localize ended with for the same model and options --
    both run classify_image.  24 images: one of 257 observations (the second trip of the 256-thread stride, read from
    global memory by both kernels), the others of 3 to 10; a tenth of all pixel coordinates displaced by up to 60 px,
    far beyond inlier_px = 8."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, seed=4247, n_cams=24, n_tags=260, visibility=1.0)
    rng = np.random.default_rng(4248)
    sizes = rng.integers(3, 11, len(s.cam_gt))
    sizes[0] = 257
    idx = np.concatenate([np.flatnonzero(s.obs_cam == c)[:m] for c, m in enumerate(sizes)])
    assert len(idx) == sizes.sum()
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tag, px = s.obs_tag[idx].astype(np.int32), s.obs_px[idx].copy()
    hit = rng.random(px.shape) < 0.1
    px[hit] += rng.uniform(-60.0, 60.0, int(hit.sum()))
    _, _, inl, _ = eng.localize(s.intr, s.dist, s.tag_gt, s.tag_wh, start, tag, px)
    d = _calibrate(s, _truth(s), start, tag, px, max_trials=0, reclassify_passes=1)
    print("flags: %d of %d observations inliers of the localisation, %d of the calibration; passes %d trials %d"
          % (int(inl.sum()), len(inl), int(d["inl"].sum()), d["report"]["passes"], d["report"]["trials"]))
    assert d["report"]["passes"] == 2 and d["report"]["trials"] == 0
    assert 0 < inl.sum() < len(inl) and not inl[start[0]:start[1]].all()   # both kinds, also in the long image
    assert d["inl"].tobytes() == inl.tobytes()


# ---- 7. edges -------------------------------------------------------------------------------------------------------

def test_edges_single_tag_empty_images_and_an_unusable_image():
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, noise_px=0.0, outlier_frac=0.0)
    start, img, tag, px = _csr(s)
    k0 = _truth(s) + 0.25 * PERTURB
    # one image with one tag: 8 residuals for 15 unknowns
    d = _calibrate(s, k0, np.array([0, 1], np.int64), tag[:1], px[:1], min_inlier_tags=1, **WIDE)
    print("single tag: status %d trials %d" % (d["report"]["status"], d["report"]["trials"]))
    _assert_clean(d)
    assert d["report"]["status"] in (_lib.CAL_SINGULAR, _lib.CAL_NO_CONVERGENCE)
    assert (d["intr_cov"] == 0).all() and (d["cam_cov"] == 0).all()
    # every image empty
    d = _calibrate(s, k0, np.zeros(4, np.int64), tag[:0], px[:0])
    _assert_clean(d)
    assert d["report"]["status"] == _lib.CAL_NO_IMAGES and d["k"].tobytes() == k0.tobytes()
    assert [r["status"] for r in d["res"]] == [_lib.LOC_NO_OBSERVATIONS] * 3
    # one unusable image (its only observation collapsed to a point: no candidate) among good ones
    b1, e1 = int(start[1]), int(start[2])
    bad_px = np.tile(px[0, :2], 4)[None, :]
    m_start = np.concatenate([[0, e1 - b1, e1 - b1 + 1], e1 - b1 + 1 + (start[3:] - start[2])]).astype(np.int64)
    m_tag = np.concatenate([tag[b1:e1], tag[:1], tag[start[2]:]])
    m_px = np.concatenate([px[b1:e1], bad_px, px[start[2]:]])
    d = _calibrate(s, _truth(s) + PERTURB, m_start, m_tag, m_px, **WIDE)
    _assert_clean(d)
    n = len(m_start) - 1
    assert d["res"][1]["status"] == _lib.LOC_NO_CANDIDATE
    assert (d["cam"][1] == [1, 0, 0, 0, 0, 0, 0]).all() and (d["cam_cov"][1] == 0).all() and not d["inl"][e1 - b1]
    assert d["report"]["status"] == _lib.CAL_OK and d["report"]["n_images_used"] == n - 1
    good = [0] + list(range(2, n))
    gq, gt = pose_gap(d["cam"][good], s.cam_gt[[1] + list(range(2, len(s.cam_gt)))])
    err = np.abs(d["k"] - _truth(s)) / np.maximum(np.abs(_truth(s)), 1.0)
    print("unusable image among %d: |dq| %.3g |dt| %.3g parameter errors %s" % (n, gq, gt, np.array2string(err, precision=3)))
    assert gq <= 1e-9 and gt <= 1e-9 and (err <= 1e-9).all()
    assert all(np.linalg.eigvalsh(d["cam_cov"][i]).min() > 0 for i in good)


# ---- 9. command line -----------------------------------------------------------------------------------------------

def test_command_line_and_reconstructor_member_recover_the_truth(tmp_path):
    from visual_marker_mapping_amd import _lib, calibration, io as vio
    from visual_marker_mapping_amd.synthetic import make_scene, write_project
    from visual_marker_mapping_amd.tag_reconstructor import CameraModel, TagReconstructor
    s = make_scene(1, noise_px=0.0, outlier_frac=0.0)
    proj = str(tmp_path / "proj")
    model, det = write_project(s, proj)
    map_file = str(tmp_path / "map.json")
    shutil.copy(os.path.join(proj, "ground_truth.json"), map_file)
    k0 = _truth(s) + PERTURB
    start_file = str(tmp_path / "start.json")
    start_model = CameraModel(*k0[:4], distortionCoefficients=k0[4:], verticalResolution=model.verticalResolution,
                              horizontalResolution=model.horizontalResolution)
    vio.writeCameraModel(start_model, start_file)
    out_file = str(tmp_path / "out" / "calibrated.json")
    os.makedirs(os.path.dirname(out_file))
    assert calibration.main(["--project_path", proj, "--map", map_file, "--intrinsics", start_file, "--output", out_file,
                             "--option", "inlier_px=1e4", "--option", "loc_inlier_px=1e4"]) == 0
    got = vio.readCameraModel(out_file)
    k = np.concatenate([[got.fx, got.fy, got.cx, got.cy], got.distortionCoefficients])
    err = np.abs(k - _truth(s)) / np.maximum(np.abs(_truth(s)), 1.0)
    print("command line: parameter errors %s" % np.array2string(err, precision=3))
    assert (err <= 1e-9).all()
    assert (got.verticalResolution, got.horizontalResolution) == (model.verticalResolution, model.horizontalResolution)
    side = vio.read_json(os.path.join(os.path.dirname(out_file), "calibration.json"))
    assert side["status"] == "ok" and int(side["n_images_used"]) == len(s.cam_gt)
    assert np.array([float(v) for v in side["parameters"]]).tobytes() == k.tobytes()
    cov = np.array([float(v) for v in side["covariance"]["coefficents"]]).reshape(9, 9)
    assert (int(side["covariance"]["rows"]), int(side["covariance"]["cols"])) == (9, 9)
    assert np.array([float(v) for v in side["standard_deviations"]]).tobytes() == np.sqrt(np.diag(cov)).tobytes()
    # the member of the reconstructor gives the same numbers
    tags, _, _ = vio.parseReconstructions(map_file)
    rec = TagReconstructor(det)
    rec.setCameraModel(vio.readCameraModel(start_file))
    rec.setReconstructedTags(tags)
    report = rec.refineCameraModel(**WIDE)
    assert report["status"] == _lib.CAL_OK
    assert report["intrinsics"].tobytes() == k.tobytes() and report["covariance"].tobytes() == cov.tobytes()
    m = rec.getCameraModel()
    assert np.concatenate([[m.fx, m.fy, m.cx, m.cy], m.distortionCoefficients]).tobytes() == k.tobytes()
    gq, gt = pose_gap(np.array([np.concatenate([report["cameras"][i].q, report["cameras"][i].t]) for i in range(len(s.cam_gt))]),
                       s.cam_gt)
    assert sorted(report["cameras"]) == list(range(len(s.cam_gt))) and gq <= 1e-9 and gt <= 1e-9
    # the same "does not exist" errors as the localisation step
    with pytest.raises(FileNotFoundError) as ei:
        calibration.main(["--project_path", proj, "--map", map_file, "--intrinsics", str(tmp_path / "none.json")])
    assert "does not exist" in str(ei.value)
