"""GPU tests of the localisation and the calibration of a multi-camera rig against a finished map (vmm_ba_rig_localize,
vmm_ba_rig_calibrate, engine.rig_localize / rig_calibrate / rig_extrinsics_start, the members of TagReconstructor and
the command line).

Yardstick throughout: tests/rig_cases.py -- numpy around oracle/oracle.py at the composed pose, proven against central
differences in tests/test_rig_cpu.py; it never calls the code under test.  Tolerances are the project's own: 1e-9 on
exact data, 1e-6 per pose between two optima, covariances to 1e-6 x max|ref|, costs to 1e-9
relative.  Scenes come from
synthetic.make_rig_scene: 12 - 20 frames, 1 - 3 cameras (8 once), 8 - 30 tags, the map is tag_gt.
tests/test_finished_map_accuracy.py supersedes in strength the 1e-6 comparisons of rig_cov for vmm_ba_rig_localize (among
them the frames of 255, 256, 257 and 600 observations): there every entry, the cost and rms_px of a frame are held to
float64 accuracy at the device's own state; the comparisons of vmm_ba_rig_calibrate are not touched by it.
tests/test_gpu_arrowhead_accuracy.py supersedes in strength, for vmm_ba_rig_calibrate, the 1e-6 x max|ref| comparisons of
ext_cov and the joint rig_cov, the 1e-9 comparison of final_cost with the host optimum and the finiteness checks of a
frame's cost, rms_px and of final_rms_px: there every entry over sqrt(truth_ii truth_jj), every scalar and one single
trial are held to float64 accuracy at the device's own state, at K = 2, 3, 4, 8 and at 1, 4, 5 and 65 frames.  The
tests here stay, their assertions unchanged.
"""
import json

import numpy as np
import pytest

import rig_cases as rc
import yardstick as ys

pytestmark = pytest.mark.gpu

# three different camera models (the first is make_scene's with the distortion of config 5)
INTR3 = np.array([[8075.0, 8083.0, 3016.0, 1996.0], [7900.0, 7950.0, 2950.0, 2050.0], [8150.0, 8100.0, 3060.0, 1960.0]])
DIST3 = np.array([[-0.186, 0.370, -2.9e-4, 4.2e-4, 0.057], [-0.10, 0.15, 3e-4, -2e-4, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])


def _run(s, **kw):
    from visual_marker_mapping_amd import engine as eng
    return eng.rig_localize(s.intr, s.dist, s.ext_qt, s.tag_gt, s.tag_wh, s.img_start, s.obs_tag, s.obs_px, **kw)


def _assert_clean(rig, cov, res):
    assert np.isfinite(rig).all() and np.isfinite(cov).all()
    for r in res:
        assert np.isfinite(r["rms_px"]) and np.isfinite(r["cost"]), r


def _frame_counts(s):
    return [int(s.img_start[(f + 1) * s.n_rig_cams] - s.img_start[f * s.n_rig_cams]) for f in range(s.n_frames)]


def _check_against_host(O, s, rig, keep, res, which, robust, label):
    """Device pose vs the host optimum over the observations of `keep`, started at the truth: 1e-6 per pose."""
    worst = (0.0, 0.0)
    for f in which:
        ref, cost = rc.host_frame_optimum(O, s, f, s.rig_gt[f], s.ext_qt, keep, robust)
        gq, gt = ys.pose_gap(rig[f], ref)
        print("%s frame %d: obs %d inliers %d trials %d |dq| %.3g |dt| %.3g cost device %.12g host %.12g"
              % (label, f, res[f]["n_obs"], res[f]["n_inlier_obs"], res[f]["trials"], gq, gt, res[f]["cost"], cost))
        worst = (max(worst[0], gq), max(worst[1], gt))
        assert gq <= 1e-6 and gt <= 1e-6, (label, f, gq, gt)
    return worst


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(rc.SCENES))
def test_exact_data_recovers_the_rig_poses(name):
    from visual_marker_mapping_amd import _lib
    s = rc.rig_scene(name, noise_px=0.0)
    rig, cov, inl, res = _run(s)
    gq, gt = ys.pose_gap(rig, s.rig_gt)
    print("%s: %d frames %d observations, max |dq| %.3g |dt| %.3g, max rms %.3g px, trials %d..%d"
          % (name, s.n_frames, len(s.obs_tag), gq, gt, max(r["rms_px"] for r in res), min(r["trials"] for r in res),
             max(r["trials"] for r in res)))
    assert [r["status"] for r in res] == [_lib.LOC_OK] * s.n_frames
    assert inl.all()
    assert [r["n_inlier_obs"] for r in res] == [r["n_obs"] for r in res] == _frame_counts(s)
    _assert_clean(rig, cov, res)
    assert gq <= 1e-9 and gt <= 1e-9, (gq, gt)


# ---- 2. one camera, identity extrinsic: vmm_ba_localize ------------------------------------------------------------

@pytest.mark.parametrize("noise", [0.0, None])
def test_one_camera_with_the_identity_extrinsic_is_the_localisation(noise):
    from visual_marker_mapping_amd import engine as eng
    kw = {} if noise is None else dict(noise_px=noise)
    s = rc.rig_scene("distortion_12x8", ext=rc.EXT3[:1], seed=5, **kw)
    rig, cov, inl, res = _run(s)
    cam, ccov, cinl, cres = eng.localize(s.intr[0], s.dist[0], s.tag_gt, s.tag_wh, s.img_start, s.obs_tag, s.obs_px)
    gq, gt = ys.pose_gap(rig, cam)
    print("K = 1, noise %s: |dq| %.3g |dt| %.3g against engine.localize" % (s.noise_px, gq, gt))
    assert [r["status"] for r in res] == [r["status"] for r in cres] and (inl == cinl).all()
    assert [r["n_inlier_obs"] for r in res] == [r["n_inlier_obs"] for r in cres]
    tol = 1e-9 if noise == 0.0 else 1e-6
    assert gq <= tol and gt <= tol, (gq, gt)
    assert np.abs(cov - ccov).max() <= 1e-6 * np.abs(ccov).max()


# ---- 3. noisy data against the host optimum, and the covariance -----------------------------------------------------

@pytest.mark.parametrize("robustify", [0, 1])
@pytest.mark.parametrize("name,models", [("config1_20x10", False), ("distortion_12x8", True)])
def test_noisy_data_reaches_the_host_optimum_and_its_covariance(oracle, name, models, robustify):
    from visual_marker_mapping_amd import _lib
    kw = dict(intr=INTR3, dist=DIST3) if models else {}
    s = rc.rig_scene(name, seed=2, **kw)   # the generator's default noise
    assert s.noise_px > 0
    rig, cov, inl, res = _run(s, robustify=robustify)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * s.n_frames
    _assert_clean(rig, cov, res)
    label = "%s robustify=%d" % (name, robustify)
    worst = _check_against_host(oracle, s, rig, inl, res, range(s.n_frames), bool(robustify), label)
    worst_cov = 0.0
    for f in range(s.n_frames):
        cost, A, _ = rc.frame_normal(oracle, s, f, rig[f], s.ext_qt, inl, bool(robustify))
        ref = np.linalg.inv(A)
        err = np.abs(cov[f] - ref).max() / np.abs(ref).max()
        worst_cov = max(worst_cov, err)
        assert err <= 1e-6, (f, err)
        assert (cov[f] == cov[f].T).all() and np.linalg.eigvalsh(cov[f]).min() > 0
        assert abs(res[f]["cost"] - cost) <= 1e-9 * cost, (f, res[f]["cost"], cost)
    print("%s: worst |dq| %.3g |dt| %.3g, worst covariance error %.3g of max|ref|" % (label, worst[0], worst[1], worst_cov))


# ---- 4. what one camera cannot do ----------------------------------------------------------------------------------

def test_a_frame_without_an_image_of_camera_0_is_localised(oracle):
    from visual_marker_mapping_amd import _lib
    missing = [(f, 0) for f in (0, 3, 4, 11)] + [(3, 1)]
    s = rc.rig_scene("closeup_12x30", seed=4, missing=missing)
    per_image = np.diff(s.img_start).reshape(s.n_frames, 3)
    assert (per_image[[0, 3, 4, 11], 0] == 0).all() and per_image[3, 1] == 0
    rig, cov, inl, res = _run(s)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * s.n_frames
    _assert_clean(rig, cov, res)
    _check_against_host(oracle, s, rig, inl, res, (0, 3, 4, 11, 5), True, "camera 0 missing")


def test_a_weak_camera_0_and_a_strong_camera_2_give_the_joint_optimum(oracle):
    from visual_marker_mapping_amd import _lib, engine as eng
    full = rc.rig_scene("config1_20x10", seed=6, noise_px=1.0)
    f = 2
    keep = np.zeros(len(full.obs_tag), bool)
    at = lambda c: np.flatnonzero((full.obs_frame == f) & (full.obs_cam == c))
    keep[at(0)[:1]] = True    # camera 0 sees one tag
    keep[at(2)[:5]] = True    # camera 2 sees five; camera 1 sees nothing
    s = rc.frames(rc.select(full, keep), [f])
    assert list(np.diff(s.img_start)) == [1, 0, 5]
    rig, cov, inl, res = _run(s)
    assert res[0]["status"] == _lib.LOC_OK and inl.all()
    joint, _ = rc.host_frame_optimum(oracle, s, 0, s.rig_gt[0], s.ext_qt, inl, True)
    gq, gt = ys.pose_gap(rig[0], joint)
    # camera 0 on its own: engine.localize on its single tag (the extrinsic of camera 0 is the identity)
    alone, _, _, ares = eng.localize(s.intr[0], s.dist[0], s.tag_gt, s.tag_wh, s.img_start[:2], s.obs_tag[:1], s.obs_px[:1])
    aq, at_ = ys.pose_gap(alone[0], joint)
    print("joint optimum: |dq| %.3g |dt| %.3g; camera 0 alone is |dq| %.3g |dt| %.3g away from it" % (gq, gt, aq, at_))
    assert gq <= 1e-6 and gt <= 1e-6, (gq, gt)
    assert ares[0]["status"] == _lib.LOC_OK and max(aq, at_) > 1e-4


# ---- 5. planted outliers -------------------------------------------------------------------------------------------

def test_planted_outliers_are_found_and_do_not_move_the_pose(oracle):
    from visual_marker_mapping_amd import _lib
    s = rc.rig_scene("closeup_12x30", seed=7, outlier_frac=0.1, outlier_px=(50.0, 200.0))
    n = len(s.obs_tag)
    assert int(s.outlier.sum()) == int(round(0.1 * n)) >= 20
    for f in range(s.n_frames):   # the condition on the input: every frame keeps a clean majority
        mine = s.obs_frame == f
        assert s.outlier[mine].sum() <= 0.3 * mine.sum()
    rig, cov, inl, res = _run(s, inlier_px=8.0)
    print("outliers: %d of %d observations planted; flags differing from the mask: %d"
          % (int(s.outlier.sum()), n, int((inl != ~s.outlier).sum())))
    assert [r["status"] for r in res] == [_lib.LOC_OK] * s.n_frames
    assert (inl == ~s.outlier).all()
    _assert_clean(rig, cov, res)
    _check_against_host(oracle, s, rig, ~s.outlier, res, range(s.n_frames), True, "outliers")


# ---- 6. repeatability ----------------------------------------------------------------------------------------------

def _bits(rig, cov, inl, res):
    return (rig.tobytes(), cov.tobytes(), inl.tobytes(), json.dumps(res, sort_keys=True))


def test_a_frame_gives_the_same_bits_alone_in_the_batch_and_elsewhere():
    s = rc.rig_scene("config1_20x10", seed=8, outlier_frac=0.05, intr=INTR3, dist=DIST3)
    first, again = _run(s), _run(s)
    assert _bits(*first) == _bits(*again)
    rig, cov, inl, res = first
    K = s.n_rig_cams
    for f in (0, 7, 19):
        b, e = int(s.img_start[f * K]), int(s.img_start[f * K + K])
        r1, c1, f1, s1 = _run(rc.frames(s, [f]))
        assert r1.tobytes() == rig[f:f + 1].tobytes() and c1.tobytes() == cov[f:f + 1].tobytes()
        assert f1.tobytes() == inl[b:e].tobytes() and s1[0] == res[f]
    perm = [int(p) for p in np.random.default_rng(3).permutation(s.n_frames)]
    r2, c2, f2, s2 = _run(rc.frames(s, perm))
    idx = np.concatenate([np.arange(s.img_start[f * K], s.img_start[f * K + K]) for f in perm])
    assert r2.tobytes() == rig[perm].tobytes() and c2.tobytes() == cov[perm].tobytes()
    assert f2.tobytes() == inl[idx].tobytes() and s2 == [res[f] for f in perm]


# ---- 7. edges ------------------------------------------------------------------------------------------------------

def test_edges_empty_frame_single_observation_and_too_few_inliers():
    from visual_marker_mapping_amd import _lib
    full = rc.rig_scene("config1_20x10", noise_px=0.0)
    keep = np.ones(len(full.obs_tag), bool)
    keep[full.obs_frame == 0] = False                       # frame 0: nothing at all
    one = np.flatnonzero((full.obs_frame == 1) & (full.obs_cam == 2))[:1]
    keep[full.obs_frame == 1] = False
    keep[one] = True                                        # frame 1: one tag, seen by camera 2 only
    s = rc.frames(rc.select(full, keep), [0, 1, 2])
    assert _frame_counts(s) == [0, 1, _frame_counts(full)[2]]
    rig, cov, inl, res = _run(s)
    _assert_clean(rig, cov, res)
    assert res[0]["status"] == _lib.LOC_NO_OBSERVATIONS and res[0]["n_obs"] == 0 and res[0]["n_inlier_obs"] == 0
    assert (rig[0] == [1, 0, 0, 0, 0, 0, 0]).all() and (cov[0] == 0).all()
    assert res[1]["status"] == _lib.LOC_OK and res[1]["n_inlier_obs"] == 1 and inl[0]
    assert np.linalg.eigvalsh(cov[1]).min() > 0
    gq, gt = ys.pose_gap(rig[1:], s.rig_gt[1:])
    print("single observation in camera 2 and a full frame behind an empty one: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert gq <= 1e-9 and gt <= 1e-9 and res[2]["status"] == _lib.LOC_OK and inl.all()
    # min_inlier_tags counts over the frame: two cameras with one tag each pass a floor of two, one tag alone does not
    two = np.zeros(len(full.obs_tag), bool)
    for c in (0, 1):
        two[np.flatnonzero((full.obs_frame == 4) & (full.obs_cam == c))[:1]] = True
    rig, cov, inl, res = _run(rc.frames(rc.select(full, two), [4]), min_inlier_tags=2)
    assert res[0]["status"] == _lib.LOC_OK and res[0]["n_inlier_obs"] == 2
    assert max(ys.pose_gap(rig[0], full.rig_gt[4])) <= 1e-9
    rig, cov, inl, res = _run(rc.frames(s, [1]), min_inlier_tags=2)
    _assert_clean(rig, cov, res)
    assert res[0]["status"] == _lib.LOC_TOO_FEW_INLIERS and (cov[0] == 0).all()


def test_eight_cameras_with_yaws_spread_over_thirty_degrees(oracle):
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import make_rig_scene
    ext = np.array([rc.yaw(a, (0.1 * (k - 3.5), 0.02 * (k % 3), 0.0)) for k, a in enumerate(np.linspace(-15.0, 15.0, 8))])
    exact = make_rig_scene(1, ext, noise_px=0.0)
    counts = np.diff(exact.img_start).reshape(exact.n_frames, 8)
    assert exact.n_rig_cams == 8 and (counts.sum(axis=1) >= 20).all() and (counts > 0).sum(axis=1).min() >= 6
    rig, cov, inl, res = _run(exact)
    gq, gt = ys.pose_gap(rig, exact.rig_gt)
    print("K = 8 exact: %d observations, |dq| %.3g |dt| %.3g" % (len(exact.obs_tag), gq, gt))
    assert [r["status"] for r in res] == [_lib.LOC_OK] * exact.n_frames and inl.all()
    assert gq <= 1e-9 and gt <= 1e-9
    noisy = make_rig_scene(1, ext, seed=9)
    rig, cov, inl, res = _run(noisy)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * noisy.n_frames
    _check_against_host(oracle, noisy, rig, inl, res, (0, 9, 19), True, "K = 8")


# ---- 8. from per-camera localisation to the rig ---------------------------------------------------------------------

def test_per_camera_localisation_gives_the_starting_extrinsics():
    from visual_marker_mapping_amd import _lib, engine as eng
    s = rc.rig_scene("distortion_12x8", noise_px=0.0, intr=INTR3, dist=DIST3, missing=[(0, 1), (1, 0)])
    K, F = s.n_rig_cams, s.n_frames
    cam, res = np.zeros((F * K, 7)), [None] * (F * K)
    for c in range(K):   # engine.localize camera by camera, each under its own model
        slots = np.arange(F) * K + c
        idx = np.concatenate([np.arange(s.img_start[i], s.img_start[i + 1]) for i in slots]).astype(np.int64)
        start = np.zeros(F + 1, np.int64)
        start[1:] = np.cumsum(np.diff(s.img_start)[slots])
        q, _, _, r = eng.localize(s.intr[c], s.dist[c], s.tag_gt, s.tag_wh, start, s.obs_tag[idx], s.obs_px[idx])
        cam[slots] = q
        for f in range(F):
            res[f * K + c] = r[f]
    assert res[1]["status"] == _lib.LOC_NO_OBSERVATIONS and res[K]["status"] == _lib.LOC_NO_OBSERVATIONS
    ext = eng.rig_extrinsics_start(K, F, cam, res)
    gq, gt = ys.pose_gap(ext, s.ext_qt)
    print("starting extrinsics from exact per-camera poses: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert gq <= 1e-9 and gt <= 1e-9
    s.ext_qt = ext
    rig, cov, inl, rres = _run(s)
    assert [r["status"] for r in rres] == [_lib.LOC_OK] * F and inl.all()
    assert max(ys.pose_gap(rig, s.rig_gt)) <= 1e-9


# ---- 9. front ends -------------------------------------------------------------------------------------------------

def test_command_line_and_reconstructor_member_match_the_engine(tmp_path):
    import os
    from visual_marker_mapping_amd import _lib, io as vio, rig as rig_cli
    from visual_marker_mapping_amd.tag_reconstructor import (Camera, CameraModel, ReconstructedTag, TagReconstructor,
                                                             detection_result_from_arrays)
    missing = [(2, 1), (5, 0)]
    s = rc.rig_scene("distortion_12x8", seed=10, intr=INTR3, dist=DIST3, missing=missing)
    K, F = s.n_rig_cams, s.n_frames
    proj = str(tmp_path / "proj")
    os.makedirs(proj)
    models = [CameraModel(*[float(v) for v in s.intr[c]], distortionCoefficients=s.dist[c], verticalResolution=4000,
                          horizontalResolution=6000) for c in range(K)]
    for c, m in enumerate(models):
        vio.writeCameraModel(m, os.path.join(proj, "camera_%d.json" % c))
    det = detection_result_from_arrays(s.obs_frame * K + s.obs_cam, s.obs_tag, s.obs_px, s.tag_wh, F * K)
    vio.writeDetectionResult(det, os.path.join(proj, "marker_detections.json"))
    tags = {t: ReconstructedTag(t, "apriltag_36h11", s.tag_gt[t, :4], s.tag_gt[t, 4:], s.tag_wh[t, 0], s.tag_wh[t, 1])
            for t in range(len(s.tag_gt))}
    vio.exportReconstructions(os.path.join(proj, "reconstruction.json"), tags, {0: Camera(0, s.rig_gt[0, :4], s.rig_gt[0, 4:])},
                              models[0])
    names = [[None if (f, c) in missing else det.images[f * K + c].filename for f in range(F)] for c in range(K)]
    rig_cli.write_rig(os.path.join(proj, "rig.json"), ["camera_%d.json" % c for c in range(K)], names, s.ext_qt)
    rig, cov, inl, res = _run(s)
    assert rig_cli.main(["--project_path", proj]) == 0
    out = vio.read_json(os.path.join(proj, "rig_localization.json"))
    assert [int(fr["id"]) for fr in out["frames"]] == list(range(F)) and len(out["extrinsics"]) == K
    for f, fr in enumerate(out["frames"]):
        pose = np.array([float(v) for v in fr["rotation"]] + [float(v) for v in fr["translation"]])
        assert pose.tobytes() == rig[f].tobytes(), f
        assert fr["status"] == "ok" and int(fr["num_inlier_observations"]) == res[f]["n_inlier_obs"]
        assert np.array([float(v) for v in fr["covariance"]["coefficents"]]).tobytes() == cov[f].tobytes()
    for c, e in enumerate(out["extrinsics"]):
        assert np.array([float(v) for v in e["rotation"]] + [float(v) for v in e["translation"]]).tobytes() == s.ext_qt[c].tobytes()
    # the member of the reconstructor, with the extrinsics given ...
    rec = TagReconstructor(det)
    rec.setReconstructedTags(tags)
    frames = [[None if (f, c) in missing else f * K + c for c in range(K)] for f in range(F)]
    got = rec.computeRigPosesFromFrames(frames, models, s.ext_qt)
    assert sorted(got) == list(range(F))
    for f in range(F):
        assert np.concatenate([got[f].q, got[f].t]).tobytes() == rig[f].tobytes()
        r = rec.lastRigLocalizationReport["frames"][f]
        assert r["status"] == _lib.LOC_OK and r["inliers"].tobytes() == inl[s.obs_frame == f].tobytes()
    # ... and without: they come from the per-camera localisation (noisy data: close to the truth, not at it)
    rig_cli.write_rig(os.path.join(proj, "rig_free.json"), ["camera_%d.json" % c for c in range(K)], names)
    other = str(tmp_path / "free.json")
    assert rig_cli.main(["--project_path", proj, "--rig", os.path.join(proj, "rig_free.json"), "--output", other]) == 0
    got = rec.computeRigPosesFromFrames(frames, models)
    ext = rec.lastRigLocalizationReport["extrinsics"]
    gq, gt = ys.pose_gap(ext, s.ext_qt)
    print("extrinsics from the per-camera localisation of noisy images: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert (ext[0] == [1, 0, 0, 0, 0, 0, 0]).all() and gq <= 1e-2 and gt <= 1e-2 and sorted(got) == list(range(F))
    free = vio.read_json(other)
    for c, e in enumerate(free["extrinsics"]):
        assert np.array([float(v) for v in e["rotation"]] + [float(v) for v in e["translation"]]).tobytes() == ext[c].tobytes()
    for f, fr in enumerate(free["frames"]):
        assert np.array([float(v) for v in fr["rotation"]]).tobytes() == got[f].q.tobytes()


# ---- 10. a frame longer than its workgroup ---------------------------------------------------------------------------

def test_a_frame_of_more_observations_than_threads_agrees_with_the_yardstick(oracle):
    """k_rig_localize has one variant; its 256 threads stride the frame's list, so frames of 255, 256 and 257 and of
    more than two strides take every path of those loops.  The map lists the same tag poses under many ids."""
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import SyntheticScene
    base = rc.frames(rc.rig_scene("closeup_12x30", seed=12), [2, 10])
    n_tags, copies = len(base.tag_gt), 12
    per_frame = [int(np.sum(base.obs_frame == f)) for f in (0, 1)]
    assert min(per_frame) * copies >= 600
    d = dict(base.__dict__)
    K = base.n_rig_cams
    tag, px, frame, cam = [], [], [], []
    for f, want in ((0, 255), (1, 256), (0, 257), (1, 600)):   # four frames cut from the two, each tag under `copies` ids
        got = 0
        for c in range(K):
            mine = np.flatnonzero((base.obs_frame == f) & (base.obs_cam == c))
            share = want - got if c == K - 1 else min(want // K, len(mine) * copies)
            rep = np.resize(np.repeat(mine, copies), share)
            ids = base.obs_tag[rep] + n_tags * (np.arange(share) % copies)
            tag.append(ids)
            px.append(base.obs_px[rep])
            frame.append(np.full(share, len(frame) // K))
            cam.append(np.full(share, c))
            got += share
    d.update(tag_gt=np.tile(base.tag_gt, (copies, 1)), tag_wh=np.tile(base.tag_wh, (copies, 1)),
             obs_tag=np.concatenate(tag).astype(np.int32), obs_px=np.concatenate(px), obs_cam=np.concatenate(cam).astype(np.int32),
             obs_frame=np.concatenate(frame).astype(np.int32), rig_gt=base.rig_gt[[0, 1, 0, 1]], n_frames=4)
    d["outlier"] = np.zeros(len(d["obs_tag"]), bool)
    start = np.zeros(4 * K + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(d["obs_frame"].astype(np.int64) * K + d["obs_cam"], minlength=4 * K))
    d["img_start"] = start
    s = SyntheticScene(**d)
    assert _frame_counts(s) == [255, 256, 257, 600]
    rig, cov, inl, res = _run(s)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * 4 and [r["n_obs"] for r in res] == [255, 256, 257, 600]
    _assert_clean(rig, cov, res)
    _check_against_host(oracle, s, rig, inl, res, range(4), True, "long frames")
    for f in range(4):
        _, A, _ = rc.frame_normal(oracle, s, f, rig[f], s.ext_qt, inl, True)
        ref = np.linalg.inv(A)
        assert np.abs(cov[f] - ref).max() <= 1e-6 * np.abs(ref).max(), f


# ---- 11. calibration of the rig: vmm_ba_rig_calibrate ---------------------------------------------------------------

# A start that is degrees off puts the other cameras' corners hundreds of pixels away: the initial localisation must take
# them as inliers all the same for the first refinement to see them (the data of these tests hold no outliers); the
# reclassification passes then run at the default inlier_px under the refined extrinsics.
ROUGH_START = dict(loc_inlier_px=1e4)


def _calibrate(s, ext0, **kw):
    from visual_marker_mapping_amd import engine as eng
    return eng.rig_calibrate(s.intr, s.dist, ext0, s.tag_gt, s.tag_wh, s.img_start, s.obs_tag, s.obs_px, **kw)


def _perturbed(oracle, ext, which, deg=2.0, metres=0.03):
    """The extrinsics `which` turned by `deg` about (1, -2, 1.5) / |.| and shifted by `metres` along (2, 1, -2) / 3."""
    out = np.array(ext, np.float64)
    axis = np.array([1.0, -2.0, 1.5]) / np.linalg.norm([1.0, -2.0, 1.5])
    step = np.concatenate([metres * np.array([2.0, 1.0, -2.0]) / 3.0, 0.5 * np.radians(deg) * axis])
    for c in which:
        out[c] = oracle.pose_plus(ext[c], step)
    return out


@pytest.mark.parametrize("name", ["config1_20x10", "distortion_12x8"])
def test_calibration_recovers_perturbed_extrinsics_on_exact_data(oracle, name):
    from visual_marker_mapping_amd import _lib
    s = rc.rig_scene(name, noise_px=0.0)
    ext0 = _perturbed(oracle, s.ext_qt, (1, 2))
    assert max(ys.pose_gap(ext0[1:], s.ext_qt[1:])) > 0.01
    ext, ext_cov, rig, rig_cov, inl, res, rep = _calibrate(s, ext0, **ROUGH_START)
    ge, gr = ys.pose_gap(ext, s.ext_qt), ys.pose_gap(rig, s.rig_gt)
    print("%s exact: extrinsics |dq| %.3g |dt| %.3g, rig poses |dq| %.3g |dt| %.3g, report %s" % (name, *ge, *gr, rep))
    assert rep["status"] == _lib.CAL_OK and rep["n_frames_used"] == s.n_frames and rep["cams_refined"] == 0b110
    assert inl.all() and [r["status"] for r in res] == [_lib.LOC_OK] * s.n_frames
    assert max(ge) <= 1e-9 and max(gr) <= 1e-9
    assert ext[0].tobytes() == ext0[0].tobytes() and (ext_cov[:6] == 0).all() and (ext_cov[:, :6] == 0).all()
    assert np.isfinite(ext_cov).all() and np.isfinite(rig_cov).all()


@pytest.mark.parametrize("robustify", [0, 1])
@pytest.mark.parametrize("name,models", [("config1_20x10", False), ("distortion_12x8", True)])
def test_calibration_of_noisy_data_reaches_the_host_optimum_and_its_covariances(oracle, name, models, robustify):
    from visual_marker_mapping_amd import _lib
    kw = dict(intr=INTR3, dist=DIST3) if models else {}
    s = rc.rig_scene(name, seed=13, **kw)
    ext0 = _perturbed(oracle, s.ext_qt, (1, 2), deg=0.5, metres=0.01)
    ext, ext_cov, rig, rig_cov, inl, res, rep = _calibrate(s, ext0, robustify=robustify, **ROUGH_START)
    assert rep["status"] == _lib.CAL_OK and rep["n_frames_used"] == s.n_frames and rep["n_obs_used"] == int(inl.sum())
    h_rig, h_ext, h_cost, H = rc.host_rig_calibration(oracle, s, s.rig_gt, s.ext_qt, inl, bool(robustify), 0b110)
    ge, gr = ys.pose_gap(ext, h_ext), ys.pose_gap(rig, h_rig)
    ref_ext, ref_rig, scale = rc.joint_covariance(s, H, inl, 0b110)
    e_ext, e_rig = np.abs(ext_cov - ref_ext).max() / scale, np.abs(rig_cov - ref_rig).max() / scale
    print("%s robustify=%d: extrinsics |dq| %.3g |dt| %.3g, rig |dq| %.3g |dt| %.3g, cost device %.12g host %.12g, "
          "covariance error ext %.3g rig %.3g of max|ref|, trials %d accepted %d passes %d"
          % (name, robustify, *ge, *gr, rep["final_cost"], h_cost, e_ext, e_rig, rep["trials"], rep["accepted"], rep["passes"]))
    assert max(ge) <= 1e-6 and max(gr) <= 1e-6
    assert abs(rep["final_cost"] - h_cost) <= 1e-9 * h_cost
    assert e_ext <= 1e-6 and e_rig <= 1e-6
    assert np.abs(ext_cov[6:12, 12:18]).max() > 0 and (ext_cov == ext_cov.T).all()   # the cross block between cameras 1 and 2
    assert abs(sum(r["cost"] for r in res) - rep["final_cost"]) <= 1e-9 * rep["final_cost"]
    # bit-identical from run to run
    again = _calibrate(s, ext0, robustify=robustify, **ROUGH_START)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:5], (ext, ext_cov, rig, rig_cov, inl)))


def test_calibration_mask_holds_cameras_and_moves_the_gauge(oracle):
    from visual_marker_mapping_amd import _lib
    s = rc.rig_scene("config1_20x10", seed=14)
    ext0 = _perturbed(oracle, s.ext_qt, (2,), deg=0.5, metres=0.01)
    # cameras 0 and 1 held: their bits come back, their covariance rows and columns are zero
    ext, ext_cov, rig, rig_cov, inl, res, rep = _calibrate(s, ext0, refine_mask=0b100, **ROUGH_START)
    assert rep["status"] == _lib.CAL_OK and rep["cams_refined"] == 0b100
    assert ext[:2].tobytes() == ext0[:2].tobytes() and ext[2].tobytes() != ext0[2].tobytes()
    assert (ext_cov[:12] == 0).all() and (ext_cov[:, :12] == 0).all() and np.linalg.eigvalsh(ext_cov[12:, 12:]).min() > 0
    h_rig, h_ext, h_cost, _ = rc.host_rig_calibration(oracle, s, s.rig_gt, ext0, inl, True, 0b100)
    assert max(ys.pose_gap(ext, h_ext)) <= 1e-6 and max(ys.pose_gap(rig, h_rig)) <= 1e-6
    # holding camera 1 instead of camera 0 moves the gauge, not the rig: the same relative extrinsics
    a_ext = _calibrate(s, ext0, refine_mask=0b110, **ROUGH_START)[0]
    b_ext, _, _, _, _, _, b_rep = _calibrate(s, ext0, refine_mask=0b101, **ROUGH_START)
    assert b_rep["status"] == _lib.CAL_OK and b_rep["cams_refined"] == 0b101 and b_ext[1].tobytes() == ext0[1].tobytes()
    inv = lambda e: np.concatenate([e[:4] * [1, -1, -1, -1], -ys.rotation(e).T @ e[4:]])
    worst = 0.0
    for c in (1, 2):
        rel_a, rel_b = rc.compose(a_ext[c], inv(a_ext[0])), rc.compose(b_ext[c], inv(b_ext[0]))
        worst = max(worst, *ys.pose_gap(rel_a, rel_b))
    print("relative extrinsics with camera 0 held and with camera 1 held differ by %.3g" % worst)
    assert worst <= 1e-6
    # a camera in the mask without any image is not refined: its bits come back
    none = rc.rig_scene("config1_20x10", seed=14, missing=[(f, 1) for f in range(s.n_frames)])
    ext, ext_cov, _, _, _, _, rep = _calibrate(none, ext0, refine_mask=0b110, **ROUGH_START)
    assert rep["status"] == _lib.CAL_OK and rep["cams_refined"] == 0b100 and ext[1].tobytes() == ext0[1].tobytes()
    assert (ext_cov[6:12] == 0).all() and (ext_cov[:, 6:12] == 0).all()
    # all cameras free, or a bit above the rig: refused
    for bad in (0b111, 0b1000):
        with pytest.raises(_lib.VmmBaError):
            _calibrate(s, ext0, refine_mask=bad)


def test_calibration_with_camera_2_absent_from_every_other_frame(oracle):
    from visual_marker_mapping_amd import _lib
    s = rc.rig_scene("closeup_12x30", seed=15, missing=[(f, 2) for f in range(0, 12, 2)])
    ext0 = _perturbed(oracle, s.ext_qt, (1, 2), deg=0.5, metres=0.01)
    ext, ext_cov, rig, rig_cov, inl, res, rep = _calibrate(s, ext0, **ROUGH_START)
    assert rep["status"] == _lib.CAL_OK and rep["cams_refined"] == 0b110 and inl.all()
    h_rig, h_ext, h_cost, H = rc.host_rig_calibration(oracle, s, s.rig_gt, s.ext_qt, inl, True, 0b110)
    ge, gr = ys.pose_gap(ext, h_ext), ys.pose_gap(rig, h_rig)
    ref_ext, ref_rig, scale = rc.joint_covariance(s, H, inl, 0b110)
    print("camera 2 in every other frame: extrinsics |dq| %.3g |dt| %.3g, rig |dq| %.3g |dt| %.3g" % (*ge, *gr))
    assert max(ge) <= 1e-6 and max(gr) <= 1e-6 and abs(rep["final_cost"] - h_cost) <= 1e-9 * h_cost
    assert np.abs(ext_cov - ref_ext).max() <= 1e-6 * scale and np.abs(rig_cov - ref_rig).max() <= 1e-6 * scale


def test_from_per_camera_localisation_to_the_calibrated_rig():
    from visual_marker_mapping_amd import _lib, engine as eng
    s = rc.rig_scene("closeup_12x30", noise_px=0.0)
    K, F = s.n_rig_cams, s.n_frames
    cam, res = np.zeros((F * K, 7)), [None] * (F * K)
    for c in range(K):
        slots = np.arange(F) * K + c
        idx = np.concatenate([np.arange(s.img_start[i], s.img_start[i + 1]) for i in slots]).astype(np.int64)
        start = np.zeros(F + 1, np.int64)
        start[1:] = np.cumsum(np.diff(s.img_start)[slots])
        q, _, _, r = eng.localize(s.intr[c], s.dist[c], s.tag_gt, s.tag_wh, start, s.obs_tag[idx], s.obs_px[idx])
        cam[slots] = q
        for f in range(F):
            res[f * K + c] = r[f]
    ext0 = eng.rig_extrinsics_start(K, F, cam, res)
    ext, _, rig, _, inl, _, rep = _calibrate(s, ext0)
    ge, gr = ys.pose_gap(ext, s.ext_qt), ys.pose_gap(rig, s.rig_gt)
    print("localise per camera -> start -> calibrate: extrinsics |dq| %.3g |dt| %.3g, rig |dq| %.3g |dt| %.3g" % (*ge, *gr))
    assert rep["status"] == _lib.CAL_OK and inl.all() and max(ge) <= 1e-9 and max(gr) <= 1e-9


def test_calibration_of_eight_cameras_reaches_the_host_optimum(oracle):
    """K = 8: the reduced system is 48 x 48, so every strided loop of k_rigcal_frame and k_rigcal_solve takes several
    trips (1176 packed entries, records of 1277 doubles)."""
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import make_rig_scene
    ext_gt = np.array([rc.yaw(a, (0.1 * (k - 3.5), 0.02 * (k % 3), 0.0)) for k, a in enumerate(np.linspace(-15.0, 15.0, 8))])
    s = rc.frames(make_rig_scene(1, ext_gt, seed=16), range(8))
    assert s.n_rig_cams == 8 and (np.bincount(s.obs_cam, minlength=8) >= 20).all()
    ext0 = _perturbed(oracle, ext_gt, range(1, 8), deg=0.5, metres=0.01)
    ext, ext_cov, rig, rig_cov, inl, res, rep = _calibrate(s, ext0, **ROUGH_START)
    assert rep["status"] == _lib.CAL_OK and rep["cams_refined"] == 0xFE and inl.all()
    h_rig, h_ext, h_cost, H = rc.host_rig_calibration(oracle, s, s.rig_gt, ext_gt, inl, True, 0xFE)
    ge, gr = ys.pose_gap(ext, h_ext), ys.pose_gap(rig, h_rig)
    ref_ext, ref_rig, scale = rc.joint_covariance(s, H, inl, 0xFE)
    e_ext, e_rig = np.abs(ext_cov - ref_ext).max() / scale, np.abs(rig_cov - ref_rig).max() / scale
    print("K = 8: extrinsics |dq| %.3g |dt| %.3g, rig |dq| %.3g |dt| %.3g, cost device %.12g host %.12g, covariance error "
          "ext %.3g rig %.3g of max|ref|" % (*ge, *gr, rep["final_cost"], h_cost, e_ext, e_rig))
    assert max(ge) <= 1e-6 and max(gr) <= 1e-6 and abs(rep["final_cost"] - h_cost) <= 1e-9 * h_cost
    assert e_ext <= 1e-6 and e_rig <= 1e-6 and ext_cov.shape == (48, 48) and (ext_cov[:6] == 0).all()


def test_calibrating_front_ends_match_the_engine(tmp_path):
    import os
    from visual_marker_mapping_amd import _lib, io as vio, rig as rig_cli
    from visual_marker_mapping_amd.tag_reconstructor import (Camera, CameraModel, ReconstructedTag, TagReconstructor,
                                                             detection_result_from_arrays)
    s = rc.rig_scene("distortion_12x8", seed=17, intr=INTR3, dist=DIST3)
    K, F = s.n_rig_cams, s.n_frames
    proj = str(tmp_path / "proj")
    os.makedirs(proj)
    models = [CameraModel(*[float(v) for v in s.intr[c]], distortionCoefficients=s.dist[c], verticalResolution=4000,
                          horizontalResolution=6000) for c in range(K)]
    for c, m in enumerate(models):
        vio.writeCameraModel(m, os.path.join(proj, "camera_%d.json" % c))
    det = detection_result_from_arrays(s.obs_frame * K + s.obs_cam, s.obs_tag, s.obs_px, s.tag_wh, F * K)
    vio.writeDetectionResult(det, os.path.join(proj, "marker_detections.json"))
    tags = {t: ReconstructedTag(t, "apriltag_36h11", s.tag_gt[t, :4], s.tag_gt[t, 4:], s.tag_wh[t, 0], s.tag_wh[t, 1])
            for t in range(len(s.tag_gt))}
    vio.exportReconstructions(os.path.join(proj, "reconstruction.json"), tags, {0: Camera(0, s.rig_gt[0, :4], s.rig_gt[0, 4:])},
                              models[0])
    names = [[det.images[f * K + c].filename for f in range(F)] for c in range(K)]
    rig_cli.write_rig(os.path.join(proj, "rig.json"), ["camera_%d.json" % c for c in range(K)], names, s.ext_qt)
    ext, ext_cov, rig, rig_cov, inl, res, rep = _calibrate(s, s.ext_qt)
    assert rep["status"] == _lib.CAL_OK
    # the member of the reconstructor
    rec = TagReconstructor(det)
    rec.setReconstructedTags(tags)
    frames = [[f * K + c for c in range(K)] for f in range(F)]
    got = rec.calibrateRig(frames, models, s.ext_qt)
    assert got["extrinsics"].tobytes() == ext.tobytes() and got["covariance"].tobytes() == ext_cov.tobytes()
    assert got["status"] == _lib.CAL_OK and got["cams_refined"] == rep["cams_refined"] == 0b110
    assert sorted(got["rigs"]) == list(range(F))
    for f in range(F):
        assert np.concatenate([got["rigs"][f].q, got["rigs"][f].t]).tobytes() == rig[f].tobytes()
        assert got["frames"][f]["covariance"].tobytes() == rig_cov[f].tobytes()
    # the command line: rig_calibrated.json holds the refined extrinsics, rig_localization.json the frames under them
    assert rig_cli.main(["--project_path", proj, "--calibrate"]) == 0
    cal = vio.read_json(os.path.join(proj, "rig_calibrated.json"))
    assert cal["report"]["status"] == "ok" and int(cal["report"]["cams_refined"]) == 0b110
    for c, cam in enumerate(cal["cameras"]):
        e = cam["extrinsic"]
        assert np.array([float(v) for v in e["rotation"]] + [float(v) for v in e["translation"]]).tobytes() == ext[c].tobytes()
        assert np.array([float(v) for v in e["covariance"]["coefficents"]]).tobytes() == ext_cov[6 * c:6 * c + 6, 6 * c:6 * c + 6].tobytes()
    models2, ext2, images2 = rig_cli.read_rig(os.path.join(proj, "rig_calibrated.json"))   # it is a rig file again
    assert ext2.tobytes() == ext.tobytes() and images2 == names
    loc = vio.read_json(os.path.join(proj, "rig_localization.json"))
    s.ext_qt = ext
    again = _run(s)[0]
    for f, fr in enumerate(loc["frames"]):
        assert np.array([float(v) for v in fr["rotation"]] + [float(v) for v in fr["translation"]]).tobytes() == again[f].tobytes()
