"""GPU tests of the localisation-accuracy prediction (vmm_ba_predict_localization, engine.predict_localization, the
reconstructor's member and the coverage step).

Yardstick throughout: tests/predict_cases.py -- the visibility rules in numpy, H, G_t and the sandwich from
oracle.obs_eval's Jacobians, inverses by cov_cases.refined_inverse; it never calls the code under test, and
tests/test_predict_cpu.py shows that no flag of its cases rests on rounding.  Tolerances: flags exact; covariances to
1e-6 x max|ref| as the existing covariance tests (test_gpu_localize.py); sigmas 1e-6 relative;
against the localisation 2e-6 x max|ref| (each side within 1e-6 of the same inverse) and the localisation test's own
1e-9 on the recovered pose.
tests/test_finished_map_accuracy.py supersedes in strength the COV_REL comparisons of cov_px and cov_map and the 1e-6
comparison of the sigmas: there every entry and both sigmas are held to float64 accuracy, at 1 to 129 tags in depth.
"""
import os
import shutil

import numpy as np
import pytest

import predict_cases as pc
import yardstick as ys

pytestmark = pytest.mark.gpu

COV_REL = 1e-6


def _predict(case, **kw):
    from visual_marker_mapping_amd import engine as eng
    return eng.predict_localization(case["intr"], case["dist"], case["tag_qt"], case["tag_wh"], case["cam_qt"], case["size"],
                                    want_visible=True, **kw)


def _assert_zero(cov_px, cov_map, r):
    assert not cov_px.any() and not cov_map.any() and r["sigma_pos_m"] == 0.0 and r["sigma_rot_rad"] == 0.0, r


@pytest.fixture(scope="module")
def scene():
    return pc.scene()


@pytest.fixture(scope="module")
def scene_cov():
    return pc.random_tag_cov(10, fixed=0)


@pytest.fixture(scope="module")
def scene_runs(scene, scene_cov):
    """The scene predicted once without and once with tag covariances; shared, never changed."""
    return _predict(scene), _predict(scene, tag_cov=scene_cov)


# ---- 1. visibility and statuses --------------------------------------------------------------------------------------

def test_visibility_equals_the_host_model_on_every_case():
    from visual_marker_mapping_amd import _lib
    n_none = 0
    for name, case in pc.all_cases():
        want, _ = pc.host_visible(case)
        cov_px, cov_map, res, vis = _predict(case)
        assert vis.shape == want.shape and (vis == want).all(), (name, np.argwhere(vis != want).tolist())
        assert [r["n_visible"] for r in res] == want.sum(axis=1).tolist(), name
        for p, r in enumerate(res):
            if want[p].sum() == 0:
                assert r["status"] == _lib.PRED_NO_VISIBLE_TAG, (name, p, r)
                _assert_zero(cov_px[p], cov_map[p], r)
                n_none += 1
            else:
                assert r["status"] in (_lib.PRED_OK, _lib.PRED_SINGULAR), (name, p, r)
        assert np.isfinite(cov_px).all() and np.isfinite(cov_map).all()
    assert n_none >= 3   # lanes with one tag: the later poses look away from it


def test_edges_under_other_options_and_too_few_tags():
    from visual_marker_mapping_amd import _lib
    case = pc.edges()
    for opt in (dict(min_side_px=0.0), dict(margin_px=25.0), dict(max_view_angle_deg=80.0)):
        want, sl = pc.host_visible(case, opt)
        assert not any(pc.rests_on_rounding(s) for s in sl[0]), opt
        _, _, res, vis = _predict(case, **opt)
        assert (vis == want).all() and res[0]["n_visible"] == want.sum(), opt
    # a pose looking away: nothing in view
    away = dict(case, cam_qt=np.array([np.concatenate([pc.axis_angle([0, 1, 0], 180.0), [0, 0, 0]])]))
    cov_px, cov_map, res, vis = _predict(away)
    assert (vis == pc.host_visible(away)[0]).all() and vis.sum() <= 1
    # tags 2..7 and 9 alone: one tag in view, min_tags = 2
    keep = [1, 2, 3, 4, 5, 6, 8]
    one = dict(case, tag_qt=case["tag_qt"][keep], tag_wh=case["tag_wh"][keep])
    cov_px, cov_map, res, vis = _predict(one, min_tags=2)
    assert vis[0].tolist() == [False] * 6 + [True] and res[0]["n_visible"] == 1
    assert res[0]["status"] == _lib.PRED_TOO_FEW_TAGS
    _assert_zero(cov_px[0], cov_map[0], res[0])
    cov_px, cov_map, res, vis = _predict(one)
    assert res[0]["status"] == _lib.PRED_OK and cov_px[0].any()
    # all nine tags hidden behind min_tags = 4
    cov_px, cov_map, res, vis = _predict(case, min_tags=4)
    assert res[0]["status"] == _lib.PRED_TOO_FEW_TAGS and res[0]["n_visible"] == 3
    _assert_zero(cov_px[0], cov_map[0], res[0])
    none = dict(case, tag_qt=case["tag_qt"][[1, 3]], tag_wh=case["tag_wh"][[1, 3]])
    cov_px, cov_map, res, vis = _predict(none)
    assert res[0]["status"] == _lib.PRED_NO_VISIBLE_TAG and not vis.any()
    _assert_zero(cov_px[0], cov_map[0], res[0])


# ---- 2. cov_px -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edges", "lanes_130x5", "scene"])
def test_cov_px_is_the_scaled_inverse_of_the_normal_matrix(oracle, name):
    from visual_marker_mapping_amd import _lib
    case = dict(pc.all_cases())[name]
    cov_px, _, res, vis = _predict(case)
    worst = 0.0
    for p, r in enumerate(res):
        if r["status"] != _lib.PRED_OK:
            continue
        ref = pc.host_pose(oracle, case, p, vis[p])[0]
        err = np.abs(cov_px[p] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= COV_REL, (name, p, err)
        assert (cov_px[p] == cov_px[p].T).all() and np.linalg.eigvalsh(cov_px[p]).min() > 0, (name, p)
    assert sum(r["status"] == _lib.PRED_OK for r in res) >= 1
    print("%s: worst cov_px error %.3g of max|ref|" % (name, worst))
    # exact scaling with sigma_px^2
    worst_ratio = 0.0
    for sigma, exact in ((2.0, True), (0.5, True), (3.0, False), (0.3, False)):
        scaled = _predict(case, sigma_px=sigma)[0]
        want = (sigma * sigma) * cov_px
        if exact:   # the ratio is a power of four: bitwise
            assert scaled.tobytes() == want.tobytes(), (name, sigma)
        nz = want != 0
        ulps = np.abs(scaled[nz] - want[nz]) / np.spacing(np.abs(want[nz]))
        worst_ratio = max(worst_ratio, float(np.abs(scaled[nz] / cov_px[nz] / (sigma * sigma) - 1).max()))
        assert (scaled[~nz] == 0).all() and ulps.max() <= 1.0, (name, sigma, ulps.max())
    print("%s: worst |ratio / sigma^2 - 1| %.3g" % (name, worst_ratio))


# ---- 3. the localisation it predicts ---------------------------------------------------------------------------------------

def test_prediction_agrees_with_the_localisation_of_noise_free_pixels(oracle, scene, scene_runs):
    from visual_marker_mapping_amd import _lib, engine as eng
    (cov_px, _, res, vis), _ = scene_runs
    ok = [p for p, r in enumerate(res) if r["status"] == _lib.PRED_OK]
    assert len(ok) >= 30
    start, tags, px = [0], [], []
    for p in ok:
        for t in np.flatnonzero(vis[p]):
            tags.append(t)
            px.append(pc.projected(oracle, scene, p, t))
        start.append(len(tags))
    cam, cam_cov, inl, lres = eng.localize(scene["intr"], scene["dist"], scene["tag_qt"], scene["tag_wh"], np.array(start, np.int64),
                                           np.array(tags, np.int32), np.array(px), robustify=0)
    assert [r["status"] for r in lres] == [_lib.LOC_OK] * len(ok) and inl.all()
    gq, gt = ys.pose_gap(cam, scene["cam_qt"][ok])
    worst = 0.0
    for k, p in enumerate(ok):
        err = np.abs(cam_cov[k] - cov_px[p]).max() / np.abs(cov_px[p]).max()   # sigma_px = 1
        worst = max(worst, err)
        assert err <= 2 * COV_REL, (p, err)
    print("localisation of the predicted pixels: |dq| %.3g |dt| %.3g, worst covariance gap %.3g of max|ref|" % (gq, gt, worst))
    assert gq <= 1e-9 and gt <= 1e-9, (gq, gt)


# ---- 4. cov_map, 5. sigmas ---------------------------------------------------------------------------------------------------

def test_cov_map_is_the_sandwich_and_the_sigmas_follow(oracle, scene, scene_cov, scene_runs):
    from visual_marker_mapping_amd import _lib
    (cov_px0, cov_map0, res0, vis0), (cov_px, cov_map, res, vis) = scene_runs
    assert (vis == vis0).all()
    assert cov_px.tobytes() == cov_px0.tobytes()          # bitwise the same with and without tag_cov
    assert not cov_map0.any()                             # tag_cov = None: exact zeros
    worst = worst_s = 0.0
    for p, r in enumerate(res):
        assert r["status"] == res0[p]["status"] and r["n_visible"] == res0[p]["n_visible"]
        for run_cov_px, run_cov_map, run_r in ((cov_px0[p], cov_map0[p], res0[p]), (cov_px[p], cov_map[p], r)):
            if r["status"] != _lib.PRED_OK:
                _assert_zero(run_cov_px, run_cov_map, run_r)
                continue
            want = pc.host_sigmas(scene["cam_qt"][p], run_cov_px + run_cov_map)
            for got, ref in zip((run_r["sigma_pos_m"], run_r["sigma_rot_rad"]), want):
                worst_s = max(worst_s, abs(got - ref) / ref)
                assert abs(got - ref) <= 1e-6 * ref, (p, got, ref)
        if r["status"] != _lib.PRED_OK:
            continue
        ref = pc.host_pose(oracle, scene, p, vis[p], tag_cov=scene_cov)[1]
        err = np.abs(cov_map[p] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= COV_REL, (p, err)
        assert (cov_map[p] == cov_map[p].T).all()
        # positive semi-definite: an eigenvalue of a symmetric 6 x 6 matrix is computed to a few ulps of its norm
        assert np.linalg.eigvalsh(cov_map[p]).min() >= -64 * np.finfo(float).eps * np.abs(cov_map[p]).max(), p
        assert r["sigma_pos_m"] > res0[p]["sigma_pos_m"] or not vis[p][1:].any()
    print("scene: worst cov_map error %.3g of max|ref|, worst sigma error %.3g" % (worst, worst_s))
    # all zeros: exact zeros
    z = _predict(scene, tag_cov=np.zeros((10, 6, 6)))
    assert not z[1].any() and z[0].tobytes() == cov_px0.tobytes()
    assert [(r["sigma_pos_m"], r["sigma_rot_rad"]) for r in z[2]] == [(r["sigma_pos_m"], r["sigma_rot_rad"]) for r in res0]
    # a covariance on one tag only changes cov_map for exactly the poses that see it
    for t in (3, 8):
        one = np.zeros((10, 6, 6))
        one[t] = scene_cov[t]
        got = _predict(scene, tag_cov=one)[1]
        changed = np.array([m.any() for m in got])
        sees = vis[:, t] & np.array([r["status"] == _lib.PRED_OK for r in res])
        assert (changed == sees).all() and sees.any() and not sees.all(), t


# ---- 6. independence -----------------------------------------------------------------------------------------------------

def _bits(out):
    cov_px, cov_map, res, vis = out
    return cov_px.tobytes(), cov_map.tobytes(), vis.tobytes(), res


@pytest.mark.parametrize("with_cov", [False, True])
def test_a_pose_gives_the_same_bytes_alone_in_the_batch_permuted_and_again(scene, scene_cov, scene_runs, with_cov):
    kw = dict(tag_cov=scene_cov) if with_cov else {}
    first = scene_runs[1 if with_cov else 0]
    assert _bits(_predict(scene, **kw)) == _bits(first)
    cov_px, cov_map, res, vis = first
    n = len(res)
    for p in range(n):
        alone = _predict(dict(scene, cam_qt=scene["cam_qt"][p:p + 1]), **kw)
        assert _bits(alone) == (cov_px[p:p + 1].tobytes(), cov_map[p:p + 1].tobytes(), vis[p:p + 1].tobytes(), res[p:p + 1]), p
    perm = np.random.default_rng(5).permutation(n)
    shuffled = _predict(dict(scene, cam_qt=scene["cam_qt"][perm]), **kw)
    assert _bits(shuffled) == (cov_px[perm].tobytes(), cov_map[perm].tobytes(), vis[perm].tobytes(), [res[p] for p in perm])


# ---- 7. never NaN ----------------------------------------------------------------------------------------------------------

def test_a_tag_of_zero_size_gives_finite_outputs():
    from visual_marker_mapping_amd import _lib
    case = pc.edges()
    point = dict(case, tag_qt=case["tag_qt"][:1], tag_wh=np.zeros((1, 2)))
    for kw in (dict(), dict(tag_cov=pc.random_tag_cov(1, fixed=-1))):
        cov_px, cov_map, res, vis = _predict(point, min_side_px=0.0, **kw)
        assert vis.all() and res[0]["n_visible"] == 1
        assert np.isfinite(cov_px).all() and np.isfinite(cov_map).all()
        assert np.isfinite(res[0]["sigma_pos_m"]) and np.isfinite(res[0]["sigma_rot_rad"])
        assert res[0]["status"] in (_lib.PRED_OK, _lib.PRED_SINGULAR)
        print("zero-size tag: status %d" % res[0]["status"])
        if res[0]["status"] == _lib.PRED_SINGULAR:
            _assert_zero(cov_px[0], cov_map[0], res[0])


# ---- 8. upper layers -------------------------------------------------------------------------------------------------------

def test_reconstructor_member_and_command_line_match_the_engine(tmp_path, capsys, scene, scene_cov, scene_runs):
    from visual_marker_mapping_amd import _lib, coverage, engine as eng, io as vio, uncertainty
    from visual_marker_mapping_amd.synthetic import make_scene, write_project
    from visual_marker_mapping_amd.tag_reconstructor import Camera, TagReconstructor
    s = make_scene(1)
    proj = str(tmp_path / "proj")
    model, det = write_project(s, proj)
    assert (model.horizontalResolution, model.verticalResolution) == scene["size"]
    shutil.copy(os.path.join(proj, "ground_truth.json"), os.path.join(proj, "reconstruction.json"))
    tags, _, _ = vio.parseReconstructions(os.path.join(proj, "reconstruction.json"))
    # the member, poses as an array and as a map of cameras under other ids
    rec = TagReconstructor(det)
    rec.setCameraModel(model)
    rec.setReconstructedTags(tags)
    covs = {t: scene_cov[t] for t in range(1, 10)}   # the origin tag has no entry
    cov_px, cov_map, res, vis = scene_runs[1]
    by_array = rec.predictLocalizationAccuracy(scene["cam_qt"], tagCovariances=covs)
    cams = {100 + 2 * p: Camera(100 + 2 * p, q[:4], q[4:]) for p, q in enumerate(scene["cam_qt"])}
    by_map = rec.predictLocalizationAccuracy(cams, tagCovariances=covs)
    for p in range(len(res)):
        for r in (by_array[p], by_map[100 + 2 * p]):
            assert {k: r[k] for k in res[p]} == res[p]
            assert r["covariance"].tobytes() == cov_px[p].tobytes() and r["covariance_map"].tobytes() == cov_map[p].tobytes()
            assert r["visible_tags"] == np.flatnonzero(vis[p]).tolist() and r["pose"].tobytes() == scene["cam_qt"][p].tobytes()
    plain = rec.predictLocalizationAccuracy(scene["cam_qt"][:3], sigma_px=2.0, image_width=3000)
    want = eng.predict_localization(s.intr, s.dist, s.tag_gt, s.tag_wh, scene["cam_qt"][:3], (3000, 4000), sigma_px=2.0)
    assert all(plain[p]["covariance"].tobytes() == want[0][p].tobytes() and not plain[p]["covariance_map"].any() for p in range(3))

    def check(path, poses, out, with_matrices):
        tree = vio.read_json(path)
        assert [int(e["id"]) for e in tree["poses"]] == list(range(len(poses)))
        for p, e in enumerate(tree["poses"]):
            pose = np.array([float(v) for v in e["rotation"]] + [float(v) for v in e["translation"]])
            assert pose.tobytes() == poses[p].tobytes(), p
            assert e["status"] == _lib.PRED_STATUS_NAMES[out[2][p]["status"]] and int(e["num_visible_tags"]) == out[2][p]["n_visible"]
            assert float(e["sigma_pos_m"]) == out[2][p]["sigma_pos_m"] and float(e["sigma_rot_rad"]) == out[2][p]["sigma_rot_rad"]
            assert ("covariance" in e) == with_matrices
            if with_matrices:
                assert vio.matrixFromPropertyTree(e["covariance"], 6, 6).tobytes() == out[0][p].tobytes()
                assert vio.matrixFromPropertyTree(e["covariance_map"], 6, 6).tobytes() == out[1][p].tobytes()
        seen = out[3].sum(axis=0)
        assert [(int(e["id"]), int(e["num_poses"])) for e in tree["tags"]] == [(t, int(seen[t])) for t in range(10)]
        never = tree["tags_never_seen"]
        assert [int(t) for t in (never if never != "" else [])] == [t for t in range(10) if seen[t] == 0]
        return tree

    # --poses: the map's own cameras, with the tags' covariances from an uncertainty file
    unc = os.path.join(proj, "reconstruction_uncertainty.json")
    uncertainty.write_uncertainty(unc, 0, False, covs, {})
    assert coverage.main(["--project_path", proj, "--poses", os.path.join(proj, "ground_truth.json"), "--uncertainty", unc,
                          "--covariances"]) == 0
    want = eng.predict_localization(s.intr, s.dist, s.tag_gt, s.tag_wh, s.cam_gt, scene["size"], tag_cov=scene_cov,
                                    want_visible=True)
    check(os.path.join(proj, "coverage.json"), s.cam_gt, want, True)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("Predicted 20 poses: 100.0 % ok, sigma_pos_m median ") and "; 0 tags never seen; wrote " in line
    # --grid with options and another output file
    other = str(tmp_path / "grid.json")
    centres = np.array([pc.camera_centre(q) for q in s.cam_gt])
    lo, hi = centres.min(axis=0), centres.max(axis=0)
    axes = [[0.0, 0.0, -1.0], [0.3, 0.0, -1.0]]
    grid = [str(float(v)) for d in range(3) for v in (lo[d], hi[d], (3, 2, 2)[d])]
    argv = ["--project_path", proj, "--grid"] + grid + ["--up", "0", "1", "0", "--min_tags", "2", "--sigma_px", "0.5",
                                                        "--output", other]
    for a in axes:
        argv += ["--axis"] + [str(v) for v in a]
    assert coverage.main(argv) == 0
    poses = eng.grid_poses(lo, hi, (3, 2, 2), axes, (0, 1, 0))
    want = eng.predict_localization(s.intr, s.dist, s.tag_gt, s.tag_wh, poses, scene["size"], want_visible=True, min_tags=2,
                                    sigma_px=0.5)
    tree = check(other, poses, want, False)
    assert tree["options"]["min_tags"] == "2" and float(tree["options"]["sigma_px"]) == 0.5
    assert (tree["options"]["image_width"], tree["options"]["image_height"]) == ("6000", "4000")
    assert any(r["status"] == _lib.PRED_OK for r in want[2])
