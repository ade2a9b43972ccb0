"""CPU-only checks of the tag location (vmm_ba_locate_tags, ABI 6, additive): the host yardstick of its GPU tests
(tests/tag_cases.py) proven against the oracle, engine.pose_minus, the entry point declared, listed, exported, validating
its arguments and answering the trivial batches before any device call (so all of this passes without a GPU), and the tree
of map_check.json."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tag_cases as tc
import yardstick as ys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_check", "map_check.json")


def _scene(**kw):
    from visual_marker_mapping_amd.synthetic import make_scene
    return make_scene(1, **kw)


# ---- the yardstick ----------------------------------------------------------------------------------------------------

def test_tag_rows_jacobian_matches_central_differences_of_the_oracle(oracle):
    O = oracle
    s = _scene()
    start, order = tc.by_tag(s)
    h, worst = 1e-6, 0.0
    for t in (1, 4, 9):
        b, e = int(start[t]), int(start[t + 1])
        cams, pxs = s.obs_cam[order[b:e]], s.obs_px[order[b:e]]
        assert e - b >= 2
        q = O.pose_plus(s.tag_gt[t], np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.03]))   # away from the optimum
        rows = list(tc.tag_rows(O, s.intr, s.dist, q, s.cam_gt, s.tag_wh[t], cams, pxs))
        assert len(rows) == 4 * (e - b)
        J = np.vstack([Jt for _, Jt in rows])
        num = np.zeros_like(J)
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            up = np.concatenate([r for r, _ in tc.tag_rows(O, s.intr, s.dist, O.pose_plus(q, d), s.cam_gt, s.tag_wh[t], cams, pxs)])
            dn = np.concatenate([r for r, _ in tc.tag_rows(O, s.intr, s.dist, O.pose_plus(q, -d), s.cam_gt, s.tag_wh[t], cams, pxs)])
            num[:, k] = (up - dn) / (2 * h)
        err = np.abs(J - num).max() / np.abs(J).max()
        worst = max(worst, err)
        # central differences of step h on a smooth function: h^2 x third derivative, plus rounding eps |r| / h
        assert err <= 1e-7, (t, err)
    print("tag Jacobian against central differences: worst %.3g of max|J|" % worst)


def test_tag_optimum_recovers_the_truth_on_exact_data(oracle):
    O = oracle
    s = _scene(noise_px=0.0, outlier_frac=0.0)
    start, order = tc.by_tag(s)
    for t in (0, 3, 7):
        b, e = int(start[t]), int(start[t + 1])
        cams, pxs = s.obs_cam[order[b:e]], s.obs_px[order[b:e]]
        q0 = O.pose_plus(s.tag_gt[t], np.array([0.02, -0.01, 0.015, 0.01, 0.02, -0.015]))
        q, cost, grad = tc.tag_optimum(O, s.intr, s.dist, q0, s.cam_gt, s.tag_wh[t], cams, pxs, False)
        gq, gt = ys.pose_gap(q, s.tag_gt[t])
        print("tag %d: %d observations, |dq| %.3g |dt| %.3g cost %.3g scaled gradient %.3g" % (t, e - b, gq, gt, cost, grad))
        assert gq <= 1e-9 and gt <= 1e-9, (t, gq, gt)


def test_tag_propagated_is_the_first_order_effect_of_moving_one_camera(oracle):
    """Moving camera c by a small step dc moves the tag's optimum by -H^-1 G_c dc: with C_c = dc dc^T and every other
    covariance zero, tag_propagated is the outer product of that displacement."""
    O = oracle
    s = _scene()
    start, order = tc.by_tag(s)
    t = 4
    b, e = int(start[t]), int(start[t + 1])
    cams, pxs = s.obs_cam[order[b:e]], s.obs_px[order[b:e]]
    q, _, _ = tc.tag_optimum(O, s.intr, s.dist, s.tag_gt[t], s.cam_gt, s.tag_wh[t], cams, pxs, False)
    dc = 1e-6 * np.array([1.0, -2.0, 0.5, 1.5, -1.0, 2.0])
    moved = s.cam_gt.copy()
    moved[cams[0]] = O.pose_plus(moved[cams[0]], dc)
    q2, _, _ = tc.tag_optimum(O, s.intr, s.dist, q, moved, s.tag_wh[t], cams, pxs, False)
    cov = np.zeros((len(s.cam_gt), 6, 6))
    cov[cams[0]] = np.outer(dc, dc)
    P = tc.tag_propagated(O, s.intr, s.dist, q, s.cam_gt, cov, s.tag_wh[t], cams, pxs, False)
    step = tc.pose_minus(O, q2, q)
    # first order: the neglected terms are O(|dc|^2 x curvature) and the residuals' second-derivative term of the Gauss-Newton H
    assert np.abs(P - np.outer(step, step)).max() <= 2e-2 * np.abs(P).max()


def test_pose_minus_inverts_pose_plus(oracle):
    from visual_marker_mapping_amd import engine
    O = oracle
    rng = np.random.default_rng(11)
    worst = 0.0
    for n in range(200):
        b = np.concatenate([rng.normal(size=4), rng.uniform(-5, 5, 3)])
        b[:4] /= np.linalg.norm(b[:4])
        d = rng.uniform(-0.5, 0.5, 6) * (1.0 if n % 4 else 1e-6)
        a = O.pose_plus(b, d)
        got = engine.pose_minus(a, b)
        worst = max(worst, np.abs(got - d).max())
        assert np.abs(got - d).max() <= 1e-14 * max(1.0, np.abs(b[4:]).max()), (n, got, d)
        # the yardstick's own route (rotation matrices) agrees to its rounding
        assert np.abs(tc.pose_minus(O, a, b) - d).max() <= 1e-12
    assert (engine.pose_minus(b, b) == 0).all()
    flipped = np.concatenate([-a[:4], a[4:]])   # the same rotation, the other sign
    assert np.abs(engine.pose_minus(flipped, b) - d).max() <= 1e-14 * max(1.0, np.abs(b[4:]).max())
    print("pose_minus: worst |error| %.3g" % worst)


def test_map_check_statistic_is_delta_in_units_of_sigma(oracle):
    O = oracle
    m = np.array([1.0, 0, 0, 0, 0.5, -0.25, 2.0])
    d = np.array([0.003, 0.0, -0.004, 0.0, 0.002, 0.0])
    cov, cams = np.diag([1.0, 2.0, 4.0, 1.0, 2.0, 4.0]) * 1e-4, np.diag([3.0, 2.0, 0.0, 3.0, 2.0, 0.0]) * 1e-4
    delta, Sigma, d2 = tc.map_check_statistic(O, O.pose_plus(m, d), m, cov, cams, 0.5)
    np.testing.assert_allclose(delta, d, atol=1e-15)
    np.testing.assert_allclose(Sigma, 0.25 * (cov + cams), rtol=0, atol=0)
    np.testing.assert_allclose(d2, (0.003 ** 2 / 4 + 0.004 ** 2 / 4 + 0.002 ** 2 / 4) / 0.25e-4, rtol=1e-12)


# ---- the entry point --------------------------------------------------------------------------------------------------

def test_locate_tags_is_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    assert "vmm_ba_locate_tags" in _lib.EXPORTS and "vmm_ba_locate_tags" in declared
    assert hasattr(_lib.lib(), "vmm_ba_locate_tags")
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.lib().vmm_ba_abi_version() == 6


def _good():
    return dict(intr=np.array([1000.0, 1000.0, 500.0, 400.0]), dist=np.zeros(5),
                cam_qt=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1)), cam_cov=None, n_tags=2,
                tag_wh=np.full((2, 2), 0.1), tag_start=np.array([0, 2, 5], np.int64),
                obs_cam=np.array([0, 2, 0, 1, 2], np.int32), obs_px=np.ones((5, 8)), tag_qt=np.zeros((2, 7)))


def _call(intr, dist, cam_qt, cam_cov, n_tags, tag_wh, tag_start, obs_cam, obs_px, tag_qt, opt=None, n_cams=None, device=0):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_locate_tags(p(intr), p(dist), len(cam_qt) if n_cams is None else n_cams, p(cam_qt), p(cam_cov),
                                         n_tags, p(tag_wh), p(tag_start), p(obs_cam), p(obs_px), opt, p(tag_qt), None, None,
                                         None, None, device)


def test_locate_tags_refuses_bad_arguments_with_their_message_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    good = _good()

    def rejected(text, **kw):
        # device 1 << 20 does not exist: a call that got as far as the device would fail with VMM_BA_ERR_HIP instead
        assert _call(**dict(good, device=1 << 20, **kw)) == _lib.ERR_ARGUMENT, kw
        assert _lib.lib().vmm_ba_last_error().decode() == "vmm_ba_locate_tags: " + text, kw

    rejected("null camera model", intr=None)
    rejected("null camera model", dist=None)
    rejected("null tag_start or tag_qt", tag_start=None)
    rejected("null tag_start or tag_qt", tag_qt=None)
    rejected("null tag_wh", tag_wh=None)
    rejected("negative size", n_tags=-1)
    rejected("negative size", n_cams=-1)
    rejected("tag_start[0] is not 0", tag_start=np.array([1, 2, 5], np.int64))
    rejected("tag_start decreases", tag_start=np.array([0, 5, 2], np.int64))
    rejected("null observations", obs_cam=None)
    rejected("null observations", obs_px=None)
    rejected("obs_cam outside [0, n_cams)", obs_cam=np.array([0, 3, 0, 1, 2], np.int32))
    rejected("obs_cam outside [0, n_cams)", obs_cam=np.array([-1, 2, 0, 1, 2], np.int32))
    rejected("obs_cam is not strictly increasing within a tag", obs_cam=np.array([0, 2, 0, 1, 1], np.int32))
    rejected("obs_cam is not strictly increasing within a tag", obs_cam=np.array([2, 0, 0, 1, 2], np.int32))
    rejected("null cam_qt", cam_qt=None, n_cams=3)
    for v in (np.nan, np.inf):
        rejected("non-finite camera model", intr=np.array([1000.0, v, 500.0, 400.0]))
        rejected("non-finite camera model", dist=np.array([0.0, 0.0, v, 0.0, 0.0]))
        for col in (0, 5):
            bad = good["cam_qt"].copy()
            bad[1, col] = v
            rejected("non-finite camera pose", cam_qt=bad)
        bad = good["tag_wh"].copy()
        bad[1, 0] = v
        rejected("non-finite tag size", tag_wh=bad)
        bad = good["obs_px"].copy()
        bad[4, 7] = v
        rejected("non-finite obs_px", obs_px=bad)
        bad = np.tile(np.eye(6), (3, 1, 1))
        bad[2, 5, 5] = v
        rejected("non-finite cam_cov", cam_cov=bad)
    zero_q = good["cam_qt"].copy()
    zero_q[2, :4] = 0.0
    rejected("zero camera quaternion", cam_qt=zero_q)
    bad_options = [dict(refine_iterations=-1), dict(reclassify_passes=-1), dict(min_inlier_tags=0)]
    for field in ("huber_a", "score_cap_px", "inlier_px"):
        bad_options += [{field: v} for v in (0.0, -1.0, np.nan, np.inf)]
    for kw in bad_options:
        o = engine.default_localize_options(**kw)
        rejected("bad localisation options", opt=C.byref(o))
        # an empty batch is answered before the options are looked at
        assert _call(**dict(good, n_tags=0, opt=C.byref(o), device=1 << 20)) == _lib.OK, kw
    # the Python wrapper refuses arrays that do not fit together, and unknown options
    g = _good()
    args = (g["intr"], g["dist"], g["cam_qt"], g["tag_wh"], g["tag_start"], g["obs_cam"], g["obs_px"])
    with pytest.raises(ValueError):
        engine.locate_tags(*args[:4], [0, 2], g["obs_cam"], g["obs_px"])
    with pytest.raises(ValueError):
        engine.locate_tags(*args[:6], g["obs_px"][:4])
    with pytest.raises(ValueError):
        engine.locate_tags(*args, cam_cov=np.zeros((2, 6, 6)))
    with pytest.raises(AttributeError):
        engine.locate_tags(*args, no_such_option=1)
    with pytest.raises(_lib.VmmBaError) as ei:
        engine.locate_tags(*args[:5], np.array([0, 2, 0, 1, 7], np.int32), g["obs_px"], device=1 << 20)
    assert ei.value.status == _lib.ERR_ARGUMENT


def test_trivial_batches_are_answered_without_a_device():
    from visual_marker_mapping_amd import _lib, engine
    g = _good()
    assert _call(**dict(g, n_tags=0, device=1 << 20)) == _lib.OK
    out = engine.locate_tags(g["intr"], g["dist"], g["cam_qt"], np.zeros((0, 2)), [0], np.zeros(0, np.int32), np.zeros((0, 8)),
                             device=1 << 20)
    assert out[0].shape == (0, 7) and out[1].shape == (0, 6, 6) and out[2].shape == (0, 6, 6) and out[4] == []
    # no tag has an observation: NO_OBSERVATIONS, the identity pose and zeros, whatever the outputs held
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    start = np.zeros(3, np.int64)
    qt, cov, cams = np.full((2, 7), 7.0), np.full((2, 36), 7.0), np.full((2, 36), 7.0)
    res = (_lib.LocalizeResult * 2)()
    for r in res:
        r.status, r.n_obs, r.n_inlier_obs, r.trials, r.rms_px, r.cost = 9, 9, 9, 9, 9.0, 9.0
    assert L.vmm_ba_locate_tags(p(g["intr"]), p(g["dist"]), 3, p(g["cam_qt"]), None, 2, p(g["tag_wh"]), p(start), None, None,
                                None, p(qt), p(cov), p(cams), None, C.cast(res, C.c_void_p), 1 << 20) == _lib.OK
    assert (qt == [1, 0, 0, 0, 0, 0, 0]).all() and (cov == 0).all() and (cams == 0).all()
    assert [(r.status, r.n_obs, r.n_inlier_obs, r.trials, r.rms_px, r.cost) for r in res] \
        == [(_lib.LOC_NO_OBSERVATIONS, 0, 0, 0, 0.0, 0.0)] * 2
    # with an observation the call does go to the device
    assert _call(**dict(g, device=1 << 20)) == _lib.ERR_HIP
    assert L.vmm_ba_last_error().decode().startswith("vmm_ba_locate_tags: hipSetDevice: ")


# ---- the tree of map_check.json ---------------------------------------------------------------------------------------

def _report():
    from visual_marker_mapping_amd import _lib
    cov = np.diag([1.0, 4.0, 9.0, 16.0, 25.0, 36.0]) * 1e-8
    cov[0, 5] = cov[5, 0] = 1.25e-9
    return {"rounds": 2, "sigma_px": 0.5, "chi2_threshold": 22.458,
            "images": {3: _lib.LOC_OK, 1: _lib.LOC_TOO_FEW_INLIERS, 2: _lib.LOC_NO_OBSERVATIONS},
            "tags": {12: {"status": _lib.LOC_OK, "n_obs": 5, "n_inlier_obs": 4, "rms_px": 0.375,
                          "pose": np.array([0.5, 0.5, -0.5, 0.5, 1.0, -2.0, 1.0 / 3.0]), "covariance": cov,
                          "delta": np.array([0.02, 0.0, -0.001, 0.0, 0.005, 0.0]), "mahalanobis2": 1900.5,
                          "max_corner_displacement": 0.0203125, "moved": True},
                     4: {"status": _lib.LOC_SINGULAR, "n_obs": 2, "n_inlier_obs": 2, "rms_px": 0.0,
                         "pose": np.array([1.0, 0, 0, 0, 0, 0, 0]), "covariance": np.zeros((6, 6)), "delta": np.zeros(6),
                         "mahalanobis2": 0.0, "max_corner_displacement": 0.0, "moved": False}},
            "skipped": [9, 7], "moved": [12]}


def test_map_check_tree_is_written_as_the_golden_text(tmp_path):
    from visual_marker_mapping_amd import io as vio, map_check
    tree = map_check.map_check_tree(_report())
    assert list(tree) == ["rounds", "sigma_px", "chi2_threshold", "tags", "skipped_tags", "images"]
    assert [t["id"] for t in tree["tags"]] == [4, 12] and [i["id"] for i in tree["images"]] == [1, 2, 3]
    assert list(tree["tags"][1]) == ["id", "rotation", "translation", "status", "num_views", "num_inlier_views", "rms_px",
                                    "covariance", "delta", "mahalanobis2", "max_corner_displacement", "moved"]
    out = str(tmp_path / "map_check.json")
    vio.write_json(out, tree)
    with open(GOLDEN) as f, open(out) as g:
        assert g.read() == f.read()
    back = vio.read_json(out)
    assert back["tags"][1]["moved"] == "true" and back["tags"][0]["status"] == "singular"
    assert vio.matrixFromPropertyTree(back["tags"][1]["covariance"], 6, 6)[0, 5] == 1.25e-9


def test_map_check_main_names_the_missing_file(tmp_path):
    from visual_marker_mapping_amd import map_check
    proj = str(tmp_path)
    with pytest.raises(FileNotFoundError) as ei:
        map_check.main(["--project_path", proj])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
    with pytest.raises(FileNotFoundError) as ei:
        map_check.main(["--project_path", proj, "--map", str(tmp_path / "my_map.json")])
    assert "my_map.json" in str(ei.value)
    open(os.path.join(proj, "reconstruction.json"), "w").write("{}")
    with pytest.raises(FileNotFoundError) as ei:
        map_check.main(["--project_path", proj])
    assert "marker_detections.json" in str(ei.value) and "does not exist" in str(ei.value)
