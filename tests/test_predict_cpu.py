"""CPU-only checks of the localisation-accuracy prediction (vmm_ba_predict_localization, ABI 6, additive): the test cases
themselves (no flag of predict_cases rests on rounding, `edges` rejects every tag for the intended rule only), the host
formula of the camera centre's covariance against finite differences, the entry declared, exported and validating its
arguments before any device call, engine.grid_poses and the coverage step's tree and command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import predict_cases as pc
import yardstick as ys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "vmm_ba_predict_localization"


# ---- the cases -------------------------------------------------------------------------------------------------------

def test_no_flag_of_any_case_rests_on_rounding():
    """A condition on the inputs, not a measurement: every quantity that decides a flag is at least predict_cases.MARGIN
    away from its threshold."""
    for name, case in pc.all_cases():
        vis, sl = pc.host_visible(case)
        near = [(p, t) for p, row in enumerate(sl) for t, s in enumerate(row) if pc.rests_on_rounding(s)]
        print("%s: %d poses x %d tags, visible per pose %s" % (name, vis.shape[0], vis.shape[1], vis.sum(axis=1).tolist()))
        assert not near, (name, near)
    # and under the options the GPU test changes
    for opt in (dict(min_side_px=0.0), dict(margin_px=25.0)):
        _, sl = pc.host_visible(pc.edges(), opt)
        assert not any(pc.rests_on_rounding(s) for s in sl[0]), opt


def test_edges_rejects_every_tag_for_the_intended_rule_only():
    case = pc.edges()
    vis, sl = pc.host_visible(case)
    assert [pc.reasons(s) for s in sl[0]] == [list(r) for r in pc.EDGE_REASONS]
    assert vis[0].tolist() == [not r for r in pc.EDGE_REASONS] and vis.sum() == 3
    # tag 7 lands inside the image although it is far outside the field of view: only the monotone test sees it
    assert sl[0][6]["image"].min() > 1.0 and sl[0][6]["monotone"].max() < 0
    # tag 8 is just inside: less than a degree, a pixel of the image and a pixel of side length to spare
    s8 = sl[0][7]
    assert 0 < s8["facing"].min() < np.cos(np.radians(69)) - np.cos(np.radians(70)) + 1e-12
    assert 0 < s8["image"].min() < 1.0 and 0 < s8["side"].min() < 1.0


# ---- the camera centre and the radians -----------------------------------------------------------------------------------

def _rotation_vector(R):
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w * (0.5 if ang < 1e-12 else ang / (2 * np.sin(ang)))


def test_centre_jacobian_and_radians_factor_agree_with_finite_differences(oracle):
    """Central differences through oracle.pose_plus at step 1e-5 (truncation O(h^2)); 1e-6 relative."""
    h = 1e-5
    case = pc.scene()
    worst = 0.0
    for q in list(case["cam_qt"][[0, 7, 23, 39]]) + [np.array([0.3, -0.5, 0.7, 0.2, 1.5, -2.5, 0.8])]:
        J = pc.centre_jacobian(q)
        fd, rot = np.zeros((3, 6)), np.zeros((3, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            plus, minus = oracle.pose_plus(q, d), oracle.pose_plus(q, -d)
            fd[:, k] = (pc.camera_centre(plus) - pc.camera_centre(minus)) / (2 * h)
            R0 = ys.rotation(q)
            rot[:, k] = (_rotation_vector(ys.rotation(plus) @ R0.T) - _rotation_vector(ys.rotation(minus) @ R0.T)) / (2 * h)
        err = np.abs(J - fd).max() / np.abs(J).max()
        want = np.hstack([np.zeros((3, 3)), pc.RADIANS * np.eye(3)])
        err_r = np.abs(rot - want).max() / pc.RADIANS
        worst = max(worst, err, err_r)
        assert err <= 1e-6 and err_r <= 1e-6, (q, err, err_r)
    print("centre Jacobian and radians factor against central differences: worst %.3g" % worst)


# ---- the entry -------------------------------------------------------------------------------------------------------

def test_predict_entry_points_are_declared_under_abi_6_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in ("vmm_ba_default_predict_options", WHO):
        assert name in _lib.EXPORTS and name in declared and hasattr(L, name), name
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.ABI_VERSION == L.vmm_ba_abi_version()
    comment = header[:header.index("enum { VMM_BA_PRED_OK")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("ABI 6, additive")
    for words in ("OCCLUSION IS NOT MODELLED", "ignores the\n *               correlations between tags", "two-fold planar ambiguity",
                  "folds and unfolds again", "errs\n *               towards too small"):
        assert words in comment, words
    for k, name in enumerate(("OK", "NO_VISIBLE_TAG", "TOO_FEW_TAGS", "SINGULAR")):
        assert re.search(r"VMM_BA_PRED_%s = %d\b" % (name, k), header), name
    assert (_lib.PRED_OK, _lib.PRED_NO_VISIBLE_TAG, _lib.PRED_TOO_FEW_TAGS, _lib.PRED_SINGULAR) == (0, 1, 2, 3)
    o = _lib.PredictOptions()
    L.vmm_ba_default_predict_options(C.byref(o))
    assert (o.image_width, o.image_height, o.sigma_px, o.margin_px, o.min_depth, o.max_view_angle_deg, o.min_side_px,
            o.min_tags) == (0, 0, 1.0, 0.0, 1e-3, 70.0, 10.0, 1)
    assert C.sizeof(_lib.PredictResult) == 24


def _call(intr, dist, tag_qt, tag_wh, cam_qt, opt, tag_cov=None, n_tags=None, n_poses=None, res=None, cov=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_predict_localization(
        p(intr), p(dist), (0 if tag_qt is None else len(tag_qt)) if n_tags is None else n_tags, p(tag_qt), p(tag_wh), p(tag_cov),
        (0 if cam_qt is None else len(cam_qt)) if n_poses is None else n_poses, p(cam_qt), None if opt is None else C.byref(opt),
        p(cov), p(cov), None, p(res), 0)


def _good():
    from visual_marker_mapping_amd import engine
    return dict(intr=np.array([1000.0, 1000.0, 500.0, 400.0]), dist=np.zeros(5),
                tag_qt=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 2.0]), (3, 1)), tag_wh=np.full((3, 2), 0.1),
                cam_qt=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (2, 1)),
                opt=engine.default_predict_options(image_width=1000, image_height=800))


def test_predict_refuses_every_bad_argument_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    good = _good()

    def rejected(text, **kw):
        assert _call(**dict(good, **kw)) == _lib.ERR_ARGUMENT, kw
        assert _lib.lib().vmm_ba_last_error().decode() == WHO + ": " + text, (kw, _lib.lib().vmm_ba_last_error())

    rejected("null camera model", intr=None)
    rejected("null camera model", dist=None)
    rejected("null cam_qt", cam_qt=None, n_poses=2)
    rejected("null options", opt=None)
    rejected("negative size", n_tags=-1)
    rejected("negative size", n_poses=-1)
    rejected("null map", tag_qt=None, n_tags=3)
    rejected("null map", tag_wh=None, n_tags=3)
    for v in (np.nan, np.inf):
        rejected("non-finite camera model", intr=np.array([1000.0, v, 500.0, 400.0]))
        rejected("non-finite camera model", dist=np.array([0.0, 0.0, v, 0.0, 0.0]))
        for col in (0, 5):
            bad = good["tag_qt"].copy()
            bad[1, col] = v
            rejected("non-finite map pose", tag_qt=bad)
            bad = good["cam_qt"].copy()
            bad[1, col] = v
            rejected("non-finite camera pose", cam_qt=bad)
        bad = good["tag_wh"].copy()
        bad[2, 1] = v
        rejected("non-finite tag size", tag_wh=bad)
        bad = np.zeros((3, 6, 6))
        bad[2, 3, 4] = v
        rejected("non-finite tag_cov", tag_cov=bad)
    zero = good["tag_qt"].copy()
    zero[2, :4] = 0.0
    rejected("zero map quaternion", tag_qt=zero)
    zero = good["cam_qt"].copy()
    zero[0, :4] = 0.0
    rejected("zero camera quaternion", cam_qt=zero)
    bad_options = [dict(image_width=0), dict(image_width=-5), dict(image_height=0), dict(min_tags=0), dict(min_tags=-1)]
    bad_options += [dict(sigma_px=v) for v in (0.0, -1.0, np.nan, np.inf)]
    for field in ("margin_px", "min_depth", "min_side_px"):
        bad_options += [{field: v} for v in (-1e-9, np.nan, np.inf)]
    bad_options += [dict(max_view_angle_deg=v) for v in (0.0, -10.0, 90.000001, np.nan, np.inf)]
    for kw in bad_options:
        rejected("bad prediction options", opt=engine.default_predict_options(**dict(dict(image_width=1000, image_height=800), **kw)))
    rejected("bad prediction options", opt=engine.default_predict_options())   # the image size has no default
    # the limits themselves are allowed (no device is reached: the batch is empty)
    for kw in (dict(max_view_angle_deg=90.0), dict(margin_px=0.0, min_depth=0.0, min_side_px=0.0)):
        o = engine.default_predict_options(image_width=1, image_height=1, **kw)
        assert _call(**dict(good, opt=o, cam_qt=np.zeros((0, 7)))) == _lib.OK, kw
    # the Python wrapper refuses arrays that do not fit together, and unknown options
    with pytest.raises(ValueError):
        engine.predict_localization(good["intr"], good["dist"], good["tag_qt"], good["tag_wh"][:2], good["cam_qt"], (10, 10))
    with pytest.raises(ValueError):
        engine.predict_localization(good["intr"], good["dist"], good["tag_qt"], good["tag_wh"], good["cam_qt"], (10, 10),
                                    tag_cov=np.zeros((2, 6, 6)))
    with pytest.raises(AttributeError) as ei:
        engine.predict_localization(good["intr"], good["dist"], good["tag_qt"], good["tag_wh"], good["cam_qt"], (10, 10), no_such=1)
    assert str(ei.value) == "unknown prediction option 'no_such'"
    with pytest.raises(_lib.VmmBaError) as ei:
        engine.predict_localization(good["intr"], good["dist"], good["tag_qt"], good["tag_wh"], good["cam_qt"], (0, 10))
    assert ei.value.status == _lib.ERR_ARGUMENT


def test_no_poses_and_no_tags_are_answered_without_a_device():
    from visual_marker_mapping_amd import _lib, engine
    good = _good()
    assert _call(**dict(good, cam_qt=np.zeros((0, 7)))) == _lib.OK
    cov_px, cov_map, res, vis = engine.predict_localization(good["intr"], good["dist"], good["tag_qt"], good["tag_wh"],
                                                            np.zeros((0, 7)), (1000, 800), want_visible=True)
    assert cov_px.shape == cov_map.shape == (0, 6, 6) and res == [] and vis.shape == (0, 3)
    # an empty map: every pose NO_VISIBLE_TAG, filled in on the host
    res = np.zeros(2, np.dtype(_lib.PredictResult))
    res["status"], res["sigma_pos_m"] = 7, 3.0
    cov = np.ones((2, 6, 6))
    assert _call(**dict(good, tag_qt=None, tag_wh=None, res=res, cov=cov)) == _lib.OK
    assert res["status"].tolist() == [_lib.PRED_NO_VISIBLE_TAG] * 2 and not res["n_visible"].any()
    assert not res["sigma_pos_m"].any() and not res["sigma_rot_rad"].any() and not cov.any()
    cov_px, cov_map, res, vis = engine.predict_localization(good["intr"], good["dist"], np.zeros((0, 7)), np.zeros((0, 2)),
                                                            good["cam_qt"], (1000, 800), tag_cov=np.zeros((0, 6, 6)),
                                                            want_visible=True)
    assert [r["status"] for r in res] == [_lib.PRED_NO_VISIBLE_TAG] * 2 and vis.shape == (2, 0)
    assert list(res[0]) == ["status", "n_visible", "sigma_pos_m", "sigma_rot_rad"]
    assert not cov_px.any() and not cov_map.any()


# ---- grid_poses -------------------------------------------------------------------------------------------------------

def test_grid_poses_puts_one_pose_on_every_node_and_axis():
    from visual_marker_mapping_amd import engine
    lo, hi, shape = (-1.0, 0.5, 1.0), (2.0, 0.5, 3.0), (4, 1, 3)
    axes = np.array([[1.0, 0, 0], [0, 2.0, 0], [1.0, 1.0, -0.5]])
    up = (0.0, 0.0, 1.0)
    poses = engine.grid_poses(lo, hi, shape, axes, up)
    assert poses.shape == (4 * 1 * 3 * 3, 7)
    xs, zs = np.linspace(-1.0, 2.0, 4), np.linspace(1.0, 3.0, 3)
    n = 0
    for x in xs:
        for z in zs:
            for a in axes:
                q = poses[n]
                R = ys.rotation(q)
                assert abs(np.linalg.norm(q[:4]) - 1) <= 1e-15
                np.testing.assert_allclose(pc.camera_centre(q), [x, 0.5, z], rtol=0, atol=1e-14)
                np.testing.assert_allclose(R[2], a / np.linalg.norm(a), rtol=0, atol=1e-15)   # the optical axis in the world
                assert abs(R[0] @ up) <= 1e-15 and R[1] @ up < 0                           # no roll: the image's y points down
                n += 1
    for bad in ([0, 0, 1.0], [0, 0, -3.0]):
        with pytest.raises(ValueError) as ei:
            engine.grid_poses(lo, hi, shape, [[1.0, 0, 0], bad], up)
        assert "parallel to up" in str(ei.value)
    with pytest.raises(ValueError):
        engine.grid_poses(lo, hi, (4, 0, 3), axes, up)


# ---- the coverage step ------------------------------------------------------------------------------------------------

def _report():
    from visual_marker_mapping_amd import _lib
    cov = np.arange(36, dtype=np.float64).reshape(6, 6) / 7
    return {4: dict(status=_lib.PRED_OK, n_visible=2, sigma_pos_m=0.0125, sigma_rot_rad=1e-3, pose=np.array([1.0, 0, 0, 0, 0.1, 0.2, 0.3]),
                    covariance=cov, covariance_map=2 * cov, visible_tags=[3, 9]),
            1: dict(status=_lib.PRED_NO_VISIBLE_TAG, n_visible=0, sigma_pos_m=0.0, sigma_rot_rad=0.0,
                    pose=np.array([0.0, 1.0, 0, 0, 1, 2, 3]), covariance=np.zeros((6, 6)), covariance_map=np.zeros((6, 6)), visible_tags=[]),
            2: dict(status=_lib.PRED_TOO_FEW_TAGS, n_visible=1, sigma_pos_m=0.0, sigma_rot_rad=0.0,
                    pose=np.array([0.0, 0, 1.0, 0, 1, 2, 3]), covariance=np.zeros((6, 6)), covariance_map=np.zeros((6, 6)), visible_tags=[9])}


def test_coverage_tree_is_written_in_the_vocabulary_of_the_other_reports(tmp_path):
    from visual_marker_mapping_amd import coverage, io as vio
    options = dict(image_width=640, image_height=480, sigma_px=0.5, min_tags=1)
    tree = coverage.coverage_tree(options, _report(), [9, 3, 5, 7], covariances=True)
    path = str(tmp_path / "coverage.json")
    vio.write_json(path, tree)
    text = open(path).read()
    # every scalar is a quoted string
    assert not re.search(r'[:\[,]\s*-?\d', text) and '"sigma_pos_m": "0.012500000000000001"' in text
    back = vio.read_json(path)
    assert back["options"] == {"image_width": "640", "image_height": "480", "sigma_px": "0.5", "min_tags": "1"}
    assert [p["id"] for p in back["poses"]] == ["1", "2", "4"]
    assert [p["status"] for p in back["poses"]] == ["no_visible_tag", "too_few_tags", "ok"]
    assert [p["num_visible_tags"] for p in back["poses"]] == ["0", "1", "2"]
    last = back["poses"][2]
    assert last["rotation"] == ["1", "0", "0", "0"] and [float(v) for v in last["translation"]] == [0.1, 0.2, 0.3]
    assert set(last["covariance"]) == {"rows", "cols", "coefficents"} and last["covariance"]["rows"] == "6"
    assert vio.matrixFromPropertyTree(last["covariance_map"], 6, 6).tobytes() == _report()[4]["covariance_map"].tobytes()
    assert back["tags"] == [{"id": "3", "num_poses": "1"}, {"id": "5", "num_poses": "0"}, {"id": "7", "num_poses": "0"},
                            {"id": "9", "num_poses": "2"}]
    assert back["tags_never_seen"] == ["5", "7"]
    # without --covariances the matrices stay out
    assert "covariance" not in coverage.coverage_tree(options, _report(), [3, 9])["poses"][0]
    line = coverage.summary_line(_report(), 2)
    assert line == "Predicted 3 poses: 33.3 % ok, sigma_pos_m median 0.0125 worst 0.0125; 2 tags never seen"


def test_coverage_main_wants_exactly_one_source_of_poses(tmp_path, capsys):
    from visual_marker_mapping_amd import coverage
    grid = ["--grid", "0", "1", "2", "0", "1", "2", "0", "1", "2", "--axis", "1", "0", "0", "--up", "0", "0", "1"]
    for argv in (["--poses", "p.json"] + grid, [], ["--grid", "0", "1", "2", "0", "1", "2", "0", "1", "2"]):
        with pytest.raises(SystemExit) as ei:
            coverage.main(["--project_path", str(tmp_path)] + argv)
        assert ei.value.code == 2
    assert "either --poses or --grid" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError) as ei:
        coverage.main(["--project_path", str(tmp_path)] + grid)
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
