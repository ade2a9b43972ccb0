"""CPU-only checks of the prediction with correlated map tags (vmm_ba_predict_localization_joint, ABI 6, additive): the
host yardstick itself (tests/predict_joint_cases.py) on the two inputs whose answer is known beforehand, the flags of the
cases the GPU test uses, the uncertainty file with the joint matrix, and every argument error that needs no device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import cov_cases as cc
import eval_cases as ec
import finished_map_cases as fm
import predict_cases as pc
import predict_joint_cases as pj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "vmm_ba_predict_localization_joint"
LD = cc.LD
# Two longdouble expressions of the same quantity: far above what the chain's few hundred roundings of 2^-64 add up to,
# far below the order-one error of a wrong matrix
SAME_IN_LONGDOUBLE = 1e-15


# ---- 1. block diagonal ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tags", [2, 65])
def test_block_diagonal_joint_covariance_gives_the_independent_formula(oracle, n_tags):
    diag = pc.random_tag_cov(n_tags, fixed=[], seed=20261204)
    case = pj.JointCase(n_tags, pj.JOINT_POSES, pj.block_diagonal(diag))
    vis, _ = case.host_visible()
    ev = case.evaluate(oracle, vis)
    assert len(ev.items) >= 2
    worst = 0.0
    for p in ev.items:
        want = pc.host_pose(oracle, case.case, p, vis[p], tag_cov=diag, opt=dict(sigma_px=case.sigma_px))
        dev = cc.entry_deviation(want[1], ev.truth[p]["prop"])
        worst = max(worst, dev)
        assert dev <= ev.bound["prop"], (p, dev, ev.bound["prop"])
        assert cc.entry_deviation(want[0], ev.truth[p]["cov"]) <= ev.bound["cov"], p
        # and in longdouble the two formulas are one
        assert cc.entry_deviation(pj.independent_prop(case, p, vis[p], diag), ev.truth[p]["prop"]) <= SAME_IN_LONGDOUBLE, p
    print("block diagonal, %d tags: host_pose's cov_map deviates %.3e from the joint truth, bound %.3e" % (n_tags, worst, ev.bound["prop"]))


# ---- 2. the rigid common mode ---------------------------------------------------------------------------------------------

def test_a_rigidly_moved_map_moves_the_camera_with_it(oracle):
    """S_st = A_s Sw A_t^T for all pairs: cov_map = B Sw B^T for every pose and every selected set that leaves H positive
    definite.  First the identity behind it per corner, Jc B + Jt A_t = 0, on the longdouble Jacobians."""
    n_tags = 65
    Sw = pj.world_covariance()
    case = pj.JointCase(n_tags, pj.JOINT_POSES, pj.rigid(pc.lanes(n_tags, 1, relief=fm.PREDICT_RELIEF)["tag_qt"], Sw))
    c = case.case
    vis, _ = case.host_visible()
    ev = case.evaluate(oracle, vis)
    assert len(ev.items) >= 5
    worst_id = worst = 0.0
    differs = 0
    for p in ev.items:
        t, Jc, Jt = case._jacobians(p, vis[p], LD)
        B = pj.rigid_camera(c["cam_qt"][p], LD)
        A = np.array([pj.rigid_tag(c["tag_qt"][k], LD) for k in t])
        left, right = Jc @ B, np.einsum("mkrp,mpq->mkrq", Jt, A)
        scale = np.abs(left).max(axis=(1, 2, 3), keepdims=True)
        worst_id = max(worst_id, float((np.abs(left + right) / scale).max()))
        want = B @ Sw.astype(LD) @ B.T
        dev = cc.entry_deviation(ev.truth[p]["prop"], want)
        worst = max(worst, dev)
        assert dev <= ev.bound["prop"], (p, dev, ev.bound["prop"])
        # a subset of the visible tags gives the same matrix
        some = vis[p].copy()
        some[np.flatnonzero(some)[::2]] = False
        if some.sum() >= 2:
            assert cc.entry_deviation(case.truth(p, some)["prop"], want) <= ev.bound["prop"], p
        # the independent formula, from the same marginals, gives something else: the defect the joint entry removes
        diag = case.joint[np.arange(n_tags), np.arange(n_tags)]
        if vis[p].sum() >= 2:
            off = cc.entry_deviation(pj.independent_prop(case, p, vis[p], diag), want)
            assert off > 1e3 * ev.bound["prop"] and off > 1e-3, (p, off)
            differs += 1
    assert worst_id <= SAME_IN_LONGDOUBLE, worst_id
    assert differs >= 5
    print("rigid common mode: per-corner identity %.3e, truth against B Sw B^T %.3e (bound %.3e)" % (worst_id, worst, ev.bound["prop"]))


# ---- 3. the flags of the GPU cases --------------------------------------------------------------------------------------------

def test_no_flag_of_the_gpu_cases_rests_on_rounding():
    for n_tags in pj.JOINT_TAGS:
        case = pc.lanes(n_tags, pj.JOINT_POSES, relief=fm.PREDICT_RELIEF)
        vis, sl = pc.host_visible(case)
        near = [(p, t) for p, row in enumerate(sl) for t, s in enumerate(row) if pc.rests_on_rounding(s)]
        print("lanes %d x %d: visible per pose %s" % (n_tags, pj.JOINT_POSES, vis.sum(axis=1).tolist()))
        assert not near, (n_tags, near)
    # at 129 tags more than one round holds visible tags for some pose, and some pose sees tags of all three
    vis, _ = pc.host_visible(pc.lanes(129, pj.JOINT_POSES, relief=fm.PREDICT_RELIEF))
    rounds = [sorted({int(t) // 64 for t in np.flatnonzero(v)}) for v in vis]
    assert any(len(r) >= 2 for r in rounds), rounds


# ---- 4. the file ----------------------------------------------------------------------------------------------------------------

def test_uncertainty_file_carries_the_joint_matrix_bit_for_bit(tmp_path):
    from visual_marker_mapping_amd import io as vio, uncertainty
    ids = [3, 7, 12]
    joint = pj.dense_spd(3, seed=5)
    tags = {t: joint[k, k] for k, t in enumerate(ids)}
    cams = {0: np.eye(6) * 1e-6}
    path = str(tmp_path / "u.json")
    uncertainty.write_uncertainty(path, 3, False, tags, cams, (ids, joint))
    back = uncertainty.read_tag_joint_covariance(path)
    assert back[0] == ids and back[1].shape == (3, 3, 6, 6) and back[1].tobytes() == joint.tobytes()
    tree = vio.read_json(path)
    assert tree["tag_joint_covariance"]["covariance"]["rows"] == tree["tag_joint_covariance"]["covariance"]["cols"] == "18"
    assert pj.dense_matrix(back[1]).tobytes() == vio.matrixFromPropertyTree(tree["tag_joint_covariance"]["covariance"], 18, 18).tobytes()
    # without the matrix: the tree of before, key by key, and the reader says None
    plain = uncertainty.uncertainty_tree(3, False, tags, cams)
    with_joint = uncertainty.uncertainty_tree(3, False, tags, cams, (ids, joint))
    assert list(plain) == ["origin_tag_id", "robustify", "reconstructed_tags", "reconstructed_cameras"]
    assert {k: with_joint[k] for k in plain} == plain and list(with_joint)[-1] == "tag_joint_covariance"
    uncertainty.write_uncertainty(path, 3, False, tags, cams)
    assert uncertainty.read_tag_joint_covariance(path) is None
    # the golden tree of the uncertainty file is that of a tree without the matrix
    golden = os.path.join(ROOT, "tests", "golden", "trees", "reconstruction_uncertainty.json")
    assert "tag_joint_covariance" not in json.load(open(golden))
    with pytest.raises(ValueError):
        uncertainty.uncertainty_tree(3, False, tags, cams, (ids[:2], joint))


# ---- 5. arguments ---------------------------------------------------------------------------------------------------------------

def _good():
    from visual_marker_mapping_amd import engine
    return dict(intr=np.array([1000.0, 1000.0, 500.0, 400.0]), dist=np.zeros(5),
                tag_qt=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 2.0]), (3, 1)), tag_wh=np.full((3, 2), 0.1),
                cam_qt=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (2, 1)), joint=np.zeros((3, 3, 6, 6)),
                opt=engine.default_predict_options(image_width=1000, image_height=800))


def _call(intr, dist, tag_qt, tag_wh, cam_qt, opt, joint, n_tags=None, n_poses=None, visible_in=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_predict_localization_joint(
        p(intr), p(dist), (0 if tag_qt is None else len(tag_qt)) if n_tags is None else n_tags, p(tag_qt), p(tag_wh), p(joint),
        (0 if cam_qt is None else len(cam_qt)) if n_poses is None else n_poses, p(cam_qt), p(visible_in),
        None if opt is None else C.byref(opt), None, None, None, None, 0)


def test_joint_entry_is_declared_under_abi_6_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    assert WHO in _lib.EXPORTS and WHO in _lib.OPTIONAL and hasattr(_lib.lib(), WHO)
    comment = header[:header.index("int " + WHO)].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("ABI 6, additive")
    for words in ("OCCLUSION IS STILL NOT MODELLED", "unit weights, no loss", "Only the blocks with s >= t are\n *               read",
                  "NaN included", "byte count"):
        assert words in comment, words
    assert len(_lib.SIGNATURES[WHO][1]) == len(_lib.SIGNATURES["vmm_ba_predict_localization"][1]) + 1


def test_joint_entry_refuses_every_bad_argument_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    good = _good()

    def rejected(text, **kw):
        assert _call(**dict(good, **kw)) == _lib.ERR_ARGUMENT, kw
        assert _lib.lib().vmm_ba_last_error().decode() == WHO + ": " + text, (kw, _lib.lib().vmm_ba_last_error())

    rejected("null tag_cov_joint", joint=None)
    for v in (np.nan, np.inf):
        for s, t in ((0, 0), (2, 0), (2, 2), (1, 0)):
            bad = good["joint"].copy()
            bad[s, t, 3, 4] = v
            rejected("non-finite tag_cov_joint", joint=bad)
    # the old entry's errors, under the new name
    rejected("null camera model", intr=None)
    rejected("null cam_qt", cam_qt=None, n_poses=2)
    rejected("null options", opt=None)
    rejected("negative size", n_tags=-1)
    rejected("null map", tag_qt=None, n_tags=3)
    rejected("non-finite camera model", dist=np.array([0.0, np.nan, 0.0, 0.0, 0.0]))
    zero = good["cam_qt"].copy()
    zero[0, :4] = 0.0
    rejected("zero camera quaternion", cam_qt=zero)
    rejected("bad prediction options", opt=engine.default_predict_options(image_width=1000, image_height=800, min_tags=0))
    # the upper block triangle is not looked at; no poses and no tags are answered without a device
    upper = good["joint"].copy()
    upper[0, 1], upper[0, 2], upper[1, 2] = np.nan, np.inf, -np.inf
    assert _call(**dict(good, joint=upper, cam_qt=np.zeros((0, 7)))) == _lib.OK
    assert _call(**dict(good, tag_qt=None, tag_wh=None, joint=None)) == _lib.OK
    cov_px, cov_map, res, vis = engine.predict_localization(good["intr"], good["dist"], np.zeros((0, 7)), np.zeros((0, 2)),
                                                            good["cam_qt"], (1000, 800), tag_cov_joint=np.zeros((0, 0, 6, 6)),
                                                            visible_in=np.zeros((2, 0)), want_visible=True)
    assert [r["status"] for r in res] == [_lib.PRED_NO_VISIBLE_TAG] * 2 and vis.shape == (2, 0) and not cov_px.any() and not cov_map.any()


def test_python_wrapper_refuses_what_does_not_fit():
    from visual_marker_mapping_amd import engine
    g = _good()
    args = (g["intr"], g["dist"], g["tag_qt"], g["tag_wh"], g["cam_qt"], (1000, 800))
    with pytest.raises(ValueError) as ei:
        engine.predict_localization(*args, tag_cov=np.zeros((3, 6, 6)), tag_cov_joint=g["joint"])
    assert "both" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        engine.predict_localization(*args, visible_in=np.ones((2, 3)))
    assert str(ei.value) == "visible_in needs tag_cov_joint"
    with pytest.raises(ValueError):
        engine.predict_localization(*args, tag_cov=np.zeros((3, 6, 6)), visible_in=np.ones((2, 3)))
    with pytest.raises(ValueError):
        engine.predict_localization(*args, tag_cov_joint=np.zeros((2, 2, 6, 6)))
    with pytest.raises(ValueError):
        engine.predict_localization(*args, tag_cov_joint=g["joint"], visible_in=np.ones((2, 2)))
    with pytest.raises(ValueError):
        engine.localization_map_covariance(*args[:5], [0, 1], [0], [True], g["joint"], (1000, 800))   # img_start too short
    with pytest.raises(ValueError):
        engine.localization_map_covariance(*args[:5], [0, 1, 1], [3], [True], g["joint"], (1000, 800))   # a tag outside the map


def test_reconstructor_refuses_a_joint_covariance_that_does_not_cover_the_map():
    from visual_marker_mapping_amd.tag_reconstructor import DetectionResult, ReconstructedTag, TagReconstructor
    rec = TagReconstructor(DetectionResult())
    rec.setReconstructedTags({t: ReconstructedTag(t, 0, np.array([1.0, 0, 0, 0]), np.zeros(3), 0.1, 0.1) for t in (2, 5, 9)})
    joint = pj.dense_spd(3, seed=6)
    got = rec._joint_for_map([9, 2, 5], joint)
    assert got.tobytes() == np.ascontiguousarray(joint[np.ix_([1, 2, 0], [1, 2, 0])]).tobytes()
    with pytest.raises(RuntimeError) as ei:
        rec._joint_for_map([2, 9], joint[:2, :2])
    assert str(ei.value) == "The joint covariance does not cover the map: no entry for tag 5."
    with pytest.raises(ValueError):
        rec._joint_for_map([2, 5, 9], joint[:2, :2])
    with pytest.raises(ValueError):
        rec.predictLocalizationAccuracy(np.zeros((0, 7)), tagCovariances={}, tagJointCovariance=([2, 5, 9], joint))
