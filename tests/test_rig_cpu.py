"""CPU-only checks of the rig entries (ABI 6, additive): vmm_ba_rig_localize and vmm_ba_rig_calibrate are declared, listed
and exported, laid out as the header says and validate their arguments before any device call; engine.rig_extrinsics_start and synthetic.make_rig_scene do what they
say.  The yardstick of tests/test_gpu_rig.py (tests/rig_cases.py over tests/yardstick.py) is proven in
tests/test_yardstick_cpu.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rig_cases as rc
import yardstick as ys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rig_entry_point_is_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    assert "vmm_ba_rig_localize" in _lib.EXPORTS and "vmm_ba_rig_localize" in declared and hasattr(L, "vmm_ba_rig_localize")
    assert int(re.search(r"#define VMM_BA_RIG_MAX_CAMS (\d+)", header).group(1)) == _lib.RIG_MAX_CAMS == 8
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.ABI_VERSION == 6 and L.vmm_ba_abi_version() == 6
    assert callable(engine.rig_localize) and callable(engine.rig_extrinsics_start)


def _call(intr, dist, ext_qt, tag_qt, tag_wh, n_frames, img_start, obs_tag, obs_px, rig_qt, K=None, opt=None, n_tags=None,
          res=None, cov=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_rig_localize(len(ext_qt) if K is None else K, p(intr), p(dist), p(ext_qt),
                                          len(tag_qt) if n_tags is None else n_tags, p(tag_qt), p(tag_wh), n_frames,
                                          p(img_start), p(obs_tag), p(obs_px), opt, p(rig_qt), p(cov), None, p(res), 0)


def test_rig_localize_validates_arguments_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    K = 2
    intr = np.tile([1000.0, 1000.0, 500.0, 400.0], (K, 1))
    dist = np.tile([0.01, -0.02, 1e-3, -1e-3, 0.005], (K, 1))
    ext = np.array([rc.yaw(0.0), rc.yaw(4.0, (-0.3, 0, 0))])
    tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1))
    tag_wh = np.full((3, 2), 0.1)
    start = np.array([0, 1, 2, 2, 3], np.int64)   # two frames of two cameras
    obs_tag = np.array([0, 1, 2], np.int32)
    obs_px = np.ones((3, 8))
    good = dict(intr=intr, dist=dist, ext_qt=ext, tag_qt=tag_qt, tag_wh=tag_wh, n_frames=2, img_start=start, obs_tag=obs_tag,
                obs_px=obs_px, rig_qt=np.zeros((2, 7)))
    for k in ("intr", "dist", "ext_qt", "tag_qt", "tag_wh", "img_start", "obs_tag", "obs_px", "rig_qt"):
        bad = dict(good)
        bad[k] = None
        if k in ("tag_qt", "tag_wh"):
            bad["n_tags"] = 3
        if k == "ext_qt":
            bad["K"] = K
        assert _call(**bad) == _lib.ERR_ARGUMENT, k
        assert b"vmm_ba_rig_localize" in _lib.lib().vmm_ba_last_error()
    # the number of cameras
    for n in (0, -1, 9):
        assert _call(**dict(good, K=n)) == _lib.ERR_ARGUMENT, n
    assert _call(**dict(good, K=0, n_frames=0)) == _lib.ERR_ARGUMENT
    # what vmm_ba_localize rejects
    assert _call(**dict(good, n_frames=-1)) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, img_start=np.array([0, 1, 3, 2, 3], np.int64))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, img_start=np.array([1, 1, 2, 2, 3], np.int64))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, obs_tag=np.array([0, 1, 3], np.int32))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, obs_tag=np.array([0, -1, 2], np.int32))) == _lib.ERR_ARGUMENT
    for v in (np.nan, np.inf):
        for col in (0, 5):
            bad_qt = tag_qt.copy()
            bad_qt[1, col] = v
            assert _call(**dict(good, tag_qt=bad_qt)) == _lib.ERR_ARGUMENT
            # a non-finite extrinsic, of any camera
            bad_ext = ext.copy()
            bad_ext[1, col] = v
            assert _call(**dict(good, ext_qt=bad_ext)) == _lib.ERR_ARGUMENT
            assert b"extrinsic" in _lib.lib().vmm_ba_last_error()
        # a non-finite camera model, of any camera
        bad_intr, bad_dist = intr.copy(), dist.copy()
        bad_intr[1, 1] = v
        bad_dist[1, 4] = v
        assert _call(**dict(good, intr=bad_intr)) == _lib.ERR_ARGUMENT
        assert b"camera model" in _lib.lib().vmm_ba_last_error()
        assert _call(**dict(good, dist=bad_dist)) == _lib.ERR_ARGUMENT
    zero = ext.copy()
    zero[1, :4] = 0.0
    assert _call(**dict(good, ext_qt=zero)) == _lib.ERR_ARGUMENT
    assert b"zero extrinsic quaternion" in _lib.lib().vmm_ba_last_error()
    zero_tag = tag_qt.copy()
    zero_tag[2, :4] = 0.0
    assert _call(**dict(good, tag_qt=zero_tag)) == _lib.ERR_ARGUMENT
    for kw in (dict(inlier_px=-1.0), dict(inlier_px=np.nan), dict(huber_a=0.0), dict(score_cap_px=0.0),
               dict(refine_iterations=-1), dict(reclassify_passes=-1), dict(min_inlier_tags=0)):
        o = engine.default_localize_options(**kw)
        assert _call(**dict(good, opt=C.byref(o))) == _lib.ERR_ARGUMENT, kw
    # n_frames == 0 is OK and makes no device call (this machine has no GPU); so are frames without any observation
    assert _call(**dict(good, n_frames=0)) == _lib.OK
    rig, cov, inl, res = engine.rig_localize(intr, dist, ext, tag_qt, tag_wh, [0], np.zeros(0, np.int32), np.zeros((0, 8)))
    assert rig.shape == (0, 7) and cov.shape == (0, 6, 6) and inl.shape == (0,) and res == []
    rig, cov, inl, res = engine.rig_localize(intr, dist, ext, tag_qt, tag_wh, [0] * 5, np.zeros(0, np.int32), np.zeros((0, 8)))
    assert [r["status"] for r in res] == [_lib.LOC_NO_OBSERVATIONS] * 2
    assert (rig == [1, 0, 0, 0, 0, 0, 0]).all() and (cov == 0).all()
    # the Python wrapper refuses arrays that do not fit together, and unknown options
    with pytest.raises(ValueError):
        engine.rig_localize(intr, dist, ext, tag_qt, tag_wh, [0, 1, 2, 3], obs_tag, obs_px)   # 3 slots, 2 cameras
    with pytest.raises(ValueError):
        engine.rig_localize(intr, dist[:1], ext, tag_qt, tag_wh, start, obs_tag, obs_px)
    with pytest.raises(AttributeError):
        engine.rig_localize(intr, dist, ext, tag_qt, tag_wh, start, obs_tag, obs_px, no_such_option=1)
    with pytest.raises(_lib.VmmBaError) as ei:
        engine.rig_localize(intr, dist, ext, tag_qt, tag_wh, start, np.array([0, 1, 7], np.int32), obs_px)
    assert ei.value.status == _lib.ERR_ARGUMENT


# ---- rig_extrinsics_start -------------------------------------------------------------------------------------------

def test_rig_extrinsics_start_returns_the_exact_extrinsic_and_names_a_camera_without_a_shared_frame():
    from visual_marker_mapping_amd import _lib, engine
    s = rc.rig_scene("config1_20x10", noise_px=0.0)
    K, F = s.n_rig_cams, s.n_frames
    cam = np.array([rc.compose(s.ext_qt[c], s.rig_gt[f]) for f in range(F) for c in range(K)])
    ok = dict(status=_lib.LOC_OK, n_obs=5, n_inlier_obs=5, trials=3, rms_px=0.0, cost=0.0)
    res = [dict(ok) for _ in range(F * K)]
    ext = engine.rig_extrinsics_start(K, F, cam, res)
    gq, gt = ys.pose_gap(ext, s.ext_qt)
    assert ext.shape == (K, 7) and gq <= 1e-12 and gt <= 1e-12, (gq, gt)
    assert (ext[0] == [1, 0, 0, 0, 0, 0, 0]).all()
    # the frame with the most inliers over the two images is the one used; ties go to the lowest frame
    spoiled = cam.copy()
    spoiled[:, 4:] += 1.0          # every image's pose is wrong ...
    spoiled[7 * K] = cam[7 * K]    # ... but those of frame 7, cameras 0 and 2
    spoiled[7 * K + 2] = cam[7 * K + 2]
    res[7 * K + 2]["n_inlier_obs"] = 9
    ext = engine.rig_extrinsics_start(K, F, spoiled, res)
    assert max(ys.pose_gap(ext[2], s.ext_qt[2])) <= 1e-12 and max(ys.pose_gap(ext[1], s.ext_qt[1])) > 1e-3
    res[11 * K + 2]["n_inlier_obs"] = 9   # a tie with a later frame changes nothing
    assert engine.rig_extrinsics_start(K, F, spoiled, res).tobytes() == ext.tobytes()
    # camera 1 never shares a localised frame with camera 0
    for f in range(F):
        res[f * K + (1 if f % 2 else 0)]["status"] = _lib.LOC_NO_CANDIDATE
    with pytest.raises(ValueError, match="camera 1"):
        engine.rig_extrinsics_start(K, F, cam, res)


# ---- make_rig_scene --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(rc.SCENES))
def test_make_rig_scene_keeps_the_visibility_floor_and_is_deterministic(name):
    s = rc.rig_scene(name, outlier_frac=0.1, seed=11)   # asserts the floor of 5 tags in every image
    again = rc.rig_scene(name, outlier_frac=0.1, seed=11)
    other = rc.rig_scene(name, outlier_frac=0.1, seed=12)
    exact = rc.rig_scene(name, noise_px=0.0)
    K, F, n = s.n_rig_cams, s.n_frames, len(s.obs_tag)
    assert K == 3 and len(s.img_start) == F * K + 1 and s.img_start[0] == 0 and s.img_start[-1] == n
    for key in ("img_start", "obs_tag", "obs_px", "obs_frame", "obs_cam", "outlier"):
        assert getattr(s, key).tobytes() == getattr(again, key).tobytes(), key
    assert s.obs_px.tobytes() != other.obs_px.tobytes() and s.obs_tag.tobytes() == other.obs_tag.tobytes()
    # slot f * K + c holds the observations of (f, c)
    slot = np.repeat(np.arange(F * K), np.diff(s.img_start))
    assert (slot == s.obs_frame * K + s.obs_cam).all()
    # exact data project onto the pixels under the composed pose (the oracle-free check: residual-free by construction)
    assert not exact.outlier.any() and exact.obs_tag.tobytes() == s.obs_tag.tobytes()
    # the planted outliers: 10 % of the observations, each moved as a whole by 50 .. 200 px, the others by noise alone
    assert int(s.outlier.sum()) == int(round(0.1 * n))
    moved = (s.obs_px - exact.obs_px).reshape(n, 4, 2)
    shift = np.linalg.norm(moved.mean(axis=1), axis=1)
    assert (shift[s.outlier] >= 50 - 6 * s.noise_px).all() and (shift[s.outlier] <= 200 + 6 * s.noise_px).all()
    assert s.noise_px > 0 and (np.abs(moved[~s.outlier]) <= 6 * s.noise_px).all()
    spread = np.abs(moved - moved.mean(axis=1, keepdims=True))
    assert (spread[s.outlier] <= 6 * s.noise_px).all()


def test_make_rig_scene_leaves_missing_images_empty_and_projects_with_each_cameras_model(oracle):
    intr = np.array([[8075.0, 8083.0, 3016.0, 1996.0], [7900.0, 7950.0, 2950.0, 2050.0], [8150.0, 8100.0, 3060.0, 1960.0]])
    dist = np.array([[-0.186, 0.370, -2.9e-4, 4.2e-4, 0.057], [-0.10, 0.15, 3e-4, -2e-4, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    missing = [(f, 2) for f in range(0, 12, 2)]
    s = rc.rig_scene("distortion_12x8", intr=intr, dist=dist, noise_px=0.0, missing=missing)
    per_image = np.diff(s.img_start).reshape(s.n_frames, 3)
    assert (per_image[0::2, 2] == 0).all() and (per_image[1::2, 2] >= rc.FLOOR).all() and (per_image[:, :2] >= rc.FLOOR).all()
    cost, r, _ = rc.rig_system(oracle, s, s.rig_gt, s.ext_qt)
    print("exact data under three camera models: largest residual %.3g px" % np.abs(r).max())
    assert np.abs(r).max() <= 1e-9


# ---- vmm_ba_rig_calibrate --------------------------------------------------------------------------------------------

def test_rig_calibrate_entry_points_and_structs_match_the_header():
    from visual_marker_mapping_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in ("vmm_ba_default_rig_calibrate_options", "vmm_ba_rig_calibrate"):
        assert name in _lib.EXPORTS and name in declared and hasattr(L, name), name
    O, R = _lib.RigCalibrateOptions, _lib.RigCalibrateReport
    # vmm_ba_localize_options (40 bytes), 6 x int32, 2 x double
    assert C.sizeof(O) == 80 and [getattr(O, f).offset for f, _ in O._fields_] == [0, 40, 44, 48, 52, 56, 60, 64, 72]
    # 8 x int32, 5 x double
    assert C.sizeof(R) == 72 and [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64]
    for struct, cls in (("vmm_ba_rig_calibrate_options", O), ("vmm_ba_rig_calibrate_report", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    o = engine.default_rig_calibrate_options()
    assert (o.max_trials, o.refine_mask, o.robustify, o.reclassify_passes, o.min_inlier_tags, o.reserved, o.huber_a,
            o.inlier_px) == (100, 0xFE, 1, 2, 2, 0, 1.0, 8.0)   # every camera but 0
    lo = _lib.LocalizeOptions()
    L.vmm_ba_default_localize_options(C.byref(lo))
    assert bytes(o.loc) == bytes(lo)
    with pytest.raises(AttributeError):
        engine.default_rig_calibrate_options(no_such_option=1)
    assert engine.default_rig_calibrate_options(loc_inlier_px=50.0).loc.inlier_px == 50.0


def _call_cal(intr, dist, ext_qt0, tag_qt, tag_wh, n_frames, img_start, obs_tag, obs_px, ext_qt, rig_qt, K=None, opt=None,
              n_tags=None, rep=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_rig_calibrate(len(ext_qt0) if K is None else K, p(intr), p(dist), p(ext_qt0),
                                           len(tag_qt) if n_tags is None else n_tags, p(tag_qt), p(tag_wh), n_frames,
                                           p(img_start), p(obs_tag), p(obs_px), opt, p(ext_qt), None, p(rig_qt), None, None,
                                           None, rep, 0)


def test_rig_calibrate_validates_arguments_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    K = 3
    intr = np.tile([1000.0, 1000.0, 500.0, 400.0], (K, 1))
    dist = np.tile([0.01, -0.02, 1e-3, -1e-3, 0.005], (K, 1))
    tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1))
    tag_wh = np.full((3, 2), 0.1)
    start = np.array([0, 1, 2, 2, 3, 3, 3], np.int64)   # two frames of three cameras
    obs_tag = np.array([0, 1, 2], np.int32)
    good = dict(intr=intr, dist=dist, ext_qt0=rc.EXT3.copy(), tag_qt=tag_qt, tag_wh=tag_wh, n_frames=2, img_start=start,
                obs_tag=obs_tag, obs_px=np.ones((3, 8)), ext_qt=np.zeros((K, 7)), rig_qt=np.zeros((2, 7)))
    for k in ("intr", "dist", "ext_qt0", "tag_qt", "tag_wh", "img_start", "obs_tag", "obs_px", "ext_qt", "rig_qt"):
        bad = dict(good)
        bad[k] = None
        if k in ("tag_qt", "tag_wh"):
            bad["n_tags"] = 3
        if k == "ext_qt0":
            bad["K"] = K
        assert _call_cal(**bad) == _lib.ERR_ARGUMENT, k
        assert b"vmm_ba_rig_calibrate" in _lib.lib().vmm_ba_last_error()
    for n in (0, 9):
        assert _call_cal(**dict(good, K=n)) == _lib.ERR_ARGUMENT
    # the gauge: all K bits, or a bit at or above K
    for mask in (0b111, 0b1000, 0b1110, -1):
        o = engine.default_rig_calibrate_options(refine_mask=mask)
        assert _call_cal(**dict(good, opt=C.byref(o))) == _lib.ERR_ARGUMENT, mask
        assert b"refine_mask" in _lib.lib().vmm_ba_last_error()
        assert _call_cal(**dict(good, n_frames=0, opt=C.byref(o))) == _lib.ERR_ARGUMENT, mask
    for kw in (dict(inlier_px=-1.0), dict(inlier_px=np.nan), dict(huber_a=0.0), dict(huber_a=np.inf), dict(max_trials=-1),
               dict(reclassify_passes=-1), dict(min_inlier_tags=0), dict(loc_inlier_px=-1.0), dict(loc_score_cap_px=0.0)):
        o = engine.default_rig_calibrate_options(**kw)
        assert _call_cal(**dict(good, opt=C.byref(o))) == _lib.ERR_ARGUMENT, kw
    # what vmm_ba_rig_localize rejects
    assert _call_cal(**dict(good, img_start=np.array([0, 1, 3, 2, 3, 3, 3], np.int64))) == _lib.ERR_ARGUMENT
    assert _call_cal(**dict(good, obs_tag=np.array([0, 1, 3], np.int32))) == _lib.ERR_ARGUMENT
    bad_ext = rc.EXT3.copy()
    bad_ext[2, :4] = 0.0
    assert _call_cal(**dict(good, ext_qt0=bad_ext)) == _lib.ERR_ARGUMENT
    bad_intr = intr.copy()
    bad_intr[2, 0] = np.inf
    assert _call_cal(**dict(good, intr=bad_intr)) == _lib.ERR_ARGUMENT
    # n_frames == 0, and frames without any observation, need no device: the start values come back
    rep = _lib.RigCalibrateReport()
    out = dict(good, n_frames=0, rep=C.byref(rep))
    assert _call_cal(**out) == _lib.OK and out["ext_qt"].tobytes() == rc.EXT3.tobytes()
    assert rep.status == _lib.CAL_NO_IMAGES and rep.trials == 0 and rep.cams_refined == 0
    ext, ext_cov, rig, rig_cov, inl, res, report = engine.rig_calibrate(intr, dist, rc.EXT3, tag_qt, tag_wh, [0] * 7,
                                                                        np.zeros(0, np.int32), np.zeros((0, 8)))
    assert report["status"] == _lib.CAL_NO_IMAGES and ext.tobytes() == rc.EXT3.tobytes() and (ext_cov == 0).all()
    assert ext_cov.shape == (18, 18) and [r["status"] for r in res] == [_lib.LOC_NO_OBSERVATIONS] * 2 and (rig_cov == 0).all()
    with pytest.raises(ValueError):
        engine.rig_calibrate(intr, dist, rc.EXT3, tag_qt, tag_wh, [0, 1, 2, 3, 3], obs_tag, np.ones((3, 8)))
