"""CPU-only checks of the calibration entry points (ABI 6, additive): declared, listed, exported, laid out as the header
says, validating their arguments before any device call.  The yardstick of tests/test_gpu_calibrate.py is
tests/yardstick.py, proven in tests/test_yardstick_cpu.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_default_calibrate_options", "vmm_ba_calibrate")


# ---- the entry points -----------------------------------------------------------------------------------------------

def test_calibrate_entry_points_are_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert hasattr(L, name), name
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.ABI_VERSION == 6 and L.vmm_ba_abi_version() == 6


def test_calibrate_structs_match_the_header_layout_and_defaults():
    from visual_marker_mapping_amd import _lib
    O, R = _lib.CalibrateOptions, _lib.CalibrateReport
    # vmm_ba_localize_options (40 bytes), 6 x int32, 2 x double
    assert C.sizeof(O) == 80
    assert [getattr(O, f).offset for f, _ in O._fields_] == [0, 40, 44, 48, 52, 56, 60, 64, 72]
    # 6 x int32, 5 x double
    assert C.sizeof(R) == 64
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56]
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    for struct, cls in (("vmm_ba_calibrate_options", O), ("vmm_ba_calibrate_report", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    o = O()
    _lib.lib().vmm_ba_default_calibrate_options(C.byref(o))
    assert (o.max_trials, o.refine_mask, o.robustify, o.reclassify_passes, o.min_inlier_tags, o.reserved, o.huber_a,
            o.inlier_px) == (100, 0x1FF, 1, 2, 2, 0, 1.0, 8.0)
    lo = _lib.LocalizeOptions()
    _lib.lib().vmm_ba_default_localize_options(C.byref(lo))
    assert bytes(o.loc) == bytes(lo)
    assert (_lib.CAL_OK, _lib.CAL_NO_IMAGES, _lib.CAL_SINGULAR, _lib.CAL_NO_CONVERGENCE) == (0, 1, 2, 3)
    for k, name in enumerate(("OK", "NO_IMAGES", "SINGULAR", "NO_CONVERGENCE")):
        assert re.search(r"VMM_BA_CAL_%s = %d\b" % (name, k), header), name


def _call(intr0, dist0, tag_qt, tag_wh, n_imgs, img_start, obs_tag, obs_px, intr, dist, cam_qt, opt=None, n_tags=None,
          rep=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_calibrate(p(intr0), p(dist0), len(tag_qt) if n_tags is None else n_tags, p(tag_qt), p(tag_wh),
                                       n_imgs, p(img_start), p(obs_tag), p(obs_px), opt, p(intr), p(dist), None, p(cam_qt),
                                       None, None, None, rep, 0)


def test_calibrate_validates_arguments_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    intr0, dist0 = np.array([1000.0, 1000.0, 500.0, 400.0]), np.array([0.01, -0.02, 1e-3, -1e-3, 0.005])
    tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1))
    tag_wh = np.full((3, 2), 0.1)
    start = np.array([0, 2, 3], np.int64)
    obs_tag = np.array([0, 1, 2], np.int32)
    obs_px = np.ones((3, 8))
    good = dict(intr0=intr0, dist0=dist0, tag_qt=tag_qt, tag_wh=tag_wh, n_imgs=2, img_start=start, obs_tag=obs_tag,
                obs_px=obs_px, intr=np.zeros(4), dist=np.zeros(5), cam_qt=np.zeros((2, 7)))
    # null pointers, the result pointers among them
    for k in ("intr0", "dist0", "tag_qt", "tag_wh", "img_start", "obs_tag", "obs_px", "intr", "dist", "cam_qt"):
        bad = dict(good)
        bad[k] = None
        if k in ("tag_qt", "tag_wh"):
            bad["n_tags"] = 3
        assert _call(**bad) == _lib.ERR_ARGUMENT, k
        assert b"vmm_ba_calibrate" in _lib.lib().vmm_ba_last_error()
    # what vmm_ba_localize rejects
    assert _call(**dict(good, img_start=np.array([0, 3, 2], np.int64))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, img_start=np.array([1, 2, 3], np.int64))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, obs_tag=np.array([0, 1, 3], np.int32))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, obs_tag=np.array([0, -1, 2], np.int32))) == _lib.ERR_ARGUMENT
    for v in (np.nan, np.inf):
        for col in (0, 5):
            bad_qt = tag_qt.copy()
            bad_qt[1, col] = v
            assert _call(**dict(good, tag_qt=bad_qt)) == _lib.ERR_ARGUMENT
        assert _call(**dict(good, intr0=np.array([1000.0, v, 500.0, 400.0]))) == _lib.ERR_ARGUMENT
    # the mask, the tolerances and the counts
    for kw in (dict(refine_mask=-1), dict(refine_mask=0x200), dict(inlier_px=-1.0), dict(inlier_px=np.nan),
               dict(huber_a=0.0), dict(huber_a=np.inf), dict(max_trials=-1), dict(reclassify_passes=-1),
               dict(min_inlier_tags=0), dict(loc_inlier_px=-1.0), dict(loc_score_cap_px=0.0), dict(loc_min_inlier_tags=0)):
        o = engine.default_calibrate_options(**kw)
        assert _call(**dict(good, opt=C.byref(o))) == _lib.ERR_ARGUMENT, kw
    # n_imgs == 0 is OK (and makes no device call: this machine has no GPU): the start values come back
    rep = _lib.CalibrateReport()
    out = dict(good, n_imgs=0, rep=C.byref(rep))
    assert _call(**out) == _lib.OK
    assert out["intr"].tobytes() == intr0.tobytes() and out["dist"].tobytes() == dist0.tobytes()
    assert rep.status == _lib.CAL_NO_IMAGES and rep.trials == 0
    intr, dist, icov, cam, ccov, inl, res, report = engine.calibrate(intr0, dist0, tag_qt, tag_wh, [0], np.zeros(0, np.int32),
                                                                     np.zeros((0, 8)))
    assert intr.tobytes() == intr0.tobytes() and dist.tobytes() == dist0.tobytes() and (icov == 0).all()
    assert cam.shape == (0, 7) and ccov.shape == (0, 6, 6) and inl.shape == (0,) and res == []
    assert report["status"] == _lib.CAL_NO_IMAGES
    # images without any observation need no device either
    intr, dist, icov, cam, ccov, inl, res, report = engine.calibrate(intr0, dist0, tag_qt, tag_wh, [0, 0, 0],
                                                                     np.zeros(0, np.int32), np.zeros((0, 8)))
    assert report["status"] == _lib.CAL_NO_IMAGES and intr.tobytes() == intr0.tobytes() and dist.tobytes() == dist0.tobytes()
    assert [r["status"] for r in res] == [_lib.LOC_NO_OBSERVATIONS] * 2 and (ccov == 0).all()
    # the Python wrapper refuses arrays that do not fit together, and unknown options, as engine.localize does
    with pytest.raises(ValueError):
        engine.calibrate(intr0, dist0, tag_qt, tag_wh, [0, 2], obs_tag, obs_px)
    with pytest.raises(ValueError):
        engine.calibrate(intr0, dist0, tag_qt, tag_wh[:2], start, obs_tag, obs_px)
    with pytest.raises(AttributeError):
        engine.calibrate(intr0, dist0, tag_qt, tag_wh, start, obs_tag, obs_px, no_such_option=1)
    with pytest.raises(AttributeError):
        engine.calibrate(intr0, dist0, tag_qt, tag_wh, start, obs_tag, obs_px, loc_no_such_option=1)
    with pytest.raises(_lib.VmmBaError) as ei:
        engine.calibrate(intr0, dist0, tag_qt, tag_wh, start, np.array([0, 1, 7], np.int32), obs_px)
    assert ei.value.status == _lib.ERR_ARGUMENT


def _call_localize(intr, dist, tag_qt, tag_wh, n_imgs, img_start, obs_tag, obs_px, cam_qt, opt=None, n_tags=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_localize(p(intr), p(dist), len(tag_qt) if n_tags is None else n_tags, p(tag_qt), p(tag_wh),
                                      n_imgs, p(img_start), p(obs_tag), p(obs_px), opt, p(cam_qt), None, None, None, 0)


def test_calibrate_and_localize_reject_the_same_batches_maps_and_localisation_options_with_the_same_text():
    """One host stage checks the batch, the map and the localisation options for both entry points: every such fault
    is an argument error of both, with the same text behind the entry point's own name."""
    from visual_marker_mapping_amd import _lib, engine
    intr0, dist0 = np.array([1000.0, 1000.0, 500.0, 400.0]), np.array([0.01, -0.02, 1e-3, -1e-3, 0.005])
    tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1))
    tag_wh = np.full((3, 2), 0.1)
    batch = dict(tag_qt=tag_qt, tag_wh=tag_wh, n_imgs=2, img_start=np.array([0, 2, 3], np.int64),
                 obs_tag=np.array([0, 1, 2], np.int32), obs_px=np.ones((3, 8)), cam_qt=np.zeros((2, 7)))

    def edited(a, row, col, v):
        a = a.copy()
        a[row, col] = v
        return a

    faults = [("img_start decreases", dict(img_start=np.array([0, 3, 2], np.int64))),
              ("img_start[0] != 0", dict(img_start=np.array([1, 2, 3], np.int64))),
              ("obs_tag too large", dict(obs_tag=np.array([0, 1, 3], np.int32))),
              ("obs_tag negative", dict(obs_tag=np.array([0, -1, 2], np.int32))),
              ("null tag_qt", dict(tag_qt=None, n_tags=3)), ("null tag_wh", dict(tag_wh=None, n_tags=3)),
              ("zero quaternion", dict(tag_qt=edited(tag_qt, 2, 0, 0.0)))]
    for v in (np.nan, np.inf, -np.inf):
        faults += [("map quaternion %r" % v, dict(tag_qt=edited(tag_qt, 1, 0, v))),
                   ("map translation %r" % v, dict(tag_qt=edited(tag_qt, 1, 5, v))),
                   ("tag width %r" % v, dict(tag_wh=edited(tag_wh, 0, 0, v))),
                   ("tag height %r" % v, dict(tag_wh=edited(tag_wh, 2, 1, v)))]
    options = [dict(refine_iterations=-1), dict(reclassify_passes=-1), dict(min_inlier_tags=0)]
    for field in ("huber_a", "score_cap_px", "inlier_px"):
        options += [{field: v} for v in (0.0, -1.0, np.nan, np.inf)]
    texts = set()
    for name, kw in faults + [(repr(o), o) for o in options]:
        is_option = name.startswith("{")
        lo = C.byref(engine.default_localize_options(**kw)) if is_option else None
        co = C.byref(engine.default_calibrate_options(**{"loc_" + k: v for k, v in kw.items()})) if is_option else None
        args = batch if is_option else dict(batch, **kw)
        assert _call_localize(intr=intr0, dist=dist0, opt=lo, **args) == _lib.ERR_ARGUMENT, name
        loc_text = _lib.lib().vmm_ba_last_error().decode()
        assert _call(intr0=intr0, dist0=dist0, intr=np.zeros(4), dist=np.zeros(5), opt=co, **args) == _lib.ERR_ARGUMENT, name
        cal_text = _lib.lib().vmm_ba_last_error().decode()
        assert loc_text.startswith("vmm_ba_localize: ") and cal_text.startswith("vmm_ba_calibrate: "), (name, loc_text, cal_text)
        assert loc_text[len("vmm_ba_localize: "):] == cal_text[len("vmm_ba_calibrate: "):] != "", (name, loc_text, cal_text)
        texts.add(cal_text)
    assert len(texts) >= 8   # the faults are told apart
    # each entry point keeps its own order: vmm_ba_calibrate looks at the options before the batch, vmm_ba_localize after
    both = dict(batch, img_start=np.array([0, 3, 2], np.int64))
    co = engine.default_calibrate_options(loc_inlier_px=-1.0)
    assert _call(intr0=intr0, dist0=dist0, intr=np.zeros(4), dist=np.zeros(5), opt=C.byref(co), **both) == _lib.ERR_ARGUMENT
    assert _lib.lib().vmm_ba_last_error().decode() == "vmm_ba_calibrate: bad localisation options"
    lo = engine.default_localize_options(inlier_px=-1.0)
    assert _call_localize(intr=intr0, dist=dist0, opt=C.byref(lo), **both) == _lib.ERR_ARGUMENT
    assert _lib.lib().vmm_ba_last_error().decode() == "vmm_ba_localize: img_start decreases"


def test_write_camera_model_round_trips(tmp_path):
    """The README's camera_intrinsics.json is laid out by hand ("%.16e", " : "); Boost's writer, whose layout the
    writers here produce, cannot emit that text.  What round-trips byte for byte: every value (bit for bit through
    "%.17g"), and the written file through a second read and write."""
    from visual_marker_mapping_amd import io as vio
    src = os.path.join(ROOT, "tests", "golden", "readme_camera_intrinsics.json")
    m = vio.readCameraModel(src)
    first, second = tmp_path / "a.json", tmp_path / "b.json"
    vio.writeCameraModel(m, str(first))
    m2 = vio.readCameraModel(str(first))
    for a, b in ((m, m2),):
        assert np.array([a.fx, a.fy, a.cx, a.cy]).tobytes() == np.array([b.fx, b.fy, b.cx, b.cy]).tobytes()
        assert a.distortionCoefficients.tobytes() == b.distortionCoefficients.tobytes()
        assert (a.verticalResolution, a.horizontalResolution) == (b.verticalResolution, b.horizontalResolution)
    vio.writeCameraModel(m2, str(second))
    assert first.read_bytes() == second.read_bytes()
    assert list(vio.read_json(str(first))) == list(vio.read_json(src))   # the keys, in the file's order


def test_calibration_main_needs_a_reconstruction(tmp_path):
    from visual_marker_mapping_amd import calibration
    with pytest.raises(FileNotFoundError) as ei:
        calibration.main(["--project_path", str(tmp_path)])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
    (tmp_path / "reconstruction.json").write_text("{}")
    with pytest.raises(FileNotFoundError) as ei:
        calibration.main(["--project_path", str(tmp_path)])
    assert "marker_detections.json" in str(ei.value) and "does not exist" in str(ei.value)
