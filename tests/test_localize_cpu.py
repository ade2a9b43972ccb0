"""CPU-only checks of the localisation entry points (ABI 6, additive): declared, listed, exported, laid out as the
header says, and validating their arguments before any device call (so all of this passes without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_default_localize_options", "vmm_ba_localize")


def test_localize_entry_points_are_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert hasattr(L, name), name
    assert "ABI 6, additive" in header
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.ABI_VERSION == 6
    assert L.vmm_ba_abi_version() == 6


def test_localize_structs_match_the_header_layout_and_defaults():
    from visual_marker_mapping_amd import _lib
    O, R = _lib.LocalizeOptions, _lib.LocalizeResult
    # int32, int32, 3 x double, int32, int32
    assert C.sizeof(O) == 40
    assert [getattr(O, f).offset for f, _ in O._fields_] == [0, 4, 8, 16, 24, 32, 36]
    # 4 x int32, 2 x double
    assert C.sizeof(R) == 32
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 24]
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    for struct, cls in (("vmm_ba_localize_options", O), ("vmm_ba_localize_result", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    o = O()
    _lib.lib().vmm_ba_default_localize_options(C.byref(o))
    assert (o.refine_iterations, o.robustify, o.huber_a, o.score_cap_px, o.inlier_px, o.reclassify_passes,
            o.min_inlier_tags) == (30, 1, 1.0, 100.0, 8.0, 2, 1)
    assert (_lib.LOC_OK, _lib.LOC_NO_OBSERVATIONS, _lib.LOC_NO_CANDIDATE, _lib.LOC_TOO_FEW_INLIERS,
            _lib.LOC_SINGULAR) == (0, 1, 2, 3, 4)
    for k, name in enumerate(("OK", "NO_OBSERVATIONS", "NO_CANDIDATE", "TOO_FEW_INLIERS", "SINGULAR")):
        assert re.search(r"VMM_BA_LOC_%s = %d\b" % (name, k), header), name


def _call(intr, dist, tag_qt, tag_wh, n_imgs, img_start, obs_tag, obs_px, cam_qt, opt=None, n_tags=None):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_localize(p(intr), p(dist), len(tag_qt) if n_tags is None else n_tags, p(tag_qt), p(tag_wh),
                                      n_imgs, p(img_start), p(obs_tag), p(obs_px), opt, p(cam_qt), None, None, None, 0)


def test_localize_validates_arguments_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    intr, dist = np.array([1000.0, 1000.0, 500.0, 400.0]), np.zeros(5)
    tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1))
    tag_wh = np.full((3, 2), 0.1)
    start = np.array([0, 2, 3], np.int64)
    obs_tag = np.array([0, 1, 2], np.int32)
    obs_px = np.ones((3, 8))
    cam = np.zeros((2, 7))
    good = dict(intr=intr, dist=dist, tag_qt=tag_qt, tag_wh=tag_wh, n_imgs=2, img_start=start, obs_tag=obs_tag,
                obs_px=obs_px, cam_qt=cam)
    # null pointers
    for k in ("intr", "dist", "tag_qt", "tag_wh", "img_start", "obs_tag", "obs_px", "cam_qt"):
        bad = dict(good)
        bad[k] = None
        if k in ("tag_qt", "tag_wh"):
            bad["n_tags"] = 3
        assert _call(**bad) == _lib.ERR_ARGUMENT, k
        assert b"vmm_ba_localize" in _lib.lib().vmm_ba_last_error()
    # img_start not monotone / not starting at zero
    assert _call(**dict(good, img_start=np.array([0, 3, 2], np.int64))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, img_start=np.array([1, 2, 3], np.int64))) == _lib.ERR_ARGUMENT
    # obs_tag outside [0, n_tags)
    assert _call(**dict(good, obs_tag=np.array([0, 1, 3], np.int32))) == _lib.ERR_ARGUMENT
    assert _call(**dict(good, obs_tag=np.array([0, -1, 2], np.int32))) == _lib.ERR_ARGUMENT
    # non-finite map poses
    for v in (np.nan, np.inf):
        for col in (0, 5):
            bad_qt = tag_qt.copy()
            bad_qt[1, col] = v
            assert _call(**dict(good, tag_qt=bad_qt)) == _lib.ERR_ARGUMENT
    # bad options
    o = engine.default_localize_options(inlier_px=-1.0)
    assert _call(**dict(good, opt=C.byref(o))) == _lib.ERR_ARGUMENT
    # n_imgs == 0 is OK (and makes no device call: this machine has no GPU)
    assert _call(**dict(good, n_imgs=0)) == _lib.OK
    cam_qt, cam_cov, inl, res = engine.localize(intr, dist, tag_qt, tag_wh, [0], np.zeros(0, np.int32), np.zeros((0, 8)))
    assert cam_qt.shape == (0, 7) and cam_cov.shape == (0, 6, 6) and inl.shape == (0,) and res == []
    # the Python wrapper refuses arrays that do not fit together, and unknown options
    with pytest.raises(ValueError):
        engine.localize(intr, dist, tag_qt, tag_wh, [0, 2], obs_tag, obs_px)
    with pytest.raises(ValueError):
        engine.localize(intr, dist, tag_qt, tag_wh[:2], start, obs_tag, obs_px)
    with pytest.raises(AttributeError):
        engine.localize(intr, dist, tag_qt, tag_wh, start, obs_tag, obs_px, no_such_option=1)
    with pytest.raises(_lib.VmmBaError) as ei:
        engine.localize(intr, dist, tag_qt, tag_wh, start, np.array([0, 1, 7], np.int32), obs_px)
    assert ei.value.status == _lib.ERR_ARGUMENT


def test_localize_checks_the_map_sizes_and_every_option_and_looks_at_no_option_of_an_empty_batch():
    from visual_marker_mapping_amd import _lib, engine
    intr, dist = np.array([1000.0, 1000.0, 500.0, 400.0]), np.zeros(5)
    tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1))
    tag_wh = np.full((3, 2), 0.1)
    good = dict(intr=intr, dist=dist, tag_qt=tag_qt, tag_wh=tag_wh, n_imgs=2, img_start=np.array([0, 2, 3], np.int64),
                obs_tag=np.array([0, 1, 2], np.int32), obs_px=np.ones((3, 8)), cam_qt=np.zeros((2, 7)))

    def rejected(text, **kw):
        assert _call(**dict(good, **kw)) == _lib.ERR_ARGUMENT, kw
        assert _lib.lib().vmm_ba_last_error().decode() == "vmm_ba_localize: " + text, kw

    zero_q = tag_qt.copy()
    zero_q[2, :4] = 0.0
    rejected("zero map quaternion", tag_qt=zero_q)
    for v in (np.nan, np.inf):
        for col in (0, 1):
            bad_wh = tag_wh.copy()
            bad_wh[1, col] = v
            rejected("non-finite tag size", tag_wh=bad_wh)
    rejected("null map", tag_qt=None, n_tags=3)
    bad_options = [dict(refine_iterations=-1), dict(reclassify_passes=-1), dict(min_inlier_tags=0)]
    for field in ("huber_a", "score_cap_px", "inlier_px"):
        bad_options += [{field: v} for v in (0.0, -1.0, np.nan, np.inf)]
    for kw in bad_options:
        o = engine.default_localize_options(**kw)
        rejected("bad localisation options", opt=C.byref(o))
        # an empty batch is answered before the options are looked at
        assert _call(**dict(good, n_imgs=0, opt=C.byref(o))) == _lib.OK, kw
    # the camera model is checked behind the batch and in front of the map
    nan_intr = np.array([1000.0, np.nan, 500.0, 400.0])
    rejected("img_start decreases", intr=nan_intr, img_start=np.array([0, 3, 2], np.int64))
    rejected("non-finite camera model", intr=nan_intr, tag_qt=zero_q)


def test_localization_main_needs_a_reconstruction(tmp_path):
    from visual_marker_mapping_amd import localization
    with pytest.raises(FileNotFoundError) as ei:
        localization.main(["--project_path", str(tmp_path)])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
