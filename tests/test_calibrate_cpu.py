"""CPU-only checks of the calibration entry points (ABI 6, additive): declared, listed, exported, laid out as the header
says, validating their arguments before any device call -- and the yardstick of tests/test_gpu_calibrate.py, proven here
before the GPU tests lean on it.

The yardstick (calib_system, host_calibration) is numpy around oracle/oracle.py: obs_eval gives the 8 residuals and the
8 x 6 camera Jacobian of one observation, huber gives rho; the nine intrinsic columns are the closed forms of the cost
functor's projection, compared below with central differences of obs_eval.  It never calls the code under test.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_default_calibrate_options", "vmm_ba_calibrate")
ALL_FREE = 0x1FF


# ---- the yardstick --------------------------------------------------------------------------------------------------

def _rot(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def intrinsic_columns(k, cam_qt, tag_qt, wh):
    """The 8 x 9 Jacobian of one observation's residuals over k = (fx, fy, cx, cy, k1, k2, p1, p2, k3) for the cost
    functor's projection: xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2),
    u = fx xd + cx, v = fy yd + cy.  Corners LL, LR, UR, UL."""
    fx, fy = k[0], k[1]
    Rc, Rt = _rot(cam_qt[:4]), _rot(tag_qt[:4])
    J = np.zeros((8, 9))
    for c, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
        pw = Rt @ np.array([sx * wh[0] / 2, sy * wh[1] / 2, 0.0]) + tag_qt[4:]
        pc = Rc @ pw + cam_qt[4:]
        x, y = pc[0] / pc[2], pc[1] / pc[2]
        r2 = x * x + y * y
        rad = 1 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]))
        xd = x * rad + 2 * k[6] * x * y + k[7] * (r2 + 2 * x * x)
        yd = y * rad + 2 * k[7] * x * y + k[6] * (r2 + 2 * y * y)
        J[2 * c] = [xd, 0, 1, 0, fx * x * r2, fx * x * r2 ** 2, fx * 2 * x * y, fx * (r2 + 2 * x * x), fx * x * r2 ** 3]
        J[2 * c + 1] = [0, yd, 0, 1, fy * y * r2, fy * y * r2 ** 2, fy * (r2 + 2 * y * y), fy * 2 * x * y, fy * y * r2 ** 3]
    return J


def calib_system(O, k, cams, tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE):
    """The calibration problem at (k, cams): cost = 1/2 sum rho(|r_corner|^2), the residuals (8 per observation) and the
    dense Jacobian over (6 per image in `cams` order, then the nine of k), both with the loss applied as Ceres' corrector
    does for rho'' <= 0 (rows and residuals scaled by sqrt(rho')).  obs_img indexes cams.  A parameter outside `mask`
    has zero columns."""
    n, n_img = len(obs_tag), len(cams)
    r_all, J = np.zeros(8 * n), np.zeros((8 * n, 6 * n_img + 9))
    free = np.array([(mask >> j) & 1 for j in range(9)], np.float64)
    cost = 0.0
    for o in range(n):
        i, t = int(obs_img[o]), int(obs_tag[o])
        r, Jc, _ = O.obs_eval(k[:4], k[4:], cams[i], tag_qt[t], tag_wh[t], obs_px[o])
        Jk = intrinsic_columns(k, cams[i], tag_qt[t], tag_wh[t]) * free
        for c in range(4):
            rows = slice(2 * c, 2 * c + 2)
            sq = float(r[rows] @ r[rows])
            rho = O.huber(a, sq) if robust else (sq, 1.0, 0.0)
            w = np.sqrt(rho[1])
            cost += 0.5 * rho[0]
            r_all[8 * o + 2 * c:8 * o + 2 * c + 2] = w * r[rows]
            J[8 * o + 2 * c:8 * o + 2 * c + 2, 6 * i:6 * i + 6] = w * Jc[rows]
            J[8 * o + 2 * c:8 * o + 2 * c + 2, 6 * n_img:] = w * Jk[rows]
    return cost, r_all, J


def _damped_step(H, g, lam, mask):
    """(H + lam diag(H)) step = -g with unit rows for the parameters outside the mask."""
    H, g = H.copy(), g.copy()
    d = np.maximum(np.diag(H), 1e-12)
    H[np.diag_indices_from(H)] += lam * d
    n = len(g) - 9
    for j in range(9):
        if not (mask >> j) & 1:
            H[n + j, :] = H[:, n + j] = 0.0
            H[n + j, n + j] = 1.0
            g[n + j] = 0.0
    s = 1.0 / np.sqrt(np.diag(H))
    return s * np.linalg.solve(H * s[:, None] * s[None, :], -g * s)


def host_calibration(O, k0, cams0, tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE, max_iter=200):
    """Dense Levenberg-Marquardt on the calibration problem from (k0, cams0), run until the step is at the rounding
    floor of the unknowns.  Returns (k, cams, cost, J^T J at the result)."""
    k, cams = np.array(k0, np.float64), np.array(cams0, np.float64)
    n_img = len(cams)
    cost, r, J = calib_system(O, k, cams, tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a, mask)
    lam = 1e-4
    for _ in range(max_iter):
        H, g = J.T @ J, J.T @ r
        try:
            step = _damped_step(H, g, lam, mask)
        except np.linalg.LinAlgError:
            lam *= 10.0
            continue
        size = max(np.abs(step[:6 * n_img]).max(), (np.abs(step[6 * n_img:]) / np.maximum(np.abs(k), 1.0)).max())
        if size < 1e-15:
            break
        cand_k = k + step[6 * n_img:]
        cand = np.array([O.pose_plus(cams[i], step[6 * i:6 * i + 6]) for i in range(n_img)])
        c2, r2, J2 = calib_system(O, cand_k, cand, tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a, mask)
        if c2 < cost:
            k, cams, cost, r, J = cand_k, cand, c2, r2, J2
            lam = max(lam * 0.1, 1e-15)
        else:
            if lam > 1e8:
                break
            lam *= 10.0
    return k, cams, cost, J.T @ J


def joint_covariance(H, n_img, mask=ALL_FREE):
    """(intr_cov (9, 9), cam_cov (n_img, 6, 6)): the blocks of the inverse of the full J^T J; the rows and columns of
    the parameters outside the mask are zero."""
    free = [6 * n_img + j for j in range(9) if (mask >> j) & 1]
    keep = list(range(6 * n_img)) + free
    inv = np.zeros_like(H)
    inv[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    cam_cov = np.array([inv[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n_img)])
    return inv[6 * n_img:, 6 * n_img:], cam_cov


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


# ---- the yardstick against central differences ----------------------------------------------------------------------

def test_reference_jacobian_matches_central_differences_of_the_oracle(oracle):
    """calib_system's nine intrinsic columns against central differences of oracle.obs_eval on the distortion scene.
    The residual is linear in each of the nine parameters (u = fx xd + cx, and xd is linear in k1, k2, k3, p1, p2), so a
    central difference has no truncation error and the step can be large: h_j = 1e-3 max(|k_j|, 1).  What is left is
    the rounding of the two residuals, 2 eps |u| / (2 h) <= 1.2e-16 * 1e4 / 1e-3 = 1.2e-9 per entry (pixel coordinates
    stay below 1e4): the bound is 1e-8 absolute on every entry."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=12, n_tags=8, visibility=0.6)
    assert np.abs(s.dist).max() > 0
    k = np.concatenate([s.intr, s.dist])
    n = min(len(s.obs_tag), 40)
    img, tag, px = s.obs_cam[:n], s.obs_tag[:n], s.obs_px[:n]
    cost, r, J = calib_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, img, tag, px, robust=False)
    n_img = len(s.cam_gt)
    assert J.shape == (8 * n, 6 * n_img + 9) and abs(cost - 0.5 * r @ r) <= 1e-12 * cost
    worst = 0.0
    for j in range(9):
        h = 1e-3 * max(abs(k[j]), 1.0)
        kp, km = k.copy(), k.copy()
        kp[j] += h
        km[j] -= h
        num = np.concatenate([(oracle.obs_eval(kp[:4], kp[4:], s.cam_gt[img[o]], s.tag_gt[tag[o]], s.tag_wh[tag[o]], px[o], jac=False)
                               - oracle.obs_eval(km[:4], km[4:], s.cam_gt[img[o]], s.tag_gt[tag[o]], s.tag_wh[tag[o]], px[o], jac=False))
                              / (kp[j] - km[j]) for o in range(n)])
        col = J[:, 6 * n_img + j]
        err = np.abs(col - num).max()
        print("parameter %d: max |column| %.3g, largest error %.3g" % (j, np.abs(num).max(), err))
        worst = max(worst, err)
        assert np.abs(px).max() < 1e4 and err <= 1e-8, (j, err)
    # the pose columns are the oracle's own, each in its image's block; a masked parameter has a zero column
    r0, Jc, _ = oracle.obs_eval(k[:4], k[4:], s.cam_gt[img[3]], s.tag_gt[tag[3]], s.tag_wh[tag[3]], px[3])
    assert (J[24:32, 6 * img[3]:6 * img[3] + 6] == Jc).all() and (r[24:32] == r0).all()
    assert np.count_nonzero(J[24:32, :6 * n_img]) == np.count_nonzero(Jc)
    _, _, Jm = calib_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, img, tag, px, robust=False, mask=0xF)
    assert (Jm[:, 6 * n_img + 4:] == 0).all() and (Jm[:, :6 * n_img + 4] == J[:, :6 * n_img + 4]).all()
    # the loss: rows and residuals scaled by sqrt(rho'), cost = 1/2 sum rho
    big = px.copy()
    big[0] += 5.0
    cost_h, r_h, J_h = calib_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, img, tag, big, robust=True)
    cost_p, r_p, J_p = calib_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, img, tag, big, robust=False)
    sq = r_p[0] ** 2 + r_p[1] ** 2
    assert sq > 1.0 and abs(r_h[0] / r_p[0] - sq ** -0.25) <= 1e-12
    assert np.allclose(J_h[0], J_p[0] * sq ** -0.25, rtol=1e-12, atol=0)
    assert cost_h < cost_p
