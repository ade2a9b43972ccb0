"""CPU-only checks of the self-calibrating bundle adjustment (ABI 6, additive: vmm_ba_set_intrinsics,
vmm_ba_get_intrinsics, vmm_ba_intrinsics_system, vmm_ba_default_selfcal_options, vmm_ba_solve_selfcal): declared, listed,
exported, laid out as the header says, refusing null arguments before any device call -- and the yardstick of
tests/test_gpu_selfcal.py, proven here before the GPU tests lean on it.

The yardstick is numpy around oracle/oracle.py and never calls the code under test:
    joint_system      the dense Jacobian over cameras, tags and the nine numbers of the camera model (obs_eval for the
                      pose columns, test_calibrate_cpu.intrinsic_columns for the model's), the loss applied as in
                      calib_system; proven below against central differences of the oracle
    host_joint_lm     dense Levenberg-Marquardt over all unknowns at once
    host_eliminated   the scheme vmm_ba_solve_selfcal runs: solve the poses for a fixed model, one LM step on the reduced
                      system S_k = C - B' A^-1 B of the model, repeat
Two optimisers that share nothing but joint_system end at the same optimum; how far apart they stop is the yardstick's own
spread, recorded in HOST_* below.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_calibrate_cpu import ALL_FREE, intrinsic_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_set_intrinsics", "vmm_ba_get_intrinsics", "vmm_ba_intrinsics_system", "vmm_ba_default_selfcal_options",
       "vmm_ba_solve_selfcal")
# the start of tests/test_gpu_calibrate.py: the truth plus this
PERTURB = np.array([200.0, -150.0, 30.0, -25.0, 0.02, -0.05, 1e-3, -1e-3, 0.02])
# How far apart host_joint_lm and host_eliminated stop on make_scene(1) (20 x 10, 200 observations, 0.3 px noise), robust,
# both from the truth poses and truth + PERTURB, the inner pose solves run to a step of 1e-8.  Measured with numpy around
# the oracle when the scheme was specified: the worst parameter 1.4e-6 standard deviations apart (sigma from the inverse of
# the full J'J), the worst pose 1e-8, the costs 4e-13 relative (the cost is flat to second order in the gap).
# test_the_two_host_optimisers_agree prints this build's figures and holds them to ten times these; the GPU tests give the
# device the same ten times.
HOST_SIGMA_GAP = 1.4e-6
HOST_POSE_GAP = 1e-8
HOST_COST_GAP = 4e-13


# ---- the yardstick --------------------------------------------------------------------------------------------------

def joint_system(O, k, cams, tags, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE,
                 obs_on=None, cam_const=None, tag_const=None, want_magnitude=False):
    """The joint problem at (k, cams, tags): cost = 1/2 sum rho(|r_corner|^2) over the active observations, the residuals
    (8 per observation) and the dense Jacobian over (6 per camera, 6 per tag, the nine of k), both with the loss applied
    as Ceres' corrector does for rho'' <= 0 (rows and residuals scaled by sqrt(rho')).  The fixed tag and the constant
    poses have zero columns; a switched-off observation has zero rows; a parameter outside `mask` has zero columns.
    want_magnitude: also |J| and the per-row residual magnitude w (|projection| + |observation|), for per-entry bounds."""
    n, nc, nt = len(obs_tag), len(cams), len(tags)
    r_all, J = np.zeros(8 * n), np.zeros((8 * n, 6 * nc + 6 * nt + 9))
    rmag = np.zeros(8 * n)
    free = np.array([(mask >> j) & 1 for j in range(9)], np.float64)
    cost = 0.0
    for o in range(n):
        if obs_on is not None and not obs_on[o]:
            continue
        i, t = int(obs_cam[o]), int(obs_tag[o])
        r, Jc, Jt = O.obs_eval(k[:4], k[4:], cams[i], tags[t], tag_wh[t], obs_px[o])
        Jk = intrinsic_columns(k, cams[i], tags[t], tag_wh[t]) * free
        if cam_const is not None and cam_const[i]:
            Jc = np.zeros_like(Jc)
        if t == fixed_tag or (tag_const is not None and tag_const[t]):
            Jt = np.zeros_like(Jt)
        for c in range(4):
            rows = slice(2 * c, 2 * c + 2)
            out = slice(8 * o + 2 * c, 8 * o + 2 * c + 2)
            sq = float(r[rows] @ r[rows])
            rho = O.huber(a, sq) if robust else (sq, 1.0, 0.0)
            w = np.sqrt(rho[1])
            cost += 0.5 * rho[0]
            r_all[out] = w * r[rows]
            rmag[out] = w * (np.abs(r[rows] + obs_px[o][rows]) + np.abs(obs_px[o][rows]))
            J[out, 6 * i:6 * i + 6] = w * Jc[rows]
            J[out, 6 * nc + 6 * t:6 * nc + 6 * t + 6] = w * Jt[rows]
            J[out, 6 * (nc + nt):] = w * Jk[rows]
    if want_magnitude:
        return cost, r_all, J, rmag
    return cost, r_all, J


def reduced_system(r, J, n_pose6):
    """(g_k, C, r_k, S_k) of joint_system's (r, J): the border and the model's system with every pose eliminated.  Poses
    without a column (constant, unobserved) get a unit diagonal, as the library gives them."""
    Jp, Jk = J[:, :n_pose6], J[:, n_pose6:]
    A, B, Cm = Jp.T @ Jp, Jp.T @ Jk, Jk.T @ Jk
    g, gk = Jp.T @ r, Jk.T @ r
    dead = np.diag(A) == 0.0
    A[dead, dead] = 1.0
    AiB, Aig = np.linalg.solve(A, B), np.linalg.solve(A, g)
    return gk, Cm, gk - B.T @ Aig, Cm - B.T @ AiB


def _unit_rows(H, g, dead):
    H, g = H.copy(), g.copy()
    H[dead, :] = 0.0
    H[:, dead] = 0.0
    H[dead, dead] = 1.0
    g[dead] = 0.0
    return H, g


def _lm_step(H, g, lam):
    """(H + lam diag H) step = -g, Jacobi-scaled; unknowns without a column get a unit row and a zero step."""
    dead = np.diag(H) == 0.0
    H, g = _unit_rows(H, g, dead)
    H[np.diag_indices_from(H)] += lam * np.where(dead, 0.0, np.diag(H))
    s = 1.0 / np.sqrt(np.diag(H))
    return s * np.linalg.solve(H * s[:, None] * s[None, :], -g * s)


def _plus(O, cams, tags, step):
    nc = len(cams)
    return (np.array([O.pose_plus(cams[i], step[6 * i:6 * i + 6]) for i in range(nc)]),
            np.array([O.pose_plus(tags[t], step[6 * nc + 6 * t:6 * nc + 6 * t + 6]) for t in range(len(tags))]))


def host_joint_lm(O, k0, cams0, tags0, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE,
                  max_iter=300, **kw):
    """Dense Levenberg-Marquardt over cameras, tags and k at once from (k0, cams0, tags0), run until the step is at the
    rounding floor of the unknowns.  Returns (k, cams, tags, cost, J'J at the result)."""
    k, cams, tags = np.array(k0, np.float64), np.array(cams0, np.float64), np.array(tags0, np.float64)
    n6 = 6 * (len(cams) + len(tags))
    args = (tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a, mask)
    cost, r, J = joint_system(O, k, cams, tags, *args, **kw)
    lam = 1e-4
    for _ in range(max_iter):
        step = _lm_step(J.T @ J, J.T @ r, lam)
        size = max(np.abs(step[:n6]).max(), (np.abs(step[n6:]) / np.maximum(np.abs(k), 1.0)).max())
        if size < 1e-15:
            break
        ck = k + step[n6:]
        cc, ct = _plus(O, cams, tags, step)
        c2, r2, J2 = joint_system(O, ck, cc, ct, *args, **kw)
        if c2 < cost:
            k, cams, tags, cost, r, J = ck, cc, ct, c2, r2, J2
            lam = max(lam * 0.1, 1e-15)
        else:
            if lam > 1e8:
                break
            lam *= 10.0
    return k, cams, tags, cost, J.T @ J


def _pose_lm(O, k, cams, tags, args, tol, kw, max_iter=200):
    """The inner problem: LM over the poses for a fixed model until the step is below tol.  Returns the state, its cost,
    (r, J) there and the iterations spent."""
    n6 = 6 * (len(cams) + len(tags))
    cost, r, J = joint_system(O, k, cams, tags, *args, **kw)
    lam, it = 1e-4, 0
    for it in range(1, max_iter + 1):
        Jp = J[:, :n6]
        step = _lm_step(Jp.T @ Jp, Jp.T @ r, lam)
        if np.abs(step).max() < tol:
            break
        cc, ct = _plus(O, cams, tags, step)
        c2, r2, J2 = joint_system(O, k, cc, ct, *args, **kw)
        if c2 < cost:
            cams, tags, cost, r, J = cc, ct, c2, r2, J2
            lam = max(lam * 0.1, 1e-15)
        else:
            if lam > 1e8:
                break
            lam *= 10.0
    return cams, tags, cost, r, J, it


def host_eliminated(O, k0, cams0, tags0, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE,
                    inner_tol=1e-8, max_outer=30, parameter_tolerance=1e-10, function_tolerance=1e-12, **kw):
    """vmm_ba_solve_selfcal's scheme in numpy: the poses solved for the fixed model; then per outer iteration one step
    (S_k + lam diag S_k) dk = -r_k, the poses solved again from where they are, the step accepted on a strictly lower
    cost (lam x 0.1 from 1e-4) and otherwise undone (lam x 10); the same stopping rules.
    Returns (k, cams, tags, cost, log) with log = [(accepted, inner iterations, cost)]."""
    k = np.array(k0, np.float64)
    n6 = 6 * (len(cams0) + len(tags0))
    args = (tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a, mask)
    cams, tags, cost, r, J, it = _pose_lm(O, k, np.array(cams0, np.float64), np.array(tags0, np.float64), args, inner_tol, kw)
    log = [(True, it, cost)]
    lam = 1e-4
    for _ in range(max_outer):
        if lam > 1e12:
            break
        _, _, rk, Sk = reduced_system(r, J, n6)
        dk = _lm_step(Sk, rk, lam)
        cc, ct, c2, r2, J2, it = _pose_lm(O, k + dk, cams, tags, args, inner_tol, kw)
        log.append((bool(c2 < cost), it, c2))
        if c2 < cost:
            small = (np.abs(dk) / np.maximum(np.abs(k), 1.0)).max() < parameter_tolerance
            rel = (cost - c2) / cost
            k, cams, tags, cost, r, J = k + dk, cc, ct, c2, r2, J2
            lam *= 0.1
            if small or rel < function_tolerance:
                break
        else:
            if c2 - cost <= 1e-10 * cost + 1e-20:
                break
            lam *= 10.0
    return k, cams, tags, cost, log


def model_covariance(H, n_pose6, mask=ALL_FREE):
    """The 9 x 9 block of the inverse of the full J'J (unknowns without a column left out); zero rows and columns for the
    parameters outside the mask."""
    keep = [j for j in range(len(H)) if H[j, j] != 0.0 and (j < n_pose6 or (mask >> (j - n_pose6)) & 1)]
    inv = np.zeros_like(H)
    inv[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    return inv[n_pose6:, n_pose6:]


def pose_gap(a, b):
    """max over the poses of |dq| (unit quaternions, sign-aligned) and |dt| / max(|t|, 1), as tests/test_gpu_calibrate.py."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    qa = a[:, :4] / np.linalg.norm(a[:, :4], axis=1, keepdims=True)
    qb = b[:, :4] / np.linalg.norm(b[:, :4], axis=1, keepdims=True)
    sign = np.sign(np.sum(qa * qb, axis=1))[:, None]
    dq = np.linalg.norm(qa * sign - qb, axis=1)
    dt = np.linalg.norm(a[:, 4:] - b[:, 4:], axis=1) / np.maximum(np.linalg.norm(b[:, 4:], axis=1), 1.0)
    return max(float(dq.max()), float(dt.max()))


def scene_args(s):
    return s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px


# ---- the entry points -----------------------------------------------------------------------------------------------

def test_selfcal_entry_points_are_declared_listed_and_exported():
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


def test_selfcal_structs_match_the_header_layout_and_defaults():
    from visual_marker_mapping_amd import _lib
    O, R = _lib.SelfcalOptions, _lib.SelfcalReport
    assert C.sizeof(O) == 24 and [getattr(O, f).offset for f, _ in O._fields_] == [0, 4, 8, 16]      # 2 x int32, 2 x double
    assert C.sizeof(R) == 40 and [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 24, 32]
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    for struct, cls in (("vmm_ba_selfcal_options", O), ("vmm_ba_selfcal_report", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    o = O()
    _lib.lib().vmm_ba_default_selfcal_options(C.byref(o))
    assert (o.max_outer_iterations, o.refine_mask, o.parameter_tolerance, o.function_tolerance) == (30, 0x1FF, 1e-10, 1e-12)
    _lib.lib().vmm_ba_default_selfcal_options(None)   # a null pointer is ignored


def test_selfcal_entry_points_refuse_null_arguments_without_a_device():
    from visual_marker_mapping_amd import _lib
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    intr, dist, cov = np.ones(4), np.zeros(5), np.zeros(81)
    rep = _lib.SelfcalReport()
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    assert L.vmm_ba_set_intrinsics(None, p(intr), p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_set_intrinsics(fake, None, p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_set_intrinsics(fake, p(intr), None) == _lib.ERR_ARGUMENT
    for v in (np.nan, np.inf, -np.inf):
        for bad_intr, bad_dist in ((np.array([1.0, v, 1.0, 1.0]), dist), (intr, np.array([0.0, 0.0, v, 0.0, 0.0]))):
            assert L.vmm_ba_set_intrinsics(fake, p(bad_intr), p(bad_dist)) == _lib.ERR_ARGUMENT
            assert b"finite" in L.vmm_ba_last_error()
    assert L.vmm_ba_get_intrinsics(None, p(intr), p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_get_intrinsics(fake, None, p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_get_intrinsics(fake, p(intr), None) == _lib.ERR_ARGUMENT
    c = C.c_double(0)
    assert L.vmm_ba_intrinsics_system(None, 1, 1.0, C.byref(c), p(cov), p(cov), p(cov), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(None, None, None, None, C.byref(rep), p(intr), p(dist), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(fake, None, None, None, None, p(intr), p(dist), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(fake, None, None, None, C.byref(rep), None, p(dist), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(fake, None, None, None, C.byref(rep), p(intr), None, p(cov)) == _lib.ERR_ARGUMENT
    for kw in (dict(refine_mask=-1), dict(refine_mask=0x200), dict(max_outer_iterations=-1),
               dict(parameter_tolerance=-1.0), dict(function_tolerance=np.nan)):
        o = _lib.SelfcalOptions()
        L.vmm_ba_default_selfcal_options(C.byref(o))
        for name, v in kw.items():
            setattr(o, name, v)
        assert L.vmm_ba_solve_selfcal(fake, None, C.byref(o), None, C.byref(rep), p(intr), p(dist), p(cov)) == _lib.ERR_ARGUMENT, kw
        assert b"solve_selfcal" in L.vmm_ba_last_error()


def test_selfcalibration_main_needs_a_reconstruction(tmp_path):
    from visual_marker_mapping_amd import selfcalibration
    with pytest.raises(FileNotFoundError) as ei:
        selfcalibration.main(["--project_path", str(tmp_path)])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
    (tmp_path / "reconstruction.json").write_text("{}")
    with pytest.raises(FileNotFoundError) as ei:
        selfcalibration.main(["--project_path", str(tmp_path)])
    assert "marker_detections.json" in str(ei.value) and "does not exist" in str(ei.value)
    with pytest.raises(SystemExit):
        selfcalibration.main(["--project_path", str(tmp_path), "--refine_mask", "0x200"])


def test_do_bundle_adjustment_keeps_its_defaults():
    """refineCameraModel is off unless asked for: the positional arguments of doBundleAdjustment are those it had."""
    import inspect
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    sig = inspect.signature(TagReconstructor.doBundleAdjustment)
    assert list(sig.parameters)[:6] == ["self", "maxNumIterations", "ceresThreads", "robustify", "printSummary", "elimination"]
    assert sig.parameters["refineCameraModel"].default is False and sig.parameters["refine_mask"].default == 0x1FF


# ---- the yardstick against central differences ----------------------------------------------------------------------

def test_joint_jacobian_matches_central_differences_of_the_oracle(oracle):
    """Every column of joint_system against central differences of oracle.obs_eval on the distortion scene at the truth.
    The nine model columns: the residual is linear in each parameter, so the step can be large, h = 1e-3 max(|k_j|, 1),
    and what is left is the rounding of the two residuals, 2 eps |u| / (2 h) <= 1.2e-9 with pixel coordinates below 1e4:
    the bound is 1e-8 absolute (tests/test_calibrate_cpu.py).  The pose columns: h = 1e-6 in the tangent, truncation
    h^2 |J'''| / 6 and rounding eps |u| / h = 1.1e-16 * 1e4 / 1e-6 = 1.1e-6 per entry against entries of 1e3 .. 1e5; the
    bound is 1e-4 absolute + 1e-6 relative, far below any entry a wrong column would miss by."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=12, n_tags=8, visibility=0.6)
    k = np.concatenate([s.intr, s.dist])
    n = min(len(s.obs_tag), 24)
    oc, ot, px = s.obs_cam[:n], s.obs_tag[:n], s.obs_px[:n]
    nc, nt = len(s.cam_gt), len(s.tag_gt)
    cam_const = np.zeros(nc, bool)
    cam_const[oc[1]] = True
    cost, r, J = joint_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, oc, ot, px, robust=False,
                              cam_const=cam_const)
    assert J.shape == (8 * n, 6 * (nc + nt) + 9) and abs(cost - 0.5 * r @ r) <= 1e-12 * cost

    def residuals(kk, cams, tags):
        return np.concatenate([oracle.obs_eval(kk[:4], kk[4:], cams[oc[o]], tags[ot[o]], s.tag_wh[ot[o]], px[o], jac=False)
                               for o in range(n)])

    assert np.abs(px).max() < 1e4
    worst_k = worst_p = 0.0
    for j in range(9):
        h = 1e-3 * max(abs(k[j]), 1.0)
        kp, km = k.copy(), k.copy()
        kp[j] += h
        km[j] -= h
        num = (residuals(kp, s.cam_gt, s.tag_gt) - residuals(km, s.cam_gt, s.tag_gt)) / (kp[j] - km[j])
        worst_k = max(worst_k, np.abs(J[:, 6 * (nc + nt) + j] - num).max())
    for col in range(6 * (nc + nt)):
        is_cam, p, a = col < 6 * nc, (col if col < 6 * nc else col - 6 * nc) // 6, col % 6
        constant = (is_cam and cam_const[p]) or (not is_cam and p == s.fixed_tag)
        if constant:
            assert not J[:, col].any(), col
            continue
        if not J[:, col].any():
            continue   # a pose outside the first n observations
        d = np.zeros(6)
        d[a] = 1e-6
        cp, cm, tp, tm = s.cam_gt.copy(), s.cam_gt.copy(), s.tag_gt.copy(), s.tag_gt.copy()
        if is_cam:
            cp[p], cm[p] = oracle.pose_plus(s.cam_gt[p], d), oracle.pose_plus(s.cam_gt[p], -d)
        else:
            tp[p], tm[p] = oracle.pose_plus(s.tag_gt[p], d), oracle.pose_plus(s.tag_gt[p], -d)
        num = (residuals(k, cp, tp) - residuals(k, cm, tm)) / 2e-6
        err = np.abs(J[:, col] - num) - 1e-6 * np.abs(num)
        worst_p = max(worst_p, err.max())
    print("largest error of a model column %.3g, of a pose column (beyond 1e-6 relative) %.3g" % (worst_k, worst_p))
    assert worst_k <= 1e-8 and worst_p <= 1e-4
    # the loss, the observation switch and the parameter mask
    big = px.copy()
    big[0] += 5.0
    _, r_h, J_h = joint_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, oc, ot, big, robust=True)
    _, r_p, J_p = joint_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, oc, ot, big, robust=False)
    sq = r_p[0] ** 2 + r_p[1] ** 2
    assert sq > 1.0 and abs(r_h[0] / r_p[0] - sq ** -0.25) <= 1e-12 and np.allclose(J_h[0], J_p[0] * sq ** -0.25, rtol=1e-12, atol=0)
    on = np.ones(n, bool)
    on[::5] = False
    c_m, r_m, J_m = joint_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, oc, ot, px, robust=False, obs_on=on,
                                 cam_const=cam_const)
    assert not r_m[:8].any() and not J_m[:8].any() and (J_m[8:40] == J[8:40]).all() and c_m < cost
    _, _, J4 = joint_system(oracle, k, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, oc, ot, px, robust=False, mask=0xF,
                            cam_const=cam_const)
    assert not J4[:, -5:].any() and (J4[:, :-5] == J[:, :-5]).all()
    # the reduced system is the Schur complement of the pose block
    gk, Cm, rk, Sk = reduced_system(r, J, 6 * (nc + nt))
    H = J.T @ J
    dead = np.diag(H) == 0.0
    H[dead, dead] = 1.0
    full = np.linalg.inv(H)[-9:, -9:]
    assert np.allclose(np.linalg.inv(Sk), full, rtol=1e-6, atol=0)


def test_the_two_host_optimisers_agree(oracle):
    """host_joint_lm and host_eliminated on make_scene(1), robust, from the truth poses and truth + PERTURB: the worst
    parameter gap in sigma, the worst pose gap and the relative cost gap are printed and held to ten times HOST_*."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    k0 = np.concatenate([s.intr, s.dist]) + PERTURB
    kj, cj, tj, cost_j, H = host_joint_lm(oracle, k0, s.cam_gt, s.tag_gt, *scene_args(s), robust=True)
    ke, ce, te, cost_e, log = host_eliminated(oracle, k0, s.cam_gt, s.tag_gt, *scene_args(s), robust=True)
    n6 = 6 * (len(cj) + len(tj))
    sigma = np.sqrt(np.diag(model_covariance(H, n6)))
    gap = np.abs(kj - ke) / sigma
    pg = max(pose_gap(ce, cj), pose_gap(te, tj))
    rel = abs(cost_e - cost_j) / cost_j
    print("outer iterations %d (accepted %d), inner iterations %s" % (len(log) - 1, sum(a for a, _, _ in log[1:]),
                                                                      [it for _, it, _ in log]))
    print("sigma %s" % np.array2string(sigma, precision=3))
    print("worst parameter gap %.3g sigma (recorded %.3g), worst pose gap %.3g (recorded %.3g), relative cost gap %.3g "
          "(recorded %.3g); cost %.15g" % (gap.max(), HOST_SIGMA_GAP, pg, HOST_POSE_GAP, rel, HOST_COST_GAP, cost_j))
    assert np.isfinite(sigma).all() and (sigma > 0).all()
    assert sigma[0] < 1e-2 * kj[0]   # fx is determined to a few pixels at 8075: the tags alone identify the model
    assert gap.max() <= 10 * HOST_SIGMA_GAP and pg <= 10 * HOST_POSE_GAP and rel <= 10 * HOST_COST_GAP
    assert len(log) - 1 <= 30
