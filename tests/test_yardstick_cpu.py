"""The proofs of the host yardstick (tests/yardstick.py, tests/rig_cases.py), on the CPU, before the GPU tests lean on it:
every Jacobian against central differences of oracle/oracle.py, the two self-calibration optimisers against each other,
the Levenberg-Marquardt loop on exact data.
"""
import numpy as np

import rig_cases as rc
from yardstick import (HOST_COST_GAP, HOST_POSE_GAP, HOST_SIGMA_GAP, PERTURB, calib_system, host_eliminated, host_joint_lm,
                       joint_system, model_covariance, pose_gap, reduced_system, rotation, scene_args)


# ---- the calibration against a finished map ---------------------------------------------------------------------------

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


# ---- the joint problem of the self-calibrating bundle adjustment ------------------------------------------------------

def test_joint_jacobian_matches_central_differences_of_the_oracle(oracle):
    """Every column of joint_system against central differences of oracle.obs_eval on the distortion scene at the truth.
    The nine model columns: the residual is linear in each parameter, so the step can be large, h = 1e-3 max(|k_j|, 1),
    and what is left is the rounding of the two residuals, 2 eps |u| / (2 h) <= 1.2e-9 with pixel coordinates below 1e4:
    the bound is 1e-8 absolute (the test above).  The pose columns: h = 1e-6 in the tangent, truncation
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
    pg = max(*pose_gap(ce, cj), *pose_gap(te, tj))
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


# ---- the rig ----------------------------------------------------------------------------------------------------------

def test_rig_jacobian_matches_central_differences_of_the_oracle(oracle):
    """rig_system's columns over both tangents against central differences of oracle.obs_eval at the composed pose, the
    poses moved by the oracle's Plus, on the distortion scene with three different camera models.
    The bound.  A pixel coordinate is u = f xd(X / Z) with f <= 8200 and |X / Z| <= 0.42 inside the 6000 x 4000 image.
    In a half-angle rotation step h the ray turns by 2 h, so d^3 u / dh^3 = 8 f tan''' <= 8 * 8200 * 2 (1 + x^2)(1 + 3 x^2)
    <= 2.4e5; along the optical axis at depth Z it is 6 f |x| / Z^3 <= 2.1e4 / Z^3 <= 7.7e5 for Z >= 0.3 m (asserted
    below; an extrinsic rotation moves the point by its lever arm, below 1 m here, which the same figure covers).  The
    distortion of this scene changes the pixel by a few per cent; a factor 2 covers its derivatives: M3 <= 1.6e6.
    Truncation h^2 M3 / 6 = 2.7e-5 at h = 1e-5.  Rounding: each residual carries a few eps |u| <= 5 * 2.2e-16 * 1e4, the
    difference of two over 2 h gives 1.1e-6.  The bound is 5e-5 absolute on entries of magnitude 1e4."""
    intr = np.array([[8075.0, 8083.0, 3016.0, 1996.0], [7900.0, 7950.0, 2950.0, 2050.0], [8150.0, 8100.0, 3060.0, 1960.0]])
    dist = np.array([[-0.186, 0.370, -2.9e-4, 4.2e-4, 0.057], [-0.10, 0.15, 3e-4, -2e-4, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    s = rc.rig_scene("distortion_12x8", intr=intr, dist=dist, noise_px=0.5, seed=3)
    keep = np.zeros(len(s.obs_tag), bool)
    keep[::7] = True   # every camera and most frames, about 36 observations
    idx = np.flatnonzero(keep)
    assert set(s.obs_cam[idx]) == {0, 1, 2} and np.abs(s.obs_px).max() < 1e4
    for o in idx:
        cam = rc.compose(s.ext_qt[s.obs_cam[o]], s.rig_gt[s.obs_frame[o]])
        assert (rotation(cam) @ s.tag_gt[s.obs_tag[o], 4:] + cam[4:])[2] >= 0.3 + 0.1
    F, K = s.n_frames, s.n_rig_cams
    cost, r, J = rc.rig_system(oracle, s, s.rig_gt, s.ext_qt, keep)
    assert J.shape == (8 * len(idx), 6 * F + 6 * K) and abs(cost - 0.5 * r @ r) <= 1e-12 * cost
    h = 1e-5
    worst = 0.0
    for col in range(6 * F + 6 * K):
        step = np.zeros(6)
        step[col % 6] = h
        num = np.zeros(8 * len(idx))
        for n, o in enumerate(idx):
            f, c, t = int(s.obs_frame[o]), int(s.obs_cam[o]), int(s.obs_tag[o])
            if (col < 6 * F and col // 6 != f) or (col >= 6 * F and (col - 6 * F) // 6 != c):
                continue
            side = []
            for sgn in (1.0, -1.0):
                rig, ext = s.rig_gt[f], s.ext_qt[c]
                if col < 6 * F:
                    rig = oracle.pose_plus(rig, sgn * step)
                else:
                    ext = oracle.pose_plus(ext, sgn * step)
                side.append(oracle.obs_eval(s.intr[c], s.dist[c], rc.compose(ext, rig), s.tag_gt[t], s.tag_wh[t], s.obs_px[o],
                                            jac=False))
            num[8 * n:8 * n + 8] = (side[0] - side[1]) / (2 * h)
        err = np.abs(J[:, col] - num).max()
        worst = max(worst, err)
        assert err <= 5e-5, (col, err)
    print("largest |J| %.3g, largest error against central differences %.3g" % (np.abs(J).max(), worst))
    assert np.abs(J).max() > 1e3
    # an observation touches its frame and its camera only
    o = 5
    f, c = int(s.obs_frame[idx[o]]), int(s.obs_cam[idx[o]])
    rows = J[8 * o:8 * o + 8]
    mask = np.zeros(6 * F + 6 * K, bool)
    mask[6 * f:6 * f + 6] = mask[6 * F + 6 * c:6 * F + 6 * c + 6] = True
    assert (rows[:, ~mask] == 0).all() and np.count_nonzero(rows[:, mask]) == 96
    # the loss: rows and residuals scaled by sqrt(rho'), cost = 1/2 sum rho
    big = rc.select(s, keep)
    big.obs_px = big.obs_px.copy()
    big.obs_px[0] += 5.0
    cost_h, r_h, J_h = rc.rig_system(oracle, big, s.rig_gt, s.ext_qt, None, robust=True)
    cost_p, r_p, J_p = rc.rig_system(oracle, big, s.rig_gt, s.ext_qt, None, robust=False)
    sq = r_p[0] ** 2 + r_p[1] ** 2
    assert sq > 1.0 and abs(r_h[0] / r_p[0] - sq ** -0.25) <= 1e-12
    assert np.allclose(J_h[0], J_p[0] * sq ** -0.25, rtol=1e-12, atol=0) and cost_h < cost_p


def test_host_frame_optimum_recovers_the_truth_on_exact_data(oracle):
    """The yardstick's own Levenberg-Marquardt from a perturbed start on exact data: back at the truth to 1e-9."""
    s = rc.rig_scene("distortion_12x8", noise_px=0.0)
    keep = np.ones(len(s.obs_tag), bool)
    start = oracle.pose_plus(s.rig_gt[3], np.array([0.02, -0.01, 0.03, 0.004, -0.003, 0.002]))
    q, cost = rc.host_frame_optimum(oracle, s, 3, start, s.ext_qt, keep, robust=True)
    gq, gt = pose_gap(q, s.rig_gt[3])
    print("host optimum on exact data: |dq| %.3g |dt| %.3g cost %.3g" % (gq, gt, cost))
    assert gq <= 1e-9 and gt <= 1e-9
