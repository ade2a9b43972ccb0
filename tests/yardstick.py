"""The host yardstick of the finished-map and constant-pose tests: numpy around oracle/oracle.py, proven in
tests/test_yardstick_cpu.py before the GPU tests lean on it (DESIGN.md section 6 lists every piece).  It never imports the
code under test.  The rotation matrix is ref_geometry.py's (conventions there) with np.linalg.norm's |q|.

obs_eval gives the 8 residuals and the 8 x 6 pose Jacobians of one observation, point_eval the same for a free point,
huber gives rho, pose_plus moves a pose; the nine columns of the camera model are the closed forms of the cost functor's
projection (intrinsic_columns).  Everything else here is summation, a damped linear solve and one Levenberg-Marquardt loop.
"""
import numpy as np

import ref_geometry as rg
from eval_cases import MARGIN

ALL_FREE = 0x1FF
# the perturbed start of the calibration tests (the start the calibration issue's scipy check used): the truth plus this
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
# Parameter gap between the device and the host optimum, in standard deviations of the parameter (from the
# reference's covariance).  host_calibration and scipy.optimize.least_squares (trf, x_scale='jac', all tolerances 1e-15,
# analytic Jacobian, poses re-centred until the step vanished), both started at the truth on make_scene(1) at its 0.3 px
# noise, non-robust, ended 1.01e-6 sigma apart at the worst parameter (cx; costs 65.3073967012152 against
# 65.3073967012186: the cost is flat to rounding over that distance).  Ten times that, the device stopping on yet another
# criterion; the cap of 1e-3 sigma does not bind.
SIGMA_GAP = 1.01e-5
# The device's C, g_k and cost against joint_system's, entry by entry over the entry's magnitude: what
# profiles/eval_accuracy.jsonl records for the blocks of the same kind (tests/test_gpu_selfcal.py, "Tolerances"), times MARGIN.
BOUND_C, BOUND_G, BOUND_COST = MARGIN * 1.26e-12, MARGIN * 2.06e-15, MARGIN * 1.458e-13
REL = 1e-6  # north_star: "within 1e-6 relative"


# ---- poses ----------------------------------------------------------------------------------------------------------

def rotation(q):
    """The rotation matrix of the quaternion q = (w, x, y, z, ...), normalised first."""
    return rg.rotation(q, np.float64, norm="linalg")


def pose_gap(a, b):
    """(dq, dt) between one pose or many: max over the poses of |dq| (unit quaternions, sign-aligned) and of
    |dt| / max(|t|, 1); (0.0, 0.0) for an empty set."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    if a.size == 0:
        return 0.0, 0.0
    qa = a[:, :4] / np.linalg.norm(a[:, :4], axis=1, keepdims=True)
    qb = b[:, :4] / np.linalg.norm(b[:, :4], axis=1, keepdims=True)
    sign = np.sign(np.sum(qa * qb, axis=1))[:, None]
    dq = np.linalg.norm(qa * sign - qb, axis=1)
    dt = np.linalg.norm(a[:, 4:] - b[:, 4:], axis=1) / np.maximum(np.linalg.norm(b[:, 4:], axis=1), 1.0)
    return float(dq.max()), float(dt.max())


# ---- the loss and the two ways of summing it ------------------------------------------------------------------------

def corner_loss(O, r, robust, a=1.0, by_squares=False):
    """(rho, rho') of every corner of r (two residuals each): Huber of width a on |r_corner|^2, or the plain square.
    |r_corner|^2 is the corner's dot product with itself; by_squares forms it as r_x^2 + r_y^2, which is how the per-pose
    blocks have always been summed: the two can differ in the last bit (the dot product may be fused), and with them rho'
    of a corner beyond the width."""
    out = []
    for c in range(len(r) // 2):
        sq = r[2 * c] ** 2 + r[2 * c + 1] ** 2 if by_squares else float(r[2 * c:2 * c + 2] @ r[2 * c:2 * c + 2])
        rho = O.huber(a, sq) if robust else (sq, 1.0, 0.0)
        out.append((rho[0], rho[1]))
    return out


def assemble(O, n_cols, rows, robust, a=1.0):
    """The dense system of a problem whose `rows` yield (r8, [(first column, J 8 x k), ...]) per observation:
    cost = 1/2 sum rho(|r_corner|^2), the residuals (8 per observation), the Jacobian (8 per observation x n_cols) and the
    weights sqrt(rho') of the rows, residuals and Jacobian with the loss applied as Ceres' corrector does for rho'' <= 0
    (both scaled by sqrt(rho'))."""
    rows = list(rows)
    r_all, w_all, J = np.zeros(8 * len(rows)), np.zeros(8 * len(rows)), np.zeros((8 * len(rows), n_cols))
    cost = 0.0
    for n, (r, blocks) in enumerate(rows):
        loss = corner_loss(O, r, robust, a)
        for rho, _ in loss:
            cost += 0.5 * rho
        out = slice(8 * n, 8 * n + 8)
        w = w_all[out] = np.repeat(np.sqrt([d for _, d in loss]), 2)
        r_all[out] = w * r
        for first, Jb in blocks:
            J[out, first:first + Jb.shape[1]] = w[:, None] * Jb
    return cost, r_all, J, w_all


def block_normal(O, rows, robust, a=1.0):
    """cost, A = sum rho' J^T J and g = sum rho' J^T r of one small block whose `rows` yield (r2, J 2 x k) per corner.
    The weight multiplies the products, not the rows: this rounds differently from assemble's J^T J."""
    A = g = None
    cost = 0.0
    for r, J in rows:
        (rho, d), = corner_loss(O, r, robust, a)
        if A is None:
            A, g = np.zeros((J.shape[1], J.shape[1])), np.zeros(J.shape[1])
        cost += 0.5 * rho
        A += d * (J.T @ J)
        g += d * (J.T @ r)
    return cost, A, g


def image_rows(O, intr, dist, q, tag_qt, tag_wh, tags, pxs):
    """block_normal's rows of one image at camera pose q: the four corners of every observed tag."""
    for t, px in zip(tags, pxs):
        r, Jc, _ = O.obs_eval(intr, dist, q, tag_qt[t], tag_wh[t], px)
        for k in range(4):
            yield r[2 * k:2 * k + 2], Jc[2 * k:2 * k + 2]


def point_rows(O, intr, dist, cam_qt, X, cams, uvs):
    """block_normal's rows of one free point at X: one per view."""
    for c, uv in zip(cams, uvs):
        r, _, Jp = O.point_eval(intr, dist, cam_qt[c], X, uv)
        yield r, Jp


# ---- steps and the one Levenberg-Marquardt loop -----------------------------------------------------------------------

def plain_step(A, g, lam):
    """(A + lam diag(max(diag A, 1e-12))) step = -g."""
    return np.linalg.solve(A + lam * np.diag(np.maximum(np.diag(A), 1e-12)), -g)


def scaled_step(H, g, lam):
    """(H + lam diag H) step = -g, Jacobi-scaled; unknowns without a column (masked, constant, unobserved) get a unit row
    and a zero step."""
    dead = np.diag(H) == 0.0
    H, g = H.copy(), g.copy()
    H[dead, :] = 0.0
    H[:, dead] = 0.0
    H[dead, dead] = 1.0
    g[dead] = 0.0
    H[np.diag_indices_from(H)] += lam * np.where(dead, 0.0, np.diag(H))
    s = 1.0 / np.sqrt(np.diag(H))
    return s * np.linalg.solve(H * s[:, None] * s[None, :], -g * s)


def dense_lm(system, plus, x0, step, floor, size=lambda x, d: np.abs(d).max(), max_iter=200):
    """Levenberg-Marquardt from x0.  system(x) gives a tuple that starts with the cost, step(that tuple, lam) the damped
    step, plus(x, step) the moved state.  lam from 1e-4, x 0.1 on a strictly lower cost (floor 1e-15), x 10 otherwise and
    when the step cannot be solved; ends when size(x, step) < floor, above lam = 1e8, or after max_iter.
    Returns (x, cost, the system at x, iterations spent)."""
    x, sys = x0, system(x0)
    lam, it = 1e-4, 0
    for it in range(1, max_iter + 1):
        try:
            d = step(sys, lam)
        except np.linalg.LinAlgError:
            lam *= 10.0
            continue
        if size(x, d) < floor:
            break
        cand = plus(x, d)
        trial = system(cand)
        if trial[0] < sys[0]:
            x, sys = cand, trial
            lam = max(lam * 0.1, 1e-15)
        else:
            if lam > 1e8:
                break
            lam *= 10.0
    return x, sys[0], sys, it


def free_inverse(H, free):
    """The inverse of H over the index set `free` (indices or a bool mask), zero rows and columns elsewhere."""
    full = np.zeros_like(H)
    full[np.ix_(free, free)] = np.linalg.inv(H[np.ix_(free, free)])
    return full


def image_optimum(O, s, q0, tags, pxs, robust, a=1.0):
    """The pose of one image of scene s against the map tag_gt from q0, run until the step is at the rounding floor of
    the pose.  Returns (pose, cost, the largest scaled gradient entry there)."""
    q, cost, (_, A, g), _ = dense_lm(
        lambda q: block_normal(O, image_rows(O, s.intr, s.dist, q, s.tag_gt, s.tag_wh, tags, pxs), robust, a),
        O.pose_plus, np.array(q0, np.float64), lambda sys, lam: plain_step(sys[1], sys[2], lam), 1e-13)
    return q, cost, float(np.abs(g / np.sqrt(np.maximum(np.diag(A), 1e-300))).max())


def point_optimum(O, s, X0, cams, uvs, robust, a=1.0):
    """The free point seen by the cameras cam_gt of scene s from X0, run until the step is at the rounding floor of the
    point.  Returns (X, cost)."""
    return dense_lm(lambda X: block_normal(O, point_rows(O, s.intr, s.dist, s.cam_gt, X, cams, uvs), robust, a),
                    lambda X, d: X + d, np.array(X0, np.float64), lambda sys, lam: plain_step(sys[1], sys[2], lam), 1e-14)[:2]


# ---- the camera model: calibration against a finished map, and the joint problem --------------------------------------

def intrinsic_columns(k, cam_qt, tag_qt, wh):
    """The 8 x 9 Jacobian of one observation's residuals over k = (fx, fy, cx, cy, k1, k2, p1, p2, k3) for the cost
    functor's projection: xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2),
    u = fx xd + cx, v = fy yd + cy.  Corners LL, LR, UR, UL."""
    fx, fy = k[0], k[1]
    Rc, Rt = rotation(cam_qt[:4]), rotation(tag_qt[:4])
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


def _mask_columns(mask):
    return np.array([(mask >> j) & 1 for j in range(9)], np.float64)


def _model_step_size(n6):
    """The step of the poses as it is, that of the camera model relative to max(|k|, 1)."""
    return lambda x, d: max(np.abs(d[:n6]).max(), (np.abs(d[n6:]) / np.maximum(np.abs(x[0]), 1.0)).max())


def _normal_step(sys, lam):
    return scaled_step(sys[2].T @ sys[2], sys[2].T @ sys[1], lam)


def _moved(O, poses, step, first=0):
    return np.array([O.pose_plus(p, step[first + 6 * i:first + 6 * i + 6]) for i, p in enumerate(poses)])


def calib_system(O, k, cams, tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE):
    """The calibration problem at (k, cams): assemble's cost, residuals and Jacobian over (6 per image in `cams` order,
    then the nine of k).  obs_img indexes cams.  A parameter outside `mask` has zero columns."""
    free = _mask_columns(mask)

    def rows():
        for i, t, px in zip(obs_img, obs_tag, obs_px):
            r, Jc, _ = O.obs_eval(k[:4], k[4:], cams[i], tag_qt[t], tag_wh[t], px)
            yield r, [(6 * int(i), Jc), (6 * len(cams), intrinsic_columns(k, cams[i], tag_qt[t], tag_wh[t]) * free)]
    return assemble(O, 6 * len(cams) + 9, rows(), robust, a)[:3]


def host_calibration(O, k0, cams0, tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE, max_iter=200):
    """Dense Levenberg-Marquardt on the calibration problem from (k0, cams0), run until the step is at the rounding
    floor of the unknowns.  Returns (k, cams, cost, J^T J at the result)."""
    n6 = 6 * len(cams0)
    (k, cams), cost, (_, _, J), _ = dense_lm(
        lambda x: calib_system(O, x[0], x[1], tag_qt, tag_wh, obs_img, obs_tag, obs_px, robust, a, mask),
        lambda x, d: (x[0] + d[n6:], _moved(O, x[1], d)), (np.array(k0, np.float64), np.array(cams0, np.float64)),
        _normal_step, 1e-15, _model_step_size(n6), max_iter)
    return k, cams, cost, J.T @ J


def calibration_covariance(H, n_img, mask=ALL_FREE):
    """(intr_cov (9, 9), cam_cov (n_img, 6, 6)): the blocks of the inverse of the full J^T J; the rows and columns of
    the parameters outside the mask are zero."""
    inv = free_inverse(H, list(range(6 * n_img)) + [6 * n_img + j for j in range(9) if (mask >> j) & 1])
    return inv[6 * n_img:, 6 * n_img:], np.array([inv[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n_img)])


def joint_system(O, k, cams, tags, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE,
                 obs_on=None, cam_const=None, tag_const=None, want_magnitude=False):
    """The joint problem at (k, cams, tags): assemble's cost, residuals and Jacobian over (6 per camera, 6 per tag, the
    nine of k), the cost over the active observations.  The fixed tag and the constant poses have zero columns; a
    switched-off observation has zero rows; a parameter outside `mask` has zero columns.
    want_magnitude: also the per-row residual magnitude w (|projection| + |observation|), for per-entry bounds."""
    nc, nt = len(cams), len(tags)
    free = _mask_columns(mask)
    mag = np.zeros((len(obs_tag), 8))

    def rows():
        for o, (i, t) in enumerate(zip(obs_cam, obs_tag)):
            if obs_on is not None and not obs_on[o]:
                yield np.zeros(8), []
                continue
            r, Jc, Jt = O.obs_eval(k[:4], k[4:], cams[i], tags[t], tag_wh[t], obs_px[o])
            blocks = [(6 * (nc + nt), intrinsic_columns(k, cams[i], tags[t], tag_wh[t]) * free)]
            if cam_const is None or not cam_const[i]:
                blocks.append((6 * int(i), Jc))
            if t != fixed_tag and (tag_const is None or not tag_const[t]):
                blocks.append((6 * nc + 6 * int(t), Jt))
            mag[o] = np.abs(r + obs_px[o]) + np.abs(obs_px[o])
            yield r, blocks
    cost, r, J, w = assemble(O, 6 * (nc + nt) + 9, rows(), robust, a)
    return (cost, r, J, w * mag.ravel()) if want_magnitude else (cost, r, J)


def scene_args(s):
    return s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px


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


def host_joint_lm(O, k0, cams0, tags0, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE,
                  max_iter=300, **kw):
    """Dense Levenberg-Marquardt over cameras, tags and k at once from (k0, cams0, tags0), run until the step is at the
    rounding floor of the unknowns.  Returns (k, cams, tags, cost, J'J at the result)."""
    nc = len(cams0)
    n6 = 6 * (nc + len(tags0))
    (k, cams, tags), cost, (_, _, J), _ = dense_lm(
        lambda x: joint_system(O, x[0], x[1], x[2], tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a, mask, **kw),
        lambda x, d: (x[0] + d[n6:], _moved(O, x[1], d), _moved(O, x[2], d, 6 * nc)),
        (np.array(k0, np.float64), np.array(cams0, np.float64), np.array(tags0, np.float64)),
        _normal_step, 1e-15, _model_step_size(n6), max_iter)
    return k, cams, tags, cost, J.T @ J


def host_eliminated(O, k0, cams0, tags0, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a=1.0, mask=ALL_FREE,
                    inner_tol=1e-8, max_outer=30, parameter_tolerance=1e-10, function_tolerance=1e-12, **kw):
    """vmm_ba_solve_selfcal's scheme in numpy: the poses solved for the fixed model; then per outer iteration one step
    (S_k + lam diag S_k) dk = -r_k, the poses solved again from where they are, the step accepted on a strictly lower
    cost (lam x 0.1 from 1e-4) and otherwise undone (lam x 10); the same stopping rules.
    Returns (k, cams, tags, cost, log) with log = [(accepted, inner iterations, cost)]."""
    k = np.array(k0, np.float64)
    nc = len(cams0)
    n6 = 6 * (nc + len(tags0))

    def pose_lm(k, cams, tags):
        """The inner problem: LM over the poses for a fixed model until the step is below inner_tol."""
        def step(sys, lam):
            Jp = sys[2][:, :n6]
            return scaled_step(Jp.T @ Jp, Jp.T @ sys[1], lam)
        (cams, tags), cost, (_, r, J), it = dense_lm(
            lambda x: joint_system(O, k, x[0], x[1], tag_wh, fixed_tag, obs_cam, obs_tag, obs_px, robust, a, mask, **kw),
            lambda x, d: (_moved(O, x[0], d), _moved(O, x[1], d, 6 * nc)), (cams, tags), step, inner_tol)
        return cams, tags, cost, r, J, it

    cams, tags, cost, r, J, it = pose_lm(k, np.array(cams0, np.float64), np.array(tags0, np.float64))
    log = [(True, it, cost)]
    lam = 1e-4
    for _ in range(max_outer):
        if lam > 1e12:
            break
        _, _, rk, Sk = reduced_system(r, J, n6)
        dk = scaled_step(Sk, rk, lam)
        cc, ct, c2, r2, J2, it = pose_lm(k + dk, cams, tags)
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
    return free_inverse(H, keep)[n_pose6:, n_pose6:]


# ---- the per-pose blocks of the bundle adjustment ---------------------------------------------------------------------

def flags(n, idx):
    f = np.zeros(n, np.uint8)
    f[list(idx)] = 1
    return f


def const_sets(s, n_tag_const, n_cam_const):
    """Constant flags that contain observation 0's camera and tag: one observation between two constant poses."""
    tags = [int(s.obs_tag[0])] + [t for t in range(len(s.tag_gt)) if t != s.obs_tag[0]][:n_tag_const - 1]
    cams = ([int(s.obs_cam[0])] + [c for c in range(len(s.cam_gt)) if c != s.obs_cam[0]][:n_cam_const - 1]
            if n_cam_const else [])
    return flags(len(s.cam_gt), cams), flags(len(s.tag_gt), tags)


def pose_blocks(O, s, cam, tag, robust, fixed_tag=-1, cam_const=None, tag_const=None):
    """V, U, W, g_cam, g_tag, cost from the oracle's per-observation residuals and Jacobians (rows scaled by sqrt(rho'),
    numpy accumulation in the caller's order); the blocks of the fixed tag and of the constant poses are zero."""
    n_c, n_t = len(cam), len(tag)
    V, U = np.zeros((n_c, 6, 6)), np.zeros((n_t, 6, 6))
    W = np.zeros((len(s.obs_cam), 6, 6))
    gc, gt = np.zeros((n_c, 6)), np.zeros((n_t, 6))
    cost = 0.0
    for i, (c, t) in enumerate(zip(s.obs_cam, s.obs_tag)):
        r, Jc, Jt = O.obs_eval(s.intr, s.dist, cam[c], tag[t], s.tag_wh[t], s.obs_px[i])
        loss = corner_loss(O, r, robust, by_squares=True)
        for rho, _ in loss:
            cost += 0.5 * rho
        w = np.repeat(np.sqrt([d for _, d in loss]), 2)
        Jc, Jt, r = w[:, None] * Jc, w[:, None] * Jt, w * r
        V[c] += Jc.T @ Jc
        U[t] += Jt.T @ Jt
        W[i] = Jc.T @ Jt
        gc[c] += Jc.T @ r
        gt[t] += Jt.T @ r
    cc = np.zeros(n_c, bool) if cam_const is None else np.asarray(cam_const, bool)
    tc = np.zeros(n_t, bool) if tag_const is None else np.asarray(tag_const, bool).copy()
    if fixed_tag >= 0:
        tc[fixed_tag] = True
    V[cc] = 0.0
    gc[cc] = 0.0
    U[tc] = 0.0
    gt[tc] = 0.0
    W[cc[s.obs_cam] | tc[s.obs_tag]] = 0.0
    return dict(V=V, U=U, W=W, g_cam=gc, g_tag=gt, cost=cost)


def free_system(s, blk, cam_const, tag_const):
    """Dense H and g over the free poses (cameras first, then tags) from the blocks; index of every free pose."""
    fc = np.flatnonzero(~np.asarray(cam_const, bool))
    ft = np.flatnonzero(~np.asarray(tag_const, bool))
    pos_c = {int(c): k for k, c in enumerate(fc)}
    pos_t = {int(t): len(fc) + k for k, t in enumerate(ft)}
    n = 6 * (len(fc) + len(ft))
    H, g = np.zeros((n, n)), np.zeros(n)
    for c, k in pos_c.items():
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = blk["V"][c]
        g[6 * k:6 * k + 6] = blk["g_cam"][c]
    for t, k in pos_t.items():
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = blk["U"][t]
        g[6 * k:6 * k + 6] = blk["g_tag"][t]
    for i, (c, t) in enumerate(zip(s.obs_cam.tolist(), s.obs_tag.tolist())):
        if c in pos_c and t in pos_t:
            a, b = pos_c[c], pos_t[t]
            H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += blk["W"][i]
            H[6 * b:6 * b + 6, 6 * a:6 * a + 6] += blk["W"][i].T
    return H, g, fc, ft


def gauss_newton(O, s, cam, tag, cam_const, tag_const, max_iter=25):
    """Undamped dense Gauss-Newton on the plain cost over the free poses, from (cam, tag), until |step|_inf < 1e-12."""
    cam, tag = cam.copy(), tag.copy()
    step = np.inf
    for it in range(max_iter):
        blk = pose_blocks(O, s, cam, tag, False, cam_const=cam_const, tag_const=tag_const)
        H, g, fc, ft = free_system(s, blk, cam_const, tag_const)
        d = np.linalg.solve(H, -g)
        step = float(np.abs(d).max())
        for k, c in enumerate(fc):
            cam[c] = O.pose_plus(cam[c], d[6 * k:6 * k + 6])
        for k, t in enumerate(ft):
            tag[t] = O.pose_plus(tag[t], d[6 * (len(fc) + k):6 * (len(fc) + k) + 6])
        if step < 1e-12:
            break
    return cam, tag, step, it + 1


def gradient_max_norm(O, blk, cam, tag, cam_const, tag_const):
    """Ceres' gradient max-norm |Plus(x, -g) - x|_inf over the free poses."""
    gm = 0.0
    for x, g, const in ((cam, blk["g_cam"], cam_const), (tag, blk["g_tag"], tag_const)):
        for p in np.flatnonzero(~np.asarray(const, bool)):
            gm = max(gm, float(np.abs(O.pose_plus(x[p], -g[p]) - x[p]).max()))
    return gm


# ---- comparisons shared by the GPU tests ------------------------------------------------------------------------------

def same_bytes(a, b):
    """Two results of intrinsics_system, bit for bit."""
    return all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in ("cost", "g_k", "C", "r_k", "S_k"))


def assert_same_solution(cam, tag, sc, wh):
    """The device's poses and world corners against the oracle scene sc after its solve, REL of the largest entry."""
    scale = max(np.abs(sc.cam_qt).max(), np.abs(sc.tag_qt).max())
    np.testing.assert_allclose(cam, sc.cam_qt, rtol=0, atol=REL * scale)
    np.testing.assert_allclose(tag, sc.tag_qt, rtol=0, atol=REL * scale)
    a, b = rg.world_corners(tag, wh, np.float64), rg.world_corners(sc.tag_qt, wh, np.float64)
    np.testing.assert_allclose(a, b, rtol=0, atol=REL * np.abs(b).max())


def assert_same_trace(out, summ, trace, rtol=1e-7):
    """The device's solve summary and iteration trace against the oracle's."""
    assert out["termination_type"] == summ["termination_type"]
    assert out["iterations"] == summ["iterations"]
    assert out["num_successful_steps"] == summ["num_successful_steps"]
    assert out["num_unsuccessful_steps"] == summ["num_unsuccessful_steps"]
    for a, b in zip(out["trace"], trace):
        assert a["iteration"] == b["iteration"]
        assert a["step_is_successful"] == b["step_is_successful"]
        np.testing.assert_allclose(a["cost"], b["cost"], rtol=rtol)
        np.testing.assert_allclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-5)
    np.testing.assert_allclose(out["final_cost"], summ["final_cost"], rtol=rtol)
    np.testing.assert_allclose(out["initial_cost"], summ["initial_cost"], rtol=1e-12)
