"""The host yardstick of the tag-location tests (vmm_ba_locate_tags, TagReconstructor.checkMap): numpy around
oracle/oracle.py through tests/yardstick.py.  It never imports the code under test.

tag_rows gives block_normal's rows of one tag over its own tangent (the third return of O.obs_eval), tag_optimum runs
yardstick.dense_lm on them as image_optimum does for a camera, tag_propagated is the first-order propagation of the
cameras' covariances and map_check_statistic the map check's delta, Sigma and d2.
"""
import numpy as np

import yardstick as ys


def by_tag(s):
    """The scene's observations grouped by tag with a stable sort: (tag_start (n_tags + 1, int64), order)."""
    start = np.zeros(len(s.tag_gt) + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(s.obs_tag, minlength=len(s.tag_gt)))
    return start, np.argsort(s.obs_tag, kind="stable")


def tag_rows(O, intr, dist, q_tag, cam_qt, wh, cams, pxs):
    """block_normal's rows of one tag at pose q_tag: (r2, Jt 2 x 6) per corner of every observation."""
    for c, px in zip(cams, pxs):
        r, _, Jt = O.obs_eval(intr, dist, cam_qt[c], q_tag, wh, px)
        for k in range(4):
            yield r[2 * k:2 * k + 2], Jt[2 * k:2 * k + 2]


def tag_optimum(O, intr, dist, q0, cam_qt, wh, cams, pxs, robust, a=1.0):
    """The pose of one tag seen by the cameras cam_qt from q0, run until the step is at the rounding floor of the pose.
    Returns (pose, cost, the largest scaled gradient entry there)."""
    q, cost, (_, A, g), _ = ys.dense_lm(
        lambda q: ys.block_normal(O, tag_rows(O, intr, dist, q, cam_qt, wh, cams, pxs), robust, a),
        O.pose_plus, np.array(q0, np.float64), lambda sys, lam: ys.plain_step(sys[1], sys[2], lam), 1e-13)
    return q, cost, float(np.abs(g / np.sqrt(np.maximum(np.diag(A), 1e-300))).max())


def tag_normal(O, intr, dist, q_tag, cam_qt, wh, cams, pxs, robust, a=1.0):
    """H = sum rho' Jt^T Jt of one tag at q_tag."""
    return ys.block_normal(O, tag_rows(O, intr, dist, q_tag, cam_qt, wh, cams, pxs), robust, a)[1]


def tag_propagated(O, intr, dist, q_tag, cam_qt, cam_cov, wh, cams, pxs, robust, a=1.0):
    """H^-1 (sum_i G_i C_i G_i^T) H^-1 with G_i = sum over observation i's four corners of rho' Jt^T Jc and
    C_i = cam_cov[cams[i]]: the cameras' own covariances propagated to the tag, camera by camera."""
    H, S = np.zeros((6, 6)), np.zeros((6, 6))
    for c, px in zip(cams, pxs):
        r, Jc, Jt = O.obs_eval(intr, dist, cam_qt[c], q_tag, wh, px)
        G = np.zeros((6, 6))
        for k, (_, d) in enumerate(ys.corner_loss(O, r, robust, a)):
            rows = slice(2 * k, 2 * k + 2)
            H += d * (Jt[rows].T @ Jt[rows])
            G += d * (Jt[rows].T @ Jc[rows])
        S += G @ cam_cov[c] @ G.T
    Hi = np.linalg.inv(H)
    return Hi @ S @ Hi


def pose_minus(O, a, b):
    """The tangent step d with O.pose_plus(b, d) == a: the translation's difference, and the axis times the half angle of
    q_a q_b^-1 found from the rotation matrices (an independent route from the code under test's quaternion product)."""
    R = ys.rotation(a) @ ys.rotation(b).T
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(axis), 0.5 * (np.trace(R) - 1.0)
    d = np.zeros(6)
    d[:3] = np.asarray(a, np.float64)[4:] - np.asarray(b, np.float64)[4:]
    if s > 0.0:
        d[3:] = axis / (2.0 * s) * (0.5 * np.arctan2(s, c))
    return d


def map_check_statistic(O, located, mapped, tag_cov, tag_cov_cams, sigma_px):
    """(delta, Sigma, d2) of the map check: delta = pose_minus(located, mapped), Sigma = sigma_px^2 (tag_cov +
    tag_cov_cams), d2 = delta^T Sigma^-1 delta."""
    delta = pose_minus(O, located, mapped)
    Sigma = sigma_px ** 2 * (np.asarray(tag_cov) + np.asarray(tag_cov_cams))
    return delta, Sigma, float(delta @ np.linalg.solve(Sigma, delta))
