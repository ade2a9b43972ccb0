"""The yardstick of the rig tests (tests/test_rig_cpu.py proves it, tests/test_gpu_rig.py leans on it) and the scenes
they share.

rig_system is tests/yardstick.py's assemble over rig_rows: obs_eval gives the 8 residuals and the 8 x 6 camera Jacobian
of one observation at the composed pose ext_c o rig_f; the chain rule carries the camera Jacobian to the two
tangents.  With camera = (R_c R_f, R_c t_f + t_c) and every pose moving as vmm_ba_pose_plus moves it (translation
added, rotation multiplied from the left by the half-angle step):
    a rig step (dt, dth) moves the camera by (R_c dt, R_c dth)                  J_rig = [Jc_t R_c | Jc_r R_c]
    an extrinsic step (ds, dph) moves it by (ds + 2 dph x (R_c t_f), dph)      J_ext = [Jc_t | Jc_r - 2 Jc_t [R_c t_f]x]
The composed pose is ref_geometry.compose_rig with the yardstick's norm; the column turn stays written out here, apart
from ref_geometry.turn_to_rig / extrinsic_columns, which the truths and references B use.  It never calls the code under test.
"""
import numpy as np

import ref_geometry as rg
from yardstick import assemble, dense_lm, free_inverse, plain_step, rotation

# rig->camera: identity; yaw 4 deg, t = (-0.3, 0, 0); yaw -15 deg, t = (0.2, 0.05, 0)
def yaw(deg, t=(0.0, 0.0, 0.0)):
    a = np.radians(deg) / 2
    return np.array([np.cos(a), 0.0, np.sin(a), 0.0, t[0], t[1], t[2]])


EXT3 = np.array([yaw(0.0), yaw(4.0, (-0.3, 0.0, 0.0)), yaw(-15.0, (0.2, 0.05, 0.0))])

# the three scenes whose every image keeps at least FLOOR tags under EXT3
SCENES = {
    "config1_20x10": (1, dict()),
    "distortion_12x8": (5, dict(n_cams=12, n_tags=8, visibility=1.0)),
    "closeup_12x30": (2, dict(n_cams=12, n_tags=30, neighbors_min=6, neighbors_max=10)),
}
FLOOR = 5


def rig_scene(name, ext=EXT3, **kw):
    """make_rig_scene on one of SCENES, with the visibility floor asserted on what the generator gave."""
    from visual_marker_mapping_amd.synthetic import make_rig_scene
    cfg, over = SCENES[name]
    s = make_rig_scene(cfg, ext, **dict(over, **kw))
    missing = {(int(f), int(c)) for f, c in kw.get("missing", ())}
    per_image = np.diff(s.img_start)
    for f in range(s.n_frames):
        for c in range(s.n_rig_cams):
            assert (f, c) in missing or per_image[f * s.n_rig_cams + c] >= FLOOR, (name, f, c)
    return s


def compose(ext, rig):
    """ext o rig as (qw, qx, qy, qz, tx, ty, tz): the Hamilton product of the unit quaternions, t = R_c t_f + t_c."""
    return rg.compose_rig(ext, rig, np.float64, norm="linalg")[0]


def rig_rows(O, intr, dist, ext, rig, tag_qt, wh, px):
    """One observation: residual (8,), Jacobian over the rig's tangent (8, 6) and over the extrinsic's (8, 6)."""
    r, Jc, _ = O.obs_eval(intr, dist, compose(ext, rig), tag_qt, wh, px)
    Rc = rotation(ext)
    J_rig = np.hstack([Jc[:, :3] @ Rc, Jc[:, 3:] @ Rc])
    J_ext = np.hstack([Jc[:, :3], Jc[:, 3:] - 2.0 * Jc[:, :3] @ rg.skew(Rc @ rig[4:])])
    return r, J_rig, J_ext


def rig_system(O, s, rig_qt, ext_qt, keep=None, robust=False, a=1.0):
    """The whole problem of scene s at (rig_qt, ext_qt) over the observations of `keep` (bool mask; None: all):
    yardstick.assemble's cost, residuals (8 n,) and Jacobian (8 n, 6 F + 6 K), the rig blocks first."""
    F, K = len(rig_qt), len(ext_qt)

    def rows():
        for o in (np.arange(len(s.obs_tag)) if keep is None else np.flatnonzero(keep)):
            f, c, t = int(s.obs_frame[o]), int(s.obs_cam[o]), int(s.obs_tag[o])
            r, Jr, Je = rig_rows(O, s.intr[c], s.dist[c], ext_qt[c], rig_qt[f], s.tag_gt[t], s.tag_wh[t], s.obs_px[o])
            yield r, [(6 * f, Jr), (6 * F + 6 * c, Je)]
    return assemble(O, 6 * F + 6 * K, rows(), robust, a)[:3]


def frame_normal(O, s, f, q, ext_qt, keep, robust, a=1.0):
    """cost, J^T J and J^T r of frame f at rig pose q over its observations in `keep`."""
    mine = (s.obs_frame == f) & keep
    rig = np.array(s.rig_gt, np.float64)
    rig[f] = q
    cost, r, J = rig_system(O, s, rig, ext_qt, mine, robust, a)
    Jf = J[:, 6 * f:6 * f + 6]
    return cost, Jf.T @ Jf, Jf.T @ r


def host_frame_optimum(O, s, f, q0, ext_qt, keep, robust, a=1.0):
    """Levenberg-Marquardt on frame f's 6 degrees of freedom from q0 over the observations of `keep` (Huber width a), run
    until the step is at the rounding floor of the pose.  Returns (pose, cost)."""
    return dense_lm(lambda q: frame_normal(O, s, f, q, ext_qt, keep, robust, a), O.pose_plus, np.array(q0, np.float64),
                    lambda sys, lam: plain_step(sys[1], sys[2], lam), 1e-13)[:2]


def select(s, keep):
    """Scene s with only the observations of `keep` (bool mask), the CSR rebuilt."""
    from visual_marker_mapping_amd.synthetic import SyntheticScene
    K = s.n_rig_cams
    slot = s.obs_frame[keep].astype(np.int64) * K + s.obs_cam[keep]
    start = np.zeros(s.n_frames * K + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(slot, minlength=s.n_frames * K))
    d = dict(s.__dict__)
    d.update(img_start=start, obs_tag=s.obs_tag[keep], obs_px=s.obs_px[keep], obs_frame=s.obs_frame[keep],
             obs_cam=s.obs_cam[keep], outlier=s.outlier[keep])
    return SyntheticScene(**d)


def frames(s, which):
    """Scene s reduced to the frames `which`, in that order (frame numbers renumbered)."""
    from visual_marker_mapping_amd.synthetic import SyntheticScene
    K = s.n_rig_cams
    idx = np.concatenate([np.arange(s.img_start[f * K], s.img_start[f * K + K]) for f in which] + [np.zeros(0, np.int64)])
    idx = idx.astype(np.int64)
    counts = np.concatenate([np.diff(s.img_start[f * K:f * K + K + 1]) for f in which])
    start = np.zeros(len(which) * K + 1, np.int64)
    start[1:] = np.cumsum(counts)
    d = dict(s.__dict__)
    d.update(img_start=start, obs_tag=s.obs_tag[idx], obs_px=s.obs_px[idx], obs_cam=s.obs_cam[idx], outlier=s.outlier[idx],
             obs_frame=np.repeat(np.arange(len(which), dtype=np.int32), [int(s.img_start[f * K + K] - s.img_start[f * K])
                                                                         for f in which]),
             rig_gt=s.rig_gt[list(which)], n_frames=len(which))
    return SyntheticScene(**d)


def free_columns(s, keep, mask):
    """Which of the 6 F + 6 K columns move: every frame with an observation in `keep`, and the extrinsics of `mask` (bit
    c) whose camera has one."""
    F, K = s.n_frames, s.n_rig_cams
    free = np.zeros(6 * F + 6 * K, bool)
    for f in set(int(v) for v in s.obs_frame[keep]):
        free[6 * f:6 * f + 6] = True
    for c in set(int(v) for v in s.obs_cam[keep]):
        if (mask >> c) & 1:
            free[6 * F + 6 * c:6 * F + 6 * c + 6] = True
    return free


def host_rig_calibration(O, s, rig0, ext0, keep, robust, mask, a=1.0):
    """Levenberg-Marquardt on all the free rig poses and extrinsics at once (dense normal equations of rig_system, every
    block moved by the oracle's Plus) from (rig0, ext0), run until the step is at the rounding floor.  Returns (rig, ext,
    cost, H): H the undamped normal matrix at the result, the loss applied."""
    F = s.n_frames
    free = free_columns(s, keep, mask)

    def system(x):
        cost, r, J = rig_system(O, s, x[0], x[1], keep, robust, a)
        return cost, J.T @ J, J.T @ r

    def step(sys, lam):
        d = np.zeros(len(free))
        d[free] = plain_step(sys[1][np.ix_(free, free)], sys[2][free], lam)
        return d

    def plus(x, d):
        poses = np.concatenate(x)
        return np.split(np.array([O.pose_plus(p, d[6 * n:6 * n + 6]) if free[6 * n] else p for n, p in enumerate(poses)]), [F])

    (rig, ext), cost, (_, H, _), _ = dense_lm(system, plus, (np.array(rig0, np.float64), np.array(ext0, np.float64)), step,
                                             1e-13)
    return rig, ext, cost, H


def joint_covariance(s, H, keep, mask):
    """(ext_cov (6 K, 6 K), rig_cov (F, 6, 6), max |entry| of the joint inverse) from the normal matrix H: the inverse
    over the free columns, zero rows and columns for the others."""
    F = s.n_frames
    full = free_inverse(H, free_columns(s, keep, mask))
    rig_cov = np.array([full[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(F)])
    return full[6 * F:, 6 * F:], rig_cov, float(np.abs(full).max())
