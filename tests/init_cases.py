"""Scenes, longdouble truth, float64 references and the host restatement for the accuracy tests of the one-shot map
initialisation (test_init_cases_cpu.py, test_gpu_init_accuracy.py, tools/init_accuracy.py): vmm_ba_quad_poses and
vmm_ba_initialize, that is k_quad_pose, k_init_score, k_init_refine, k_init_begin and k_init_stats (kernels_init.hip over
pose_lm.hpp and small_solve.hpp).  numpy only: nothing here calls the engine, and there are no tests in here.

Input.  Every stage of the recipe is observable through the call's own options: refine_iterations = 0 with sweeps = 0
returns the pure selection, refine_iterations = 1 one Levenberg-Marquardt trial, constant poses turn a pass into one round
with known counterparts.  A test reads the device's state bit for bit and forms the truth there in np.longdouble.

Truth (geometry and conventions: ref_geometry.py; B's algebra and summation orders: ref_algebra.py).  project_cm is
CameraModel::projectPoint (ref_geometry.distort's aliased term 2 p2 (xd - x) y included), which k_quad_pose fits;
eval_cases.corner_chain is the functor's projection, which scoring, refinement and the report use.  Candidates are
ref_geometry.quat_from_R(chain(quad pose, counterpart)); a score is sum min(e^2, cap^2) over the usable observations' corners; one trial
is -(H + lam diag max(H_jj, 1e-12))^-1 g at lam = kLamInit through cov_cases.refined_inverse and the longdouble pose_plus.

References.  A: the oracle's functor through yardstick (image_rows / tag_rows, block_normal, plain_step), for the planar
solver pnp.project (with the aliased term added where p2 != 0: pnp.project is OpenCV's model by design).  B: the device's
scheme in numpy with the same expressions in the same order.  The bound of a case and quantity is MARGIN (8) x the larger
deviation of A and B over all items of the case -- never a figure the kernels produced.
"""
import numpy as np

import cov_cases as cc
import eval_cases as ec
import finished_map_cases as fm
import ref_algebra as ra
import ref_geometry as rg
import tag_cases as tc
import yardstick as ys
from ref_geometry import quat_from_R

LD = ec.LD
MARGIN = ec.MARGIN
COST_GAP = fm.COST_GAP
SCORE_GAP = 1e-9          # relative: a pose whose two best scores lie closer is left out of the argmin comparison
WINNER_MARGIN = 1e-6      # relative: what a placed winner must win by
LAM_INIT = 1e-3           # kLamInit, small_solve.hpp
QUAD_TRIALS = 60          # kQuadTrials
REFINE_TRIALS = 30        # the default refine_iterations
SCORE_CAP_PX = 40.0       # below the smallest placed outlier (10 x inlier_px = 80 px): an outlier's corners add cap^2
TIE_CAP_PX = 1e-6         # every corner of a noisy scene lies further out: all scores have the same bits
NOISE_PX = fm.NOISE_PX
INF = np.inf
IDENTITY_CAM = np.array([1.0, 0, 0, 0, 0, 0, 1.0])   # the pose a degenerate quad reports, and the cameras' placeholder
IDENTITY_TAG = np.array([1.0, 0, 0, 0, 0, 0, 0.0])
QUAD_SIZES = (1, 63, 64, 65, 129)
SELECT_COUNTS = (1, 2, 32, 33, 63, 64, 65, 511, 512, 513)
# list position of the observation with exact pixels in a list of that length: 0, 31, 32, 511, 512 and m - 1
WINNER_AT = {1: 0, 2: 1, 32: 31, 33: 32, 63: 62, 64: 0, 65: 64, 511: 31, 512: 511, 513: 512}
TRIAL_COUNTS = (1, 63, 64, 65, 129, 513)
REPORT_COUNTS = (1, 255, 256, 257, 513)
FAMILIES = ("cam", "tag")


# ---- small geometry in a dtype of the caller's choice ---------------------------------------------------------------------

def _mat3(a, b, transpose_b=False):
    """a @ b (or a @ b^T) for stacks of 3 x 3, the three products of an entry added from left to right."""
    if transpose_b:
        b = np.swapaxes(b, -1, -2)
    return a[..., :, 0, None] * b[..., None, 0, :] + a[..., :, 1, None] * b[..., None, 1, :] + a[..., :, 2, None] * b[..., None, 2, :]


def _matvec(a, v):
    return a[..., :, 0] * v[..., None, 0] + a[..., :, 1] * v[..., None, 1] + a[..., :, 2] * v[..., None, 2]


def chain(fam, rel_qt, oth_qt, dtype=LD):
    """chain_camera (fam "cam": T_cam = T_rel o T_tag^-1) or chain_tag (T_tag = T_cam^-1 o T_rel) for (n, 7) each.
    Returns (R (n, 3, 3), t (n, 3))."""
    rel_qt, oth_qt = np.asarray(rel_qt, dtype).reshape(-1, 7), np.asarray(oth_qt, dtype).reshape(-1, 7)
    Rr, Ro = rg.rotation(rel_qt, dtype), rg.rotation(oth_qt, dtype)
    if fam == "cam":
        R = _mat3(Rr, Ro, transpose_b=True)
        return R, rel_qt[:, 4:] - _matvec(R, oth_qt[:, 4:])
    RoT = np.swapaxes(Ro, -1, -2)
    return _mat3(RoT, Rr), _matvec(RoT, rel_qt[:, 4:] - oth_qt[:, 4:])


def chained_pose(fam, rel_qt, oth_qt, dtype=LD):
    """(n, 7): quat_from_R of the chain and its translation, the quaternion normalised once more as k_init_refine does
    before it stores a pose."""
    R, t = chain(fam, rel_qt, oth_qt, dtype)
    q, _ = quat_from_R(R, dtype)
    q = q * (dtype(1) / np.sqrt((q * q).sum(axis=1, keepdims=True)))
    return np.concatenate([q, t], axis=1)


def chained_pose_a(fam, rel_qt, oth_qt):
    """Reference A of a chained pose: numpy's matrix products and pnp.quat_from_R, float64."""
    from visual_marker_mapping_amd import pnp
    out = []
    for rel, oth in zip(np.asarray(rel_qt, np.float64).reshape(-1, 7), np.asarray(oth_qt, np.float64).reshape(-1, 7)):
        Rr, Ro = ys.rotation(rel), ys.rotation(oth)
        if fam == "cam":
            R = Rr @ Ro.T
            t = rel[4:] - R @ oth[4:]
        else:
            R = Ro.T @ Rr
            t = Ro.T @ (rel[4:] - oth[4:])
        out.append(np.r_[pnp.quat_from_R(R), t])
    return np.array(out)


def pose_deviation(got, truth):
    """Per pose: max over the quaternion's components of |dq| and over the translation's of |dt| / max(|t|, 1).  The sign
    of the quaternion counts: quat_from_R fixes it."""
    got, truth = np.asarray(got, LD).reshape(-1, 7), np.asarray(truth, LD).reshape(-1, 7)
    dq = np.abs(got[:, :4] - truth[:, :4]).max(axis=1)
    dt = np.abs(got[:, 4:] - truth[:, 4:]).max(axis=1) / np.maximum(np.abs(truth[:, 4:]).max(axis=1), LD(1))
    return np.maximum(dq, dt).astype(np.float64)


# ---- CameraModel::projectPoint and the quad's sums ---------------------------------------------------------------------

def project_cm(intr, dist, pc, dtype=LD):
    """CameraModel::projectPoint of camera-frame points pc (..., 3): the functor's projection with the y tangential term
    formed from the already distorted x, yd = y rad + 2 p2 xd y + p1 (r2 + 2 y^2) = functor + 2 p2 (xd - x) y."""
    intr, dist, pc = np.asarray(intr, dtype), np.asarray(dist, dtype), np.asarray(pc, dtype)
    iz = dtype(1) / pc[..., 2]
    xd, yd, _, _ = rg.distort(pc[..., 0] * iz, pc[..., 1] * iz, dist, dtype, aliased=True)
    return rg.pixel(intr, xd, yd)


def chain_points(model):
    """The camera-frame points the CameraModel chain is checked on, on the CPU against pnp.project and on the GPU against
    engine.project_points: 400 seeded points from 0.15 m to 8 m out to the image's edge, and every corner of the quad
    batches at its true pose."""
    rng = np.random.default_rng(5)
    pc = np.c_[rng.uniform(-1.0, 1.0, 400), rng.uniform(-0.7, 0.7, 400), rng.uniform(0.15, 8.0, 400)]
    pc[:, :2] *= pc[:, 2:] / 3.0
    corners = [quad_points(quad_batch(model, n).qt_gt, quad_batch(model, n).wh, np.float64)[0].reshape(-1, 3) for n in QUAD_SIZES]
    return np.concatenate([pc] + corners)


def chain_deviation(got, truth, intr):
    """max |got - truth| per entry magnitude |f xd| + |c| (the two numbers a pixel coordinate is the sum of)."""
    mag = np.abs(np.asarray(truth, LD) - np.asarray(intr, LD)[2:]) + np.abs(np.asarray(intr, LD)[2:])
    return float((np.abs(np.asarray(got, LD) - truth) / mag).max())


def project_cm_a(intr, dist, pc):
    """Reference A of project_cm: pnp.project, and where p2 != 0 the aliased term added to its v."""
    from visual_marker_mapping_amd import pnp
    pc = np.asarray(pc, np.float64).reshape(-1, 3)
    uv = pnp.project(pc, np.eye(3), np.zeros(3), tuple(intr), tuple(dist))
    p2 = dist[3]
    if p2 != 0.0:
        x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        uv[:, 1] += intr[1] * (2.0 * p2 * (rg.distort(x, y, dist, np.float64)[0] - x) * y)
    return uv


def quad_points(qt, wh, dtype=LD):
    """(n, 4, 3): the quad's corners (LL, LR, UR, UL) under the tag->camera poses qt, and the rotated corners b = R X."""
    qt, wh = np.asarray(qt, dtype).reshape(-1, 7), np.asarray(wh, dtype).reshape(-1, 2)
    R = rg.rotation(qt, dtype)
    X = rg.local_corners(wh, dtype)
    b = R[:, None, :, 0] * X[:, :, 0, None] + R[:, None, :, 1] * X[:, :, 1, None]    # z = 0: two columns of R
    return b + qt[:, None, 4:], b


def quad_residuals(intr, dist, qt, wh, px, dtype=LD):
    """(n, 4, 2) pixel residuals of the quads under qt, by CameraModel::projectPoint."""
    pc, _ = quad_points(qt, wh, dtype)
    return project_cm(intr, dist, pc, dtype) - np.asarray(px, dtype).reshape(-1, 4, 2)


def quad_cost(intr, dist, qt, wh, px, dtype=LD):
    r = quad_residuals(intr, dist, qt, wh, px, dtype)
    return (r * r).sum(axis=(1, 2))


def quad_rms(intr, dist, qt, wh, px, dtype=LD):
    """The RMS corner distance k_quad_pose reports: sqrt(cost / 4)."""
    return np.sqrt(quad_cost(intr, dist, qt, wh, px, dtype) / dtype(4))


def quad_rms_a(intr, dist, qt, wh, px):
    """Reference A of the quad's RMS: pnp.project as test_gpu_init.py uses it, float64."""
    qt, wh, px = np.asarray(qt, np.float64).reshape(-1, 7), np.asarray(wh).reshape(-1, 2), np.asarray(px).reshape(-1, 4, 2)
    out = np.zeros(len(qt))
    for i in range(len(qt)):
        pc = rg.local_corners(wh[i], np.float64)[0] @ ys.rotation(qt[i]).T + qt[i, 4:]
        e = project_cm_a(intr, dist, pc) - px[i]
        out[i] = np.sqrt((e ** 2).sum(axis=1).mean())
    return out


def quad_sums(intr, dist, qt, wh, px):
    """quad_cost<true> in float64 with project_camera_point<true, true>'s expressions: cost (n,), J^T J (n, 6, 6) and
    J^T r (n, 6), the four corners added in order."""
    intr, dist = np.asarray(intr, np.float64), np.asarray(dist, np.float64)
    fx, fy, cx, cy = intr
    k1, k2, p1, p2, k3 = dist
    qt = np.asarray(qt, np.float64).reshape(-1, 7)
    pc, b = quad_points(qt, wh, np.float64)
    px = np.asarray(px, np.float64).reshape(-1, 4, 2)
    iz = 1.0 / pc[..., 2]
    x, y = pc[..., 0] * iz, pc[..., 1] * iz
    xd, yd, r2, rad = rg.distort(x, y, dist, np.float64, aliased=True)
    ru, rv = fx * xd + cx - px[..., 0], fy * yd + cy - px[..., 1]
    dr = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2)
    D00 = rad + 2.0 * x * x * dr + 2.0 * p1 * y + 6.0 * p2 * x
    D01 = 2.0 * x * y * dr + 2.0 * p1 * x + 2.0 * p2 * y
    D11 = rad + 2.0 * y * y * dr + 2.0 * p2 * x + 6.0 * p1 * y
    D10 = D01 + 2.0 * p2 * y * (D00 - 1.0)
    D11 = D11 + 2.0 * p2 * (xd - x) + 2.0 * p2 * y * D01
    g = np.stack([np.stack([fx * D00 * iz, fx * D01 * iz, -fx * (D00 * x + D01 * y) * iz], axis=-1),
                  np.stack([fy * D10 * iz, fy * D11 * iz, -fy * (D10 * x + D11 * y) * iz], axis=-1)], axis=-2)   # (n, 4, 2, 3)
    bb = b[:, :, None, :]
    J = np.concatenate([g, 2.0 * np.stack([bb[..., 1] * g[..., 2] - bb[..., 2] * g[..., 1],
                                           bb[..., 2] * g[..., 0] - bb[..., 0] * g[..., 2],
                                           bb[..., 0] * g[..., 1] - bb[..., 1] * g[..., 0]], axis=-1)], axis=-1)   # (n, 4, 2, 6)
    cost, A, gr = np.zeros(len(qt)), np.zeros((len(qt), 6, 6)), np.zeros((len(qt), 6))
    for k in range(4):
        cost = cost + (ru[:, k] * ru[:, k] + rv[:, k] * rv[:, k])
        A = A + (J[:, k, 0, :, None] * J[:, k, 0, None, :] + J[:, k, 1, :, None] * J[:, k, 1, None, :])
        gr = gr + (J[:, k, 0] * ru[:, k, None] + J[:, k, 1] * rv[:, k, None])
    return cost, A, gr


# ---- small_solve.hpp's trial loop in numpy ------------------------------------------------------------------------------

def damped_step(A, g, lam):
    """(A + lam diag(max(A_ii, 1e-12))) step = -g for stacks; (step, ok): ok is damped_solve's verdict (positive
    definite, finite)."""
    A, g = np.asarray(A, np.float64), np.asarray(g, np.float64)
    n = A.shape[-1]
    D = A.copy()
    d = np.einsum("bii->bi", A)
    D[:, np.arange(n), np.arange(n)] = d + np.asarray(lam)[:, None] * np.maximum(d, 1e-12)
    fin = np.isfinite(D).all(axis=(1, 2)) & np.isfinite(g).all(axis=1)
    D[~fin] = np.eye(n)
    ok = fin & (np.linalg.eigvalsh(D).min(axis=1) > 0)
    D[~ok] = np.eye(n)
    step = np.linalg.solve(D, -np.where(ok[:, None], g, 0.0)[..., None])[..., 0]
    return step, ok & np.isfinite(step).all(axis=1)


def lm_model(sums, x0, max_trials, stop_small):
    """lm_trials<6, 7, ., STOP_SMALL> for a batch of independent poses x0 (n, 7).  sums(x (b, 7), index (b,)) gives cost (b,),
    A (b, 6, 6), g (b, 6) of the poses `index`.  Returns (x, cost, trials spent, why): why is "spent" where the trials ran
    out and otherwise the rule that stopped the loop ("lambda", "tiny", "small", "floor")."""
    x = np.array(x0, np.float64).reshape(-1, 7)
    n = len(x)
    lam = np.full(n, LAM_INIT)
    cost, A, g = sums(x, np.arange(n))
    live, why, spent = np.ones(n, bool), np.full(n, "spent", object), np.zeros(n, int)

    def stop(idx, reason):
        why[idx] = reason
        live[idx] = False

    for it in range(max_trials):
        stop(live & (~np.isfinite(cost) | (lam > 1e12)), "lambda")
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        spent[idx] = it + 1
        step, ok = damped_step(A[idx], g[idx], lam[idx])
        lam[idx[~ok]] *= 10.0
        idx, step = idx[ok], step[ok]
        sm = np.abs(step).max(axis=1) if len(idx) else np.zeros(0)
        stop(idx[sm < 1e-14], "tiny")
        idx, step, sm = idx[sm >= 1e-14], step[sm >= 1e-14], sm[sm >= 1e-14]
        if not len(idx):
            continue
        cand = rg.pose_plus(x[idx], step)
        cc_, _, _ = sums(cand, idx)
        acc = np.isfinite(cc_) & (cc_ < cost[idx])
        rej = idx[~acc]
        at_floor = (sm[~acc] < 1e-10) | (cc_[~acc] - cost[rej] <= 1e-10 * cost[rej] + 1e-20)
        stop(rej[at_floor], "floor")
        lam[rej[~at_floor]] *= 10.0
        a = idx[acc]
        x[a] = cand[acc]
        lam[a] = np.maximum(lam[a] * 0.1, 1e-12)
        if stop_small:
            stop(a[sm[acc] < 1e-9], "small")
            a = a[sm[acc] >= 1e-9]
        if len(a):
            cost[a], A[a], g[a] = sums(x[a], a)
    return x, cost, spent, why


# ---- the planar solver restated on the host -----------------------------------------------------------------------------

def quad_homography(intr, dist, wh, px):
    """k_quad_pose's homography in float64: undistortion, the unit square -> image quad in closed form, the change of
    variables to the tag's metric frame.  Columns h1, h2, h3 (n, 3) each; a degenerate quad gives non-finite numbers."""
    fx, fy, cx, cy = np.asarray(intr, np.float64)
    k1, k2, p1, p2, k3 = np.asarray(dist, np.float64)
    wh, px = np.asarray(wh, np.float64).reshape(-1, 2), np.asarray(px, np.float64).reshape(-1, 4, 2)
    hw, hh = 0.5 * wh[:, 0], 0.5 * wh[:, 1]
    with np.errstate(all="ignore"):
        x0, y0 = (px[..., 0] - cx) / fx, (px[..., 1] - cy) / fy
        x, y = x0.copy(), y0.copy()
        for _ in range(20):
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dx) / rad, (y0 - dy) / rad
        dx1, dx2, sx = x[:, 1] - x[:, 2], x[:, 3] - x[:, 2], x[:, 0] - x[:, 1] + x[:, 2] - x[:, 3]
        dy1, dy2, sy = y[:, 1] - y[:, 2], y[:, 3] - y[:, 2], y[:, 0] - y[:, 1] + y[:, 2] - y[:, 3]
        den = dx1 * dy2 - dx2 * dy1
        hg, hh2 = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
        c0 = np.stack([x[:, 1] - x[:, 0] + hg * x[:, 1], y[:, 1] - y[:, 0] + hg * y[:, 1], hg], axis=1)
        c1 = np.stack([x[:, 3] - x[:, 0] + hh2 * x[:, 3], y[:, 3] - y[:, 0] + hh2 * y[:, 3], hh2], axis=1)
        c2 = np.stack([x[:, 0], y[:, 0], np.ones(len(x))], axis=1)
        return c0 / (2.0 * hw)[:, None], c1 / (2.0 * hh)[:, None], 0.5 * c0 + 0.5 * c1 + c2


def quad_start(intr, dist, wh, px):
    """k_quad_pose's closed-form start: the decomposition of the homography, the two unit columns made orthogonal
    symmetrically.  (n, 7) tag->camera poses."""
    with np.errstate(all="ignore"):
        h1, h2, h3 = quad_homography(intr, dist, wh, px)
        n1, n2 = np.sqrt((h1 * h1).sum(axis=1)), np.sqrt((h2 * h2).sum(axis=1))
        s = 2.0 / (n1 + n2)
        s = np.where(h3[:, 2] * s < 0.0, -s, s)
        sg = np.where(s < 0.0, -1.0, 1.0)
        r1, r2_ = h1 / n1[:, None] * sg[:, None], h2 / n2[:, None] * sg[:, None]
        cs, df = r1 + r2_, r1 - r2_
        nc, nd = 1.0 / np.sqrt(2.0 * (cs * cs).sum(axis=1)), 1.0 / np.sqrt(2.0 * (df * df).sum(axis=1))
        r1, r2_ = cs * nc[:, None] + df * nd[:, None], cs * nc[:, None] - df * nd[:, None]
        r3 = np.cross(r1, r2_)
        R = np.stack([r1, r2_, r3], axis=2)
        q, _ = quat_from_R(R, np.float64)
        return np.concatenate([q, h3 * s[:, None]], axis=1)


def quad_weak_starts(intr, dist, wh, px):
    """k_quad_pose's fallback starts, (n, 2, 7): the two planar poses the homography's first order at the tag centre
    allows.  With the camera turned so that the line of sight to the centre is its axis (Q), the 2 x 2 Jacobian of the
    image point over the tag's coordinates is the upper left block of the rotation over the distance: its larger singular
    value gives the distance, the unit length of the two columns gives |r1z| and |r2z|, their orthogonality the sign of
    r1z r2z, and the sign of r1z is the planar ambiguity itself."""
    with np.errstate(all="ignore"):
        h1, h2, h3 = quad_homography(intr, dist, wh, px)
        p0 = h3[:, :2] / h3[:, 2:]
        j1 = (h1[:, :2] - p0 * h1[:, 2:]) / h3[:, 2:]
        j2 = (h2[:, :2] - p0 * h2[:, 2:]) / h3[:, 2:]
        m = np.sqrt(p0[:, 0] * p0[:, 0] + p0[:, 1] * p0[:, 1] + 1.0)
        v = np.stack([p0[:, 0] / m, p0[:, 1] / m, 1.0 / m], axis=1)
        kx, ky, f = v[:, 1], -v[:, 0], 1.0 / (1.0 + v[:, 2])           # Q = I + [k]x + [k]x^2 / (1 + v_z), k = v x e_z
        Q = np.zeros((len(m), 3, 3))
        Q[:, 0, 0], Q[:, 0, 1], Q[:, 0, 2] = 1.0 - f * ky * ky, f * kx * ky, ky
        Q[:, 1, 0], Q[:, 1, 1], Q[:, 1, 2] = f * kx * ky, 1.0 - f * kx * kx, -kx
        Q[:, 2, 0], Q[:, 2, 1], Q[:, 2, 2] = -ky, kx, 1.0 - f * (kx * kx + ky * ky)
        a1 = np.stack([Q[:, 0, 0] * j1[:, 0] + Q[:, 0, 1] * j1[:, 1], Q[:, 1, 0] * j1[:, 0] + Q[:, 1, 1] * j1[:, 1]], axis=1) / m[:, None]
        a2 = np.stack([Q[:, 0, 0] * j2[:, 0] + Q[:, 0, 1] * j2[:, 1], Q[:, 1, 0] * j2[:, 0] + Q[:, 1, 1] * j2[:, 1]], axis=1) / m[:, None]
        # larger eigenvalue of A A^T, A = [a1 a2]
        sxx, syy, sxy = a1[:, 0] * a1[:, 0] + a2[:, 0] * a2[:, 0], a1[:, 1] * a1[:, 1] + a2[:, 1] * a2[:, 1], a1[:, 0] * a1[:, 1] + a2[:, 0] * a2[:, 1]
        lam = 0.5 * (sxx + syy) + np.sqrt(0.25 * (sxx - syy) * (sxx - syy) + sxy * sxy)
        dist_c = 1.0 / np.sqrt(lam)
        b1, b2 = a1 * dist_c[:, None], a2 * dist_c[:, None]
        z1 = np.sqrt(np.maximum(1.0 - (b1 * b1).sum(axis=1), 0.0))
        z2 = np.sqrt(np.maximum(1.0 - (b2 * b2).sum(axis=1), 0.0)) * np.where((b1 * b2).sum(axis=1) > 0.0, -1.0, 1.0)
        out = np.zeros((len(m), 2, 7))
        for k, sign in enumerate((1.0, -1.0)):
            r1 = np.concatenate([b1, (sign * z1)[:, None]], axis=1)
            r2 = np.concatenate([b2, (sign * z2)[:, None]], axis=1)
            Rp = np.stack([r1, r2, np.cross(r1, r2)], axis=2)
            R = _mat3(np.swapaxes(Q, -1, -2), Rp)
            q, _ = quat_from_R(R, np.float64)
            out[:, k, :4] = q
            out[:, k, 4:] = v * dist_c[:, None]
        return out


def quad_mirror(qt):
    """The second planar start: the tag normal mirrored about the line of sight to the tag centre (k_quad_pose)."""
    qt = np.asarray(qt, np.float64).reshape(-1, 7)
    R = rg.rotation(qt, np.float64)
    t = qt[:, 4:]
    v = t / np.sqrt((t * t).sum(axis=1, keepdims=True))
    nrm = R[:, :, 2]
    nv = (nrm * v).sum(axis=1, keepdims=True)
    m = 2.0 * nv * v - nrm
    ax = np.cross(nrm, m)
    sn = np.sqrt((ax * ax).sum(axis=1))
    c = (nrm * m).sum(axis=1)
    ch, sh = np.sqrt(np.maximum(0.5 * (1.0 + c), 0.0)), np.sqrt(np.maximum(0.5 * (1.0 - c), 0.0)) / np.where(sn > 1e-12, sn, 1.0)
    z = np.where((sn > 1e-12)[:, None], np.concatenate([ch[:, None], sh[:, None] * ax], axis=1), [[1.0, 0.0, 0.0, 0.0]])
    out = qt.copy()
    out[:, :4] = rg.qmul(z, qt[:, :4])
    return out


def host_quad(intr, dist, wh, px, max_trials=QUAD_TRIALS, fallback=True):
    """vmm_ba_quad_poses restated: (qt2 (n, 2, 7), rms2 (n, 2)), the lower RMS first, a degenerate quad +inf and
    IDENTITY_CAM.  max_trials above kQuadTrials runs each solution to its floor.  fallback: k_quad_pose's, for the
    solutions that spend all their trials; without it the restatement is the kernel before it had one."""
    wh, px = np.asarray(wh, np.float64).reshape(-1, 2), np.asarray(px, np.float64).reshape(-1, 8)
    n = len(px)
    qt2, rms2 = np.tile(IDENTITY_CAM, (n, 2, 1)), np.full((n, 2), INF)

    def sums(x, idx):
        with np.errstate(all="ignore"):
            return quad_sums(intr, dist, x, wh[idx], px[idx])

    with np.errstate(all="ignore"):
        q0, c0, _, why0 = lm_model(sums, quad_start(intr, dist, wh, px), max_trials, False)
        good = np.isfinite(q0).all(axis=1)
        start1 = np.where(good[:, None], q0, IDENTITY_CAM)
        q1, c1, _, why1 = lm_model(sums, quad_mirror(start1), max_trials, False)
        # the fallback: a solution that spent all its trials (its start sat at the saddle between the two planar minima)
        # is replaced by a weak-perspective start refined the same way, where that ends lower
        stalled = np.stack([why0 == "spent", why1 == "spent"], axis=1) & good[:, None]
        rows = np.flatnonzero(stalled.any(axis=1))
        if len(rows) and fallback:
            w = quad_weak_starts(intr, dist, wh[rows], px[rows])
            sub = lambda x, idx: sums(x, rows[idx])
            w0, d0, _, _ = lm_model(sub, np.where(np.isfinite(w[:, 0]).all(axis=1)[:, None], w[:, 0], IDENTITY_CAM), max_trials, False)
            w1, d1, _, _ = lm_model(sub, np.where(np.isfinite(w[:, 1]).all(axis=1)[:, None], w[:, 1], IDENTITY_CAM), max_trials, False)
            for i, r in enumerate(rows):
                ws, ds = (w0[i], w1[i]), (d0[i], d1[i])
                if stalled[r].all():
                    pick = (0, 1)
                else:
                    keep = q1[r] if stalled[r, 0] else q0[r]
                    nk = rg.rotation(keep, np.float64)[:, 2]
                    far = int((rg.rotation(ws[1], np.float64)[:, 2] @ nk) < (rg.rotation(ws[0], np.float64)[:, 2] @ nk))
                    pick = (far, far)
                for s_, (q, c) in enumerate(((q0, c0), (q1, c1))):
                    j = pick[s_]
                    if stalled[r, s_] and np.isfinite(ds[j]) and ds[j] < c[r]:
                        q[r], c[r] = ws[j], ds[j]
    for k, (q, c) in enumerate(((q0, c0), (q1, c1))):
        qn = q[:, :4] / np.sqrt((q[:, :4] * q[:, :4]).sum(axis=1, keepdims=True))
        full = np.concatenate([qn, q[:, 4:]], axis=1)
        ok = np.isfinite(c) & np.isfinite(full).all(axis=1) & good
        qt2[ok, k] = full[ok]
        rms2[ok, k] = np.sqrt(0.25 * c[ok])
    swap = rms2[:, 1] < rms2[:, 0]
    qt2[swap] = qt2[swap][:, ::-1]
    rms2[swap] = rms2[swap][:, ::-1]
    return qt2, rms2


def quad_optimum(intr, dist, qt, wh, px, max_trials=400):
    """The float64 optimum a Levenberg-Marquardt run from qt reaches at its floor, (n, 7), and the stopping rules."""
    wh, px = np.asarray(wh, np.float64).reshape(-1, 2), np.asarray(px, np.float64).reshape(-1, 8)
    x, _, _, why = lm_model(lambda x, idx: quad_sums(intr, dist, x, wh[idx], px[idx]), qt, max_trials, False)
    return x, why


# ---- batches for the planar solver ---------------------------------------------------------------------------------------

def _axis_quat(axis, deg):
    a = np.radians(deg) / 2
    return np.r_[np.cos(a), np.sin(a) * np.asarray(axis, np.float64) / np.linalg.norm(axis)]


def _flip():
    return np.array([0.0, 1.0, 0.0, 0.0])   # the tag faces the camera: its normal points at it


def _geometries(model):
    """The special tag->camera poses and sizes every batch holds: (name, q, t, wh).  `facing` rotates the tag about its
    own normal while it faces the camera (R = Rx(180) Rz(a)): the returned quaternions then come from all four branches
    of quat_from_R."""
    f = _flip()
    geo = [("frontal", rg.qmul(_axis_quat([1, 0.3, 0], 1.5), f), [0.1, -0.05, 3.0], [0.1285, 0.1285]),
           ("oblique 80", rg.qmul(_axis_quat([0, 1, 0], 80.0), f), [0.2, 0.1, 2.5], [0.1285, 0.1285]),
           ("19 px", rg.qmul(_axis_quat([1, 1, 0], 20.0), f), [0.4, -0.3, 8.0], [0.0188, 0.0188]),
           ("close-up", rg.qmul(_axis_quat([1, -1, 0], 15.0), f), [0.01, 0.02, 0.15], [0.1285, 0.1285]),
           ("corner", rg.qmul(_axis_quat([0, 1, 0.2], 25.0), f), [1.0, 0.68, 3.0], [0.1165, 0.0923]),
           ("w != h", rg.qmul(_axis_quat([1, 0, 0], 35.0), f), [-0.3, 0.2, 2.0], [0.21, 0.07])]
    # Facing the camera, in-plane rotations of 0, 90, 180, 270 degrees.  With the corners in detection order (the tag's
    # normal towards the camera, R = Rx(180) Rz(a), trace -1) only branches 1 and 2 of quat_from_R occur; the same four
    # rotations with the corners in mirrored order (the normal away from the camera, R = Rz(a), trace 1 + 2 cos a), which the
    # solver fits just as well, give branches 0 and 3.
    tilt = _axis_quat([0.3, 1, 0], 6.0)
    for a in (0, 90, 180, 270):
        geo.append(("facing %d" % a, rg.qmul(tilt, rg.qmul(f, _axis_quat([0, 0, 1], a + 7.0))), [0.05 * (a / 90), -0.1, 2.2],
                    [0.1285, 0.1285]))
    for a in (0, 90, 180, 270):
        geo.append(("mirrored %d" % a, rg.qmul(tilt, _axis_quat([0, 0, 1], a + 7.0)), [-0.1, 0.04 * (a / 90), 2.4],
                    [0.1165, 0.0923]))
    return geo


def special_positions(n):
    return sorted({p for p in (0, 63, 64, n - 1) if 0 <= p < n})


def quad_batch(model, n, noise_px=NOISE_PX, seed=20270101):
    """n observations, one lane each.  The special geometries stand at positions 0, 63, 64 and n - 1 (in rotation from
    batch to batch and from position to position) and fill the batch's front; ordinary tilted tags 2.5 .. 5 m away take the
    rest.  Scene fields: intr, dist, qt_gt (n, 7), wh (n, 2), px (n, 8), clean_px, names."""
    def make():
        rng = np.random.default_rng(seed + 1000 * fm.MODELS.index(model) + n)
        intr, dist = fm.camera_model(model)
        geo = _geometries(model)
        qt, wh, names = np.zeros((n, 7)), np.zeros((n, 2)), [""] * n
        for i in range(n):
            q = rg.qmul(rg.small_quat(rng, 0.25), _flip())
            qt[i] = np.r_[q / np.linalg.norm(q), rng.uniform(-0.8, 0.8), rng.uniform(-0.5, 0.5), rng.uniform(2.5, 5.0)]
            wh[i] = [0.1285, 0.1285] if rng.random() < 0.5 else [0.1165, 0.0923]
            names[i] = "ordinary"
        slots = special_positions(n) + [p for p in range(n) if p not in special_positions(n)]
        first = {1: 0, 63: 1, 64: 3, 65: 5, 129: 7}.get(n, 0)
        for k, p in enumerate(slots[:min(n, len(geo))]):
            name, q, t, w = geo[(first + k) % len(geo)]
            qt[p], wh[p], names[p] = np.r_[np.asarray(q) / np.linalg.norm(q), t], w, name
        pc, _ = quad_points(qt, wh, LD)
        assert (pc[..., 2] > 0).all()
        assert (fm.radial_slope(dist, pc) > 0).all(), "the radial map is not rising at a corner"
        assert n < len(geo) or set(branches_of(qt).tolist()) == {0, 1, 2, 3}, "a branch of quat_from_R does not occur"
        clean = project_cm(intr, dist, pc, LD).reshape(n, 8).astype(np.float64)
        px = clean + rng.normal(0, noise_px, clean.shape) if noise_px else clean.copy()
        return ec.Scene(model=model, intr=intr, dist=dist, qt_gt=qt, wh=wh, px=px, clean_px=clean, names=names)
    return ec.cached(("init quad", model, n, float(noise_px), seed), make)


def exact_batch(model):
    """16 exact observations over the special geometries (each once, six of them twice with another size)."""
    def make():
        intr, dist = fm.camera_model(model)
        geo = _geometries(model)
        rows = [(g[0], g[1], g[2], g[3]) for g in geo] + [(g[0] + " small", g[1], g[2], [0.6 * g[3][0], 0.8 * g[3][1]]) for g in geo[:6]]
        qt = np.array([np.r_[np.asarray(q) / np.linalg.norm(q), t] for _, q, t, _ in rows])
        wh = np.array([w for _, _, _, w in rows], np.float64)
        pc, _ = quad_points(qt, wh, LD)
        clean = project_cm(intr, dist, pc, LD).reshape(len(qt), 8).astype(np.float64)
        return ec.Scene(model=model, intr=intr, dist=dist, qt_gt=qt, wh=wh, px=clean, clean_px=clean, names=[r[0] for r in rows])
    return ec.cached(("init quad exact", model), make)


def branches_of(qt):
    """The branch of quat_from_R each pose's rotation takes."""
    return quat_from_R(rg.rotation(qt, np.float64), np.float64)[1]


DEGENERATE = {"coincident": [100.0, 100.0] * 4, "collinear": [100.0, 100.0, 200.0, 100.0, 300.0, 100.0, 400.0, 100.0]}


def recovery_error(qt, qt_gt):
    """Per pose: max |dR| and |dt| against the truth (test_gpu_init.py's measure), longdouble."""
    dR = np.abs(rg.rotation(qt, LD) - rg.rotation(qt_gt, LD)).max(axis=(1, 2))
    dt = np.abs(np.asarray(qt, LD)[:, 4:] - np.asarray(qt_gt, LD)[:, 4:]).max(axis=1)
    return np.maximum(dR, dt).astype(np.float64)


def exact_references(s):
    """The recovery errors two float64 solvers reach on the exact pixels of s: A pnp.solvePnP (the host implementation the
    incremental driver uses; OpenCV's model, so under distortion on the pixels without the aliased term), B host_quad."""
    from visual_marker_mapping_amd import pnp
    refs = {"B host_quad": recovery_error(host_quad(s.intr, s.dist, s.wh, s.px)[0][:, 0], s.qt_gt)}
    px = s.px.reshape(-1, 4, 2).copy()
    if s.dist[3] != 0.0:
        # pnp.solvePnP fits OpenCV's model: it gets the same poses' pixels without the aliased term (the term taken from the
        # longdouble chain at the true pose and rounded once)
        pc, _ = quad_points(s.qt_gt, s.wh, LD)
        x, y = pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2]
        xd = rg.distort(x, y, np.asarray(s.dist, LD), LD)[0]
        px[..., 1] = (px[..., 1].astype(LD) - LD(s.intr[1]) * LD(2) * LD(s.dist[3]) * (xd - x) * y).astype(np.float64)
    got = []
    for i in range(len(px)):
        R, t = pnp.solvePnP(rg.local_corners(s.wh[i], np.float64)[0], px[i], tuple(s.intr), tuple(s.dist))
        got.append(np.r_[pnp.quat_from_R(R), t])
    refs["A pnp.solvePnP"] = recovery_error(np.array(got), s.qt_gt)
    return refs


# ---- handles -------------------------------------------------------------------------------------------------------------

class Handle:
    """The arguments of engine.BundleAdjuster plus the constant flags and the mask; `own`: the family the scene is about.
    lists(fam) gives every pose's observation list in the device's order (a stable sort of the caller's order)."""

    def __init__(self, **kw):
        self.mask = None
        self.__dict__.update(kw)
        self.n_cams, self.n_tags, self.n_obs = len(self.cam_qt), len(self.tag_qt), len(self.obs_cam)
        if self.mask is None:
            self.mask = np.ones(self.n_obs, np.uint8)

    def copy(self, **kw):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()}
        d.update(kw)
        return Handle(**d)

    def const(self, fam):
        c = np.array(self.cam_const if fam == "cam" else self.tag_const, bool).copy()
        if fam == "tag" and self.fixed_tag >= 0:
            c[self.fixed_tag] = True
        return c

    def lists(self, fam):
        own = self.obs_cam if fam == "cam" else self.obs_tag
        order = np.argsort(own, kind="stable")
        n = self.n_cams if fam == "cam" else self.n_tags
        start = np.searchsorted(own[order], np.arange(n + 1))
        return [order[start[p]:start[p + 1]] for p in range(n)]

    def without(self, keep):
        """The handle built without the observations where keep is False (and without a mask)."""
        keep = np.asarray(keep, bool)
        return self.copy(obs_cam=self.obs_cam[keep], obs_tag=self.obs_tag[keep], obs_px=self.obs_px[keep], mask=None)


def open_handle(eng, h):
    """The BundleAdjuster of a Handle with its constants and mask set (the caller closes it)."""
    ba = eng.BundleAdjuster(h.intr, h.dist, h.cam_qt, h.tag_qt, h.tag_wh, h.fixed_tag, h.obs_cam, h.obs_tag, h.obs_px)
    ba.set_constant_poses(np.asarray(h.cam_const, np.uint8), np.asarray(h.tag_const, np.uint8))
    if not np.all(h.mask):
        ba.set_observation_mask(h.mask)
    return ba


def select_handle(fam, model, winners=False, counts=SELECT_COUNTS, outliers=True):
    """fam "cam": finished_map_cases.localize_scene as a handle, every tag constant at the truth and the cameras at
    placeholders, camera i with counts[i] observations; fam "tag": the dual from locate_scene, every camera constant.
    winners: in every list the observation at WINNER_AT gets its exact pixels."""
    def make():
        if fam == "cam":
            s = fm.localize_scene(model, outliers, counts=counts)
            obs_cam, obs_tag = s.obs_item.astype(np.int32), s.obs_tag
            cam_qt, tag_qt = np.tile(IDENTITY_CAM, (len(s.cam_gt), 1)), s.tag_gt.copy()
        else:
            s = fm.locate_scene(model, outliers, counts=counts)
            obs_cam, obs_tag = s.obs_cam, s.obs_item.astype(np.int32)
            cam_qt, tag_qt = s.cam_gt.copy(), np.tile(IDENTITY_TAG, (len(s.tag_gt), 1))
        px, label = s.obs_px.copy(), s.label.copy()
        winner = np.full(len(s.counts), -1)
        if winners:
            for i, m in enumerate(s.counts):
                d = int(s.start[i]) + WINNER_AT[m]
                px[d], label[d], winner[i] = s.clean_px[d], True, WINNER_AT[m]
        return Handle(own=fam, model=model, intr=s.intr, dist=s.dist, cam_qt=cam_qt, tag_qt=tag_qt, tag_wh=s.tag_wh,
                      fixed_tag=0 if fam == "cam" else -1, obs_cam=obs_cam, obs_tag=obs_tag, obs_px=px, label=label,
                      cam_const=np.full(len(cam_qt), fam == "tag", np.uint8), tag_const=np.full(len(tag_qt), fam == "cam", np.uint8),
                      cam_gt=s.cam_gt, tag_gt=s.tag_gt, counts=list(s.counts), winner=winner, clean_px=s.clean_px)
    return ec.cached(("init select", fam, model, bool(winners), tuple(counts), bool(outliers)), make)


def corridor(model, cross=False, n_cams=12, seed=20270102):
    """Camera k sees tags k and k + 1 (cross: also tag k + 3 where it exists); tag 0 is the origin.  The last tag has one
    observation only, so the default min_tag_observations leaves it out (without cross links)."""
    def make():
        rng = np.random.default_rng(seed + cross)
        intr, dist = fm.camera_model(model)
        n_tags = n_cams + 1
        # every tag 25 degrees out of the wall about the corridor's axis, up and down in turn: the cameras look along the
        # corridor, so no line of sight comes near a tag's normal.  A tag seen frontally has its two planar solutions meet,
        # the two candidates of its first observation then tie to rounding and the pose would be left out
        tag = np.array([np.r_[rg.qmul(_axis_quat([1.0, 0.0, 0.0], 25.0 if k % 2 else -25.0), rg.small_quat(rng, 0.05)),
                              0.45 * k + rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)]
                        for k in range(n_tags)])
        tag[0] = IDENTITY_TAG
        wh = np.where(rng.random(n_tags)[:, None] < 0.5, [[0.1285, 0.1285]], [[0.1165, 0.0923]])
        cam = np.array([np.r_[rg.qmul(rg.small_quat(rng, 0.04), _flip()), -(0.45 * k + 0.3) + rng.uniform(-0.05, 0.05),
                              rng.uniform(-0.1, 0.1), rng.uniform(2.6, 3.2)] for k in range(n_cams)])
        pairs = [(k, t) for k in range(n_cams) for t in ((k, k + 1, k + 3) if cross else (k, k + 1)) if t < n_tags]
        oc, ot = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
        pc = rg.camera_points(cam[oc], tag[ot], wh[ot])
        assert (pc[..., 2] > 0).all() and (fm.radial_slope(dist, pc) > 0).all()
        clean, px = rg.pixels(rng, intr, dist, cam[oc], tag[ot], wh[ot], NOISE_PX)
        tag0 = np.tile(IDENTITY_TAG, (n_tags, 1))
        return Handle(own="both", model=model, intr=intr, dist=dist, cam_qt=np.tile(IDENTITY_CAM, (n_cams, 1)), tag_qt=tag0,
                      tag_wh=wh, fixed_tag=0, obs_cam=oc, obs_tag=ot, obs_px=px, clean_px=clean, cam_gt=cam, tag_gt=tag,
                      cam_const=np.zeros(n_cams, np.uint8), tag_const=np.zeros(n_tags, np.uint8))
    return ec.cached(("init corridor", model, bool(cross), n_cams, seed), make)


def growth_handle(model, variant):
    """The corridor and what the growth tests do to it.
    corridor         as it stands: one tag per round, the last tag (one observation) is left out
    cross links      camera k sees tag k + 3 as well
    cut              both observations of camera 6 masked: tag 6 keeps one active observation, everything behind it its bytes
    constant camera  no origin tag; camera 6 constant at its true pose: growth starts there in both directions
    degenerate end   the last camera's observation of tag 11 has coincident corners: its only usable observation gives no
                     candidate, the camera keeps its bytes and is reported unreached"""
    h = corridor(model, cross=variant == "cross links")
    if variant in ("corridor", "cross links"):
        return h
    if variant == "cut":
        return h.copy(mask=(h.obs_cam != 6).astype(np.uint8))
    if variant == "constant camera":
        out = h.copy(fixed_tag=-1)
        out.cam_const[6] = 1
        out.cam_qt[6] = h.cam_gt[6]
        return out
    assert variant == "degenerate end"
    out = h.copy()
    d = int(np.flatnonzero((h.obs_cam == h.n_cams - 1) & (h.obs_tag == h.n_cams - 1))[0])
    out.obs_px[d] = DEGENERATE["coincident"]
    out.no_candidate = np.zeros(h.n_obs, bool)
    out.no_candidate[d] = True
    return out


def reach(h, min_tag_observations=2):
    """Breadth-first search over the visibility graph: (cam_reached, tag_reached, rounds).  A round reaches the cameras
    with an active observation of a reached tag, then the tags with >= min_tag_observations active observations one of
    which is a reached camera's; the round that reaches nothing is counted.  An observation named in h.no_candidate
    (a degenerate quad) counts as active and reaches nothing."""
    act = np.asarray(h.mask) != 0
    on = act & ~getattr(h, "no_candidate", np.zeros(h.n_obs, bool))
    cam_ok, tag_ok = h.const("cam"), h.const("tag")
    n_act = np.bincount(h.obs_tag[act], minlength=h.n_tags)
    rounds = 0
    while True:
        rounds += 1
        new_c = np.zeros(h.n_cams, bool)
        new_c[h.obs_cam[on & tag_ok[h.obs_tag]]] = True
        new_c &= ~cam_ok
        cam_ok = cam_ok | new_c
        new_t = np.zeros(h.n_tags, bool)
        new_t[h.obs_tag[on & cam_ok[h.obs_cam]]] = True
        new_t &= ~tag_ok & (n_act >= min_tag_observations)
        tag_ok = tag_ok | new_t
        if not new_c.any() and not new_t.any():
            return cam_ok, tag_ok, rounds


# ---- scores, candidates and one pass ------------------------------------------------------------------------------------

def scores(fam, h, p, cand, usable, oth_qt, cap_px, dtype=LD, chunk=96):
    """The truncated scores of the candidate poses cand (c, 7) of pose p of family fam over the observations `usable`
    (caller indices) whose counterparts stand at oth_qt (n_other, 7): (score (c,), corners below the cap (c, m))."""
    cand = np.asarray(cand, dtype).reshape(-1, 7)
    other = (h.obs_tag if fam == "cam" else h.obs_cam)[usable]
    oq = np.asarray(oth_qt, dtype)[other]
    wh = np.asarray(h.tag_wh, dtype)[other if fam == "cam" else np.full(len(usable), p)]
    px = np.asarray(h.obs_px, dtype)[usable].reshape(-1, 4, 2)
    cap2 = dtype(np.float64(cap_px) * np.float64(cap_px))
    local = rg.local_corners(wh, dtype)
    Ro = rg.rotation(oq, dtype)
    if fam == "cam":
        pw = np.einsum("mij,mkj->mki", Ro, local) + oq[:, None, 4:]
    intr, dist = np.asarray(h.intr, dtype), np.asarray(h.dist, dtype)
    out, below = np.zeros(len(cand), dtype), np.zeros((len(cand), len(usable)), np.int8)
    for b in range(0, len(cand), chunk):
        c = cand[b:b + chunk]
        Rc = rg.rotation(c, dtype)
        if fam == "cam":
            pc = np.einsum("cij,mkj->cmki", Rc, pw) + c[:, None, None, 4:]
        else:
            w = np.einsum("cij,mkj->cmki", Rc, local) + c[:, None, None, 4:]
            pc = np.einsum("mij,cmkj->cmki", Ro, w) + oq[None, :, None, 4:]
        x, y = pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2]
        xd, yd, _, _ = rg.distort(x, y, dist, dtype)
        ru, rv = intr[0] * xd + intr[2] - px[None, ..., 0], intr[1] * yd + intr[3] - px[None, ..., 1]
        e2 = ru * ru + rv * rv
        low = e2 < cap2
        out[b:b + chunk] = np.where(low, e2, np.where(np.isfinite(e2), cap2, dtype(INF))).sum(axis=(1, 2))
        below[b:b + chunk] = low.sum(axis=2)
    return out, below


class Pick:
    """What the selection of one pose amounts to: the candidates (index = 2 x list position + solution), their
    longdouble poses and scores, the winner, the margin between the two best scores."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def select_pose(fam, h, p, lst, placed_other, oth_qt, quad_qt2, quad_rms2, cap_px, min_obs=1, current=None):
    """k_init_score for pose p with the observation list lst (caller indices in list order).  None: the pose is not
    placed (no usable observation, too few active ones, or no candidate).  current: the pose as it stands, which
    competes as candidate -1 and wins ties (a sweep)."""
    other = (h.obs_tag if fam == "cam" else h.obs_cam)[lst]
    active = np.asarray(h.mask)[lst] != 0
    use = active & placed_other[other]
    if not use.any() or active.sum() < min_obs:
        return None
    usable = lst[use]
    index, rel, oth = [], [], []
    for pos in np.flatnonzero(use):
        for sol in range(2):
            if quad_rms2[lst[pos], sol] < INF:
                index.append(2 * pos + sol)
                rel.append(quad_qt2[lst[pos], sol])
                oth.append(oth_qt[other[pos]])
    if current is not None:
        index.append(-1)
    if not index:
        return None
    poses = chained_pose(fam, np.array(rel), np.array(oth), LD) if rel else np.zeros((0, 7), LD)
    if current is not None:
        poses = np.concatenate([poses, np.asarray(current, LD)[None]])
    sc, below = scores(fam, h, p, poses, usable, oth_qt, cap_px)
    index = np.array(index)
    if not (sc < LD(INF)).any():
        return None
    # lowest score, ties to the lowest index (-1, the pose as it stands, first)
    order = np.lexsort((index, sc))
    best = order[0]
    second = sc[order[1]] if len(order) > 1 else LD(INF)
    margin = float((second - sc[best]) / sc[best]) if sc[best] > 0 and np.isfinite(second) else INF
    tied = np.flatnonzero(sc - sc[best] <= LD(SCORE_GAP) * sc[best])     # positions whose score is the best's within SCORE_GAP
    return Pick(index=index, poses=poses, scores=sc, below=below, best=int(best), winner=int(index[best]), margin=margin, tied=tied,
                usable=usable, rel=np.array(rel), oth=np.array(oth), use=use)


def restate(h, quad_qt2, quad_rms2, cap_px, min_tag_observations=2, known=None, max_rounds=None):
    """vmm_ba_initialize with refine_iterations = 0 and sweeps = 0 as a function of the quad poses: each round runs the
    camera pass (against the tags placed before it) and then the tag pass (which sees the cameras of the same round); the
    run ends with the round that places nothing.  known = (cam_qt, tag_qt): the device's returned state, from which every
    placed pose is read bit for bit in place of the restated float64 chain (without sweeps a placed pose never changes).
    Returns dict(rounds, cam_placed, tag_placed, cam_qt, tag_qt, picks {(fam, p): Pick}, placed_in {(fam, p): round})."""
    state = {"cam": np.array(h.cam_qt, np.float64), "tag": np.array(h.tag_qt, np.float64)}
    placed = {"cam": h.const("cam"), "tag": h.const("tag")}
    const = {"cam": h.const("cam"), "tag": h.const("tag")}
    lists = {f: h.lists(f) for f in FAMILIES}
    picks, placed_in, rounds = {}, {}, 0
    n_pose = h.n_cams + h.n_tags
    while rounds < (max_rounds or n_pose):
        rounds += 1
        n_new = 0
        for fam in FAMILIES:
            oth_fam = "tag" if fam == "cam" else "cam"
            before = placed[oth_fam].copy()
            new = []
            for p, lst in enumerate(lists[fam]):
                if const[fam][p] or placed[fam][p] or not len(lst):
                    continue
                oq = state[oth_fam] if known is None else known[0 if oth_fam == "cam" else 1]
                pick = select_pose(fam, h, p, lst, before, oq, quad_qt2, quad_rms2, cap_px,
                                   1 if fam == "cam" else min_tag_observations)
                if pick is None:
                    continue
                picks[(fam, p)], placed_in[(fam, p)] = pick, rounds
                new.append(p)
                if known is None:
                    state[fam][p] = chained_pose(fam, pick.rel[pick.best], pick.oth[pick.best], np.float64)[0]
                else:
                    state[fam][p] = known[0 if fam == "cam" else 1][p]
            placed[fam][new] = True
            n_new += len(new)
        if n_new == 0:
            break
    return dict(rounds=rounds, cam_placed=placed["cam"], tag_placed=placed["tag"], cam_qt=state["cam"], tag_qt=state["tag"],
                picks=picks, placed_in=placed_in)


def pick_references(fam, pick):
    """The winner's pose by the two float64 references and their deviations from the longdouble chain."""
    rel, oth = pick.rel[pick.best][None], pick.oth[pick.best][None]
    truth = pick.poses[pick.best]
    return {"A numpy": float(pose_deviation(chained_pose_a(fam, rel, oth), truth)[0]),
            "B device scheme": float(pose_deviation(chained_pose(fam, rel, oth, np.float64), truth)[0])}


# ---- one pose against its fixed counterparts: sums, one trial, the optimum ------------------------------------------------

def pose_rows(fam, h, p, q, usable, oth_qt, dtype=LD):
    """(r (m, 4, 2), J (m, 4, 2, 6)) of pose p at q over the observations `usable`, eval_cases.corner_chain."""
    other = (h.obs_tag if fam == "cam" else h.obs_cam)[usable]
    oq = np.asarray(oth_qt)[other]
    own = np.tile(np.asarray(q), (len(usable), 1))
    cam, tag = (own, oq) if fam == "cam" else (oq, own)
    wh = h.tag_wh[other if fam == "cam" else np.full(len(usable), p)]
    r, _, Jc, Jt = ec.corner_chain(h.intr, h.dist, cam, tag, wh, h.obs_px[usable], dtype)
    return r, (Jc if fam == "cam" else Jt)


def ld_cost(fam, h, p, q, usable, oth_qt):
    r, _ = pose_rows(fam, h, p, q, usable, oth_qt, LD)
    return (r * r).sum(dtype=LD)


def pose_sums_b(fam, h, p, q, usable, oth_qt):
    """refine_sums<., true> in float64: cost, J^T J, J^T r in the device's order."""
    r, J = pose_rows(fam, h, p, q, usable, oth_qt, np.float64)
    cost = ra.wave_total(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])
    A = ra.wave_total(J[:, :, 0, :, None] * J[:, :, 0, None, :] + J[:, :, 1, :, None] * J[:, :, 1, None, :])
    g = ra.wave_total(J[:, :, 0] * r[:, :, 0, None] + J[:, :, 1] * r[:, :, 1, None])
    return cost, A, g


def _oracle_rows(O, fam, h, p, q, usable, oth_qt):
    other = (h.obs_tag if fam == "cam" else h.obs_cam)[usable]
    if fam == "cam":
        return ys.image_rows(O, h.intr, h.dist, q, oth_qt, h.tag_wh, other, h.obs_px[usable])
    return tc.tag_rows(O, h.intr, h.dist, q, oth_qt, h.tag_wh[p], other, h.obs_px[usable])


def trial(O, fam, h, p, start, usable, oth_qt):
    """One Levenberg-Marquardt trial of pose p from `start` at lam = kLamInit over the usable observations, no loss.
    Returns dict(truth (7,), scale sqrt(H_jj), accepted, refs {name: deviation}, cost0, cost1): the deviation of a pose is
    max_j |pose_minus(pose, truth)_j| sqrt(H_jj)."""
    r, J = pose_rows(fam, h, p, start, usable, oth_qt, LD)
    H = np.einsum("mkrp,mkrq->pq", J, J)
    g = np.einsum("mkrp,mkr->p", J, r)
    D = H + LD(LAM_INIT) * np.diag(np.maximum(np.diag(H), LD(1e-12)))
    inv, corr = cc.refined_inverse(D)
    step = -(inv @ g)
    truth = rg.pose_plus(start, step, LD)
    scale = np.sqrt(np.diag(H))
    out = dict(truth=truth, scale=scale, step=step, correction=float(np.abs((corr @ g) * scale).max()),
               cost0=(r * r).sum(dtype=LD), cost1=ld_cost(fam, h, p, truth, usable, oth_qt))
    out["accepted"] = bool(out["cost1"] < out["cost0"])
    _, A, ga = ys.block_normal(O, _oracle_rows(O, fam, h, p, np.asarray(start, np.float64), usable, oth_qt), False)
    a = O.pose_plus(np.asarray(start, np.float64), ys.plain_step(A, ga, LAM_INIT))
    _, B, gb = pose_sums_b(fam, h, p, start, usable, oth_qt)
    b = rg.pose_plus(start, ra.damped_solve(B, gb, LAM_INIT), np.float64)
    b[:4] = b[:4] * (1.0 / np.sqrt((b[:4] * b[:4]).sum()))
    out["refs"] = {"A oracle": trial_deviation(a, out), "B device scheme": trial_deviation(b, out)}
    return out


TRIAL_RESOLVED = 1e-9    # relative: three orders above the 1e-12 that pixel coordinates of a few thousand put into a cost


def trial_decrease(tr):
    """By how much of the cost the trial lowers it, from the longdouble costs before and after."""
    return float((tr["cost0"] - tr["cost1"]) / tr["cost0"])


def trial_resolved(tr):
    """Whether the trial is accepted whatever a float64 cost's rounding does: the decrease is above TRIAL_RESOLVED.  A
    list of one observation under the pinhole model is not: the planar solver has minimised that very cost."""
    return trial_decrease(tr) > TRIAL_RESOLVED


def trial_deviation(pose, tr):
    return float(np.abs(rg.pose_minus(pose, tr["truth"], LD) * tr["scale"]).max())


def refine_model(fam, h, p, start, usable, oth_qt, max_trials=REFINE_TRIALS):
    """lm_trials<6, 7, true, STOP_SMALL = true> of k_init_refine in numpy, float64: (pose, trials spent, why)."""
    def sums(x, idx):
        c, A, g = pose_sums_b(fam, h, p, x[0], usable, oth_qt)
        return np.array([c]), A[None], g[None]
    x, _, spent, why = lm_model(sums, np.asarray(start, np.float64)[None], max_trials, True)
    return x[0], int(spent[0]), why[0]


def host_optimum(O, fam, h, p, start, usable, oth_qt):
    """yardstick.image_optimum, or its tag dual, from `start` over the usable observations, no loss: (pose, cost)."""
    other = (h.obs_tag if fam == "cam" else h.obs_cam)[usable]
    if fam == "cam":
        s = ec.Scene(intr=h.intr, dist=h.dist, tag_gt=np.asarray(oth_qt), tag_wh=h.tag_wh)
        q, cost, _ = ys.image_optimum(O, s, start, other, h.obs_px[usable], False)
    else:
        q, cost, _ = tc.tag_optimum(O, h.intr, h.dist, start, np.asarray(oth_qt), h.tag_wh[p], other, h.obs_px[usable], False)
    return q, cost


# ---- the report ----------------------------------------------------------------------------------------------------------

def report_truth(h, cam_qt, tag_qt, cam_ok, tag_ok, dtype=LD):
    """avg_reprojection_px: the mean corner distance over the active observations between reached poses, and their
    number of corners."""
    on = (np.asarray(h.mask) != 0) & np.asarray(cam_ok)[h.obs_cam] & np.asarray(tag_ok)[h.obs_tag]
    if not on.any():
        return dtype(0), 0
    r, _, _, _ = ec.corner_chain(h.intr, h.dist, cam_qt[h.obs_cam[on]], tag_qt[h.obs_tag[on]], h.tag_wh[h.obs_tag[on]],
                                 h.obs_px[on], dtype)
    d = np.sqrt((r * r).sum(axis=-1))
    return d.sum(dtype=dtype) / dtype(d.size), int(d.size)


def report_floor(h, cam_qt, tag_qt, cam_ok, tag_ok):
    """What one rounding of every projected pixel does to the mean, relative: a corner distance of a third of a pixel is
    the difference of two coordinates of a few thousand and carries about 2^-53 (|proj| + |obs|) whatever its own size;
    over n corners the roundings add like a random walk, sqrt(sum (2^-53 (|proj| + |obs|))^2) / sum d.  A float64 mean
    cannot be expected below this and either reference may land far below it by luck, which is why A and B cannot be held
    within a factor of each other for a mean (test_init_cases_cpu.py); no bound uses this figure."""
    on = (np.asarray(h.mask) != 0) & np.asarray(cam_ok)[h.obs_cam] & np.asarray(tag_ok)[h.obs_tag]
    r, proj, _, _ = ec.corner_chain(h.intr, h.dist, cam_qt[h.obs_cam[on]], tag_qt[h.obs_tag[on]], h.tag_wh[h.obs_tag[on]],
                                    h.obs_px[on], LD)
    moved = LD(cc.U64) * (np.abs(proj) + np.abs(proj - r))
    return float(np.sqrt((moved * moved).sum()) / np.sqrt((r * r).sum(axis=-1)).sum())


def report_a(O, h, cam_qt, tag_qt, cam_ok, tag_ok):
    """Reference A: the oracle's residuals, numpy's mean."""
    on = (np.asarray(h.mask) != 0) & np.asarray(cam_ok)[h.obs_cam] & np.asarray(tag_ok)[h.obs_tag]
    d = []
    for i in np.flatnonzero(on):
        r = O.obs_eval(h.intr, h.dist, cam_qt[h.obs_cam[i]], tag_qt[h.obs_tag[i]], h.tag_wh[h.obs_tag[i]], h.obs_px[i], jac=False)
        r = np.asarray(r[0] if isinstance(r, tuple) else r).reshape(4, 2)
        d.append(np.sqrt((r * r).sum(axis=1)))
    return float(np.mean(d)) if d else 0.0


def report_b(h, cam_qt, tag_qt, cam_ok, tag_ok):
    """Reference B: k_init_stats and k_init_stats_sum in float64 -- per camera thread-private sums over d = thread,
    thread + 256, ... corner by corner, block_sum2's tree, then the cameras' partials the same way."""
    part_s, part_c = np.zeros(h.n_cams), np.zeros(h.n_cams)
    for p, lst in enumerate(h.lists("cam")):
        if not cam_ok[p] or not len(lst):
            continue
        use = (np.asarray(h.mask)[lst] != 0) & np.asarray(tag_ok)[h.obs_tag[lst]]
        r, _, _, _ = ec.corner_chain(h.intr, h.dist, np.tile(cam_qt[p], (len(lst), 1)), tag_qt[h.obs_tag[lst]],
                                     h.tag_wh[h.obs_tag[lst]], h.obs_px[lst], np.float64)
        d = np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])
        s, c = np.zeros(256), np.zeros(256)
        for pos in np.flatnonzero(use):
            for k in range(4):
                s[pos % 256] = s[pos % 256] + d[pos, k]
                c[pos % 256] += 1.0
        part_s[p], part_c[p] = ra.tree256(s), ra.tree256(c)
    s, c = np.zeros(256), np.zeros(256)
    for p in range(h.n_cams):
        s[p % 256] = s[p % 256] + part_s[p]
        c[p % 256] = c[p % 256] + part_c[p]
    total, count = ra.tree256(s), ra.tree256(c)
    return total / count if count > 0 else 0.0


def report_handle(model, masked=False, unreached=False):
    """The localize_scene handle with cameras of 1, 255, 256, 257 and 513 observations (the 256-thread stride of
    k_init_stats).  masked: every 5th observation off and the second-stride one of the 257 list; unreached: every
    observation of the 255 camera off."""
    h = select_handle("cam", model, counts=REPORT_COUNTS, outliers=False)
    if not (masked or unreached):
        return h
    mask = np.ones(h.n_obs, np.uint8)
    lists = h.lists("cam")
    if masked:
        mask[::5] = 0
        mask[lists[h.counts.index(257)][256]] = 0
        mask[lists[h.counts.index(513)][512]] = 1
    if unreached:
        mask[lists[h.counts.index(255)]] = 0
    return h.copy(mask=mask)


def relative(got, truth):
    truth = LD(truth)
    return float(abs(LD(got) - truth) / abs(truth))
