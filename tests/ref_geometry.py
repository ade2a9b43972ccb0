"""The geometry under every test reference, once: the case modules (eval_cases, cov_cases, finished_map_cases,
arrowhead_cases, init_cases, predict*_cases, rig_cases, linalg_cases) and yardstick.py build their truths and references
from these.  numpy only; it imports neither the engine nor the oracle, and there are no tests in here
(test_ref_modules_cpu.py checks it).

Conventions.  A pose is (qw, qx, qy, qz, tx, ty, tz): the quaternion w first and normalised before use, x -> R x + t.
A tangent step is (dt, d): Plus adds dt to the translation and multiplies the quaternion from the left by
(cos |d|, sin |d| d / |d|), a rotation by 2 |d| about d applied after the pose's own (the half-angle tangent), so
d(R p)/dd = -2 [R p]x.  A tag's corners run LL, LR, UR, UL in its own plane, signs * wh / 2 at z = 0.

Every function computes in the dtype the caller names -- np.longdouble for a truth, np.float64 for a reference B -- one
IEEE operation per written operation, in the written order: the bounds of the GPU tests are made of these bits
(tools/test_reference_bits.py prints them).  Where two float64 routes differ in bits and both are in use, the variant is a
named option: norm="linalg" takes |q| from np.linalg.norm of the one quaternion (a dot product), as the host yardstick
always has, up to 4.4e-16 away from sqrt(sum q q).
"""
import numpy as np

LD = np.longdouble
CORNER_SIGNS = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])   # LL, LR, UR, UL


# ---- rotations ----------------------------------------------------------------------------------------------------------

def unit(q, dtype=LD, norm="sum"):
    """q (..., 4+) -> its quaternion over its length; norm="linalg": one quaternion, |q| from np.linalg.norm."""
    q = np.asarray(q, dtype)[..., :4]
    if norm == "linalg":
        assert q.ndim == 1
        return q / np.linalg.norm(q)
    return q / np.sqrt((q * q).sum(axis=-1, keepdims=True))


def rotation(q, dtype=LD, norm="sum"):
    """(..., 3, 3) rotation of q (..., 4+) / |q| (make_kats.quat_rotate, load_rigid<true>)."""
    q = unit(q, dtype, norm)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = dtype(1), dtype(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def qmul(a, b):
    """The Hamilton product a b of (..., 4) quaternions, in their own dtype."""
    a, b = np.asarray(a), np.asarray(b)
    a0, a1, a2, a3 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    b0, b1, b2, b3 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                     a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                     a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], axis=-1)


def skew(v):
    """(..., 3, 3) matrix [v]x with [v]x u = v x u."""
    v = np.asarray(v)
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], axis=-1),
                     np.stack([v[..., 2], z, -v[..., 0]], axis=-1),
                     np.stack([-v[..., 1], v[..., 0], z], axis=-1)], axis=-2)


def quat_from_R(R, dtype=LD):
    """pose_lm.hpp's quat_from_R (Eigen's trace test) for (n, 3, 3).  Returns (q (n, 4) normalised, branch (n,) in 0..3)."""
    R = np.asarray(R, dtype).reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    branch = np.where(tr > 0, 0, np.where((R[:, 0, 0] >= R[:, 1, 1]) & (R[:, 0, 0] >= R[:, 2, 2]), 1,
                                          np.where(R[:, 1, 1] >= R[:, 2, 2], 2, 3)))
    q = np.zeros((len(R), 4), dtype)
    one, two, quarter = dtype(1), dtype(2), dtype(0.25)
    for b in range(4):
        m = branch == b
        if not m.any():
            continue
        r = R[m]
        if b == 0:
            s = np.sqrt(tr[m] + one) * two
            q[m] = np.stack([quarter * s, (r[:, 2, 1] - r[:, 1, 2]) / s, (r[:, 0, 2] - r[:, 2, 0]) / s,
                             (r[:, 1, 0] - r[:, 0, 1]) / s], axis=1)
        else:
            i = b - 1
            j, k = (i + 1) % 3, (i + 2) % 3
            s = np.sqrt(r[:, i, i] - r[:, j, j] - r[:, k, k] + one) * two
            v = np.zeros((len(r), 4), dtype)
            v[:, 0] = (r[:, k, j] - r[:, j, k]) / s
            v[:, 1 + i] = quarter * s
            v[:, 1 + j] = (r[:, j, i] + r[:, i, j]) / s
            v[:, 1 + k] = (r[:, k, i] + r[:, i, k]) / s
            q[m] = v
    return q / np.sqrt((q * q).sum(axis=1, keepdims=True)), branch


# ---- Plus and its inverse ---------------------------------------------------------------------------------------------------

def pose_plus(qt, d, dtype=None):
    """vmm_ba_pose_plus, geom.hpp's pose_plus, oracle/vmm_oracle.c's vo_pose_plus: (7,) and (6,), or (n, 7) and (n, 6), in
    `dtype` (None: that of d).  A zero rotation step leaves the quaternion as it is."""
    d = np.asarray(d) if dtype is None else np.asarray(d, dtype)
    dt = d.dtype.type
    single = d.ndim == 1
    qt, d = np.asarray(qt).astype(dt).reshape(-1, 7), d.reshape(-1, 6)
    out = qt.copy()
    out[:, 4:] = qt[:, 4:] + d[:, :3]
    r = d[:, 3:]
    nd = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
    nz = nd > 0
    safe = np.where(nz, nd, dt(1))
    s = np.sin(safe) / safe
    z = np.stack([np.cos(safe), s * r[:, 0], s * r[:, 1], s * r[:, 2]], axis=1)
    out[:, :4] = np.where(nz[:, None], qmul(z, qt[:, :4]), qt[:, :4])
    return out[0] if single else out


def pose_minus(a, b, dtype=LD):
    """The tangent d with pose_plus(b, d) = a for two poses (7,) (the quaternions taken as rotations: their lengths and
    signs do not count)."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    z = qmul(a[:4], np.concatenate([b[:1], -b[1:4]]))
    z = z / np.sqrt((z * z).sum())
    z = -z if z[0] < 0 else z
    nv = np.sqrt((z[1:] * z[1:]).sum())
    rot = z[1:] * (np.arctan2(nv, z[0]) / nv) if nv > 0 else np.zeros(3, dtype)
    return np.concatenate([a[4:] - b[4:], rot])


# ---- a tag's corners --------------------------------------------------------------------------------------------------------

def local_corners(wh, dtype=LD):
    """(n, 4, 3): the corners of tags of size wh (n, 2) in their own frame, signs * wh / 2 at z = 0."""
    wh = np.asarray(wh, dtype).reshape(-1, 2)
    local = np.zeros((len(wh), 4, 3), dtype)
    local[:, :, :2] = CORNER_SIGNS.astype(dtype)[None] * (wh / dtype(2))[:, None, :]
    return local


def world_corners(tag_qt, wh, dtype=LD, parts=False):
    """(n, 4, 3): the corners of the tags at tag_qt (n, 7) in the world.  parts: (corners, R_t p before the translation)."""
    tag_qt = np.asarray(tag_qt, dtype).reshape(-1, 7)
    a = np.einsum("nij,nkj->nki", rotation(tag_qt, dtype), local_corners(wh, dtype))
    pw = a + tag_qt[:, None, 4:]
    return (pw, a) if parts else pw


def camera_points(cam_qt, tag_qt, wh, dtype=LD, parts=False):
    """(n, 4, 3): the corners in the frames of the cameras cam_qt (n, 7).  parts: (points, R_c, R_t p, R_c P_w), what the
    chain's Jacobians are made of."""
    cam_qt = np.asarray(cam_qt, dtype).reshape(-1, 7)
    pw, a = world_corners(tag_qt, wh, dtype, parts=True)
    Rc = rotation(cam_qt, dtype)
    b = np.einsum("nij,nkj->nki", Rc, pw)
    pc = b + cam_qt[:, None, 4:]
    return (pc, Rc, a, b) if parts else pc


# ---- the camera model -------------------------------------------------------------------------------------------------------

def distort(x, y, dist, dtype=LD, aliased=False):
    """The cost functor's distortion of the normalised point (x, y) under dist = (k1, k2, p1, p2, k3):
    xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2), rad = 1 + r2 (k1 + r2 (k2 + r2 k3)).
    aliased: CameraModel::projectPoint's yd, whose tangential term is formed from the already distorted x,
    2 p2 xd y: the functor's + 2 p2 (xd - x) y.  Returns (xd, yd, r2, rad)."""
    k1, k2, p1, p2, k3 = dist
    two = dtype(2)
    r2 = x * x + y * y
    rad = dtype(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + two * p1 * x * y + p2 * (r2 + two * x * x)
    yd = y * rad + two * p2 * (xd if aliased else x) * y + p1 * (r2 + two * y * y)
    return xd, yd, r2, rad


def pixel(intr, xd, yd):
    """(..., 2): u = fx xd + cx, v = fy yd + cy."""
    return np.stack([intr[0] * xd + intr[2], intr[1] * yd + intr[3]], axis=-1)


def project(intr, dist, cam_qt, tag_qt, wh, dtype=LD):
    """(n, 4, 2): the functor's pixels of the corners of tag_qt (n, 7) in the cameras cam_qt (n, 7)."""
    pc = camera_points(cam_qt, tag_qt, wh, dtype)
    xd, yd, _, _ = distort(pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2], np.asarray(dist, dtype), dtype)
    return pixel(np.asarray(intr, dtype), xd, yd)


# ---- a camera on a rig ------------------------------------------------------------------------------------------------------

def compose_rig(ext, rig, dtype=LD, norm="sum"):
    """Camera = ext o rig: (the pose (q_c q_f, R_c t_f + t_c), R_c, R_c t_f)."""
    ext, rig = np.asarray(ext, dtype), np.asarray(rig, dtype)
    Rc = rotation(ext, dtype, norm)
    v = Rc @ rig[4:]
    return np.concatenate([qmul(unit(ext, dtype, norm), unit(rig, dtype, norm)), v + ext[4:]]), Rc, v


def turn_to_rig(Jc, Rc):
    """The camera columns Jc (..., 6) over the rig's tangent: a rig step (dt, dth) moves the camera by (R_c dt, R_c dth),
    J_rig = [Jc_t R_c | Jc_r R_c]."""
    return np.concatenate([Jc[..., :3] @ Rc, Jc[..., 3:] @ Rc], axis=-1)


def extrinsic_columns(Jc, v, dtype=LD):
    """The camera columns over the extrinsic's own tangent: a step (ds, dphi) moves the camera by (ds + 2 dphi x v, dphi)
    with v = R_c t_f, J_ext = [Jc_t | Jc_r - 2 Jc_t [v]x]."""
    return np.concatenate([Jc[..., :3], Jc[..., 3:] - dtype(2) * (Jc[..., :3] @ skew(v))], axis=-1)


# ---- seeded pieces of the scenes ----------------------------------------------------------------------------------------------

def small_quat(rng, sigma=0.08):
    """A unit quaternion near the identity: three draws of rng."""
    v = np.r_[1.0, rng.normal(0, sigma, 3)]
    return v / np.linalg.norm(v)


def pixels(rng, intr, dist, cam, tag, wh, noise_px):
    """(clean pixels (n, 8) from the longdouble chain rounded to double, the same with seeded Gaussian noise)."""
    clean = project(intr, dist, cam, tag, wh, LD).reshape(-1, 8).astype(np.float64)
    return clean, clean + rng.normal(0, noise_px, clean.shape)


def start(counts):
    """The CSR offsets (len + 1, int64) of lists of the given lengths."""
    out = np.zeros(len(counts) + 1, np.int64)
    out[1:] = np.cumsum(counts)
    return out
