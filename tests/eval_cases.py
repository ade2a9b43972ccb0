"""References and scenes for the per-entry tests of the evaluation (test_eval_cases_cpu.py, test_gpu_eval_accuracy.py,
tools/eval_accuracy.py).  numpy only: nothing here calls the engine.

The corner chain (tag corner -> world -> camera -> distorted pixel -> residual, its 2x6 tangent Jacobians, the Huber
weight) is restated from the formulas of tests/golden/make_kats.py over ref_geometry.py's pieces (conventions there),
vectorised over observations, in a dtype of the caller's choice:

    np.longdouble   the reference every deviation is measured against
    np.float64      reference B: what a plain f64 evaluation achieves
    f32 products    reference F: f64 Jacobians, J products and block sums in float32 (VMM_BA_PRECISION_F32_ACCUM)

Reference A is the oracle's functor summed in numpy (test_gpu_kernels._blocks_from_oracle's scheme, here with the
Huber width, the constant flags and the mask).

The metric.  Every output entry is a sum; its MAGNITUDE is the same sum with every summand replaced by its absolute
value: sum w^2 |J_rp| |J_rq| for V, U and W, sum w^2 |J_rp| (|proj_r| + |obs_r|) for the gradients (the residual is itself
a difference of two pixel coordinates), the cost for the cost.  The DEVIATION of a result is
max over entries |got - longdouble| / magnitude, per array; an entry of magnitude 0 (constant or unobserved pose, masked
observation) must be exactly 0 and is left out of the ratio.  A block with one observation, an outlier's down-weighted
rows or a small gradient entry counts as much as the largest block of the scene -- 1e-10 x max|array| does not see them.
"""
import json
import os

import numpy as np

import ref_geometry as rg

LD = np.longdouble
MARGIN = 8.0          # the device may deviate 8 x as far as the worse of references A and B (tests/linalg_cases.py)
ARRAYS = ("V", "U", "W", "g_cam", "g_tag", "cost")
README_INTR = [8.0752937867635346e+03, 8.0831676114192869e+03, 3.0163896805084278e+03, 1.9962896554785455e+03]
README_DIST = [-1.8618183262669760e-01, 3.7018092365577054e-01, -2.9390604003594177e-04, 4.1533180829908799e-04,
               5.7043887874185996e-02]


class Scene:
    """intr, dist, cam_qt, tag_qt, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px (+ whatever the builder adds)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_obs(self):
        return len(self.obs_cam)


# ---- the corner chain -------------------------------------------------------------------------------------------------

def corner_chain(intr, dist, cam_qt, tag_qt, wh, px, dtype=LD, want_magnitude=False):
    """n observations: cam_qt (n, 7), tag_qt (n, 7), wh (n, 2), px (n, 8).  Returns the residuals r (n, 4, 2), the
    projections proj (n, 4, 2) and the tangent Jacobians Jc, Jt (n, 4, 2, 6) (translation, then half-angle rotation:
    Plus multiplies the quaternion from the left by (cos|d|, sin|d| d / |d|), a rotation by 2|d| about d applied after
    the pose's own, so d(R p)/dd = -2 [R p]x).  want_magnitude: also the magnitudes of Jc and Jt, the same matrix
    products over absolute values (an entry of the Jacobian is itself a sum that may cancel, exactly so without
    distortion)."""
    intr, dist = np.asarray(intr, dtype), np.asarray(dist, dtype)
    cam_qt, tag_qt = np.asarray(cam_qt, dtype).reshape(-1, 7), np.asarray(tag_qt, dtype).reshape(-1, 7)
    wh, px = np.asarray(wh, dtype).reshape(-1, 2), np.asarray(px, dtype).reshape(-1, 4, 2)
    two = dtype(2)
    pc, Rc, a, b = rg.camera_points(cam_qt, tag_qt, wh, dtype, parts=True)      # a = R_t p, b = R_c P_w
    x, y = pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2]
    k1, k2, p1, p2, k3 = dist
    xd, yd, r2, rad = rg.distort(x, y, dist, dtype)
    proj = rg.pixel(intr, xd, yd)
    r = proj - px
    # d(xd, yd) / d(x, y)
    drad = k1 + r2 * (two * k2 + dtype(3) * k3 * r2)          # d rad / d r2
    D = np.empty(x.shape + (2, 2), dtype)
    D[..., 0, 0] = rad + two * x * x * drad + two * p1 * y + dtype(6) * p2 * x
    D[..., 0, 1] = two * x * y * drad + two * p1 * x + two * p2 * y
    D[..., 1, 0] = two * x * y * drad + two * p2 * y + two * p1 * x
    D[..., 1, 1] = rad + two * y * y * drad + two * p2 * x + dtype(6) * p1 * y
    # d(x, y) / d P_c
    iz = dtype(1) / pc[..., 2]
    Pi = np.zeros(x.shape + (2, 3), dtype)
    Pi[..., 0, 0] = iz
    Pi[..., 1, 1] = iz
    Pi[..., 0, 2] = -x * iz
    Pi[..., 1, 2] = -y * iz
    G = np.einsum("r,nkrs,nksj->nkrj", intr[:2], D, Pi)       # d residual / d P_c  (n, 4, 2, 3)
    Jc = np.concatenate([G, -two * np.einsum("nkri,nkij->nkrj", G, rg.skew(b))], axis=-1)
    Gw = np.einsum("nkri,nij->nkrj", G, Rc)                   # d residual / d P_w
    Jt = np.concatenate([Gw, -two * np.einsum("nkri,nkij->nkrj", Gw, rg.skew(a))], axis=-1)
    if not want_magnitude:
        return r, proj, Jc, Jt
    Ga = np.einsum("r,nkrs,nksj->nkrj", np.abs(intr[:2]), np.abs(D), np.abs(Pi))
    Jc_mag = np.concatenate([Ga, two * np.einsum("nkri,nkij->nkrj", Ga, np.abs(rg.skew(b)))], axis=-1)
    Gwa = np.einsum("nkri,nij->nkrj", Ga, np.abs(Rc))
    Jt_mag = np.concatenate([Gwa, two * np.einsum("nkri,nkij->nkrj", Gwa, np.abs(rg.skew(a)))], axis=-1)
    return r, proj, Jc, Jt, Jc_mag, Jt_mag


def huber(a, s, dtype=LD):
    """rho (.., 3) of ceres::HuberLoss(a) at s; the threshold is the f64 product a * a (make_kats.huber_width_cases)."""
    s = np.asarray(s, dtype)
    a64 = np.float64(a)
    b = dtype(a64 * a64)
    a = dtype(a64)
    out = np.zeros(s.shape + (3,), dtype)
    lin = s > b
    rt = np.sqrt(np.where(lin, s, dtype(1)))
    out[..., 0] = np.where(lin, dtype(2) * a * rt - b, s)
    out[..., 1] = np.where(lin, a / rt, dtype(1))
    out[..., 2] = np.where(lin, -(a / rt) / (dtype(2) * np.where(lin, s, dtype(1))), dtype(0))
    return out


# ---- the blocks of a scene --------------------------------------------------------------------------------------------

def flags(s, cam_const, tag_const):
    """(cameras, tags) held constant, bool: the given sets and the fixed tag."""
    cc = np.zeros(len(s.cam_qt), bool) if cam_const is None else np.asarray(cam_const) != 0
    tc = np.zeros(len(s.tag_qt), bool) if tag_const is None else np.asarray(tag_const) != 0
    tc = tc.copy()
    if s.fixed_tag >= 0:
        tc[s.fixed_tag] = True
    return cc, tc


def _sum_blocks(s, r, Jc, Jt, w, cost_terms, dtype, products=None):
    """V, U, W, g_cam, g_tag, cost from weighted rows.  r (n, 4, 2); Jc, Jt (n, 4, 2, 6) (already zero for
    constant poses); w (n, 4) row weights (zero for masked observations); products: dtype of the J^T J products and
    sums (reference F: float32), the gradients and the cost stay in `dtype`."""
    pt = products or dtype
    n_c, n_t = len(s.cam_qt), len(s.tag_qt)
    Jcw, Jtw = Jc * w[:, :, None, None], Jt * w[:, :, None, None]
    rw = r * w[:, :, None]
    jc, jt = Jcw.astype(pt).reshape(-1, 8, 6), Jtw.astype(pt).reshape(-1, 8, 6)
    Vo, Uo, W = np.zeros((len(jc), 6, 6), pt), np.zeros((len(jc), 6, 6), pt), np.zeros((len(jc), 6, 6), pt)
    for k in range(8):    # row by row in the products' own dtype (einsum may accumulate wider)
        Vo += jc[:, k, :, None] * jc[:, k, None, :]
        Uo += jt[:, k, :, None] * jt[:, k, None, :]
        W += jc[:, k, :, None] * jt[:, k, None, :]
    V, U = np.zeros((n_c, 6, 6), pt), np.zeros((n_t, 6, 6), pt)
    np.add.at(V, s.obs_cam, Vo)
    np.add.at(U, s.obs_tag, Uo)
    gc, gt = np.zeros((n_c, 6), dtype), np.zeros((n_t, 6), dtype)
    np.add.at(gc, s.obs_cam, np.einsum("nkrp,nkr->np", Jcw, rw))
    np.add.at(gt, s.obs_tag, np.einsum("nkrp,nkr->np", Jtw, rw))
    return dict(V=V, U=U, W=W, g_cam=gc, g_tag=gt, cost=cost_terms.sum(dtype=dtype))


def assemble(s, a=1.0, robust=True, dtype=LD, products=None, mask=None, cam_const=None, tag_const=None,
             want_magnitude=False):
    """The blocks of scene s at its poses.  want_magnitude: also the dict of magnitudes (see the module docstring)."""
    chain_dtype = np.float64 if products is not None else dtype
    r, proj, Jc, Jt = corner_chain(s.intr, s.dist, s.cam_qt[s.obs_cam], s.tag_qt[s.obs_tag], s.tag_wh[s.obs_tag],
                                   s.obs_px, chain_dtype)
    cc, tc = flags(s, cam_const, tag_const)
    on = np.ones(s.n_obs, bool) if mask is None else np.asarray(mask) != 0
    Jc = np.where(cc[s.obs_cam][:, None, None, None], chain_dtype(0), Jc)
    Jt = np.where(tc[s.obs_tag][:, None, None, None], chain_dtype(0), Jt)
    sq = (r * r).sum(axis=-1)
    rho = huber(a, sq, chain_dtype) if robust else np.stack([sq, np.ones_like(sq), np.zeros_like(sq)], axis=-1)
    w = np.where(on[:, None], np.sqrt(rho[..., 1]), chain_dtype(0))
    cost_terms = np.where(on[:, None], rho[..., 0] / chain_dtype(2), chain_dtype(0))
    out = _sum_blocks(s, r, Jc, Jt, w, cost_terms, chain_dtype, products)
    if not want_magnitude:
        return out
    absr = np.abs(proj) + np.abs(np.asarray(s.obs_px, chain_dtype).reshape(-1, 4, 2))
    # the same sums over absolute values: |J| w in place of J w, (|proj| + |obs|) w in place of r w
    mag = _sum_blocks(s, absr, np.abs(Jc), np.abs(Jt), w, cost_terms, chain_dtype)
    return out, mag


def blocks_from_oracle(O, s, a=1.0, robust=True, mask=None, cam_const=None, tag_const=None):
    """Reference A: the oracle's residuals, Jacobians (O.obs_eval) and Huber values (O.huber(a, .)), summed in numpy f64 in
    the caller's order, as test_gpu_kernels._blocks_from_oracle does for a = 1."""
    n_c, n_t = len(s.cam_qt), len(s.tag_qt)
    cc, tc = flags(s, cam_const, tag_const)
    V, U, W = np.zeros((n_c, 6, 6)), np.zeros((n_t, 6, 6)), np.zeros((s.n_obs, 6, 6))
    gc, gt = np.zeros((n_c, 6)), np.zeros((n_t, 6))
    cost = 0.0
    for i, (c, t) in enumerate(zip(s.obs_cam, s.obs_tag)):
        if mask is not None and not mask[i]:
            continue
        r, Jc, Jt = O.obs_eval(s.intr, s.dist, s.cam_qt[c], s.tag_qt[t], s.tag_wh[t], s.obs_px[i])
        if cc[c]:
            Jc = np.zeros_like(Jc)
        if tc[t]:
            Jt = np.zeros_like(Jt)
        for k in range(4):
            sq = r[2 * k] ** 2 + r[2 * k + 1] ** 2
            rho = O.huber(a, sq) if robust else np.array([sq, 1.0, 0.0])
            cost += 0.5 * rho[0]
            w = np.sqrt(rho[1])
            Jc[2 * k:2 * k + 2] *= w
            Jt[2 * k:2 * k + 2] *= w
            r[2 * k:2 * k + 2] *= w
        V[c] += Jc.T @ Jc
        U[t] += Jt.T @ Jt
        W[i] = Jc.T @ Jt
        gc[c] += Jc.T @ r
        gt[t] += Jt.T @ r
    return dict(V=V, U=U, W=W, g_cam=gc, g_tag=gt, cost=cost)


def deviation(got, ref, mag):
    """{array: (max |got - ref| / magnitude over the entries of non-zero magnitude, all entries of zero magnitude are
    exactly zero)}."""
    out = {}
    for k in ARRAYS:
        g, r, m = (np.atleast_1d(np.asarray(v, LD)) for v in (got[k], ref[k], mag[k]))
        nz = m > 0
        dev = float(np.max(np.abs(g - r)[nz] / m[nz])) if nz.any() else 0.0
        out[k] = (dev, bool(np.all(g[~nz] == 0)))
    return out


class Case:
    """One scene in one configuration (width, robust, mask, constant poses) with its longdouble blocks, magnitudes and the
    deviations of the CPU references; computed once and shared (cases())."""

    def __init__(self, O, s, a=1.0, robust=True, mask=None, cam_const=None, tag_const=None, f32=False):
        self.scene, self.a, self.robust, self.mask, self.cam_const, self.tag_const = s, a, robust, mask, cam_const, tag_const
        kw = dict(a=a, robust=robust, mask=mask, cam_const=cam_const, tag_const=tag_const)
        self.ref, self.mag = assemble(s, dtype=LD, want_magnitude=True, **kw)
        self.refs = {"A oracle": deviation(blocks_from_oracle(O, s, **kw), self.ref, self.mag),
                     "B float64": deviation(assemble(s, dtype=np.float64, **kw), self.ref, self.mag)}
        self.bound = {k: MARGIN * max(d[k][0] for d in self.refs.values()) for k in ARRAYS}
        if f32:
            self.refs["F float32 products"] = deviation(assemble(s, products=np.float32, **kw), self.ref, self.mag)
            self.bound_f32 = dict(self.bound)
            for k in ("V", "U", "W"):
                self.bound_f32[k] = MARGIN * self.refs["F float32 products"][k][0]

    def check(self, got, label, bound=None, out=print):
        """Prints deviation, bound and ratio of every array of `got`; returns the list of failures (empty: all well)."""
        bound = bound or self.bound
        bad = []
        for k, (dev, zeros_ok) in deviation(got, self.ref, self.mag).items():
            ratio = dev / bound[k] if bound[k] else (0.0 if dev == 0 else float("inf"))
            out("%s %-5s deviation %.3e  bound %.3e  ratio %.3f%s" % (label, k, dev, bound[k], ratio,
                                                                      "" if zeros_ok else "  NON-ZERO where the magnitude is 0"))
            if not (dev <= bound[k]):
                bad.append("%s %s: deviation %.3e above the bound %.3e" % (label, k, dev, bound[k]))
            if not zeros_ok:
                bad.append("%s %s: an entry of magnitude 0 is not exactly 0" % (label, k))
        return bad


_CASES = {}


def cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ---- scenes -----------------------------------------------------------------------------------------------------------

def _wall(rng, n_cams, n_tags):
    """Tags near the plane z = 0, cameras about 3 m in front of it looking at it (the layout of the `obs` KATs)."""
    tag = np.array([np.r_[rg.small_quat(rng), rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.normal(0, 0.05)]
                    for _ in range(n_tags)])
    cam = np.array([np.r_[rg.qmul(rg.small_quat(rng), [0.0, 1.0, 0.0, 0.0]), rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4),
                          rng.uniform(2.5, 4.0)] for _ in range(n_cams)])
    wh = np.where(rng.random(n_tags)[:, None] < 0.5, [[0.1285, 0.1285]], [[0.1165, 0.0923]])
    return cam, tag, wh


def mixed_scene(a):
    """12 x 9 poses, every pair observed, README distortion; pixel noise of sigma = a / sqrt(2 ln 2), at which half of the
    corners have |r|^2 above a^2 (|r|^2 / sigma^2 is chi-square with two degrees of freedom)."""
    def make():
        rng = np.random.default_rng(20261101)
        cam, tag, wh = _wall(rng, 12, 9)
        oc, ot = (v.reshape(-1).astype(np.int32) for v in np.meshgrid(np.arange(12), np.arange(9), indexing="ij"))
        px = rg.pixels(rng, README_INTR, README_DIST, cam[oc], tag[ot], wh[ot], float(a) / np.sqrt(2 * np.log(2)))[1]
        return Scene(intr=np.array(README_INTR), dist=np.array(README_DIST), cam_qt=cam, tag_qt=tag, tag_wh=wh, fixed_tag=0,
                     obs_cam=oc, obs_tag=ot, obs_px=px)
    return cached(("mixed", float(a)), make)


def fraction_above(s, a):
    """Share of the corners of s with |r|^2 > a^2, from the longdouble chain."""
    r, _, _, _ = corner_chain(s.intr, s.dist, s.cam_qt[s.obs_cam], s.tag_qt[s.obs_tag], s.tag_wh[s.obs_tag], s.obs_px)
    a64 = np.float64(a)
    return float(((r * r).sum(axis=-1) > LD(a64 * a64)).mean())


RAGGED_COUNTS = (1, 63, 64, 65, 128, 129)


def ragged_scene(few="tags"):
    """130 poses of one family, six of the other; the six have exactly 1, 63, 64, 65, 128 and 129 observations (pose k
    of the six sees poses 0 .. count-1 of the 130, the single observation is of pose 5), so pose 129 of the 130 has none.
    One wave takes 64 observations of one pose: the six make 1+1+1+2+2+3 = 10 tasks, the 130 make 129, neither a multiple
    of the four tasks of a workgroup.  few = "tags": 130 cameras x 6 tags, no fixed tag; "cams": 6 cameras x 130 tags, tag
    3 fixed.  Observations come pose by pose of the six, so `last_of_65` is lane 0 of that pose's second task."""
    def make():
        rng = np.random.default_rng(20261102 + (few == "cams"))
        many, six = [], []
        for k, n in enumerate(RAGGED_COUNTS):
            many += [5] if n == 1 else list(range(n))
            six += [k] * n
        many, six = np.array(many, np.int32), np.array(six, np.int32)
        if few == "tags":
            cam, tag, wh = _wall(rng, 130, 6)
            oc, ot, fixed = many, six, -1
        else:
            cam, tag, wh = _wall(rng, 6, 130)
            oc, ot, fixed = six, many, 3
        px = rg.pixels(rng, README_INTR, README_DIST, cam[oc], tag[ot], wh[ot], 0.8)[1]
        last_of_65 = int(np.flatnonzero(six == RAGGED_COUNTS.index(65))[-1])
        return Scene(intr=np.array(README_INTR), dist=np.array(README_DIST), cam_qt=cam, tag_qt=tag, tag_wh=wh,
                     fixed_tag=fixed, obs_cam=oc, obs_tag=ot, obs_px=px, few=few, last_of_65=last_of_65,
                     six=six, many=many)
    return cached(("ragged", few), make)


def ragged_mask(s):
    """Every 7th observation off, and the last one of the 65-observation pose."""
    m = np.ones(s.n_obs, np.uint8)
    m[::7] = 0
    m[s.last_of_65] = 0
    return m


def ragged_constants(s):
    """One camera and one tag (besides the fixed one) held constant: the poses with 64 observations (of the six) and
    pose 2 of the 130."""
    cc, tc = np.zeros(len(s.cam_qt), np.uint8), np.zeros(len(s.tag_qt), np.uint8)
    few_flags, many_flags = (tc, cc) if s.few == "tags" else (cc, tc)
    few_flags[RAGGED_COUNTS.index(64)] = 1
    many_flags[2] = 1
    return cc, tc


def task_counts(s):
    """(tasks of the camera family, of the tag family): one per started 64 observations of a pose."""
    return tuple(int(np.sum((np.bincount(idx, minlength=n) + 63) // 64))
                 for idx, n in ((s.obs_cam, len(s.cam_qt)), (s.obs_tag, len(s.tag_qt))))


def load_kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_residual.json")) as f:
        return json.load(f)


def _inverse_pose(qt):
    """world->camera pose as camera->world (unit quaternion), longdouble."""
    qt = np.asarray(qt, LD)
    q = rg.unit(qt)
    return np.r_[q[0], -q[1:]], -rg.rotation(qt).T @ qt[4:]


def _compose(q1, t1, q2, t2):
    """x -> R1 (R2 x + t2) + t1."""
    return rg.qmul(q1, q2), rg.rotation(q1) @ t2 + t1


def single_record_scene(case):
    """One `obs` / `obs_hard` record as a scene of one camera, one tag, one observation, no fixed tag."""
    return Scene(intr=np.array(case["intr"]), dist=np.array(case["dist"]), cam_qt=np.array([case["cam_qt"]]),
                 tag_qt=np.array([case["tag_qt"]]), tag_wh=np.array([case["wh"]]), fixed_tag=-1,
                 obs_cam=np.zeros(1, np.int32), obs_tag=np.zeros(1, np.int32), obs_px=np.array([case["px"]]))


def hard_batch(strong, kats=None):
    """The eight `obs_hard` records of one distortion (strong or none), each with its own camera: the camera of record i
    sees 65 tags of its own.  Its observation 0 is the record itself (its tag, its pixels), observations 63 and 64 carry
    the geometry of records i+1 and i+2 (their tag's pose relative to their camera, moved in front of camera i; their
    residual pattern, so an outlier stays one), observations 1 .. 62 are ordinary tags about 3 m in front of the camera.
    Lanes 0 and 63 of the camera's first task and lane 0 of its second are the hard ones."""
    def make():
        recs = [c for c in (kats or load_kats())["obs_hard"] if (np.abs(c["dist"]).max() > 0) == bool(strong)]
        rng = np.random.default_rng(20261103 + bool(strong))
        intr, dist = recs[0]["intr"], recs[0]["dist"]
        cams, tags, whs, oc, ot, pxs = [], [], [], [], [], []
        for i, rec in enumerate(recs):
            cams.append(rec["cam_qt"])
            qi, ti = _inverse_pose(rec["cam_qt"])
            for slot in range(65):
                if slot == 0:
                    tag, wh, px = np.array(rec["tag_qt"]), rec["wh"], np.array(rec["px"])
                else:
                    if slot >= 63:
                        other = recs[(i + slot - 62) % len(recs)]
                        qo, to = np.asarray(other["tag_qt"][:4], LD), np.asarray(other["tag_qt"][4:], LD)
                        q_ct, t_ct = _compose(np.asarray(other["cam_qt"][:4], LD) / np.linalg.norm(other["cam_qt"][:4]),
                                              np.asarray(other["cam_qt"][4:], LD), qo / np.sqrt((qo * qo).sum()), to)
                        wh, resid = other["wh"], np.array(other["residual"])
                    else:
                        q_ct = rg.qmul(rg.small_quat(rng), [0.0, 1.0, 0.0, 0.0]).astype(LD)
                        t_ct = np.array([rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(2.5, 4.0)], LD)
                        wh, resid = [0.1285, 0.1285], -rng.normal(0, 0.8, 8)
                    q, t = _compose(qi, ti, q_ct, t_ct)
                    tag = np.r_[q, t].astype(np.float64)
                    _, proj, _, _ = corner_chain(intr, dist, [rec["cam_qt"]], [tag], [wh], np.zeros(8))
                    px = proj.reshape(8).astype(np.float64) - resid
                tags.append(tag)
                whs.append(wh)
                oc.append(i)
                ot.append(len(tags) - 1)
                pxs.append(px)
        return Scene(intr=np.array(intr), dist=np.array(dist), cam_qt=np.array(cams), tag_qt=np.array(tags),
                     tag_wh=np.array(whs), fixed_tag=-1, obs_cam=np.array(oc, np.int32), obs_tag=np.array(ot, np.int32),
                     obs_px=np.array(pxs))
    return cached(("hard", bool(strong)), make)
