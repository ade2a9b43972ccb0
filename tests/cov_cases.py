"""References and scenes for the accuracy tests of the covariance entries (test_cov_cases_cpu.py,
test_gpu_cov_accuracy.py, tools/covariance_accuracy.py): vmm_ba_covariance_blocks, vmm_ba_tag_translation_covariance and
vmm_ba_intrinsics_system.  numpy only: nothing here calls the engine, and there are no tests in here.

Input.  A covariance case starts from the float64 blocks V, U, W of the state under test -- on the GPU the ones the same
handle's eval_blocks(robustify, huber_a) returns, on the CPU eval_cases.assemble in float64 -- so the covariance stage is
measured without the evaluation (tests/linalg_cases.py's LM-step reference does the same).  vmm_ba_eval_blocks and
cov_factor_and (csrc/covariance.hip) both call launch_eval_passes(e, robustify, huber_a, false) after flush_state, on the
handle's stream, into the working copies H_cam / H_tag / W that eval_blocks then copies out and that launch_cov_prepare /
launch_elim then read: the same kernels, arguments and buffers, so the blocks a test reads are the bits the factorisation
starts from.  The one difference is around the call, not in it: cov_factor_and first writes a fresh control block
(init_ctl) and, on a handle of the block-sparse or tree-ordered path, runs with sparse_schur and chol_nz_on switched off
(CovDensePath); neither is read by launch_eval_passes' kernels at use_ctl = false.

H is the dense normal matrix over the free, active poses (cameras first, then tags), as
yardstick.free_system builds it.  The geometry of the model columns is ref_geometry.py's (conventions there).

Truth.  inv(H) in np.longdouble, in eliminated form: rows and columns scaled by powers of two near 1 / sqrt(H_ii) (exact,
and the metric below does not see it), the larger family eliminated by its 6x6 blocks, the small reduced matrix inverted by
Newton refinement of its float64 inverse, X <- X + X (I - A X), the other blocks rebuilt from
Cov_EF = -T Cov_FF, Cov_EE = H_EE^-1 + T Cov_FF T^T with T = H_EE^-1 H_EF.

Metric.  For a block (a, b): max_ij |got_ij - truth_ij| / sqrt(truth_aa,ii truth_bb,jj) -- invariant to the units of the
unknowns (the system mixes metres and radians).  Blocks that name a constant, origin or residual-free pose must be 0.

Bound.  MARGIN (8, linalg_cases.py) x the larger deviation of two float64 CPU references over ALL blocks of the case:
A, np.linalg.inv(H); B, a numpy restatement of the device's scheme for the handle's elimination (6x6 Cholesky of the
eliminated blocks, Z, S = H_FF - Z^T Z, Cholesky, [X | U] = L^-1 [I | Z^T], the Gram and transform formulas of k_cov_pair).
Never a figure that the kernels produced.
"""
import numpy as np

import eval_cases as ec
import ref_geometry as rg
import yardstick as ys
from linalg_cases import MARGIN, refined_solution

LD = np.longdouble
U64 = 2.0 ** -53
REFERENCE_CAP = 1e-9      # sanity cap on references A and B (test_cov_cases_cpu.py), not a bound of any GPU test
REFINEMENT_SHARE = 1.0 / 64


# ---- extended-precision inverses ----------------------------------------------------------------------------------------

def pow2_scale(diag):
    """Powers of two near 1 / sqrt(diag): scaling by them is exact."""
    d = np.asarray(diag, np.float64)
    return np.ldexp(1.0, -np.rint(0.5 * np.log2(d)).astype(int))


def refined_inverse(A, rounds=4):
    """(inverse, last Newton correction) of a symmetric positive definite matrix, both np.longdouble: the float64 inverse
    of the power-of-two scaled matrix, then X <- X + X (I - A X) in longdouble.  Also for stacks of matrices."""
    A = np.asarray(A, LD)
    s = pow2_scale(np.diagonal(A, axis1=-2, axis2=-1).astype(np.float64)).astype(LD)
    As = s[..., :, None] * A * s[..., None, :]
    X = np.linalg.inv(As.astype(np.float64)).astype(LD)
    eye = np.eye(A.shape[-1], dtype=LD)
    corr = np.zeros_like(X)
    for _ in range(rounds):
        corr = X @ (eye - As @ X)
        X = X + corr
    X = 0.5 * (X + np.swapaxes(X, -1, -2))
    return s[..., :, None] * X * s[..., None, :], s[..., :, None] * corr * s[..., None, :]


def entry_deviation(got, truth, d_rows=None, d_cols=None):
    """max_ij |got_ij - truth_ij| / sqrt(d_rows_i d_cols_j); d defaults to the diagonal of truth."""
    truth = np.asarray(truth, LD)
    d_rows = np.diag(truth) if d_rows is None else np.asarray(d_rows, LD)
    d_cols = d_rows if d_cols is None else np.asarray(d_cols, LD)
    return float(np.max(np.abs(np.asarray(got).astype(LD) - truth) / np.sqrt(d_rows[:, None] * d_cols[None, :])))


def eliminated_inverse(H, n_front):
    """inv(H) in longdouble for H = [[cameras, W], [W^T, tags]] with 6x6 block-diagonal families, the first n_front
    rows being the cameras.  Returns (inverse, last Newton correction of the reduced inverse in the metric)."""
    n = len(H)
    s = pow2_scale(np.diag(H)).astype(LD)
    Hs = s[:, None] * np.asarray(H, LD) * s[None, :]
    front = np.arange(n_front)
    back = np.arange(n_front, n)
    e, f = (front, back) if n_front >= n - n_front else (back, front)
    if len(e) == 0 or len(f) == 0:
        X, corr = refined_inverse(Hs)
        return s[:, None] * X * s[None, :], entry_deviation(X + corr, X)
    ne = len(e) // 6
    E = Hs[np.ix_(e, e)].reshape(ne, 6, ne, 6)[np.arange(ne), :, np.arange(ne), :]
    Einv, _ = refined_inverse(E)
    Hef = Hs[np.ix_(e, f)].reshape(ne, 6, len(f))
    T = Einv @ Hef                                               # H_EE^-1 H_EF, block row by block row
    S = Hs[np.ix_(f, f)] - np.einsum("eaf,eag->fg", Hef, T)
    S = 0.5 * (S + S.T)
    Cff, corr = refined_inverse(S)
    T2 = T.reshape(len(e), len(f))
    Cef = -(T2 @ Cff)
    Cee = -(Cef @ T2.T)
    for k in range(ne):
        Cee[6 * k:6 * k + 6, 6 * k:6 * k + 6] += Einv[k]
    Cee = 0.5 * (Cee + Cee.T)
    X = np.zeros((n, n), LD)
    X[np.ix_(e, e)], X[np.ix_(e, f)], X[np.ix_(f, e)], X[np.ix_(f, f)] = Cee, Cef, Cef.T, Cff
    return s[:, None] * X * s[None, :], entry_deviation(Cff + corr, Cff)


def device_model(H, n_front, eliminate_front):
    """Reference B: the device's scheme in float64 (kernels_cov.hip's header) on the free system."""
    H = np.asarray(H, np.float64)
    n = len(H)
    e = np.arange(n_front) if eliminate_front else np.arange(n_front, n)
    f = np.arange(n_front, n) if eliminate_front else np.arange(n_front)
    ne = len(e) // 6
    Linv_e = np.zeros((len(e), len(e)))
    for k in range(ne):
        b = e[6 * k:6 * k + 6]
        Linv_e[6 * k:6 * k + 6, 6 * k:6 * k + 6] = np.tril(np.linalg.solve(np.linalg.cholesky(H[np.ix_(b, b)]), np.eye(6)))
    Z = Linv_e @ H[np.ix_(e, f)]
    S = H[np.ix_(f, f)] - Z.T @ Z
    L = np.linalg.cholesky(0.5 * (S + S.T))
    XU = np.linalg.solve(L, np.hstack([np.eye(len(f)), Z.T]))
    X, Um = np.tril(XU[:, :len(f)]), XU[:, len(f):]
    out = np.zeros((n, n))
    out[np.ix_(f, f)] = X.T @ X
    out[np.ix_(e, f)] = -(Linv_e.T @ (Um.T @ X))
    out[np.ix_(f, e)] = out[np.ix_(e, f)].T
    out[np.ix_(e, e)] = Linv_e.T @ (np.eye(len(e)) + Um.T @ Um) @ Linv_e
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------

class CovScene(ec.Scene):
    """eval_cases.Scene (cam_qt, tag_qt, ...) + name, robust, mask, cam_const, tag_const."""


def _from_synthetic(name, s, robust=False, mask=None):
    return CovScene(name=name, intr=s.intr, dist=s.dist, cam_qt=s.cam_gt, tag_qt=s.tag_gt, tag_wh=s.tag_wh, fixed_tag=0,
                    obs_cam=s.obs_cam, obs_tag=s.obs_tag, obs_px=s.obs_px, robust=robust, mask=mask, cam_const=None,
                    tag_const=None)


def _weak_mask(s):
    """Tag 11 and camera 23 keep exactly one observation each (not of each other, not of the origin tag)."""
    m = np.ones(len(s.obs_cam), np.uint8)
    of_tag = np.flatnonzero((s.obs_tag == 11) & (s.obs_cam != 23))
    of_cam = np.flatnonzero((s.obs_cam == 23) & (s.obs_tag != 11) & (s.obs_tag != 0))
    m[s.obs_tag == 11] = 0
    m[s.obs_cam == 23] = 0
    m[of_tag[0]] = 1
    m[of_cam[0]] = 1
    return m


def _ragged(name, few):
    s = ec.ragged_scene(few)
    cc, tc = ec.ragged_constants(s)
    return CovScene(name=name, intr=s.intr, dist=s.dist, cam_qt=s.cam_qt, tag_qt=s.tag_qt, tag_wh=s.tag_wh,
                    fixed_tag=s.fixed_tag, obs_cam=s.obs_cam, obs_tag=s.obs_tag, obs_px=s.obs_px, robust=False, mask=None,
                    cam_const=cc, tag_const=tc, few=few, last_of_65=s.last_of_65)


def _make_scene(name):
    from visual_marker_mapping_amd.synthetic import make_scene
    if name == "20x10":
        return _from_synthetic(name, make_scene(1))
    if name == "24x12":
        return _from_synthetic(name, make_scene(1, n_cams=24, n_tags=12, visibility=0.7))
    if name == "24x12_robust":
        return _from_synthetic(name, make_scene(5, n_cams=24, n_tags=12, visibility=0.7), robust=True)
    if name == "24x12_weak":
        s = make_scene(1, n_cams=24, n_tags=12, visibility=0.7)
        return _from_synthetic(name, s, mask=_weak_mask(s))
    if name == "24x12_sparse_view":
        return _from_synthetic(name, make_scene(2, n_cams=24, n_tags=12, neighbors_min=2, neighbors_max=3))
    if name == "44x10":
        return _from_synthetic(name, make_scene(1, n_cams=44, n_tags=10, visibility=0.6))
    if name == "10x44":
        return _from_synthetic(name, make_scene(1, n_cams=10, n_tags=44, visibility=0.6))
    if name == "ragged_tags":
        return _ragged(name, "tags")
    if name == "ragged_cams":
        return _ragged(name, "cams")
    raise KeyError(name)


# name: the eliminations the GPU tests run it under (the issue's table)
SCENES = {
    "20x10": ("cams", "tags"),
    "24x12": ("cams", "tags"),
    "24x12_robust": ("cams", "tags"),
    "24x12_weak": ("cams", "tags"),
    "24x12_sparse_view": ("cams", "tags"),
    "44x10": ("tags", "cams"),      # tags eliminated: 264 kept rows, n_pad 320 > 256
    "10x44": ("cams", "tags"),      # cameras eliminated: 264 kept rows
    "ragged_tags": ("cams", "tags"),
    "ragged_cams": ("cams", "tags"),
}


def scene(name):
    return ec.cached(("cov scene", name), lambda: _make_scene(name))


def cpu_blocks(sc):
    """The float64 blocks of the scene without a GPU (eval_cases' reference B)."""
    return ec.assemble(sc, robust=sc.robust, dtype=np.float64, mask=sc.mask, cam_const=sc.cam_const, tag_const=sc.tag_const)


def free_poses(sc):
    """(free cameras, free tags): not constant, not the origin, at least one observation that is switched on."""
    cc, tc = ec.flags(sc, sc.cam_const, sc.tag_const)
    on = np.ones(sc.n_obs, bool) if sc.mask is None else np.asarray(sc.mask) != 0
    seen_c = np.bincount(sc.obs_cam[on], minlength=len(sc.cam_qt)) > 0
    seen_t = np.bincount(sc.obs_tag[on], minlength=len(sc.tag_qt)) > 0
    return np.flatnonzero(~cc & seen_c), np.flatnonzero(~tc & seen_t)


def free_system(sc, blk):
    """Dense H over the free poses (cameras, then tags) from V, U, W by yardstick.free_system; the blocks of every other
    pose and of every switched-off observation must be zero.  Returns (H, free cameras, free tags)."""
    fc, ft = free_poses(sc)
    on = np.ones(sc.n_obs, bool) if sc.mask is None else np.asarray(sc.mask) != 0
    held_c, held_t = np.ones(len(sc.cam_qt), bool), np.ones(len(sc.tag_qt), bool)
    held_c[fc], held_t[ft] = False, False
    assert not np.asarray(blk["V"])[held_c].any() and not np.asarray(blk["U"])[held_t].any()
    assert not np.asarray(blk["W"])[held_c[sc.obs_cam] | held_t[sc.obs_tag] | ~on].any()
    return ys.free_system(sc, blk, held_c, held_t)[0], fc, ft


class Case:
    """One scene under one elimination, from the float64 blocks of its state: H, the longdouble inverse, the deviations of
    references A and B over all blocks, the bound.  Pose indices are the entry's: cameras, then tags."""

    def __init__(self, sc, elim, blk):
        self.scene, self.elim = sc, elim
        self.n_cams, self.n_tags = len(sc.cam_qt), len(sc.tag_qt)
        self.input_bytes = b"".join(np.asarray(blk[k], np.float64).tobytes() for k in ("V", "U", "W"))
        self.H, fc, ft = free_system(sc, blk)
        self.order = len(self.H)
        self.pos = {int(c): 6 * k for k, c in enumerate(fc)}
        self.pos.update({self.n_cams + int(t): 6 * (len(fc) + k) for k, t in enumerate(ft)})
        self.min_eig = float(np.linalg.eigvalsh(self.H).min())
        self.truth, self.last_correction = eliminated_inverse(self.H, 6 * len(fc))
        self.diag = np.diag(self.truth)
        self.refs = {"A lapack inverse": entry_deviation(np.linalg.inv(self.H), self.truth),
                     "B device scheme": entry_deviation(device_model(self.H, 6 * len(fc), elim == "cams"), self.truth)}
        self.bound = MARGIN * max(self.refs.values())

    def free(self, p):
        return int(p) in self.pos

    def block(self, a, b):
        """truth block (longdouble) or None for a pair that names a pose outside the free set."""
        if not (self.free(a) and self.free(b)):
            return None
        i, j = self.pos[int(a)], self.pos[int(b)]
        return self.truth[i:i + 6, j:j + 6]

    def block_deviation(self, a, b, got, rows=6):
        """Deviation of a 6x6 block (or its leading rows x rows part) in the metric; None for a pair outside the free set."""
        t = self.block(a, b)
        if t is None:
            return None
        i, j = self.pos[int(a)], self.pos[int(b)]
        return entry_deviation(np.asarray(got)[:rows, :rows], t[:rows, :rows], self.diag[i:i + rows], self.diag[j:j + rows])

    def check(self, pairs, cov, label, out=print):
        """Every block of a covariance_blocks result: free pairs within the bound, the others exactly zero.  Prints the
        worst deviation, the bound and their ratio; returns (failures, worst deviation)."""
        bad, worst = [], 0.0
        for (a, b), got in zip(np.asarray(pairs).tolist(), cov):
            dev = self.block_deviation(a, b, got)
            if dev is None:
                if np.asarray(got).any():
                    bad.append("%s (%d, %d): a block of a constant, origin or residual-free pose is not zero" % (label, a, b))
                continue
            worst = max(worst, dev)
            if not dev <= self.bound:
                bad.append("%s (%d, %d): deviation %.3e above the bound %.3e" % (label, a, b, dev, self.bound))
        out("%s: order %d, %d blocks, deviation %.3e  bound %.3e  ratio %.3f" % (label, self.order, len(cov), worst, self.bound,
                                                                               worst / self.bound))
        return bad, worst


def cpu_case(name, elim):
    return ec.cached(("cov cpu case", name, elim), lambda: Case(scene(name), elim, cpu_blocks(scene(name))))


def device_case(ba, sc, elim):
    """The case of a handle (scene sc under elimination elim, mask and constants set) from its own eval_blocks; built once
    per (scene, elimination) and checked to belong to the same bits afterwards."""
    blk = ba.eval_blocks(robustify=sc.robust)
    case = ec.cached(("cov device case", sc.name, elim), lambda: Case(sc, elim, blk))
    assert case.input_bytes == b"".join(np.asarray(blk[k], np.float64).tobytes() for k in ("V", "U", "W"))
    return case


def all_pairs(n):
    up = [(a, b) for a in range(n) for b in range(a, n)]
    return np.array(up + [(b, a) for a, b in up if a != b], np.int32)


def marginals_and_cross(n, n_cross=60, seed=20261104, extra=()):
    """Every marginal, n_cross cross pairs drawn with a fixed seed, and `extra`."""
    rng = np.random.default_rng(seed)
    cross = []
    while len(cross) < n_cross:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b:
            cross.append((a, b))
    return np.array([(p, p) for p in range(n)] + cross + list(extra), np.int32)


# ---- the camera-model system ---------------------------------------------------------------------------------------------

def model_columns(intr, dist, cam_qt, tag_qt, wh, dtype=LD, want_magnitude=False):
    """J_k (n, 4, 2, 9) of the residuals over (fx, fy, cx, cy, k1, k2, p1, p2, k3), next to eval_cases.corner_chain's
    projection and in its notation: u = fx xd + cx, v = fy yd + cy,
    xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2).  want_magnitude: also the same
    formulas over absolute values, x and y carried through the chain as sums of absolute values."""
    intr, dist = np.asarray(intr, dtype), np.asarray(dist, dtype)
    cam_qt, tag_qt = np.asarray(cam_qt, dtype).reshape(-1, 7), np.asarray(tag_qt, dtype).reshape(-1, 7)
    wh = np.asarray(wh, dtype).reshape(-1, 2)
    two = dtype(2)
    pc, Rc, _, _ = rg.camera_points(cam_qt, tag_qt, wh, dtype, parts=True)

    def columns(x, y, fx, fy, *k):
        xd, yd, r2, _ = rg.distort(x, y, k, dtype)
        zero, one = np.zeros_like(x), np.ones_like(x)
        Ju = np.stack([xd, zero, one, zero, fx * x * r2, fx * x * r2 * r2, fx * two * x * y, fx * (r2 + two * x * x),
                       fx * x * r2 * r2 * r2], axis=-1)
        Jv = np.stack([zero, yd, zero, one, fy * y * r2, fy * y * r2 * r2, fy * (r2 + two * y * y), fy * two * x * y,
                       fy * y * r2 * r2 * r2], axis=-1)
        return np.stack([Ju, Jv], axis=-2)

    Jk = columns(pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2], intr[0], intr[1], *dist)
    if not want_magnitude:
        return Jk
    pw_m = np.einsum("nij,nkj->nki", np.abs(rg.rotation(tag_qt, dtype)), np.abs(rg.local_corners(wh, dtype))) + np.abs(tag_qt[:, None, 4:])
    pc_m = np.einsum("nij,nkj->nki", np.abs(Rc), pw_m) + np.abs(cam_qt[:, None, 4:])
    iz = dtype(1) / np.abs(pc[..., 2])
    return Jk, columns(pc_m[..., 0] * iz, pc_m[..., 1] * iz, abs(intr[0]), abs(intr[1]), *np.abs(dist))


def border_sums(sc, k, robust, mask, dtype):
    """A (dense, over the free poses), B (rows of A x 9), g, C, g_k, cost in `dtype` from the restated chain."""
    s = CovScene(**dict(sc.__dict__, intr=np.asarray(k[:4], np.float64), dist=np.asarray(k[4:], np.float64), mask=mask,
                        robust=robust))
    r, _, Jc, Jt = ec.corner_chain(s.intr, s.dist, s.cam_qt[s.obs_cam], s.tag_qt[s.obs_tag], s.tag_wh[s.obs_tag], s.obs_px,
                                   dtype)
    Jk = model_columns(s.intr, s.dist, s.cam_qt[s.obs_cam], s.tag_qt[s.obs_tag], s.tag_wh[s.obs_tag], dtype)
    on = np.ones(s.n_obs, bool) if mask is None else np.asarray(mask) != 0
    sq = (r * r).sum(axis=-1)
    rho = ec.huber(1.0, sq, dtype) if robust else np.stack([sq, np.ones_like(sq), np.zeros_like(sq)], axis=-1)
    w2 = np.where(on[:, None], rho[..., 1], dtype(0))
    cost = np.where(on[:, None], rho[..., 0] / dtype(2), dtype(0)).sum(dtype=dtype)
    fc, ft = free_poses(s)
    pos_c = -np.ones(len(s.cam_qt), int)
    pos_c[fc] = np.arange(len(fc))
    pos_t = -np.ones(len(s.tag_qt), int)
    pos_t[ft] = len(fc) + np.arange(len(ft))
    n = 6 * (len(fc) + len(ft))
    A, B, g = np.zeros((n, n), dtype), np.zeros((n, 9), dtype), np.zeros(n, dtype)
    Jkw = Jk * w2[:, :, None, None]
    C = np.einsum("nkrp,nkrq->pq", Jkw, Jk)
    gk = np.einsum("nkrp,nkr->p", Jkw, r)
    for i, (c, t) in enumerate(zip(s.obs_cam.tolist(), s.obs_tag.tolist())):
        if not on[i]:
            continue
        parts = [(pos_c[c], Jc[i]), (pos_t[t], Jt[i])]
        for p, J in parts:
            if p < 0:
                continue
            Jw = J * w2[i][:, None, None]
            A[6 * p:6 * p + 6, 6 * p:6 * p + 6] += np.einsum("krp,krq->pq", Jw, J)
            B[6 * p:6 * p + 6] += np.einsum("krp,krq->pq", Jw, Jk[i])
            g[6 * p:6 * p + 6] += np.einsum("krp,kr->p", Jw, r[i])
        if pos_c[c] >= 0 and pos_t[t] >= 0:
            Wi = np.einsum("krp,krq->pq", Jc[i] * w2[i][:, None, None], Jt[i])
            a, b = 6 * pos_c[c], 6 * pos_t[t]
            A[a:a + 6, b:b + 6] += Wi
            A[b:b + 6, a:a + 6] += Wi.T
    return A, B, g, C, gk, cost


def _model_measures(Sk, rk):
    """(inv(S_k), inv(S_k) r_k) in longdouble from a system given in any precision (the inversion adds no error)."""
    cov, _ = refined_inverse(np.asarray(Sk, LD))
    return cov, cov @ np.asarray(rk, LD)


class ModelCase:
    """vmm_ba_intrinsics_system on one scene at camera model k: the longdouble S_k, r_k, the deviations of references A
    (yardstick.reduced_system on the oracle's Jacobian) and B (float64 Y = L^-1 [B | g], S_k = C - Y^T Y) in the two
    metrics -- inv(S_k) entry by entry over sqrt(c_ii c_jj), the step inv(S_k) r_k in units of sqrt(c_ii) -- and the bounds
    MARGIN x the larger deviation."""

    def __init__(self, O, sc, k, robust, mask):
        self.scene, self.k, self.robust, self.mask = sc, np.asarray(k, np.float64), robust, mask
        A, B, g, C, gk, cost = border_sums(sc, self.k, robust, mask, LD)
        X = refined_solution(A.astype(np.float64), np.column_stack([B, g]))
        # refined_solution's residual is against the float64 rounding of A: two more rounds against A itself
        A64 = A.astype(np.float64)
        Li = np.tril(np.linalg.solve(np.linalg.cholesky(A64), np.eye(len(A64))))
        rhs = np.column_stack([B, g])
        for _ in range(4):
            R = rhs - A @ X
            X = X + (Li.T @ (Li @ R.astype(np.float64))).astype(LD)
        self.Sk, self.rk = C - B.T @ X[:, :9], gk - B.T @ X[:, 9]
        self.Sk = 0.5 * (self.Sk + self.Sk.T)
        self.cov, self.step = _model_measures(self.Sk, self.rk)
        self.sigma = np.sqrt(np.diag(self.cov))
        # reference A and the oracle's float64 quantities for C, g_k and the cost (test_gpu_selfcal.py's comparison)
        on = None if mask is None else np.asarray(mask) != 0
        n6 = 6 * (len(sc.cam_qt) + len(sc.tag_qt))
        cc, tc = ec.flags(sc, sc.cam_const, sc.tag_const)
        o_cost, r, J, rmag = ys.joint_system(O, self.k, sc.cam_qt, sc.tag_qt, sc.tag_wh, sc.fixed_tag, sc.obs_cam, sc.obs_tag,
                                          sc.obs_px, robust, obs_on=on, cam_const=cc, tag_const=tc, want_magnitude=True)
        gk_o, C_o, rk_o, Sk_o = ys.reduced_system(r, J, n6)
        Jk_abs = np.abs(J[:, n6:])
        self.oracle = dict(cost=o_cost, g_k=gk_o, C=C_o, mag_C=Jk_abs.T @ Jk_abs, mag_g=Jk_abs.T @ rmag)
        A6, B6, g6, C6, gk6, _ = border_sums(sc, self.k, robust, mask, np.float64)
        Y = np.linalg.solve(np.linalg.cholesky(A6), np.column_stack([B6, g6]))
        self.refs = {"A oracle reduced_system": self.deviation(Sk_o, rk_o),
                     "B device form": self.deviation(C6 - Y[:, :9].T @ Y[:, :9], gk6 - Y[:, :9].T @ Y[:, 9])}
        self.bound_cov = MARGIN * max(d[0] for d in self.refs.values())
        self.bound_step = MARGIN * max(d[1] for d in self.refs.values())

    def deviation(self, Sk, rk):
        """(inv(S_k) in the entry metric, the step in standard deviations) against the longdouble system."""
        cov, step = _model_measures(Sk, rk)
        return (entry_deviation(cov, self.cov), float(np.max(np.abs(step - self.step) / self.sigma)))


MODEL_VARIANTS = (("plain", False, False), ("robust", True, False), ("masked", True, True))


def model_case(O, name, variant):
    """ragged_tags / ragged_cams with ragged_constants at k = truth + 0.01 PERTURB (test_system_matches_the_host_jacobian):
    plain, robust, and robust with ragged_mask."""
    label, robust, masked = next(v for v in MODEL_VARIANTS if v[0] == variant)

    def make():
        sc = scene(name)
        k = np.concatenate([sc.intr, sc.dist]) + 0.01 * ys.PERTURB
        return ModelCase(O, sc, k, robust, ec.ragged_mask(sc) if masked else None)
    return ec.cached(("cov model case", name, label), make)


# ---- the request edges of vmm_ba_covariance_blocks on the 24 x 12 scenes --------------------------------------------------

def chunks_at(n_cams, n_tags, elim, pairs):
    """The host side of vmm_ba_covariance_blocks restated: the distinct poses of the request take slots (six columns each),
    eliminated family first, then the kept poses by ascending row; a 64-column chunk starts at the first block row in which
    any of its slots is non-zero (0 for an eliminated pose, 6 family_index / 64 for a kept one); chunks_at[k] = the number of
    leading chunks that block row k of the substitution works on (0: its launches are skipped)."""
    n_kept = n_tags if elim == "cams" else n_cams
    n_blk = (6 * n_kept + 63) // 64
    eliminated = (lambda p: p < n_cams) if elim == "cams" else (lambda p: p >= n_cams)
    poses = sorted({int(p) for p in np.asarray(pairs).reshape(-1)}, key=lambda p: (not eliminated(p), p))
    n_chunks = (6 * len(poses) + 63) // 64
    first = [n_blk] * n_chunks
    for s, p in enumerate(poses):
        row = 0 if eliminated(p) else 6 * (p if p < n_cams else p - n_cams) // 64
        for c in range(6 * s // 64, (6 * s + 5) // 64 + 1):
            first[c] = min(first[c], row)
    return [sum(1 for c in range(n_chunks) if all(first[d] <= k for d in range(c + 1))) for k in range(n_blk)], poses


def edge_requests(elim, n_cams=24, n_tags=12):
    """[(label, pairs, chunks_at the request produces)] on a 24 x 12 scene.  K i / E i: the kept / eliminated pose of family
    index i.  Tags eliminated: 24 kept cameras, 144 rows, three block rows; cameras eliminated: 12 kept tags, 72 rows, two."""
    K = (lambda i: n_cams + i) if elim == "cams" else (lambda i: i)
    E = (lambda i: i) if elim == "cams" else (lambda i: n_cams + i)
    t = elim == "tags"

    def req(poses, extra=()):
        chain = [(a, b) for a, b in zip(poses[:-1], poses[1:])]
        return np.array([(p, p) for p in poses] + chain + [(b, a) for a, b in chain[::3]] + list(extra), np.int32)
    out = [
        # rows 60 .. 65 straddle block rows 0 and 1; one slot, one chunk from block row 0 on
        ("kept pose 10 alone", req([K(10)]), [1, 1, 1] if t else [1, 1]),
        # nothing to do before the last block row
        ("last block row only", req([K(22), K(23)] if t else [K(11)]), [0, 0, 1] if t else [0, 1]),
        # 13 slots, two chunks, slot 10 (camera 21) across them; with the cameras eliminated tag 11 is the only such pose
        ("block rows >= 1 only", req([K(i) for i in range(11, 24)] if t else [K(11), K(11)]), [0, 2, 2] if t else [0, 1]),
        # slot 10 = columns 60 .. 65 across chunks 0 and 1
        ("11 poses, slot 10 eliminated", req([E(i) for i in range(11)]), [2, 2, 2] if t else [2, 2]),
        ("11 poses, slot 10 kept", req([E(i) for i in (1, 2, 3, 4)] + [K(i) for i in ((0, 5, 10, 11, 15, 21, 23) if t else
                                                                                      (1, 3, 5, 7, 9, 10, 11))]),
         [1, 1, 2] if t else [1, 2]),
        # 132 columns: three chunks, the last pair of k_trsm_update_mfma half empty
        ("22 slots", req([E(i) for i in range(1, 9)] + [K(i) for i in range(14)] if t else
                         [E(i) for i in range(10)] + [K(i) for i in range(12)]), [2, 3, 3] if t else [2, 3]),
        # 192 columns: three full chunks
        ("32 slots", req([E(i) for i in range(12)] + [K(i) for i in range(4, 24)] if t else
                         [E(i) for i in range(20)] + [K(i) for i in range(12)]), [2, 3, 3] if t else [3, 3]),
        # 198 columns: four chunks, six columns in the last
        ("33 slots", req([E(i) for i in range(12)] + [K(i) for i in range(3, 24)] if t else
                         [E(i) for i in range(21)] + [K(i) for i in range(12)]), [2, 3, 4] if t else [3, 4]),
    ]
    return out
