"""Host yardstick of the localisation-accuracy prediction with correlated map tags (vmm_ba_predict_localization_joint).
numpy only: nothing here calls the engine, and there are no tests in here.

JointCase is finished_map_cases.PredictCase with the tags' joint covariance in the place of their marginals: the same
lanes scene with PREDICT_RELIEF of depth, the same cov_px and sigmas, the same metric and bound (MARGIN x the larger
deviation of the two float64 references from the longdouble truth, over all poses of the case), and

    cov_map = H^-1 M H^-1,  M = sum_{s in V} sum_{t in V} G_s S_st G_t^T,  G_t = sum over the tag's corners of Jc^T Jt

Truth.  np.longdouble: M as the full double sum over the selected set, symmetrised, between cov_cases.refined_inverse's
H^-1.  S is the matrix the entry reads: the blocks s >= t as given, S_ts = S_st^T (lower_symmetric).
Reference A.  float64: the oracle's obs_eval Jacobians, the full double sum, numpy.linalg.inv.
Reference B.  float64 in the device's scheme (kernels_predict_joint.hip's header): per s in ascending order the pairs
t < s as X_st + X_st^T with X = (G_s S_st) G_t^T, then the diagonal term (G_s S_ss) G_s^T; ref_algebra.py's
spd_inverse and sandwich.

Joint covariances
  block_diagonal   predict_cases.random_tag_cov's blocks on the diagonal, zero cross blocks
  dense_spd        a seeded dense A A^T of a map's magnitudes (millimetres, milliradians) with a strong common mode: what
                   stands in for a bundle adjustment's own where there is no device
  tiled            a (T0, T0, 6, 6) joint covariance spread over n tags (tag k takes the rows of one of `rows`, in turn):
                   P S P^T with a selection matrix P, symmetric positive semi-definite like S
  rigid            S_st = A_s Sw A_t^T: the whole map moved rigidly by a tangent w ~ Sw (rigid_tag / rigid_camera)
"""
import numpy as np

import cov_cases as cc
import finished_map_cases as fm
import predict_cases as pc
import ref_algebra as ra
import ref_geometry as rg

LD = cc.LD
JOINT_TAGS, JOINT_POSES = (1, 2, 63, 64, 65, 129), 9
SCALE = np.array([2e-3, 2e-3, 2e-3, 1e-3, 1e-3, 1e-3])   # predict_cases.random_tag_cov's magnitudes


# ---- joint covariances ---------------------------------------------------------------------------------------------------

def lower_symmetric(joint):
    """The matrix the entry reads of a (T, T, 6, 6) array: the blocks s >= t as given (the diagonal blocks in full), the
    blocks s < t the transposes of their mirror images."""
    joint = np.asarray(joint)
    T = len(joint)
    out = joint.copy()
    s, t = np.triu_indices(T, 1)
    out[s, t] = np.swapaxes(joint[t, s], 1, 2)
    return out


def dense_matrix(joint):
    """(6 T, 6 T) of a (T, T, 6, 6) block array."""
    T = len(joint)
    return np.asarray(joint).transpose(0, 2, 1, 3).reshape(6 * T, 6 * T)


def blocks(dense):
    T = len(dense) // 6
    return np.ascontiguousarray(np.asarray(dense).reshape(T, 6, T, 6).transpose(0, 2, 1, 3))


def block_diagonal(diag):
    T = len(diag)
    out = np.zeros((T, T, 6, 6))
    out[np.arange(T), np.arange(T)] = diag
    return out


def dense_spd(n_tags, seed=20261020):
    rng = np.random.default_rng(seed)
    own = 0.3 * rng.standard_normal((6 * n_tags, 6 * n_tags)) / np.sqrt(6 * n_tags)
    common = np.tile(rng.standard_normal((6, 6)), (n_tags, 1))
    B = np.hstack([own, common]) * np.tile(SCALE, n_tags)[:, None]
    return blocks(B @ B.T + 1e-8 * np.eye(6 * n_tags))


def tiled(joint, n_tags, rows):
    idx = np.asarray(rows)[np.arange(n_tags) % len(rows)]
    return np.ascontiguousarray(np.asarray(joint)[np.ix_(idx, idx)])


def rigid_tag(tag_qt, dtype=np.float64):
    """A_t: the tangent step of the tag->world pose tag_qt when the world moves by the tangent w = (d, delta), x -> R(2
    delta) x + d: the translation goes to t + d + 2 delta x t, the rotation is left-multiplied (geom.hpp's pose_plus)."""
    A = np.eye(6, dtype=dtype)
    A[:3, 3:] = -2 * rg.skew(np.asarray(tag_qt[4:], dtype))
    return A


def rigid_camera(cam_qt, dtype=np.float64):
    """B: the tangent step of the world->camera pose that moves with the world: R' = R R_w^T, t' = t - R' d."""
    R = rg.rotation(cam_qt, dtype)
    B = np.zeros((6, 6), dtype)
    B[:3, :3] = -R
    B[3:, 3:] = -R
    return B


def world_covariance(seed=20261021, translation_only=False):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((6, 6)) * SCALE[:, None]
    if translation_only:
        A[3:] = 0.0
    return A @ A.T


def rigid(tag_qt, Sw):
    A = np.array([rigid_tag(q) for q in tag_qt])
    return np.einsum("sab,bc,tdc->stad", A, Sw, A)


# ---- the case ---------------------------------------------------------------------------------------------------------------

class JointCase(fm.PredictCase):
    """PredictCase with `joint` (n_tags, n_tags, 6, 6) in the place of tag_cov; only its blocks s >= t count."""

    def __init__(self, n_tags, n_poses, joint, relief=fm.PREDICT_RELIEF):
        super().__init__(n_tags, n_poses, True)
        if relief != fm.PREDICT_RELIEF:
            self.case = pc.lanes(n_tags, n_poses, relief=relief)
        self.tag_cov = None
        self.joint = np.ascontiguousarray(joint, np.float64).reshape(n_tags, n_tags, 6, 6)
        self.S = lower_symmetric(self.joint)

    def responses(self, p, vis, dtype):
        """(selected tags, H, G (m, 6, 6)) from the restated chain."""
        t, Jc, Jt = self._jacobians(p, vis, dtype)
        return t, np.einsum("mkrp,mkrq->pq", Jc, Jc), np.einsum("mkrp,mkrq->mpq", Jc, Jt)

    def truth(self, p, vis):
        t, H, G = self.responses(p, vis, LD)
        Hi, corr = cc.refined_inverse(H)
        cov_px = LD(np.float64(self.sigma_px) * np.float64(self.sigma_px)) * Hi
        M = np.einsum("spa,stab,tqb->pq", G, self.S[np.ix_(t, t)].astype(LD), G)
        prop = Hi @ (0.5 * (M + M.T)) @ Hi
        out = dict(cov=cov_px, prop=prop, H=H, M=M, correction=cc.entry_deviation(Hi + corr, Hi))
        out["sigma_pos"], out["sigma_rot"] = self._sigmas(self.case["cam_qt"][p], cov_px + prop, LD)
        return out

    def reference_a(self, O, p, vis):
        c = self.case
        t = np.flatnonzero(vis)
        H, G = np.zeros((6, 6)), []
        for k in t:
            _, Jc, Jt = O.obs_eval(c["intr"], c["dist"], c["cam_qt"][p], c["tag_qt"][k], c["tag_wh"][k], np.zeros(8))
            H += Jc.T @ Jc
            G.append(Jc.T @ Jt)
        G = np.array(G).reshape(-1, 6, 6)
        M = np.einsum("spa,stab,tqb->pq", G, self.S[np.ix_(t, t)], G)
        Hi = np.linalg.inv(H)
        cov_px = self.sigma_px ** 2 * Hi
        prop = Hi @ M @ Hi
        sp, sr = pc.host_sigmas(c["cam_qt"][p], cov_px + prop)
        return dict(cov=cov_px, prop=prop, sigma_pos=sp, sigma_rot=sr)

    def reference_b(self, p, vis):
        t, Jc, Jt = self._jacobians(p, vis, np.float64)
        P = Jc[:, :, 0, :, None] * Jc[:, :, 0, None, :] + Jc[:, :, 1, :, None] * Jc[:, :, 1, None, :]
        Hi = ra.spd_inverse(ra.ordered_sum(P.reshape(-1, 6, 6)))
        cov_px = (self.sigma_px * self.sigma_px) * Hi
        G = np.zeros((len(t), 6, 6))
        for k in range(4):
            G += Jc[:, k, 0, :, None] * Jt[:, k, 0, None, :] + Jc[:, k, 1, :, None] * Jt[:, k, 1, None, :]
        S = self.joint[np.ix_(t, t)]                       # only [s, t] with s >= t is used below
        X = (G[:, None] @ S) @ np.swapaxes(G, 1, 2)[None]    # X[s, t] = (G_s S_st) G_t^T
        terms = []
        for s in range(len(t)):
            terms += [X[s, u] + X[s, u].T for u in range(s)]
            terms.append(np.tril(X[s, s]) + np.tril(X[s, s], -1).T)   # the lower triangle, as the kernel forms it
        prop = ra.sandwich(Hi, ra.ordered_sum(np.array(terms)))
        sp, sr = self._sigmas(self.case["cam_qt"][p], cov_px + prop, np.float64)
        return dict(cov=cov_px, prop=prop, sigma_pos=float(sp), sigma_rot=float(sr))

    def sub_case(self, tags):
        """The case of the sub-map made of `tags` alone (ascending), with their joint blocks."""
        tags = np.asarray(tags)
        sub = JointCase.__new__(JointCase)
        sub.__dict__.update(self.__dict__)
        sub.case = dict(self.case, tag_qt=self.case["tag_qt"][tags], tag_wh=self.case["tag_wh"][tags])
        sub.n_tags = len(tags)
        sub.joint = np.ascontiguousarray(self.joint[np.ix_(tags, tags)])
        sub.S = lower_symmetric(sub.joint)
        return sub


def independent_prop(case, p, vis, diag):
    """The independent formula's cov_map (vmm_ba_predict_localization's) of a JointCase in longdouble: the marginals
    `diag` (n_tags, 6, 6) alone."""
    t, H, G = case.responses(p, vis, LD)
    Hi = cc.refined_inverse(H)[0]
    M = np.einsum("mpa,mab,mqb->pq", G, np.asarray(diag)[t].astype(LD), G)
    return Hi @ (0.5 * (M + M.T)) @ Hi
