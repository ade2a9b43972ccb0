"""Scenes, longdouble truth and float64 references for the accuracy tests of the two joint refinements over the arrowhead
solver (test_arrowhead_cases_cpu.py, test_gpu_arrowhead_accuracy.py, tools/arrowhead_accuracy.py): vmm_ba_calibrate (the
nine numbers of the camera model and one pose per image) and vmm_ba_rig_calibrate (6 K extrinsic parameters and one rig
pose per frame).  numpy only: nothing here calls the engine, and there are no tests in here.

Input.  Everything the two entries report is a function of a STATE (the shared unknowns and one pose per item), a FLAG
SET (the inlier observations) and a PARTICIPATION SET (the items that take part): on the GPU the device's own, read bit
for bit, on the CPU the start or the host optimum.  At that state

    H = sum rho' J^T J over all 6 n_part + P_free unknowns at once, g = sum rho' J^T r
    H^-1                       its lower-right block is intr_cov / ext_cov, its diagonal 6 x 6 blocks cam_cov / rig_cov
    cost_i = 1/2 sum rho, rms_i = sqrt(sum |r|^2 / (4 n_inlier))      and their totals: final_cost, final_rms_px
    1/2 g^T H^-1 g             the Gauss-Newton decrement: what is left to gain
    -(H + lam diag H)^-1 g     one Levenberg-Marquardt trial at lam = kLamInit (small_solve.hpp), over the free columns;
                               the candidate is k + dk and pose_plus of every pose and extrinsic

Truth.  np.longdouble: eval_cases.corner_chain for the residuals and the pose columns (for the rig the camera stands at
ext_c o rig_f and the columns are turned by ref_geometry.turn_to_rig, as finished_map_cases.RigCase.chain's),
cov_cases.model_columns for the nine model columns, and ref_geometry.extrinsic_columns, derived from vmm_ba.h's definition: extrinsic c moves in its own
tangent as vmm_ba_pose_plus moves a pose, so a step (ds, dphi) gives t_c + ds and R(2 dphi) R_c, the camera
R(2 dphi) R_c R_f, R(2 dphi) R_c t_f + t_c + ds: it moves by (ds + 2 dphi x (R_c t_f), dphi) in its own tangent, and
J_ext = [Jc_t | Jc_r - 2 Jc_t [R_c t_f]x].  The whole matrix is inverted at once (whole_inverse: cov_cases.refined_inverse,
and for orders above DENSE_LIMIT the same Newton iteration with the residual in longdouble over the arrow's blocks and the
correction multiplied in float64) -- deliberately not the device's scheme, which eliminates every item and uses
A^-1 + A^-1 B S^-1 B^T A^-1.

References (B's small algebra and summation orders: ref_algebra.py).  A: the oracle's functor through yardstick.calib_system / rig_cases.rig_system with np.linalg.inv and
np.linalg.solve on the full matrix; the per-item cost and rms through finished_map_cases' reference A.  B: the device's
scheme in float64, read from arrowhead.hpp, kernels_calibrate.hip and kernels_rig.hip: row pairs scaled by sqrt(rho'), sums
in list order, the damped 6 x 6 Cholesky per item, Y = L^-1 B, y = L^-1 g, the records C_i - Y'Y, g_s - Y'y summed in four
interleaved chains combined ((0 + 1) + 2) + 3, Jacobi scaling with unit rows for the inactive unknowns, Cholesky, L^-1, its
Gram matrix, rescaled; L^-T (I + Y S^-1 Y') L^-1; the step by forward and backward substitution and arrow_pose_step.

Metric.  A covariance entry |got - truth| / sqrt(truth_ii truth_jj) (cov_cases.entry_deviation: invariant to the units, the
point for intr_cov, whose variances span ten orders of magnitude); cost and rms relative; a step component
|got - truth| sqrt(H_jj), the difference of two poses taken by a longdouble pose_minus, that of two models k - k'.
Bound.  MARGIN (8) x the larger deviation of A and B over all items of the case.  Never a figure the kernels produced.
"""
import numpy as np

import cov_cases as cc
import eval_cases as ec
import finished_map_cases as fm
import ref_algebra as ra
import ref_geometry as rg
import rig_cases as rc
import yardstick as ys
from ref_geometry import pose_minus, pose_plus

LD = cc.LD
MARGIN = ec.MARGIN
LAM_INIT = 1e-3             # kLamInit, small_solve.hpp
# The start of every case: the truth + START x yardstick.PERTURB.  Not 0.25: from there the first step is 900 standard
# deviations long (the cost falls from 9.6e5 to 9.2e2), and reference A's float64 solve of it sits at 1.1e-9 standard
# deviations, above cov_cases.REFERENCE_CAP, which is absolute in that metric (pinhole, plain, all nine free)
START = 0.05
# The start of the extrinsics the mask frees: the truth moved by START x this tangent (metres, half-angle radians), its
# sign alternating with the camera; a held extrinsic starts at the truth.  Half a millimetre and a third of a
# milliradian: a frame of one tag takes no part, keeps the pose the localisation fitted to that one tag under the start
# extrinsics, and is classified again under the refined ones -- at 1.7 mm and 1 mrad (the first choice here) its flag
# came back as an outlier's on the device, which the placed labels do not allow for
EXT_PERTURB = np.array([0.01, -0.008, 0.006, 0.002, -0.003, 0.0015])
DENSE_LIMIT = 640           # orders above it: whole_inverse's mixed iteration (longdouble matmul is cubic and unblocked)
ITEM_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 257)      # k_calib_solve's chains, the 64-thread kernels, arrow_control's stride
# Tags per image of the item edges.  Not 6: from the same six tags in every image the scaled H has a condition of 2e6 to
# 6e6, and the truth's last Newton correction (condition x 2^-64) came to 1 / 64 of the larger reference at 63 images,
# the whole of its share; twelve tags bring the condition to 4e5 .. 7e5
TAGS_PER_IMAGE = 12
FRAME_COUNTS = (1, 4, 5, 65)
RIG_CAMS = (2, 3, 4, 8)
# Observations of the last camera of the added frame.  camera_normal_sums' second trip begins at the camera's 257th, but
# the frame's last observation is an outlier by the placement rule: one more, so that an inlier is summed on that trip
SECOND_TRIP = 258
QUANTITIES = ("cost", "rms", "shared_cov", "item_cov", "step_shared", "step_pose")
REFS = ("A oracle, numpy inverse", "B device scheme")


# ---- the inverse of the whole matrix -----------------------------------------------------------------------------------------

def _arrow_product(As, n_items, X):
    """As @ X in longdouble for As = [[blockdiag(A_i), B], [B^T, C]] with n_items 6 x 6 blocks, block by block."""
    n6 = 6 * n_items
    A = As[:n6, :n6].reshape(n_items, 6, n_items, 6)[np.arange(n_items), :, np.arange(n_items), :]
    B, C = As[:n6, n6:], As[n6:, n6:]
    top = np.einsum("jab,jbn->jan", A, X[:n6].reshape(n_items, 6, -1)).reshape(n6, -1) + B @ X[n6:]
    return np.concatenate([top, B.T @ X[:n6] + C @ X[n6:]])


def whole_inverse(H, n_items, force_mixed=False):
    """(inverse, last Newton correction) of the arrowhead H (n_items 6 x 6 blocks, then the shared unknowns), longdouble.
    Up to DENSE_LIMIT: cov_cases.refined_inverse.  Above: the same scaling and start, X <- X + X0 (I - H X) with the
    residual in longdouble (block by block: nothing of H is left out) and X0, the float64 inverse, applied in float64; the
    error shrinks by |I - X0 H| (condition x 2^-53) per round."""
    H = np.asarray(H, LD)
    if len(H) <= DENSE_LIMIT and not force_mixed:
        return cc.refined_inverse(H)
    s = cc.pow2_scale(np.diag(H).astype(np.float64)).astype(LD)
    As = s[:, None] * H * s[None, :]
    X0 = np.linalg.inv(As.astype(np.float64))
    X, eye = X0.astype(LD), np.eye(len(H), dtype=LD)
    corr = np.zeros_like(X)
    for _ in range(4):
        corr = (X0 @ (eye - _arrow_product(As, n_items, X)).astype(np.float64)).astype(LD)
        X = X + corr
    X = 0.5 * (X + X.T)
    return s[:, None] * X * s[None, :], s[:, None] * corr * s[None, :]


def _rel(got, truth):
    return float(abs(LD(got) - truth) / truth)


# ---- a case ----------------------------------------------------------------------------------------------------------------

class ArrowCase:
    """One scene of one entry under one loss and one refine_mask.  The subclasses say what the shared unknowns are."""

    def __init__(self, scene, loss, mask, exercises):
        self.scene, self.loss, self.mask, self.exercises = scene, loss, mask, exercises
        self.robust, self.a = fm.LOSSES[loss]
        self.n_items = len(scene.start) - 1

    def span(self, i):
        return int(self.scene.start[i]), int(self.scene.start[i + 1])

    loss_terms = fm.Case.loss_terms

    def flags_list(self, obs_flags):
        return [np.asarray(obs_flags[slice(*self.span(i))], bool) for i in range(self.n_items)]

    def participants(self, flags, min_inlier_tags=2):
        return [int(f.sum()) >= min_inlier_tags for f in flags]

    # -- sums per item, any precision --
    def item_sums(self, i, shared, pose, on, dtype, ordered=False):
        """N ((6 + P) x (6 + P): A, B, C_i), gradient (6 + P), sum rho, sum |r|^2 of item i over the flagged observations;
        the held columns are zero.  ordered: rows scaled by sqrt(rho') and summed corner by corner in list order."""
        r, Jp, Js = self.columns(i, shared, pose, dtype)
        J = np.concatenate([Jp, np.where(self.held(), dtype(0), Js)], axis=-1)[on]
        r = r[on]
        sq, rho0, rho1 = self.loss_terms(r, dtype)
        if not ordered:
            return (np.einsum("mk,mkrp,mkrq->pq", rho1, J, J), np.einsum("mk,mkrp,mkr->p", rho1, J, r), rho0.sum(dtype=dtype),
                    sq.sum(dtype=dtype))
        w = np.sqrt(rho1)
        J, r = J * w[..., None, None], r * w[..., None]
        n = J.shape[-1]
        N = np.zeros((n, n))
        for m in range(0, len(J), 64):      # in pieces: a frame of 513 observations at P = 48 is 48 MB of products at once
            Pm = J[m:m + 64, :, 0, :, None] * J[m:m + 64, :, 0, None, :] + J[m:m + 64, :, 1, :, None] * J[m:m + 64, :, 1, None, :]
            N = ra.ordered_sum(np.concatenate([N[None], Pm.reshape(-1, n, n)]))
        g = ra.ordered_sum((J[:, :, 0, :] * r[:, :, 0, None] + J[:, :, 1, :] * r[:, :, 1, None]).reshape(-1, n))
        return N, g, ra.ordered_sum(rho0.reshape(-1)), ra.ordered_sum(sq.reshape(-1))

    # -- the truth --
    def truth(self, shared, poses, flags, part, lam=None):
        P = self.P
        items = [i for i in range(self.n_items) if part[i]]
        sums = {i: self.item_sums(i, shared, poses[i], flags[i], LD) for i in items}
        C = sum(sums[i][0][6:, 6:] for i in items)
        free = np.flatnonzero(~self.held() & (np.diag(C) > 0))
        n6, n = 6 * len(items), 6 * len(items) + len(free)
        H, g = np.zeros((n, n), LD), np.zeros(n, LD)
        for j, i in enumerate(items):
            N, gi = sums[i][:2]
            H[6 * j:6 * j + 6, 6 * j:6 * j + 6] = N[:6, :6]
            H[6 * j:6 * j + 6, n6:] = N[:6, 6:][:, free]
            H[n6:, 6 * j:6 * j + 6] = N[:6, 6:][:, free].T
            g[6 * j:6 * j + 6] = gi[:6]
            g[n6:] += gi[6:][free]
        H[n6:, n6:] = C[np.ix_(free, free)]
        Hi, corr = whole_inverse(H, len(items))
        n_in = {i: int(np.sum(flags[i])) for i in items}
        rho_all, sq_all, obs_all = (sum(sums[i][2] for i in items), sum(sums[i][3] for i in items), sum(n_in.values()))
        shared_cov = np.zeros((P, P), LD)
        shared_cov[np.ix_(free, free)] = Hi[n6:, n6:]
        blocks = lambda M: {i: M[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j, i in enumerate(items)}
        item_cov, item_corr = blocks(Hi), blocks(corr)
        correction = max([cc.entry_deviation(Hi[n6:, n6:] + corr[n6:, n6:], Hi[n6:, n6:])]
                         + [cc.entry_deviation(item_cov[i] + item_corr[i], item_cov[i]) for i in items])
        t = dict(items=items, free=free, n_in=n_in, H=H, g=g, inverse=Hi, correction=correction,
                 cost={i: sums[i][2] / LD(2) for i in items},
                 rms={i: np.sqrt(sums[i][3] / LD(4 * n_in[i])) for i in items},
                 final_cost=rho_all / LD(2), final_rms=np.sqrt(sq_all / LD(4 * obs_all)), n_obs_used=obs_all,
                 shared_cov=shared_cov, item_cov=item_cov, decrement=(g @ Hi @ g) / LD(2))
        if lam is not None:
            Hd = H + LD(lam) * np.diag(np.diag(H))
            Hdi, corr_d = whole_inverse(Hd, len(items))
            step = -(Hdi @ g)
            step = step - Hdi @ (Hd @ step + g)           # one more refinement of the solution itself
            ds = np.zeros(P, LD)
            ds[free] = step[n6:]
            t.update(step=step, step_correction=float(np.max(np.abs(corr_d @ g) * np.sqrt(np.diag(H)))),
                     shared_cand=self.shared_plus(shared, ds, LD),
                     pose_cand={i: pose_plus(poses[i], step[6 * j:6 * j + 6], LD) for j, i in enumerate(items)})
        return t

    def ld_cost(self, shared, poses, flags, part):
        """1/2 sum rho in longdouble at a state given in any precision that float64 holds."""
        total = LD(0)
        for i in range(self.n_items):
            if part[i]:
                r, _, _ = self.columns(i, shared, poses[i], LD)
                total += self.loss_terms(r[flags[i]], LD)[1].sum(dtype=LD)
        return total / LD(2)

    def classify(self, shared, poses):
        """(flags per item, the smallest distance of a largest corner distance from inlier_px) in longdouble."""
        out, gap = [], np.inf
        for i in range(self.n_items):
            r, _, _ = self.columns(i, shared, poses[i], LD)
            dmax = np.sqrt((r * r).sum(axis=-1).max(axis=-1))
            out.append(dmax <= LD(fm.INLIER_PX))
            gap = min(gap, float(np.abs(dmax - LD(fm.INLIER_PX)).min()))
        return out, gap

    # -- reference A --
    def reference_a(self, O, shared, poses, flags, part, lam=None):
        P, n_all = self.P, self.n_items
        items = [i for i in range(n_all) if part[i]]
        keep = np.concatenate([np.asarray(flags[i], bool) & bool(part[i]) for i in range(n_all)])
        cost, r, J = self.system_a(O, shared, poses, keep)
        H, g = J.T @ J, J.T @ r
        free = np.flatnonzero(np.diag(H)[6 * n_all:] > 0)
        cols = np.concatenate([np.arange(6 * i, 6 * i + 6) for i in items] + [6 * n_all + free])
        Hc, n6 = H[np.ix_(cols, cols)], 6 * len(items)
        inv = np.linalg.inv(Hc)
        at = self.at(shared)
        per = {i: at.reference_a(O, i, poses[i], flags[i]) for i in items}
        raw2 = sum(per[i]["rms"] ** 2 * 4 * int(np.sum(flags[i])) for i in items)
        out = dict(cost={i: per[i]["cost"] for i in items}, rms={i: per[i]["rms"] for i in items}, final_cost=cost,
                   final_rms=np.sqrt(raw2 / (4.0 * int(keep.sum()))), shared_cov=np.zeros((P, P)),
                   item_cov={i: inv[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j, i in enumerate(items)}, free=free)
        out["shared_cov"][np.ix_(free, free)] = inv[n6:, n6:]
        if lam is not None:
            step = np.linalg.solve(Hc + lam * np.diag(np.diag(Hc)), -g[cols])
            ds = np.zeros(P)
            ds[free] = step[n6:]
            out.update(shared_cand=self.shared_plus(shared, ds, np.float64),
                       pose_cand={i: pose_plus(poses[i], step[6 * j:6 * j + 6], np.float64) for j, i in enumerate(items)})
        return out

    # -- reference B --
    def reference_b(self, shared, poses, flags, part, lam=None):
        P, n_all = self.P, self.n_items
        items = [i for i in range(n_all) if part[i]]
        damp = 0.0 if lam is None else lam
        T = P * (P + 1) // 2
        rec_S, rec_g, rec_d, stat = np.zeros((n_all, P, P)), np.zeros((n_all, P)), np.zeros((n_all, P)), np.zeros((n_all, 3))
        elim = {}
        for i in items:
            N, gv, rho, sq = self.item_sums(i, shared, poses[i], flags[i], np.float64, ordered=True)
            L = ra.cholesky(ra.damped(N[:6, :6], damp))
            Yy = ra.forward(L, np.column_stack([N[:6, 6:], gv[:6]]))
            Y, y = Yy[:, :P], Yy[:, P]
            S, gs = N[6:, 6:].copy(), gv[6:].copy()
            for k in range(6):
                S = S - Y[k][:, None] * Y[k][None, :]
                gs = gs - Y[k] * y[k]
            rec_S[i], rec_g[i], rec_d[i], stat[i] = S, gs, np.diag(N[6:, 6:]), (rho, sq, float(np.sum(flags[i])))
            elim[i] = (L, Y, y)
        S, gs, Cd, st = ra.chains4(rec_S), ra.chains4(rec_g), ra.chains4(rec_d), ra.chains4(stat)
        act = ~self.held() & (self.active_probe(Cd) > 0)
        free = np.flatnonzero(act)
        d = np.where(act, np.diag(S) + damp * Cd, 1.0)
        sc = np.where(act, 1.0 / np.sqrt(d), 1.0)
        M = np.where(act[:, None] & act[None, :], S * sc[:, None] * sc[None, :], 0.0)
        M[np.diag_indices(P)] = 1.0
        out = dict(cost={i: 0.5 * stat[i, 0] for i in items}, rms={i: np.sqrt(stat[i, 1] / (4.0 * stat[i, 2])) for i in items},
                   final_cost=0.5 * st[0], final_rms=np.sqrt(st[1] / (4.0 * st[2])), free=free)
        if lam is None:
            Si = np.where(act[:, None] & act[None, :], ra.spd_inverse(M) * sc[:, None] * sc[None, :], 0.0)
            out["shared_cov"], out["item_cov"] = Si, {}
            for i in items:
                L, Y, _ = elim[i]
                W = ra.forward(L, np.eye(6))
                cov = W.T @ ((np.eye(6) + (Y @ Si) @ Y.T) @ W)
                out["item_cov"][i] = np.tril(cov) + np.tril(cov, -1).T
            return out
        Lm = ra.cholesky(M)
        ds = ra.backward(Lm, ra.forward(Lm, np.where(act, -gs * sc, 0.0))) * sc
        ds = np.where(act, ds, 0.0)
        out.update(shared_cand=self.shared_plus(shared, ds, np.float64), pose_cand={})
        for i in items:
            L, Y, y = elim[i]
            out["pose_cand"][i] = pose_plus(poses[i], ra.backward(L, -(y + Y @ ds)), np.float64)
        return out

    def active_probe(self, Cd):
        """What k_*_solve looks at to call a free column active (calibrate: nothing but the mask)."""
        return np.ones(self.P)

    # -- the metric --
    def deviation(self, got, t):
        """{quantity: the largest deviation of `got` from the truth t over its items}."""
        it, f = t["items"], t["free"]
        dev = {}
        if "cost" in got:
            dev = dict(cost=max([_rel(got["cost"][i], t["cost"][i]) for i in it] + [_rel(got["final_cost"], t["final_cost"])]),
                       rms=max([_rel(got["rms"][i], t["rms"][i]) for i in it] + [_rel(got["final_rms"], t["final_rms"])]))
        if "shared_cov" in got:
            dev["shared_cov"] = cc.entry_deviation(np.asarray(got["shared_cov"])[np.ix_(f, f)], t["shared_cov"][np.ix_(f, f)])
            dev["item_cov"] = max(cc.entry_deviation(got["item_cov"][i], t["item_cov"][i]) for i in it)
        if "shared_cand" in got:
            root = np.sqrt(np.diag(t["H"]))
            n6 = 6 * len(it)
            dev["step_shared"] = float(np.max(np.abs(self.shared_minus(got["shared_cand"], t["shared_cand"]))[f] * root[n6:]))
            dev["step_pose"] = max(float(np.max(np.abs(pose_minus(got["pose_cand"][i], t["pose_cand"][i])) * root[6 * j:6 * j + 6]))
                                   for j, i in enumerate(it))
        return dev

    def evaluate(self, O, shared, poses, flags, part, lam=None):
        """Truth, the two references' deviations and the bound per quantity at one state.  lam: one trial from that state
        (the quantities are the two steps); None: what the covariance stage reports there."""
        ev = Evaluation(self)
        ev.truth = self.truth(shared, poses, flags, part, lam)
        for name, ref in ((REFS[0], self.reference_a(O, shared, poses, flags, part, lam)),
                          (REFS[1], self.reference_b(shared, poses, flags, part, lam))):
            assert ref["free"].tolist() == ev.truth["free"].tolist(), "%s and the truth disagree on the active unknowns" % name
            ev.refs[name] = self.deviation(self.only(ref, lam), ev.truth)
        ev.bound = {q: MARGIN * max(d[q] for d in ev.refs.values()) for q in ev.refs[REFS[0]]}
        return ev

    @staticmethod
    def only(result, lam):
        """The quantities of a result that are compared: the candidates of a trial, or everything else."""
        trial = ("shared_cand", "pose_cand")
        return {k: v for k, v in result.items() if (k in trial) == (lam is not None)}


class Evaluation:
    def __init__(self, case):
        self.case, self.truth, self.refs, self.bound = case, None, {}, {}

    def larger_reference(self, q):
        return max(d[q] for d in self.refs.values())

    def conditions(self, label):
        """The conditions every evaluation must meet, on the CPU and at the device's state: both references below
        cov_cases.REFERENCE_CAP, the truth's last Newton correction at most 1 / 64 of the larger of them.  Returns failures."""
        bad = ["%s: %s deviates by %.3e in %s, above the cap of the references" % (label, ref, v, q)
               for ref, d in self.refs.items() for q, v in d.items() if not v < cc.REFERENCE_CAP]
        if "shared_cov" in self.bound:
            larger = max(self.larger_reference("shared_cov"), self.larger_reference("item_cov"))
            if not self.truth["correction"] <= cc.REFINEMENT_SHARE * larger:
                bad.append("%s: the truth's last Newton correction %.3e is more than 1 / 64 of the larger reference's %.3e"
                           % (label, self.truth["correction"], larger))
        return bad

    def check(self, got, label):
        """A result against the bound: (failures, {quantity: deviation})."""
        dev = self.case.deviation(got, self.truth)
        return (["%s %s: deviation %.3e above the bound %.3e (%.2f x)" % (label, q, v, self.bound[q], v / self.bound[q])
                 for q, v in dev.items() if not v <= self.bound[q]], dev)


# ---- vmm_ba_calibrate ----------------------------------------------------------------------------------------------------

class CalibCase(ArrowCase):
    entry, P = "calibrate", 9

    def shared_truth(self):
        return np.concatenate([self.scene.intr, self.scene.dist])

    def shared_start(self):
        return self.shared_truth() + START * ys.PERTURB

    def held(self):
        return np.array([not (self.mask >> j) & 1 for j in range(9)])

    def at(self, shared):
        """finished_map_cases' localisation case of the same scene under the camera model `shared`."""
        return fm.LocalizeCase(ec.Scene(**dict(self.scene.__dict__, intr=np.array(shared[:4], np.float64),
                                               dist=np.array(shared[4:], np.float64))), self.loss)

    def columns(self, i, shared, pose, dtype):
        """r (m, 4, 2), the pose columns (m, 4, 2, 6) and the nine model columns (m, 4, 2, 9) of image i."""
        s, (b, e) = self.scene, self.span(i)
        t = s.obs_tag[b:e]
        cam = np.tile(np.asarray(pose, np.float64), (e - b, 1))
        k = np.asarray(shared, np.float64)
        r, _, Jc, _ = ec.corner_chain(k[:4], k[4:], cam, s.tag_gt[t], s.tag_wh[t], s.obs_px[b:e], dtype)
        return r, Jc, cc.model_columns(k[:4], k[4:], cam, s.tag_gt[t], s.tag_wh[t], dtype)

    def shared_plus(self, shared, d, dtype):
        return np.asarray(shared, dtype) + np.asarray(d, dtype)

    def shared_minus(self, a, b):
        return np.asarray(a, LD) - np.asarray(b, LD)

    def system_a(self, O, shared, poses, keep):
        s, o = self.scene, np.flatnonzero(keep)
        return ys.calib_system(O, np.asarray(shared, np.float64), np.asarray(poses, np.float64), s.tag_gt, s.tag_wh, s.obs_item[o],
                               s.obs_tag[o], s.obs_px[o], self.robust, self.a, self.mask)

    def host_optimum(self, O, part=None):
        """(k, poses, cost) of yardstick.host_calibration over the clean observations from the truth."""
        s = self.scene
        o = np.flatnonzero(s.label)
        k, cams, cost, _ = ys.host_calibration(O, self.shared_truth(), s.cam_gt, s.tag_gt, s.tag_wh, s.obs_item[o], s.obs_tag[o],
                                               s.obs_px[o], self.robust, self.a, self.mask)
        return k, cams, cost


def observation_edges(model, outliers, loss, mask=0x1FF):
    s = fm.localize_scene(model, outliers)
    return CalibCase(s, loss, mask, dict(observations_per_image=list(s.counts), images=len(s.counts),
                                         note="image_normal_sums' 256 stride: 255, 256, 257, 511, 512, 513; outliers at list "
                                              "positions 0, 63, 64, 255, 256, m - 1"))


def item_edges(n, loss="plain", model="distorted"):
    s = fm.localize_scene(model, False, counts=(TAGS_PER_IMAGE,) * n, seed=20261210 + n)
    return CalibCase(s, loss, 0x1FF, dict(images=n, observations_per_image=TAGS_PER_IMAGE,
                                          note="k_calib_solve's four chains, the 64-thread kernels, arrow_control's 256 stride"))


# ---- vmm_ba_rig_calibrate --------------------------------------------------------------------------------------------------

class RigCalCase(ArrowCase):
    entry = "rig_calibrate"

    def __init__(self, scene, loss, mask, exercises):
        super().__init__(scene, loss, mask, exercises)
        self.K = scene.n_rig_cams
        self.P = 6 * self.K

    def shared_truth(self):
        return np.array(self.scene.ext_qt, np.float64)

    def shared_start(self):
        """Every extrinsic the mask frees moved by START x EXT_PERTURB, the sign alternating with the camera."""
        ext = self.shared_truth()
        for c in range(self.K):
            if (self.mask >> c) & 1:
                ext[c] = pose_plus(ext[c], START * EXT_PERTURB * (-1.0) ** c, np.float64)
        return ext

    def held(self):
        return np.repeat([not (self.mask >> c) & 1 for c in range(self.K)], 6)

    def active_probe(self, Cd):
        return np.repeat(Cd[0::6], 6)       # k_rigcal_solve: the extrinsic's first diagonal entry of sum C

    def at(self, shared):
        return fm.RigCase(ec.Scene(**dict(self.scene.__dict__, ext_qt=np.array(shared, np.float64))), self.loss)

    def columns(self, i, shared, pose, dtype):
        """r (m, 4, 2), the rig columns (m, 4, 2, 6) and the extrinsic columns (m, 4, 2, 6 K: six per observation that are
        not zero, its camera's) of frame i; the module's docstring derives them."""
        s, (b, e) = self.scene, self.span(i)
        r, Jr, Je = np.zeros((e - b, 4, 2), dtype), np.zeros((e - b, 4, 2, 6), dtype), np.zeros((e - b, 4, 2, self.P), dtype)
        for c in np.unique(s.obs_cam[b:e]):
            of = np.flatnonzero(s.obs_cam[b:e] == c)
            cam, Rc, v = rg.compose_rig(shared[c], pose, dtype)
            t = s.obs_tag[b:e][of]
            rr, _, Jc, _ = ec.corner_chain(s.intr[c], s.dist[c], np.tile(cam, (len(of), 1)), s.tag_gt[t], s.tag_wh[t],
                                           s.obs_px[b:e][of], dtype)
            r[of] = rr
            Jr[of] = rg.turn_to_rig(Jc, Rc)
            Je[of, :, :, 6 * c:6 * c + 6] = rg.extrinsic_columns(Jc, v, dtype)
        return r, Jr, Je

    def shared_plus(self, shared, d, dtype):
        return np.array([pose_plus(shared[c], np.asarray(d, dtype)[6 * c:6 * c + 6], dtype) for c in range(self.K)])

    def shared_minus(self, a, b):
        return np.concatenate([pose_minus(a[c], b[c]) for c in range(self.K)])

    def system_a(self, O, shared, poses, keep):
        cost, r, J = rc.rig_system(O, self.scene, np.asarray(poses, np.float64), np.asarray(shared, np.float64), keep, self.robust,
                                   self.a)
        J[:, 6 * self.n_items:][:, self.held()] = 0.0
        return cost, r, J

    def host_optimum(self, O):
        s = self.scene
        rig, ext, cost, _ = rc.host_rig_calibration(O, s, s.rig_gt, s.ext_qt, s.label, self.robust, self.mask, self.a)
        return ext, rig, cost


def default_rig_mask(K):
    return (1 << K) - 2            # every camera but camera 0 (vmm_ba.h)


def rig_edges(K, outliers, loss, mask=None):
    """finished_map_cases.rig_scene(K) and one frame more: two observations in every camera but the last, SECOND_TRIP in
    the last (the one before the frame's last is an inlier on the second trip of camera_normal_sums)."""
    s = fm.rig_scene(K, outliers, extra=[[2] * (K - 1) + [SECOND_TRIP]])
    P = 6 * K
    return RigCalCase(s, loss, default_rig_mask(K) if mask is None else mask,
                      dict(frames=s.n_frames, per_frame=s.per_frame.tolist(), n_rec=P * (P + 1) // 2 + 2 * P + 5, n_el=27 + 6 * P,
                           note="k_rigcal_frame's record and elimination loops, k_rigcal_cov_pose's 64 stride (6 P = %d), "
                                "camera_normal_sums' second trip in the last frame" % (6 * P)))


INACTIVE_CAMERA = 1


def frame_edges(n, loss="plain", inactive=False):
    """n small frames at K = 3 (three observations per camera).  inactive: camera INACTIVE_CAMERA sees nothing in any
    frame and the mask frees it and the last camera."""
    s = fm.rig_scene(3, False, seed=20261220 + n + (1000 if inactive else 0), frames=[[3, 0 if inactive else 3, 3]] * n)
    return RigCalCase(s, loss, 0b110, dict(frames=n, per_frame=[3, 0 if inactive else 3, 3],
                                           note="k_rigcal_solve's four chains, the 64-thread begin kernel"
                                                + (", an extrinsic that is freed and inactive (s_act)" if inactive else "")))


# ---- the lists of the CPU and the GPU tests ---------------------------------------------------------------------------------

# (a) the covariance stage and (b) the result on the observation edges: both models x three losses with the placed outliers,
# and the two other masks
CALIB_EDGE_CASES = [(m, True, l, 0x1FF) for m in fm.MODELS for l in fm.LOSSES] + [("distorted", True, "huber0.5", 0x1EF),
                                                                               ("pinhole", True, "plain", 0x00F)]
RIG_EDGE_CASES = [(K, True, l, None) for K in RIG_CAMS for l in fm.LOSSES] + [(3, True, "huber0.5", 0b100), (8, True, "plain", 0x80)]
# (c) one trial
CALIB_TRIAL_CASES = [(m, True, l, k) for m in fm.MODELS for k in (0x1FF, 0x00F) for l in ("plain", "huber0.5")]
RIG_TRIAL_CASES = [(K, True, l, None) for K in (2, 4, 8) for l in ("plain", "huber0.5")]


def case_id(args):
    """K2-outliers-plain-default for an edge case (mask: default or hexadecimal), n5-huber0.5-inactive for a batch of n."""
    if len(args) == 4:
        return fm.case_id(args[:3]) + ("-default" if args[3] is None else "-mask%x" % args[3])
    return "-".join(("inactive" if a else "active") if isinstance(a, bool) else "n%d" % a if isinstance(a, int) else str(a) for a in args)
