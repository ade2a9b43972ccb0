"""Scenes, longdouble truth and float64 references for the accuracy tests of the stateless calls against a finished map
(test_finished_map_cases_cpu.py, test_finished_map_accuracy.py, tools/finished_map_accuracy.py): vmm_ba_localize,
vmm_ba_rig_localize, vmm_ba_locate_tags, vmm_ba_triangulate and vmm_ba_predict_localization.  numpy only: nothing here
calls the engine, and there are no tests in here.

Input.  Everything these kernels report behind the last LM trial is a function of the returned state (pose or point), the
returned flags and the inputs.  A case therefore takes a STATE and a FLAG SET per item -- on the GPU the device's own,
read bit for bit, on the CPU the host yardstick's optimum over the clean observations -- and forms at that state

    cost = 1/2 sum rho(|r|^2)                         over the flagged observations' corners
    rms  = sqrt(sum |r|^2 / (4 n_inlier))             k_localize, k_rig_localize, k_locate_tags (as each kernel computes it)
           sqrt(sum |r|^2 / n_inlier)                 k_triangulate (one corner per view, kernels_triangulate.hip)
    H    = sum rho' J^T J, H^-1                       cam_cov, tag_cov, xyz_cov; sigma_px^2 H^-1 = cov_px (no loss)
    H^-1 (sum_i G_i C_i G_i^T) H^-1                   tag_cov_cams (G_i = sum over the four corners of rho' Jt^T Jc),
                                                      xyz_cov_cams (G_i = rho'_i Jp_i^T Jc_i), cov_map (G_t = sum Jc^T Jt)
    the largest corner distance of every observation  the classification (triangulate: and Z > 0)

Truth.  np.longdouble throughout (geometry and conventions: ref_geometry.py): eval_cases.corner_chain for residuals and Jacobians (a free point is a tag of zero
size at the point: its tag-translation columns are Jp), eval_cases.huber, cov_cases.refined_inverse (power-of-two Jacobi
scaling, Newton refinement of the float64 inverse).

References.  A: the oracle's functor (yardstick.image_rows / point_rows, tag_cases.tag_rows, predict_cases.host_pose's
sums) through yardstick.block_normal, inverted with np.linalg.inv.  B: a float64 restatement of the device's scheme from
small_solve.hpp's and pose_lm.hpp's words: corner_chain in float64, rows scaled by sqrt(rho'), sums in list order
(ref_algebra.ordered_sum), ref_algebra.spd_inverse (cholesky -> lower_inverse -> lower_gram), the symmetrised C S C
of ref_algebra.sandwich for the propagated parts.  Neither calls the library.

Metric.  Covariances entry by entry, |got - truth| / sqrt(truth_ii truth_jj) (cov_cases.entry_deviation); cost, rms and
the sigmas relative.  The bound of a case and quantity is MARGIN (8) x the larger deviation of A and B over ALL items of
the case -- never a figure that the kernels produced.
"""
import numpy as np

import cov_cases as cc
import eval_cases as ec
import predict_cases as pc
import ref_algebra as ra
import ref_geometry as rg
import rig_cases as rc
import tag_cases as tc
import yardstick as ys

LD = cc.LD
MARGIN = ec.MARGIN
U64 = cc.U64
INLIER_PX = 8.0           # the default of every options struct of the family
NOISE_PX = 0.3
THRESHOLD_GAP = 1e-9      # px: no largest corner distance may lie this close to inlier_px where flags are compared
COST_GAP = 1e-9           # the project's figure for a cost between two optima (test_gpu_rig.py, test_gpu_triangulate.py)
LOSSES = {"plain": (False, 1.0), "huber0.5": (True, 0.5), "huber2.5": (True, 2.5)}
MODELS = ("pinhole", "distorted")
EDGE_POSITIONS = (0, 63, 64, 255, 256)    # and m - 1: stride and wave edges of the 256-thread and the 64-lane lists
MIN_FOR_OUTLIERS = 8                      # shorter lists keep all their observations
LOCALIZE_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)
LOCATE_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
TRACK_COUNTS = (2, 3, 63, 64, 65, 127, 128, 129, 130)
QUANTITIES = ("cost", "rms", "cov", "prop")


def camera_model(name):
    """(intr, dist): synthetic.make_scene(5)'s camera, with its distortion or without any."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = ec.cached(("finished map model",), lambda: make_scene(5))
    assert name in MODELS
    return np.array(s.intr, np.float64), (np.array(s.dist, np.float64) if name == "distorted" else np.zeros(5))


# ---- geometry ---------------------------------------------------------------------------------------------------------

def _tags(rng, n):
    """n small tags in a slab 0.8 m deep (not a plane), tilted by some tens of degrees, facing +z."""
    qt = np.array([np.r_[rg.small_quat(rng, 0.12), rng.uniform(-1.2, 1.2), rng.uniform(-0.8, 0.8), rng.uniform(-0.4, 0.4)]
                   for _ in range(n)])
    wh = np.where(rng.random(n)[:, None] < 0.5, [[0.1285, 0.1285]], [[0.1165, 0.0923]])
    return qt, wh


def _cameras(rng, n, spread=(0.4, 0.3)):
    """n world->camera poses 3.2 .. 4.5 m in front of the slab, looking at it (eval_cases._wall's layout)."""
    return np.array([np.r_[rg.qmul(rg.small_quat(rng, 0.04), [0.0, 1.0, 0.0, 0.0]), rng.uniform(-spread[0], spread[0]),
                           rng.uniform(-spread[1], spread[1]), rng.uniform(3.2, 4.5)] for _ in range(n)])


def radial_slope(dist, p_cam):
    """1 + 3 k1 r2 + 5 k2 r2^2 + 7 k3 r2^3 at every corner: positive where the radial map rises
    (vmm_ba_predict_localization's visibility rule)."""
    x, y = p_cam[..., 0] / p_cam[..., 2], p_cam[..., 1] / p_cam[..., 2]
    r2 = x * x + y * y
    return 1 + r2 * (3 * LD(dist[0]) + r2 * (5 * LD(dist[1]) + r2 * 7 * LD(dist[4])))


NEAR_DEPTH = 1.2   # m: how far the only camera of a one-observation item stands from its tag


def _in_front(cam_qt, at):
    """The world point at camera coordinates `at` of the world->camera pose cam_qt."""
    return ys.rotation(cam_qt).T @ (np.asarray(at, np.float64) - cam_qt[4:])


def outlier_positions(m):
    """The list positions of an m-long list that get an outlier: 0, 63, 64, 255, 256 and m - 1 where they exist."""
    if m < MIN_FOR_OUTLIERS:
        return []
    return sorted({p for p in EDGE_POSITIONS + (m - 1,) if p < m})


def _place_outliers(rng, px, start, width):
    """Moves the observations at outlier_positions of every list by 10 .. 40 x inlier_px (all its corners alike, as
    test_outliers_are_found_and_do_not_move_the_pose does).  Returns the labels (True: clean)."""
    label = np.ones(len(px), bool)
    for i in range(len(start) - 1):
        b, e = int(start[i]), int(start[i + 1])
        for p in outlier_positions(e - b):
            ang, amp = rng.uniform(0, 2 * np.pi), rng.uniform(10.0, 40.0) * INLIER_PX
            px[b + p] += np.tile([amp * np.cos(ang), amp * np.sin(ang)], width // 2)
            label[b + p] = False
    return label


def _assert_conditions(s, p_cam):
    """The builder's conditions (test_finished_map_cases_cpu.py asserts them again from the scene)."""
    assert (p_cam[..., 2] > 0).all(), "a corner behind its camera"
    assert (radial_slope(s.dist, p_cam) > 0).all(), "the radial map is not rising at a corner"
    d = np.linalg.norm((s.obs_px[s.label] - s.clean_px[s.label]).reshape(len(s.clean_px[s.label]), -1, 2), axis=2)
    assert (d <= INLIER_PX / 4).all(), "a clean corner further than inlier_px / 4 from its pixel"


def localize_scene(model, outliers, counts=LOCALIZE_COUNTS, seed=20261201):
    """A map of max(counts) tags and one image per count, in a shuffled order: image i sees exactly counts[i] tags."""
    def make():
        rng = np.random.default_rng(seed)
        intr, dist = camera_model(model)
        cnt = [int(counts[k]) for k in rng.permutation(len(counts))]
        tag_qt, wh = _tags(rng, max(cnt))
        cam = _cameras(rng, len(cnt))
        obs_tag = np.concatenate([rng.permutation(len(tag_qt))[:c] for c in cnt]).astype(np.int32)
        obs_img = np.repeat(np.arange(len(cnt)), cnt)
        clean, px = rg.pixels(rng, intr, dist, cam[obs_img], tag_qt[obs_tag], wh[obs_tag], NOISE_PX)
        start = rg.start(cnt)
        label = _place_outliers(rng, px, start, 8) if outliers else np.ones(len(px), bool)
        s = ec.Scene(kind="localize", model=model, intr=intr, dist=dist, tag_gt=tag_qt, tag_wh=wh, cam_gt=cam, counts=cnt,
                     start=start, obs_tag=obs_tag, obs_item=obs_img, obs_px=px, clean_px=clean, label=label)
        _assert_conditions(s, rg.camera_points(cam[obs_img], tag_qt[obs_tag], wh[obs_tag]))
        return s
    return ec.cached(("finished map localize", model, bool(outliers), tuple(counts), seed), make)


def locate_scene(model, outliers, counts=LOCATE_COUNTS, seed=20261202):
    """The dual: max(counts) known cameras, one tag per count in a shuffled order; tag t is seen by exactly counts[t]
    cameras, obs_cam strictly increasing within a tag.  cam_cov: seeded SPD blocks (millimetres, milliradians)."""
    def make():
        rng = np.random.default_rng(seed)
        intr, dist = camera_model(model)
        cnt = [int(counts[k]) for k in rng.permutation(len(counts))]
        tag_qt, wh = _tags(rng, len(cnt))
        cam = _cameras(rng, max(cnt))
        obs_cam = np.concatenate([np.sort(rng.permutation(len(cam))[:c]) for c in cnt]).astype(np.int32)
        obs_tag = np.repeat(np.arange(len(cnt)), cnt)
        # the tag with one observation stands NEAR_DEPTH in front of its only camera: 4 m away its propagated part came
        # out of the two references a factor 15 apart (condition 7e2), here they agree (condition 45)
        t1 = cnt.index(1)
        tag_qt[t1, 4:] = _in_front(cam[obs_cam[rg.start(cnt)[t1]]], [0.05, -0.04, NEAR_DEPTH])
        clean, px = rg.pixels(rng, intr, dist, cam[obs_cam], tag_qt[obs_tag], wh[obs_tag], NOISE_PX)
        start = rg.start(cnt)
        label = _place_outliers(rng, px, start, 8) if outliers else np.ones(len(px), bool)
        s = ec.Scene(kind="locate", model=model, intr=intr, dist=dist, tag_gt=tag_qt, tag_wh=wh, cam_gt=cam, counts=cnt,
                     start=start, obs_cam=obs_cam, obs_item=obs_tag, obs_px=px, clean_px=clean, label=label,
                     cam_cov=pc.random_tag_cov(len(cam), fixed=[], seed=seed))
        for t in range(len(cnt)):
            assert (np.diff(obs_cam[start[t]:start[t + 1]]) > 0).all()
        _assert_conditions(s, rg.camera_points(cam[obs_cam], tag_qt[obs_tag], wh[obs_tag]))
        return s
    return ec.cached(("finished map locate", model, bool(outliers), tuple(counts), seed), make)


def triangulate_scene(model, outliers, counts=TRACK_COUNTS, seed=20261203):
    """max(counts) known cameras spread over 3 m x 2 m, sorted from left to right; one free point per count in a shuffled
    order, seen by exactly counts[p] cameras (strictly increasing); the two-view track takes the outermost cameras.  One
    more point, the last, is the ill-conditioned kind: two views from the two cameras that stand closest together."""
    def make():
        rng = np.random.default_rng(seed)
        intr, dist = camera_model(model)
        cnt = [int(counts[k]) for k in rng.permutation(len(counts))] + [2]
        cam = _cameras(rng, max(cnt), spread=(1.5, 1.0))
        cam = cam[np.argsort(cam[:, 4])]
        pts = np.stack([rng.uniform(-0.5, 0.5, len(cnt)), rng.uniform(-0.4, 0.4, len(cnt)), rng.uniform(-0.4, 0.4, len(cnt))],
                       axis=1)
        views = [np.sort(rng.permutation(len(cam))[:c]) if c > 2 else np.array([0, len(cam) - 1]) for c in cnt]
        centre = np.array([pc.camera_centre(c) for c in cam])
        gap = np.linalg.norm(centre[:, None] - centre[None], axis=2) + 1e9 * np.eye(len(cam))
        views[-1] = np.sort(np.unravel_index(np.argmin(gap), gap.shape))
        obs_cam = np.concatenate(views).astype(np.int32)
        obs_pt = np.repeat(np.arange(len(cnt)), cnt)
        tag = point_as_tag(pts)
        clean, px = rg.pixels(rng, intr, dist, cam[obs_cam], tag[obs_pt], np.zeros((len(obs_pt), 2)), NOISE_PX)
        clean, px = clean[:, :2].copy(), px[:, :2].copy()
        start = rg.start(cnt)
        label = _place_outliers(rng, px, start, 2) if outliers else np.ones(len(px), bool)
        s = ec.Scene(kind="triangulate", model=model, intr=intr, dist=dist, pts_gt=pts, cam_gt=cam, counts=cnt, start=start,
                     obs_cam=obs_cam, obs_item=obs_pt, obs_px=px, clean_px=clean, label=label,
                     cam_cov=pc.random_tag_cov(len(cam), fixed=[], seed=seed))
        _assert_conditions(s, rg.camera_points(cam[obs_cam], tag[obs_pt], np.zeros((len(obs_pt), 2))))
        return s
    return ec.cached(("finished map triangulate", model, bool(outliers), tuple(counts), seed), make)


def point_as_tag(X):
    """A free point as a tag of zero size at X with the identity rotation: all four corners are the point, and the
    translation columns of the tag Jacobian are Jp."""
    X = np.asarray(X).reshape(-1, 3)
    out = np.zeros((len(X), 7), X.dtype)
    out[:, 0] = 1
    out[:, 4:] = X
    return out


# ---- one entry point on one scene under one loss ------------------------------------------------------------------------

class Case:
    """A scene of one entry point under one loss.  evaluate(O, states, flags) forms the truth and both references at the
    given states over the given flags; the subclasses say what an item's rows are."""
    n = 6            # unknowns of an item
    corners = 4      # corners per observation
    front_rule = False

    def __init__(self, scene, loss):
        self.scene, self.loss = scene, loss
        self.robust, self.a = LOSSES[loss]
        self.n_items = len(scene.start) - 1

    def span(self, i):
        return int(self.scene.start[i]), int(self.scene.start[i + 1])

    # -- supplied by the entry point --
    def chain(self, i, state, dtype):
        """r (m, corners, 2), J (m, corners, 2, n), the other side's Jc (m, corners, 2, 6), depth (m, corners)."""
        raise NotImplementedError

    def oracle_rows(self, O, i, state, keep):
        """[(r (2,), J (2, n), Jc (2, 6) of the other side, local observation)] per corner of the kept observations."""
        raise NotImplementedError

    def other_cov(self, i):
        """(m, 6, 6): the covariance behind every observation's other side, or None."""
        return None

    def optimum(self, O, i, keep):
        """(state, float64 cost) of the host yardstick's optimiser over the kept observations, started at the truth."""
        raise NotImplementedError

    def pixels(self, i):
        b, e = self.span(i)
        return self.scene.obs_px[b:e].reshape(e - b, self.corners, 2)

    def rounding_floor(self, i, state, flags):
        """What one rounding of every projected pixel does to the cost and to rms, relative: a residual is the difference
        of two pixel coordinates and carries about 2^-53 (|proj| + |obs|) of absolute error whatever its own size, so
        d cost = sum rho' |r| 2^-53 (|proj| + |obs|) and d sum |r|^2 twice that without the loss.  An item with one
        observation has a cost of a few hundredths from coordinates of a few thousand; a reference that comes out below
        this by luck is counted at it when the two references are compared (test_finished_map_cases_cpu.py)."""
        on = np.asarray(flags, bool)
        r = self.chain(i, state, LD)[0][on]
        px = self.pixels(i)[on].astype(LD)
        sq, rho0, rho1 = self.loss_terms(r, LD)
        moved = LD(U64) * np.abs(r) * (np.abs(r + px) + np.abs(px))
        return dict(cost=float((rho1[..., None] * moved).sum() / (rho0.sum() / LD(2))), rms=float(moved.sum() / sq.sum()))

    # -- the truth --
    def loss_terms(self, r, dtype):
        """(|r|^2, rho, rho') per corner of r (..., 2) under the case's loss."""
        sq = (r * r).sum(axis=-1)
        if not self.robust:
            return sq, sq, np.ones_like(sq)
        rho = ec.huber(self.a, sq, dtype)
        return sq, rho[..., 0], rho[..., 1]

    def classify(self, i, state):
        """(flags, distance of the nearest largest corner distance from inlier_px) in longdouble."""
        r, _, _, depth = self.chain(i, state, LD)
        dmax = np.sqrt((r * r).sum(axis=-1).max(axis=-1))
        flags = dmax <= LD(INLIER_PX)
        if self.front_rule:
            flags &= (depth > 0).all(axis=-1)
        return flags, float(np.abs(dmax - LD(INLIER_PX)).min())

    def ld_cost(self, i, state, flags):
        r, _, _, _ = self.chain(i, state, LD)
        _, rho0, _ = self.loss_terms(r[flags], LD)
        return rho0.sum(dtype=LD) / LD(2)

    def truth(self, i, state, flags):
        r, J, Jo, _ = self.chain(i, state, LD)
        on = np.asarray(flags, bool)
        sq, rho0, rho1 = self.loss_terms(r[on], LD)
        n_in = int(on.sum())
        H = np.einsum("mk,mkrp,mkrq->pq", rho1, J[on], J[on])
        cov, corr = cc.refined_inverse(H)
        out = dict(cost=rho0.sum(dtype=LD) / LD(2), rms=np.sqrt(sq.sum(dtype=LD) / LD(self.corners * n_in)), cov=cov, prop=None,
                   H=H, correction=cc.entry_deviation(cov + corr, cov))
        C = self.other_cov(i)
        if C is not None:
            G = np.einsum("mk,mkrp,mkrq->mpq", rho1, J[on], Jo[on])
            S = np.einsum("mpa,mab,mqb->pq", G, C[on].astype(LD), G)
            out["prop"] = cov @ (0.5 * (S + S.T)) @ cov
        return out

    # -- the references --
    def reference_a(self, O, i, state, flags):
        on = np.asarray(flags, bool)
        rows = self.oracle_rows(O, i, state, on)
        cost, A, _ = ys.block_normal(O, [(r, J) for r, J, _, _ in rows], self.robust, self.a)
        raw2 = sum(float(r @ r) for r, _, _, _ in rows)
        cov = np.linalg.inv(A)
        out = dict(cost=cost, rms=np.sqrt(raw2 / (self.corners * int(on.sum()))), cov=cov, prop=None)
        C = self.other_cov(i)
        if C is not None:
            G = np.zeros((len(on), self.n, 6))
            for r, J, Jc, d in rows:
                (_, w), = ys.corner_loss(O, r, self.robust, self.a)
                G[d] += w * (J.T @ Jc)
            S = sum(G[d] @ C[d] @ G[d].T for d in np.flatnonzero(on))
            out["prop"] = cov @ S @ cov
        return out

    def reference_b(self, i, state, flags):
        r, J, Jo, _ = self.chain(i, state, np.float64)
        on = np.asarray(flags, bool)
        sq, rho0, rho1 = self.loss_terms(r[on], np.float64)
        wgt = np.sqrt(rho1)
        j = J[on] * wgt[..., None, None]
        P = j[:, :, 0, :, None] * j[:, :, 0, None, :] + j[:, :, 1, :, None] * j[:, :, 1, None, :]
        H = ra.ordered_sum(P.reshape(-1, self.n, self.n))
        cov = ra.spd_inverse(H)
        n_in = int(on.sum())
        out = dict(cost=0.5 * ra.ordered_sum(rho0.reshape(-1)), rms=np.sqrt(ra.ordered_sum(sq.reshape(-1)) / (float(self.corners) * n_in)),
                   cov=cov, prop=None)
        C = self.other_cov(i)
        if C is not None:
            w2 = wgt * wgt
            jo = Jo[on]
            G = np.zeros((n_in, self.n, 6))
            for k in range(self.corners):
                G += w2[:, k, None, None] * (J[on][:, k, 0, :, None] * jo[:, k, 0, None, :] + J[on][:, k, 1, :, None] * jo[:, k, 1, None, :])
            S = ra.ordered_sum((G @ C[on]) @ np.swapaxes(G, 1, 2))
            out["prop"] = ra.sandwich(cov, S)
        return out

    @staticmethod
    def deviation(got, truth):
        """{quantity: deviation of `got` from the truth in the metric}; prop only where the truth has it."""
        dev = dict(cost=float(abs(LD(got["cost"]) - truth["cost"]) / truth["cost"]),
                   rms=float(abs(LD(got["rms"]) - truth["rms"]) / truth["rms"]),
                   cov=cc.entry_deviation(got["cov"], truth["cov"]))
        if truth["prop"] is not None:
            dev["prop"] = cc.entry_deviation(got["prop"], truth["prop"])
        return dev

    def evaluate(self, O, states, flags, items=None):
        """The truth and the references of the items at `states` over `flags` (lists indexed by item).  Returns
        Evaluation: per item the truth and the deviations of A and B, per quantity the bound."""
        items = list(range(self.n_items)) if items is None else list(items)
        ev = Evaluation(self, items)
        for i in items:
            t = self.truth(i, states[i], flags[i])
            ev.truth[i] = t
            ev.refs[i] = {"A oracle, numpy inverse": self.deviation(self.reference_a(O, i, states[i], flags[i]), t),
                          "B device scheme": self.deviation(self.reference_b(i, states[i], flags[i]), t)}
            for q, v in self.rounding_floor(i, states[i], flags[i]).items():
                ev.floor[q] = max(ev.floor.get(q, 0.0), v)
        ev.finish()
        return ev


class Evaluation:
    def __init__(self, case, items):
        self.case, self.items = case, items
        self.truth, self.refs, self.floor = {}, {}, {}

    def finish(self):
        names = sorted({q for i in self.items for d in self.refs[i].values() for q in d}, key=QUANTITIES.index)
        self.reference_deviation = {ref: {q: max(self.refs[i][ref].get(q, 0.0) for i in self.items) for q in names}
                                    for ref in next(iter(self.refs.values()))}
        self.bound = {q: MARGIN * max(d[q] for d in self.reference_deviation.values()) for q in names}

    def check(self, i, got, label):
        """The device's (or anybody's) result of item i against the bound: (failures, {quantity: deviation})."""
        dev = self.case.deviation(got, self.truth[i])
        bad = ["%s item %d %s: deviation %.3e above the bound %.3e" % (label, i, q, v, self.bound[q]) for q, v in dev.items()
               if not v <= self.bound[q]]
        return bad, dev


def symmetric_bits(M):
    M = np.asarray(M)
    return M.tobytes() == np.ascontiguousarray(np.swapaxes(M, -1, -2)).tobytes()


# ---- the entry points -----------------------------------------------------------------------------------------------------

class LocalizeCase(Case):
    """vmm_ba_localize: item = image, state = its world->camera pose, J over the camera's tangent."""

    def chain(self, i, state, dtype):
        s, (b, e) = self.scene, self.span(i)
        t = s.obs_tag[b:e]
        r, _, Jc, _ = ec.corner_chain(s.intr, s.dist, np.tile(np.asarray(state, np.float64), (e - b, 1)), s.tag_gt[t], s.tag_wh[t],
                                      s.obs_px[b:e], dtype)
        return r, Jc, None, None

    def oracle_rows(self, O, i, state, keep):
        s, (b, e) = self.scene, self.span(i)
        d = np.flatnonzero(keep)
        rows = ys.image_rows(O, s.intr, s.dist, np.asarray(state, np.float64), s.tag_gt, s.tag_wh, s.obs_tag[b:e][d], s.obs_px[b:e][d])
        return [(r, J, None, int(d[k // 4])) for k, (r, J) in enumerate(rows)]

    def optimum(self, O, i, keep):
        s, (b, e) = self.scene, self.span(i)
        return ys.image_optimum(O, s, s.cam_gt[i], s.obs_tag[b:e][keep], s.obs_px[b:e][keep], self.robust, self.a)[:2]


class LocateCase(Case):
    """vmm_ba_locate_tags: item = tag, state = its tag->world pose, J over the tag's tangent; with_cams: cam_cov given."""

    def __init__(self, scene, loss, with_cams):
        super().__init__(scene, loss)
        self.with_cams = with_cams

    def chain(self, i, state, dtype):
        s, (b, e) = self.scene, self.span(i)
        r, _, Jc, Jt = ec.corner_chain(s.intr, s.dist, s.cam_gt[s.obs_cam[b:e]], np.tile(np.asarray(state, np.float64), (e - b, 1)),
                                       np.tile(s.tag_wh[i], (e - b, 1)), s.obs_px[b:e], dtype)
        return r, Jt, Jc, None

    def oracle_rows(self, O, i, state, keep):
        s, (b, e) = self.scene, self.span(i)
        out = []
        for d in np.flatnonzero(keep):
            r, Jc, Jt = O.obs_eval(s.intr, s.dist, s.cam_gt[s.obs_cam[b + d]], np.asarray(state, np.float64), s.tag_wh[i], s.obs_px[b + d])
            out += [(r[2 * k:2 * k + 2], Jt[2 * k:2 * k + 2], Jc[2 * k:2 * k + 2], int(d)) for k in range(4)]
        return out

    def other_cov(self, i):
        b, e = self.span(i)
        return self.scene.cam_cov[self.scene.obs_cam[b:e]] if self.with_cams else None

    def optimum(self, O, i, keep):
        s, (b, e) = self.scene, self.span(i)
        return tc.tag_optimum(O, s.intr, s.dist, s.tag_gt[i], s.cam_gt, s.tag_wh[i], s.obs_cam[b:e][keep], s.obs_px[b:e][keep],
                              self.robust, self.a)[:2]


class TriangulateCase(Case):
    """vmm_ba_triangulate: item = point, state = its coordinates, J = Jp; one corner per view, and Z > 0 to be an inlier."""
    n = 3
    corners = 1
    front_rule = True

    def __init__(self, scene, loss, with_cams):
        super().__init__(scene, loss)
        self.with_cams = with_cams

    def chain(self, i, state, dtype):
        s, (b, e) = self.scene, self.span(i)
        tag = np.tile(point_as_tag(np.asarray(state, np.float64)), (e - b, 1))
        cam = s.cam_gt[s.obs_cam[b:e]]
        r, _, Jc, Jt = ec.corner_chain(s.intr, s.dist, cam, tag, np.zeros((e - b, 2)), np.tile(s.obs_px[b:e], (1, 4)), dtype)
        depth = rg.camera_points(cam, tag, np.zeros((e - b, 2)))[:, :1, 2]
        return r[:, :1], Jt[:, :1, :, :3], Jc[:, :1], depth

    def oracle_rows(self, O, i, state, keep):
        s, (b, e) = self.scene, self.span(i)
        out = []
        for d in np.flatnonzero(keep):
            r, Jc, Jp = O.point_eval(s.intr, s.dist, s.cam_gt[s.obs_cam[b + d]], np.asarray(state, np.float64), s.obs_px[b + d])
            out.append((r, Jp, Jc, int(d)))
        return out

    def other_cov(self, i):
        b, e = self.span(i)
        return self.scene.cam_cov[self.scene.obs_cam[b:e]] if self.with_cams else None

    def optimum(self, O, i, keep):
        s, (b, e) = self.scene, self.span(i)
        return ys.point_optimum(O, s, s.pts_gt[i], s.obs_cam[b:e][keep], s.obs_px[b:e][keep], self.robust, self.a)


RIG_TOTALS = (1, 64, 65, 255, 256, 257, 513)
RIG_ALL_IN_LAST, RIG_EMPTY_MIDDLE = 65, 130   # totals of the two special frames (K > 1)
RIG_CAMS = (1, 3, 8)


def _split(rng, total, K):
    """total observations over K cameras, every camera at least one where the total allows it."""
    if total < K:
        out = np.zeros(K, int)
        out[rng.permutation(K)[:total]] = 1
        return out
    return 1 + rng.multinomial(total - K, np.full(K, 1.0 / K))


def rig_scene(K, outliers, seed=20261205, extra=(), frames=None):
    """A rig of K cameras with different models (distorted and not, focal lengths 2 % apart) a few degrees and decimetres
    apart; one frame per total of RIG_TOTALS in a shuffled order, split over the cameras at random, and for K > 1 one frame
    with all its observations in the last camera and one with an empty camera in the middle.  extra: rows of K counts,
    frames appended behind those; frames: rows of K counts that stand in the place of all of them (arrowhead_cases.py)."""
    def make():
        rng = np.random.default_rng(seed + K)
        models = [camera_model(MODELS[(c + 1) % 2]) for c in range(K)]
        intr = np.array([m[0] * (1 + 0.02 * c) for c, m in enumerate(models)])
        dist = np.array([m[1] for m in models])
        ext = np.array([rc.yaw(3.0 * (c - (K - 1) / 2), (0.1 * (c - (K - 1) / 2), 0.02 * (c % 3), 0.0)) for c in range(K)])
        if frames is None:
            per_frame = [_split(rng, int(RIG_TOTALS[k]), K) for k in rng.permutation(len(RIG_TOTALS))]
            if K > 1:
                last = np.zeros(K, int)
                last[-1] = RIG_ALL_IN_LAST
                hole = _split(rng, RIG_EMPTY_MIDDLE, K - 1)
                per_frame += [last, np.insert(hole, K // 2, 0)]
            per_frame += [np.asarray(row, int) for row in extra]
        else:
            per_frame = [np.asarray(row, int) for row in frames]
        per_frame = np.array(per_frame).reshape(-1, K)
        F = len(per_frame)
        tag_qt, wh = _tags(rng, int(per_frame.sum(axis=1).max()))
        rig = _cameras(rng, F)
        slots = per_frame.reshape(-1)
        obs_frame = np.repeat(np.repeat(np.arange(F), K), slots).astype(np.int32)
        obs_cam = np.repeat(np.tile(np.arange(K), F), slots).astype(np.int32)
        obs_tag = np.concatenate([rng.permutation(len(tag_qt))[:n] for n in per_frame.sum(axis=1)]).astype(np.int32)
        cam = np.array([rc.compose(ext[c], rig[f]) for f, c in zip(obs_frame, obs_cam)])
        clean, px = np.zeros((len(obs_tag), 8)), np.zeros((len(obs_tag), 8))
        for c in range(K):
            of = obs_cam == c
            if of.any():
                clean[of], px[of] = rg.pixels(rng, intr[c], dist[c], cam[of], tag_qt[obs_tag[of]], wh[obs_tag[of]], NOISE_PX)
        start = rg.start(per_frame.sum(axis=1))
        label = _place_outliers(rng, px, start, 8) if outliers else np.ones(len(px), bool)
        s = ec.Scene(kind="rig", model="K%d" % K, intr=intr, dist=dist, ext_qt=ext, tag_gt=tag_qt, tag_wh=wh, rig_gt=rig,
                     counts=[int(v) for v in per_frame.sum(axis=1)], per_frame=per_frame, start=start, img_start=rg.start(slots),
                     obs_frame=obs_frame, obs_cam=obs_cam, obs_tag=obs_tag, obs_item=obs_frame, obs_px=px, clean_px=clean,
                     label=label, n_frames=F, n_rig_cams=K)
        p_cam = rg.camera_points(cam, tag_qt[obs_tag], wh[obs_tag])
        assert (p_cam[..., 2] > 0).all()
        for c in range(K):
            assert (radial_slope(dist[c], p_cam[obs_cam == c]) > 0).all()
        d = np.linalg.norm((px[label] - clean[label]).reshape(-1, 4, 2), axis=2)
        assert (d <= INLIER_PX / 4).all()
        return s
    shape = (tuple(map(tuple, extra)), None if frames is None else tuple(map(tuple, frames)))
    return ec.cached(("finished map rig", K, bool(outliers), seed) + (shape if shape != ((), None) else ()), make)


class RigCase(Case):
    """vmm_ba_rig_localize: item = frame, state = its world->rig pose; camera c stands at ext_c o rig, and a rig step
    (dt, dth) moves it by (R_c dt, R_c dth): J = [Jc_t R_c | Jc_r R_c] (rig_cases.rig_rows does it in float64)."""

    def chain(self, i, state, dtype):
        s, (b, e) = self.scene, self.span(i)
        r, J = np.zeros((e - b, 4, 2), dtype), np.zeros((e - b, 4, 2, 6), dtype)
        for c in np.unique(s.obs_cam[b:e]):
            of = np.flatnonzero(s.obs_cam[b:e] == c)
            cam, Rc, _ = rg.compose_rig(s.ext_qt[c], state, dtype)
            t = s.obs_tag[b:e][of]
            rr, _, Jc, _ = ec.corner_chain(s.intr[c], s.dist[c], np.tile(cam, (len(of), 1)), s.tag_gt[t], s.tag_wh[t],
                                           s.obs_px[b:e][of], dtype)
            r[of] = rr
            J[of] = rg.turn_to_rig(Jc, Rc)
        return r, J, None, None

    def oracle_rows(self, O, i, state, keep):
        s, (b, e) = self.scene, self.span(i)
        out = []
        for d in np.flatnonzero(keep):
            c, t = int(s.obs_cam[b + d]), int(s.obs_tag[b + d])
            r, Jr, _ = rc.rig_rows(O, s.intr[c], s.dist[c], s.ext_qt[c], np.asarray(state, np.float64), s.tag_gt[t], s.tag_wh[t],
                                   s.obs_px[b + d])
            out += [(r[2 * k:2 * k + 2], Jr[2 * k:2 * k + 2], None, int(d)) for k in range(4)]
        return out

    def optimum(self, O, i, keep):
        s, (b, e) = self.scene, self.span(i)
        mask = np.zeros(len(s.obs_tag), bool)
        mask[b:e] = keep
        return rc.host_frame_optimum(O, s, i, s.rig_gt[i], s.ext_qt, mask, self.robust, self.a)


def localize_case(model, outliers, loss):
    return LocalizeCase(localize_scene(model, outliers), loss)


def locate_case(model, outliers, loss, with_cams):
    return LocateCase(locate_scene(model, outliers), loss, with_cams)


def triangulate_case(model, outliers, loss, with_cams):
    return TriangulateCase(triangulate_scene(model, outliers), loss, with_cams)


def rig_case(K, outliers, loss):
    return RigCase(rig_scene(K, outliers), loss)


# the cases of the CPU and the GPU tests: every loss, with and without the placed outliers
LOCALIZE_CASES = [(m, o, l) for m in MODELS for o in (False, True) for l in LOSSES]
# with cam_cov / without, the camera model alternating so that each of the two is met with each of the others' values
LOCATE_CASES = [(MODELS[(o + w) % 2], o, l, w) for o in (False, True) for l in LOSSES for w in (True, False)]
TRIANGULATE_CASES = [(MODELS[(o + w + 1) % 2], o, l, w) for o in (False, True) for l in LOSSES for w in (True, False)]
RIG_CASES = [(K, o, l) for K in RIG_CAMS for o in (False, True) for l in LOSSES]
PREDICT_CASES = [(n, w) for n in (1, 63, 64, 65, 129) for w in (True, False)]
BUILDERS = {"localize": (localize_case, LOCALIZE_CASES), "locate_tags": (locate_case, LOCATE_CASES),
            "triangulate": (triangulate_case, TRIANGULATE_CASES), "rig_localize": (rig_case, RIG_CASES)}


def case_id(args):
    return "-".join(("outliers" if a else "clean") if i == 1 else ("cams" if a else "nocams") if isinstance(a, bool) else
                    ("K%d" % a if isinstance(a, int) else str(a)) for i, a in enumerate(args))


def host_states(O, case):
    """(states, flags, float64 costs) of the host optimiser over the clean observations of every item: the state the CPU
    tests evaluate a case at.  Computed once per scene and loss."""
    s = case.scene
    def make():
        out = [case.optimum(O, i, s.label[slice(*case.span(i))]) for i in range(case.n_items)]
        return [q for q, _ in out], [s.label[slice(*case.span(i))] for i in range(case.n_items)], [c for _, c in out]
    return ec.cached(("finished map host states", s.kind, s.model, bool((~s.label).any()), case.loss), make)


def condition_number(H):
    """Of the power-of-two scaled H (units taken out), float64."""
    H = np.asarray(H, np.float64)
    sc = cc.pow2_scale(np.diag(H))
    return float(np.linalg.cond(sc[:, None] * H * sc[None, :]))


# ---- the prediction: no state to find, no loss --------------------------------------------------------------------------

PREDICT_TAGS, PREDICT_POSES = (1, 63, 64, 65, 129), (1, 3, 4, 5)
PREDICT_RELIEF = 0.6      # m: the tags of the lanes stand between 3.4 m and 4.6 m


class PredictCase:
    """vmm_ba_predict_localization on predict_cases.lanes(n_tags, n_poses) with PREDICT_RELIEF of depth (on the plain wall
    the float64 references came out a factor 10 apart on the covariance): item = pose.  truth / references at a given
    visible set: cov_px = sigma_px^2 H^-1, cov_map = H^-1 (sum_t G_t S_t G_t^T) H^-1 with G_t = sum Jc^T Jt, and the two
    sigmas by predict_cases.host_sigmas' formulas."""

    def __init__(self, n_tags, n_poses, with_map):
        self.case = pc.lanes(n_tags, n_poses, relief=PREDICT_RELIEF)
        self.n_tags, self.n_items, self.with_map = n_tags, n_poses, with_map
        self.tag_cov = pc.random_tag_cov(n_tags, fixed=[], seed=20261204) if with_map else None
        self.sigma_px = 0.7

    def _jacobians(self, p, vis, dtype):
        c = self.case
        t = np.flatnonzero(vis)
        _, _, Jc, Jt = ec.corner_chain(c["intr"], c["dist"], np.tile(c["cam_qt"][p], (len(t), 1)), c["tag_qt"][t], c["tag_wh"][t],
                                       np.zeros((len(t), 8)), dtype)
        return t, Jc, Jt

    @staticmethod
    def _sigmas(cam_qt, cov, dtype):
        q = np.asarray(cam_qt, dtype)
        R, t = rg.rotation(q, dtype), q[4:]
        J = -R.T @ np.concatenate([np.eye(3, dtype=dtype), dtype(2) * rg.skew(t)], axis=1)
        return np.sqrt(np.trace(J @ cov @ J.T)), np.sqrt(dtype(pc.RADIANS) ** 2 * np.trace(cov[3:, 3:]))

    def truth(self, p, vis):
        t, Jc, Jt = self._jacobians(p, vis, LD)
        H = np.einsum("mkrp,mkrq->pq", Jc, Jc)
        Hi, corr = cc.refined_inverse(H)
        cov_px = LD(np.float64(self.sigma_px) * np.float64(self.sigma_px)) * Hi
        out = dict(cov=cov_px, prop=None, H=H, correction=cc.entry_deviation(Hi + corr, Hi))
        total = cov_px
        if self.with_map:
            G = np.einsum("mkrp,mkrq->mpq", Jc, Jt)
            S = np.einsum("mpa,mab,mqb->pq", G, self.tag_cov[t].astype(LD), G)
            out["prop"] = Hi @ (0.5 * (S + S.T)) @ Hi
            total = cov_px + out["prop"]
        out["sigma_pos"], out["sigma_rot"] = self._sigmas(self.case["cam_qt"][p], total, LD)
        return out

    def reference_a(self, O, p, vis):
        # predict_cases.host_pose's sums; it inverts them in longdouble, reference A with numpy
        H, M = np.zeros((6, 6)), np.zeros((6, 6))
        c = self.case
        for t in np.flatnonzero(vis):
            _, Jc, Jt = O.obs_eval(c["intr"], c["dist"], c["cam_qt"][p], c["tag_qt"][t], c["tag_wh"][t], np.zeros(8))
            H += Jc.T @ Jc
            if self.with_map:
                G = Jc.T @ Jt
                M += G @ self.tag_cov[t] @ G.T
        Hi = np.linalg.inv(H)
        cov_px = self.sigma_px ** 2 * Hi
        prop = Hi @ M @ Hi if self.with_map else None
        sp, sr = pc.host_sigmas(c["cam_qt"][p], cov_px + (prop if self.with_map else 0.0))
        return dict(cov=cov_px, prop=prop, sigma_pos=sp, sigma_rot=sr)

    def reference_b(self, p, vis):
        t, Jc, Jt = self._jacobians(p, vis, np.float64)
        P = Jc[:, :, 0, :, None] * Jc[:, :, 0, None, :] + Jc[:, :, 1, :, None] * Jc[:, :, 1, None, :]
        Hi = ra.spd_inverse(ra.ordered_sum(P.reshape(-1, 6, 6)))
        cov_px = (self.sigma_px * self.sigma_px) * Hi
        prop, total = None, cov_px
        if self.with_map:
            G = np.zeros((len(t), 6, 6))
            for k in range(4):
                G += Jc[:, k, 0, :, None] * Jt[:, k, 0, None, :] + Jc[:, k, 1, :, None] * Jt[:, k, 1, None, :]
            prop = ra.sandwich(Hi, ra.ordered_sum((G @ self.tag_cov[t]) @ np.swapaxes(G, 1, 2)))
            total = cov_px + prop
        sp, sr = self._sigmas(self.case["cam_qt"][p], total, np.float64)
        return dict(cov=cov_px, prop=prop, sigma_pos=float(sp), sigma_rot=float(sr))

    @staticmethod
    def deviation(got, truth):
        dev = dict(cov=cc.entry_deviation(got["cov"], truth["cov"]),
                   sigma_pos=float(abs(LD(got["sigma_pos"]) - truth["sigma_pos"]) / truth["sigma_pos"]),
                   sigma_rot=float(abs(LD(got["sigma_rot"]) - truth["sigma_rot"]) / truth["sigma_rot"]))
        if truth["prop"] is not None:
            dev["prop"] = cc.entry_deviation(got["prop"], truth["prop"])
        return dev

    def host_visible(self):
        """((n_poses, n_tags) flags by the header's rules, whether any of them rests on rounding)."""
        vis, sl = pc.host_visible(self.case)
        return vis, any(pc.rests_on_rounding(x) for row in sl for x in row)

    def evaluate(self, O, visible):
        """Truth, references and bounds of the poses that have a visible tag, over the given flags."""
        ev = PredictEvaluation(self, [p for p in range(self.n_items) if visible[p].any()])
        for p in ev.items:
            t = self.truth(p, visible[p])
            ev.truth[p] = t
            ev.refs[p] = {"A oracle, numpy inverse": self.deviation(self.reference_a(O, p, visible[p]), t),
                          "B device scheme": self.deviation(self.reference_b(p, visible[p]), t)}
        ev.finish()
        return ev


PREDICT_QUANTITIES = ("cov", "prop", "sigma_pos", "sigma_rot")


class PredictEvaluation(Evaluation):
    def finish(self):
        names = [q for q in PREDICT_QUANTITIES if any(q in d for i in self.items for d in self.refs[i].values())]
        refs = ("A oracle, numpy inverse", "B device scheme")
        self.reference_deviation = {ref: {q: max([self.refs[i][ref].get(q, 0.0) for i in self.items] + [0.0]) for q in names}
                                    for ref in refs}
        self.bound = {q: MARGIN * max(d[q] for d in self.reference_deviation.values()) for q in names}
