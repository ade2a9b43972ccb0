"""The scenes, truth and references of tests/arrowhead_cases.py, checked on the CPU before test_gpu_arrowhead_accuracy.py
relies on them: the builders' counts, the longdouble columns (the extrinsic ones included) against longdouble central
differences and against the oracle's rows, the block-inverse identity of the truth, references A and B under
cov_cases.REFERENCE_CAP with the truth's last Newton correction at most 1 / 64 of the larger of them, exact zeros for the
masked and the inactive unknowns, the decrement at the host optimum, and the conditions of the one-trial cases.

Every case is evaluated at its start: the shared unknowns of shared_start(), the scene's true poses, the placed labels as
flags and the items of at least two inliers taking part (the default min_inlier_tags).
"""
import numpy as np
import pytest

import arrowhead_cases as ah
import cov_cases as cc
import finished_map_cases as fm
import rig_cases as rc

LD = ah.LD
ALL_CASES = ([("calib edges", a) for a in ah.CALIB_EDGE_CASES] + [("rig edges", a) for a in ah.RIG_EDGE_CASES]
             + [("items", (n,)) for n in ah.ITEM_COUNTS] + [("frames", (n,)) for n in ah.FRAME_COUNTS]
             + [("frames", (5, "huber0.5", True))])
TRIAL_CASES = [("calib edges", a) for a in ah.CALIB_TRIAL_CASES] + [("rig edges", a) for a in ah.RIG_TRIAL_CASES]
BUILD = {"calib edges": ah.observation_edges, "rig edges": ah.rig_edges, "items": ah.item_edges, "frames": ah.frame_edges}


def _ids(v):
    return v if isinstance(v, str) else ah.case_id(v)


def _start_state(case, min_inlier_tags=2):
    s = case.scene
    flags = case.flags_list(s.label)
    return case.shared_start(), (s.cam_gt if case.entry == "calibrate" else s.rig_gt), flags, case.participants(flags, min_inlier_tags)


# ---- the builders ---------------------------------------------------------------------------------------------------------

def test_builders_give_the_prescribed_counts_and_labels():
    s = ah.observation_edges("distorted", True, "plain").scene
    assert sorted(s.counts) == sorted(fm.LOCALIZE_COUNTS)
    for i, m in enumerate(s.counts):
        assert np.flatnonzero(~s.label[s.start[i]:s.start[i + 1]]).tolist() == fm.outlier_positions(m)
    for n in ah.ITEM_COUNTS:
        case = ah.item_edges(n)
        assert case.n_items == n and list(case.scene.counts) == [ah.TAGS_PER_IMAGE] * n and case.scene.label.all()
    for K in ah.RIG_CAMS:
        case = ah.rig_edges(K, True, "plain")
        s = case.scene
        assert s.per_frame[-1].tolist() == [2] * (K - 1) + [ah.SECOND_TRIP] and s.n_frames == len(fm.RIG_TOTALS) + 3
        assert sorted(s.counts[:-1]) == sorted(fm.RIG_TOTALS + (fm.RIG_ALL_IN_LAST, fm.RIG_EMPTY_MIDDLE))
        assert case.mask == (1 << K) - 2 and case.P == 6 * K
        assert case.exercises["n_rec"] == {2: 107, 3: 212, 4: 353, 8: 1277}[K] and case.exercises["n_el"] == {2: 99, 3: 135, 4: 171, 8: 315}[K]
        f = s.n_frames - 1
        assert np.flatnonzero(~s.label[s.start[f]:s.start[f + 1]]).tolist() == fm.outlier_positions(int(s.counts[f]))
        second_trip = s.label[s.start[f]:s.start[f + 1]][2 * (K - 1) + 256:]
        assert len(second_trip) == 2 and second_trip[0] and not second_trip[1]     # an inlier on camera_normal_sums' second trip
    for n in ah.FRAME_COUNTS:
        assert ah.frame_edges(n).scene.per_frame.tolist() == [[3, 3, 3]] * n
    s = ah.frame_edges(5, inactive=True).scene
    assert not (s.obs_cam == ah.INACTIVE_CAMERA).any() and s.per_frame.tolist() == [[3, 0, 3]] * 5
    # the scenes the earlier tests use are the ones they had
    assert fm.rig_scene(3, True).n_frames == len(fm.RIG_TOTALS) + 2


# ---- the columns ------------------------------------------------------------------------------------------------------------

def _central(f, x0, plus, n, h):
    """Central differences of f over the n tangent directions of `plus` at x0, longdouble."""
    cols = []
    for j in range(n):
        d = np.zeros(n, LD)
        d[j] = h[j]
        cols.append((f(plus(x0, d)) - f(plus(x0, -d))) / (2 * h[j]))
    return np.stack(cols, axis=-1)


def _block_deviation(got, ref):
    """max over the corners of |got - ref| over the largest entry of the corner's 2 x n block of ref."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    scale = np.abs(ref).max(axis=(-1, -2), keepdims=True)
    return float(np.max(np.abs(got - ref) / scale))


@pytest.mark.parametrize("K", [2, 3])
def test_rig_columns_match_central_differences_and_the_oracle(oracle, K):
    """The rig and the extrinsic columns of every frame against longdouble central differences (step 1e-7: truncation and
    rounding both near 1e-12 of a column), against finished_map_cases.RigCase.chain (the rig columns, to longdouble
    rounding) and against rig_cases.rig_rows: the oracle's float64 rows may deviate MARGIN x as far as this module's own
    float64 chain does."""
    case = ah.rig_edges(K, True, "plain")
    s, ext = case.scene, case.shared_start()
    at = case.at(ext)
    dev_o = dev_b = 0.0
    for i in range(case.n_items):
        b, e = case.span(i)
        pose = s.rig_gt[i]
        r, Jr, Je = case.columns(i, ext, pose, LD)
        assert _block_deviation(at.chain(i, pose, LD)[1], Jr) < 1e-17
        h = np.full(6, LD(1e-7))
        num_r = _central(lambda q: case.columns(i, ext, q.astype(np.float64), LD)[0], np.asarray(pose, LD), ah.pose_plus, 6, h)
        assert _block_deviation(num_r, Jr) < 1e-9
        for c in np.unique(s.obs_cam[b:e]):
            of = s.obs_cam[b:e] == c

            def moved(q, c=c):
                x = ext.copy()
                x[c] = q.astype(np.float64)
                return case.columns(i, x, pose, LD)[0][of]
            num_e = _central(moved, np.asarray(ext[c], LD), ah.pose_plus, 6, h)
            assert _block_deviation(num_e, Je[of][..., 6 * c:6 * c + 6]) < 1e-9
            other = np.ones(case.P, bool)
            other[6 * c:6 * c + 6] = False
            assert not Je[of][..., other].any()
        rb, Jrb, Jeb = case.columns(i, ext, pose, np.float64)
        for d in range(e - b):
            c, t = int(s.obs_cam[b + d]), int(s.obs_tag[b + d])
            _, Jro, Jeo = rc.rig_rows(oracle, s.intr[c], s.dist[c], ext[c], pose, s.tag_gt[t], s.tag_wh[t], s.obs_px[b + d])
            ref = np.concatenate([Jr[d], Je[d][..., 6 * c:6 * c + 6]], axis=-1)
            dev_o = max(dev_o, _block_deviation(np.hstack([Jro, Jeo]).reshape(4, 2, 12), ref))
            dev_b = max(dev_b, _block_deviation(np.concatenate([Jrb[d], Jeb[d][..., 6 * c:6 * c + 6]], axis=-1), ref))
    print("rig K%d: the oracle's rows %.1f, this module's float64 chain %.1f x 2^-53 from the longdouble columns"
          % (K, dev_o * 2.0 ** 53, dev_b * 2.0 ** 53))
    assert dev_o <= ah.MARGIN * dev_b


def test_calibration_columns_match_central_differences_and_the_oracle(oracle):
    import yardstick as ys
    case = ah.observation_edges("distorted", True, "plain")
    s, k = case.scene, case.shared_start()
    dev_o = dev_b = 0.0
    for i in (s.counts.index(1), s.counts.index(65)):
        b, e = case.span(i)
        pose = s.cam_gt[i]
        r, Jp, Jk = case.columns(i, k, pose, LD)
        num_p = _central(lambda q: case.columns(i, k, q.astype(np.float64), LD)[0], np.asarray(pose, LD), ah.pose_plus, 6, np.full(6, LD(1e-7)))
        assert _block_deviation(num_p, Jp) < 1e-9
        h = np.maximum(np.abs(k), 1.0).astype(LD) * LD(2.0) ** -24     # exactly representable steps of k, a float64 input
        num_k = _central(lambda x: case.columns(i, x.astype(np.float64), pose, LD)[0], np.asarray(k, LD), lambda x, d: x + d, 9, h)
        assert _block_deviation(num_k, Jk) < 1e-9
        _, Jpb, Jkb = case.columns(i, k, pose, np.float64)
        for d in range(e - b):
            t = int(s.obs_tag[b + d])
            _, Jco, _ = oracle.obs_eval(k[:4], k[4:], pose, s.tag_gt[t], s.tag_wh[t], s.obs_px[b + d])
            ref = np.concatenate([Jp[d], Jk[d]], axis=-1)
            got = np.hstack([Jco, ys.intrinsic_columns(k, pose, s.tag_gt[t], s.tag_wh[t])]).reshape(4, 2, 15)
            dev_o = max(dev_o, _block_deviation(got, ref))
            dev_b = max(dev_b, _block_deviation(np.concatenate([Jpb[d], Jkb[d]], axis=-1), ref))
    print("calibrate: the oracle's rows %.1f, this module's float64 chain %.1f x 2^-53 from the longdouble columns"
          % (dev_o * 2.0 ** 53, dev_b * 2.0 ** 53))
    assert dev_o <= ah.MARGIN * dev_b


# ---- the truth ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,args", [("calib edges", ("distorted", True, "huber0.5", 0x1EF)), ("rig edges", (3, True, "huber2.5", None)),
                                       ("items", (65,))], ids=_ids)
def test_truth_meets_the_block_inverse_identity(name, args):
    """The lower-right block of H^-1 is S^-1 and the diagonal blocks are A^-1 + A^-1 B S^-1 B' A^-1, formed here in
    longdouble from H's blocks with refined inverses: to the refinement floor (64 x the last Newton correction, at least
    2^-53 -- two longdouble routes of a condition near 1e5)."""
    case = BUILD[name](*args)
    t = case.truth(*_start_state(case))
    n, H = len(t["items"]), t["H"]
    n6 = 6 * n
    A = H[:n6, :n6].reshape(n, 6, n, 6)[np.arange(n), :, np.arange(n), :]
    Ai, _ = cc.refined_inverse(A)
    B = H[:n6, n6:].reshape(n, 6, -1)
    AiB = Ai @ B
    S = H[n6:, n6:] - np.einsum("jap,jaq->pq", B, AiB)
    Si, _ = cc.refined_inverse(0.5 * (S + S.T))
    f = t["free"]
    floor = max(64 * t["correction"], 2.0 ** -53)
    assert cc.entry_deviation(Si, t["shared_cov"][np.ix_(f, f)]) <= floor
    for j, i in enumerate(t["items"]):
        assert cc.entry_deviation(Ai[j] + AiB[j] @ Si @ AiB[j].T, t["item_cov"][i]) <= floor


def test_the_two_routes_of_whole_inverse_agree():
    """cov_cases.refined_inverse and the mixed iteration of the large orders on the same matrix (65 images)."""
    case = ah.item_edges(65)
    t = case.truth(*_start_state(case))
    X, corr = ah.whole_inverse(t["H"], 65, force_mixed=True)
    d = np.diag(t["inverse"])
    assert cc.entry_deviation(X, t["inverse"]) <= max(64 * t["correction"], 2.0 ** -53)
    assert cc.entry_deviation(X + corr, X, d, d) <= 64 * t["correction"] + 2.0 ** -60


RATIOS = {}


@pytest.mark.parametrize("name,args", ALL_CASES, ids=_ids)
def test_references_stay_under_the_cap(oracle, name, args):
    """A and B below cov_cases.REFERENCE_CAP in every quantity, the truth's last Newton correction at most 1 / 64 of the
    larger of the two on the covariances; a masked or inactive unknown has exactly zero rows in the truth and in both."""
    case = BUILD[name](*args)
    state = _start_state(case)
    ev = case.evaluate(oracle, *state)
    for q in ev.bound:
        a, b = (ev.refs[r][q] for r in ah.REFS)
        RATIOS[(name, args, q)] = max(a, b) / max(min(a, b), 1e-300)
        print("%s %s %-10s A %.3e  B %.3e  ratio %.1f" % (name, _ids(args), q, a, b, RATIOS[(name, args, q)]))
    assert not ev.conditions(name), ev.conditions(name)
    dead = np.ones(case.P, bool)
    dead[ev.truth["free"]] = False
    assert dead[case.held()].all()
    for res in (ev.truth, case.reference_a(oracle, *state), case.reference_b(*state)):
        assert not np.asarray(res["shared_cov"])[dead].any() and not np.asarray(res["shared_cov"])[:, dead].any()
    if len(args) > 2 and args[-1] is True and name == "frames":
        assert dead[6 * ah.INACTIVE_CAMERA:6 * ah.INACTIVE_CAMERA + 6].all() and not dead[12:].any()


def test_the_one_tag_item_takes_part_only_when_asked(oracle):
    """min_inlier_tags = 1 lets the image of one tag in; both references stay under the cap with it."""
    case = ah.observation_edges("distorted", True, "huber0.5")
    state = _start_state(case, 1)
    assert all(state[3]) and not all(_start_state(case)[3])
    ev = case.evaluate(oracle, *state)
    assert not ev.conditions("one tag"), ev.conditions("one tag")


# ---- the optimum ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,args", [("items", (5,)), ("frames", (5,)), ("frames", (5, "huber0.5", True))], ids=_ids)
def test_the_decrement_vanishes_at_the_host_optimum(oracle, name, args):
    """1/2 g' H^-1 g at yardstick.host_calibration's / rig_cases.host_rig_calibration's optimum is at most COST_GAP of the
    cost: the assertion the GPU test makes of the device is one the host optimiser meets."""
    case = BUILD[name](*args)
    shared, poses, cost = case.host_optimum(oracle)
    flags = case.flags_list(case.scene.label)
    t = case.truth(shared, poses, flags, case.participants(flags))
    print("%s %s: decrement %.3e of the cost %.6g" % (name, _ids(args), float(t["decrement"] / t["final_cost"]), float(t["final_cost"])))
    assert abs(float(t["final_cost"]) - cost) <= 1e-12 * cost
    assert t["decrement"] <= fm.COST_GAP * t["final_cost"]


# ---- one trial --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,args", TRIAL_CASES, ids=_ids)
def test_one_trial_from_the_start_must_be_accepted_and_is_measurable(oracle, name, args):
    """The longdouble cost at the truth's candidate is below the cost at the start, so the device must accept the trial;
    no component of the truth's step is below 1e-6 of its largest in the sqrt(H_jj) metric; the references' candidates stay
    under the cap."""
    case = BUILD[name](*args)
    shared, poses, flags, part = _start_state(case)
    ev = case.evaluate(oracle, shared, poses, flags, part, ah.LAM_INIT)
    t = ev.truth
    cand_poses = [np.asarray(t["pose_cand"][i], np.float64) if part[i] else poses[i] for i in range(case.n_items)]
    before, after = case.ld_cost(shared, poses, flags, part), case.ld_cost(np.asarray(t["shared_cand"], np.float64), cand_poses, flags, part)
    size = np.abs(t["step"]) * np.sqrt(np.diag(t["H"]))
    print("%s %s: cost %.6g -> %.6g; step components %.3e .. %.3e; A %s  B %s" % (name, _ids(args), float(before), float(after), size.min(),
                                                                               size.max(), *(ev.refs[r] for r in ah.REFS)))
    assert after < before
    assert size.min() >= 1e-6 * size.max()
    assert not ev.conditions(name), ev.conditions(name)
