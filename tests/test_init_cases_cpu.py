"""CPU checks of tests/init_cases.py, the case module of test_gpu_init_accuracy.py: the longdouble CameraModel chain, the
host restatement of the planar solver and of the growth, the agreement of the two float64 references on every case, and
the conditions the GPU tests rest on (winner margins, resolved trials, a stopping rule before the trials are spent, the
branches of quat_from_R, no pose left out of the argmin comparison).  The states are the host restatement's; the GPU tests
assert the same conditions again at the device's."""
import numpy as np
import pytest

import eval_cases as ec
import finished_map_cases as fm
import init_cases as ic
import ref_geometry as rg

LD = ic.LD
AGREE = 8.0     # references A and B within this factor of each other on every case (the issue's figure)
CHAIN_UNITS = 64.0


def _agree(a, b, what):
    assert a > 0 and b > 0 and max(a, b) <= AGREE * min(a, b), "%s: references A %.3g and B %.3g are further apart than %g x" % (what, a, b, AGREE)


def _host_state(fam, model, winners=False, counts=ic.SELECT_COUNTS):
    """(handle, quads, restatement) of a selection scene with the host's quad poses, computed once."""
    def make():
        h = ic.select_handle(fam, model, winners=winners, counts=counts)
        qt2, rms2 = ic.host_quad(h.intr, h.dist, h.tag_wh[h.obs_tag], h.obs_px)
        return h, (qt2, rms2), ic.restate(h, qt2, rms2, ic.SCORE_CAP_PX, 1)
    return ec.cached(("init cpu state", fam, model, winners, tuple(counts)), make)


# ---- the chain -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", fm.MODELS)
def test_camera_model_chain_against_pnp(model):
    from visual_marker_mapping_amd import pnp
    intr, dist = fm.camera_model(model)
    pc = ic.chain_points(model)
    truth = ic.project_cm(intr, dist, pc)
    mag = np.abs(truth) + np.abs(np.asarray(intr, LD)[2:])
    for name, got in (("A pnp.project", ic.project_cm_a(intr, dist, pc)), ("B float64", ic.project_cm(intr, dist, pc, np.float64))):
        dev = ic.chain_deviation(got, truth, intr)
        print("%s %s: %.2f x 2^-53" % (model, name, dev / 2.0 ** -53))
        assert dev <= CHAIN_UNITS * 2.0 ** -53, (name, dev)
    # without p2 the chain is pnp.project itself; with it the two differ by the aliased term and nothing else
    no_p2 = np.array(dist, np.float64)
    no_p2[3] = 0.0
    plain = pnp.project(pc, np.eye(3), np.zeros(3), tuple(intr), tuple(no_p2))
    assert float((np.abs(plain - ic.project_cm(intr, no_p2, pc)) / mag).max()) <= CHAIN_UNITS * 2.0 ** -53
    if dist[3] != 0.0:
        _, proj, _, _ = ec.corner_chain(intr, dist, [[1.0, 0, 0, 0, 0, 0, 0]] * len(pc), np.c_[np.tile([1.0, 0, 0, 0], (len(pc), 1)), pc],
                                        np.zeros((len(pc), 2)), np.zeros((len(pc), 8)))
        x, y = LD(1) * pc[:, 0] / pc[:, 2], LD(1) * pc[:, 1] / pc[:, 2]
        alias = truth[:, 1] - proj[:, 0, 1]
        xd = (proj[:, 0, 0] - LD(intr[2])) / LD(intr[0])
        assert np.abs(alias - LD(intr[1]) * 2 * LD(dist[3]) * (xd - x) * y).max() <= 1e-12
        assert np.abs(alias).max() > 1e-4            # the term is there: the functor's chain is not this one


def test_quat_from_R_and_the_chains_against_pnp():
    from visual_marker_mapping_amd import pnp
    rng = np.random.default_rng(6)
    q = rng.normal(size=(400, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    R = rg.rotation(q, np.float64)
    got, branch = ic.quat_from_R(R, np.float64)
    assert set(branch.tolist()) == {0, 1, 2, 3}
    want = np.array([pnp.quat_from_R(r) for r in R])
    assert np.abs(got - want).max() <= 8 * 2.0 ** -53
    a, b = np.c_[q[:200], rng.normal(size=(200, 3))], np.c_[q[200:], rng.normal(size=(200, 3))]
    for fam in ic.FAMILIES:
        truth = ic.chained_pose(fam, a, b)
        assert ic.pose_deviation(ic.chained_pose_a(fam, a, b), truth).max() <= 64 * 2.0 ** -53
        assert ic.pose_deviation(ic.chained_pose(fam, a, b, np.float64), truth).max() <= 64 * 2.0 ** -53


# ---- the planar solver ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", fm.MODELS)
def test_host_quad_recovers_exact_poses(model):
    s = ic.exact_batch(model)
    assert set(ic.branches_of(s.qt_gt).tolist()) == {0, 1, 2, 3}
    qt2, rms2 = ic.host_quad(s.intr, s.dist, s.wh, s.px)
    err = ic.recovery_error(qt2[:, 0], s.qt_gt)
    print("%s: worst recovery error %.3g (%s), rms %.3g" % (model, err.max(), s.names[int(np.argmax(err))], rms2[:, 0].max()))
    assert err.max() <= 1e-9 and (rms2[:, 0] <= rms2[:, 1]).all()      # the project's figure for exact data (test_gpu_init.py)
    refs = {k: float(v.max()) for k, v in ic.exact_references(s).items()}
    print(refs)
    assert all(v <= 1e-9 for v in refs.values())


@pytest.mark.parametrize("model", fm.MODELS)
def test_weak_perspective_starts_are_exact_on_exact_data(model):
    """The first order of a plane's homography at the tag centre is exact: one of the two fallback starts is the pose."""
    s = ic.exact_batch(model)
    w = ic.quad_weak_starts(s.intr, s.dist, s.wh, s.px)
    err = np.minimum(ic.recovery_error(w[:, 0], s.qt_gt), ic.recovery_error(w[:, 1], s.qt_gt))
    print("%s: worst error of the better start %.3g (%s)" % (model, err.max(), s.names[int(np.argmax(err))]))
    # pinhole: rounding alone.  Distorted: the pixels carry CameraModel's aliased term (up to 0.02 px), which the
    # undistortion (the functor's model) does not take out: 0.02 px against a tag of 19 px and more
    assert err.max() <= (1e-9 if model == "pinhole" else 1e-3)


@pytest.mark.parametrize("n", ic.QUAD_SIZES)
@pytest.mark.parametrize("model", fm.MODELS)
def test_host_quad_is_stationary(model, n):
    """What the GPU test asks of the device holds for the restatement: every returned solution lies within COST_GAP of the
    optimum reached from it.  Without the fallback three observations of the pinhole batches stall at the saddle between
    the two planar minima (the condition that found the defect, kept as a check that the scenes still contain them)."""
    s = ic.quad_batch(model, n)
    stalled = 0
    for fallback in (False, True):
        qt2, _ = ic.host_quad(s.intr, s.dist, s.wh, s.px, fallback=fallback)
        for k in range(2):
            opt, _ = ic.quad_optimum(s.intr, s.dist, qt2[:, k], s.wh, s.px)
            c0, c1 = ic.quad_cost(s.intr, s.dist, qt2[:, k], s.wh, s.px), ic.quad_cost(s.intr, s.dist, opt, s.wh, s.px)
            above = ((c0 - c1) / c1).astype(np.float64)
            if fallback:
                assert above.max() <= ic.COST_GAP, (k, int(np.argmax(above)), above.max())
            else:
                stalled += int((above > ic.COST_GAP).sum())
    assert (stalled > 0) == ((model, n) in (("pinhole", 63), ("pinhole", 64), ("pinhole", 65)))


def test_host_quad_degenerate_observations():
    s = ic.quad_batch("pinhole", 65)
    px = s.px.copy()
    px[0], px[63], px[64] = ic.DEGENERATE["coincident"], ic.DEGENERATE["collinear"], ic.DEGENERATE["coincident"]
    qt2, rms2 = ic.host_quad(s.intr, s.dist, s.wh, px)
    assert not np.isnan(qt2).any() and np.isposinf(rms2[[0, 63, 64]]).all() and np.isfinite(np.delete(rms2, [0, 63, 64], axis=0)).all()
    assert (qt2[[0, 63, 64]] == ic.IDENTITY_CAM).all()


@pytest.mark.parametrize("n", ic.QUAD_SIZES)
@pytest.mark.parametrize("model", fm.MODELS)
def test_quad_batches_and_their_references(model, n):
    """The builder's assertions (depth, rising radial map, the four branches), the special geometries at the lane edges,
    and references A and B of the RMS within the factor at the host restatement's poses."""
    s = ic.quad_batch(model, n)
    assert all(s.names[p] != "ordinary" for p in ic.special_positions(n))
    if n >= 63:
        assert {"frontal", "oblique 80", "19 px", "close-up", "corner", "w != h"} <= set(s.names)
        width = np.linalg.norm(s.clean_px[s.names.index("19 px")].reshape(4, 2)[1] - s.clean_px[s.names.index("19 px")].reshape(4, 2)[0])
        assert 17.0 <= width <= 21.0, width
        assert len({tuple(w) for w in s.wh.tolist()}) >= 4
    qt2, rms2 = ic.host_quad(s.intr, s.dist, s.wh, s.px)
    assert np.isfinite(rms2).all() and (rms2[:, 0] <= rms2[:, 1]).all()
    a = b = 0.0
    for k in range(2):
        truth = ic.quad_rms(s.intr, s.dist, qt2[:, k], s.wh, s.px)
        a = max(a, float((np.abs(ic.quad_rms_a(s.intr, s.dist, qt2[:, k], s.wh, s.px) - truth) / truth).max()))
        b = max(b, float((np.abs(np.sqrt(0.25 * ic.quad_sums(s.intr, s.dist, qt2[:, k], s.wh, s.px)[0]) - truth) / truth).max()))
    print("%s n=%d: rms references A %.3g B %.3g" % (model, n, a, b))
    _agree(a, b, "quad rms %s n=%d" % (model, n))


# ---- selection ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("winners", [False, True], ids=["noisy", "placed winners"])
@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_selection_scenes_meet_their_conditions(fam, model, winners):
    h, _, res = _host_state(fam, model, winners)
    assert res["rounds"] == 2 and len(res["picks"]) == len(h.counts)
    assert sorted(h.counts) == sorted(ic.SELECT_COUNTS)
    a = b = 0.0
    for (f, p), pk in res["picks"].items():
        assert pk.margin > ic.SCORE_GAP, ("left out", p, pk.margin)
        lab = h.label[pk.usable]
        assert (pk.below[pk.best][~lab] == 0).all(), "an outlier's corner below the cap under the winner"
        assert lab[pk.winner // 2], "an outlier's candidate wins"
        if winners:
            assert pk.winner == 2 * ic.WINNER_AT[h.counts[p]] and pk.margin >= ic.WINNER_MARGIN, (p, pk.winner, pk.margin)
        refs = ic.pick_references(f, pk)
        a, b = max(a, refs["A numpy"]), max(b, refs["B device scheme"])
    if winners:
        assert {pk.winner for pk in res["picks"].values()} >= {0, 62, 64, 1022, 1024}
    print("%s %s: pose references A %.3g B %.3g, smallest margin %.3g" % (fam, model, a, b, min(pk.margin for pk in res["picks"].values())))
    _agree(a, b, "selection %s %s" % (fam, model))


@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_tie_scene_ties(fam, model):
    """score_cap_px = 1e-6 on the noisy scene: no corner of the 513 list lies below the cap under any candidate."""
    h, (qt2, rms2), _ = _host_state(fam, model)
    p = h.counts.index(513)
    oth = h.tag_qt if fam == "cam" else h.cam_qt
    pk = ic.select_pose(fam, h, p, h.lists(fam)[p], np.ones(len(oth), bool), oth, qt2, rms2, ic.TIE_CAP_PX)
    assert pk.below.sum() == 0 and (pk.scores == pk.scores[0]).all() and pk.winner == 0 and pk.margin == 0.0


# ---- one trial, the refinement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_trial_scenes_meet_their_conditions(oracle, fam, model):
    h, _, res = _host_state(fam, model, counts=ic.TRIAL_COUNTS)
    assert sorted(h.counts) == sorted(ic.TRIAL_COUNTS)
    oth = h.tag_qt if fam == "cam" else h.cam_qt
    state = res["cam_qt"] if fam == "cam" else res["tag_qt"]
    a = b = 0.0
    for p, lst in enumerate(h.lists(fam)):
        tr = ic.trial(oracle, fam, h, p, state[p], lst, oth)
        _, spent, why = ic.refine_model(fam, h, p, state[p], lst, oth)
        print("%s %s list of %d: decrease %.3g, references A %.3g B %.3g, correction %.2g; the refinement stops after %d trials (%s)"
              % (fam, model, len(lst), ic.trial_decrease(tr), tr["refs"]["A oracle"], tr["refs"]["B device scheme"], tr["correction"], spent, why))
        assert why != "spent" and spent < ic.REFINE_TRIALS, (p, spent, why)
        if (model, len(lst)) == ("pinhole", 1):
            assert not ic.trial_resolved(tr)      # pinned, not excused silently: the start is the optimum of this very cost
            continue
        assert tr["accepted"] and ic.trial_resolved(tr), (p, ic.trial_decrease(tr))
        assert tr["correction"] <= max(tr["refs"].values()) / 64
        a, b = max(a, tr["refs"]["A oracle"]), max(b, tr["refs"]["B device scheme"])
    _agree(a, b, "trial %s %s" % (fam, model))


# ---- growth, report ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ("corridor", "cross links", "cut", "constant camera", "degenerate end"))
@pytest.mark.parametrize("model", fm.MODELS)
def test_restated_growth_is_the_breadth_first_search(model, variant):
    h = ic.growth_handle(model, variant)
    qt2, rms2 = ic.host_quad(h.intr, h.dist, h.tag_wh[h.obs_tag], h.obs_px)
    res = ic.restate(h, qt2, rms2, ic.SCORE_CAP_PX, 2)
    cam_ok, tag_ok, rounds = ic.reach(h)
    print("%s %s: %d rounds, %d cameras, %d tags" % (model, variant, rounds, cam_ok.sum(), tag_ok.sum()))
    assert res["rounds"] == rounds and np.array_equal(res["cam_placed"], cam_ok) and np.array_equal(res["tag_placed"], tag_ok)
    expect = {"corridor": (13, 12, 12), "cross links": (6, 12, 13), "cut": (7, 6, 6), "constant camera": (8, 12, 11),
              "degenerate end": (12, 11, 12)}[variant]
    assert (rounds, int(cam_ok.sum()), int(tag_ok.sum())) == expect
    a = b = 0.0
    for (f, p), pk in res["picks"].items():
        assert pk.margin > ic.SCORE_GAP, ("left out", f, p, pk.margin)
        refs = ic.pick_references(f, pk)
        a, b = max(a, refs["A numpy"]), max(b, refs["B device scheme"])
    _agree(a, b, "growth %s %s" % (model, variant))
    # every placed pose lands near the truth (the corridor's frame is the origin tag's, or the constant camera's)
    gt_c, gt_t = (h.cam_gt, h.tag_gt)
    if variant != "constant camera":
        return
    for got, gt, ok in ((res["cam_qt"], gt_c, cam_ok), (res["tag_qt"], gt_t, tag_ok)):
        assert np.abs(got[ok, 4:] - gt[ok, 4:]).max() < 0.2


@pytest.mark.parametrize("variant", ("all", "masked", "unreached", "masked, unreached"))
@pytest.mark.parametrize("model", fm.MODELS)
def test_report_references(oracle, model, variant):
    masked, unreached = "masked" in variant.split(", "), "unreached" in variant
    h = ic.report_handle(model, masked, unreached)
    assert sorted(h.counts) == sorted(ic.REPORT_COUNTS)
    cam_ok, tag_ok, _ = ic.reach(h, 1)
    assert cam_ok.sum() == h.n_cams - unreached
    truth, corners = ic.report_truth(h, h.cam_gt, h.tag_gt, cam_ok, tag_ok)
    a = ic.relative(ic.report_a(oracle, h, h.cam_gt, h.tag_gt, cam_ok, tag_ok), truth)
    b = ic.relative(ic.report_b(h, h.cam_gt, h.tag_gt, cam_ok, tag_ok), truth)
    floor = ic.report_floor(h, h.cam_gt, h.tag_gt, cam_ok, tag_ok)
    print("%s %s: %d corners, mean %.6g px, references A %.3g B %.3g, rounding floor %.3g" % (model, variant, corners, float(truth), a, b, floor))
    # The factor between A and B is NOT asserted for this quantity, and cannot be: a mean over thousands of corners is a
    # random walk of their roundings, either reference may end anywhere below the walk's width, and the two came out 1.1 to
    # 31 x apart on these scenes without either being wrong.  What is asserted is that neither is
    # worse than the roundings of its pixels explain.  The GPU bound is 8 x max(A, B) as everywhere.
    print("   A and B are a factor %.3g apart" % (max(a, b) / min(a, b)))
    assert 0 < a <= floor and 0 < b <= floor
