"""The scenes, truth and references of tests/finished_map_cases.py, checked on the CPU before the GPU tests
(test_finished_map_accuracy.py) rely on them: the longdouble chain against the oracle's functor on every scene, the
builders' conditions and prescribed counts, the Newton refinement of every truth inverse, the agreement of references A
and B, and the distance of every observation from the inlier threshold at the host optimum.

Every case is evaluated at the host yardstick's optimum over the clean observations (finished_map_cases.host_states).
"""
import numpy as np
import pytest

import cov_cases as cc
import eval_cases as ec
import finished_map_cases as fm
import ref_algebra as ra
import ref_geometry as rg

LD = fm.LD
AGREE = 8.0     # references A and B within this factor of each other on every case (the issue's figure)
ALL_CASES = [(entry, args) for entry, (_, cases) in fm.BUILDERS.items() for args in cases]


def _ids(v):
    return v if isinstance(v, str) else fm.case_id(v)


# ---- the chain and the oracle ---------------------------------------------------------------------------------------------

def _worst(got, ref, mag):
    got, ref, mag = (np.asarray(v, LD).reshape(-1) for v in (got, ref, mag))
    nz = mag > 0
    assert np.all(got[~nz] == ref[~nz])
    return float(np.max(np.abs(got - ref)[nz] / mag[nz]))


def _observations(s):
    """(intr, dist, cam (n, 7), tag (n, 7), wh (n, 2), px (n, 8)) of every observation of a scene, camera model by model."""
    import rig_cases as rc
    if s.kind == "localize":
        yield s.intr, s.dist, s.cam_gt[s.obs_item], s.tag_gt[s.obs_tag], s.tag_wh[s.obs_tag], s.obs_px
    elif s.kind == "locate":
        yield s.intr, s.dist, s.cam_gt[s.obs_cam], s.tag_gt[s.obs_item], s.tag_wh[s.obs_item], s.obs_px
    elif s.kind == "triangulate":
        yield (s.intr, s.dist, s.cam_gt[s.obs_cam], fm.point_as_tag(s.pts_gt[s.obs_item]), np.zeros((len(s.obs_cam), 2)),
               np.tile(s.obs_px, (1, 4)))
    else:
        for c in range(s.n_rig_cams):
            of = s.obs_cam == c
            cam = np.array([rc.compose(s.ext_qt[c], s.rig_gt[f]) for f in s.obs_frame[of]])
            yield s.intr[c], s.dist[c], cam, s.tag_gt[s.obs_tag[of]], s.tag_wh[s.obs_tag[of]], s.obs_px[of]


SCENES = [("localize", ("pinhole", True)), ("localize", ("distorted", True)), ("locate_tags", ("pinhole", True)),
          ("locate_tags", ("distorted", True)), ("triangulate", ("pinhole", True)), ("triangulate", ("distorted", True)),
          ("rig_localize", (1, True)), ("rig_localize", (3, True)), ("rig_localize", (8, True))]
SCENE_BUILDERS = {"localize": fm.localize_scene, "locate_tags": fm.locate_scene, "triangulate": fm.triangulate_scene,
                  "rig_localize": fm.rig_scene}


@pytest.mark.parametrize("entry,args", SCENES, ids=_ids)
def test_longdouble_chain_and_oracle_describe_the_same_function(oracle, entry, args):
    """Residuals and Jacobians of every observation, entry by entry over the entry's magnitude (section 4.13's metric; a
    pixel coordinate's magnitude is |f xd| + |c| + |obs|: these images reach across the principal point's axes, where
    |proj| + |obs| no longer measures what was added up).  The oracle's functor runs in float64, so section 4.13's figure
    for known answers stored as doubles (64 x 2^-64 beyond the stored rounding) cannot be asked of it: what is asked is
    MARGIN x the deviation of the plain float64 chain (reference B) from the longdouble chain on the same scene, a sample
    of the same class; both are printed in units of 2^-53."""
    s = SCENE_BUILDERS[entry](*args)
    dev_o, dev_b = np.zeros(3), np.zeros(3)
    for intr, dist, cam, tag, wh, px in _observations(s):
        r, proj, Jc, Jt, Jc_mag, Jt_mag = ec.corner_chain(intr, dist, cam, tag, wh, px, LD, want_magnitude=True)
        rb, _, Jcb, Jtb = ec.corner_chain(intr, dist, cam, tag, wh, px, np.float64)
        c = np.asarray(intr[2:4], LD)
        r_mag = np.abs(proj - c) + np.abs(c) + np.abs(np.asarray(px, LD).reshape(-1, 4, 2))
        for n in range(len(cam)):
            if s.kind == "triangulate":
                ro, Jco, Jpo = oracle.point_eval(intr, dist, cam[n], tag[n, 4:], px[n, :2])
                got = ((ro, rb[n, 0], r[n, 0], r_mag[n, 0]), (Jco, Jcb[n, 0], Jc[n, 0], Jc_mag[n, 0]),
                       (Jpo, Jtb[n, 0, :, :3], Jt[n, 0, :, :3], Jt_mag[n, 0, :, :3]))
            else:
                ro, Jco, Jto = oracle.obs_eval(intr, dist, cam[n], tag[n], wh[n], px[n])
                got = ((ro, rb[n], r[n], r_mag[n]), (Jco, Jcb[n], Jc[n], Jc_mag[n]), (Jto, Jtb[n], Jt[n], Jt_mag[n]))
            for k, (o, b, ref, mag) in enumerate(got):
                dev_o[k] = max(dev_o[k], _worst(o, ref, mag))
                dev_b[k] = max(dev_b[k], _worst(b, ref, mag))
    print("%s %s: oracle / float64 chain from the longdouble chain, x 2^-53: residual %.1f / %.1f  J_cam %.1f / %.1f  J_tag %.1f / %.1f"
          % (entry, _ids(args), *(v * 2.0 ** 53 for pair in zip(dev_o, dev_b) for v in pair)))
    assert (dev_o <= fm.MARGIN * dev_b).all(), (dev_o, dev_b)


# ---- the builders ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry,args", SCENES + [(e, (a[0], False)) for e, a in SCENES], ids=_ids)
def test_builder_meets_its_conditions_and_counts(entry, args):
    s = SCENE_BUILDERS[entry](*args)
    lengths = np.diff(s.start)
    assert lengths.tolist() == list(s.counts)
    want = {"localize": fm.LOCALIZE_COUNTS, "locate": fm.LOCATE_COUNTS, "triangulate": fm.TRACK_COUNTS + (2,),
            "rig": fm.RIG_TOTALS + ((fm.RIG_ALL_IN_LAST, fm.RIG_EMPTY_MIDDLE) if s.kind == "rig" and s.n_rig_cams > 1 else ())}
    assert sorted(s.counts) == sorted(want[s.kind])
    assert s.counts != sorted(s.counts)          # shuffled
    width = s.obs_px.shape[1]
    if s.kind in ("locate", "triangulate"):
        for i in range(len(lengths)):
            assert (np.diff(s.obs_cam[s.start[i]:s.start[i + 1]]) > 0).all()
        assert s.cam_cov.shape == (len(s.cam_gt), 6, 6) and (np.linalg.eigvalsh(s.cam_cov) > 0).all()
    if s.kind == "rig":
        K = s.n_rig_cams
        assert np.diff(s.img_start).reshape(-1, K).sum(axis=1).tolist() == list(s.counts)
        assert (np.diff(s.obs_frame) >= 0).all()
        for f in range(s.n_frames):
            assert (np.diff(s.obs_cam[s.start[f]:s.start[f + 1]]) >= 0).all()
        if K > 1:
            assert s.per_frame[-2].tolist() == [0] * (K - 1) + [fm.RIG_ALL_IN_LAST]
            assert s.per_frame[-1][K // 2] == 0 and (np.delete(s.per_frame[-1], K // 2) > 0).all()
            assert len({tuple(np.r_[i, d]) for i, d in zip(s.intr, s.dist)}) == K      # different models
    else:
        relief = s.tag_gt[:, 6] if s.kind != "triangulate" else s.pts_gt[:, 2]
        assert len(relief) < 3 or relief.max() - relief.min() > 0.5                    # not a plane
    # the geometry: every corner in front of its camera, on the rising part of the radial map
    for intr, dist, cam, tag, wh, _ in _observations(s):
        p_cam = rg.camera_points(cam, tag, wh)
        assert (p_cam[..., 2] > 0).all() and (fm.radial_slope(dist, p_cam) > 0).all()
    # the pixels: clean ones within inlier_px / 4 of the noise-free corner, replaced ones 10 .. 40 x inlier_px away, all
    # corners alike, at the list positions 0, 63, 64, 255, 256 and m - 1 of every list that is long enough
    moved = np.linalg.norm((s.obs_px - s.clean_px).reshape(len(s.obs_px), -1, 2), axis=2)
    assert (moved[s.label] <= fm.INLIER_PX / 4).all()
    if args[1]:
        assert (~s.label).any()
        for i, m in enumerate(lengths):
            assert np.flatnonzero(~s.label[s.start[i]:s.start[i + 1]]).tolist() == fm.outlier_positions(int(m))
        # the noise (at most inlier_px / 4) on top of a shift of 10 .. 40 x inlier_px
        assert (moved[~s.label] >= 10 * fm.INLIER_PX - fm.INLIER_PX / 4).all()
        assert (moved[~s.label] <= 40 * fm.INLIER_PX + fm.INLIER_PX / 4).all()
        assert fm.outlier_positions(513) == [0, 63, 64, 255, 256, 512] and fm.outlier_positions(7) == []
    else:
        assert s.label.all()
    assert width == (2 if s.kind == "triangulate" else 8)


# ---- truth and references ---------------------------------------------------------------------------------------------------

def _assert_references(label, ev, items, truth, cap=cc.REFERENCE_CAP):
    """Section 4.14's criterion on every truth inverse, and the references within AGREE of each other per quantity.  A
    scalar can come out nearly exact by luck: a deviation below 2^-53, or for cost and rms below what one rounding of every
    projected pixel does to them (finished_map_cases.Case.rounding_floor), counts as that; the bounds of the GPU tests do not
    use these floors."""
    for i in items:
        smaller = min(d["cov"] for d in ev.refs[i].values())
        assert truth[i]["correction"] <= cc.REFINEMENT_SHARE * smaller, (label, i, truth[i]["correction"], smaller)
    a, b = ev.reference_deviation.values()
    for q in ev.bound:
        floor = max(fm.U64, ev.floor.get(q, 0.0))
        # a sigma is the root of a sum of covariance entries: a reference whose sigma deviates less than half of what its
        # own covariance entries do owes that to cancellation
        own = (0.5 * a["cov"], 0.5 * b["cov"]) if q.startswith("sigma") else (0.0, 0.0)
        lo, hi = sorted((max(a[q], floor, own[0]), max(b[q], floor, own[1])))
        print("%s %-9s A %.3e  B %.3e  bound %.3e" % (label, q, a[q], b[q], ev.bound[q]))
        assert hi <= AGREE * lo, (label, q, a[q], b[q])
        assert ev.bound[q] <= cap, (label, q, ev.bound[q])


@pytest.mark.parametrize("entry,args", ALL_CASES, ids=_ids)
def test_references_agree_at_the_host_optimum(oracle, entry, args):
    case = fm.BUILDERS[entry][0](*args)
    s, label = case.scene, "%s %s" % (entry, fm.case_id(args))
    states, flags, costs = fm.host_states(oracle, case)
    for i in range(case.n_items):
        b, e = case.span(i)
        # nothing is left out of the flag comparison: every observation is far from the threshold, on its label's side
        at_state, gap = case.classify(i, states[i])
        assert gap > fm.THRESHOLD_GAP, (label, i, gap)
        assert (at_state == s.label[b:e]).all(), (label, i)
        # the yardstick's float64 cost is the longdouble cost at its state
        assert abs(float(case.ld_cost(i, states[i], flags[i])) - costs[i]) <= 1e-9 * costs[i], (label, i)
    ev = case.evaluate(oracle, states, flags)
    _assert_references(label, ev, range(case.n_items), ev.truth)
    hard = [i for i in range(case.n_items) if fm.condition_number(ev.truth[i]["H"]) > 1e3]
    for i in hard:
        print("%s item %d (%d observations): condition number %.3g of the scaled normal matrix, references %s"
              % (label, i, s.counts[i], fm.condition_number(ev.truth[i]["H"]),
                 {k: "%.2e" % v["cov"] for k, v in ev.refs[i].items()}))
    if entry in ("localize", "triangulate"):
        assert hard, "the ill-conditioned item of this kind (a single-tag image, a two-view track at low parallax) is gone"


@pytest.mark.parametrize("n_tags,with_map", fm.PREDICT_CASES, ids=lambda v: ("map" if v else "nomap") if isinstance(v, bool) else "%dtags" % v)
def test_predict_references_agree(oracle, n_tags, with_map):
    seen = 0
    for n_poses in fm.PREDICT_POSES:
        case = fm.PredictCase(n_tags, n_poses, with_map)
        visible, on_rounding = case.host_visible()
        assert not on_rounding
        ev = case.evaluate(oracle, visible)
        if ev.items:
            # the sanity cap: a pose that sees one tag of 19 px is the ill-conditioned kind of this entry point
            _assert_references("predict %d x %d" % (n_tags, n_poses), ev, ev.items, ev.truth, cap=1e-6 if n_tags == 1 else cc.REFERENCE_CAP)
            for p in ev.items:
                if fm.condition_number(ev.truth[p]["H"]) > 1e3:
                    print("predict %d x %d pose %d: condition number %.3g of the scaled normal matrix, references %s"
                          % (n_tags, n_poses, p, fm.condition_number(ev.truth[p]["H"]), {k: "%.2e" % v["cov"] for k, v in ev.refs[p].items()}))
        seen += len(ev.items)
    assert seen >= 1


# ---- the device's algebra in float64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 6])
def test_restated_algebra_inverts_and_sandwiches(n):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, 2 * n))
    A = A @ A.T
    C = ra.spd_inverse(A)
    assert (C == C.T).all()
    np.testing.assert_allclose(C @ A, np.eye(n), atol=1e-12)
    S = rng.standard_normal((n, n))
    S = S @ S.T
    W = ra.sandwich(C, S)
    assert (W == W.T).all()
    np.testing.assert_allclose(W, C @ S @ C, rtol=1e-12, atol=1e-15 * np.abs(W).max())
