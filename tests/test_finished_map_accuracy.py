"""What the stateless calls against a finished map report, entry by entry against a longdouble truth formed at the
device's own returned state and flags: vmm_ba_localize, vmm_ba_rig_localize, vmm_ba_locate_tags, vmm_ba_triangulate and
vmm_ba_predict_localization (tests/finished_map_cases.py has scenes, truth, references, metric and bound; DESIGN.md
section 4.15 the measured figures).

Per case (a scene under one loss: plain, Huber 0.5 or 2.5; with and without outliers placed at list positions 0, 63, 64,
255, 256 and m - 1; the list lengths on every stride and staging edge in one shuffled batch):
  * status OK and the prescribed counts;
  * no largest corner distance within 1e-9 px of inlier_px at the returned state, and the flags equal the longdouble
    classification there (predict: the visible bytes equal the header's rules, none of which rests on rounding);
  * cost, rms_px, every covariance and the sigmas within 8 x the larger deviation of the two float64 CPU references from
    the truth over the device's flags; a matrix the contract says is zero is exactly zero;
  * every covariance symmetric in its bits;
  * the longdouble cost at the device's state exceeds the longdouble cost at the host optimum over the same inliers by at
    most 1e-9 relative;
  * every item alone gives the bytes it has in the batch.
The run_* functions return (failures, records); tools/finished_map_accuracy.py writes the records down.
"""
import json

import numpy as np
import pytest

import finished_map_cases as fm
import ref_geometry as rg

pytestmark = pytest.mark.gpu

LD = fm.LD


def _loss_options(case):
    return dict(dict(robustify=int(case.robust), huber_a=case.a), **getattr(case, "options", {}))


# ---- the device's results per entry point: (states, flags, got per item, results, bytes per item) ---------------------------

def _call_localize(eng, case, items=None):
    s = case.scene
    start, sel = _select(s.start, items)
    cam, cov, inl, res = eng.localize(s.intr, s.dist, s.tag_gt, s.tag_wh, start, s.obs_tag[sel], s.obs_px[sel], **_loss_options(case))
    return cam, [cov], inl, res


def _call_rig(eng, case, items=None):
    s = case.scene
    K = s.n_rig_cams
    start, sel = _select(s.start, items)
    frames = range(case.n_items) if items is None else items
    slots = np.concatenate([np.diff(s.img_start[f * K:f * K + K + 1]) for f in frames])
    rig, cov, inl, res = eng.rig_localize(s.intr, s.dist, s.ext_qt, s.tag_gt, s.tag_wh, rg.start(slots), s.obs_tag[sel], s.obs_px[sel],
                                          **_loss_options(case))
    return rig, [cov], inl, res


def _call_locate(eng, case, items=None):
    s = case.scene
    start, sel = _select(s.start, items)
    wh = s.tag_wh if items is None else s.tag_wh[list(items)]
    tag, cov, cov_cams, inl, res = eng.locate_tags(s.intr, s.dist, s.cam_gt, wh, start, s.obs_cam[sel], s.obs_px[sel],
                                                   cam_cov=s.cam_cov if case.with_cams else None, **_loss_options(case))
    return tag, [cov, cov_cams], inl, res


def _call_triangulate(eng, case, items=None):
    s = case.scene
    start, sel = _select(s.start, items)
    xyz, cov, cov_cams, inl, res = eng.triangulate(s.intr, s.dist, s.cam_gt, start, s.obs_cam[sel], s.obs_px[sel],
                                                   cam_cov=s.cam_cov if case.with_cams else None,
                                                   **_loss_options(case))
    return xyz, [cov, cov_cams], inl, res


CALLS = {"localize": _call_localize, "rig_localize": _call_rig, "locate_tags": _call_locate, "triangulate": _call_triangulate}


def _select(start, items):
    """(the start array, the observation indices) of the batch made of `items` in that order (None: the whole batch)."""
    if items is None:
        return start, np.arange(int(start[-1]))
    sel = np.concatenate([np.arange(start[i], start[i + 1]) for i in items] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rg.start([int(start[i + 1] - start[i]) for i in items]), sel


def _item_bytes(state, covs, inl, res, k, b, e):
    return (state[k].tobytes(),) + tuple(c[k].tobytes() for c in covs) + (inl[b:e].tobytes(), json.dumps(res[k], sort_keys=True))


def run_case(eng, O, entry, args, alone=True, out=print, options=None):
    """One case of entry point `entry` on the device: every assertion of the module's docstring.  Returns (failures, record)."""
    from visual_marker_mapping_amd import _lib
    build, _ = fm.BUILDERS[entry]
    case = build(*args)
    if options:
        case.options = options
    s, label = case.scene, "%s %s%s" % (entry, fm.case_id(args), " %s" % options if options else "")
    ok_status = _lib.TRI_OK if entry == "triangulate" else _lib.LOC_OK
    state, covs, inl, res = CALLS[entry](eng, case)
    bad = []
    states, flags = [], []
    for i in range(case.n_items):
        b, e = case.span(i)
        if res[i]["status"] != ok_status or res[i]["n_obs"] != s.counts[i]:
            bad.append("%s item %d: status %d, n_obs %d of %d" % (label, i, res[i]["status"], res[i]["n_obs"], s.counts[i]))
        truth_flags, gap = case.classify(i, state[i])
        if not gap > fm.THRESHOLD_GAP:
            bad.append("%s item %d: a corner distance %.3g px from inlier_px" % (label, i, gap))
        if not (inl[b:e] == truth_flags).all() or res[i]["n_inlier_obs"] != int(truth_flags.sum()):
            bad.append("%s item %d: %d flags differ from the longdouble classification" % (label, i, int((inl[b:e] != truth_flags).sum())))
        if not (inl[b:e] == s.label[b:e]).all():
            bad.append("%s item %d: %d flags differ from the placed outliers" % (label, i, int((inl[b:e] != s.label[b:e]).sum())))
        states.append(state[i])
        flags.append(inl[b:e])
    if bad:     # the truth below is taken over the device's flags: without them there is nothing to compare
        return bad, None
    ev = case.evaluate(O, states, flags)
    worst = {q: 0.0 for q in ev.bound}
    host_states, _, _ = fm.host_states(O, case)     # the flags are the labels: the optimum over the same inliers
    cost_gap = 0.0
    for i in range(case.n_items):
        got = dict(cost=res[i]["cost"], rms=res[i]["rms_px"], cov=covs[0][i], prop=covs[1][i] if len(covs) > 1 else None)
        if len(covs) > 1 and ev.truth[i]["prop"] is None and covs[1][i].any():
            bad.append("%s item %d: a propagated part without cam_cov is not exactly zero" % (label, i))
        b_i, dev = ev.check(i, got, label)
        bad += b_i
        for q, v in dev.items():
            worst[q] = max(worst[q], v)
        if not all(fm.symmetric_bits(c[i]) for c in covs):
            bad.append("%s item %d: a covariance is not symmetric in its bits" % (label, i))
        at_device, at_host = case.ld_cost(i, states[i], flags[i]), case.ld_cost(i, host_states[i], flags[i])
        gap = float((at_device - at_host) / at_host)
        cost_gap = max(cost_gap, gap)
        if not gap <= fm.COST_GAP:
            bad.append("%s item %d: cost %.15g at the device's state, %.15g at the host optimum (%.3g relative)"
                       % (label, i, float(at_device), float(at_host), gap))
    for q in ev.bound:
        out("%s %-4s deviation %.3e  bound %.3e  ratio %.3f" % (label, q, worst[q], ev.bound[q], worst[q] / ev.bound[q]))
    out("%s cost above the host optimum's: %.3g relative" % (label, cost_gap))
    if alone:
        for i in range(case.n_items):
            b, e = case.span(i)
            one = CALLS[entry](eng, case, [i])
            if _item_bytes(*one, 0, 0, e - b) != _item_bytes(state, covs, inl, res, i, b, e):
                bad.append("%s item %d (%d observations): alone it gives other bytes than in the batch" % (label, i, e - b))
    rec = dict(entry=entry, case=fm.case_id(args), options=options or {}, items=case.n_items, observations=int(s.start[-1]),
               reference_deviation=ev.reference_deviation, bound=ev.bound, deviation=worst,
               ratio_to_bound={q: worst[q] / ev.bound[q] for q in ev.bound}, cost_above_host_optimum=cost_gap)
    return bad, rec


@pytest.mark.parametrize("args", fm.LOCALIZE_CASES, ids=fm.case_id)
def test_localize(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_case(eng, oracle, "localize", args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", fm.RIG_CASES, ids=fm.case_id)
def test_rig_localize(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_case(eng, oracle, "rig_localize", args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", fm.LOCATE_CASES, ids=fm.case_id)
def test_locate_tags(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_case(eng, oracle, "locate_tags", args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", fm.TRIANGULATE_CASES, ids=fm.case_id)
def test_triangulate(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_case(eng, oracle, "triangulate", args)
    assert not bad, "\n".join(bad)


# max_pair_views 2 and 64 (16 is the default of the cases above); the outliers sit among the first views, so two pair views
# are only asked of clean tracks
PAIR_VIEWS = [(("distorted", False, "huber0.5", True), 2), (("pinhole", False, "plain", False), 2),
              (("distorted", True, "huber2.5", True), 64), (("pinhole", True, "plain", False), 64)]


@pytest.mark.parametrize("args,max_pair", PAIR_VIEWS, ids=lambda v: fm.case_id(v) if isinstance(v, tuple) else "pairs%d" % v)
def test_triangulate_pair_views(oracle, args, max_pair):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_case(eng, oracle, "triangulate", args, options=dict(max_pair_views=max_pair))
    assert not bad, "\n".join(bad)


def run_triangulate_batches(eng, args):
    """n_pts of 1, 3, 4, 5 and 9 (whole and partial workgroups of four waves): the leading points of the batch give the
    bytes they have in the whole batch of ten.  Returns the failures."""
    case = fm.triangulate_case(*args)
    whole = _call_triangulate(eng, case)
    bad = []
    for n in (1, 3, 4, 5, 9):
        part = _call_triangulate(eng, case, list(range(n)))
        for i in range(n):
            b, e = case.span(i)
            if _item_bytes(*part, i, b, e) != _item_bytes(*whole, i, b, e):
                bad.append("triangulate %s: point %d of a batch of %d differs from the batch of %d" % (fm.case_id(args), i, n, case.n_items))
    return bad


@pytest.mark.parametrize("args", [fm.TRIANGULATE_CASES[0], fm.TRIANGULATE_CASES[-1]], ids=fm.case_id)
def test_triangulate_batch_sizes(args):
    from visual_marker_mapping_amd import engine as eng
    bad = run_triangulate_batches(eng, args)
    assert not bad, "\n".join(bad)


def run_too_few(eng, entry, args):
    """min_inlier_tags / min_inlier_views = 4: the items of fewer observations end TOO_FEW_INLIERS with covariances that
    are exactly zero (the contract for every status but OK), the others stay OK.  Returns the failures."""
    from visual_marker_mapping_amd import _lib
    case = fm.BUILDERS[entry][0](*args)
    case.options = {"min_inlier_views" if entry == "triangulate" else "min_inlier_tags": 4}
    _, covs, _, res = CALLS[entry](eng, case)
    few = _lib.TRI_TOO_FEW_INLIERS if entry == "triangulate" else _lib.LOC_TOO_FEW_INLIERS
    bad, n_few = [], 0
    for i, n in enumerate(case.scene.counts):
        if res[i]["status"] != (few if n < 4 else 0):
            bad.append("%s item %d of %d observations: status %d" % (entry, i, n, res[i]["status"]))
        if n < 4:
            n_few += 1
            if any(c[i].any() for c in covs):
                bad.append("%s item %d: status %d with a covariance that is not exactly zero" % (entry, i, res[i]["status"]))
        elif not covs[0][i].any():
            bad.append("%s item %d: no covariance" % (entry, i))
    return bad + ([] if n_few else ["%s: no item below four observations" % entry])


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_a_status_other_than_ok_leaves_exact_zeros(entry):
    from visual_marker_mapping_amd import engine as eng
    args = next(a for a in fm.BUILDERS[entry][1] if a[1] is False and a[-1] is not False)   # clean; with cam_cov where there is one
    bad = run_too_few(eng, entry, args)
    assert not bad, "\n".join(bad)


# ---- the prediction -----------------------------------------------------------------------------------------------------------

def run_predict(eng, O, n_tags, with_map, out=print):
    """n_tags tags under 1, 3, 4 and 5 poses.  Returns (failures, records)."""
    from visual_marker_mapping_amd import _lib
    bad, recs = [], []
    for n_poses in fm.PREDICT_POSES:
        case = fm.PredictCase(n_tags, n_poses, with_map)
        c, label = case.case, "predict %d tags x %d poses %s" % (n_tags, n_poses, "map" if with_map else "nomap")
        want, on_rounding = case.host_visible()
        if on_rounding:
            bad.append("%s: a visibility flag rests on rounding" % label)

        def call(poses):
            return eng.predict_localization(c["intr"], c["dist"], c["tag_qt"], c["tag_wh"], c["cam_qt"][poses], c["size"],
                                            tag_cov=case.tag_cov, want_visible=True, sigma_px=case.sigma_px)
        cov_px, cov_map, res, vis = call(list(range(n_poses)))
        if not (vis == want).all():
            bad.append("%s: %d visible bytes differ from the header's rules" % (label, int((vis != want).sum())))
            continue
        ev = case.evaluate(O, vis)
        worst = {q: 0.0 for q in ev.bound}
        for p in range(n_poses):
            n_vis = int(vis[p].sum())
            if res[p]["n_visible"] != n_vis or res[p]["status"] != (_lib.PRED_OK if n_vis else _lib.PRED_NO_VISIBLE_TAG):
                bad.append("%s pose %d: status %d, n_visible %d of %d" % (label, p, res[p]["status"], res[p]["n_visible"], n_vis))
                continue
            if not n_vis:
                if cov_px[p].any() or cov_map[p].any() or res[p]["sigma_pos_m"] != 0 or res[p]["sigma_rot_rad"] != 0:
                    bad.append("%s pose %d: no visible tag, but a result that is not exactly zero" % (label, p))
                continue
            if not with_map and cov_map[p].any():
                bad.append("%s pose %d: cov_map without tag_cov is not exactly zero" % (label, p))
            got = dict(cov=cov_px[p], prop=cov_map[p], sigma_pos=res[p]["sigma_pos_m"], sigma_rot=res[p]["sigma_rot_rad"])
            b_p, dev = ev.check(p, got, label)
            bad += b_p
            for q, v in dev.items():
                worst[q] = max(worst[q], v)
            if not (fm.symmetric_bits(cov_px[p]) and fm.symmetric_bits(cov_map[p])):
                bad.append("%s pose %d: a covariance is not symmetric in its bits" % (label, p))
            one = call([p])
            if (one[0][0].tobytes(), one[1][0].tobytes(), one[2][0], one[3][0].tobytes()) != \
                    (cov_px[p].tobytes(), cov_map[p].tobytes(), res[p], vis[p].tobytes()):
                bad.append("%s pose %d: alone it gives other bytes than in the batch" % (label, p))
        if not ev.items:
            continue
        for q in ev.bound:
            out("%s %-9s deviation %.3e  bound %.3e  ratio %.3f" % (label, q, worst[q], ev.bound[q], worst[q] / ev.bound[q]))
        recs.append(dict(entry="predict", case="%dx%d-%s" % (n_tags, n_poses, "map" if with_map else "nomap"), items=len(ev.items),
                         observations=int(vis.sum()), reference_deviation=ev.reference_deviation, bound=ev.bound, deviation=worst,
                         ratio_to_bound={q: worst[q] / ev.bound[q] for q in ev.bound}))
    return bad, recs


@pytest.mark.parametrize("n_tags,with_map", fm.PREDICT_CASES, ids=lambda v: ("map" if v else "nomap") if isinstance(v, bool) else "%dtags" % v)
def test_predict(oracle, n_tags, with_map):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_predict(eng, oracle, n_tags, with_map)
    assert not bad, "\n".join(bad)
