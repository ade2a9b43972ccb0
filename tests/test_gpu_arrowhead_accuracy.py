"""What vmm_ba_calibrate and vmm_ba_rig_calibrate report, entry by entry against a longdouble truth formed at the device's
own state, flags and participation (tests/arrowhead_cases.py has scenes, truth, references, metric and bound; DESIGN.md
section 4.16 the measured figures).  Every bound is 8 x the larger deviation of two float64 CPU references from that
truth, never a figure of the kernels.

  a. the covariance stage alone (max_trials = 0, reclassify_passes = 0, the shared unknowns perturbed): poses and flags
     are the bytes of engine.localize / engine.rig_localize, the shared unknowns come back as they went in, trials == 0;
     intr_cov / ext_cov, every cam_cov / rig_cov, per-item cost, rms_px, n_inlier_obs and the report's totals within the
     bound at that state, where the residuals are large and the Huber weights active;
  b. the result under the default options: status OK, the flags are the placed labels and so is the longdouble
     classification at the returned state (nothing within 1e-9 px of inlier_px), every quantity of (a) at the returned
     state, covariances symmetric in their bits, held and inactive unknowns returned bit for bit with exactly zero rows
     and columns, the longdouble Gauss-Newton decrement at most 1e-9 of the cost;
  c. one trial (max_trials = 1, reclassify_passes = 0): accepted, and the returned shared unknowns and every pose within
     the bound of the longdouble candidate -(H + lam diag H)^-1 g formed from (a)'s state; initial_cost is (a)'s final_cost;
  d. bits: trailing empty items change nothing, and two calls agree.
The run_* functions return (failures, record); tools/arrowhead_accuracy.py writes the records down.
"""
import json

import numpy as np
import pytest

import arrowhead_cases as ah
import eval_cases as ec
import finished_map_cases as fm

pytestmark = pytest.mark.gpu

LD = ah.LD


# ---- the device ---------------------------------------------------------------------------------------------------------

def call(eng, case, shared0, n_empty=0, **opts):
    """One call of the case's entry from shared0, `n_empty` empty items behind the batch.  Returns a dict: shared,
    shared_cov, poses, item_cov, inl, res, report, n_used."""
    s = case.scene
    o = dict(dict(robustify=int(case.robust), huber_a=case.a, refine_mask=case.mask), **opts)
    if case.entry == "calibrate":
        start = np.concatenate([s.start, np.full(n_empty, s.start[-1])])
        intr, dist, scov, poses, icov, inl, res, rep = eng.calibrate(shared0[:4], shared0[4:], s.tag_gt, s.tag_wh, start, s.obs_tag,
                                                                     s.obs_px, **o)
        shared, n_used = np.concatenate([intr, dist]), rep["n_images_used"]
    else:
        start = np.concatenate([s.img_start, np.full(n_empty * case.K, s.img_start[-1])])
        shared, scov, poses, icov, inl, res, rep = eng.rig_calibrate(s.intr, s.dist, shared0, s.tag_gt, s.tag_wh, start, s.obs_tag,
                                                                     s.obs_px, **o)
        n_used = rep["n_frames_used"]
    return dict(shared=shared, shared_cov=scov, poses=poses, item_cov=icov, inl=inl, res=res, report=rep, n_used=n_used)


def localisation(eng, case, shared0):
    """(poses, flags) of the entry's localisation under shared0 and the default options."""
    s = case.scene
    if case.entry == "calibrate":
        out = eng.localize(shared0[:4], shared0[4:], s.tag_gt, s.tag_wh, s.start, s.obs_tag, s.obs_px)
    else:
        out = eng.rig_localize(s.intr, s.dist, shared0, s.tag_gt, s.tag_wh, s.img_start, s.obs_tag, s.obs_px)
    return out[0], out[2]


def _bytes(d, n):
    """What (d) compares of the first n items: shared unknowns and their covariance, poses, their covariances, flags."""
    return (np.asarray(d["shared"]).tobytes(), d["shared_cov"].tobytes(), d["poses"][:n].tobytes(), d["item_cov"][:n].tobytes(),
            d["inl"].tobytes(), json.dumps(d["res"][:n], sort_keys=True))


def check_state(case, O, d, shared0, label, min_tags, out=print):
    """Everything a result says about its own state: the counts, the quantities of (a) against the bound, symmetry, the
    dead unknowns and the items that take no part.  Returns (failures, evaluation, deviations)."""
    from visual_marker_mapping_amd import _lib
    bad = []
    flags = case.flags_list(d["inl"])
    n_in = [int(f.sum()) for f in flags]
    ok = [r["status"] == _lib.LOC_OK for r in d["res"]]
    part = [ok[i] and n_in[i] >= min_tags for i in range(case.n_items)]
    for i in range(case.n_items):
        # an item that takes no part keeps the localisation's n_inlier_obs, whatever a later pass made of its flags (vmm_ba.h)
        if part[i] and d["res"][i]["n_inlier_obs"] != n_in[i]:
            bad.append("%s item %d: n_inlier_obs %d, %d flags set" % (label, i, d["res"][i]["n_inlier_obs"], n_in[i]))
        if not part[i] and d["item_cov"][i].any():
            bad.append("%s item %d takes no part, but its covariance is not exactly zero" % (label, i))
    rep = d["report"]
    if d["n_used"] != sum(part) or rep["n_obs_used"] != sum(n for n, p in zip(n_in, part) if p):
        bad.append("%s: %d items and %d observations used, the flags say %d and %d"
                   % (label, d["n_used"], rep["n_obs_used"], sum(part), sum(n for n, p in zip(n_in, part) if p)))
    if bad:
        return bad, None, None
    ev = case.evaluate(O, d["shared"], d["poses"], flags, part)
    items = ev.truth["items"]
    got = dict(cost={i: d["res"][i]["cost"] for i in items}, rms={i: d["res"][i]["rms_px"] for i in items}, final_cost=rep["final_cost"],
               final_rms=rep["final_rms_px"], shared_cov=d["shared_cov"], item_cov={i: d["item_cov"][i] for i in items})
    b, dev = ev.check(got, label)
    bad += b + ev.conditions(label)
    if not (fm.symmetric_bits(d["shared_cov"]) and fm.symmetric_bits(d["item_cov"])):
        bad.append("%s: a covariance is not symmetric in its bits" % label)
    dead = np.ones(case.P, bool)
    dead[ev.truth["free"]] = False
    if d["shared_cov"][dead].any() or d["shared_cov"][:, dead].any():
        bad.append("%s: a held or inactive unknown has a row or column of the covariance that is not exactly zero" % label)
    width = 1 if case.entry == "calibrate" else 6
    for u in np.flatnonzero(dead[::width]):
        if np.asarray(d["shared"])[u].tobytes() != np.asarray(shared0)[u].tobytes():
            bad.append("%s: the held or inactive unknown %d did not come back with its input bits" % (label, u))
    for q in ev.bound:
        out("%s %-10s deviation %.3e  bound %.3e  ratio %.3f" % (label, q, dev[q], ev.bound[q], dev[q] / ev.bound[q]))
    return bad, ev, dev


def _record(case, stage, args, ev, dev, **more):
    return dict(entry=case.entry, stage=stage, case=ah.case_id(args), exercises=case.exercises, items=case.n_items,
                observations=int(case.scene.start[-1]),
                reference_deviation={r: ev.refs[r] for r in ah.REFS}, bound=ev.bound, deviation=dev,
                ratio_to_bound={q: dev[q] / ev.bound[q] for q in ev.bound}, truth_correction=ev.truth["correction"], **more)


def _stage_call(eng, case, args, min_tags):
    """(a)'s call, shared with (c): made once per case and left unchanged."""
    return ec.cached(("arrowhead stage", case.entry, args, min_tags),
                     lambda: call(eng, case, case.shared_start(), max_trials=0, reclassify_passes=0, min_inlier_tags=min_tags))


# ---- a. the covariance stage alone ------------------------------------------------------------------------------------------

def run_stage(eng, O, build, args, min_tags=2, out=print):
    case = build(*args)
    label = "%s stage %s%s" % (case.entry, ah.case_id(args), "" if min_tags == 2 else " min_inlier_tags=%d" % min_tags)
    shared0 = case.shared_start()
    d = _stage_call(eng, case, args, min_tags)
    poses, flags = localisation(eng, case, shared0)
    bad = []
    if d["poses"].tobytes() != poses.tobytes() or d["inl"].tobytes() != flags.tobytes():
        bad.append("%s: poses or flags are not the bytes of the localisation under the same model" % label)
    if np.asarray(d["shared"]).tobytes() != np.asarray(shared0).tobytes():
        bad.append("%s: the shared unknowns did not come back as the input bytes" % label)
    if d["report"]["trials"] != 0 or d["report"]["accepted"] != 0:
        bad.append("%s: %d trials" % (label, d["report"]["trials"]))
    one_tag = [i for i, f in enumerate(case.flags_list(d["inl"])) if int(f.sum()) == 1]
    if min_tags == 2 and not one_tag and "observations_per_image" in case.exercises and isinstance(case.exercises["observations_per_image"], list):
        bad.append("%s: no item of one inlier" % label)
    b, ev, dev = check_state(case, O, d, shared0, label, min_tags, out)
    if ev is None:
        return bad + b, None
    if min_tags == 1 and one_tag and not all(i in ev.truth["items"] for i in one_tag):
        bad.append("%s: the item of one tag takes no part" % label)
    return bad + b, _record(case, "covariance stage", args, ev, dev, min_inlier_tags=min_tags)


@pytest.mark.parametrize("args", ah.CALIB_EDGE_CASES, ids=ah.case_id)
def test_calibrate_covariance_stage(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_stage(eng, oracle, ah.observation_edges, args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", ah.RIG_EDGE_CASES, ids=ah.case_id)
def test_rig_calibrate_covariance_stage(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_stage(eng, oracle, ah.rig_edges, args)
    assert not bad, "\n".join(bad)


ONE_TAG = [(ah.observation_edges, ("distorted", True, "huber0.5", 0x1FF)), (ah.rig_edges, (3, True, "huber0.5", None))]


@pytest.mark.parametrize("build,args", ONE_TAG, ids=lambda v: ah.case_id(v) if isinstance(v, tuple) else v.__name__)
def test_the_item_of_one_tag_takes_part_when_asked(oracle, build, args):
    """min_inlier_tags = 1; at the default, in the tests above, it keeps the localisation's pose and a zero covariance."""
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_stage(eng, oracle, build, args, min_tags=1)
    assert not bad, "\n".join(bad)


# ---- b. the result ----------------------------------------------------------------------------------------------------------

def run_result(eng, O, build, args, out=print):
    from visual_marker_mapping_amd import _lib
    case = build(*args)
    s, label = case.scene, "%s result %s" % (case.entry, ah.case_id(args))
    shared0 = case.shared_start()
    d = call(eng, case, shared0)
    rep, bad = d["report"], []
    if rep["status"] != _lib.CAL_OK:
        bad.append("%s: status %d" % (label, rep["status"]))
    if not (d["inl"] == s.label).all():
        bad.append("%s: %d flags differ from the placed labels" % (label, int((d["inl"] != s.label).sum())))
    truth_flags, gap = case.classify(d["shared"], d["poses"])
    if not gap > fm.THRESHOLD_GAP:
        bad.append("%s: a corner distance %.3g px from inlier_px" % (label, gap))
    if not (np.concatenate(truth_flags) == s.label).all():
        bad.append("%s: the longdouble classification at the returned state differs from the labels" % label)
    b, ev, dev = check_state(case, O, d, shared0, label, 2, out)
    if ev is None:
        return bad + b, None
    left = float(ev.truth["decrement"] / ev.truth["final_cost"])
    out("%s: trials %d accepted %d passes %d; decrement %.3e of the cost" % (label, rep["trials"], rep["accepted"], rep["passes"], left))
    if not left <= fm.COST_GAP:
        bad.append("%s: the Gauss-Newton decrement is %.3e of the cost" % (label, left))
    return bad + b, _record(case, "result", args, ev, dev, decrement_over_cost=left, trials=rep["trials"])


@pytest.mark.parametrize("args", ah.CALIB_EDGE_CASES, ids=ah.case_id)
def test_calibrate_result(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_result(eng, oracle, ah.observation_edges, args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", ah.ITEM_COUNTS)
def test_calibrate_result_by_number_of_images(oracle, n):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_result(eng, oracle, ah.item_edges, (n,))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", ah.RIG_EDGE_CASES, ids=ah.case_id)
def test_rig_calibrate_result(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_result(eng, oracle, ah.rig_edges, args)
    assert not bad, "\n".join(bad)


FRAME_CASES = [(n,) for n in ah.FRAME_COUNTS] + [(5, "huber0.5", True)]


@pytest.mark.parametrize("args", FRAME_CASES, ids=ah.case_id)
def test_rig_calibrate_result_by_number_of_frames(oracle, args):
    """The last case frees a camera that saw nothing: it comes back bit for bit, with exactly zero rows and columns."""
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_result(eng, oracle, ah.frame_edges, args)
    assert not bad, "\n".join(bad)


# ---- c. one trial -----------------------------------------------------------------------------------------------------------

def run_trial(eng, O, build, args, out=print):
    from visual_marker_mapping_amd import _lib
    case = build(*args)
    label = "%s trial %s" % (case.entry, ah.case_id(args))
    shared0 = case.shared_start()
    d0 = _stage_call(eng, case, args, 2)
    d1 = call(eng, case, shared0, max_trials=1, reclassify_passes=0)
    rep, bad = d1["report"], []
    if rep["trials"] != 1 or rep["accepted"] != 1:
        bad.append("%s: trials %d, accepted %d" % (label, rep["trials"], rep["accepted"]))
    if np.float64(rep["initial_cost"]).tobytes() != np.float64(d0["report"]["final_cost"]).tobytes():
        bad.append("%s: initial_cost %.17g is not the covariance stage's final_cost %.17g" % (label, rep["initial_cost"],
                                                                                           d0["report"]["final_cost"]))
    flags = case.flags_list(d0["inl"])
    part = [r["status"] == _lib.LOC_OK and int(f.sum()) >= 2 for r, f in zip(d0["res"], flags)]
    ev = case.evaluate(O, shared0, d0["poses"], flags, part, ah.LAM_INIT)
    b, dev = ev.check(dict(shared_cand=d1["shared"], pose_cand={i: d1["poses"][i] for i in ev.truth["items"]}), label)
    bad += ev.conditions(label)
    for i in range(case.n_items):
        if not part[i] and d1["poses"][i].tobytes() != d0["poses"][i].tobytes():
            bad.append("%s item %d takes no part, but its pose moved" % (label, i))
    for q in ev.bound:
        out("%s %-11s deviation %.3e  bound %.3e  ratio %.3f" % (label, q, dev[q], ev.bound[q], dev[q] / ev.bound[q]))
    return bad + b, _record(case, "one trial", args, ev, dev)


@pytest.mark.parametrize("args", ah.CALIB_TRIAL_CASES, ids=ah.case_id)
def test_calibrate_one_trial(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_trial(eng, oracle, ah.observation_edges, args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", ah.RIG_TRIAL_CASES, ids=ah.case_id)
def test_rig_calibrate_one_trial(oracle, args):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_trial(eng, oracle, ah.rig_edges, args)
    assert not bad, "\n".join(bad)


# ---- d. bits ------------------------------------------------------------------------------------------------------------------

def run_bits(eng, build, args, repeat=False):
    """1 .. 4 empty items behind the batch: the bytes of the batch alone, and for the added items the localisation's
    nothing (no part, zero covariance).  repeat: two calls of the batch agree."""
    case = build(*args)
    label = "%s bits %s" % (case.entry, ah.case_id(args))
    shared0, n = case.shared_start(), case.n_items
    alone = call(eng, case, shared0)
    bad = []
    if repeat and _bytes(call(eng, case, shared0), n) != _bytes(alone, n):
        bad.append("%s: two calls give different bytes" % label)
    for n_empty in (1, 2, 3, 4):
        d = call(eng, case, shared0, n_empty=n_empty)
        if _bytes(d, n) != _bytes(alone, n):
            bad.append("%s: %d trailing empty items change the bytes of the batch" % (label, n_empty))
        if d["item_cov"][n:].any() or d["n_used"] != alone["n_used"]:
            bad.append("%s: an empty item has a covariance or takes part" % label)
    return bad


BITS = [(ah.item_edges, (5,), False), (ah.item_edges, (257,), True), (ah.frame_edges, (5,), False), (ah.frame_edges, (65,), True),
        (ah.rig_edges, (4, True, "huber0.5", None), False)]


@pytest.mark.parametrize("build,args,repeat", BITS, ids=lambda v: ah.case_id(v) if isinstance(v, tuple) else getattr(v, "__name__", str(v)))
def test_trailing_empty_items_change_no_bit(build, args, repeat):
    from visual_marker_mapping_amd import engine as eng
    bad = run_bits(eng, build, args, repeat)
    assert not bad, "\n".join(bad)
