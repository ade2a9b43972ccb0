"""The one-shot map initialisation stage by stage against a longdouble truth formed at the device's own returned state:
vmm_ba_quad_poses and vmm_ba_initialize (tests/init_cases.py has scenes, truth, references, the host restatement, metric
and bound; DESIGN.md section 4.17 the measured figures).  The stronger check beside test_gpu_init.py.

  1. the planar solver: rms2 against the longdouble RMS at the returned pose, the order of the two solutions, unit
     quaternions, stationarity, the two optima of the host restatement, exact data, degenerate observations in a batch;
  2. selection alone (refine_iterations = 0, sweeps = 0): the returned pose is exactly one candidate formed from
     engine.quad_poses, and that one is the longdouble argmin; placed winners up to candidate 2 m - 1, exact ties, masks;
  3. one Levenberg-Marquardt trial against the longdouble step, and the converged refinement against the host optimum;
  4. growth, sweep and report against the host restatement; a second call changes no bit.
The run_* functions return (failures, records); tools/init_accuracy.py writes the records down.
"""
import numpy as np
import pytest

import finished_map_cases as fm
import init_cases as ic

pytestmark = pytest.mark.gpu

LD = ic.LD
UNIT_TOL = 4 * 2.0 ** -53     # |q| of a quaternion scaled by one rounded reciprocal square root: a few roundings
SELECT_OPTIONS = dict(sweeps=0, refine_iterations=0, score_cap_px=ic.SCORE_CAP_PX, min_tag_observations=1)


def _eng():
    from visual_marker_mapping_amd import engine as eng
    return eng


def _record(entry, case, refs, bound, deviation, **more):
    ratio = {q: (deviation[q] / bound[q] if bound[q] else (0.0 if deviation[q] == 0 else float("inf"))) for q in deviation}
    return dict(dict(entry=entry, case=case, reference_deviation=refs, bound=bound, deviation=deviation, ratio_to_bound=ratio), **more)


def _check(bad, label, rec):
    for q, r in rec["ratio_to_bound"].items():
        print("%s %-6s deviation %.3e bound %.3e ratio %.3f" % (label, q, rec["deviation"][q], rec["bound"][q], r))
        if not r <= 1.0:
            bad.append("%s %s: deviation %.3e above the bound %.3e" % (label, q, rec["deviation"][q], rec["bound"][q]))


# ---- 1. the planar solver -----------------------------------------------------------------------------------------------

def run_chain(eng, model):
    """The longdouble CameraModel::projectPoint chain, the truth of k_quad_pose, against engine.project_points: the device
    may deviate 8 x as far per entry magnitude as the float64 chain itself."""
    intr, dist = fm.camera_model(model)
    pc = ic.chain_points(model)
    truth = ic.project_cm(intr, dist, pc)
    refs = {"A pnp.project": dict(chain=ic.chain_deviation(ic.project_cm_a(intr, dist, pc), truth, intr)),
            "B float64 chain": dict(chain=ic.chain_deviation(ic.project_cm(intr, dist, pc, np.float64), truth, intr))}
    rec = _record("projection", model, refs, dict(chain=ic.MARGIN * refs["B float64 chain"]["chain"]),
                  dict(chain=ic.chain_deviation(eng.project_points(intr, dist, pc), truth, intr)), points=len(pc))
    bad = []
    _check(bad, "chain %s (%d points)" % (model, len(pc)), rec)
    return bad, rec


@pytest.mark.parametrize("model", fm.MODELS)
def test_camera_model_chain_is_the_device_projection(model):
    bad, _ = run_chain(_eng(), model)
    assert not bad, "\n".join(bad)


def run_quad(eng, model, n):
    s = ic.quad_batch(model, n)
    label = "quad %s n=%d" % (model, n)
    qt2, rms2 = eng.quad_poses(s.intr, s.dist, s.wh, s.px)
    bad = []
    if not (np.isfinite(qt2).all() and np.isfinite(rms2).all()):
        return ["%s: a non-finite result on an ordinary observation" % label], None
    if not (rms2[:, 0] <= rms2[:, 1]).all():
        bad.append("%s: rms2[:, 0] > rms2[:, 1] somewhere" % label)
    norm = np.abs(np.sqrt((qt2[..., :4].astype(LD) ** 2).sum(axis=-1)) - 1).max()
    if not norm <= UNIT_TOL:
        bad.append("%s: a quaternion %.3g from unit length" % (label, norm))
    dev, ref_a, ref_b, gap, pair = 0.0, 0.0, 0.0, 0.0, 0.0
    host, _ = ic.host_quad(s.intr, s.dist, s.wh, s.px, max_trials=400)
    c_dev = np.stack([ic.quad_cost(s.intr, s.dist, qt2[:, k], s.wh, s.px) for k in range(2)], axis=1)
    c_host = np.sort(np.stack([ic.quad_cost(s.intr, s.dist, host[:, k], s.wh, s.px) for k in range(2)], axis=1), axis=1)
    for k in range(2):
        truth = ic.quad_rms(s.intr, s.dist, qt2[:, k], s.wh, s.px)
        dev = max(dev, float((np.abs(rms2[:, k] - truth) / truth).max()))
        ref_a = max(ref_a, float((np.abs(ic.quad_rms_a(s.intr, s.dist, qt2[:, k], s.wh, s.px) - truth) / truth).max()))
        ref_b = max(ref_b, float((np.abs(np.sqrt(0.25 * ic.quad_sums(s.intr, s.dist, qt2[:, k], s.wh, s.px)[0]) - truth) / truth).max()))
        opt, _ = ic.quad_optimum(s.intr, s.dist, qt2[:, k], s.wh, s.px)
        c_opt = ic.quad_cost(s.intr, s.dist, opt, s.wh, s.px)
        above = ((c_dev[:, k] - c_opt) / c_opt).astype(np.float64)
        gap = max(gap, float(above.max()))
        for i in np.flatnonzero(above > ic.COST_GAP):
            bad.append("%s observation %d (%s) solution %d: cost %.9g, %.3g above the optimum reached from it"
                       % (label, i, s.names[i], k, float(c_dev[i, k]), above[i]))
    apart = (np.abs(np.sort(c_dev, axis=1) - c_host) / c_host).astype(np.float64)
    pair = float(apart.max())
    for i, k in zip(*np.nonzero(apart > ic.COST_GAP)):
        bad.append("%s observation %d (%s): cost %.9g of solution %d against %.9g of the host restatement's"
                   % (label, i, s.names[i], float(np.sort(c_dev, axis=1)[i, k]), k, float(c_host[i, k])))
    if n >= 63:
        seen = set(ic.branches_of(qt2[:, 0]).tolist()) | set(ic.branches_of(qt2[:, 1]).tolist())
        if seen != {0, 1, 2, 3}:
            bad.append("%s: the returned quaternions come from branches %s of quat_from_R only" % (label, sorted(seen)))
    rec = _record("quad_poses", "%s n=%d" % (model, n), {"A pnp.project": dict(rms=ref_a), "B device scheme": dict(rms=ref_b)},
                  dict(rms=ic.MARGIN * max(ref_a, ref_b)), dict(rms=dev), cost_above_optimum=gap, cost_from_host_optima=pair)
    print("%s: cost above the optimum reached from it %.3g, from the host restatement's optima %.3g (%.0e is asked)"
          % (label, gap, pair, ic.COST_GAP))
    _check(bad, label, rec)
    return bad, rec


@pytest.mark.parametrize("n", ic.QUAD_SIZES)
@pytest.mark.parametrize("model", fm.MODELS)
def test_quad_poses_per_solution(model, n):
    """rms2, order, unit quaternions, stationarity, the host restatement's two optima, the branches of quat_from_R.  Three
    of these cases (pinhole n = 63, 64, 65) failed their stationarity assertion before k_quad_pose got its fallback start:
    DESIGN.md section 4.17 has the figures."""
    bad, _ = run_quad(_eng(), model, n)
    assert not bad, "\n".join(bad[:20])


def run_quad_exact(eng, model):
    s = ic.exact_batch(model)
    qt2, rms2 = eng.quad_poses(s.intr, s.dist, s.wh, s.px)
    refs = {k: float(v.max()) for k, v in ic.exact_references(s).items()}
    err = ic.recovery_error(qt2[:, 0], s.qt_gt)
    rec = _record("quad_poses", "%s exact" % model, {k: dict(recovery=v) for k, v in refs.items()},
                  dict(recovery=ic.MARGIN * max(refs.values())), dict(recovery=float(err.max())))
    bad = []
    _check(bad, "quad %s exact (worst: %s)" % (model, s.names[int(np.argmax(err))]), rec)
    return bad, rec


@pytest.mark.parametrize("model", fm.MODELS)
def test_quad_poses_exact_data(model):
    bad, _ = run_quad_exact(_eng(), model)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("model", fm.MODELS)
def test_quad_poses_degenerate_in_a_batch(model):
    """Degenerate observations at positions 0, 63 and 64 of a batch of 65: +inf and the documented pose; every other
    observation has the bytes it has alone.  Under distortion a quad collinear in pixels is not collinear in normalised
    coordinates: it may come back finite, never NaN."""
    eng = _eng()
    s = ic.quad_batch(model, 65)
    px = s.px.copy()
    kinds = {0: "coincident", 63: "collinear", 64: "coincident"}
    for p, kind in kinds.items():
        px[p] = ic.DEGENERATE[kind]
    qt2, rms2 = eng.quad_poses(s.intr, s.dist, s.wh, px)
    assert not np.isnan(qt2).any() and not np.isnan(rms2).any()
    for p, kind in kinds.items():
        if kind == "coincident" or model == "pinhole":
            assert np.isposinf(rms2[p]).all(), (p, kind, rms2[p])
        for k in range(2):
            if np.isposinf(rms2[p, k]):
                assert qt2[p, k].tobytes() == ic.IDENTITY_CAM.tobytes(), (p, k, qt2[p, k])
    for i in range(65):
        if i not in kinds:
            q1, r1 = eng.quad_poses(s.intr, s.dist, s.wh[i:i + 1], px[i:i + 1])
            assert q1[0].tobytes() == qt2[i].tobytes() and r1[0].tobytes() == rms2[i].tobytes(), i


# ---- 2. selection alone ---------------------------------------------------------------------------------------------------

def _initialize(eng, h, **options):
    """(report, cam_ok, tag_ok, cam_qt, tag_qt, the same of a second call on the same handle)."""
    with ic.open_handle(eng, h) as ba:
        first = ba.initialize(**options) + ba.get_state()
        second = ba.initialize(**options) + ba.get_state()
    return first, second


def _same_call(a, b):
    ra, rb = dict(a[0], time_s=0.0), dict(b[0], time_s=0.0)
    return ra == rb and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def _device_quads(eng, h):
    return eng.quad_poses(h.intr, h.dist, h.tag_wh[h.obs_tag], h.obs_px)


def check_picks(h, res, cam_qt, tag_qt, label, bad, winners=False):
    """Every placed pose of the restatement `res` against the device's state: exactly one candidate within the bound, that
    one the longdouble argmin, no pose left out for a narrow margin.  Returns (refs, deviation)."""
    refs, dev, rows = {"A numpy": 0.0, "B device scheme": 0.0}, 0.0, []
    for (fam, p), pk in sorted(res["picks"].items()):
        for k, v in ic.pick_references(fam, pk).items():
            refs[k] = max(refs[k], v)
        got = (cam_qt if fam == "cam" else tag_qt)[p]
        rows.append((fam, p, pk, ic.pose_deviation(np.tile(got, (len(pk.poses), 1)), pk.poses)))
    bound = ic.MARGIN * max(refs.values())
    for fam, p, pk, d in rows:
        near = np.flatnonzero(d <= bound)
        dev = max(dev, float(d[pk.best]))
        if not pk.margin > ic.SCORE_GAP:
            bad.append("%s %s %d: the two best scores lie %.3g apart, the pose is left out" % (label, fam, p, pk.margin))
        if len(near) != 1 or near[0] != pk.best:
            bad.append("%s %s %d: the device's pose is candidate(s) %s within the bound, the longdouble argmin is %d (%.3g off)"
                       % (label, fam, p, pk.index[near].tolist(), pk.winner, d[pk.best]))
        lab = h.label[pk.usable] if hasattr(h, "label") else np.ones(len(pk.usable), bool)
        if (pk.below[pk.best][~lab] != 0).any():
            bad.append("%s %s %d: an outlier's corner adds less than cap^2 to the winner's score" % (label, fam, p))
        if pk.winner >= 0 and not lab[np.flatnonzero(pk.use).tolist().index(pk.winner // 2)]:
            bad.append("%s %s %d: an outlier's candidate wins" % (label, fam, p))
        if winners:
            if pk.winner != 2 * h.winner[p]:
                bad.append("%s %s %d: candidate %d wins, not the exact observation's %d" % (label, fam, p, pk.winner, 2 * h.winner[p]))
            if not pk.margin >= ic.WINNER_MARGIN:
                bad.append("%s %s %d: the placed winner wins by %.3g only" % (label, fam, p, pk.margin))
    return refs, bound, dev


def check_reach(h, res, first, label, bad, start=None):
    """rounds, counts and flags against the restatement; poses that were not placed, and constant ones, keep their bytes."""
    report, cam_ok, tag_ok, cam_qt, tag_qt = first
    if report["rounds"] != res["rounds"]:
        bad.append("%s: %d rounds, the restatement has %d" % (label, report["rounds"], res["rounds"]))
    if not (np.array_equal(cam_ok, res["cam_placed"]) and np.array_equal(tag_ok, res["tag_placed"])):
        bad.append("%s: reached flags differ from the restatement (cameras %s, tags %s)"
                   % (label, np.flatnonzero(cam_ok != res["cam_placed"]).tolist(), np.flatnonzero(tag_ok != res["tag_placed"]).tolist()))
    if report["cams_reached"] != int(cam_ok.sum()) or report["tags_reached"] != int(tag_ok.sum()):
        bad.append("%s: the report's counts differ from its flags" % label)
    for fam, got, ok, was in (("cam", cam_qt, cam_ok, h.cam_qt), ("tag", tag_qt, tag_ok, h.tag_qt)):
        keep = ~ok | h.const(fam)
        if got[keep].tobytes() != np.asarray(was, np.float64)[keep].tobytes():
            bad.append("%s: a %s pose that is constant or was not reached lost its bytes" % (label, fam))


def run_select(eng, fam, model, winners):
    h = ic.select_handle(fam, model, winners=winners)
    label = "select %s %s%s" % (fam, model, " winners" if winners else "")
    first, second = _initialize(eng, h, **SELECT_OPTIONS)
    bad = []
    if not _same_call(first, second):
        bad.append("%s: a second call changed a bit" % label)
    qt2, rms2 = _device_quads(eng, h)
    res = ic.restate(h, qt2, rms2, ic.SCORE_CAP_PX, 1, known=first[3:5])
    if res["rounds"] != 2:
        bad.append("%s: the restatement needs %d rounds" % (label, res["rounds"]))
    check_reach(h, res, first, label, bad)
    n_own = h.n_cams if fam == "cam" else h.n_tags
    if len(res["picks"]) != n_own:
        bad.append("%s: %d of %d poses placed" % (label, len(res["picks"]), n_own))
    refs, bound, dev = check_picks(h, res, first[3], first[4], label, bad, winners)
    rec = _record("select", "%s %s%s" % (fam, model, " winners" if winners else ""), {k: dict(pose=v) for k, v in refs.items()},
                  dict(pose=bound), dict(pose=dev), smallest_margin=min(pk.margin for pk in res["picks"].values()))
    _check(bad, label, rec)
    return bad, rec


@pytest.mark.parametrize("winners", [False, True], ids=["noisy", "placed winners"])
@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_selection_is_the_longdouble_argmin(fam, model, winners):
    bad, _ = run_select(_eng(), fam, model, winners)
    assert not bad, "\n".join(bad[:20])


def _tie_masks(h, p):
    lst = h.lists(h.own)[p]
    out = []
    for pos in (0, 63, 64, 512):
        mask = np.ones(h.n_obs, np.uint8)
        mask[lst[:pos]] = 0
        out.append((pos, mask))
    return out


@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_exact_ties_go_to_the_first_candidate(fam, model):
    """score_cap_px = 1e-6: every corner adds the same cap^2 in the same order, all scores have the same bits, and solution
    0 of the first usable observation must win -- at list positions 0, 63, 64 and 512 (thread 0's second trip), and once
    behind a degenerate first observation."""
    eng = _eng()
    h0 = ic.select_handle(fam, model)
    p = h0.counts.index(513)
    lst = h0.lists(fam)[p]
    degenerate = h0.copy()
    degenerate.obs_px[lst[0]] = ic.DEGENERATE["coincident"]
    options = dict(SELECT_OPTIONS, score_cap_px=ic.TIE_CAP_PX)
    bad = []
    for h, cases in ((h0, _tie_masks(h0, p)), (degenerate, [(1, np.ones(h0.n_obs, np.uint8))])):
        qt2, rms2 = _device_quads(eng, h)
        with ic.open_handle(eng, h) as ba:
            for pos, mask in cases:
                ba.set_state(h.cam_qt, h.tag_qt)
                ba.set_observation_mask(mask)
                ba.initialize(**options)
                state = ba.get_state()
                hm = h.copy(mask=mask)
                oth = state[1] if fam == "cam" else state[0]
                placed_other = np.ones(len(oth), bool)
                pk = ic.select_pose(fam, hm, p, lst, placed_other, oth, qt2, rms2, ic.TIE_CAP_PX)
                label = "ties %s %s first usable at %d" % (fam, model, pos)
                assert pk.below.sum() == 0 and (pk.scores == pk.scores[0]).all(), label
                assert pk.winner == 2 * pos, (label, pk.winner)
                refs = ic.pick_references(fam, pk)
                d = ic.pose_deviation(np.tile((state[0] if fam == "cam" else state[1])[p], (len(pk.poses), 1)), pk.poses)
                near = np.flatnonzero(d <= ic.MARGIN * max(refs.values()))
                print("%s: winner %d, %.3g off its chain (bound %.3g)" % (label, pk.index[int(np.argmin(d))], d[pk.best],
                                                                         ic.MARGIN * max(refs.values())))
                if len(near) != 1 or near[0] != pk.best:
                    bad.append("%s: the device's pose is candidate(s) %s, not %d" % (label, pk.index[near].tolist(), pk.winner))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_masked_observations_take_no_part(fam, model):
    """A masked observation gives no candidate and no score term: the selected poses are byte-identical to those of a
    handle built without the masked observations (every third one and the list edges 0, 63, 64 of every list)."""
    eng = _eng()
    h = ic.select_handle(fam, model)
    mask = np.ones(h.n_obs, np.uint8)
    mask[::3] = 0
    for lst in h.lists(fam):
        if len(lst) > 2:
            mask[lst[[q for q in (0, 63, 64) if q < len(lst)]]] = 0
    (_, c1, t1, cam1, tag1), _ = _initialize(eng, h.copy(mask=mask), **SELECT_OPTIONS)
    (_, c2, t2, cam2, tag2), _ = _initialize(eng, h.without(mask), **SELECT_OPTIONS)
    assert np.array_equal(c1, c2) and np.array_equal(t1, t2)
    assert cam1.tobytes() == cam2.tobytes() and tag1.tobytes() == tag2.tobytes()
    unmasked = _initialize(eng, h, **SELECT_OPTIONS)[0]
    assert unmasked[3].tobytes() != cam1.tobytes() or unmasked[4].tobytes() != tag1.tobytes()


# ---- 3. one trial and the converged refinement ---------------------------------------------------------------------------

def _own(fam, pair):
    return pair[0] if fam == "cam" else pair[1]


def run_trial(eng, O, fam, model):
    h = ic.select_handle(fam, model, counts=ic.TRIAL_COUNTS)
    label = "trial %s %s" % (fam, model)
    (_, _, _, cam0, tag0), _ = _initialize(eng, h, **SELECT_OPTIONS)
    (_, _, _, cam1, tag1), _ = _initialize(eng, h, **dict(SELECT_OPTIONS, refine_iterations=1))
    oth = tag0 if fam == "cam" else cam0
    bad, refs, rows, unresolved = [], {"A oracle": 0.0, "B device scheme": 0.0}, [], []
    for p, lst in enumerate(h.lists(fam)):
        start, got = _own(fam, (cam0, tag0))[p], _own(fam, (cam1, tag1))[p]
        tr = ic.trial(O, fam, h, p, start, lst, oth)
        m = len(lst)
        if not ic.trial_resolved(tr):
            if (model, m) != ("pinhole", 1):
                bad.append("%s list of %d: the trial's decrease %.3g is not resolved" % (label, m, ic.trial_decrease(tr)))
                continue
            # The start is the optimum of this very cost and rounding decides whether the trial is accepted: the pose is
            # the start (its translation bit for bit, its quaternion to the rounding of k_init_refine's normalisation) or
            # the truth within the bound
            unresolved.append((m, start, got, tr))
            continue
        if not tr["correction"] <= max(tr["refs"].values()) / 64:
            bad.append("%s list of %d: the truth's last Newton correction %.3g" % (label, m, tr["correction"]))
        for k, v in tr["refs"].items():
            refs[k] = max(refs[k], v)
        rows.append((m, ic.trial_deviation(got, tr)))
    bound = ic.MARGIN * max(refs.values())
    for m, d in rows:
        print("%s list of %d: deviation %.3e bound %.3e" % (label, m, d, bound))
        if not d <= bound:
            bad.append("%s list of %d: the step deviates %.3e, above the bound %.3e" % (label, m, d, bound))
    for m, start, got, tr in unresolved:
        stays = got[4:].tobytes() == start[4:].tobytes() and np.abs(got[:4] - start[:4]).max() <= 2.0 ** -52
        d = ic.trial_deviation(got, tr)
        print("%s list of %d (unresolved): %s, %.3e from the truth" % (label, m, "the start" if stays else "moved", d))
        if not (stays or d <= bound):
            bad.append("%s list of %d: neither the start nor the truth (%.3e off, bound %.3e)" % (label, m, d, bound))
    rec = _record("one trial", "%s %s" % (fam, model), {k: dict(step=v) for k, v in refs.items()}, dict(step=bound),
                  dict(step=max(d for _, d in rows)))
    return bad, rec


@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_one_trial_is_the_longdouble_step(oracle, fam, model):
    bad, _ = run_trial(_eng(), oracle, fam, model)
    assert not bad, "\n".join(bad)


def run_refined(eng, O, fam, model):
    h = ic.select_handle(fam, model, counts=ic.TRIAL_COUNTS)
    label = "refined %s %s" % (fam, model)
    (_, _, _, cam, tag), _ = _initialize(eng, h, sweeps=0, score_cap_px=ic.SCORE_CAP_PX, min_tag_observations=1)
    oth = tag if fam == "cam" else cam
    bad, worst = [], 0.0
    for p, lst in enumerate(h.lists(fam)):
        got = _own(fam, (cam, tag))[p]
        opt, _ = ic.host_optimum(O, fam, h, p, got, lst, oth)
        c_got, c_opt = ic.ld_cost(fam, h, p, got, lst, oth), ic.ld_cost(fam, h, p, opt, lst, oth)
        above = float((c_got - c_opt) / c_opt)
        worst = max(worst, above)
        print("%s list of %d: cost %.9g, %.3g above the host optimum's" % (label, len(lst), float(c_got), above))
        if not above <= ic.COST_GAP:
            bad.append("%s list of %d: the cost lies %.3g above the host optimum's" % (label, len(lst), above))
    return bad, dict(entry="refined", case="%s %s" % (fam, model), cost_above_host_optimum=worst)


@pytest.mark.parametrize("model", fm.MODELS)
@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_default_refinement_reaches_the_host_optimum(oracle, fam, model):
    bad, _ = run_refined(_eng(), oracle, fam, model)
    assert not bad, "\n".join(bad)


# ---- 4. growth, sweeps, report ---------------------------------------------------------------------------------------------

GROWTH_OPTIONS = dict(sweeps=0, refine_iterations=0, score_cap_px=ic.SCORE_CAP_PX)
GROWTH_CASES = ("corridor", "cross links", "cut", "constant camera", "degenerate end")


def run_growth(eng, model, variant):
    h = ic.growth_handle(model, variant)
    label = "growth %s %s" % (model, variant)
    first, second = _initialize(eng, h, **GROWTH_OPTIONS)
    bad = []
    if not _same_call(first, second):
        bad.append("%s: a second call changed a bit" % label)
    qt2, rms2 = _device_quads(eng, h)
    res = ic.restate(h, qt2, rms2, ic.SCORE_CAP_PX, 2, known=first[3:5])
    check_reach(h, res, first, label, bad)
    want_c, want_t, want_rounds = ic.reach(h)
    if not (np.array_equal(first[1], want_c) and np.array_equal(first[2], want_t) and first[0]["rounds"] == want_rounds):
        bad.append("%s: the reach differs from the breadth-first search's" % label)
    refs, bound, dev = check_picks(h, res, first[3], first[4], label, bad)
    rec = _record("growth", "%s %s" % (model, variant), {k: dict(pose=v) for k, v in refs.items()}, dict(pose=bound), dict(pose=dev),
                  rounds=first[0]["rounds"], cams_reached=first[0]["cams_reached"], tags_reached=first[0]["tags_reached"])
    _check(bad, label, rec)
    return bad, rec


@pytest.mark.parametrize("variant", GROWTH_CASES)
@pytest.mark.parametrize("model", fm.MODELS)
def test_growth_is_the_restated_recipe(model, variant):
    bad, _ = run_growth(_eng(), model, variant)
    assert not bad, "\n".join(bad[:20])


def run_sweep(eng, model, cap_px):
    """sweeps = 1 on the corridor with cross links against the restated sweep formed from the device's own states before
    (a fresh handle with sweeps = 0) and after: the cameras against the tags before, then the tags against the cameras after."""
    h = ic.growth_handle(model, "cross links")
    label = "sweep %s cap %g" % (model, cap_px)
    options = dict(GROWTH_OPTIONS, score_cap_px=cap_px)
    (rep0, c0, t0, cam0, tag0), _ = _initialize(eng, h, **options)
    first, second = _initialize(eng, h, **dict(options, sweeps=1))
    rep1, c1, t1, cam1, tag1 = first
    bad = []
    if not _same_call(first, second):
        bad.append("%s: a second call changed a bit" % label)
    if not (np.array_equal(c0, c1) and np.array_equal(t0, t1) and rep0["rounds"] == rep1["rounds"]):
        bad.append("%s: the sweep changed the reach" % label)
    qt2, rms2 = _device_quads(eng, h)
    refs, rows, moved, stayed, tied = {"A numpy": 0.0, "B device scheme": 0.0}, [], 0, 0, 0

    def stands(p, before, after):
        """Only k_init_refine's normalisation has touched the pose."""
        return after[p, 4:].tobytes() == before[p, 4:].tobytes() and np.abs(after[p, :4] - before[p, :4]).max() <= 2.0 ** -52

    for fam, ok, before, after, oth, oth_ok in (("cam", c1, cam0, cam1, tag0, t0), ("tag", t1, tag0, tag1, cam1, c1)):
        const = h.const(fam)
        for p, lst in enumerate(h.lists(fam)):
            if const[p] or not ok[p]:
                if after[p].tobytes() != before[p].tobytes():
                    bad.append("%s: %s %d is constant or unreached and lost its bytes" % (label, fam, p))
                continue
            pk = ic.select_pose(fam, h, p, lst, oth_ok, oth, qt2, rms2, cap_px, 1 if fam == "cam" else 2, current=before[p])
            if cap_px == ic.TIE_CAP_PX or (pk.winner < 0 and len(pk.tied) == 1):
                # the pose as it stands wins, decisively or by the tie rule
                stayed += 1
                if pk.winner >= 0 or not stands(p, before, after):
                    bad.append("%s: %s %d stands (margin %.3g) and moved by %.3g" % (label, fam, p, pk.margin,
                                                                                  np.abs(after[p] - before[p]).max()))
                continue
            for k, v in ic.pick_references(fam, pk).items() if pk.winner >= 0 else ():
                refs[k] = max(refs[k], v)
            rows.append((fam, p, pk, before, after, ic.pose_deviation(np.tile(after[p], (len(pk.poses) - 1, 1)), pk.poses[:-1])))
    bound, dev = ic.MARGIN * max(refs.values()), 0.0
    for fam, p, pk, before, after, d in rows:
        near = set(np.flatnonzero(d <= bound).tolist())
        if len(pk.tied) == 1:
            moved += 1
            dev = max(dev, float(d[pk.best]))
            if near != {pk.best}:
                bad.append("%s %s %d: the device's pose is candidate(s) %s, the restated sweep picks %d" % (label, fam, p,
                                                                                                         pk.index[sorted(near)].tolist(), pk.winner))
            continue
        # Without refinement the poses are chains of quad poses: a candidate through a counterpart that was itself placed
        # through this pose is this pose again, to rounding, and its score the same to rounding.  Which of them wins is
        # then decided below float64's resolution; the device's pose must be one of those that tie.
        tied += 1
        members = set(pk.tied.tolist())
        if not ((near & members) or (len(pk.poses) - 1 in members and stands(p, before, after))):
            bad.append("%s %s %d: the device's pose is candidate(s) %s, none of those that tie (%s)" % (label, fam, p,
                       pk.index[sorted(near)].tolist(), pk.index[pk.tied].tolist()))
    print("%s: %d poses replaced decisively (deviation %.3e, bound %.3e), %d stand, %d among candidates that tie to rounding"
          % (label, moved, dev, bound, stayed, tied))
    rec = _record("sweep", "%s cap %g" % (model, cap_px), {k: dict(pose=v) for k, v in refs.items()}, dict(pose=bound), dict(pose=dev),
                  replaced=moved, stand=stayed, tied=tied)
    return bad, rec


@pytest.mark.parametrize("cap_px", [ic.SCORE_CAP_PX, ic.TIE_CAP_PX], ids=["scored", "exact ties"])
@pytest.mark.parametrize("model", fm.MODELS)
def test_sweep_is_the_restated_sweep(model, cap_px):
    bad, rec = run_sweep(_eng(), model, cap_px)
    assert not bad, "\n".join(bad[:20])
    if cap_px == ic.TIE_CAP_PX:
        assert rec["replaced"] == 0, "a pose was replaced although every score ties"
    else:
        assert rec["replaced"] > 0, "no pose of the scene is replaced decisively"


REPORT_CASES = {"all": (False, False), "masked": (True, False), "unreached": (False, True), "masked, unreached": (True, True)}


def run_report(eng, O, model, variant):
    h = ic.report_handle(model, *REPORT_CASES[variant])
    label = "report %s %s" % (model, variant)
    first, second = _initialize(eng, h, score_cap_px=ic.SCORE_CAP_PX, min_tag_observations=1)
    report, cam_ok, tag_ok, cam, tag = first
    bad = []
    if not _same_call(first, second):
        bad.append("%s: a second call changed a bit" % label)
    want_c, want_t, _ = ic.reach(h, 1)
    if not (np.array_equal(cam_ok, want_c) and np.array_equal(tag_ok, want_t)):
        bad.append("%s: the reach differs from the breadth-first search's" % label)
    truth, corners = ic.report_truth(h, cam, tag, cam_ok, tag_ok)
    refs = {"A oracle": dict(avg=ic.relative(ic.report_a(O, h, cam, tag, cam_ok, tag_ok), truth)),
            "B device scheme": dict(avg=ic.relative(ic.report_b(h, cam, tag, cam_ok, tag_ok), truth))}
    rec = _record("report", "%s %s" % (model, variant), refs, dict(avg=ic.MARGIN * max(r["avg"] for r in refs.values())),
                  dict(avg=ic.relative(report["avg_reprojection_px"], truth)), corners=corners,
                  avg_reprojection_px=report["avg_reprojection_px"], rounding_floor=ic.report_floor(h, cam, tag, cam_ok, tag_ok))
    _check(bad, label, rec)
    return bad, rec


@pytest.mark.parametrize("variant", list(REPORT_CASES))
@pytest.mark.parametrize("model", fm.MODELS)
def test_report_is_the_longdouble_mean(oracle, model, variant):
    bad, _ = run_report(_eng(), oracle, model, variant)
    assert not bad, "\n".join(bad)
