"""GPU tests of the prediction with correlated map tags (vmm_ba_predict_localization_joint, k_predict_joint, and the layers
above it: engine.predict_localization(tag_cov_joint=, visible_in=), BundleAdjuster.tag_joint_covariance, the
reconstructor's members, uncertainty.py --joint, coverage.py --correlated, localization.py --uncertainty).

Yardstick: tests/predict_joint_cases.py -- the longdouble truth, the two float64 references and the bound of
tests/finished_map_cases.py (8 x the larger deviation of the references from the truth, entry by entry in the metric
|got - truth| / sqrt(truth_ii truth_jj)); it never calls the code under test, and tests/test_predict_joint_cpu.py shows that
no flag of its cases rests on rounding.  The run_* functions return (failures, records); tools/predict_joint_accuracy.py
writes the records down.

Bytes.  A selected set and the sub-map of its tags give the same bytes when the sums run in the same order.  They do for
up to two selected tags (a wave's total is then the sum of at most two lanes' values, which does not depend on the lanes)
and trivially for all tags; with three or more the tags of the sub-map sit in other lanes, the butterfly adds them in
another order, and the two results are compared within the bound instead.
"""
import os
import shutil

import numpy as np
import pytest

import cov_cases as cc
import finished_map_cases as fm
import predict_cases as pc
import predict_joint_cases as pj

pytestmark = pytest.mark.gpu

KINDS = ("real", "rigid")


def _make_scene():
    from visual_marker_mapping_amd.synthetic import make_scene
    return make_scene(1)


def bundle_adjusted():
    """make_scene(1) bundle-adjusted: (scene, tag_joint_covariance, pose_covariances' tag blocks)."""
    from visual_marker_mapping_amd import engine as eng
    s = _make_scene()
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px, device=0)
    ba.solve(eng.default_options(robustify=1))
    joint = ba.tag_joint_covariance()
    tag_cov = ba.pose_covariances()[1]
    ba.close()
    return s, joint, tag_cov


@pytest.fixture(scope="module")
def adjusted():
    """Shared, never changed."""
    return bundle_adjusted()


def joint_of(kind, n_tags, adjusted):
    if kind == "rigid":
        return pj.rigid(pc.lanes(n_tags, 1, relief=fm.PREDICT_RELIEF)["tag_qt"], pj.world_covariance())
    s, joint, _ = adjusted
    return pj.tiled(joint, n_tags, [t for t in range(len(s.tag_gt)) if t != s.fixed_tag])


def _call(eng, case, poses=None, joint=None, **kw):
    c = case.case
    cam = c["cam_qt"] if poses is None else c["cam_qt"][poses]
    return eng.predict_localization(c["intr"], c["dist"], c["tag_qt"], c["tag_wh"], cam, c["size"], want_visible=True,
                                    tag_cov_joint=case.joint if joint is None else joint, sigma_px=case.sigma_px, **kw)


def _bits(out, p=None):
    cov_px, cov_map, res, vis = out
    if p is None:
        return cov_px.tobytes(), cov_map.tobytes(), res, vis.tobytes()
    return cov_px[p].tobytes(), cov_map[p].tobytes(), res[p], vis[p].tobytes()


def _check_pose(ev, p, out, k, n_sel, label, bad, worst, min_tags=1):
    """Pose p of the evaluation against entry k of the device's output `out`."""
    from visual_marker_mapping_amd import _lib
    cov_px, cov_map, res, _ = out
    want = _lib.PRED_NO_VISIBLE_TAG if n_sel == 0 else _lib.PRED_TOO_FEW_TAGS if n_sel < min_tags else _lib.PRED_OK
    if res[k]["n_visible"] != n_sel or res[k]["status"] != want:
        bad.append("%s pose %d: status %d, n_visible %d of %d" % (label, p, res[k]["status"], res[k]["n_visible"], n_sel))
        return
    if want != _lib.PRED_OK:
        if cov_px[k].any() or cov_map[k].any() or res[k]["sigma_pos_m"] != 0 or res[k]["sigma_rot_rad"] != 0:
            bad.append("%s pose %d: status %d, but a result that is not exactly zero" % (label, p, want))
        return
    got = dict(cov=cov_px[k], prop=cov_map[k], sigma_pos=res[k]["sigma_pos_m"], sigma_rot=res[k]["sigma_rot_rad"])
    b_p, dev = ev.check(p, got, label)
    bad += b_p
    for q, v in dev.items():
        worst[q] = max(worst.get(q, 0.0), v)
    if not (fm.symmetric_bits(cov_px[k]) and fm.symmetric_bits(cov_map[k])):
        bad.append("%s pose %d: a covariance is not symmetric in its bits" % (label, p))
    if not (np.isfinite(cov_px[k]).all() and np.isfinite(cov_map[k]).all()):
        bad.append("%s pose %d: a non-finite entry" % (label, p))


def _record(label, ev, worst, out, **extra):
    for q in ev.bound:
        out("%s %-9s deviation %.3e  bound %.3e  ratio %.3f" % (label, q, worst.get(q, 0.0), ev.bound[q], worst.get(q, 0.0) / ev.bound[q]))
    return dict(dict(entry="predict_joint", case=label, items=len(ev.items), reference_deviation=ev.reference_deviation,
                     bound=ev.bound, deviation={q: worst.get(q, 0.0) for q in ev.bound},
                     ratio_to_bound={q: worst.get(q, 0.0) / ev.bound[q] for q in ev.bound}), **extra)


# ---- 1. accuracy --------------------------------------------------------------------------------------------------------------

def run_accuracy(eng, O, n_tags, kind, adjusted, out=print):
    bad, recs = [], []
    case = pj.JointCase(n_tags, pj.JOINT_POSES, joint_of(kind, n_tags, adjusted))
    label = "joint %s %d tags x %d poses" % (kind, n_tags, pj.JOINT_POSES)
    want, on_rounding = case.host_visible()
    if on_rounding:
        bad.append("%s: a visibility flag rests on rounding" % label)
    res = _call(eng, case)
    if not (res[3] == want).all():
        return bad + ["%s: %d visible bytes differ from the header's rules" % (label, int((res[3] != want).sum()))], recs
    ev = case.evaluate(O, res[3])
    worst = {}
    for p in range(pj.JOINT_POSES):
        _check_pose(ev, p, res, p, int(want[p].sum()), label, bad, worst)
    if ev.items:
        recs.append(_record(label, ev, worst, out, observations=int(want.sum())))
    return bad, recs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_tags", pj.JOINT_TAGS)
def test_accuracy(oracle, adjusted, n_tags, kind):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_accuracy(eng, oracle, n_tags, kind, adjusted)
    assert not bad, "\n".join(bad)


# ---- 2. against the existing path ----------------------------------------------------------------------------------------------

def run_against_independent(eng, O, n_tags, out=print):
    """A block-diagonal joint covariance against predict_localization(tag_cov = its diagonal)."""
    bad = []
    old_case = fm.PredictCase(n_tags, pj.JOINT_POSES, True)
    case = pj.JointCase(n_tags, pj.JOINT_POSES, pj.block_diagonal(old_case.tag_cov))
    c, label = case.case, "joint block-diagonal %d tags" % n_tags
    new = _call(eng, case)
    old = eng.predict_localization(c["intr"], c["dist"], c["tag_qt"], c["tag_wh"], c["cam_qt"], c["size"], tag_cov=old_case.tag_cov,
                                   want_visible=True, sigma_px=case.sigma_px)
    if new[3].tobytes() != old[3].tobytes() or [(r["status"], r["n_visible"]) for r in new[2]] != \
            [(r["status"], r["n_visible"]) for r in old[2]]:
        bad.append("%s: visible, status or n_visible differ from the existing entry's" % label)
    # sweep 1 of k_predict_joint is k_predict's pass over H statement by statement, butterfly included: the same bits
    if new[0].tobytes() != old[0].tobytes():
        bad.append("%s: cov_px differs in its bits from the existing entry's" % label)
    ev_new, ev_old = case.evaluate(O, new[3]), old_case.evaluate(O, old[3])
    worst = {}
    gap = 0.0
    for p in ev_new.items:
        _check_pose(ev_new, p, new, p, int(new[3][p].sum()), label, bad, worst)
        truth = ev_new.truth[p]["prop"]
        d = np.sqrt(np.diag(truth))
        dev = float((np.abs(new[1][p].astype(fm.LD) - old[1][p].astype(fm.LD)) / (d[:, None] * d[None, :])).max())
        gap = max(gap, dev)
        if not dev <= ev_new.bound["prop"] + ev_old.bound["prop"]:
            bad.append("%s pose %d: cov_map %.3e from the existing entry's, above %.3e + %.3e" % (label, p, dev, ev_new.bound["prop"],
                                                                                                  ev_old.bound["prop"]))
    out("%s: cov_map differs from the existing entry's by %.3e, bounds %.3e + %.3e" % (label, gap, ev_new.bound["prop"],
                                                                                         ev_old.bound["prop"]))
    return bad, [_record(label, ev_new, worst, out, gap_to_independent_entry=gap, bound_of_independent_entry=ev_old.bound["prop"])]


@pytest.mark.parametrize("n_tags", [2, 65, 129])
def test_block_diagonal_agrees_with_the_existing_entry(oracle, n_tags):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_against_independent(eng, oracle, n_tags)
    assert not bad, "\n".join(bad)


# ---- 3. the loop edges, through visible_in ---------------------------------------------------------------------------------------

EDGE_SETS = (("none", []), ("one", [5]), ("last", [128]), ("across rounds", [63, 64]), ("one per round", [0, 64, 128]),
             ("all", list(range(129))))
SAME_ORDER = ("one", "last", "across rounds", "all")   # see the module's docstring


def run_edges(eng, O, adjusted, kind="real", out=print):
    from visual_marker_mapping_amd import _lib
    bad, recs = [], []
    n_tags, poses = 129, [0, 1]     # both see every tag of the sets by the rules, so H stays well conditioned
    case = pj.JointCase(n_tags, pj.JOINT_POSES, joint_of(kind, n_tags, adjusted))
    for name, tags in EDGE_SETS:
        label = "joint edges %s, %s" % (kind, name)
        sel = np.zeros((len(poses), n_tags), bool)
        sel[:, tags] = True
        res = _call(eng, case, poses, visible_in=sel)
        if not (res[3] == sel).all():
            bad.append("%s: `visible` does not repeat visible_in" % label)
            continue
        full = np.zeros((pj.JOINT_POSES, n_tags), bool)
        full[poses] = sel
        ev = case.evaluate(O, full)
        worst = {}
        for k, p in enumerate(poses):
            _check_pose(ev, p, res, k, len(tags), label, bad, worst)
        if not tags:
            continue
        recs.append(_record(label, ev, worst, out))
        # the sub-map of the selected tags alone, all of them selected
        sub = case.sub_case(tags)
        alone = _call(eng, sub, poses, visible_in=np.ones((len(poses), len(tags)), bool))
        if name in SAME_ORDER:
            if (alone[0].tobytes(), alone[1].tobytes(), alone[2]) != (res[0].tobytes(), res[1].tobytes(), res[2]):
                bad.append("%s: the sub-map of the selected tags gives other bytes" % label)
        else:
            worst_sub = {}
            for k, p in enumerate(poses):
                _check_pose(ev, p, alone, k, len(tags), label + " (sub-map)", bad, worst_sub)
    # min_tags above the count
    sel = np.zeros((len(poses), n_tags), bool)
    sel[:, [63, 64]] = True
    res = _call(eng, case, poses, visible_in=sel, min_tags=3)
    ev = case.evaluate(O, np.zeros((pj.JOINT_POSES, n_tags), bool))
    for k, p in enumerate(poses):
        _check_pose(ev, p, res, k, 2, "joint edges, min_tags 3", bad, {}, min_tags=3)
    if [r["status"] for r in res[2]] != [_lib.PRED_TOO_FEW_TAGS] * len(poses):
        bad.append("joint edges, min_tags 3: not TOO_FEW_TAGS")
    return bad, recs


def test_loop_edges_through_visible_in(oracle, adjusted):
    from visual_marker_mapping_amd import engine as eng
    bad, _ = run_edges(eng, oracle, adjusted)
    assert not bad, "\n".join(bad)


# ---- 4. behind the camera --------------------------------------------------------------------------------------------------------

def test_a_selected_tag_behind_the_camera_is_singular():
    from visual_marker_mapping_amd import _lib, engine as eng
    case = pj.JointCase(65, 2, pj.dense_spd(65))
    c = case.case
    behind = c["tag_qt"].copy()
    behind[7, 4:] = pc.camera_centre(c["cam_qt"][0]) - 2.0 * np.array([0.0, 0.0, 1.0])   # two metres behind pose 0, which looks along +z
    moved = pj.JointCase.__new__(pj.JointCase)
    moved.__dict__.update(case.__dict__)
    moved.case = dict(c, tag_qt=behind)
    sel = np.zeros((2, 65), bool)
    sel[:, [3, 7, 40]] = True
    cov_px, cov_map, res, vis = _call(eng, moved, visible_in=sel)
    assert (vis == sel).all()
    for p in range(2):
        assert res[p]["status"] == _lib.PRED_SINGULAR and res[p]["n_visible"] == 3, res[p]
        assert not cov_px[p].any() and not cov_map[p].any() and res[p]["sigma_pos_m"] == 0.0 and res[p]["sigma_rot_rad"] == 0.0
    # without that tag the same poses are fine
    sel[:, 7] = False
    assert [r["status"] for r in _call(eng, moved, visible_in=sel)[2]] == [_lib.PRED_OK] * 2


# ---- 5. the upper block triangle, 6. independence ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch(adjusted):
    from visual_marker_mapping_amd import engine as eng
    case = pj.JointCase(129, pj.JOINT_POSES, joint_of("real", 129, adjusted))
    return case, _call(eng, case)


def test_the_upper_block_triangle_is_never_read(batch):
    from visual_marker_mapping_amd import engine as eng
    case, first = batch
    s, t = np.triu_indices(129, 1)
    for fill in ("nan", "garbage"):
        joint = case.joint.copy()
        joint[s, t] = np.nan if fill == "nan" else 1e6 * (1 + joint[t, s])   # not transposed: anything but S_st^T
        assert _bits(_call(eng, case, joint=joint)) == _bits(first), fill


def test_a_pose_gives_the_same_bytes_alone_in_the_batch_shuffled_and_again(batch):
    from visual_marker_mapping_amd import engine as eng
    case, first = batch
    assert _bits(_call(eng, case)) == _bits(first)
    for p in range(pj.JOINT_POSES):
        assert _bits(_call(eng, case, [p]), 0) == _bits(first, p), p
    perm = np.random.default_rng(5).permutation(pj.JOINT_POSES)
    shuffled = _call(eng, case, list(perm))
    for k, p in enumerate(perm):
        assert _bits(shuffled, k) == _bits(first, p), p
    # and with a selection handed in: the rules' own flags give the rules' bytes
    given = _call(eng, case, visible_in=first[3])
    assert _bits(given) == _bits(first)


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------

def test_errors_come_before_any_device_call():
    """tests/test_predict_joint_cpu.py walks the list where no device exists; here the same calls on a machine that has one."""
    from visual_marker_mapping_amd import _lib, engine as eng
    case = pj.JointCase(2, 1, pj.dense_spd(2))
    bad = case.joint.copy()
    bad[1, 0, 2, 2] = np.nan
    with pytest.raises(_lib.VmmBaError) as ei:
        _call(eng, case, joint=bad)
    assert ei.value.status == _lib.ERR_ARGUMENT and "non-finite tag_cov_joint" in str(ei.value)
    with pytest.raises(_lib.VmmBaError) as ei:
        _call(eng, case, min_tags=0)
    assert ei.value.status == _lib.ERR_ARGUMENT
    c = case.case
    out = eng.predict_localization(c["intr"], c["dist"], c["tag_qt"], c["tag_wh"], np.zeros((0, 7)), c["size"], tag_cov_joint=case.joint)
    assert out[0].shape == (0, 6, 6) and out[2] == []


# ---- 8. the layers above ------------------------------------------------------------------------------------------------------------

def test_tag_joint_covariance_is_symmetric_and_holds_the_marginals(adjusted):
    s, joint, tag_cov = adjusted
    T = len(s.tag_gt)
    assert joint.shape == (T, T, 6, 6)
    dense = pj.dense_matrix(joint)
    assert dense.tobytes() == np.ascontiguousarray(dense.T).tobytes()
    assert joint[np.arange(T), np.arange(T)].tobytes() == tag_cov.tobytes()
    assert not joint[s.fixed_tag].any() and not joint[:, s.fixed_tag].any()
    free = [t for t in range(T) if t != s.fixed_tag]
    assert np.linalg.eigvalsh(pj.dense_matrix(joint[np.ix_(free, free)])).min() > 0
    # neighbouring tags far from the origin move together: cross blocks as large as the marginals
    a, b = slice(6 * free[0], 6 * free[0] + 3), slice(6 * free[1], 6 * free[1] + 3)
    corr = np.abs(dense[a, b]) / np.sqrt(np.outer(np.diag(dense)[a], np.diag(dense)[b]))
    assert corr.max() > 0.1


def test_command_lines_carry_the_joint_covariance(tmp_path):
    from visual_marker_mapping_amd import _lib, coverage, engine as eng, io as vio, localization, uncertainty
    from visual_marker_mapping_amd.synthetic import write_project
    s = _make_scene()
    proj = str(tmp_path / "proj")
    model, _ = write_project(s, proj)
    det = vio.readDetectionResult(os.path.join(proj, "marker_detections.json"))
    size = (model.horizontalResolution, model.verticalResolution)
    shutil.copy(os.path.join(proj, "ground_truth.json"), os.path.join(proj, "reconstruction.json"))
    plain, with_joint = os.path.join(proj, "u_plain.json"), os.path.join(proj, "u_joint.json")
    assert uncertainty.main(["--project_path", proj, "--output", plain]) == 0
    assert uncertainty.main(["--project_path", proj, "--output", with_joint, "--joint"]) == 0
    tree_plain, tree_joint = vio.read_json(plain), vio.read_json(with_joint)
    assert "tag_joint_covariance" not in tree_plain and {k: tree_joint[k] for k in tree_plain} == tree_plain
    ids, joint = uncertainty.read_tag_joint_covariance(with_joint)
    assert ids == list(range(len(s.tag_gt))) and uncertainty.read_tag_joint_covariance(plain) is None
    for k, t in enumerate(ids):
        entry = tree_joint["reconstructed_tags"][k]
        assert int(entry["id"]) == t and vio.matrixFromPropertyTree(entry["covariance"], 6, 6).tobytes() == joint[k, k].tobytes()
    # coverage.py: --correlated writes the joint call's matrices and the new key; without it nothing changes
    poses = os.path.join(proj, "ground_truth.json")
    base = ["--project_path", proj, "--poses", poses, "--covariances"]
    out_a, out_b, out_c = (os.path.join(proj, n) for n in ("cov_a.json", "cov_b.json", "cov_c.json"))
    assert coverage.main(base + ["--uncertainty", plain, "--output", out_a]) == 0
    assert coverage.main(base + ["--uncertainty", with_joint, "--output", out_b]) == 0
    assert coverage.main(base + ["--uncertainty", with_joint, "--correlated", "--output", out_c]) == 0
    assert open(out_a).read() == open(out_b).read() and "map_covariance" not in vio.read_json(out_a)
    tree = vio.read_json(out_c)
    assert tree["map_covariance"] == "joint"
    want = eng.predict_localization(s.intr, s.dist, s.tag_gt, s.tag_wh, s.cam_gt, size, tag_cov_joint=joint, want_visible=True)
    for p, e in enumerate(tree["poses"]):
        assert vio.matrixFromPropertyTree(e["covariance_map"], 6, 6).tobytes() == want[1][p].tobytes(), p
        assert float(e["sigma_pos_m"]) == want[2][p]["sigma_pos_m"] and e["status"] == _lib.PRED_STATUS_NAMES[want[2][p]["status"]]
    assert any(r["status"] == _lib.PRED_OK for r in want[2])
    with pytest.raises(RuntimeError) as ei:
        coverage.main(base + ["--uncertainty", plain, "--correlated", "--output", out_c])
    assert "uncertainty.py --joint" in str(ei.value)
    # localization.py: --uncertainty adds the three keys; without it the file is today's
    loc_a, loc_b = os.path.join(proj, "loc_a.json"), os.path.join(proj, "loc_b.json")
    assert localization.main(["--project_path", proj, "--output", loc_a]) == 0
    assert localization.main(["--project_path", proj, "--output", loc_b, "--uncertainty", with_joint]) == 0
    ta, tb = vio.read_json(loc_a)["reconstructed_cameras"], vio.read_json(loc_b)["reconstructed_cameras"]
    new_keys = {"map_covariance", "sigma_pos_m", "sigma_rot_rad"}
    assert all(not (new_keys & set(e)) for e in ta)
    assert [{k: v for k, v in e.items() if k not in new_keys} for e in tb] == ta and all(new_keys <= set(e) for e in tb)
    # ... and they are the joint call's, with visible_in built from the localisation's own inlier flags
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    tags, _, _ = vio.parseReconstructions(os.path.join(proj, "reconstruction.json"))
    rec = TagReconstructor(det)
    rec.setCameraModel(model)
    rec.setReconstructedTags(tags)
    img_ids, order, tag_qt, tag_wh, img_start, obs_tag, obs_px = rec._pack_against_map(det, None)
    cam, _, inl, lres = eng.localize(s.intr, s.dist, tag_qt, tag_wh, img_start, obs_tag, obs_px)
    assert all(r["status"] == _lib.LOC_OK for r in lres)
    _, cov_map, res, sel = eng.localization_map_covariance(s.intr, s.dist, tag_qt, tag_wh, cam, img_start, obs_tag, inl, joint, size)
    assert sel.sum() == len({(int(i), int(t)) for i, t, f in zip(np.repeat(np.arange(len(cam)), np.diff(img_start)), obs_tag, inl) if f})
    for n, e in enumerate(tb):
        assert int(e["id"]) == img_ids[n]
        assert vio.matrixFromPropertyTree(e["map_covariance"], 6, 6).tobytes() == cov_map[n].tobytes(), n
        assert float(e["sigma_pos_m"]) == res[n]["sigma_pos_m"] and float(e["sigma_rot_rad"]) == res[n]["sigma_rot_rad"]
    assert any(m.any() for m in cov_map)
