"""GPU tests of the tag location from known cameras (vmm_ba_locate_tags, engine.locate_tags, TagReconstructor.locateTags
and checkMap, the map_check command line).

Yardstick throughout: tests/tag_cases.py -- block_normal over tag_rows, tag_optimum, tag_propagated and
map_check_statistic, numpy around oracle/oracle.py; they never call the code under test.  Tolerances are the project's:
1e-9 per pose (yardstick.pose_gap) on exact data, 1e-6 per pose between two optima, covariances to 1e-6 x max|ref|.
Scenes come from synthetic.make_scene, the cameras are cam_gt unless said otherwise, the observations are grouped by tag
with a stable sort.
tests/test_finished_map_accuracy.py supersedes in strength the 1e-6 x max|ref| comparisons of tag_cov and tag_cov_cams
and the finiteness checks of cost and rms_px: there every entry is held to float64 accuracy at the device's own state, for
tags seen by 1 to 513 cameras.
"""
import contextlib
import io
import json
import os
import types

import numpy as np
import pytest

import tag_cases as tc
import yardstick as ys

pytestmark = pytest.mark.gpu

INLIER_PX = 8.0   # the default of vmm_ba_localize_options


# ---- helpers --------------------------------------------------------------------------------------------------------

def _csr(s):
    """The scene's observations grouped by tag: (tag_start, obs_cam, obs_px, order); cameras ascend within a tag."""
    start, order = tc.by_tag(s)
    cam = s.obs_cam[order].astype(np.int32)
    for t in range(len(start) - 1):
        assert (np.diff(cam[start[t]:start[t + 1]]) > 0).all()
    return start, cam, s.obs_px[order].copy(), order


def _locate(eng, s, start, cam, px, **kw):
    return eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh, start, cam, px, **kw)


def _check_against_host(O, s, start, cam, px, tag, keep_all, res, tags, robust, label, a=1.0):
    """Device pose vs the host optimum (Huber width a) over the inlier set keep_all, started at tag_gt: 1e-6 per pose."""
    worst = (0.0, 0.0)
    for t in tags:
        b, e = int(start[t]), int(start[t + 1])
        keep = keep_all[b:e]
        ref, cost, grad = tc.tag_optimum(O, s.intr, s.dist, s.tag_gt[t], s.cam_gt, s.tag_wh[t], cam[b:e][keep], px[b:e][keep],
                                         robust, a)
        gq, gt = ys.pose_gap(tag[t], ref)
        print("%s tag %d: obs %d inliers %d trials %d |dq| %.3g |dt| %.3g cost device %.12g host %.12g scaled gradient %.3g"
              % (label, t, e - b, int(keep.sum()), res[t]["trials"], gq, gt, res[t]["cost"], cost, grad))
        worst = (max(worst[0], gq), max(worst[1], gt))
        assert gq <= 1e-6 and gt <= 1e-6, (label, t, gq, gt)
    return worst


def _assert_clean(tag, cov, cams, res):
    assert np.isfinite(tag).all() and np.isfinite(cov).all() and np.isfinite(cams).all()
    for r in res:
        assert np.isfinite(r["rms_px"]) and np.isfinite(r["cost"]), r


SCENES = {
    "config1_20x10": (1, dict()),
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "distortion_30x40": (5, dict(n_cams=30, n_tags=40, visibility=0.5)),
}


def _scene(name, **kw):
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, base = SCENES[name]
    return make_scene(cfg, **dict(base, **kw))


def _statuses(_lib, start):
    return [_lib.LOC_OK if start[t + 1] > start[t] else _lib.LOC_NO_OBSERVATIONS for t in range(len(start) - 1)]


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["config1_20x10", "distortion_30x40"])
def test_exact_data_recovers_the_ground_truth(name):
    from visual_marker_mapping_amd import _lib, engine as eng
    s = _scene(name, noise_px=0.0, outlier_frac=0.0)
    start, cam, px, _ = _csr(s)
    assert np.diff(start).min() >= 1
    tag, cov, cams, inl, res = _locate(eng, s, start, cam, px)
    gq, gt = ys.pose_gap(tag, s.tag_gt)
    print("%s: %d tags %d observations, max |dq| %.3g |dt| %.3g, max rms %.3g px, trials %d..%d"
          % (name, len(tag), len(cam), gq, gt, max(r["rms_px"] for r in res), min(r["trials"] for r in res),
             max(r["trials"] for r in res)))
    assert [r["status"] for r in res] == [_lib.LOC_OK] * len(tag)
    assert inl.all()
    assert [r["n_inlier_obs"] for r in res] == [r["n_obs"] for r in res] == list(np.diff(start))
    _assert_clean(tag, cov, cams, res)
    assert gq <= 1e-9 and gt <= 1e-9, (gq, gt)


# ---- 2. noisy data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robustify", [0, 1])
@pytest.mark.parametrize("name", ["config1_20x10", "100x60_vis0.30"])
def test_noisy_data_reaches_the_host_optimum(oracle, name, robustify):
    from visual_marker_mapping_amd import _lib, engine as eng
    s = _scene(name)   # the generator's default noise
    assert s.noise_px > 0
    start, cam, px, _ = _csr(s)
    tag, cov, cams, inl, res = _locate(eng, s, start, cam, px, robustify=robustify)
    assert [r["status"] for r in res] == _statuses(_lib, start)
    _assert_clean(tag, cov, cams, res)
    seen = [t for t in range(len(tag)) if start[t + 1] > start[t]]
    worst = _check_against_host(oracle, s, start, cam, px, tag, inl, res, seen, bool(robustify),
                                "%s robustify=%d" % (name, robustify))
    print("%s robustify=%d: worst |dq| %.3g |dt| %.3g, trials %s" % (name, robustify, worst[0], worst[1],
                                                                   sorted({r["trials"] for r in res})))


# ---- 3. outliers ---------------------------------------------------------------------------------------------------

def test_outliers_are_found_and_do_not_move_the_pose(oracle):
    from visual_marker_mapping_amd import _lib, engine as eng
    s = _scene("100x60_vis0.30", noise_px=0.3, outlier_frac=0.0)
    start, cam, px, order = _csr(s)
    rng = np.random.default_rng(7)
    label = np.ones(len(cam), bool)
    shifted = 0
    for t in range(len(s.tag_gt)):
        b, e = int(start[t]), int(start[t + 1])
        n_bad = min(int(0.3 * (e - b)), e - b - 3)
        if n_bad <= 0:
            continue
        for d in rng.choice(e - b, n_bad, replace=False):
            ang = rng.uniform(0, 2 * np.pi)
            amp = rng.uniform(10.0, 40.0) * INLIER_PX
            px[b + d] += np.tile([amp * np.cos(ang), amp * np.sin(ang)], 4)
            label[b + d] = False
            shifted += 1
    # the condition on the input: at most 30 % per tag, at least 3 clean observations wherever something was displaced,
    # every displaced corner between 10 and 40 x inlier_px away from where it was
    clean_px = s.obs_px[order]
    for t in range(len(s.tag_gt)):
        b, e = int(start[t]), int(start[t + 1])
        bad = int((~label[b:e]).sum())
        assert bad <= 0.3 * (e - b)
        assert bad == 0 or int(label[b:e].sum()) >= 3
    moved = np.linalg.norm((px - clean_px).reshape(-1, 4, 2), axis=2)
    assert shifted > 50 and (moved[~label] >= 10 * INLIER_PX - 1e-9).all() and (moved[~label] <= 40 * INLIER_PX + 1e-9).all()
    assert (moved[label] == 0).all()
    tag, cov, cams, inl, res = _locate(eng, s, start, cam, px)
    print("outliers: %d of %d observations displaced; flags differing from the labels: %d"
          % (shifted, len(cam), int((inl != label).sum())))
    assert [r["status"] for r in res] == _statuses(_lib, start)
    assert (inl == label).all()
    _assert_clean(tag, cov, cams, res)
    seen = [t for t in range(len(tag)) if start[t + 1] > start[t]]
    _check_against_host(oracle, s, start, cam, px, tag, label, res, seen, True, "outliers")


# ---- 4. covariances ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robustify", [0, 1])
def test_covariances_match_the_host(oracle, robustify):
    from visual_marker_mapping_amd import _lib, engine as eng
    s = _scene("config1_20x10")
    start, cam, px, _ = _csr(s)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(len(s.cam_gt), 6, 6)) * 1e-3
    cam_cov = A @ A.transpose(0, 2, 1) + 1e-9 * np.eye(6)   # random symmetric positive definite
    tag, cov, cams, inl, res = _locate(eng, s, start, cam, px, robustify=robustify, cam_cov=cam_cov)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * len(tag)
    worst = [0.0, 0.0]
    for t in range(len(tag)):
        b, e = int(start[t]), int(start[t + 1])
        keep = inl[b:e]
        args = (oracle, s.intr, s.dist, tag[t], s.cam_gt)
        ref = np.linalg.inv(tc.tag_normal(*args, s.tag_wh[t], cam[b:e][keep], px[b:e][keep], bool(robustify)))
        ref_cams = tc.tag_propagated(*args, cam_cov, s.tag_wh[t], cam[b:e][keep], px[b:e][keep], bool(robustify))
        err = np.abs(cov[t] - ref).max() / np.abs(ref).max()
        err_cams = np.abs(cams[t] - ref_cams).max() / np.abs(ref_cams).max()
        worst = [max(worst[0], err), max(worst[1], err_cams)]
        assert err <= 1e-6 and err_cams <= 1e-6, (t, err, err_cams)
        # both are symmetric to the last bit: the library stores one triangle twice
        assert (cov[t] == cov[t].T).all() and (cams[t] == cams[t].T).all()
        assert np.linalg.eigvalsh(cov[t]).min() > 0 and np.linalg.eigvalsh(cams[t]).min() > 0
    print("robustify=%d: worst error of tag_cov %.3g, of tag_cov_cams %.3g of max|ref|" % (robustify, *worst))
    # without cam_cov the propagated part is exactly zero, and nothing else changes
    tag0, cov0, cams0, inl0, res0 = _locate(eng, s, start, cam, px, robustify=robustify)
    assert (cams0 == 0).all()
    assert tag0.tobytes() == tag.tobytes() and cov0.tobytes() == cov.tobytes() and inl0.tobytes() == inl.tobytes() and res0 == res
    # independent check: the bundle adjuster's own tag blocks at the same state (all observations are inliers)
    assert inl.all()
    with eng.BundleAdjuster(s.intr, s.dist, s.cam_gt, tag, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        U = ba.eval_blocks(robustify=bool(robustify), want_W=False)["U"]
    for t in range(len(tag)):
        if t == s.fixed_tag:   # the fixed tag has no block
            continue
        ref = np.linalg.inv(U[t])
        assert np.abs(cov[t] - ref).max() <= 1e-6 * np.abs(ref).max(), t


# ---- 5. determinism ------------------------------------------------------------------------------------------------

def _bits(tag, cov, cams, inl, res):
    return (tag.tobytes(), cov.tobytes(), cams.tobytes(), inl.tobytes(), json.dumps(res, sort_keys=True))


def test_results_are_bit_identical_alone_in_a_batch_and_permuted():
    from visual_marker_mapping_amd import engine as eng
    s = _scene("100x60_vis0.30")
    start, cam, px, _ = _csr(s)
    A = np.random.default_rng(9).normal(size=(len(s.cam_gt), 6, 6)) * 1e-3
    cam_cov = A @ A.transpose(0, 2, 1)
    first = _locate(eng, s, start, cam, px, cam_cov=cam_cov)
    again = _locate(eng, s, start, cam, px, cam_cov=cam_cov)
    assert _bits(*first) == _bits(*again)
    tag, cov, cams, inl, res = first
    for t in (0, 17, 31, 42, 59):
        b, e = int(start[t]), int(start[t + 1])
        t1, v1, c1, f1, r1 = eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh[t:t + 1], np.array([0, e - b], np.int64),
                                             cam[b:e], px[b:e], cam_cov=cam_cov)
        assert t1.tobytes() == tag[t:t + 1].tobytes() and v1.tobytes() == cov[t:t + 1].tobytes()
        assert c1.tobytes() == cams[t:t + 1].tobytes() and f1.tobytes() == inl[b:e].tobytes() and r1[0] == res[t]
    perm = np.random.default_rng(3).permutation(len(tag))
    p_start = np.zeros_like(start)
    p_start[1:] = np.cumsum(np.diff(start)[perm])
    idx = np.concatenate([np.arange(start[t], start[t + 1]) for t in perm]).astype(np.int64)
    t2, v2, c2, f2, r2 = eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh[perm], p_start, cam[idx], px[idx], cam_cov=cam_cov)
    assert t2.tobytes() == tag[perm].tobytes() and v2.tobytes() == cov[perm].tobytes() and c2.tobytes() == cams[perm].tobytes()
    assert f2.tobytes() == inl[idx].tobytes() and r2 == [res[t] for t in perm]


# ---- 6. edges ------------------------------------------------------------------------------------------------------

def test_edges_empty_tag_single_observation_and_collapsed_observation():
    from visual_marker_mapping_amd import _lib, engine as eng
    s = _scene("config1_20x10", noise_px=0.0, outlier_frac=0.0)
    start, cam, px, _ = _csr(s)
    assert start[2] - start[1] >= 1 and start[3] - start[2] >= 3
    # tag 0: no observation; tag 1: one observation; tag 2: three observations, the first collapsed to a point
    b1, b2 = int(start[1]), int(start[2])
    e_cam = np.concatenate([cam[b1:b1 + 1], cam[b2:b2 + 3]])
    e_px = np.concatenate([px[b1:b1 + 1], px[b2:b2 + 3]])
    e_px[1] = np.tile(e_px[1, :2], 4)
    e_start = np.array([0, 0, 1, 4], np.int64)
    tag, cov, cams, inl, res = eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh[:3], e_start, e_cam, e_px)
    _assert_clean(tag, cov, cams, res)
    assert res[0]["status"] == _lib.LOC_NO_OBSERVATIONS and res[0]["n_obs"] == 0
    assert (tag[0] == [1, 0, 0, 0, 0, 0, 0]).all() and (cov[0] == 0).all() and (cams[0] == 0).all()
    assert res[1]["status"] == _lib.LOC_OK and res[1]["n_inlier_obs"] == 1 and inl[0]
    assert np.linalg.eigvalsh(cov[1]).min() > 0
    gq, gt = ys.pose_gap(tag[1], s.tag_gt[1])
    print("single observation: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert gq <= 1e-9 and gt <= 1e-9
    assert res[2]["status"] == _lib.LOC_OK
    assert not inl[1] and inl[2:].all() and res[2]["n_inlier_obs"] == 2
    gq, gt = ys.pose_gap(tag[2], s.tag_gt[2])
    print("collapsed observation: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert gq <= 1e-9 and gt <= 1e-9
    assert np.linalg.eigvalsh(cov[2]).min() > 0
    # a tag whose only observation is collapsed has no candidate
    one = np.array([0, 1], np.int64)
    tag, cov, cams, inl, res = eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh[2:3], one, e_cam[1:2], e_px[1:2])
    _assert_clean(tag, cov, cams, res)
    assert res[0]["status"] == _lib.LOC_NO_CANDIDATE and not inl.any()
    assert (tag[0] == [1, 0, 0, 0, 0, 0, 0]).all() and (cov[0] == 0).all() and (cams[0] == 0).all()
    # min_inlier_tags above what the tag has: the best-effort pose, flagged
    tag, cov, cams, inl, res = eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh[1:2], one, cam[b1:b1 + 1], px[b1:b1 + 1],
                                               cam_cov=np.tile(np.eye(6) * 1e-6, (len(s.cam_gt), 1, 1)), min_inlier_tags=2)
    _assert_clean(tag, cov, cams, res)
    assert res[0]["status"] == _lib.LOC_TOO_FEW_INLIERS and (cov[0] == 0).all() and (cams[0] == 0).all()
    assert not (tag[0] == [1, 0, 0, 0, 0, 0, 0]).all()


# ---- 7. both staging forms -----------------------------------------------------------------------------------------

def test_long_tags_read_global_memory_and_mix_with_staged_ones(oracle):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=260, n_tags=4)
    start, cam, px, _ = _csr(s)
    # the library exports no accessor for the stage capacity (256 observations)
    assert np.diff(start).min() > 256
    full = _locate(eng, s, start, cam, px)
    tag, cov, cams, inl, res = full
    assert [r["status"] for r in res] == [_lib.LOC_OK] * 4
    _assert_clean(tag, cov, cams, res)
    _check_against_host(oracle, s, start, cam, px, tag, inl, res, range(4), True, "260x4 unstaged")
    assert _bits(*full) == _bits(*_locate(eng, s, start, cam, px))
    # a mixed batch: every tag truncated to its first 200 observations (staged) next to the full one (not staged)
    parts, wh = [], []
    for t in range(4):
        b, e = int(start[t]), int(start[t + 1])
        parts += [(b, b + 200), (b, e)]
        wh += [s.tag_wh[t], s.tag_wh[t]]
    m_start = np.zeros(9, np.int64)
    m_start[1:] = np.cumsum([e - b for b, e in parts])
    idx = np.concatenate([np.arange(b, e) for b, e in parts])
    mixed = eng.locate_tags(s.intr, s.dist, s.cam_gt, np.array(wh), m_start, cam[idx], px[idx])
    for k, (b, e) in enumerate(parts):
        alone = eng.locate_tags(s.intr, s.dist, s.cam_gt, np.array(wh[k:k + 1]), np.array([0, e - b], np.int64), cam[b:e], px[b:e])
        mb, me = int(m_start[k]), int(m_start[k + 1])
        assert alone[0].tobytes() == mixed[0][k:k + 1].tobytes() and alone[1].tobytes() == mixed[1][k:k + 1].tobytes(), k
        assert alone[2].tobytes() == mixed[2][k:k + 1].tobytes() and alone[3].tobytes() == mixed[3][mb:me].tobytes(), k
        assert alone[4][0] == mixed[4][k], k
        if k % 2:   # the full tag in the mixed batch is the full tag of the first call
            assert mixed[0][k].tobytes() == tag[k // 2].tobytes() and mixed[4][k] == res[k // 2]
        else:
            assert mixed[4][k]["status"] == _lib.LOC_OK and mixed[4][k]["n_obs"] == 200


# ---- 8. the map check, end to end ------------------------------------------------------------------------------------

MOVED = {4: (0.02, 0, 0, 0, 0, 0), 11: (0, 0, 0.005, 0, 0, 0), 17: (0, 0, 0, 0.02, 0, 0), 26: (0.003, -0.002, 0.001, 0, 0, 0.005)}
SIGMA_PX, CHI2 = 0.3, 22.458


def _host_check(O, s, det, map_qt, rec):
    """The map check's statistic from the host yardstick over the device's inlier sets of its last round: every image
    at its host optimum against the map (the observations the device's localisation used and kept), its covariance
    inv(A) there; every tag at its host optimum from the map pose under those cameras; tag_propagated; d2."""
    loc, tags = rec.lastLocalizationReport, rec.lastTagLocationReport
    scene = types.SimpleNamespace(intr=s.intr, dist=s.dist, tag_gt=map_qt, tag_wh=s.tag_wh)
    n = len(s.cam_gt)
    cam_qt, cam_cov = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (n, 1)), np.zeros((n, 6, 6))
    ok = [i for i in sorted(loc) if loc[i]["status"] == 0]
    for i in ok:
        keep = [k for k, f in zip(loc[i]["observations"], loc[i]["inliers"]) if f]
        ts, pxs = [det.tagObservations[k].tagId for k in keep], [np.asarray(det.tagObservations[k].corners).reshape(8) for k in keep]
        cam_qt[i], _, _ = ys.image_optimum(O, scene, s.cam_gt[i], ts, pxs, True)
        cam_cov[i] = np.linalg.inv(ys.block_normal(O, ys.image_rows(O, s.intr, s.dist, cam_qt[i], map_qt, s.tag_wh, ts, pxs), True)[1])
    out = {}
    for t, r in tags.items():
        keep = [k for k, f in zip(r["observations"], r["inliers"]) if f]
        cs, pxs = [det.tagObservations[k].imageId for k in keep], [np.asarray(det.tagObservations[k].corners).reshape(8) for k in keep]
        q, _, _ = tc.tag_optimum(O, s.intr, s.dist, map_qt[t], cam_qt, s.tag_wh[t], cs, pxs, True)
        cov = np.linalg.inv(tc.tag_normal(O, s.intr, s.dist, q, cam_qt, s.tag_wh[t], cs, pxs, True))
        cams = tc.tag_propagated(O, s.intr, s.dist, q, cam_qt, cam_cov, s.tag_wh[t], cs, pxs, True)
        delta, Sigma, d2 = tc.map_check_statistic(O, q, map_qt[t], cov, cams, SIGMA_PX)
        out[t] = dict(pose=q, Sigma=Sigma, d2=d2)
    return out


def test_map_check_finds_the_moved_tags_and_the_command_line_writes_the_same(oracle, tmp_path):
    from visual_marker_mapping_amd import io as vio, map_check
    from visual_marker_mapping_amd.synthetic import make_scene, write_project
    from visual_marker_mapping_amd.tag_reconstructor import ReconstructedTag, TagReconstructor
    O = oracle
    # if another detail of the yardstick ever breaks the precondition below, change this scene's seed, not the band
    s = make_scene(1, n_cams=40, n_tags=30, visibility=0.5, noise_px=0.3, outlier_frac=0.0)
    map_qt = s.tag_gt.copy()
    for j, d in MOVED.items():
        map_qt[j] = O.pose_plus(s.tag_gt[j], np.array(d, np.float64))
    proj = str(tmp_path / "proj")
    model, _ = write_project(s, proj)
    vio.exportReconstructions(os.path.join(proj, "reconstruction.json"),
                              {t: ReconstructedTag(t, "apriltag_36h11", map_qt[t, :4], map_qt[t, 4:], s.tag_wh[t, 0], s.tag_wh[t, 1])
                               for t in range(len(map_qt))}, {}, model)
    # the same inputs the command line reads
    tags, _, model2 = vio.parseReconstructions(os.path.join(proj, "reconstruction.json"))
    det = vio.readDetectionResult(os.path.join(proj, "marker_detections.json"))
    assert np.array([np.concatenate([tags[t].q, tags[t].t]) for t in sorted(tags)]).tobytes() == map_qt.tobytes()
    rec = TagReconstructor(det)
    rec.setCameraModel(model2)
    rec.setReconstructedTags(tags)
    report = rec.checkMap(sigma_px=SIGMA_PX)
    assert report is rec.lastMapCheckReport and report["chi2_threshold"] == CHI2
    host = _host_check(O, s, det, map_qt, rec)
    assert sorted(host) == sorted(report["tags"]) == list(range(30)), report["skipped"]
    # the precondition: no host value so close to the threshold that the 1e-6 pose tolerance (against sigmas of about
    # 5e-5 m) could put the device on the other side
    for t in sorted(host):
        assert not (CHI2 / 1.2 <= host[t]["d2"] <= 1.2 * CHI2), (t, host[t]["d2"])
    gaps = {False: 0.0, True: 0.0}
    for t in sorted(host):
        dev = report["tags"][t]
        gap = abs(dev["mahalanobis2"] - host[t]["d2"]) / host[t]["d2"]
        gaps[t in MOVED] = max(gaps[t in MOVED], gap)
        print("tag %2d: d2 device %.6g host %.6g (relative gap %.3g) corner displacement %.3g m moved %s"
              % (t, dev["mahalanobis2"], host[t]["d2"], gap, dev["max_corner_displacement"], dev["moved"]))
    print("largest relative gap of d2 between host and device: unmoved tags %.3g, moved tags %.3g" % (gaps[False], gaps[True]))
    assert report["moved"] == sorted(MOVED)
    assert sorted(t for t in host if host[t]["d2"] > CHI2) == sorted(MOVED)
    assert report["rounds"] == 2
    for j in sorted(MOVED):
        dev = report["tags"][j]
        gq, gt = ys.pose_gap(dev["pose"], host[j]["pose"])
        assert gq <= 1e-6 and gt <= 1e-6, (j, gq, gt)
        _, _, d2_true = tc.map_check_statistic(O, dev["pose"], s.tag_gt[j], dev["covariance"], np.zeros((6, 6)), 1.0)
        print("moved tag %d: |dq| %.3g |dt| %.3g to the host optimum; %.3g sigma from its true pose" % (j, gq, gt, np.sqrt(d2_true)))
        assert d2_true <= 25.0, (j, d2_true)
    # the command line on the written project: the same numbers, bit for bit
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        assert map_check.main(["--project_path", proj, "--sigma_px", str(SIGMA_PX)]) == 0
    printed = said.getvalue()
    assert [int(line.split()[1]) for line in printed.splitlines() if line.startswith("tag ")] == sorted(MOVED)
    out = vio.read_json(os.path.join(proj, "map_check.json"))
    assert int(out["rounds"]) == 2 and [int(t["id"]) for t in out["tags"]] == list(range(30))
    for t in out["tags"]:
        dev = report["tags"][int(t["id"])]
        pose = np.array([float(v) for v in t["rotation"]] + [float(v) for v in t["translation"]])
        assert pose.tobytes() == dev["pose"].tobytes()
        assert vio.matrixFromPropertyTree(t["covariance"], 6, 6).tobytes() == dev["covariance"].tobytes()
        assert np.array([float(v) for v in t["delta"]]).tobytes() == dev["delta"].tobytes()
        assert float(t["mahalanobis2"]) == dev["mahalanobis2"]
        assert float(t["max_corner_displacement"]) == dev["max_corner_displacement"]
        assert (t["moved"] == "true") == dev["moved"] and int(t["num_inlier_views"]) == dev["n_inlier_obs"]
    assert [(int(i["id"]), i["status"]) for i in out["images"]] == [(i, "ok") for i in range(40)]
