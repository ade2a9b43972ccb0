"""GPU tests of the localisation against a finished map (vmm_ba_localize, engine.localize, the batch member of
TagReconstructor and the command line).

Yardstick throughout: tests/yardstick.py -- block_normal over image_rows and image_optimum, numpy around
oracle/oracle.py; they never call the code under test.  Tolerances: 1e-9 on exact data, 1e-6 per pose between two
optima, covariances to 1e-6 x max|ref| as the existing covariance tests.  Scenes come from
synthetic.make_scene, the map is tag_gt.
tests/test_finished_map_accuracy.py supersedes in strength the covariance comparison of
test_covariance_matches_the_inverse_normal_matrix (1e-6 x max|ref|) and the finiteness checks of cost and rms_px: there
every entry, the cost and rms_px are held to float64 accuracy at the device's own state, at 1 to 513 observations.
"""
import json
import os
import shutil

import numpy as np
import pytest

import yardstick as ys

pytestmark = pytest.mark.gpu

INLIER_PX = 8.0   # the default of vmm_ba_localize_options


# ---- helpers --------------------------------------------------------------------------------------------------------

def _csr(s):
    """The scene's observations grouped by image: (img_start, obs_tag, obs_px, order)."""
    start, order = s.by_image()
    return start, s.obs_tag[order].astype(np.int32), s.obs_px[order].copy(), order


def _localize(eng, s, start, tag, px, **kw):
    return eng.localize(s.intr, s.dist, s.tag_gt, s.tag_wh, start, tag, px, **kw)


def _check_against_host(O, s, start, tag, px, cam, inl, res, images, robust, label, a=1.0):
    """Device pose vs the host optimum (Huber width a) over the same inlier set, started at cam_gt: 1e-6 per pose."""
    worst = (0.0, 0.0)
    for i in images:
        b, e = int(start[i]), int(start[i + 1])
        keep = inl[b:e]
        ref, cost, grad = ys.image_optimum(O, s, s.cam_gt[i], tag[b:e][keep], px[b:e][keep], robust, a)
        gq, gt = ys.pose_gap(cam[i], ref)
        print("%s image %d: obs %d inliers %d trials %d |dq| %.3g |dt| %.3g cost device %.12g host %.12g "
              "scaled gradient %.3g" % (label, i, e - b, int(keep.sum()), res[i]["trials"], gq, gt, res[i]["cost"], cost,
                                        grad))
        worst = (max(worst[0], gq), max(worst[1], gt))
        assert gq <= 1e-6 and gt <= 1e-6, (label, i, gq, gt)
    return worst


def _assert_clean(cam, cov, res):
    assert np.isfinite(cam).all() and np.isfinite(cov).all()
    for r in res:
        assert np.isfinite(r["rms_px"]) and np.isfinite(r["cost"]), r


EXACT = {
    "config1_20x10": (1, dict()),
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "closeup_60x80": (2, dict(n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)),
    "distortion_30x40": (5, dict(n_cams=30, n_tags=40, visibility=0.5)),
}


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_data_recovers_the_ground_truth(name):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = EXACT[name]
    s = make_scene(cfg, noise_px=0.0, outlier_frac=0.0, **kw)
    start, tag, px, _ = _csr(s)
    cam, cov, inl, res = _localize(eng, s, start, tag, px)
    gq, gt = ys.pose_gap(cam, s.cam_gt)
    print("%s: %d images %d observations, max |dq| %.3g |dt| %.3g, max rms %.3g px, trials %d..%d"
          % (name, len(cam), len(tag), gq, gt, max(r["rms_px"] for r in res), min(r["trials"] for r in res),
             max(r["trials"] for r in res)))
    assert [r["status"] for r in res] == [_lib.LOC_OK] * len(cam)
    assert inl.all()
    assert [r["n_inlier_obs"] for r in res] == [r["n_obs"] for r in res] == list(np.diff(start))
    _assert_clean(cam, cov, res)
    assert gq <= 1e-9 and gt <= 1e-9, (gq, gt)


# ---- 2. noisy data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robustify", [0, 1])
@pytest.mark.parametrize("name", ["config1_20x10", "100x60_vis0.30"])
def test_noisy_data_reaches_the_host_optimum(oracle, name, robustify):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = EXACT[name]
    s = make_scene(cfg, **kw)   # the generator's default noise
    assert s.noise_px > 0
    start, tag, px, _ = _csr(s)
    cam, cov, inl, res = _localize(eng, s, start, tag, px, robustify=robustify)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * len(cam)
    _assert_clean(cam, cov, res)
    worst = _check_against_host(oracle, s, start, tag, px, cam, inl, res, range(len(cam)), bool(robustify),
                                "%s robustify=%d" % (name, robustify))
    print("%s robustify=%d: worst |dq| %.3g |dt| %.3g, trials %s" % (name, robustify, worst[0], worst[1],
                                                                   sorted({r["trials"] for r in res})))


# ---- 3. outliers ---------------------------------------------------------------------------------------------------

def test_outliers_are_found_and_do_not_move_the_pose(oracle):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=100, n_tags=60, visibility=0.30, noise_px=0.3, outlier_frac=0.0)
    start, tag, px, _ = _csr(s)
    rng = np.random.default_rng(7)
    label = np.ones(len(tag), bool)
    shifted = 0
    for i in range(len(s.cam_gt)):
        b, e = int(start[i]), int(start[i + 1])
        n_bad = min(int(0.3 * (e - b)), e - b - 3)
        if n_bad <= 0:
            continue
        for d in rng.choice(e - b, n_bad, replace=False):
            ang = rng.uniform(0, 2 * np.pi)
            amp = rng.uniform(10.0, 40.0) * INLIER_PX
            px[b + d] += np.tile([amp * np.cos(ang), amp * np.sin(ang)], 4)
            label[b + d] = False
            shifted += 1
    # the condition on the input: at most 30 % per image, at least 3 clean tags wherever something was replaced,
    # every replaced corner at least 10 x inlier_px away from where it was
    clean_px = s.obs_px[np.argsort(s.obs_cam, kind="stable")]
    for i in range(len(s.cam_gt)):
        b, e = int(start[i]), int(start[i + 1])
        bad = int((~label[b:e]).sum())
        assert bad <= 0.3 * (e - b)
        assert bad == 0 or int(label[b:e].sum()) >= 3
    moved = np.linalg.norm((px - clean_px).reshape(-1, 4, 2), axis=2)
    assert shifted > 50 and (moved[~label] >= 10 * INLIER_PX - 1e-9).all() and (moved[label] == 0).all()
    cam, cov, inl, res = _localize(eng, s, start, tag, px)
    print("outliers: %d of %d observations replaced; flags differing from the labels: %d"
          % (shifted, len(tag), int((inl != label).sum())))
    assert [r["status"] for r in res] == [_lib.LOC_OK if start[i + 1] > start[i] else _lib.LOC_NO_OBSERVATIONS
                                          for i in range(len(cam))]
    assert (inl == label).all()
    _assert_clean(cam, cov, res)
    images = [i for i in range(len(cam)) if start[i + 1] > start[i]]
    _check_against_host(oracle, s, start, tag, px, cam, label, res, images, True, "outliers")


# ---- 4. covariance -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robustify", [0, 1])
@pytest.mark.parametrize("name", ["config1_20x10", "closeup_60x80"])
def test_covariance_matches_the_inverse_normal_matrix(oracle, name, robustify):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = EXACT[name]
    s = make_scene(cfg, **kw)
    start, tag, px, order = _csr(s)
    cam, cov, inl, res = _localize(eng, s, start, tag, px, robustify=robustify)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * len(cam)
    worst = 0.0
    for i in range(len(cam)):
        b, e = int(start[i]), int(start[i + 1])
        keep = inl[b:e]
        _, A, _ = ys.block_normal(oracle, ys.image_rows(oracle, s.intr, s.dist, cam[i], s.tag_gt, s.tag_wh, tag[b:e][keep],
                                                        px[b:e][keep]), bool(robustify))
        ref = np.linalg.inv(A)
        err = np.abs(cov[i] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= 1e-6, (i, err)
        assert (cov[i] == cov[i].T).all()
        assert np.linalg.eigvalsh(cov[i]).min() > 0
    print("%s robustify=%d: worst covariance error %.3g of max|ref|" % (name, robustify, worst))
    if name == "config1_20x10":
        # independent check: the bundle adjuster's own camera blocks at the same state (all observations are inliers)
        assert inl.all()
        with eng.BundleAdjuster(s.intr, s.dist, cam, s.tag_gt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                s.obs_px) as ba:
            V = ba.eval_blocks(robustify=bool(robustify), want_W=False)["V"]
        for i in range(len(cam)):
            ref = np.linalg.inv(V[i])
            assert np.abs(cov[i] - ref).max() <= 1e-6 * np.abs(ref).max(), i


# ---- 5. determinism ------------------------------------------------------------------------------------------------

def _bits(cam, cov, inl, res):
    return (cam.tobytes(), cov.tobytes(), inl.tobytes(), json.dumps(res, sort_keys=True))


def test_results_are_bit_identical_alone_in_a_batch_and_permuted():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=100, n_tags=60, visibility=0.30)
    start, tag, px, _ = _csr(s)
    first = _localize(eng, s, start, tag, px)
    again = _localize(eng, s, start, tag, px)
    assert _bits(*first) == _bits(*again)
    cam, cov, inl, res = first
    for i in (0, 17, 42, 63, 99):
        b, e = int(start[i]), int(start[i + 1])
        c1, v1, f1, r1 = _localize(eng, s, np.array([0, e - b], np.int64), tag[b:e], px[b:e])
        assert c1.tobytes() == cam[i:i + 1].tobytes() and v1.tobytes() == cov[i:i + 1].tobytes()
        assert f1.tobytes() == inl[b:e].tobytes() and r1[0] == res[i]
    perm = np.random.default_rng(3).permutation(len(cam))
    p_start = np.zeros_like(start)
    p_start[1:] = np.cumsum(np.diff(start)[perm])
    idx = np.concatenate([np.arange(start[i], start[i + 1]) for i in perm]).astype(np.int64)
    c2, v2, f2, r2 = _localize(eng, s, p_start, tag[idx], px[idx])
    assert c2.tobytes() == cam[perm].tobytes() and v2.tobytes() == cov[perm].tobytes()
    assert f2.tobytes() == inl[idx].tobytes() and r2 == [res[i] for i in perm]


# ---- 6. edges ------------------------------------------------------------------------------------------------------

def test_edges_empty_image_single_tag_and_collapsed_observation():
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, noise_px=0.0, outlier_frac=0.0)
    start, tag, px, _ = _csr(s)
    n0, n1, n2 = (int(start[i + 1] - start[i]) for i in range(3))
    assert n1 >= 1 and n2 >= 3
    # image 0: no observations; image 1: one tag; image 2: its first observation collapsed to a point
    b1, b2, e2 = int(start[1]), int(start[2]), int(start[3])
    e_tag = np.concatenate([tag[b1:b1 + 1], tag[b2:e2]])
    e_px = np.concatenate([px[b1:b1 + 1], px[b2:e2]])
    e_px[1] = np.tile(e_px[1, :2], 4)
    e_start = np.array([0, 0, 1, 1 + (e2 - b2)], np.int64)
    cam, cov, inl, res = _localize(eng, s, e_start, e_tag, e_px)
    _assert_clean(cam, cov, res)
    assert res[0]["status"] == _lib.LOC_NO_OBSERVATIONS and res[0]["n_obs"] == 0
    assert (cam[0] == [1, 0, 0, 0, 0, 0, 0]).all() and (cov[0] == 0).all()
    assert res[1]["status"] == _lib.LOC_OK and res[1]["n_inlier_obs"] == 1 and inl[0]
    assert np.linalg.eigvalsh(cov[1]).min() > 0
    gq, gt = ys.pose_gap(cam[1], s.cam_gt[1])
    print("single tag: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert gq <= 1e-9 and gt <= 1e-9
    assert res[2]["status"] == _lib.LOC_OK
    assert not inl[1] and inl[2:].all() and res[2]["n_inlier_obs"] == e2 - b2 - 1
    gq, gt = ys.pose_gap(cam[2], s.cam_gt[2])
    print("collapsed observation: |dq| %.3g |dt| %.3g" % (gq, gt))
    assert gq <= 1e-9 and gt <= 1e-9
    assert np.linalg.eigvalsh(cov[2]).min() > 0
    # an image whose only observation is collapsed has no candidate
    cam, cov, inl, res = _localize(eng, s, np.array([0, 1], np.int64), e_tag[1:2], e_px[1:2])
    _assert_clean(cam, cov, res)
    assert res[0]["status"] == _lib.LOC_NO_CANDIDATE and not inl.any()
    assert (cam[0] == [1, 0, 0, 0, 0, 0, 0]).all() and (cov[0] == 0).all()
    # min_inlier_tags above what the image has: the best-effort pose, flagged
    cam, cov, inl, res = _localize(eng, s, np.array([0, 1], np.int64), tag[b1:b1 + 1], px[b1:b1 + 1], min_inlier_tags=2)
    _assert_clean(cam, cov, res)
    assert res[0]["status"] == _lib.LOC_TOO_FEW_INLIERS and (cov[0] == 0).all()


# ---- 7. size -------------------------------------------------------------------------------------------------------

SIZES = {
    "500x200_full": (2, dict()),
    "closeup_2000": (2, dict(n_cams=2000, n_tags=1000, neighbors_min=6, neighbors_max=10)),
    "6x300_full_unstaged": (2, dict(n_cams=6, n_tags=300)),   # more observations per image than k_localize stages in LDS
}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_large_batches_complete_and_agree_with_the_host(oracle, name):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SIZES[name]
    s = make_scene(cfg, **kw)
    start, tag, px, _ = _csr(s)
    if name == "500x200_full":
        assert len(tag) == 100000
    if name == "6x300_full_unstaged":
        assert np.diff(start).min() > 256
    cam, cov, inl, res = _localize(eng, s, start, tag, px)
    _assert_clean(cam, cov, res)
    with_obs = np.flatnonzero(np.diff(start) > 0)
    assert all(res[i]["status"] == _lib.LOC_OK for i in with_obs)
    sample = with_obs[np.linspace(0, len(with_obs) - 1, min(10, len(with_obs))).astype(int)]
    worst = _check_against_host(oracle, s, start, tag, px, cam, inl, res, sample, True, name)
    print("%s: %d images %d observations, sampled worst |dq| %.3g |dt| %.3g" % (name, len(cam), len(tag), *worst))
    if name == "6x300_full_unstaged":
        again = _localize(eng, s, start, tag, px)
        assert _bits(cam, cov, inl, res) == _bits(*again)


# ---- 8. surface ----------------------------------------------------------------------------------------------------

def test_command_line_and_reconstructor_member_match_the_engine(tmp_path, capsys):
    from visual_marker_mapping_amd import _lib, engine as eng, io as vio, localization
    from visual_marker_mapping_amd.synthetic import make_scene, write_project
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    s = make_scene(1)
    proj = str(tmp_path / "proj")
    model, det = write_project(s, proj)
    shutil.copy(os.path.join(proj, "ground_truth.json"), os.path.join(proj, "reconstruction.json"))
    assert localization.main(["--project_path", proj]) == 0
    out = vio.read_json(os.path.join(proj, "localization.json"))
    start, tag, px, _ = _csr(s)
    cam, cov, inl, res = _localize(eng, s, start, tag, px)
    cams = out["reconstructed_cameras"]
    assert [int(c["id"]) for c in cams] == list(range(len(cam)))
    for i, c in enumerate(cams):
        pose = np.array([float(v) for v in c["rotation"]] + [float(v) for v in c["translation"]])
        assert pose.tobytes() == cam[i].tobytes(), i
        assert c["status"] == "ok" and int(c["num_inlier_observations"]) == res[i]["n_inlier_obs"]
        assert float(c["rms_px"]) == res[i]["rms_px"]
        m = c["covariance"]
        assert (int(m["rows"]), int(m["cols"])) == (6, 6)
        assert np.array([float(v) for v in m["coefficents"]]).tobytes() == cov[i].tobytes()
    # a second detection file and output through the options
    other = str(tmp_path / "other.json")
    assert localization.main(["--project_path", proj, "--detections", os.path.join(proj, "marker_detections.json"),
                              "--output", other]) == 0
    assert open(other).read() == open(os.path.join(proj, "localization.json")).read()
    # the batch member of the reconstructor
    tags, _, model2 = vio.parseReconstructions(os.path.join(proj, "reconstruction.json"))
    rec = TagReconstructor(det)
    rec.setCameraModel(model2)
    rec.setReconstructedTags(tags)
    got = rec.computeRelativeCameraPosesFromImgs()
    assert sorted(got) == list(range(len(cam)))
    for i in range(len(cam)):
        assert np.concatenate([got[i].q, got[i].t]).tobytes() == cam[i].tobytes()
        assert rec.lastLocalizationReport[i]["status"] == _lib.LOC_OK
    # observations of tags that are not reconstructed are dropped
    del tags[max(tags)]
    rec.setReconstructedTags(tags)
    some = rec.computeRelativeCameraPosesFromImgs(imageIds=[3, 5])
    assert sorted(some) == [3, 5]
    assert all(det.tagObservations[k].tagId in tags for r in rec.lastLocalizationReport.values()
               for k in r["observations"])
