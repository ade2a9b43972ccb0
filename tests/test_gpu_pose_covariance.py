"""GPU tests of vmm_ba_covariance_blocks: any 6x6 marginal or cross block of the pose covariance.

Yardstick: the numpy inverse of the dense H over the free poses, H assembled from the CPU oracle's per-observation
residuals and Jacobians (yardstick.pose_blocks / free_system).  Tolerances: a diagonal block 1e-6 of
its largest entry (the project's figure for the same quantity in test_gpu_solve.py and test_gpu_constant_poses.py), a
cross block 1e-6 * sqrt(max|Cov_aa| * max|Cov_bb|); two factorisation paths of one matrix 1e-9 (test_gpu_solve.py).
"""
import itertools
import json
import os

import numpy as np
import pytest

from yardstick import const_sets, free_system, pose_blocks

pytestmark = pytest.mark.gpu


def _handle(eng, s, cam, tag, fixed_tag=0, **kw):
    return eng.BundleAdjuster(s.intr, s.dist, cam, tag, s.tag_wh, fixed_tag, s.obs_cam, s.obs_tag, s.obs_px, **kw)


class _Reference:
    """inv(H) over the free poses; block(a, b) in the pose index space of the entry (cameras, then tags), zeros for a
    pair that names a pose outside the free set."""

    def __init__(self, O, s, cam, tag, robust, cam_const, tag_const, obs_mask=None):
        if obs_mask is not None:
            import copy
            s = copy.copy(s)
            s.obs_cam, s.obs_tag, s.obs_px = s.obs_cam[obs_mask], s.obs_tag[obs_mask], s.obs_px[obs_mask]
        blk = pose_blocks(O, s, cam, tag, robust, cam_const=cam_const, tag_const=tag_const)
        H, _, fc, ft = free_system(s, blk, cam_const, tag_const)
        assert np.all(np.linalg.eigvalsh(H) > 0)
        self.order = len(H)
        self.inv = np.linalg.inv(H)
        self.pos = {int(c): 6 * k for k, c in enumerate(fc)}
        self.pos.update({len(cam) + int(t): 6 * (len(fc) + k) for k, t in enumerate(ft)})

    def block(self, a, b):
        if a not in self.pos or b not in self.pos:
            return np.zeros((6, 6))
        return self.inv[self.pos[a]:self.pos[a] + 6, self.pos[b]:self.pos[b] + 6]

    def check(self, pairs, cov, label):
        """Every block against the reference at the tolerances of the module docstring; prints the worst figures."""
        worst_d = worst_x = 0.0
        for (a, b), got in zip(np.asarray(pairs).tolist(), cov):
            ref = self.block(a, b)
            if a not in self.pos or b not in self.pos:
                assert not got.any(), (label, a, b)
                continue
            scale = np.sqrt(np.abs(self.block(a, a)).max() * np.abs(self.block(b, b)).max())
            assert scale > 0
            err = np.abs(got - ref).max() / scale
            if a == b:
                worst_d = max(worst_d, err)
            else:
                worst_x = max(worst_x, err)
            assert err <= 1e-6, (label, a, b, err)
        print("%s: H of order %d, %d blocks; worst |gpu - numpy| / scale: marginals %.3g, cross blocks %.3g"
              % (label, self.order, len(cov), worst_d, worst_x))


def _all_pairs(n):
    up = [(a, b) for a in range(n) for b in range(a, n)]
    return np.array(up + [(b, a) for a, b in up if a != b], np.int32)


def _marginal_pairs(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)


# ---- 1. - 3. all pairs, both eliminations; subset and bits; the existing entry ------------------------------------------

@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("elim", ["cams", "tags"])
def test_all_pairs_match_numpy_and_the_bits_do_not_depend_on_the_request(oracle, elim, robust):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5 if robust else 1, n_cams=30, n_tags=14, visibility=0.7)
    n_c, n_t = len(s.cam_init), len(s.tag_init)
    n = n_c + n_t
    pairs = _all_pairs(n)
    assert len(pairs) == 44 * 45 // 2 + 44 * 43 // 2
    sub = np.array([(2, 2), (2, n_c + 5), (n_c + 5, n_c + 9)], np.int32)
    mixed = np.concatenate([sub[::-1], sub, sub[1:2]])
    with _handle(eng, s, s.cam_init, s.tag_init, elimination=eng.ELIM_CAMERAS if elim == "cams" else eng.ELIM_TAGS) as ba:
        out = ba.solve(eng.default_options(robustify=int(robust)))
        assert out["termination_type"] == eng.CONVERGENCE
        cam, tag = ba.get_state()
        old_before = ba.tag_translation_covariance(robustify=robust)
        cov = ba.covariance_blocks(pairs, robustify=robust)
        cov2 = ba.covariance_blocks(pairs, robustify=robust)          # idempotent, leaves the state alone
        cam2, tag2 = ba.get_state()
        cov_sub = ba.covariance_blocks(sub, robustify=robust)
        cov_mixed = ba.covariance_blocks(mixed, robustify=robust)
        cam_cov, tag_cov = ba.pose_covariances(robustify=robust)
        old_after = ba.tag_translation_covariance(robustify=robust)
        again = ba.solve(eng.default_options(robustify=int(robust)))   # and the handle still solves
    assert cov.shape == (len(pairs), 6, 6)
    assert cov.tobytes() == cov2.tobytes() and cam.tobytes() == cam2.tobytes() and tag.tobytes() == tag2.tobytes()
    assert again["termination_type"] == eng.CONVERGENCE
    tag_const = np.zeros(n_t, np.uint8)
    tag_const[0] = 1
    ref = _Reference(oracle, s, cam, tag, robust, np.zeros(n_c, np.uint8), tag_const)
    ref.check(pairs, cov, "30x14 elim %s robust %d" % (elim, robust))
    at = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
    # the origin tag: zeros, the cross blocks included
    for p in range(n):
        assert not cov[at[(p, n_c)]].any() and not cov[at[(n_c, p)]].any()
    # Cov(b, a) = Cov(a, b)^T
    worst = 0.0
    for a, b in itertools.combinations(range(n), 2):
        if a == n_c or b == n_c:
            continue
        scale = np.sqrt(np.abs(cov[at[(a, a)]]).max() * np.abs(cov[at[(b, b)]]).max())
        gap = np.abs(cov[at[(b, a)]] - cov[at[(a, b)]].T).max() / scale
        worst = max(worst, gap)
        assert gap <= 1e-6, (a, b, gap)
    # marginals: symmetric in their bits, positive definite
    for p in range(n):
        m = cov[at[(p, p)]]
        assert m.tobytes() == np.ascontiguousarray(m.T).tobytes(), p
        if p != n_c:
            assert np.all(np.linalg.eigvalsh(m) > 0), p
    # the joint covariance of two poses is positive semi-definite
    low = 0.0
    for a, b in ((0, 17), (3, n_c + 4), (n_c + 2, n_c + 11)):
        J = eng.joint_covariance(cov[at[(a, a)]], cov[at[(a, b)]], cov[at[(b, b)]])
        w = np.linalg.eigvalsh(0.5 * (J + J.T))
        low = min(low, w[0] / w[-1])
        assert w[0] >= -1e-9 * w[-1], (a, b, w)
    print("   max |Cov(b,a) - Cov(a,b)^T| / scale %.3g; lowest joint eigenvalue / largest %.3g" % (worst, low))
    # 2. a block's bits do not depend on the rest of the request
    for k, (a, b) in enumerate(sub.tolist()):
        assert cov_sub[k].tobytes() == cov[at[(a, b)]].tobytes(), (a, b)
    for k, (a, b) in enumerate(mixed.tolist()):
        assert cov_mixed[k].tobytes() == cov[at[(a, b)]].tobytes(), (a, b)
    for p in range(n):
        assert (cam_cov[p] if p < n_c else tag_cov[p - n_c]).tobytes() == cov[at[(p, p)]].tobytes(), p
    # 3. the existing entry: same numbers to 1e-9, and its own bits are not disturbed
    assert old_before.tobytes() == old_after.tobytes()
    worst = 0.0
    for t in range(1, n_t):
        scale = np.abs(old_before[t]).max()
        assert scale > 0
        gap = np.abs(tag_cov[t][:3, :3] - old_before[t]).max() / scale
        worst = max(worst, gap)
        assert gap <= 1e-9, (t, gap)
    print("   translation blocks against tag_translation_covariance: worst gap %.3g of the block's largest entry" % worst)


# ---- 4. small reduced systems ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["20x10_cams", "12x24_auto"])
def test_small_reduced_systems(oracle, case):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    if case == "20x10_cams":
        s, mode = make_scene(1), eng.ELIM_CAMERAS      # a reduced system of one block: no update launch
    else:
        s, mode = make_scene(1, n_cams=12, n_tags=24, visibility=0.5), eng.ELIM_AUTO
    n_c, n_t = len(s.cam_init), len(s.tag_init)
    pairs = _all_pairs(n_c + n_t)
    with _handle(eng, s, s.cam_init, s.tag_init, elimination=mode) as ba:
        assert ba.solve(eng.default_options(robustify=0))["termination_type"] == eng.CONVERGENCE
        cam, tag = ba.get_state()
        cov = ba.covariance_blocks(pairs)
    tag_const = np.zeros(n_t, np.uint8)
    tag_const[0] = 1
    _Reference(oracle, s, cam, tag, False, np.zeros(n_c, np.uint8), tag_const).check(pairs, cov, case)


# ---- 5. constants and inactive poses -----------------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ["cams", "tags"])
def test_constant_and_residual_free_poses_give_zero_blocks(oracle, elim):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    n_c, n_t = len(s.cam_init), len(s.tag_init)
    cam_const, tag_const = const_sets(s, 3, 2)
    pairs = _all_pairs(n_c + n_t)
    lost = int(np.flatnonzero(cam_const == 0)[1])      # a free camera that loses all its observations
    mask = s.obs_cam != lost
    with _handle(eng, s, s.cam_init, s.tag_init, fixed_tag=-1,
                 elimination=eng.ELIM_CAMERAS if elim == "cams" else eng.ELIM_TAGS) as ba:
        ba.set_constant_poses(cam_const, tag_const)
        assert ba.solve(eng.default_options(robustify=0))["termination_type"] == eng.CONVERGENCE
        cam, tag = ba.get_state()
        cov = ba.covariance_blocks(pairs)
        ba.set_observation_mask(mask)
        cov_masked = ba.covariance_blocks(pairs)
    ref = _Reference(oracle, s, cam, tag, False, cam_const, tag_const)
    ref.check(pairs, cov, "20x10 elim %s, 3 constant tags, 2 constant cameras" % elim)
    const = set(np.flatnonzero(cam_const).tolist()) | {n_c + int(t) for t in np.flatnonzero(tag_const)}
    assert len(const) == 5
    n_zero = 0
    for (a, b), blk in zip(pairs.tolist(), cov):
        if a in const or b in const:
            assert not blk.any(), (a, b)
            n_zero += 1
        else:
            assert blk.any(), (a, b)
    assert n_zero > 0
    # the camera without observations is outside the problem: its blocks are zeros, the others are conditional on less
    cc = cam_const.copy()
    cc[lost] = 1
    ref = _Reference(oracle, s, cam, tag, False, cc, tag_const, obs_mask=mask)
    ref.check(pairs, cov_masked, "   camera %d without observations" % lost)
    for (a, b), blk in zip(pairs.tolist(), cov_masked):
        if a == lost or b == lost:
            assert not blk.any(), (a, b)


# ---- 6. a handle on the block-sparse path ------------------------------------------------------------------------------

def test_block_sparse_handle_switches_over_and_back(oracle, monkeypatch):
    """The create-time cost model keeps a scene of this size on the dense elimination, so the block-sparse path is
    asked for (VMM_BA_SCHUR, read at create), as test_gpu_constant_poses.py does on the same scene."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    monkeypatch.setenv("VMM_BA_SCHUR", "sparse")
    s = make_scene(2, n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)
    n_c, n_t = len(s.cam_init), len(s.tag_init)
    n = n_c + n_t
    rng = np.random.default_rng(11)
    cross = []
    while len(cross) < 50:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b:
            cross.append((a, b))
    pairs = np.concatenate([_marginal_pairs(n), np.array(cross, np.int32)])
    with _handle(eng, s, s.cam_init, s.tag_init) as ba:
        before = ba.solve(eng.default_options(robustify=0))
        assert before["termination_type"] == eng.CONVERGENCE and before["block_sparse"] == 1
        cam, tag = ba.get_state()
        cov = ba.covariance_blocks(pairs)
        after = ba.solve(eng.default_options(robustify=0))
    assert (after["block_sparse"], after["tree_ordering"]) == (before["block_sparse"], before["tree_ordering"])
    tag_const = np.zeros(n_t, np.uint8)
    tag_const[0] = 1
    ref = _Reference(oracle, s, cam, tag, False, np.zeros(n_c, np.uint8), tag_const)
    assert ref.order == 834
    ref.check(pairs, cov, "closeup 60x80 (block-sparse handle)")


# ---- 7. arguments ------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    n = len(s.cam_init) + len(s.tag_init)
    with _handle(eng, s, s.cam_init, s.tag_init) as ba:
        for bad in ([(-1, 0)], [(0, n)], [(0, 0), (n, 1)]):
            with pytest.raises(_lib.VmmBaError) as ei:
                ba.covariance_blocks(bad)
            assert ei.value.status == _lib.ERR_ARGUMENT, bad
        assert ba.covariance_blocks(np.zeros((0, 2), np.int32)).shape == (0, 6, 6)
        assert ba.covariance_blocks([(0, n - 1)]).any()
    with _handle(eng, s, s.cam_init, s.tag_init, landmarks=eng.LANDMARK_POINTS) as ba:
        with pytest.raises(_lib.VmmBaError) as ei:
            ba.covariance_blocks([(0, 0)])
        assert ei.value.status == _lib.ERR_STATE


# ---- 8. the driver and the command line --------------------------------------------------------------------------------

def test_driver_and_command_line(oracle, tmp_path, capsys):
    from visual_marker_mapping_amd import io as vio, synthetic, uncertainty
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    s = synthetic.make_scene(1)
    proj = str(tmp_path)
    synthetic.write_project(s, proj)
    rec = TagReconstructor(vio.readDetectionResult(os.path.join(proj, "marker_detections.json")))
    rec.setCameraModel(vio.readCameraModel(os.path.join(proj, "camera_intrinsics.json")))
    rec.startReconstructionGlobal(1)
    report = dict(rec.lastCovariances)
    got = rec.computePoseCovariances()
    assert got is rec.lastPoseCovariances
    assert sorted(got["tags"]) == sorted(rec.reconstructedTags) == list(range(len(s.tag_gt)))
    assert sorted(got["cameras"]) == sorted(rec.reconstructedCameras) == list(range(len(s.cam_gt)))
    assert all(np.array_equal(report[t], rec.lastCovariances[t]) for t in report)     # the printed report's blocks stay
    cam = np.array([np.r_[rec.reconstructedCameras[c].q, rec.reconstructedCameras[c].t] for c in range(len(s.cam_gt))])
    tag = np.array([np.r_[rec.reconstructedTags[t].q, rec.reconstructedTags[t].t] for t in range(len(s.tag_gt))])
    tag_const = np.zeros(len(tag), np.uint8)
    tag_const[rec.originTagId] = 1
    ref = _Reference(oracle, s, cam, tag, False, np.zeros(len(cam), np.uint8), tag_const)
    ids = list(range(len(cam) + len(tag)))
    cov = np.array([got["cameras"][c] for c in range(len(cam))] + [got["tags"][t] for t in range(len(tag))])
    ref.check(_marginal_pairs(len(ids)), cov, "driver, 20x10")
    assert not got["tags"][rec.originTagId].any()
    vio.exportReconstructions(os.path.join(proj, "reconstruction.json"), rec.reconstructedTags, rec.reconstructedCameras,
                              rec.getCameraModel())
    rec.close()
    capsys.readouterr()
    assert uncertainty.main(["--project_path", proj]) == 0
    with open(os.path.join(proj, "reconstruction_uncertainty.json")) as f:
        tree = json.load(f)
    assert tree["origin_tag_id"] == "0" and tree["robustify"] == "false"
    assert [int(e["id"]) for e in tree["reconstructed_tags"]] == sorted(got["tags"])
    assert [int(e["id"]) for e in tree["reconstructed_cameras"]] == sorted(got["cameras"])
    file_cov = np.array([[float(v) for v in e["covariance"]["coefficents"]]
                         for e in tree["reconstructed_cameras"] + tree["reconstructed_tags"]]).reshape(-1, 6, 6)
    ref.check(_marginal_pairs(len(ids)), file_cov, "command line, 20x10")
