"""GPU tests of the one-shot map initialisation (vmm_ba_quad_poses, vmm_ba_initialize, startReconstructionGlobal).

Yardsticks: exact data (zero noise) for the planar solver and the whole recipe; pnp.py (the host implementation
the incremental driver uses) for the planar solver under noise; and for everything downstream the optimum the
bundle adjustment reaches from the scene generator's perturbed ground truth -- an initialisation is right when
the solver ends in the same place from it.  Tolerances: 1e-9 on exact data, 1e-6 per pose between two optima
(parity gate).
The stronger check, stage by stage against a longdouble truth: tests/test_gpu_init_accuracy.py.
"""
import numpy as np
import pytest

import yardstick as ys

pytestmark = pytest.mark.gpu

INTR = (8075.29, 8083.17, 3016.39, 1996.29)
DIST = (-0.18618, 0.37018, -2.939e-4, 4.153e-4, 0.05704)

SCENES = {
    "config1_20x10": (1, {}),
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "closeup_60x80": (2, dict(n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)),
    "config5_30x40": (5, dict(n_cams=30, n_tags=40, visibility=0.5)),
    "small_tags_30x200": (2, dict(n_cams=30, n_tags=200, visibility=0.4)),
}


def _quad(w, h):
    return np.array([[-w / 2, -h / 2, 0], [w / 2, -h / 2, 0], [w / 2, h / 2, 0], [-w / 2, h / 2, 0]])


def _placeholders(s):
    """Start poses that carry no information: cameras at q = 1, t = (0, 0, 1), tags at identity, the origin tag at
    its ground-truth pose."""
    cam = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 1.0]), (len(s.cam_gt), 1))
    tag = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0.0]), (len(s.tag_gt), 1))
    tag[s.fixed_tag] = s.tag_gt[s.fixed_tag]
    return cam, tag


def _handle(eng, s, cam, tag, **kw):
    return eng.BundleAdjuster(s.intr, s.dist, cam, tag, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px, **kw)


def _two_solves(eng, ba):
    a = ba.solve(eng.default_options(robustify=1, max_num_iterations=1500))
    b = ba.solve(eng.default_options(robustify=0, max_num_iterations=1500, function_tolerance=1e-14,
                                     parameter_tolerance=1e-12))
    return a, b


def _same_optimum(eng, s, label, mask_init=None, mask_solve=None, keep_cam=None, keep_tag=None):
    """Check 3: handle A = placeholders + initialize, handle B = the perturbed ground truth; the same two solves."""
    cam0, tag0 = _placeholders(s)
    with _handle(eng, s, cam0, tag0) as A, _handle(eng, s, s.cam_init, s.tag_init) as B:
        if mask_init is not None:
            A.set_observation_mask(mask_init)
        report, cam_ok, tag_ok = A.initialize()
        cam_i, tag_i = A.get_state()
        if mask_solve is not None:
            A.set_observation_mask(mask_solve)
            B.set_observation_mask(mask_solve)
        a_rob, a_plain = _two_solves(eng, A)
        b_rob, b_plain = _two_solves(eng, B)
        camA, tagA = A.get_state()
        camB, tagB = B.get_state()
    kc = np.ones(len(camA), bool) if keep_cam is None else keep_cam
    kt = np.ones(len(tagA), bool) if keep_tag is None else keep_tag
    gq_c, gt_c = ys.pose_gap(camA[kc], camB[kc])
    gq_t, gt_t = ys.pose_gap(tagA[kt], tagB[kt])
    print("%s: obs %d rounds %d reached %d/%d cams %d/%d tags, avg reprojection after initialize %.4g px; robust "
          "iterations A %d B %d, plain A %d B %d; max |dq| cams %.3g tags %.3g, max |dt| cams %.3g tags %.3g; "
          "final cost A %.12g B %.12g; initialize %.4f s"
          % (label, s.n_obs, report["rounds"], report["cams_reached"], len(cam_ok), report["tags_reached"], len(tag_ok),
             report["avg_reprojection_px"], a_rob["iterations"], b_rob["iterations"], a_plain["iterations"],
             b_plain["iterations"], gq_c, gq_t, gt_c, gt_t, a_plain["final_cost"], b_plain["final_cost"],
             report["time_s"]))
    for out in (a_rob, a_plain, b_rob, b_plain):
        assert out["termination_type"] == eng.CONVERGENCE, out
    assert max(gq_c, gq_t) <= 1e-6 and max(gt_c, gt_t) <= 1e-6, (gq_c, gq_t, gt_c, gt_t)
    return report, cam_ok, tag_ok, (cam0, tag0), (cam_i, tag_i)


# ---- 1. the planar solver on exact data ---------------------------------------------------------------------------

@pytest.mark.parametrize("dist", [(0.0,) * 5, DIST])
def test_quad_poses_recover_exact_poses(dist):
    from visual_marker_mapping_amd import engine as eng, pnp
    rng = np.random.default_rng(7)
    w = 0.1285
    quad = _quad(w, w)
    Rs, ts, px = [], [], []
    for _ in range(10):
        R = pnp.rodrigues(rng.normal(size=3) * 0.4)
        t = np.array([rng.normal() * 0.2, rng.normal() * 0.2, 3.0 + 3.0 * rng.random()])
        Rs.append(R)
        ts.append(t)
        px.append(eng.project_points(INTR, dist, quad @ R.T + t).reshape(8))
    qt2, rms2 = eng.quad_poses(INTR, dist, np.full((10, 2), w), np.array(px))
    assert np.all(np.isfinite(qt2)) and np.all(rms2[:, 0] <= rms2[:, 1])
    worst = 0.0
    for i in range(10):
        eR = np.abs(ys.rotation(qt2[i, 0, :4]) - Rs[i]).max()
        et = np.abs(qt2[i, 0, 4:] - ts[i]).max()
        worst = max(worst, eR, et)
        print("pose %d: |dR| %.3g |dt| %.3g rms %.3g / %.3g px" % (i, eR, et, rms2[i, 0], rms2[i, 1]))
        assert eR < 1e-9 and et < 1e-9, (i, eR, et)
    print("distortion %s: worst error %.3g" % ("on" if any(dist) else "off", worst))


def test_quad_poses_degenerate_observation_gives_inf_not_nan():
    from visual_marker_mapping_amd import engine as eng
    px = np.array([[100.0, 100.0] * 4,                      # four coincident corners
                   [100.0, 100.0, 200.0, 100.0, 300.0, 100.0, 400.0, 100.0]])   # collinear
    qt2, rms2 = eng.quad_poses(INTR, (0.0,) * 5, np.full((2, 2), 0.1), px)
    assert np.all(np.isfinite(qt2))
    assert np.all(np.isposinf(rms2) | np.isfinite(rms2)) and np.isposinf(rms2[0]).all()


# ---- 2. against the host implementation, under noise ---------------------------------------------------------------

def test_quad_poses_against_pnp_on_config1():
    from visual_marker_mapping_amd import engine as eng, pnp
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    assert s.n_obs == 200 and not np.any(s.dist)
    qt2, rms2 = eng.quad_poses(s.intr, s.dist, s.tag_wh[s.obs_tag], s.obs_px)
    intr, dist = tuple(s.intr), tuple(s.dist)
    worst_ratio, worst_angle = 0.0, 0.0
    for i in range(s.n_obs):
        Q = _quad(*s.tag_wh[s.obs_tag[i]])
        px = s.obs_px[i].reshape(4, 2)
        R, t = pnp.solvePnP(Q, px, intr, dist)
        rms_cpu = np.sqrt(((pnp.project(Q, R, t, intr, dist) - px) ** 2).sum(axis=1).mean())
        # the kernel's own RMS is what it says it is
        for k in range(2):
            e = pnp.project(Q, ys.rotation(qt2[i, k, :4]), qt2[i, k, 4:], intr, dist) - px
            assert abs(np.sqrt((e ** 2).sum(axis=1).mean()) - rms2[i, k]) <= 1e-9 * max(1.0, rms2[i, k])
        worst_ratio = max(worst_ratio, rms2[i, 0] / rms_cpu)
        assert rms2[i, 0] <= rms_cpu * (1 + 1e-6), (i, rms2[i], rms_cpu)
        Rg = ys.rotation(s.cam_gt[s.obs_cam[i], :4]) @ ys.rotation(s.tag_gt[s.obs_tag[i], :4])
        ang = min(np.degrees(np.arccos(np.clip((np.trace(Rg.T @ ys.rotation(qt2[i, k, :4])) - 1) / 2, -1, 1))) for k in range(2))
        worst_angle = max(worst_angle, ang)
        assert ang < 10.0, (i, ang)
    print("200 observations: max rms_gpu / rms_cpu %.9f, worst angle of the better solution %.3f deg"
          % (worst_ratio, worst_angle))


# ---- 3. same optimum as from the perturbed ground truth ----------------------------------------------------------------

@pytest.mark.parametrize("name", list(SCENES))
def test_initialize_leads_to_the_same_optimum(name):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    report, cam_ok, tag_ok, _, _ = _same_optimum(eng, s, name)
    assert cam_ok.all() and tag_ok.all()
    assert report["cams_reached"] == len(s.cam_gt) and report["tags_reached"] == len(s.tag_gt)


# ---- 4. zero noise ---------------------------------------------------------------------------------------------------

def test_initialize_zero_noise_reaches_ground_truth():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, noise_px=0.0)
    cam0, tag0 = _placeholders(s)
    with _handle(eng, s, cam0, tag0) as ba:
        report, cam_ok, tag_ok = ba.initialize()
        print("zero noise: average reprojection error straight after initialize %.3g px, %d rounds"
              % (report["avg_reprojection_px"], report["rounds"]))
        _two_solves(eng, ba)
        cam, tag = ba.get_state()
    assert cam_ok.all() and tag_ok.all()
    for got, gt in ((cam, s.cam_gt), (tag, s.tag_gt)):
        sign = np.sign(np.sum(got[:, :4] * gt[:, :4], axis=1))[:, None]
        print("zero noise: max |dq| %.3g max |dt| %.3g" % (np.abs(got[:, :4] * sign - gt[:, :4]).max(),
                                                          np.abs(got[:, 4:] - gt[:, 4:]).max()))
        np.testing.assert_allclose(got[:, :4] * sign, gt[:, :4], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got[:, 4:], gt[:, 4:], rtol=0, atol=1e-9)


# ---- 5. determinism --------------------------------------------------------------------------------------------------

def test_initialize_is_bit_identical_from_run_to_run():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES["100x60_vis0.30"]
    s = make_scene(cfg, **kw)
    states = []
    for _ in range(2):
        cam0, tag0 = _placeholders(s)
        with _handle(eng, s, cam0, tag0) as ba:
            ba.initialize()
            states.append(ba.get_state())
    assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])
    assert not np.array_equal(states[0][0], _placeholders(s)[0])


# ---- 6. reach and errors -----------------------------------------------------------------------------------------------

def test_initialize_reach_flags_and_untouched_state():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    lost_cam, lone_tag = len(s.cam_gt) - 1, len(s.tag_gt) - 1
    assert lone_tag != s.fixed_tag
    mask_init = s.obs_cam != lost_cam                       # the camera sees nothing at all
    of_tag = np.flatnonzero((s.obs_tag == lone_tag) & mask_init)
    assert len(of_tag) >= 2
    mask_init[of_tag[1:]] = False                           # the tag keeps a single observation
    mask_solve = mask_init & (s.obs_tag != lone_tag)
    keep_cam = np.arange(len(s.cam_gt)) != lost_cam
    keep_tag = np.arange(len(s.tag_gt)) != lone_tag
    report, cam_ok, tag_ok, (cam0, tag0), (cam_i, tag_i) = _same_optimum(
        eng, s, "masked config1", mask_init=mask_init, mask_solve=mask_solve, keep_cam=keep_cam, keep_tag=keep_tag)
    assert np.array_equal(cam_ok, keep_cam) and np.array_equal(tag_ok, keep_tag)
    assert report["cams_reached"] == len(s.cam_gt) - 1 and report["tags_reached"] == len(s.tag_gt) - 1
    assert cam_i[lost_cam].tobytes() == cam0[lost_cam].tobytes()
    assert tag_i[lone_tag].tobytes() == tag0[lone_tag].tobytes()
    assert tag_i[s.fixed_tag].tobytes() == tag0[s.fixed_tag].tobytes()   # the origin keeps its pose


def test_initialize_errors():
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    cam0, tag0 = _placeholders(s)
    with eng.BundleAdjuster(s.intr, s.dist, cam0, tag0, s.tag_wh, -1, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        with pytest.raises(_lib.VmmBaError) as ei:
            ba.initialize()
        assert ei.value.status == _lib.ERR_ARGUMENT
    with _handle(eng, s, cam0, tag0, landmarks=eng.LANDMARK_POINTS) as ba:
        with pytest.raises(_lib.VmmBaError) as ei:
            ba.initialize()
        assert ei.value.status == _lib.ERR_STATE
    half = s.obs_cam < len(s.cam_gt) // 2
    with eng.BundleAdjuster(s.intr, s.dist, cam0, tag0, s.tag_wh, s.fixed_tag, s.obs_cam[half], s.obs_tag[half],
                            s.obs_px[half], rank=0, world_size=2) as ba:
        with pytest.raises(_lib.VmmBaError) as ei:
            ba.initialize()
        assert ei.value.status == _lib.ERR_STATE
    with _handle(eng, s, cam0, tag0) as ba:
        with pytest.raises(AttributeError):
            ba.initialize(no_such_option=1)
        with pytest.raises(_lib.VmmBaError) as ei:
            ba.initialize(score_cap_px=0.0)
        assert ei.value.status == _lib.ERR_ARGUMENT


def test_get_state_after_set_state_and_initialize():
    """flush_state semantics: poses staged by set_state reach the device before initialize reads the origin tag, and a
    get_state afterwards returns the initialised poses."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    cam0, tag0 = _placeholders(s)
    with _handle(eng, s, cam0, tag0) as a, _handle(eng, s, s.cam_init, s.tag_init) as b:
        a.initialize()
        b.set_state(cam0, tag0)
        b.initialize()
        ca, ta = a.get_state()
        cb, tb = b.get_state()
    assert np.array_equal(ca, cb) and np.array_equal(ta, tb)


# ---- 7. the driver -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [2, 1])   # 2: the scene of `bench.py --workload incremental`; 1: the same sizes, config 1
def test_start_reconstruction_global_matches_the_incremental_driver(cfg, tmp_path, capsys):
    from visual_marker_mapping_amd import io as vio, synthetic
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    s = synthetic.make_scene(cfg, n_cams=100, n_tags=60, visibility=0.30)
    synthetic.write_project(s, str(tmp_path))
    model = vio.readCameraModel(str(tmp_path / "camera_intrinsics.json"))
    glob = TagReconstructor(vio.readDetectionResult(str(tmp_path / "marker_detections.json")))
    glob.setCameraModel(model)
    glob.startReconstructionGlobal(1)
    out = capsys.readouterr().out
    assert glob.originTagId == 0 and out.count("Solution ") == 2 and "Starting final bundle adjustment" in out
    assert glob.reconstructedTags[0].q.tolist() == [1.0, 0.0, 0.0, 0.0] and glob.reconstructedTags[0].t.tolist() == [0.0] * 3
    inc = TagReconstructor(vio.readDetectionResult(str(tmp_path / "marker_detections.json")))
    inc.setCameraModel(model)
    inc.startReconstruction(1)
    capsys.readouterr()
    assert sorted(glob.reconstructedCameras) == sorted(inc.reconstructedCameras)
    assert sorted(glob.reconstructedTags) == sorted(inc.reconstructedTags)
    fg, fi = glob.lastSummary["final_cost"], inc.lastSummary["final_cost"]
    with capsys.disabled():
        print("\ndriver: final cost global %.12g incremental %.12g (relative difference %.3g); %d cameras, %d tags; "
              "initialisation %s" % (fg, fi, abs(fg - fi) / fi, len(glob.reconstructedCameras),
                                     len(glob.reconstructedTags), glob.lastInitReport))
    assert abs(fg - fi) <= 1e-6 * fi
    for t in glob.reconstructedTags:
        er = np.abs(ys.rotation(glob.reconstructedTags[t].q) - ys.rotation(s.tag_gt[t, :4])).max()
        et = np.abs(glob.reconstructedTags[t].t - s.tag_gt[t, 4:]).max()
        assert er < 5e-3 and et < 5e-3, (t, er, et)


def test_start_reconstruction_global_errors(capsys):
    from visual_marker_mapping_amd import io as vio
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    det = vio.DetectionResult([vio.TagImg(0, "a")], [vio.Tag(5, "t", 0.1, 0.1)], [])
    rec = TagReconstructor(det)
    rec.setOriginTagId(9)
    with pytest.raises(RuntimeError, match="Could not use tag with id 9 as origin tag, because it was not detected."):
        rec.startReconstructionGlobal()
    # the origin tag is known but no image sees it: nothing can be placed
    rec = TagReconstructor(vio.DetectionResult([vio.TagImg(0, "a")], [vio.Tag(5, "t", 0.1, 0.1)], []))
    with pytest.raises(RuntimeError, match="No reconstructed tags in image found."):
        rec.startReconstructionGlobal()
