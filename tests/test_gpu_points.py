"""Point-landmark variant on the GPU (vmm_ba_create_options.landmarks = VMM_BA_LANDMARK_POINTS), through the C-ABI,
against the CPU oracle's restatement of doBundleAdjustment_points (src/TagReconstructor.cpp:457-644) and
OpenCVReprojectionError (TagReconstructionCostFunction.h:9-84); the oracle's functor is pinned by the mpmath KATs
(tests/test_oracle_kat.py::test_point_functor_matches_mpmath).  PARITY UNPINNED against Ceres, like the tag model."""
import numpy as np
import pytest

from yardstick import assert_same_trace

pytestmark = pytest.mark.gpu
REL = 1e-6


def _ba(eng, s, elim="auto", cam=None, tag=None):
    mode = {"auto": eng.ELIM_AUTO, "cams": eng.ELIM_CAMERAS, "tags": eng.ELIM_TAGS}[elim]
    return eng.BundleAdjuster(s.intr, s.dist, s.cam_init if cam is None else cam, s.tag_init if tag is None else tag,
                              s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px, elimination=mode,
                              landmarks=eng.LANDMARK_POINTS)


def test_point_blocks_match_oracle(oracle):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=9, n_tags=6, visibility=0.8)    # README distortion
    sc, pts = oracle.point_scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                 s.obs_px)
    with _ba(eng, s) as ba:
        np.testing.assert_allclose(ba.get_points(), pts, rtol=0, atol=1e-15)     # computeMarkerCorners3D (:483)
        blk = ba.eval_blocks(robustify=False, want_W=False)
        cost = ba.cost(robustify=False)
    V, g = np.zeros((len(s.cam_init), 6, 6)), np.zeros((len(s.cam_init), 6))
    ref_cost = 0.0
    for c, t, px in zip(s.obs_cam, s.obs_tag, s.obs_px):
        for k in range(4):
            r, Jc, _ = oracle.point_eval(s.intr, s.dist, s.cam_init[c], pts[t, k], px[2 * k:2 * k + 2])
            V[c] += Jc.T @ Jc
            g[c] += Jc.T @ r
            ref_cost += 0.5 * (r @ r)
    np.testing.assert_allclose(cost, ref_cost, rtol=1e-12)
    np.testing.assert_allclose(blk["cost"], ref_cost, rtol=1e-12)
    np.testing.assert_allclose(blk["V"], V, rtol=0, atol=1e-10 * np.abs(V).max())
    np.testing.assert_allclose(blk["g_cam"], g, rtol=0, atol=1e-10 * np.abs(g).max())
    assert cost == pytest.approx(oracle.cost(sc, oracle.default_options(robustify=0)), rel=1e-12)


@pytest.mark.parametrize("elim", ["cams", "tags"])
def test_point_solve_matches_oracle(oracle, elim):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    with _ba(eng, s, elim) as ba:
        out = ba.solve(eng.default_options(robustify=0), trace_capacity=128)
        cam, _ = ba.get_state()
        pts = ba.get_points()
    sc, pts0 = oracle.point_scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                  s.obs_px)
    summ, trace = oracle.solve(sc, oracle.default_options(robustify=0, linear_solver=oracle.DENSE_NORMAL))
    assert out["termination_type"] == eng.CONVERGENCE
    assert_same_trace(out, summ, trace)
    scale = max(np.abs(sc.cam_qt).max(), np.abs(oracle.scene_points(sc)).max())
    np.testing.assert_allclose(cam, sc.cam_qt, rtol=0, atol=REL * scale)
    np.testing.assert_allclose(pts, oracle.scene_points(sc), rtol=0, atol=REL * scale)
    np.testing.assert_array_equal(pts[s.fixed_tag], pts0[s.fixed_tag])       # the origin tag's corners are constant


def test_point_zero_noise_recovers_corners_and_tag_poses(oracle):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, noise_px=0.0)
    with _ba(eng, s) as ba:
        out = ba.solve(eng.default_options(robustify=0, function_tolerance=1e-16, parameter_tolerance=1e-14,
                                           max_num_iterations=60))
        cam, tag = ba.get_state()
        pts = ba.get_points()
    _, gt = oracle.point_scene(s.intr, s.dist, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
    assert out["final_cost"] < 1e-10
    np.testing.assert_allclose(pts, gt, rtol=0, atol=1e-8)
    # tag poses rebuilt from the corners (src/TagReconstructor.cpp:608-639): the ground-truth poses again
    sign = np.sign(np.sum(tag[:, :4] * s.tag_gt[:, :4], axis=1))[:, None]
    np.testing.assert_allclose(tag[:, :4] * sign, s.tag_gt[:, :4], rtol=0, atol=1e-7)
    np.testing.assert_allclose(tag[:, 4:], s.tag_gt[:, 4:], rtol=0, atol=1e-8)
    sign = np.sign(np.sum(cam[:, :4] * s.cam_gt[:, :4], axis=1))[:, None]
    np.testing.assert_allclose(cam[:, :4] * sign, s.cam_gt[:, :4], rtol=0, atol=1e-8)


def test_point_full_size_matches_oracle(oracle):
    """500 images x 200 tags: 800 free points, 400 000 corner residual blocks."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(2)
    with _ba(eng, s) as ba:
        out = ba.solve(eng.default_options(robustify=0), trace_capacity=128)
        cam, tag = ba.get_state()
        pts = ba.get_points()
        ba.set_state(s.cam_init, s.tag_init)                # tag poses -> corners again: the same solve
        again = ba.solve(eng.default_options(robustify=0))
    sc, _ = oracle.point_scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                               s.obs_px)
    summ, trace = oracle.solve(sc, oracle.default_options(robustify=0, num_threads=8))
    assert out["termination_type"] == eng.CONVERGENCE
    assert_same_trace(out, summ, trace)
    scale = max(np.abs(sc.cam_qt).max(), np.abs(oracle.scene_points(sc)).max())
    np.testing.assert_allclose(cam, sc.cam_qt, rtol=0, atol=REL * scale)
    np.testing.assert_allclose(pts, oracle.scene_points(sc), rtol=0, atol=REL * scale)
    assert again["final_cost"] == out["final_cost"] and again["iterations"] == out["iterations"]
    # expected optimum: 8 residuals per tag observation, 6 parameters per camera + 12 per free tag
    n_res = 8 * s.n_obs
    expect = 0.5 * s.noise_px ** 2 * (n_res - 6 * len(cam) - 12 * (len(tag) - 1))
    assert abs(out["final_cost"] - expect) < 0.02 * expect
    assert np.abs(tag[:, 4:] - s.tag_gt[:, 4:]).max() < 5e-3      # rebuilt poses: near the ground truth


def test_point_mode_refuses_what_it_does_not_have():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=4, n_tags=3)
    with _ba(eng, s) as ba:
        with pytest.raises(Exception):
            ba.reprojection_stats()
        with pytest.raises(Exception):
            ba.tag_translation_covariance()
    with pytest.raises(Exception):
        eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px,
                           landmarks=eng.LANDMARK_POINTS, precision=eng.PRECISION_F32_ACCUM)
    with eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        with pytest.raises(Exception):
            ba.get_points()
