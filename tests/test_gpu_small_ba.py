"""GPU tests of vmm_ba_solve_small (engine.solve_small): a whole bundle adjustment in one workgroup, a batch per launch.

References: the CPU oracle where it has a counterpart (the iteration trace and the converged solution, as
tests/test_gpu_solve.py holds vmm_ba_solve to them), the handle path (BundleAdjuster, the code before this entry existed)
where it has none (constant poses, poses without observations), and the entry itself for the independence of a problem
from its batch (bit for bit).  Tolerances are the project's own: yardstick.assert_same_trace, assert_same_solution and
pose_gap against REL.
"""
import functools
import types

import numpy as np
import pytest

from yardstick import REL, assert_same_solution, assert_same_trace, const_sets, pose_gap

pytestmark = pytest.mark.gpu

REJECTED = dict(n_cams=20, n_tags=10, cam_rot_deg=50.0, cam_trans_m=0.8, tag_rot_deg=50.0, tag_trans_m=0.5)
# name -> (make_scene seed, its keywords, robustify): the differently sized scenes of the oracle cases
SIZES = {
    "20x10": (1, {}, 1),
    "30x12": (5, dict(n_cams=30, n_tags=12), 1),                      # distortion and outliers
    "70x24": (1, dict(n_cams=70, n_tags=24, visibility=0.3), 1),      # the limit: 24 kept tags, a camera with one observation
    "24x70": (1, dict(n_cams=24, n_tags=70, visibility=0.3), 1),      # the limit the other way round: 24 kept cameras
    "1x70": (1, dict(n_cams=1, n_tags=70), 0),                        # one kept pose, every tag seen once
    "130x3": (1, dict(n_cams=130, n_tags=3), 0),                      # more than two waves of observations on one pose
    "3x2": (1, dict(n_cams=3, n_tags=2), 1),
    "2x1": (1, dict(n_cams=2, n_tags=1), 1),
}


@functools.lru_cache(maxsize=None)
def _scene(seed, items):
    from visual_marker_mapping_amd.synthetic import make_scene
    return make_scene(seed, **dict(items))


def scene(seed, **kw):
    return _scene(seed, tuple(sorted(kw.items())))


def problem(s, fixed_tag=None):
    return (s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag if fixed_tag is None else fixed_tag, s.obs_cam,
            s.obs_tag, s.obs_px)


def oracle_run(O, s, **opt):
    sc = O.Scene(*problem(s))
    summ, trace = O.solve(sc, O.default_options(linear_solver=O.DENSE_NORMAL if len(s.cam_gt) <= 40 else O.SCHUR_AUTO, **opt))
    return summ, trace, sc


def small_run(s, elimination=None, **opt):
    from visual_marker_mapping_amd import engine as eng
    (cam, tag, out), = eng.solve_small([problem(s)], options=eng.default_options(**opt), trace_capacity=256,
                                       elimination=eng.ELIM_AUTO if elimination is None else elimination)
    return cam, tag, out


def against_oracle(O, s, rtol=1e-7, elimination=None, **opt):
    summ, trace, sc = oracle_run(O, s, **opt)
    cam, tag, out = small_run(s, elimination, **opt)
    print("oracle: termination %d, %d iterations, %d rejected, cost %.12g; device: %d iterations, cost %.12g" % (
        summ["termination_type"], summ["iterations"], summ["num_unsuccessful_steps"], summ["final_cost"], out["iterations"],
        out["final_cost"]))
    assert_same_trace(out, summ, trace, rtol=rtol)
    assert_same_solution(cam, tag, sc, s.tag_wh)
    assert not np.isnan(cam).any() and not np.isnan(tag).any()
    return out, summ


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ["cams", "tags"])
@pytest.mark.parametrize("robust", [0, 1])
def test_config1_matches_oracle(oracle, elim, robust):
    from visual_marker_mapping_amd import engine as eng
    mode = eng.ELIM_CAMERAS if elim == "cams" else eng.ELIM_TAGS
    out, summ = against_oracle(oracle, scene(1), elimination=mode, robustify=robust)
    assert out["elimination"] == mode and summ["termination_type"] == oracle.CONVERGENCE
    assert out["time_solve_s"] > 0.0 and out["time_eval_s"] == 0.0 and out["num_sync_timeouts"] == 0
    assert out["block_sparse"] == 0 and out["tree_ordering"] == 0
    assert out["num_jacobian_evals"] == summ["num_jacobian_evals"] and out["num_cost_evals"] == summ["num_cost_evals"]


def test_rejected_steps_match_oracle(oracle):
    out, summ = against_oracle(oracle, scene(1, **REJECTED), rtol=1e-6, robustify=0)
    assert summ["num_unsuccessful_steps"] >= 3 and summ["termination_type"] == oracle.CONVERGENCE
    assert [t["step_is_successful"] for t in out["trace"]].count(0) == summ["num_unsuccessful_steps"]


@pytest.mark.parametrize("name", [k for k in SIZES if k != "20x10"])
def test_sizes_match_oracle(oracle, name):
    from visual_marker_mapping_amd import engine as eng
    seed, kw, robust = SIZES[name]
    s = scene(seed, **kw)
    out, summ = against_oracle(oracle, s, robustify=robust)
    assert summ["termination_type"] == oracle.CONVERGENCE
    assert out["elimination"] == (eng.ELIM_CAMERAS if len(s.cam_gt) >= len(s.tag_gt) else eng.ELIM_TAGS)


def test_without_jacobi_scaling_matches_oracle(oracle):
    against_oracle(oracle, scene(1), robustify=1, jacobi_scaling=0)


def test_iteration_limit_matches_oracle(oracle):
    out, _ = against_oracle(oracle, scene(1), robustify=1, max_num_iterations=2)
    assert out["termination_type"] == oracle.NO_CONVERGENCE and out["iterations"] == 3


# ---- 2. against the handle path -------------------------------------------------------------------------------------------

def handle_run(s, fixed_tag, cam_const=None, tag_const=None, **opt):
    from visual_marker_mapping_amd import engine as eng
    with eng.BundleAdjuster(*problem(s, fixed_tag)) as ba:
        if cam_const is not None or tag_const is not None:
            ba.set_constant_poses(cam_const, tag_const)
        out = ba.solve(eng.default_options(**opt), trace_capacity=256)
        cam, tag = ba.get_state()
    return cam, tag, out


def against_handle(s, fixed_tag, cam_const=None, tag_const=None, **opt):
    from visual_marker_mapping_amd import engine as eng
    hcam, htag, hout = handle_run(s, fixed_tag, cam_const, tag_const, **opt)
    (cam, tag, out), = eng.solve_small([problem(s, fixed_tag)], cam_const=None if cam_const is None else [cam_const],
                                       tag_const=None if tag_const is None else [tag_const],
                                       options=eng.default_options(**opt), trace_capacity=256)
    print("handle: termination %d, %d iterations, cost %.12g; one launch: %d iterations, cost %.12g" % (
        hout["termination_type"], hout["iterations"], hout["final_cost"], out["iterations"], out["final_cost"]))
    assert_same_trace(out, hout, hout["trace"])
    assert_same_solution(cam, tag, types.SimpleNamespace(cam_qt=hcam, tag_qt=htag), s.tag_wh)
    return cam, tag, out


def test_constant_poses_match_the_handle_and_keep_their_bits():
    s = scene(1)
    cam_const, tag_const = const_sets(s, 3, 2)
    cam, tag, out = against_handle(s, -1, cam_const, tag_const, robustify=1)
    assert out["termination_type"] == 0 and cam_const.sum() == 2 and tag_const.sum() == 3
    np.testing.assert_array_equal(cam[cam_const != 0], s.cam_init[cam_const != 0])
    np.testing.assert_array_equal(tag[tag_const != 0], s.tag_init[tag_const != 0])
    assert np.abs(cam[cam_const == 0] - s.cam_init[cam_const == 0]).max() > 0.0


def test_problem_without_observations_matches_the_handle():
    s = scene(1)
    empty = types.SimpleNamespace(intr=s.intr, dist=s.dist, cam_init=s.cam_init, tag_init=s.tag_init, tag_wh=s.tag_wh,
                                  fixed_tag=s.fixed_tag, obs_cam=s.obs_cam[:0], obs_tag=s.obs_tag[:0], obs_px=s.obs_px[:0])
    cam, tag, out = against_handle(empty, s.fixed_tag, robustify=1)
    assert out["iterations"] == 1 and out["final_cost"] == 0.0
    np.testing.assert_array_equal(cam, s.cam_init)
    np.testing.assert_array_equal(tag, s.tag_init)


def test_unobserved_camera_and_tag_are_inactive_and_unchanged():
    s = scene(1)
    c, t = len(s.cam_gt) - 1, len(s.tag_gt) - 1
    assert t != s.fixed_tag
    keep = (s.obs_cam != c) & (s.obs_tag != t)
    part = types.SimpleNamespace(intr=s.intr, dist=s.dist, cam_init=s.cam_init, tag_init=s.tag_init, tag_wh=s.tag_wh,
                                 fixed_tag=s.fixed_tag, obs_cam=s.obs_cam[keep], obs_tag=s.obs_tag[keep], obs_px=s.obs_px[keep])
    cam, tag, out = against_handle(part, s.fixed_tag, robustify=1)
    assert out["termination_type"] == 0 and out["iterations"] > 2
    np.testing.assert_array_equal(cam[c], s.cam_init[c])
    np.testing.assert_array_equal(tag[t], s.tag_init[t])


# ---- 3. independence --------------------------------------------------------------------------------------------------------

def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for k in ("termination_type", "iterations", "num_successful_steps", "num_unsuccessful_steps", "num_lm_iterations",
              "num_jacobian_evals", "num_cost_evals", "elimination"):
        assert a[2][k] == b[2][k], k
    np.testing.assert_array_equal([a[2]["initial_cost"], a[2]["final_cost"]], [b[2]["initial_cost"], b[2]["final_cost"]])
    assert len(a[2]["trace"]) == len(b[2]["trace"]) > 0
    for ra, rb in zip(a[2]["trace"], b[2]["trace"]):
        np.testing.assert_array_equal([ra[k] for k in ra], [rb[k] for k in rb])


def test_a_problem_gives_the_same_bits_alone_and_anywhere_in_a_batch():
    from visual_marker_mapping_amd import engine as eng
    ps = [problem(scene(seed, **kw)) for seed, kw, _ in SIZES.values()]
    run = lambda batch: eng.solve_small(batch, options=eng.default_options(robustify=1), trace_capacity=64)
    forward = run(ps)
    backward = run(ps[::-1])[::-1]
    alone = [run([p])[0] for p in ps]
    again = run(ps)
    for f, b, a, g in zip(forward, backward, alone, again):
        _same(f, b)
        _same(f, a)
        _same(f, g)


def test_more_problems_than_compute_units_give_identical_copies():
    from visual_marker_mapping_amd import engine as eng
    out = eng.solve_small([problem(scene(1))] * 300, options=eng.default_options(robustify=1), trace_capacity=32)
    assert len(out) == 300 and out[0][2]["termination_type"] == 0
    for o in out[1:]:
        _same(out[0], o)


# ---- 4. the driver ------------------------------------------------------------------------------------------------------------

def test_start_reconstruction_in_one_launch_reaches_the_same_map(tmp_path, capsys, monkeypatch):
    from visual_marker_mapping_amd import engine as eng, io as vio, synthetic
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    s = synthetic.make_scene(1, n_cams=12, n_tags=8)
    synthetic.write_project(s, str(tmp_path))
    model = vio.readCameraModel(str(tmp_path / "camera_intrinsics.json"))
    runs, calls, inner = [], [], eng.solve_small
    monkeypatch.setattr(eng, "solve_small", lambda *a, **k: calls.append(len(a[0])) or inner(*a, **k))
    for one_launch in (False, True):
        rec = TagReconstructor(vio.readDetectionResult(str(tmp_path / "marker_detections.json")))
        rec.setCameraModel(model)
        rec.startReconstruction(1, oneLaunch=one_launch)
        out = capsys.readouterr().out
        assert out.count("Solution ") == len(rec.reconstructedCameras) + 2
        # every bundle adjustment but the last (printSummary) fits (at most 12 x 8) and goes through solve_small
        assert len(calls) == (len(rec.reconstructedCameras) + 1 if one_launch else 0)
        runs.append(rec)
        rec.close()
    ref, one = runs
    assert sorted(one.reconstructedTags) == sorted(ref.reconstructedTags)         # the same prunings
    assert sorted(one.reconstructedCameras) == sorted(ref.reconstructedCameras)
    flat = lambda d: np.array([np.r_[d[k].q, d[k].t] for k in sorted(d)])
    for a, b in ((one.reconstructedTags, ref.reconstructedTags), (one.reconstructedCameras, ref.reconstructedCameras)):
        dq, dt = pose_gap(flat(a), flat(b))
        print("one launch against the handle path: dq %.3g, dt %.3g" % (dq, dt))
        assert dq <= REL and dt <= REL
