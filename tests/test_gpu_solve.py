"""GPU parity tests of the whole hot path (vmm_ba_solve) against the CPU oracle.

north_star tolerance: converged poses / marker corners within 1e-6 relative of the reference
semantics on the same detections.  The oracle restates Ceres' trust-region policy (PARITY UNPINNED
against Ceres itself, see oracle/vmm_oracle.h), so beyond the end state the whole iteration trace is
compared.
"""
import numpy as np
import pytest

from yardstick import REL, assert_same_solution, assert_same_trace

pytestmark = pytest.mark.gpu



def _run_both(eng, O, s, elim, **opt):
    mode = {"auto": eng.ELIM_AUTO, "cams": eng.ELIM_CAMERAS, "tags": eng.ELIM_TAGS}[elim]
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam,
                            s.obs_tag, s.obs_px, elimination=mode)
    out = ba.solve(eng.default_options(**opt), trace_capacity=256)
    cam, tag = ba.get_state()
    ba.close()
    sc = O.Scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
    oopt = {k: v for k, v in opt.items() if k != "poll_interval"}
    summ, trace = O.solve(sc, O.default_options(linear_solver=O.DENSE_NORMAL if len(s.cam_gt) <= 40 else O.SCHUR_AUTO,
                                                **oopt))
    return out, cam, tag, summ, trace, sc


@pytest.mark.parametrize("elim", ["cams", "tags"])
@pytest.mark.parametrize("robust", [0, 1])
def test_config1_matches_oracle(oracle, elim, robust):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)  # BASELINE.json configs[0]: 20 images x 10 tags
    out, cam, tag, summ, trace, sc = _run_both(eng, oracle, s, elim, robustify=robust)
    assert_same_trace(out, summ, trace)
    assert_same_solution(cam, tag, sc, s.tag_wh)


def test_distortion_outliers_robust_matches_oracle(oracle):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=30, n_tags=12)  # configs[4] shape at a size the dense oracle solves fast
    out, cam, tag, summ, trace, sc = _run_both(eng, oracle, s, "auto", robustify=1)
    assert_same_trace(out, summ, trace)
    assert_same_solution(cam, tag, sc, s.tag_wh)


def test_sparse_visibility_matches_oracle(oracle):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=40, n_tags=30, visibility=0.25)
    out, cam, tag, summ, trace, sc = _run_both(eng, oracle, s, "auto", robustify=1)
    assert_same_trace(out, summ, trace)
    assert_same_solution(cam, tag, sc, s.tag_wh)


def test_zero_noise_scene_recovers_ground_truth():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, noise_px=0.0)
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam,
                            s.obs_tag, s.obs_px)
    out = ba.solve(eng.default_options(robustify=0, function_tolerance=1e-16, parameter_tolerance=1e-14,
                                       max_num_iterations=50))
    cam, tag = ba.get_state()
    ba.close()
    assert out["final_cost"] < 1e-10
    for got, gt in ((cam, s.cam_gt), (tag, s.tag_gt)):
        sign = np.sign(np.sum(got[:, :4] * gt[:, :4], axis=1))[:, None]
        np.testing.assert_allclose(got[:, :4] * sign, gt[:, :4], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got[:, 4:], gt[:, 4:], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(tag[0], s.tag_init[0])  # origin tag constant


def test_iteration_cap_and_polling_do_not_change_results():
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    res = []
    for poll in (1, 4):
        ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam,
                                s.obs_tag, s.obs_px)
        out = ba.solve(eng.default_options(poll_interval=poll), trace_capacity=64)
        res.append((out, ba.get_state()))
        capped = None
        ba.set_state(s.cam_init, s.tag_init)
        capped = ba.solve(eng.default_options(max_num_iterations=2, poll_interval=poll))
        assert capped["termination_type"] == eng.NO_CONVERGENCE and capped["iterations"] == 3
        ba.close()
    assert res[0][0]["iterations"] == res[1][0]["iterations"]
    np.testing.assert_array_equal(res[0][1][0], res[1][1][0])
    np.testing.assert_array_equal(res[0][1][1], res[1][1][1])


@pytest.mark.parametrize("cfg", [2])
def test_full_size_config2_properties(oracle, cfg):
    """BASELINE.json configs[1] (500 x 200, f64): trace parity with the oracle's Schur path plus
    size-independent properties (cost decreases monotonically, origin fixed, unit quaternions)."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(cfg)
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam,
                            s.obs_tag, s.obs_px)
    out = ba.solve(eng.default_options(robustify=0), trace_capacity=64)
    cam, tag = ba.get_state()
    ba.close()
    costs = [t["cost"] for t in out["trace"] if t["step_is_successful"]]
    assert all(b < a for a, b in zip(costs, costs[1:]))
    assert out["termination_type"] == eng.CONVERGENCE
    np.testing.assert_array_equal(tag[0], s.tag_init[0])
    np.testing.assert_allclose(np.linalg.norm(cam[:, :4], axis=1), 1.0, atol=1e-12)
    # expected optimum cost ~ 1/2 * sigma^2 * (residuals - dof)
    n_res = 8 * s.n_obs
    expect = 0.5 * s.noise_px ** 2 * (n_res - 6 * (len(cam) + len(tag) - 1))
    assert abs(out["final_cost"] - expect) < 0.02 * expect
    sc = oracle.Scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
    summ, trace = oracle.solve(sc, oracle.default_options(robustify=0, num_threads=8))
    assert_same_trace(out, summ, trace)
    assert_same_solution(cam, tag, sc, s.tag_wh)


@pytest.mark.parametrize("elim", ["cams", "tags"])
@pytest.mark.parametrize("robust", [False, True])
def test_tag_translation_covariance_matches_oracle(oracle, elim, robust):
    """ceres::Covariance block of src/TagReconstructor.cpp:744-783: 3x3 blocks of (J^T J)^-1.  GPU: Schur
    factor + blocked forward substitution; oracle: dense Cholesky of the full normal matrix.  1e-6 relative."""
    from visual_marker_mapping_amd import engine
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5 if robust else 1, n_cams=30, n_tags=14, visibility=0.7)
    e = engine.ELIM_CAMERAS if elim == "cams" else engine.ELIM_TAGS
    ba = engine.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px,
                               elimination=e)
    try:
        ba.solve(engine.default_options(robustify=int(robust)))
        cam, tag = ba.get_state()
        cov = ba.tag_translation_covariance(robustify=robust)
        cov2 = ba.tag_translation_covariance(robustify=robust)      # idempotent, leaves the state alone
        cam2, tag2 = ba.get_state()
        again = ba.solve(engine.default_options(robustify=int(robust)))   # and the handle still solves
    finally:
        ba.close()
    assert np.array_equal(cov, cov2) and np.array_equal(cam, cam2) and np.array_equal(tag, tag2)
    assert again["termination_type"] == engine.CONVERGENCE
    sc = oracle.Scene(s.intr, s.dist, cam, tag, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px)
    ref = oracle.tag_translation_covariance(sc, oracle.default_options(robustify=int(robust)))
    assert np.all(cov[0] == 0.0)                                     # origin tag: constant block
    for t in range(1, len(tag)):
        scale = np.abs(ref[t]).max()
        assert scale > 0
        np.testing.assert_allclose(cov[t], ref[t], rtol=0, atol=1e-6 * scale)
        assert np.all(np.linalg.eigvalsh(cov[t]) > 0)


@pytest.mark.parametrize("n_tags", [260, 560])
def test_tag_translation_covariance_on_every_factorisation_path(monkeypatch, n_tags):
    """The covariance needs the factor, the reciprocal diagonals and the inverse of EVERY diagonal block.  Reduced tag
    systems of 25 blocks (k_chol_dataflow with more workgroups than compute units) and 53 blocks (k_chol_step for the
    leading columns + k_chol_dataflow on the trailing ones) against the same handle data factored by one k_chol_step
    launch per block column (VMM_BA_NO_DATAFLOW=1, read at create)."""
    from visual_marker_mapping_amd import engine
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=2 * n_tags, n_tags=n_tags, visibility=0.1)
    covs = []
    for no_df in ("0", "1"):
        monkeypatch.setenv("VMM_BA_NO_DATAFLOW", no_df)
        ba = engine.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px,
                                   elimination=engine.ELIM_CAMERAS)
        try:
            out = ba.solve(engine.default_options(robustify=0))
            assert out["termination_type"] == engine.CONVERGENCE and out["num_sync_timeouts"] == 0
            ba.set_state(s.cam_gt, s.tag_gt)              # the same point for both handles
            covs.append(ba.tag_translation_covariance(robustify=False))
        finally:
            ba.close()
    assert np.all(covs[0][0] == 0.0)
    for t in range(1, n_tags):
        scale = np.abs(covs[1][t]).max()
        assert scale > 0
        np.testing.assert_allclose(covs[0][t], covs[1][t], rtol=0, atol=1e-9 * scale)


@pytest.mark.parametrize("config", [1, 5])
def test_f32_accumulate_precision_reaches_the_f64_optimum(oracle, config):
    """VMM_BA_PRECISION_F32_ACCUM (BASELINE.json configs[3]): J^T J blocks in f32, residuals / gradient /
    reduced system / LM decisions in f64.  The blocks match the oracle to f32 rounding and the solve ends at
    the f64 optimum: cost to 1e-8 relative, poses to 1e-5 of the pose scale (both runs stop on the same
    1e-6 relative-cost-change test, somewhere inside that distance of the minimiser)."""
    from visual_marker_mapping_amd import engine
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(config, n_cams=40, n_tags=16)
    robust = config == 5
    res = {}
    for name, prec in (("f64", engine.PRECISION_F64), ("f32", engine.PRECISION_F32_ACCUM)):
        ba = engine.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px,
                                   precision=prec)
        try:
            blocks = ba.eval_blocks(robustify=robust)
            summ = ba.solve(engine.default_options(robustify=int(robust)))
            cam, tag = ba.get_state()
            cost = ba.cost(robustify=robust)
        finally:
            ba.close()
        res[name] = (blocks, summ, cam, tag, cost)
    b64, b32 = res["f64"][0], res["f32"][0]
    for key in ("V", "U", "W"):
        scale = np.abs(b64[key]).max()
        assert np.abs(b32[key] - b64[key]).max() < 2e-5 * scale          # f32 products summed over <= 64 x 8 rows
        assert np.abs(b32[key] - b64[key]).max() > 0                      # and it really is a different precision
    np.testing.assert_allclose(b32["g_cam"], b64["g_cam"], rtol=0, atol=1e-12 * np.abs(b64["g_cam"]).max())   # f64 both
    assert b32["cost"] == b64["cost"]
    assert res["f32"][1]["termination_type"] == engine.CONVERGENCE
    assert abs(res["f32"][4] - res["f64"][4]) <= 1e-8 * res["f64"][4]
    for k in (2, 3):
        scale = np.abs(res["f64"][k]).max()
        assert np.abs(res["f32"][k] - res["f64"][k]).max() < 1e-5 * scale
    with pytest.raises(Exception):
        engine.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px,
                              precision=7)


def test_phase_report_accounts_for_the_solve():
    """vmm_ba_summary.time_*_s (the per-phase part of summary.FullReport(), src/TagReconstructor.cpp:741-742): device
    time per group measured with in-kernel 100 MHz stamps.  Every phase ran, and together they fit into the wall
    time of the call."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(2)
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                            s.obs_px)
    try:
        ba.solve(eng.default_options(robustify=0))            # first call: graph capture
        ba.set_state(s.cam_init, s.tag_init)
        out = ba.solve(eng.default_options(robustify=0))
    finally:
        ba.close()
    phases = [out[k] for k in ("time_eval_s", "time_eliminate_s", "time_factor_solve_s", "time_step_s", "time_control_s")]
    assert all(p > 0.0 for p in phases)
    assert sum(phases) <= out["time_solve_s"]
    assert sum(phases) >= 0.5 * out["time_solve_s"]           # the device is busy for most of a solve
    n = out["num_lm_iterations"]
    assert 50e-6 * n < out["time_factor_solve_s"] < 1e-3 * n   # the Cholesky dominates: 0.2-0.3 ms per iteration
    assert out["time_eval_s"] < out["time_factor_solve_s"]


@pytest.mark.parametrize("elim", ["cams", "tags"])
def test_rejected_steps_match_oracle(oracle, elim):
    """A start far from the optimum (50 degrees / 0.8 m off): the trust region has to shrink through several
    consecutive REJECTED steps before the solve converges.  Every LM iteration evaluates at the candidate; a rejected
    candidate's blocks and W must be dropped (LmCtl::w_which unchanged), the diagonal reused, the radius divided --
    the trace has to follow the oracle's through the rejections, and the converged poses have to agree."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=20, n_tags=10, cam_rot_deg=50.0, cam_trans_m=0.8, tag_rot_deg=50.0, tag_trans_m=0.5)
    sc = oracle.Scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
    summ, trace = oracle.solve(sc, oracle.default_options(robustify=0, num_threads=4, linear_solver=oracle.DENSE_NORMAL))
    assert summ["num_unsuccessful_steps"] >= 3 and summ["termination_type"] == 0
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                            s.obs_px, elimination=eng.ELIM_CAMERAS if elim == "cams" else eng.ELIM_TAGS)
    try:
        out = ba.solve(eng.default_options(robustify=0), trace_capacity=128)
        cam, tag = ba.get_state()
        # the same handle again: the second solve starts from w_which = 0 whatever the first one left
        ba.set_state(s.cam_init, s.tag_init)
        out2 = ba.solve(eng.default_options(robustify=0), trace_capacity=128)
        cam2, tag2 = ba.get_state()
    finally:
        ba.close()
    assert_same_trace(out, summ, trace, rtol=1e-6)
    assert [t["step_is_successful"] for t in out["trace"]].count(0) == summ["num_unsuccessful_steps"]
    assert_same_solution(cam, tag, sc, s.tag_wh)
    assert out2["iterations"] == out["iterations"] and out2["final_cost"] == out["final_cost"]
    np.testing.assert_array_equal(cam2, cam)
    np.testing.assert_array_equal(tag2, tag)


def test_random_scenes_match_oracle(oracle):
    """Thirty small scenes of varying size, visibility, loss and distance from the optimum: termination type, iteration
    count, the accept / reject pattern and the final cost have to follow the oracle's on the twenty started near the
    optimum; the ten far starts (rejected steps, runs into the iteration limit) are pinned as far as chaos allows."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    rng = np.random.default_rng(20261004)
    n_rejecting = 0
    for case in range(30):
        n_c, n_t = int(rng.integers(4, 26)), int(rng.integers(3, 14))
        far = case % 3 == 0
        kw = dict(n_cams=n_c, n_tags=n_t, seed=int(rng.integers(1, 1 << 30)), visibility=float(rng.choice([1.0, 0.8, 0.6])))
        if far:
            kw.update(cam_rot_deg=float(rng.uniform(25, 50)), cam_trans_m=float(rng.uniform(0.3, 0.8)),
                      tag_rot_deg=float(rng.uniform(25, 50)), tag_trans_m=float(rng.uniform(0.2, 0.5)))
        s = make_scene(5 if case % 2 else 1, **kw)
        robust = case % 2
        if len(set(s.obs_cam)) < 2 or len(s.obs_cam) < 8:
            continue
        sc = oracle.Scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
        summ, trace = oracle.solve(sc, oracle.default_options(robustify=robust, num_threads=2, max_num_iterations=60))
        ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                s.obs_px, elimination=eng.ELIM_TAGS if case % 4 == 1 else eng.ELIM_AUTO)
        try:
            out = ba.solve(eng.default_options(robustify=robust, max_num_iterations=60), trace_capacity=128)
        finally:
            ba.close()
        n_rejecting += summ["num_unsuccessful_steps"] > 0
        msg = "case %d: %r" % (case, kw)
        ok_gpu = [t["step_is_successful"] for t in out["trace"]]
        ok_ref = [t["step_is_successful"] for t in trace]
        if far:
            # Starts with costs of 1e16 (corners behind cameras) are chaotic: a 1e-9 difference in iteration 8 is
            # 1e-3 in iteration 15 and a different accept / reject decision in iteration 28 (seen on case 3, both
            # paths valid).  Pinned there: the first eight iterations, and the optimum when both runs reach it.
            assert ok_gpu[:8] == ok_ref[:8], msg
            np.testing.assert_allclose([t["cost"] for t in out["trace"][:8]], [t["cost"] for t in trace[:8]], rtol=1e-6,
                                       err_msg=msg)
            if out["termination_type"] == summ["termination_type"] == eng.CONVERGENCE:
                np.testing.assert_allclose(out["final_cost"], summ["final_cost"], rtol=1e-5, err_msg=msg)
            continue
        assert out["termination_type"] == summ["termination_type"], msg
        assert out["iterations"] == summ["iterations"], msg
        assert ok_gpu == ok_ref, msg
        np.testing.assert_allclose(out["final_cost"], summ["final_cost"], rtol=1e-7, err_msg=msg)
    assert n_rejecting >= 2


def test_passes_per_graph_do_not_change_the_solve(monkeypatch):
    """The iteration graph holds VMM_BA_GRAPH_PASSES LM passes (default 2); passes recorded behind the terminating one
    find `done` set and return at once.  One, two, three passes per graph and eager launches (VMM_BA_NO_GRAPH=1) run
    the same kernels in the same order: the solves must be bit-identical, also when the pass count of the solve is
    not a multiple of the passes per graph (max_num_iterations = 4)."""
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    res = []
    for env in ({"VMM_BA_GRAPH_PASSES": "1"}, {"VMM_BA_GRAPH_PASSES": "2"}, {"VMM_BA_GRAPH_PASSES": "3"},
                {"VMM_BA_NO_GRAPH": "1"}):
        for k in ("VMM_BA_GRAPH_PASSES", "VMM_BA_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                s.obs_px)
        try:
            full = ba.solve(eng.default_options(robustify=1), trace_capacity=64)
            state = ba.get_state()
            ba.set_state(s.cam_init, s.tag_init)
            capped = ba.solve(eng.default_options(robustify=1, max_num_iterations=4), trace_capacity=64)
            state4 = ba.get_state()
        finally:
            ba.close()
        res.append((full, state, capped, state4))
    ref = res[0]
    assert ref[2]["termination_type"] == eng.NO_CONVERGENCE and ref[2]["iterations"] == 5
    for full, state, capped, state4 in res[1:]:
        for a, b in ((full, ref[0]), (capped, ref[2])):
            assert a["iterations"] == b["iterations"] and a["termination_type"] == b["termination_type"]
            assert a["final_cost"] == b["final_cost"]
            assert [t["cost"] for t in a["trace"]] == [t["cost"] for t in b["trace"]]
        np.testing.assert_array_equal(state[0], ref[1][0])
        np.testing.assert_array_equal(state[1], ref[1][1])
        np.testing.assert_array_equal(state4[0], ref[3][0])
        np.testing.assert_array_equal(state4[1], ref[3][1])
