"""A spin give-up is not an indefinite matrix.

k_chol_dataflow and k_backsolve_chain (kernels_chol_dataflow.hip, kernels_backsolve.hip in visual_marker_mapping_amd/csrc)
hand data between workgroups inside one launch with bounded spins.  A spin that gives up -- a GPU time-sliced between rank processes, a profiler
serialising workgroups -- used to raise LmCtl::lin_fail, which the trust-region policy (Ceres' HandleInvalidStep:
radius shrink, retry, FAILURE after five) takes for a failed linear solve: a scheduling event silently changed the LM
trajectory.  Now it raises LmCtl::sync_timeout, pauses the pass, and the host redoes that pass's factorisation on the
launch-per-block-column path; vmm_ba_summary reports how often and in which kernel.  The debug variables
VMM_BA_DEBUG_SPIN_LIMIT / _KERNEL / _ONCE (read at vmm_ba_create) force the give-ups here.

Reference semantics at stake: the exact linear solve inside ceres::Solve (src/TagReconstructor.cpp:737-738) -- a
recovered pass must give the same step as an undisturbed one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAR = dict(n_cams=40, n_tags=24, cam_rot_deg=50.0, cam_trans_m=0.8, tag_rot_deg=50.0, tag_trans_m=0.5)


def _solve(s, robust, elim=None):
    from visual_marker_mapping_amd import engine as eng
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                            s.obs_px, elimination=eng.ELIM_AUTO if elim is None else elim)
    try:
        out = ba.solve(eng.default_options(robustify=robust), trace_capacity=256)
        cam, tag = ba.get_state()
        again = None
        if out["num_sync_timeouts"]:
            # the handle keeps working: a second solve from the start walks the same path
            ba.set_state(s.cam_init, s.tag_init)
            again = ba.solve(eng.default_options(robustify=robust))
    finally:
        ba.close()
    return out, cam, tag, again


def _same(a, b, ca, ta, cb, tb):
    assert a["termination_type"] == b["termination_type"] and a["iterations"] == b["iterations"]
    assert a["num_unsuccessful_steps"] == b["num_unsuccessful_steps"]
    for x, y in zip(a["trace"], b["trace"]):
        assert x["step_is_valid"] == y["step_is_valid"] and x["step_is_successful"] == y["step_is_successful"]
        np.testing.assert_allclose(x["cost"], y["cost"], rtol=1e-9)
        np.testing.assert_allclose(x["trust_region_radius"], y["trust_region_radius"], rtol=1e-6)
    np.testing.assert_allclose(ca, cb, rtol=0, atol=1e-8 * np.abs(cb).max())
    np.testing.assert_allclose(ta, tb, rtol=0, atol=1e-8 * np.abs(tb).max())


@pytest.mark.parametrize("kernel,bit", [("df", 1), ("chain", 2), ("both", 1)])
@pytest.mark.parametrize("once", ["0", "1"])
@pytest.mark.parametrize("far", [False, True])
def test_forced_spin_give_ups_keep_the_trajectory(monkeypatch, kernel, bit, once, far):
    import os
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    # the suite is also run with one of the one-launch kernels switched off (VMM_BA_NO_DATAFLOW / VMM_BA_NO_CHAIN, DESIGN.md
    # section 6): a kernel that does not run cannot give up
    alive = {"df": os.environ.get("VMM_BA_NO_DATAFLOW") != "1", "chain": os.environ.get("VMM_BA_NO_CHAIN") != "1"}
    if kernel == "both":
        if not (alive["df"] or alive["chain"]):
            pytest.skip("both one-launch kernels are switched off")
        bit = 1 if alive["df"] else 2
    elif not alive[kernel]:
        pytest.skip("the %s kernel is switched off by the environment" % kernel)
    # 24 / 30 kept poses: reduced order 144 / 180 = 3 blocks, so both one-launch kernels have workgroups that wait
    s = make_scene(1, **FAR) if far else make_scene(5, n_cams=60, n_tags=30)
    robust = 0 if far else 1
    ref, cam0, tag0, _ = _solve(s, robust)
    assert ref["num_sync_timeouts"] == 0 and ref["sync_timeout_kernels"] == 0
    if far:
        assert ref["num_unsuccessful_steps"] >= 2
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_LIMIT", "1")
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_KERNEL", kernel)
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_ONCE", once)
    out, cam, tag, again = _solve(s, robust)
    assert out["termination_type"] == eng.CONVERGENCE
    assert out["num_sync_timeouts"] >= 1 and out["sync_timeout_kernels"] & bit
    if once == "1":
        assert out["num_sync_timeouts"] == 1          # the one-launch kernels are back for the rest of the solve
    else:
        assert out["num_sync_timeouts"] == out["num_lm_iterations"]   # every pass was redone
    _same(out, ref, cam, tag, cam0, tag0)
    assert again["iterations"] == ref["iterations"]
    np.testing.assert_allclose(again["final_cost"], ref["final_cost"], rtol=1e-9)


def test_give_up_and_indefinite_matrix_are_told_apart(monkeypatch):
    """vmm_ba_dense_spd_solve: with the spins forced to give up an SPD system is still solved (fallback path) and an
    indefinite one is still reported through info -- by the fallback's own pivots, not by the time-out."""
    from visual_marker_mapping_amd import engine as eng
    rng = np.random.default_rng(7)
    n = 300
    M = rng.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    b = rng.standard_normal(n)
    x_ref = np.linalg.solve(A, b)
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_LIMIT", "1")
    x, info = eng.dense_spd_solve(A, b)
    assert info == 0
    np.testing.assert_allclose(x, x_ref, rtol=0, atol=1e-10 * np.abs(x_ref).max())
    B = A.copy()
    B[200, 200] = -1.0
    _, info = eng.dense_spd_solve(B, b)
    assert info != 0


def test_covariance_survives_a_give_up(monkeypatch):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1, n_cams=60, n_tags=30)

    def cov():
        ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_gt, s.tag_gt, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px)
        try:
            return ba.tag_translation_covariance(robustify=False)
        finally:
            ba.close()
    ref = cov()
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_LIMIT", "1")
    got = cov()
    np.testing.assert_allclose(got, ref, rtol=1e-7, atol=1e-20)


def _two_clusters(s):
    """The close-up scene cut into two walls that no image sees both of: tags [0, n/2) and [n/2, n); an image keeps
    the observations of the half its first tag is in.  The co-observation graph of the tags then has (at least) two
    components -- a tree ordering gets independent roots without a separator between them."""
    import copy
    n_tags = len(s.tag_init)
    half = n_tags // 2
    first = {}
    for c, t in zip(s.obs_cam, s.obs_tag):
        first.setdefault(int(c), int(t) >= half)
    keep = np.array([(int(t) >= half) == first[int(c)] for c, t in zip(s.obs_cam, s.obs_tag)])
    t = copy.copy(s)
    t.obs_cam, t.obs_tag, t.obs_px = s.obs_cam[keep].copy(), s.obs_tag[keep].copy(), s.obs_px[keep].copy()
    return t


@pytest.mark.parametrize("order", ["nd", "natural"])
def test_give_up_of_a_single_workgroup_is_reported(monkeypatch, order):
    """ONE workgroup of the one-launch factorisation gives up (VMM_BA_DEBUG_SPIN_WG), the others only learn of it through
    the abort word -- or not at all: with a tree ordering of two walls that share no image the last block column of the
    factor does not depend on the other wall's columns, and until round 3 only that column's workgroup reported give-ups
    (ADVICE round 3).  Whichever workgroup it is: the pass is redone and the trajectory is the undisturbed one."""
    import os
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    if os.environ.get("VMM_BA_NO_DATAFLOW") == "1":   # (the forced-path runs of the whole suite)
        pytest.skip("the one-launch factorisation is switched off by the environment: no workgroup of it can give up")
    s = _two_clusters(make_scene(2, n_cams=300, n_tags=200, neighbors_min=6, neighbors_max=10))
    monkeypatch.setenv("VMM_BA_ORDER", order)
    monkeypatch.setenv("VMM_BA_SCHUR", "sparse")
    ref, cam0, tag0, _ = _solve(s, 0, eng.ELIM_CAMERAS)
    assert ref["num_sync_timeouts"] == 0
    if order == "nd":
        assert ref["tree_ordering"] >= 2
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_LIMIT", "1")
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_KERNEL", "df")
    monkeypatch.setenv("VMM_BA_DEBUG_SPIN_ONCE", "1")
    hit = 0
    for wg in range(1, 280, 12):   # block columns early and late, leaves and separators, diagonal-only workgroups
        monkeypatch.setenv("VMM_BA_DEBUG_SPIN_WG", str(wg))
        out, cam, tag, again = _solve(s, 0, eng.ELIM_CAMERAS)
        assert out["num_sync_timeouts"] in (0, 1)      # a workgroup without anything to wait for cannot give up
        hit += out["num_sync_timeouts"]
        if out["num_sync_timeouts"]:
            assert out["sync_timeout_kernels"] & 1
        _same(out, ref, cam, tag, cam0, tag0)
    assert hit >= 4, "hardly any of the chosen workgroups had to wait: the test checks nothing"
