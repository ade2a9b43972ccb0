"""The yardsticks of the GPU accuracy tests, checked without a GPU (helpers: tests/linalg_cases.py).

The GPU tests hold the kernels to 8 x the error of two f64 CPU references on the same system.  That margin means
something only if the generator delivers the conditioning it names, the two references are samples of ONE error class,
and the numpy restatement of an LM step is the step the oracle takes.
"""
import numpy as np
import pytest

import linalg_cases as lc

if np.finfo(np.longdouble).eps >= 1e-18:
    pytest.skip("np.longdouble is no wider than f64 here", allow_module_level=True)


@pytest.mark.parametrize("n", [65, 333])
@pytest.mark.parametrize("kappa", lc.KAPPAS)
def test_generator_delivers_unit_diagonal_and_the_condition_number(n, kappa):
    for seed in (0, 1):
        A = lc.spd_unit_diagonal(n, kappa, seed)
        assert A.shape == (n, n) and A.dtype == np.float64
        np.testing.assert_array_equal(np.diag(A), np.ones(n))
        np.testing.assert_array_equal(A, A.T)
        cond = np.linalg.cond(A)
        print("n %d kappa %.0e seed %d: cond / kappa = %.3f" % (n, kappa, seed, cond / kappa))
        assert kappa / 2 <= cond <= 2 * kappa
        assert lc.spd_unit_diagonal(n, kappa, seed) is A     # built once


def _gpu_cases_up_to_1408():
    cases = set(lc.PATH_CASES) | {(n, k) for _, n, k in lc.FALLBACK_CASES} | set(lc.SCALING_CASES)
    cases |= {(n, lc.BOUNDARY_KAPPA) for n in lc.BOUNDARY_ORDERS} | {(700, 1e4)}
    return sorted(c for c in cases if c[0] <= 1408)


@pytest.mark.parametrize("n,kappa", _gpu_cases_up_to_1408())
def test_the_two_references_are_one_error_class(n, kappa):
    """Backward errors within a factor of 8 of one another (measured: up to ~5), both at the level of f64 roundoff
    whatever the condition number; the forward error is what the condition number makes of it."""
    c = lc.case_bounds(n, kappa, 0)
    be = [r["backward"] for r in c["refs"].values()]
    print("n %d kappa %.0e: backward %.2e %.2e, forward %.2e %.2e" % ((n, kappa) + tuple(be) + tuple(
        r["forward"] for r in c["refs"].values())))
    assert max(be) <= 8 * min(be)
    assert max(be) <= 4 * lc.U64 * max(1.0, np.sqrt(n) / 8)     # backward stable: a small multiple of u
    assert c["bound"] == max(be) and c["forward_bound"] <= 100 * kappa * lc.U64
    # the refined solution is converged: its own backward error is far below any f64 solve's
    assert lc.backward_error(c["A"], c["b"], c["x_ref"], c["norm_A"], c["A_ld"]) <= 1e-3 * max(c["bound"], lc.U64)
    if n <= 129:
        assert lc.reference_bound(c["A"], c["b"]) == pytest.approx(c["bound"], rel=1e-3)


def test_blocked_model_handles_a_ragged_last_block_and_other_block_sizes():
    c = lc.case_bounds(333, 1e8, 0)
    for nb in (8, 64, 100, 333, 500):
        x = lc.blocked_explicit_inverse_solve(c["A"], c["b"], nb=nb)
        assert lc.backward_error(c["A"], c["b"], x, c["norm_A"], c["A_ld"]) <= 8 * c["bound"]


def test_syrk_bound_holds_for_numpy_products():
    """The derived bound gamma_k |Z|^T |Z| admits every f64 summation order: numpy's (BLAS) and a plain loop's."""
    Z, e = lc.scaled_columns(37, 65, 3)
    exact, bound = lc.syrk_exact(Z), lc.syrk_bound(Z)
    assert np.all(np.abs(exact - lc.syrk_exact_plain(Z)) <= 2.0 ** -10 * bound)     # the sliced product is the plain one
    assert np.all(np.abs((Z.T @ Z).astype(lc.LD) - exact) <= bound)
    loop = np.zeros((65, 65))
    for r in Z:
        loop += np.outer(r, r)
    assert np.all(np.abs(loop.astype(lc.LD) - exact) <= bound)
    assert exact.max() / np.abs(exact)[np.abs(exact) > 0].min() > 2.0 ** 60     # small entries beside large ones
    Zc, zero = lc.cancelling_rows(100, 33, 4)
    exact = lc.syrk_exact(Zc, zero)
    assert zero.any() and exact[~zero].all()
    assert np.all(np.abs(lc.syrk_exact(Zc)[zero]) <= 2.0 ** -10 * lc.syrk_bound(Zc)[zero])   # longdouble's own rounding
    assert np.all(np.abs((Zc.T @ Zc).astype(lc.LD) - exact) <= lc.syrk_bound(Zc))


def test_numpy_plus_matches_the_kats(kats):
    qt = np.array([c["qt"] for c in kats["plus"]])
    delta = np.array([c["delta"] for c in kats["plus"]])
    ref = np.array([c["out"] for c in kats["plus"]])
    np.testing.assert_allclose(lc.pose_plus(qt, delta), ref, rtol=0, atol=lc.PLUS_ATOL)
    np.testing.assert_allclose(lc.pose_plus(qt, delta.astype(lc.LD)).astype(np.float64), ref, rtol=0, atol=lc.PLUS_ATOL)
    np.testing.assert_array_equal(lc.pose_plus(qt, np.zeros_like(delta)), qt)


@pytest.mark.parametrize("radius", [1e4, 1e12])
@pytest.mark.parametrize("robust", [0, 1])
@pytest.mark.parametrize("solver", ["DENSE_NORMAL", "SCHUR_ELIM_CAMS", "SCHUR_ELIM_TAGS"])
def test_numpy_lm_step_is_the_oracles_first_iteration(oracle, solver, robust, radius):
    """One iteration of oracle.solve on config 1 against the longdouble restatement, to the bound of
    test_gpu_lm_step.py: 8 x the deviation of the two f64 numpy solves of the same step."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    blk = lc.blocks_from_oracle(oracle, s, s.cam_init, s.tag_init, robust, s.fixed_tag)
    tag_const = np.arange(len(s.tag_init)) == s.fixed_tag
    prob = lc.LmProblem(blk, s.obs_cam, s.obs_tag, s.cam_init, s.tag_init, None, tag_const)
    three = lc.lm_step_reference(prob, radius, "tags" if solver == "SCHUR_ELIM_TAGS" else "cams")
    bound = lc.lm_bounds(three)
    sc = oracle.Scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
    summ, trace = oracle.solve(sc, oracle.default_options(robustify=robust, max_num_iterations=1,
                                                          initial_trust_region_radius=radius,
                                                          linear_solver=getattr(oracle, solver)))
    assert summ["iterations"] == 2 and trace[1]["step_is_valid"] == 1 and trace[1]["step_is_successful"] == 1
    got = dict(cam=sc.cam_qt, tag=sc.tag_qt, gradient_max_norm=trace[0]["gradient_max_norm"],
               model_cost_change=trace[1]["model_cost_change"], step_norm=trace[1]["step_norm"])
    dev = lc.lm_deviation(got, three["ref"])
    for k in sorted(dev):
        print("%s robust %d radius %.0e: %s deviation %.3e, bound %.3e" % (solver, robust, radius, k, dev[k], bound[k]))
    assert abs(trace[0]["cost"] - blk["cost"]) <= 1e-13 * blk["cost"]
    assert dev["state"] <= bound["state"]
    np.testing.assert_array_equal(sc.tag_qt[s.fixed_tag], s.tag_init[s.fixed_tag])
    for k in lc.LM_SCALARS:
        assert dev[k] <= bound[k], k
