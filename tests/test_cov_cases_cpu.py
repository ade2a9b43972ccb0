"""CPU-only checks of tests/cov_cases.py, the yardstick of tests/test_gpu_cov_accuracy.py, proven here before the GPU tests
lean on it: every scene's H is positive definite, the longdouble inverse has converged (its last Newton correction is at
most 1/64 of the smaller reference deviation), the eliminated form equals the plain full-matrix refined inverse, references
A and B both land within 1e-9 of it (a sanity cap, not the GPU tests' bound), and the longdouble camera-model Jacobian and
reduced system agree with the oracle's.  The blocks come from eval_cases.assemble in float64 here, from the handle's
eval_blocks on the GPU.
"""
import numpy as np
import pytest

import cov_cases as cc

CASES = [(name, elim) for name, elims in cc.SCENES.items() for elim in elims]


@pytest.mark.parametrize("name,elim", CASES)
def test_scene_is_positive_definite_and_the_references_are_sound(name, elim):
    case = cc.cpu_case(name, elim)
    lo, hi = min(case.refs.values()), max(case.refs.values())
    Hs = case.H * np.outer(cc.pow2_scale(np.diag(case.H)), cc.pow2_scale(np.diag(case.H)))
    print("%s elim %s: order %d, smallest eigenvalue %.3e, condition %.2e plain / %.2e scaled; references %s; last "
          "correction %.3e" % (name, elim, case.order, case.min_eig, np.linalg.cond(case.H), np.linalg.cond(Hs),
                               {k: "%.3e" % v for k, v in case.refs.items()}, case.last_correction))
    assert case.min_eig > 0
    assert case.last_correction <= cc.REFINEMENT_SHARE * lo
    assert 0 < lo and hi <= cc.REFERENCE_CAP
    assert case.truth.dtype == cc.LD and np.array_equal(case.truth, case.truth.T)


def test_scene_shapes_are_the_ones_the_gpu_tests_count_on():
    s = cc.scene("24x12")
    assert (len(s.cam_qt), len(s.tag_qt)) == (24, 12)
    assert cc.cpu_case("24x12", "tags").order == 6 * 35      # the origin tag is outside
    weak = cc.scene("24x12_weak")
    on = weak.mask != 0
    assert np.sum(on & (weak.obs_tag == 11)) == 1 and np.sum(on & (weak.obs_cam == 23)) == 1
    sparse = cc.scene("24x12_sparse_view")
    assert min(np.bincount(sparse.obs_cam, minlength=24).min(), np.bincount(sparse.obs_tag, minlength=12).min()) >= 2
    assert 6 * len(cc.scene("44x10").cam_qt) > 256 and 6 * len(cc.scene("10x44").tag_qt) > 256
    for name, n_free in (("ragged_tags", 130 + 6 - 3), ("ragged_cams", 130 + 6 - 4)):
        case = cc.cpu_case(name, "cams")
        assert case.order == 6 * n_free, name      # pose 129 of the 130, the two constants (and the fixed tag) are outside
        many_first = case.n_cams if name == "ragged_cams" else 0
        assert not case.free(many_first + 129) and not case.free(many_first + 2)


def test_eliminated_form_equals_the_full_refined_inverse():
    case = cc.cpu_case("20x10", "cams")
    full, corr = cc.refined_inverse(case.H)
    gap = cc.entry_deviation(full, case.truth)
    print("20x10: eliminated form against the full refined inverse %.3e; references %s" % (gap, case.refs))
    assert gap <= cc.REFINEMENT_SHARE * min(case.refs.values())
    assert cc.entry_deviation(full + corr, full) <= cc.REFINEMENT_SHARE * min(case.refs.values())
    # and it is an inverse: H X = I to longdouble rounding
    assert np.abs(case.H.astype(cc.LD) @ case.truth - np.eye(case.order)).max() <= 1e-14


def test_the_metric_is_invariant_to_units():
    case = cc.cpu_case("20x10", "cams")
    d = np.ldexp(1.0, np.random.default_rng(3).integers(-20, 21, case.order))
    got = np.linalg.inv(case.H)
    a = cc.entry_deviation(got, case.truth)
    b = cc.entry_deviation(d[:, None] * got * d[None, :], d[:, None] * case.truth * d[None, :])
    assert a == b


def test_a_single_precision_intermediate_misses_the_bound():
    """What the bound is for: reference B with Z rounded to float32 deviates by far more than 8 x the references."""
    case = cc.cpu_case("24x12", "tags")
    H = case.H
    n_front = 6 * sum(1 for p in case.pos if p < case.n_cams)
    e, f = np.arange(n_front, case.order), np.arange(n_front)
    Hf = H.copy()
    Hf[np.ix_(e, f)] = H[np.ix_(e, f)].astype(np.float32)
    Hf[np.ix_(f, e)] = Hf[np.ix_(e, f)].T
    dev = cc.entry_deviation(cc.device_model(Hf, n_front, False), case.truth)
    print("coupling blocks in float32: deviation %.3e, bound %.3e" % (dev, case.bound))
    assert dev > 1e3 * case.bound


# ---- the camera-model system ---------------------------------------------------------------------------------------------

def test_model_columns_match_the_oracle(oracle):
    """The longdouble J_k against yardstick.joint_system's (yardstick.intrinsic_columns, float64) on the
    ragged scene, entry by entry over the entry's magnitude (the same formulas over absolute values).  An entry is a product
    of at most nine factors, each the result of a chain of under ten roundings (quaternion norm, rotation entry, two
    three-term sums, the division, r2 and its powers): 64 units of float64 roundoff bound it with room; a wrong column or
    power misses by the entry itself."""
    from yardstick import joint_system
    sc = cc.scene("ragged_tags")
    k = np.concatenate([sc.intr, sc.dist])
    n = 130
    oc, ot, px = sc.obs_cam[:n], sc.obs_tag[:n], sc.obs_px[:n]
    _, _, J = joint_system(oracle, k, sc.cam_qt, sc.tag_qt, sc.tag_wh, sc.fixed_tag, oc, ot, px, robust=False)
    Jk, mag = cc.model_columns(sc.intr, sc.dist, sc.cam_qt[oc], sc.tag_qt[ot], sc.tag_wh[ot], want_magnitude=True)
    got = J[:, -9:].reshape(n, 4, 2, 9)
    live = mag > 0
    assert not got[~live].any() and not Jk[~live].any()
    dev = float(np.max(np.abs(got.astype(cc.LD) - Jk)[live] / mag[live]))
    print("J_k: oracle against longdouble, worst |difference| / magnitude %.3e (bound %.3e)" % (dev, 64 * cc.U64))
    assert dev <= 64 * cc.U64
    assert np.all(np.abs(Jk) <= mag * (1 + 1e-15))


@pytest.mark.parametrize("variant", [v[0] for v in cc.MODEL_VARIANTS])
@pytest.mark.parametrize("name", ["ragged_tags", "ragged_cams"])
def test_model_system_references_are_sound(oracle, name, variant):
    case = cc.model_case(oracle, name, variant)
    print("%s %s: sigma %s; step of %.3g sigma; references (inv(S_k), step) %s" % (
        name, variant, np.array2string(case.sigma.astype(np.float64), precision=3),
        float(np.max(np.abs(case.step) / case.sigma)), {k: "%.3e %.3e" % v for k, v in case.refs.items()}))
    assert np.all(np.linalg.eigvalsh(case.Sk.astype(np.float64)) > 0)
    for dev_cov, dev_step in case.refs.values():
        assert 0 < dev_cov <= cc.REFERENCE_CAP and 0 < dev_step <= cc.REFERENCE_CAP
    # the oracle's C and g_k against the longdouble sums, in test_gpu_selfcal.py's metric and at its bounds
    from yardstick import BOUND_C, BOUND_COST, BOUND_G
    A, B, g, C, gk, cost = cc.border_sums(case.scene, case.k, case.robust, case.mask, cc.LD)
    o = case.oracle
    live = o["mag_C"] > 0
    assert not o["C"][~live].any() and not C[~live].any()
    assert float(np.max(np.abs(o["C"] - C)[live] / o["mag_C"][live])) <= BOUND_C
    assert float(np.max(np.abs(o["g_k"] - gk) / o["mag_g"])) <= BOUND_G
    assert abs(o["cost"] - cost) <= BOUND_COST * o["cost"]
