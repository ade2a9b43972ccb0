"""The evaluation kernels (k_eval_both, k_eval_fused, k_reduce_pose, the cost kernel, k_stats) entry by entry: Huber widths
other than 1, task and workgroup edges, hard geometry, f32 accumulation, and the width through the other entry points.

The bound.  For every array the device's deviation from the longdouble reference (tests/eval_cases.py: per entry,
relative to the entry's magnitude = the same sum over absolute values) may be at most 8 x the larger deviation of two CPU
references on the same case and array: A, the oracle's functor summed in numpy, and B, a plain float64 restatement.
Entries of magnitude 0 must be exactly 0.  The references set the bound, never the code under test; every test prints
deviation, bound and ratio (tools/eval_accuracy.py records them, DESIGN.md section 4.13 holds the measured ones).
"""

import numpy as np
import pytest

import eval_cases as ec
import yardstick as ys

pytestmark = pytest.mark.gpu

BLOCKS = ("V", "U", "W", "g_cam", "g_tag")


@pytest.fixture(scope="module")
def eng():
    from visual_marker_mapping_amd import engine
    return engine


def run_blocks(eng, setenv, s, elim="cams", mode="twopass", group=None, robust=True, a=1.0, mask=None, consts=None,
               precision=None):
    """eval_blocks twice and cost() on a fresh handle of scene s.  setenv(name, value or None) sets the switches that the
    handle reads when it is created.  Returns (blocks, blocks of the second call, cost())."""
    setenv("VMM_BA_EVAL", mode)
    setenv("VMM_BA_FUSED_GROUP", None if group is None else str(group))
    kw = {} if precision is None else {"precision": precision}
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_qt, s.tag_qt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px,
                            elimination=eng.ELIM_CAMERAS if elim == "cams" else eng.ELIM_TAGS, **kw)
    try:
        if mask is not None:
            ba.set_observation_mask(mask)
        if consts is not None:
            ba.set_constant_poses(*consts)
        b = ba.eval_blocks(robustify=robust, huber_a=a)
        b2 = ba.eval_blocks(robustify=robust, huber_a=a)
        c = ba.cost(robustify=robust, huber_a=a)
    finally:
        ba.close()
    return b, b2, c


def _setenv(monkeypatch):
    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return setenv


def _same_bits(b, b2):
    return all(np.array_equal(b[k], b2[k]) for k in BLOCKS) and b["cost"] == b2["cost"]


def _check_all(case, results, bound=None):
    """results: {label: (blocks, second call, cost())}.  Every array within the bound, zero where the magnitude is zero,
    the second call bit-equal, cost() within the bound of the cost."""
    bad = []
    for label, (b, b2, c) in results.items():
        bad += case.check(b, label, bound)
        dev = ec.deviation(dict(b, cost=c), case.ref, case.mag)["cost"][0]
        lim = (bound or case.bound)["cost"]
        print("%s cost() deviation %.3e  bound %.3e  ratio %.3f; bit-equal to eval_blocks()['cost']: %s"
              % (label, dev, lim, dev / lim if lim else float(dev > 0), c == b["cost"]))
        if not dev <= lim:
            bad.append("%s cost(): deviation %.3e above the bound %.3e" % (label, dev, lim))
        if not _same_bits(b, b2):
            bad.append("%s: the second call gives other bits" % label)
    assert not bad, "\n".join(bad)


def _check_fused_equals_twopass(case, results, twopass, fused_labels, bound=None):
    bad = []
    for label in fused_labels:
        dev = ec.deviation(results[label][0], results[twopass][0], case.mag)
        for k, (d, zeros_ok) in dev.items():
            lim = (bound or case.bound)[k]
            print("%s against %s %-5s deviation %.3e  bound %.3e" % (label, twopass, k, d, lim))
            if not (d <= lim and zeros_ok):
                bad.append("%s against %s %s: %.3e above %.3e" % (label, twopass, k, d, lim))
    assert not bad, "\n".join(bad)


# ---- per-entry blocks at three widths ---------------------------------------------------------------------------------

def mixed_case(O, a, robust, f32=False):
    return ec.cached(("case", "mixed", float(a), bool(robust)) + (("f32",) if f32 else ()),
                     lambda: ec.Case(O, ec.mixed_scene(a), a=a, robust=robust, f32=f32))


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("a", [0.5, 1.0, 2.5])
def test_blocks_entry_by_entry_at_three_widths(eng, oracle, monkeypatch, a, robust):
    """Half of the corners of mixed_scene(a) lie on either side of s = a^2, so a misplaced `a` in any of huber()'s three
    places moves half of the weights."""
    case = mixed_case(oracle, a, robust)
    results = {}
    for elim in ("cams", "tags"):
        for mode in ("twopass", "fused"):
            results["a=%g robust=%d %s %s" % (a, robust, elim, mode)] = run_blocks(
                eng, _setenv(monkeypatch), case.scene, elim, mode, robust=robust, a=a)
    _check_all(case, results)


# ---- task and workgroup edges -----------------------------------------------------------------------------------------

def ragged_case(O, few, masked, const, f32=False):
    def make():
        s = ec.ragged_scene(few)
        cc, tc = ec.ragged_constants(s) if const else (None, None)
        return ec.Case(O, s, mask=ec.ragged_mask(s) if masked else None, cam_const=cc, tag_const=tc, f32=f32)
    return ec.cached(("case", "ragged", few, bool(masked), bool(const)) + (("f32",) if f32 else ()), make)


RAGGED_MODES = (("twopass", None), ("fused", 1), ("fused", 4), ("fused", 7))


def ragged_results(eng, setenv, case, elim, precision=None):
    consts = None if case.cam_const is None else (case.cam_const, case.tag_const)
    return {"%s %s%s" % (elim, mode, "" if group is None else " group %d" % group):
            run_blocks(eng, setenv, case.scene, elim, mode, group, mask=case.mask, consts=consts, precision=precision)
            for mode, group in RAGGED_MODES}


@pytest.mark.parametrize("const", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("elim", ["cams", "tags"])
@pytest.mark.parametrize("few", ["tags", "cams"])
def test_task_edges(eng, oracle, monkeypatch, few, elim, masked, const):
    """Poses with exactly 1, 63, 64, 65, 128 and 129 observations (a wave takes 64), task counts of 10 and 129 (four to a
    workgroup), a pose without observations, 130 kept poses (chunks of 64) and 129 or 6 eliminated ones in groups of 1, 4
    and 7; optionally every 7th observation and lane 0 of a second task masked, one camera and one more tag constant."""
    case = ragged_case(oracle, few, masked, const)
    results = ragged_results(eng, _setenv(monkeypatch), case, elim)
    _check_all(case, results)
    labels = list(results)
    _check_fused_equals_twopass(case, results, labels[0], labels[1:])


# ---- hard geometry ----------------------------------------------------------------------------------------------------

def record_case(O, kats, section, i, robust):
    return ec.cached(("case", section, i, bool(robust)),
                     lambda: ec.Case(O, ec.single_record_scene(kats[section][i]), robust=robust))


def _robust_settings(case):
    what = case.get("what", "")
    return (False, True) if what.startswith(("tag behind", "observation 1e5")) else (False,)


@pytest.mark.parametrize("i", range(16))
def test_hard_records_alone(eng, oracle, kats, monkeypatch, i):
    """One camera, one tag, one observation, as test_gpu_kernels.test_residual_and_jacobian_kats_through_the_engine, but
    entry by entry; the record behind the camera and the one 1e5 px off also with the loss on."""
    rec = kats["obs_hard"][i]
    for robust in _robust_settings(rec):
        case = record_case(oracle, kats, "obs_hard", i, robust)
        _check_all(case, {"%s robust=%d" % (rec["what"], robust):
                          run_blocks(eng, _setenv(monkeypatch), case.scene, robust=robust)})


def hard_batch_case(O, kats, strong, robust):
    return ec.cached(("case", "hard", bool(strong), bool(robust)),
                     lambda: ec.Case(O, ec.hard_batch(strong, kats), robust=robust))


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("strong", [False, True])
def test_hard_batch(eng, oracle, kats, monkeypatch, strong, robust):
    """The hard records in lanes 0 and 63 of a camera's first task and lane 0 of its second, ordinary tags between."""
    case = hard_batch_case(oracle, kats, strong, robust)
    results = {}
    for elim in ("cams", "tags"):
        for mode in ("twopass", "fused"):
            results["hard batch strong=%d robust=%d %s %s" % (strong, robust, elim, mode)] = run_blocks(
                eng, _setenv(monkeypatch), case.scene, elim, mode, robust=robust)
    _check_all(case, results)


# ---- f32 accumulation -------------------------------------------------------------------------------------------------

def f32_cases(O):
    yield "mixed a=1", mixed_case(O, 1.0, True, f32=True)
    for few in ("tags", "cams"):
        yield "ragged %s" % few, ragged_case(O, few, False, False, f32=True)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_f32_accumulation(eng, oracle, monkeypatch, which):
    """VMM_BA_PRECISION_F32_ACCUM: V, U and W within 8 x the deviation of reference F (f64 Jacobians, products and sums in
    float32); the gradients and the cost meet the f64 bound unchanged, as the kernel's header says they are always f64."""
    label, case = list(f32_cases(oracle))[which]
    results = {}
    for elim in ("cams", "tags"):
        for mode, group in (("twopass", None), ("fused", 7)):
            b, b2, c = run_blocks(eng, _setenv(monkeypatch), case.scene, elim, mode, group, a=case.a,
                                  precision=eng.PRECISION_F32_ACCUM)
            results["f32 %s %s %s" % (label, elim, mode)] = (b, b2, c)
    _check_all(case, results, case.bound_f32)


# ---- the width through the other entry points -------------------------------------------------------------------------

@pytest.mark.parametrize("a", [0.5, 2.5])
def test_solve_with_another_width_matches_the_oracle(eng, oracle, a):
    import test_gpu_solve as ts
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=30, n_tags=12)
    out, cam, tag, summ, trace, sc = ts._run_both(eng, oracle, s, "auto", robustify=1, huber_a=a)
    print("huber_a %g: %d iterations, final cost device %.12g oracle %.12g" % (a, out["iterations"], out["final_cost"],
                                                                            summ["final_cost"]))
    ys.assert_same_trace(out, summ, trace)
    ys.assert_same_solution(cam, tag, sc, s.tag_wh)


@pytest.mark.parametrize("first,second", [(1.0, 2.5), (2.5, 1.0)])
def test_a_second_solve_with_another_width_has_the_bits_of_a_fresh_handle(eng, first, second):
    """vmm_ba_solve captures its iteration graph with the width in the kernels' arguments and captures again when the
    width changes: a handle that has solved with one width, put back to the start, gives the bits of a fresh one."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=30, n_tags=12)

    def handle():
        return eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                                  s.obs_px)
    with handle() as ba:
        o1 = ba.solve(eng.default_options(robustify=1, huber_a=first), trace_capacity=64)
        ba.set_state(s.cam_init, s.tag_init)
        o2 = ba.solve(eng.default_options(robustify=1, huber_a=second), trace_capacity=64)
        cam2, tag2 = ba.get_state()
    with handle() as ba:
        of = ba.solve(eng.default_options(robustify=1, huber_a=second), trace_capacity=64)
        camf, tagf = ba.get_state()
    print("width %g then %g: final costs %.15g then %.15g; fresh handle %.15g" % (first, second, o1["final_cost"],
                                                                              o2["final_cost"], of["final_cost"]))
    assert o1["final_cost"] != o2["final_cost"]      # the widths do differ on this scene
    assert o2["iterations"] == of["iterations"] and o2["final_cost"] == of["final_cost"]
    assert [t["cost"] for t in o2["trace"]] == [t["cost"] for t in of["trace"]]
    np.testing.assert_array_equal(cam2, camf)
    np.testing.assert_array_equal(tag2, tagf)


def _inverse_longdouble(H):
    """inv(H) to longdouble accuracy: the float64 inverse, then Newton steps X <- X + X (I - H X) in longdouble."""
    H = np.asarray(H, ec.LD)
    X = np.linalg.inv(H.astype(np.float64)).astype(ec.LD)
    for _ in range(3):
        X = X + X @ (np.eye(len(H), dtype=ec.LD) - H @ X)
    return X


def test_covariance_with_another_width_matches_the_inverse_normal_matrix(eng, oracle):
    """covariance_blocks(robustify=True, huber_a=2.5) against the inverse of the longdouble normal matrix of
    mixed_scene(2.5), at the tolerance of test_gpu_pose_covariance.py (1e-6 of the geometric mean of the two marginals'
    largest entries)."""
    a = 2.5
    case = mixed_case(oracle, a, True)
    s = case.scene
    n_c, n_t = len(s.cam_qt), len(s.tag_qt)
    free = [p for p in range(n_c + n_t) if p != n_c + s.fixed_tag]
    H = np.zeros((6 * (n_c + n_t), 6 * (n_c + n_t)), ec.LD)
    for c in range(n_c):
        H[6 * c:6 * c + 6, 6 * c:6 * c + 6] = case.ref["V"][c]
    for t in range(n_t):
        H[6 * (n_c + t):6 * (n_c + t) + 6, 6 * (n_c + t):6 * (n_c + t) + 6] = case.ref["U"][t]
    for i, (c, t) in enumerate(zip(s.obs_cam, s.obs_tag)):
        H[6 * c:6 * c + 6, 6 * (n_c + t):6 * (n_c + t) + 6] += case.ref["W"][i]
        H[6 * (n_c + t):6 * (n_c + t) + 6, 6 * c:6 * c + 6] += case.ref["W"][i].T
    idx = np.concatenate([np.arange(6 * p, 6 * p + 6) for p in free])
    inv = np.zeros_like(H)
    inv[np.ix_(idx, idx)] = _inverse_longdouble(H[np.ix_(idx, idx)])
    n = n_c + n_t
    pairs = np.array([(p, p) for p in range(n)] + [(0, n_c + 1), (n_c + 2, 3), (1, 2), (n_c + 1, n_c + 3),
                                                   (0, n_c + s.fixed_tag)], np.int32)
    with eng.BundleAdjuster(s.intr, s.dist, s.cam_qt, s.tag_qt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        cov = ba.covariance_blocks(pairs, robustify=True, huber_a=a)
        cov1 = ba.covariance_blocks(pairs, robustify=True, huber_a=1.0)
    worst = 0.0
    for (p, q), got in zip(pairs.tolist(), cov):
        ref = inv[6 * p:6 * p + 6, 6 * q:6 * q + 6].astype(np.float64)
        if p not in free or q not in free:
            assert not got.any(), (p, q)
            continue
        scale = np.sqrt(np.abs(inv[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() * np.abs(inv[6 * q:6 * q + 6, 6 * q:6 * q + 6]).max())
        err = float(np.abs(got - ref).max() / scale)
        worst = max(worst, err)
        assert err <= 1e-6, (p, q, err)
    moved = float(np.abs(cov - cov1).max() / np.abs(cov).max())
    print("huber_a 2.5: %d blocks, worst |device - longdouble inverse| / scale %.3g; the width 1 moves the blocks by %.3g of "
          "their largest entry" % (len(pairs), worst, moved))
    assert moved > 1e-3      # half of the corners lie between the two thresholds: the two widths are not the same matrix


def test_localize_with_another_width_reaches_the_host_optimum(eng, oracle, monkeypatch):
    """engine.localize(huber_a=0.5) against yardstick.image_optimum run with the same width, at its
    tolerance (1e-6 per pose).  make_scene(1) has 0.3 px of noise: a quarter of the corners have |r| > 0.5 px."""
    import test_gpu_localize as tl
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import make_scene
    a = 0.5
    s = make_scene(1)
    assert s.noise_px == 0.3
    start, tag, px, _ = tl._csr(s)
    cam, cov, inl, res = tl._localize(eng, s, start, tag, px, robustify=1, huber_a=a)
    cam1, _, _, _ = tl._localize(eng, s, start, tag, px, robustify=1)
    assert [r["status"] for r in res] == [_lib.LOC_OK] * len(cam)
    tl._assert_clean(cam, cov, res)
    worst = tl._check_against_host(oracle, s, start, tag, px, cam, inl, res, range(len(cam)), True, "huber_a=%g" % a, a=a)
    gap = ys.pose_gap(cam, cam1)
    print("huber_a %g: worst |dq| %.3g |dt| %.3g against the host; the default width lands |dq| %.3g |dt| %.3g away"
          % (a, worst[0], worst[1], gap[0], gap[1]))
    assert max(gap) > 1e-5      # ten times the tolerance: the comparison above can tell the two widths apart


def test_calibrate_with_another_width_reaches_the_host_optimum(eng, oracle):
    """engine.calibrate(huber_a=0.5) against yardstick.host_calibration(a=0.5) at the tolerances of
    test_gpu_calibrate.py."""
    import test_gpu_calibrate as tc
    from visual_marker_mapping_amd import _lib
    from visual_marker_mapping_amd.synthetic import make_scene
    a = 0.5
    s = make_scene(1)
    assert s.noise_px == 0.3
    start, img, tag, px = tc._csr(s)
    d = tc._calibrate(s, tc._truth(s) + ys.PERTURB, start, tag, px, robustify=1, huber_a=a, loc_huber_a=a,
                      reclassify_passes=0, **tc.WIDE)
    tc._assert_clean(d)
    assert d["report"]["status"] == _lib.CAL_OK and d["inl"].all()
    ref = ys.host_calibration(oracle, tc._truth(s), s.cam_gt, s.tag_gt, s.tag_wh, img, tag, px, robust=True, a=a)
    tc._check_against_host(oracle, s, d, ref, np.arange(len(s.cam_gt)), "huber_a=%g" % a)
    ref1 = ys.host_calibration(oracle, tc._truth(s), s.cam_gt, s.tag_gt, s.tag_wh, img, tag, px, robust=True)
    icov, _ = ys.calibration_covariance(ref[3], len(ref[1]), 0x1FF)
    apart = np.abs(ref[0] - ref1[0]) / np.sqrt(np.diag(icov))
    print("host optima at width %g and at width 1 are %s sigma apart" % (a, np.array2string(apart, precision=3)))
    assert (apart > 10 * ys.SIGMA_GAP).all()      # the comparison above can tell the two widths apart


def test_initialize_then_solves_with_another_width_lead_to_the_same_optimum(eng, monkeypatch):
    """vmm_ba_initialize itself takes no width (vmm_ba_init_options holds none); the width enters through the solves that
    follow it.  test_gpu_init.test_initialize_leads_to_the_same_optimum on config1_20x10 with the robust solve at
    huber_a = 0.3 (the noise is 0.3 px: 60 % of the corners are beyond it)."""
    import test_gpu_init as ti
    from visual_marker_mapping_amd.synthetic import make_scene

    def two_solves(eng_, ba):
        a = ba.solve(eng_.default_options(robustify=1, huber_a=0.3, max_num_iterations=1500))
        b = ba.solve(eng_.default_options(robustify=0, max_num_iterations=1500, function_tolerance=1e-14,
                                          parameter_tolerance=1e-12))
        return a, b
    monkeypatch.setattr(ti, "_two_solves", two_solves)
    cfg, kw = ti.SCENES["config1_20x10"]
    s = make_scene(cfg, **kw)
    report, cam_ok, tag_ok, _, _ = ti._same_optimum(eng, s, "config1_20x10 huber_a=0.3")
    assert cam_ok.all() and tag_ok.all()
    assert report["cams_reached"] == len(s.cam_gt) and report["tags_reached"] == len(s.tag_gt)


# ---- the statistics path off the unit sphere --------------------------------------------------------------------------

def test_reprojection_statistics_with_quaternions_off_the_unit_sphere(eng, oracle):
    """k_stats rotates like Eigen::Quaterniond::toRotationMatrix, which does not normalise: cameras at |q| = 1.3, tags at
    0.8, against the oracle at the tolerances of test_gpu_kernels.test_reprojection_statistics_match_oracle."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(5, n_cams=7, n_tags=5)
    cam, tag = s.cam_init.copy(), s.tag_init.copy()
    cam[:, :4] *= 1.3
    tag[:, :4] *= 0.8
    sc = oracle.Scene(s.intr, s.dist, cam, tag, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px)
    pc, pt, avg, corner = oracle.reprojection_stats(sc)
    with eng.BundleAdjuster(s.intr, s.dist, cam, tag, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        gc, gt, gavg, gcorner = ba.reprojection_stats()
    unit = oracle.reprojection_stats(oracle.Scene(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, 0, s.obs_cam,
                                                  s.obs_tag, s.obs_px))[3]
    moved = np.abs(corner - unit).max(axis=1)
    print("average error %.6g px; the norms move every observation's corners by %.3g .. %.3g px; worst |device - oracle| "
          "per corner %.3g px" % (avg, moved.min(), moved.max(), np.abs(gcorner - corner).max()))
    assert moved.min() > 1.0      # the norms matter on this path: a kernel that normalised would be off by pixels
    np.testing.assert_allclose(gcorner, corner, rtol=0, atol=1e-9)
    np.testing.assert_allclose(gc, pc, rtol=1e-12)
    np.testing.assert_allclose(gt, pt, rtol=1e-12)
    assert abs(gavg - avg) <= 1e-12 * avg


def test_per_corner_statistics_match_the_known_answers(eng, kats):
    """reprojection_error_camera_model of the `obs` cases 4 and 5 (|q| = 1.7 and 0.6) and of every `obs_hard` record, to
    1e-9 of |proj| + |obs| per coordinate."""
    worst = 0.0
    for label, case in [("obs %d" % i, kats["obs"][i]) for i in (4, 5)] + [(c["what"], c) for c in kats["obs_hard"]]:
        with eng.BundleAdjuster(case["intr"], case["dist"], [case["cam_qt"]], [case["tag_qt"]], [case["wh"]], -1, [0], [0],
                                [case["px"]]) as ba:
            corner = ba.reprojection_stats()[3][0]
        ref, px = np.array(case["reprojection_error_camera_model"]), np.array(case["px"])
        rel = np.abs(corner - ref) / (np.abs(ref + px) + np.abs(px))
        print("%-70s worst |device - 50 digits| / (|proj| + |obs|) %.3g" % (label, rel.max()))
        worst = max(worst, rel.max())
        assert rel.max() <= 1e-9, label
    print("worst %.3g" % worst)
