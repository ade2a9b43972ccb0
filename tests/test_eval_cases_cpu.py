"""The references and scenes of tests/eval_cases.py, checked on the CPU before the GPU tests rely on them:
the longdouble restatement against the 50-digit known answers, the oracle on the hard geometry (recorded), the builders'
conditions, and references A (oracle), B (float64) and the longdouble assembly against one another.

Known answers are stored as doubles, so a comparison with one is exact only up to 2^-53 |stored value|; what is asked
of the longdouble chain beyond that is KAT_UNITS x 2^-64 x the entry's magnitude (eval_cases: the entry's own sum over
absolute values).
"""
import numpy as np
import pytest

import eval_cases as ec
import ref_geometry as rg

LD = ec.LD
KAT_UNITS = 64.0


def _condition(case):
    """How many times the camera-frame depth Z = (R_c P_w)_z + t_z is smaller than the numbers it is the sum of, times how
    many times a pixel coordinate f xd + c is smaller than |f xd| + |c| (a close-up reaches across the principal point's
    axes, where the coordinate passes through 0 and |proj| + |obs| no longer measures what was added up).  Only the cases
    named in NEEDS_MORE get their tolerance multiplied by it."""
    cam, tag = np.array(case["cam_qt"]), np.array(case["tag_qt"])
    _, proj, _, _ = ec.corner_chain(case["intr"], case["dist"], [cam], [tag], [case["wh"]], [case["px"]])
    c = np.array([case["intr"][2], case["intr"][3]], LD)
    px = np.abs(np.array(case["px"], LD).reshape(4, 2))
    pixel = float(np.max((np.abs(proj[0] - c) + np.abs(c) + px) / (np.abs(proj[0]) + px)))
    Rc = rg.rotation(cam, LD)
    Rt = rg.rotation(tag, LD)
    worst = 1.0
    for sx, sy in rg.CORNER_SIGNS:
        a = Rt @ np.array([sx * case["wh"][0] / 2, sy * case["wh"][1] / 2, 0.0], LD)
        pw = a + tag[4:]
        b = Rc @ pw
        z = b[2] + cam[6]
        worst = max(worst, float((np.abs(Rc[2]) @ (np.abs(a) + np.abs(tag[4:])) + abs(cam[6])) / abs(z)))
    return worst * pixel


# Measured with this file: every `obs` and `obs_hard` record is inside 64 x 2^-64 except these, where the depth cancels
# (Z = 0.15 m from terms of about 1 m: x 2 .. 4; Z = 3 m from terms of about 1e3 m: x 1000) and every later quantity
# inherits the depth's relative error -- of the input poses as given, not of the chain; the close-up with the strong
# distortion also has a corner 31 px from the image's left edge, whose |proj| + |obs| is 1 / 100 of |f xd| + |c|.
NEEDS_MORE = ("camera 0.15 m from the tag", "translations near 1e3 m")


def _kat_tolerance_units(case):
    what = case.get("what", "")
    return KAT_UNITS * (_condition(case) if what.startswith(NEEDS_MORE) else 1.0)


def _excess(got, stored, mag):
    """Worst (|got - stored| - 2^-53 |stored|) / magnitude over the entries of non-zero magnitude, in units of 2^-64;
    entries of zero magnitude must agree exactly."""
    got, stored, mag = (np.asarray(v, LD).reshape(-1) for v in (got, stored, mag))
    nz = mag > 0
    assert np.all(got[~nz] == stored[~nz])
    err = np.abs(got - stored) - LD(2.0 ** -53) * np.abs(stored)
    return float(np.max(err[nz] / mag[nz])) * 2.0 ** 64


@pytest.mark.parametrize("section", ["obs", "obs_hard"])
def test_longdouble_chain_reproduces_the_known_answers(kats, section):
    for i, case in enumerate(kats[section]):
        r, proj, Jc, Jt, Jc_mag, Jt_mag = ec.corner_chain(case["intr"], case["dist"], [case["cam_qt"]], [case["tag_qt"]],
                                                          [case["wh"]], [case["px"]], want_magnitude=True)
        r_mag = np.abs(proj) + np.abs(np.array(case["px"], LD).reshape(1, 4, 2))
        units = _kat_tolerance_units(case)
        got = (_excess(r, case["residual"], r_mag), _excess(Jc, case["J_cam"], Jc_mag), _excess(Jt, case["J_tag"], Jt_mag))
        print("%s %2d %-70s residual %9.1f  J_cam %9.1f  J_tag %9.1f  (x 2^-64 beyond the stored rounding; allowed %.0f)"
              % (section, i, case.get("what", ""), got[0], got[1], got[2], units))
        assert max(got) <= units, (section, i, case.get("what"))


@pytest.mark.parametrize("section", ["huber", "huber_widths"])
def test_longdouble_huber_reproduces_the_known_answers(kats, section):
    for case in kats[section]:
        got = ec.huber(case["a"], case["s"])
        ref = np.array(case["rho"], LD)
        # rho is 2 a sqrt(s) - b above the threshold: its magnitude is 2 a sqrt(s) + b; rho' and rho'' are single terms
        mag = np.abs(ref)
        if case["s"] > case["a"] * case["a"]:
            mag[0] = 2 * LD(case["a"]) * np.sqrt(LD(case["s"])) + LD(case["a"] * case["a"])
        if np.any(mag == 0):
            assert np.all(got[mag == 0] == 0)
        assert _excess(got[mag > 0], ref[mag > 0], mag[mag > 0]) <= KAT_UNITS, case


def test_oracle_huber_matches_the_widths(oracle, kats):
    """oracle.huber at a != 1, at the tolerance of test_oracle_kat.test_huber_matches_closed_form."""
    for case in kats["huber_widths"]:
        np.testing.assert_allclose(oracle.huber(case["a"], case["s"]), case["rho"], rtol=1e-15, atol=0, err_msg=str(case))


def test_oracle_on_the_hard_geometry_is_recorded(oracle, kats):
    """oracle.obs_eval has not seen such input before.  Its deviation from the longdouble chain, entry by entry relative
    to the entry's magnitude, is printed beside that of the plain float64 chain (reference B) in units of 2^-53; nothing is
    asserted of its size beyond being finite -- the GPU tests take their bound from these two references, so a reference
    that is far off shows as a slack bound there, and the figures are in DESIGN.md."""
    for section in ("obs", "obs_hard"):
        for i, case in enumerate(kats[section]):
            args = (case["intr"], case["dist"], [case["cam_qt"]], [case["tag_qt"]], [case["wh"]], [case["px"]])
            r, proj, Jc, Jt, Jc_mag, Jt_mag = ec.corner_chain(*args, want_magnitude=True)
            r_mag = np.abs(proj) + np.abs(np.array(case["px"], LD).reshape(1, 4, 2))
            ro, Jco, Jto = oracle.obs_eval(case["intr"], case["dist"], case["cam_qt"], case["tag_qt"], case["wh"], case["px"])
            rb, _, Jcb, Jtb = ec.corner_chain(*args, dtype=np.float64)
            line = []
            for got_o, got_b, ref, mag in ((ro, rb, r, r_mag), (Jco, Jcb, Jc, Jc_mag), (Jto, Jtb, Jt, Jt_mag)):
                ref, mag = ref.reshape(-1), mag.reshape(-1)
                nz = mag > 0
                devs = [float(np.max(np.abs(np.asarray(g, LD).reshape(-1) - ref)[nz] / mag[nz])) * 2.0 ** 53
                        for g in (got_o, got_b)]
                assert np.all(np.isfinite(devs))
                line.append("%8.1f /%8.1f" % tuple(devs))
            print("%s %2d %-70s oracle / float64, x 2^-53: residual %s  J_cam %s  J_tag %s"
                  % (section, i, case.get("what", ""), line[0], line[1], line[2]))


# ---- the builders' conditions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("few", ["tags", "cams"])
def test_ragged_scene_has_the_counts_it_promises(few):
    s = ec.ragged_scene(few)
    assert (len(s.cam_qt), len(s.tag_qt)) == ((130, 6) if few == "tags" else (6, 130))
    six_idx, many_idx = (s.obs_tag, s.obs_cam) if few == "tags" else (s.obs_cam, s.obs_tag)
    assert tuple(np.bincount(six_idx, minlength=6)) == (1, 63, 64, 65, 128, 129)
    per_many = np.bincount(many_idx, minlength=130)
    assert (per_many == 0).sum() == 1 and per_many[129] == 0
    assert len(set(zip(s.obs_cam.tolist(), s.obs_tag.tolist()))) == s.n_obs      # no pair twice (the fused lookup table)
    tc, tt = ec.task_counts(s)
    assert sorted((tc, tt)) == [10, 129] and tc % 4 and tt % 4
    # the mask switches off the last observation of the 65-observation pose: lane 0 of that pose's second task
    m = ec.ragged_mask(s)
    k65 = ec.RAGGED_COUNTS.index(65)
    assert m[s.last_of_65] == 0 and np.flatnonzero(six_idx == k65)[64] == s.last_of_65
    assert (m[::7] == 0).all() and m.sum() < s.n_obs
    cc, tc_ = ec.ragged_constants(s)
    assert cc.sum() == 1 and tc_.sum() == 1 and (s.fixed_tag < 0 or not tc_[s.fixed_tag])


@pytest.mark.parametrize("a", [0.5, 1.0, 2.5])
def test_mixed_scene_puts_corners_on_both_sides_of_the_threshold(a):
    s = ec.mixed_scene(a)
    assert (len(s.cam_qt), len(s.tag_qt), s.n_obs) == (12, 9, 108)
    above = ec.fraction_above(s, a)
    print("a = %g: %.1f %% of the corners have |r|^2 > a^2" % (a, 100 * above))
    assert 0.2 <= above <= 0.8


@pytest.mark.parametrize("strong", [False, True])
def test_hard_batch_places_the_records(kats, strong):
    s = ec.hard_batch(strong, kats)
    recs = [c for c in kats["obs_hard"] if (np.abs(c["dist"]).max() > 0) == strong]
    assert len(recs) == 8 and len(s.cam_qt) == 8 and s.n_obs == 8 * 65
    assert (np.bincount(s.obs_cam) == 65).all()
    r, _, _, _ = ec.corner_chain(s.intr, s.dist, s.cam_qt[s.obs_cam], s.tag_qt[s.obs_tag], s.tag_wh[s.obs_tag], s.obs_px)
    for i, rec in enumerate(recs):
        np.testing.assert_array_equal(s.obs_px[65 * i], rec["px"])
        np.testing.assert_array_equal(s.tag_qt[s.obs_tag[65 * i]], rec["tag_qt"])
        # lanes 63 and 64 carry the residual pattern of the next two records (up to the rounding of the moved tag's pose)
        for slot, other in ((63, recs[(i + 1) % 8]), (64, recs[(i + 2) % 8])):
            ref = np.array(other["residual"])
            assert np.abs(r[65 * i + slot].reshape(8).astype(np.float64) - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
        assert np.abs(r[65 * i + 1:65 * i + 63]).max() < 10.0


# ---- the references agree ---------------------------------------------------------------------------------------------

def _cpu_cases(oracle, kats):
    s1 = ec.ragged_scene("tags")
    cc, tc = ec.ragged_constants(s1)
    yield "mixed a=0.5", ec.cached(("case", "mixed", 0.5, True), lambda: ec.Case(oracle, ec.mixed_scene(0.5), a=0.5))
    yield "mixed a=2.5 not robust", ec.cached(("case", "mixed", 2.5, False),
                                              lambda: ec.Case(oracle, ec.mixed_scene(2.5), a=2.5, robust=False))
    yield "ragged tags, mask, constants", ec.cached(("case", "ragged", "tags", True, True), lambda: ec.Case(
        oracle, s1, mask=ec.ragged_mask(s1), cam_const=cc, tag_const=tc))
    yield "ragged cams", ec.cached(("case", "ragged", "cams", False, False), lambda: ec.Case(oracle, ec.ragged_scene("cams")))
    for strong in (False, True):
        yield "hard batch%s" % (" strong" if strong else ""), ec.cached(
            ("case", "hard", strong, True), lambda: ec.Case(oracle, ec.hard_batch(strong, kats)))


def test_references_agree_on_the_assembled_blocks(oracle, kats):
    """A (oracle functor, numpy sums), B (float64 chain) and the longdouble assembly, per entry relative to the entry's
    magnitude.  What limits an f64 evaluation here is not the sums but the Huber weight a / |r|: |r| is a difference of
    pixel coordinates of some 6e3 px and is known to 6e3 x 2^-53 x a few = 1e-12 px, so to 1e-12 .. 1e-11 of itself at
    |r| = 0.5 .. a few px, and every weighted entry inherits that.  Hence 1e-11 here (per entry, where the older tests ask
    1e-10 of the largest entry); the hard batch holds the records whose depth cancels a thousandfold (test above), so its
    limit is that much wider.  Entries of magnitude 0 are exactly 0 in all of them."""
    for label, c in _cpu_cases(oracle, kats):
        limit = 1e-8 if label.startswith("hard") else 1e-11
        for name, dev in c.refs.items():
            print("%-30s %-10s %s" % (label, name, "  ".join("%s %.2e" % (k, dev[k][0]) for k in ec.ARRAYS)))
            for k in ec.ARRAYS:
                assert dev[k][1], (label, name, k)
                assert dev[k][0] <= limit, (label, name, k, dev[k][0])
        # the magnitudes bound the entries they belong to
        for k in ec.ARRAYS:
            assert np.all(np.abs(np.asarray(c.ref[k])) <= np.asarray(c.mag[k]) * (1 + 1e-15))


def test_float32_reference_deviates_at_float32_level(oracle):
    c = ec.cached(("case", "mixed", 1.0, True, "f32"), lambda: ec.Case(oracle, ec.mixed_scene(1.0), a=1.0, f32=True))
    f = c.refs["F float32 products"]
    print("reference F on mixed a=1: " + "  ".join("%s %.2e" % (k, f[k][0]) for k in ec.ARRAYS))
    for k in ("V", "U", "W"):
        assert 2.0 ** -26 <= f[k][0] <= 64 * 2.0 ** -24
    for k in ("g_cam", "g_tag", "cost"):    # f64 whatever the products' type
        assert f[k][0] <= 1e3 * 2.0 ** -53
