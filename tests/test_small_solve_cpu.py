"""The small dense algebra of visual_marker_mapping_amd/csrc/small_solve.hpp (the Cholesky factorisation of a 3-, 6-
or 9-unknown system, its substitutions, inverses, pivot policies and the Levenberg-Marquardt trial loop) driven through
tests/cpp/small_solve_test, built with g++ from the header alone, and compared with numpy on the CPU.

Tolerances.  Cholesky's backward error bounds the relative error of a solution or of an inverse by a small multiple of
N eps kappa: 100 N eps kappa relative to the largest entry, kappa = numpy's condition number of the generated matrix.
L L^T against A: 100 N eps entry by entry, relative to max |A|."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SIZES = (3, 6, 9)
KAPPAS = (1.0, 1e2, 1e4)


@pytest.fixture(scope="module")
def run():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-s", "small_solve_test"])
    exe = os.path.join(ROOT, "tests", "cpp", "small_solve_test")

    def call(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [[float(t) for t in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return call


def _num(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, np.float64).reshape(-1))


def _spd(n, kappa, seed):
    """Eigenvalues log-spaced from 1 to kappa in a seeded orthogonal basis."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    a = (q * np.logspace(0.0, np.log10(kappa), n)) @ q.T
    return (a + a.T) / 2


def _tol(n, a):
    return 100 * n * EPS * np.linalg.cond(a)


def _cases():
    return [(n, k, 100 * n + i) for n in SIZES for i, k in enumerate(KAPPAS)]


def _layouts(n):
    return ("p", "r") if n == 6 else ("p",)   # the engine factors row-major only at 6 x 6 (L_e)


def test_factor_reproduces_the_matrix(run):
    todo = [(n, a, lay) for n, k, seed in _cases() for a in [_spd(n, k, seed)] for lay in _layouts(n)]
    got = run(["factor %d %s %s" % (n, lay, _num(a)) for n, a, lay in todo])
    for (n, a, lay), g in zip(todo, got):
        assert g[0] == 1
        L = np.array(g[1:]).reshape(n, n)
        assert (np.triu(L, 1) == 0).all() and (np.diag(L) > 0).all()
        gap = np.abs(L @ L.T - a).max() / np.abs(a).max()
        print("factor", n, lay, "gap", gap, "bound", 100 * n * EPS)
        assert gap <= 100 * n * EPS


def test_solve_against_numpy(run):
    todo = []
    for n, k, seed in _cases():
        a, b = _spd(n, k, seed), np.random.default_rng(seed + 50).normal(size=n)
        todo += [(n, a, b, lay) for lay in _layouts(n)]
    got = run(["solve %d %s %s %s" % (n, lay, _num(a), _num(b)) for n, a, b, lay in todo])
    for (n, a, b, lay), g in zip(todo, got):
        ref = np.linalg.solve(a, b)
        gap = np.abs(np.array(g[1:]) - ref).max() / np.abs(ref).max()
        print("solve", n, lay, "gap", gap, "bound", _tol(n, a))
        assert g[0] == 1 and gap <= _tol(n, a)


def test_inverse_against_numpy(run):
    todo = [(n, _spd(n, k, seed)) for n, k, seed in _cases()]
    got = run(["inverse %d %s" % (n, _num(a)) for n, a in todo])
    for (n, a), g in zip(todo, got):
        ref = np.linalg.inv(a)
        c = np.array(g[3:]).reshape(n, n)
        gap = np.abs(c - ref).max() / np.abs(ref).max()
        print("inverse", n, "gap", gap, "bound", _tol(n, a))
        assert g[:3] == [1, 1, 1] and (c == c.T).all() and gap <= _tol(n, a)


def test_row_major_block_forms_against_numpy(run):
    """forward_block<6, 6> (k_form_z's L^-1 X) and lower_inverse_full<6> (the covariance kernels' L^-1)."""
    for i, k in enumerate(KAPPAS):
        a, x = _spd(6, k, 700 + i), np.random.default_rng(750 + i).normal(size=(6, 6))
        got = run(["block %s %s" % (_num(a), _num(x)), "invfull %s" % _num(a)])
        L = np.linalg.cholesky(a)
        for g, ref in zip(got, (np.linalg.solve(L, x), np.linalg.inv(L))):
            gap = np.abs(np.array(g[1:]).reshape(6, 6) - ref).max() / np.abs(ref).max()
            print("block form, kappa", k, "gap", gap, "bound", _tol(6, a))
            assert g[0] == 1 and gap <= _tol(6, a)
        assert (np.triu(np.array(got[1][1:]).reshape(6, 6), 1) == 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_damped_solve_against_numpy(run, n):
    """(A + lam diag(max(A_ii, 1e-12))) step = -g at lam 0, 1e-3 and 1e3, on a matrix whose last diagonal entry, 1e-13,
    is below the floor (an unknown the sums do not see: its row and column are otherwise zero) and on a plain one."""
    rng = np.random.default_rng(800 + n)
    tiny = np.zeros((n, n))
    tiny[:n - 1, :n - 1] = _spd(n - 1, 1e2, 810 + n)
    tiny[n - 1, n - 1] = 1e-13
    for a in (tiny, _spd(n, 1e2, 820 + n)):
        g = rng.normal(size=n)
        lams = (0.0, 1e-3, 1e3)
        got = run(["damped %d %r %s %s" % (n, lam, _num(a), _num(g)) for lam in lams])
        for lam, res in zip(lams, got):
            damped = a + lam * np.diag(np.maximum(np.diag(a), 1e-12))
            ref = np.linalg.solve(damped, -g)
            gap = np.abs(np.array(res[2:]) - ref).max() / np.abs(ref).max()
            print("damped", n, lam, "gap", gap, "bound", _tol(n, damped))
            assert res[:2] == [1, 1] and gap <= _tol(n, damped)
        if a is tiny:   # the floor decides the last unknown's step at lam = 1e3: without it the step is ten times larger
            last = -g[n - 1] / (1e-13 + 1e3 * 1e-12)
            assert abs(got[2][-1] - last) <= 100 * EPS * abs(last)


def _singular(n):
    """Integer entries, the last two rows and columns equal: A = L0 L0^T with an integer L0 whose diagonal entries are
    powers of two, so that every square root and reciprocal of the factorisation is exact and the last pivot is exactly 0."""
    rng = np.random.default_rng(900 + n)
    l0 = np.tril(rng.integers(-2, 3, (n, n)).astype(np.float64), -1) + np.diag(2.0 ** rng.integers(0, 3, n))
    l0[n - 1] = l0[n - 2]
    a = l0 @ l0.T
    assert (a[n - 1] == a[n - 2]).all() and (a == np.round(a)).all()
    return a


def _bad_matrices(n):
    good = _spd(n, 1e2, 950 + n)
    indefinite = good.copy()
    indefinite[n // 2, n // 2] *= -1.0
    out = {"singular": _singular(n), "indefinite": indefinite}
    for name, value in (("nan", np.nan), ("inf", np.inf)):
        for where, (i, j) in (("diagonal", (n // 2, n // 2)), ("off_diagonal", (n - 1, 0))):
            m = good.copy()
            m[i, j] = m[j, i] = value
            out["%s_%s" % (name, where)] = m
    return out


@pytest.mark.parametrize("n", SIZES)
def test_every_policy_refuses_a_bad_matrix(run, n):
    bad = _bad_matrices(n)
    ones = _num(np.ones(n))
    for name, a in bad.items():
        got = run(["policy %d positive %s" % (n, _num(a)), "policy %d bits %s" % (n, _num(a)),
                   "policy %d orone %s" % (n, _num(a)), "policy %d weighted %s %s 0.0" % (n, _num(a), ones),
                   "damped %d 0.0 %s %s" % (n, _num(a), ones)])
        assert [g[0] for g in got[:4]] == [0, 0, 0, 0], name
        # replace-by-1 repairs pivots; a non-finite entry off the diagonal is copied into L by any rule
        assert got[2][1] == (0 if "off_diagonal" in name else 1), name + ": the replace-by-1 factor"
        assert got[4][:2] == [0, 0], name
    good = _spd(n, 1e2, 950 + n)
    got = run(["policy %d %s %s%s" % (n, p, _num(good), " %s 0.0" % ones if p == "weighted" else "")
               for p in ("positive", "bits", "orone", "weighted")])
    assert [g[:2] for g in got] == [[1, 1]] * 4


def test_the_one_inverse_rule_against_the_per_pivot_rule(run):
    """spd_inverse's single finiteness test of the Gram sum against the rule inverse3 had (a test per pivot next to it), on
    3 x 3 inputs.  They agree on the singular, the indefinite and the NaN inputs and on +inf off the diagonal.  They do
    not agree on +inf on the diagonal: that pivot's square root is +inf and its reciprocal 0, so its row and column
    come out as finite zeros and the single test passes.  That is why kernels_triangulate.hip, whose sums can overflow,
    asks for spd_inverse<3, PivotPositive<true>>, which is inverse3's rule on every input."""
    bad = _bad_matrices(3)
    got = run(["inverse 3 %s" % _num(a) for a in bad.values()])
    for name, g in zip(bad, got):
        one_rule, per_pivot, old = g[:3]
        assert per_pivot == old == 0, name
        assert one_rule == (1 if name == "inf_diagonal" else 0), name


def test_weighted_policy_judges_the_weighted_pivot(run):
    """chol9's rule: d weight[j] > min_pivot.  diag(1, 1e-14, 1) with min_pivot 1e-13: unweighted the middle pivot is
    below the bound, with weight 100 it is above; diag(1, 1e-12, 1): unweighted above, with weight 0.01 below."""
    for n in SIZES:
        for d, w, expect_plain, expect_weighted in ((1e-14, 100.0, 0, 1), (1e-12, 0.01, 1, 0)):
            a, weight = np.eye(n), np.ones(n)
            a[1, 1], weight[1] = d, w
            got = run(["policy %d weighted %s %s 1e-13" % (n, _num(a), _num(np.ones(n))),
                       "policy %d weighted %s %s 1e-13" % (n, _num(a), _num(weight))])
            assert [got[0][0], got[1][0]] == [expect_plain, expect_weighted], (n, d)


def _lsq(n, seed, scale=1.0):
    """A consistent system b = J x: with a residual at the minimum the cost could not resolve a change of x below
    sqrt(eps) (cost = c* + |J dx|^2), and the loop, which accepts only a lower cost, would stop there by design."""
    rng = np.random.default_rng(seed)
    m = 3 * n
    J = rng.normal(size=(m, n))
    x = scale * rng.normal(size=n)
    return m, J, J @ x


def _lm_line(n, stop_small, mode, max_trials, m, J, b, x0):
    return "lm %d %d %s %d %d %s %s %s" % (n, stop_small, mode, max_trials, m, _num(J), _num(b), _num(x0))


@pytest.mark.parametrize("n", (3, 6))
def test_trial_loop_solves_linear_least_squares(run, n):
    m, J, b = _lsq(n, 1000 + n)
    (g,) = run([_lm_line(n, 0, "plain", 50, m, J, b, np.zeros(n))])
    ref = np.linalg.lstsq(J, b, rcond=None)[0]
    trials, cost, cost_again, x = int(g[0]), g[1], g[2], np.array(g[3:])
    gap = np.abs(x - ref).max() / np.abs(ref).max()
    print("lm", n, "trials", trials, "gap", gap, "bound", _tol(n, J.T @ J))
    assert trials <= 50 and gap <= _tol(n, J.T @ J)
    assert cost == cost_again   # the same sums at the returned state, bit for bit


@pytest.mark.parametrize("n", (3, 6))
def test_trial_loop_without_trials(run, n):
    m, J, b = _lsq(n, 1010 + n)
    x0 = np.random.default_rng(1020 + n).normal(size=n)
    (g,) = run([_lm_line(n, 0, "plain", 0, m, J, b, x0)])
    assert g[0] == 0 and g[1] == g[2] and np.array(g[3:]).tobytes() == x0.tobytes()


@pytest.mark.parametrize("n", (3, 6))
def test_trial_loop_ends_on_the_damping_bound(run, n):
    """Every candidate costs +inf: each trial is rejected and multiplies the damping by ten until it exceeds kLamMax.  The
    minimum is 1e6 away, so the step stays above the 1e-10 limit up to the largest damping (1e6 / 1e12 = 1e-6)."""
    m, J, b = _lsq(n, 1030 + n, scale=1e6)
    x0 = np.random.default_rng(1040 + n).normal(size=n)
    (g,) = run([_lm_line(n, 0, "inf", 100, m, J, b, x0)])
    lam, expect = 1e-3, 0
    while not lam > 1e12:
        expect += 1
        lam *= 10.0
    assert g[0] == expect and expect < 100
    assert np.array(g[3:]).tobytes() == x0.tobytes() and g[1] == g[2]


@pytest.mark.parametrize("n", (3, 6))
def test_stop_small_ends_after_a_small_accepted_step(run, n):
    """From 1e-10 beside the minimum of a consistent system the first step is accepted (the cost falls by six orders) and
    is below 1e-9: STOP_SMALL ends there, the plain loop goes on to the next trial.  The count is the loop's index when
    it leaves, so the trial an exit happens in is not part of it: 0 for the exit in the first trial, at least 1 for the
    loop that goes on."""
    m, J, b = _lsq(n, 1050 + n)
    x0 = np.linalg.lstsq(J, b, rcond=None)[0] + 1e-10
    small, plain = run([_lm_line(n, 1, "plain", 50, m, J, b, x0), _lm_line(n, 0, "plain", 50, m, J, b, x0)])
    assert small[0] == 0 and plain[0] >= 1
    assert np.array(small[3:]).tobytes() != x0.tobytes()   # the step was taken


def test_sanitizer_build_runs_clean(run):
    """The same program under the address and undefined-behaviour sanitizers, as an executable of its own."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-s", "small_solve_test_san"])
    lines = ["factor 6 r %s" % _num(_spd(6, 1e2, 1)), "inverse 9 %s" % _num(_spd(9, 1e2, 2)), "inverse 3 %s" % _num(_singular(3)),
             "block %s %s" % (_num(_spd(6, 1e2, 3)), _num(np.eye(6))), "invfull %s" % _num(_spd(6, 1e2, 4)),
             "damped 9 1e-3 %s %s" % (_num(_spd(9, 1e2, 5)), _num(np.ones(9))),
             "policy 9 weighted %s %s 1e-13" % (_num(_spd(9, 1e2, 6)), _num(np.ones(9)))]
    for n in (3, 6):
        m, J, b = _lsq(n, 1060 + n)
        lines.append(_lm_line(n, 0, "plain", 50, m, J, b, np.zeros(n)))
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "small_solve_test_san")], input="\n".join(lines) + "\n",
                       capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == len(lines), r.stdout + r.stderr
