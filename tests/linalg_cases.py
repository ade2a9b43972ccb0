"""Helpers of the accuracy tests (test_linalg_cases_cpu.py, test_gpu_linear_accuracy.py, test_gpu_lm_step.py and
tools/linear_accuracy.py): ill-conditioned test systems, extended-precision references, and a numpy restatement of one
Levenberg-Marquardt step.  numpy only; no tests in here.

Every bound the GPU tests assert is 8 x the error of plain f64 CPU algorithms on the SAME system (reference_bound,
lm_bounds), measured against an np.longdouble reference -- never a figure taken from the kernels.
"""
import numpy as np

import eval_cases as ec
from ref_geometry import pose_plus     # Plus of oracle/vmm_oracle.c (vo_pose_plus) in the dtype of the step
from yardstick import const_sets, free_system

LD = np.longdouble
U64 = 2.0 ** -53      # unit roundoff of f64
MARGIN = 8.0          # the kernel is a third sample of the error class of the two CPU references (they differ by up to ~5)
PLUS_ATOL = 4e-15     # the Plus KAT tolerance of tests/test_oracle_kat.py and test_gpu_kernels.py


# ---- ill-conditioned systems with unit diagonal --------------------------------------------------------------------

def _build_spd_unit_diagonal(n, kappa, seed):
    rng = np.random.default_rng([int(n), int(round(np.log2(kappa) * 1024)), int(seed)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(-np.log10(kappa), 0.0, n)
    A = (Q * lam) @ Q.T
    d = 1.0 / np.sqrt(np.diag(A))
    A = d[:, None] * A * d[None, :]
    A = 0.5 * (A + A.T)
    np.fill_diagonal(A, 1.0)
    return A


_CASES = {}


def spd_unit_diagonal(n, kappa, seed):
    """Q diag(lam) Q^T with lam log-spaced over [1/kappa, 1], scaled symmetrically to unit diagonal (what Jacobi scaling
    makes of an LM pass's reduced system), symmetric, diagonal exactly 1.0.  Built once per session; read-only."""
    return case(n, kappa, seed)["A"]


def case(n, kappa, seed):
    """One test system per (n, kappa, seed), built once per session: A, b, ||A||_2, the refined solution, the two CPU
    references' solutions with their backward and forward errors, and the bounds the kernels are held to."""
    key = (int(n), float(kappa), int(seed))
    c = _CASES.get(key)
    if c is None:
        A = _build_spd_unit_diagonal(*key)
        b = np.random.default_rng([key[0], 77, key[2]]).standard_normal(key[0])
        A.setflags(write=False)
        b.setflags(write=False)
        c = _CASES[key] = dict(n=key[0], kappa=key[1], seed=key[2], A=A, b=b)
    return c


def case_bounds(n, kappa, seed):
    """case() plus everything that costs host time (a few seconds at n = 3136), computed on first use."""
    c = case(n, kappa, seed)
    if "bound" not in c:
        A, b = c["A"], c["b"]
        c["A_ld"] = A.astype(LD)
        c["norm_A"] = spectral_norm(A)
        c["x_ref"] = refined_solution(A, b)
        c["refs"] = {}
        for name, fn in REFERENCE_SOLVERS:
            x = fn(A, b)
            c["refs"][name] = dict(x=x, backward=backward_error(A, b, x, c["norm_A"], c["A_ld"]),
                                   forward=forward_error(x, c["x_ref"]))
        c["bound"] = max(r["backward"] for r in c["refs"].values())
        c["forward_bound"] = max(r["forward"] for r in c["refs"].values())
    return c


def spectral_norm(A):
    """||A||_2 of a symmetric matrix."""
    return float(np.abs(np.linalg.eigvalsh(A)).max())


# ---- extended-precision reference, error measures ------------------------------------------------------------------

def _inverse_factor(A):
    """L^-1 of the f64 Cholesky factor (numpy has no triangular solve; the inverse is applied twice per solve)."""
    L = np.linalg.cholesky(A)
    return np.tril(np.linalg.solve(L, np.eye(len(L))))


def refined_solution(A, b, rounds=8):
    """f64 Cholesky solve + `rounds` of iterative refinement with the residual in np.longdouble; returns longdouble.
    Converges to ~cond(A) * eps(longdouble): 1e-7 at cond 1e12, a hundred times below any f64 solve."""
    Li = _inverse_factor(np.asarray(A, np.float64))
    A_ld, b_ld = np.asarray(A).astype(LD), np.asarray(b).astype(LD)
    x = (Li.T @ (Li @ np.asarray(b, np.float64))).astype(LD)
    for _ in range(rounds):
        r = b_ld - A_ld @ x
        x = x + (Li.T @ (Li @ r.astype(np.float64))).astype(LD)
    return x


def backward_error(A, b, x, norm_A=None, A_ld=None):
    """Normwise backward error ||b - A x||_2 / (||A||_2 ||x||_2 + ||b||_2), residual in np.longdouble."""
    A_ld = np.asarray(A).astype(LD) if A_ld is None else A_ld
    b_ld, x_ld = np.asarray(b).astype(LD), np.asarray(x).astype(LD)
    r = b_ld - A_ld @ x_ld
    if norm_A is None:
        norm_A = np.linalg.norm(np.asarray(A, np.float64), 2)
    nrm = lambda v: np.sqrt(np.sum(v * v))
    return float(nrm(r) / (LD(norm_A) * nrm(x_ld) + nrm(b_ld)))


def forward_error(x, x_ref):
    """max|x - x_ref| / max|x_ref| against the longdouble reference."""
    x_ref = np.asarray(x_ref, LD)
    return float(np.abs(np.asarray(x).astype(LD) - x_ref).max() / np.abs(x_ref).max())


# ---- the two f64 reference solvers ---------------------------------------------------------------------------------

def lapack_solve(A, b):
    return np.linalg.solve(np.asarray(A, np.float64), np.asarray(b, np.float64))


def blocked_explicit_inverse_solve(A, b, nb=64):
    """numpy model of the device algorithm: right-looking Cholesky in blocks of nb (panel by triangular solve, trailing
    update of the whole remaining lower triangle), then both substitutions block by block, each multiplying by the
    EXPLICIT inverse of the nb x nb diagonal factor."""
    S = np.array(A, np.float64)
    n = len(S)
    y = np.array(b, np.float64)
    starts = list(range(0, n, nb))
    inv = []
    for k in starts:
        e = min(k + nb, n)
        Lkk = np.linalg.cholesky(S[k:e, k:e])
        Lkk_inv = np.tril(np.linalg.solve(Lkk, np.eye(e - k)))
        inv.append(Lkk_inv)
        S[k:e, k:e] = Lkk
        if e < n:
            S[e:, k:e] = np.linalg.solve(Lkk, S[e:, k:e].T).T
            S[e:, e:] -= S[e:, k:e] @ S[e:, k:e].T
    for i, k in enumerate(starts):      # forward: y_k = L_kk^-1 (b_k - sum_j<k L_kj y_j)
        e = min(k + nb, n)
        y[k:e] = inv[i] @ (y[k:e] - S[k:e, :k] @ y[:k])
    for i, k in reversed(list(enumerate(starts))):   # backward: x_k = L_kk^-T (y_k - sum_j>k L_jk^T x_j)
        e = min(k + nb, n)
        y[k:e] = inv[i].T @ (y[k:e] - S[e:, k:e].T @ y[e:])
    return y


REFERENCE_SOLVERS = (("lapack", lapack_solve), ("blocked_explicit_inverse", blocked_explicit_inverse_solve))


def reference_bound(A, b):
    """The larger of the two references' backward errors on this system."""
    norm_A = np.linalg.norm(np.asarray(A, np.float64), 2)
    A_ld = np.asarray(A).astype(LD)
    return max(backward_error(A, b, fn(A, b), norm_A, A_ld) for _, fn in REFERENCE_SOLVERS)


# ---- the cases of tests/test_gpu_linear_accuracy.py (shared with the CPU module and tools/linear_accuracy.py) -------

KAPPAS = (1e4, 1e8, 1e12)
# n: which factorisation path: 2 and 6 blocks, 19 (every dataflow workgroup resident), 22 (more
# workgroups than compute units), 49 (paired k_chol_step launches, update-only launch, dataflow tail)
PATH_CASES = [(n, k) for n in (65, 333, 1200, 1408) for k in KAPPAS] + [(3136, 1e8)]
FALLBACK_CASES = [(env, n, 1e8) for env in ("VMM_BA_NO_DATAFLOW", "VMM_BA_NO_CHAIN") for n in (333, 1200)]
BOUNDARY_ORDERS = (1, 2, 7, 8, 9, 63, 64, 127, 128, 129, 3072, 3073)
BOUNDARY_KAPPA = 1e4
SCALING_CASES = [(333, 1e8), (1200, 1e8)]


# ---- SYRK: exact product and the componentwise bound ---------------------------------------------------------------

def syrk_exact_plain(Z):
    """Z^T Z as a plain np.longdouble product (slow: numpy has no BLAS for longdouble; small shapes only)."""
    Z_ld = np.asarray(Z).astype(LD)
    return np.einsum("ki,kj->ij", Z_ld, Z_ld)


def syrk_exact(Z, zero=None):
    """Z^T Z in np.longdouble, error ~2^-64 |Z|^T |Z| (2^-11 of the bound below), at BLAS speed: every column is
    scaled to below 1 by a power of two and cut into three slices whose entries are integers of at most `bits` bits
    (times a power of two), so that every slice product P_a^T P_b is EXACT in f64 whatever the summation order
    (2 bits + log2 k <= 52); the nine products are summed in longdouble, the remainder below 2^-57 enters to first
    order, and the column scales go back on.  `zero` marks entries that cancel exactly by construction
    (cancelling_rows), where the first-order remainder term leaves its rounding."""
    Z = np.asarray(Z, np.float64)
    k = Z.shape[0]
    bits = (52 - int(np.ceil(np.log2(max(k, 2))))) // 2
    _, ex = np.frexp(np.abs(Z).max(axis=0))
    R = np.ldexp(Z, -ex[None, :])
    parts = []
    for i in range(3):
        P = np.ldexp(np.rint(np.ldexp(R, bits * (i + 1))), -bits * (i + 1))
        parts.append(P)
        R = R - P      # exact
    C = np.zeros((Z.shape[1], Z.shape[1]), LD)
    for i in range(2, -1, -1):      # small terms first
        for j in range(2, -1, -1):
            C += parts[i].T @ parts[j]
    Zn = parts[0] + parts[1] + parts[2]
    C += (Zn.T @ R) + (R.T @ Zn)
    C = C * np.ldexp(LD(1), ex)[:, None] * np.ldexp(LD(1), ex)[None, :]
    if zero is not None:
        C[zero] = 0
    return C


def syrk_bound(Z):
    """gamma_k |Z|^T |Z| with gamma_k = k u / (1 - k u): holds entry by entry for Z^T Z summed in ANY order, with or
    without FMA (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  |Z|^T |Z| itself is an f64
    product of non-negative terms, low by at most gamma_k of itself: made good by the factor 1 + 2 gamma_k."""
    k = Z.shape[0]
    Za = np.abs(np.asarray(Z, np.float64))
    _, ex = np.frexp(Za.max(axis=0))
    Za = np.ldexp(Za, -ex[None, :])      # no overflow or underflow whatever the column scales
    gamma = LD(k) * LD(U64) / (1 - LD(k) * LD(U64))
    scale = np.ldexp(LD(1), ex)
    return gamma * (1 + 2 * gamma) * (Za.T @ Za).astype(LD) * scale[:, None] * scale[None, :]


def scaled_columns(k, n, seed, lo=-30, hi=30):
    """(Z, e): standard-normal Z with column j scaled by 2^e_j, so that small entries of Z^T Z sit beside large ones."""
    rng = np.random.default_rng(seed)
    e = rng.integers(lo, hi + 1, n)
    return np.ldexp(rng.standard_normal((k, n)), e[None, :]), e


def cancelling_rows(k, n, seed):
    """(Z, zero): the second half of the rows is the first half with a column-dependent sign, so C_ij is exactly 0
    wherever the signs of columns i and j differ (the mask `zero`)."""
    Z, _ = scaled_columns(k // 2, n, seed)
    sign = np.where(np.random.default_rng(seed + 1).integers(0, 2, n) == 1, 1.0, -1.0)
    # interleaved with a permutation of the second half, so that no summation order pairs the terms by accident
    perm = np.random.default_rng(seed + 2).permutation(k // 2)
    return np.vstack([Z, (Z * sign[None, :])[perm]]), sign[:, None] != sign[None, :]


# ---- one Levenberg-Marquardt step, restated (oracle/vmm_oracle.c: vo_solve); Plus is ref_geometry.pose_plus -----------

def blocks_from_oracle(O, s, cam, tag, robustify, fixed_tag):
    """eval_cases.blocks_from_oracle (reference A of the blocks) at the poses (cam, tag) of a synthetic scene: what
    BundleAdjuster.eval_blocks returns, without a GPU."""
    return ec.blocks_from_oracle(O, ec.Scene(intr=s.intr, dist=s.dist, cam_qt=cam, tag_qt=tag, tag_wh=s.tag_wh, fixed_tag=fixed_tag,
                                             obs_cam=s.obs_cam, obs_tag=s.obs_tag, obs_px=s.obs_px), robust=bool(robustify))


class LmProblem:
    """The full normal equations of one LM iteration over the ACTIVE poses (cameras first, then tags): poses with at
    least one observation that are not held constant (vo_solve: `active`; the fixed tag is constant)."""

    def __init__(self, blk, obs_cam, obs_tag, cam, tag, cam_const=None, tag_const=None):
        obs_cam, obs_tag = np.asarray(obs_cam), np.asarray(obs_tag)
        self.cam, self.tag = np.array(cam, np.float64).reshape(-1, 7), np.array(tag, np.float64).reshape(-1, 7)
        n_c, n_t = len(self.cam), len(self.tag)
        cc = np.zeros(n_c, bool) if cam_const is None else np.asarray(cam_const).astype(bool)
        tc = np.zeros(n_t, bool) if tag_const is None else np.asarray(tag_const).astype(bool)
        self.act_c = np.flatnonzero((np.bincount(obs_cam, minlength=n_c) > 0) & ~cc)
        self.act_t = np.flatnonzero((np.bincount(obs_tag, minlength=n_t) > 0) & ~tc)
        self.n_ac, self.n_at = len(self.act_c), len(self.act_t)
        held_c, held_t = np.ones(n_c, bool), np.ones(n_t, bool)
        held_c[self.act_c], held_t[self.act_t] = False, False
        self.H, self.g, _, _ = free_system(ec.Scene(obs_cam=obs_cam, obs_tag=obs_tag), blk, held_c, held_t)
        self.cost = blk["cost"]
        self.x = np.vstack([self.cam[self.act_c], self.tag[self.act_t]])   # (active poses, 7)

    def gradient_max_norm(self, dtype):
        """max |Plus(x, -g) - x| over the active poses (vo_solve: gradient_norms)."""
        g = self.g.astype(dtype).reshape(-1, 6)
        return np.abs(self.x.astype(dtype) - pose_plus(self.x, -g)).max()

    def damped_system(self, radius, dtype, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
        """(M, s): M = s H s + diag(clamp(diag(s H s))) / radius with the Jacobi scale s = 1 / (1 + sqrt(diag H))."""
        H = self.H.astype(dtype)
        s = 1 / (1 + np.sqrt(np.diag(H)))
        Hs = s[:, None] * H * s[None, :]
        d = np.clip(np.diag(Hs), dtype(min_lm_diagonal), dtype(max_lm_diagonal))
        lm = np.sqrt(d / dtype(radius))      # vo_solve squares the square root
        return Hs + np.diag(lm * lm), s

    def finish(self, step, s):
        """From the solution of the damped system to what an iteration reports: delta = s step, the candidate state,
        model_cost_change = -delta^T (g + H delta / 2), step_norm over the 7-parameter states of the active poses."""
        dtype = step.dtype.type
        delta = s * step
        H, g = self.H.astype(dtype), self.g.astype(dtype)
        cand = pose_plus(self.x, delta.reshape(-1, 6))
        diff = self.x.astype(dtype) - cand
        cam, tag = self.cam.astype(dtype), self.tag.astype(dtype)
        cam[self.act_c] = cand[:self.n_ac]
        tag[self.act_t] = cand[self.n_ac:]
        return dict(cam=cam, tag=tag, model_cost_change=-(delta @ (g + H @ delta / 2)),
                    step_norm=np.sqrt(np.sum(diff * diff)))


def _chol_solve64(M, rhs):
    Li = _inverse_factor(M)
    return Li.T @ (Li @ rhs)


def _schur_solve64(M, rhs, n_elim_front, eliminate_front):
    """Block elimination of one pose family with explicit 6x6 block inverses, Cholesky solve of the reduced system,
    back-substitution (the family of oracle/vmm_oracle.c: solve_schur, and of the device path)."""
    m = 6 * n_elim_front
    idx_e = np.arange(m) if eliminate_front else np.arange(m, len(M))
    idx_k = np.arange(m, len(M)) if eliminate_front else np.arange(m)
    E, B, K = M[np.ix_(idx_e, idx_e)], M[np.ix_(idx_e, idx_k)], M[np.ix_(idx_k, idx_k)]
    Einv = np.zeros_like(E)
    for k in range(0, len(E), 6):
        Einv[k:k + 6, k:k + 6] = np.linalg.inv(E[k:k + 6, k:k + 6])
    Z = Einv @ B
    S = K - B.T @ Z
    yk = _chol_solve64(0.5 * (S + S.T), rhs[idx_k] - Z.T @ rhs[idx_e])
    out = np.zeros(len(M))
    out[idx_k] = yk
    out[idx_e] = Einv @ (rhs[idx_e] - B @ yk)
    return out


def lm_step_reference(prob, radius, eliminate="cams", **clamp):
    """One LM step three times: `ref` in np.longdouble (f64 solve refined with longdouble residuals, everything else
    in longdouble), and the two f64 samples of the error class, `cholesky` (plain Cholesky of M) and `schur` (block
    elimination of the cameras or tags).  Each is the dict of LmProblem.finish plus gradient_max_norm."""
    M_ld, s_ld = prob.damped_system(radius, LD, **clamp)
    rhs_ld = s_ld * prob.g.astype(LD)
    M64 = M_ld.astype(np.float64)
    Li = _inverse_factor(M64)
    x = (Li.T @ (Li @ rhs_ld.astype(np.float64))).astype(LD)
    for _ in range(8):
        r = rhs_ld - M_ld @ x
        x = x + (Li.T @ (Li @ r.astype(np.float64))).astype(LD)
    out = {"ref": prob.finish(-x, s_ld)}
    out["ref"]["gradient_max_norm"] = prob.gradient_max_norm(LD)
    M, s = prob.damped_system(radius, np.float64, **clamp)
    rhs = s * prob.g
    for name, y in (("cholesky", _chol_solve64(M, rhs)),
                    ("schur", _schur_solve64(M, rhs, prob.n_ac, eliminate == "cams"))):
        out[name] = prob.finish(-y, s)
        out[name]["gradient_max_norm"] = prob.gradient_max_norm(np.float64)
    return out


LM_SCALARS = ("gradient_max_norm", "model_cost_change", "step_norm")


def lm_deviation(got, ref):
    """|got - ref| of every compared quantity against the longdouble reference; the state in the max-norm."""
    dev = {k: float(abs(LD(got[k]) - ref[k])) for k in LM_SCALARS}
    dev["state"] = float(max(np.abs(np.asarray(got["cam"]).astype(LD) - ref["cam"]).max(),
                             np.abs(np.asarray(got["tag"]).astype(LD) - ref["tag"]).max()))
    return dev


def lm_bounds(three):
    """Per quantity, 8 x the larger deviation of the two f64 samples from the longdouble reference.  The state is
    compared in the max-norm over all entries (one entry's own deviation can be zero by luck) and gets the floor of
    the Plus KAT tolerance, 4e-15 * max|state|."""
    ref = three["ref"]
    devs = [lm_deviation(three[k], ref) for k in ("cholesky", "schur")]
    bound = {k: MARGIN * max(d[k] for d in devs) for k in devs[0]}
    # both samples take g from the same evaluation, so their gradient_max_norm carries no error of g at all, while
    # the in-solve evaluation sums the same terms in another order: one unit in the last place is that class's sample
    bound["gradient_max_norm"] = MARGIN * max(max(d["gradient_max_norm"] for d in devs),
                                              float(np.spacing(np.float64(ref["gradient_max_norm"]))))
    scale = float(max(np.abs(ref["cam"]).max(), np.abs(ref["tag"]).max()))
    bound["state"] = max(bound["state"], PLUS_ATOL * scale)
    return bound


# ---- the cases of tests/test_gpu_lm_step.py (shared with tools/linear_accuracy.py) -----------------------------------

_CLOSE_UP = dict(n_cams=60, n_tags=40, neighbors_min=4, neighbors_max=7)
_QUARTER = dict(n_cams=40, n_tags=30, visibility=0.25)


def _lm_cases():
    cases = []
    for radius in (1e4, 1e12):      # the second leaves the reduced system at its natural conditioning
        for elim in ("cams", "tags"):
            for robust in (0, 1):   # 20 x 10, dense
                cases.append(dict(name="20x10", config=1, scene={}, elim=elim, robust=robust, env={}, radius=radius))
            for schur in ("dense", "sparse"):   # distortion, outliers, Huber
                cases.append(dict(name="quarter", config=5, scene=_QUARTER, elim=elim, robust=1,
                                  env={"VMM_BA_SCHUR": schur}, radius=radius))
        # block-sparse; with the tags eliminated (60 kept cameras, 6 block columns) this size has a dissection tree, with
        # the cameras eliminated (40 kept tags) it has none
        for order in ("natural", "nd"):
            cases.append(dict(name="close_up", config=1, scene=_CLOSE_UP, elim="tags", robust=0,
                              env={"VMM_BA_SCHUR": "sparse", "VMM_BA_ORDER": order}, radius=radius))
        cases.append(dict(name="20x10_constant_poses", config=1, scene={}, elim="cams", robust=1, env={}, radius=radius,
                          constant=(3, 2)))
    return cases


LM_CASES = _lm_cases()


def lm_case_id(case):
    env = "-".join(v for _, v in sorted(case["env"].items()))
    return "%s-%s-robust%d%s-radius%.0e" % (case["name"], case["elim"], case["robust"], "-" + env if env else "",
                                           case["radius"])


def run_lm_case(eng, case, setenv):
    """One LM iteration on the device (BundleAdjuster.solve, max_num_iterations = 1) and its three restatements from
    the same handle's eval_blocks at the start state.  setenv(name, value) sets a switch that the handle reads when
    it is created (value None: unset).  Returns (out, got, three, bound, extra)."""
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(case["config"], **case["scene"])
    for name in ("VMM_BA_SCHUR", "VMM_BA_ORDER"):
        setenv(name, case["env"].get(name))
    cam_const, tag_const = None, np.zeros(len(s.tag_init), np.uint8)
    if case.get("constant"):
        cam_const, tag_const = const_sets(s, *case["constant"])
    mode = eng.ELIM_CAMERAS if case["elim"] == "cams" else eng.ELIM_TAGS
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag,
                            s.obs_px, elimination=mode)
    try:
        if case.get("constant"):
            ba.set_constant_poses(cam_const, tag_const)
        blk = ba.eval_blocks(robustify=bool(case["robust"]))
        out = ba.solve(eng.default_options(robustify=case["robust"], max_num_iterations=1,
                                           initial_trust_region_radius=case["radius"]), trace_capacity=8)
        cam, tag = ba.get_state()
        cost_after = ba.cost(robustify=bool(case["robust"]))
    finally:
        ba.close()
    tag_const = tag_const.astype(bool)
    tag_const[s.fixed_tag] = True      # a fixed tag in every case: the gauge
    prob = LmProblem(blk, s.obs_cam, s.obs_tag, s.cam_init, s.tag_init, cam_const, tag_const)
    three = lm_step_reference(prob, case["radius"], case["elim"])
    trace = out["trace"]
    got = dict(cam=cam, tag=tag, gradient_max_norm=trace[0]["gradient_max_norm"],
               model_cost_change=trace[1]["model_cost_change"] if len(trace) > 1 else np.nan,
               step_norm=trace[1]["step_norm"] if len(trace) > 1 else np.nan)
    extra = dict(scene=s, cost_after=cost_after, cam_const=cam_const, tag_const=tag_const, start_cost=blk["cost"])
    return out, got, three, lm_bounds(three), extra
