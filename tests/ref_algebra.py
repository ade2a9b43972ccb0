"""The device's small dense algebra and its summation orders restated in float64, one IEEE operation at a time, once: what
every reference B (finished_map_cases, arrowhead_cases, init_cases, predict_joint_cases) is made of.  numpy only; it
imports neither the engine nor the oracle, and there are no tests in here (test_ref_modules_cpu.py checks it).  Each
docstring names the routine it restates; a change to that routine's order of operations is made here and nowhere else.
"""
import numpy as np


# ---- small_solve.hpp ----------------------------------------------------------------------------------------------------------

def cholesky(A):
    """small_solve.hpp's cholesky<N>: the lower factor column by column, d -= L_jk^2 and v -= L_ik L_jk in ascending k,
    one reciprocal per column."""
    n = len(A)
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        L[j, j] = np.sqrt(d)
        inv = 1.0 / L[j, j]
        for i in range(j + 1, n):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v * inv
    return L


def forward(L, b):
    """forward_substitute<N> / forward_block<N, NC>: L^-1 b, b a vector or the columns of a matrix."""
    out = np.zeros_like(b, dtype=np.float64)
    for i in range(len(L)):
        v = b[i]
        for k in range(i):
            v = v - L[i, k] * out[k]
        out[i] = v / L[i, i]
    return out


def backward(L, b):
    """backward_substitute<N>: L^-T b."""
    out = np.zeros_like(b, dtype=np.float64)
    for i in range(len(L) - 1, -1, -1):
        v = b[i]
        for k in range(i + 1, len(L)):
            v = v - L[k, i] * out[k]
        out[i] = v / L[i, i]
    return out


def lower_inverse(L):
    """lower_inverse<N>: M = L^-1, column by column, k from j up."""
    n = len(L)
    M = np.zeros((n, n))
    for j in range(n):
        M[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, n):
            v = 0.0
            for k in range(j, i):
                v = v - L[i, k] * M[k, j]
            M[i, j] = v / L[i, i]
    return M


def lower_gram(M):
    """lower_gram<N>: C = M^T M of a lower triangle, k from a up, both triangles filled."""
    n = len(M)
    C = np.zeros((n, n))
    for a in range(n):
        for b in range(a + 1):
            v = 0.0
            for k in range(a, n):
                v = v + M[k, a] * M[k, b]
            C[a, b] = C[b, a] = v
    return C


def spd_inverse(A):
    """spd_inverse<N>: cholesky -> lower_inverse -> lower_gram."""
    return lower_gram(lower_inverse(cholesky(np.asarray(A, np.float64))))


def damped(A, lam):
    """damped_solve's matrix: A + lam diag(max(A_ii, 1e-12))."""
    D = np.array(A, np.float64)
    D[np.diag_indices(len(D))] += lam * np.maximum(np.diag(D), 1e-12)
    return D


def damped_solve(A, g, lam):
    """damped_solve<N>: (A + lam diag(max(A_ii, 1e-12))) step = -g by cholesky, forward and backward substitution."""
    L = cholesky(damped(A, lam))
    return backward(L, forward(L, -np.asarray(g, np.float64)))


# ---- pose_lm.hpp ----------------------------------------------------------------------------------------------------------------

def sandwich(C, S):
    """pose_lm.hpp's sandwich6 (and k_triangulate's 3 x 3 twin): T = C S, entry (r, c) of T C averaged with its mirror
    image."""
    n = len(C)
    T = np.zeros((n, n))
    for r in range(n):
        for c in range(n):
            t = 0.0
            for k in range(n):
                t = t + C[r, k] * S[k, c]
            T[r, c] = t
    out = np.zeros((n, n))
    for r in range(n):
        for c in range(r + 1):
            x = y = 0.0
            for k in range(n):
                x = x + T[r, k] * C[k, c]
                y = y + T[c, k] * C[k, r]
            out[r, c] = out[c, r] = 0.5 * (x + y)
    return out


# ---- summation orders -------------------------------------------------------------------------------------------------------------

def ordered_sum(terms):
    """The sum of terms[0], terms[1], ... in that order, as a thread adds its list (np.cumsum adds one after the other)."""
    return np.cumsum(terms, axis=0)[-1]


def chains4(x):
    """arrowhead.hpp's record sums (k_calib_solve, k_rigcal_solve): item i in chain i mod 4, the four interleaved chains
    combined ((0 + 1) + 2) + 3."""
    t = [ordered_sum(x[g::4]) if len(x[g::4]) else np.zeros(x.shape[1:]) for g in range(4)]
    return ((t[0] + t[1]) + t[2]) + t[3]


def tree256(v):
    """kernels_init.hip's block_sum2: the tree over 256 thread-private sums, the upper half added onto the lower."""
    v = np.asarray(v, np.float64).copy()
    m = 128
    while m >= 1:
        v[:m] = v[:m] + v[m:2 * m]
        m //= 2
    return v[0]


def wave_total(terms):
    """kernels_init.hip's refine_sums order for terms (m, 4, ...): lane l adds its observations l, l + 64, ... corner by
    corner, then geom.hpp's wave_sum butterfly; lane 0's total."""
    terms = np.asarray(terms)
    v = np.zeros((64,) + terms.shape[2:], terms.dtype)
    for lane in range(min(64, len(terms))):
        for t in terms[lane::64].reshape((-1,) + terms.shape[2:]):
            v[lane] = v[lane] + t
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ m]
    return v[0]
