// The dense algebra of the 3-, 6- and 9-unknown systems, once: everything the single-pose solver (pose_lm.hpp), the
// single-point solver (point_lm.hpp), the arrowhead solver (arrowhead.hpp, kernels_calibrate.hip) and the block
// elimination of the bundle adjustment (kernels_schur.hip, kernels_border.hip, kernels_lm.hip, kernels_cov.hip) do with a
// tiny symmetric matrix in one thread's registers.
//   tri6, finite_d / finite_bits / finite_v    packed lower indexing and the tests of finiteness
//   Packed, RowMajor<LD>                 where entry (i, j), i >= j, of a lower triangle lives
//   PivotPositive<BITS>, PivotUnchecked, PivotWeighted, PivotOrOne   what a pivot must satisfy
//   cholesky<N>                          L L^T = A, in place or not
//   forward_substitute / backward_substitute<N>, forward_block<N, NC>   L y = b, L^T x = y, L X = B
//   damped_solve<N, BITS>                (A + lam diag(max(A_ii, 1e-12))) step = -g
//   lower_inverse / lower_gram<N>, spd_inverse<N>, lower_inverse_full<N>   L^-1, M^T M, A^-1
//   lm_trials<N, NS, BITS, STOP_SMALL>   the Levenberg-Marquardt trial loop; max_abs<N>, cost_at_floor
// The header depends on nothing of the engine: under hipcc every function is __host__ __device__ __forceinline__ and
// lives in registers, under a plain C++ compiler it is inline, which is how tests/cpp/small_solve_test.cpp checks the
// algebra on the CPU.  Every sum has a fixed order: d -= L_jk^2 and v -= L_ik L_jk in ascending k, the square root of the
// pivot, one reciprocal per column.
#pragma once
#include <cmath>
#include <type_traits>

#if defined(__HIPCC__)
#define VMM_SMALL __host__ __device__ __forceinline__
#define VMM_UNROLL _Pragma("unroll")
#else
#define VMM_SMALL inline
#define VMM_UNROLL
#endif

namespace vmm {

constexpr double kLamInit = 1e-3, kLamMin = 1e-12, kLamMax = 1e12;

VMM_SMALL int tri6(int a, int b) { return a * (a + 1) / 2 + b; }   // a >= b: packed lower, any order

VMM_SMALL bool finite_d(double v) { return v - v == 0.0; }

// The same question asked of the bits.  finite_d's subtraction may be contracted with the arithmetic that produced v
// (v = a * b + c: v - v becomes fma(a, b, c - v), the rounding error of v instead of zero), which reports a perfectly
// finite v as non-finite; where that would be wrong rather than merely slow, ask this one.
VMM_SMALL bool finite_bits(double v) { return __builtin_isfinite(v); }

template <bool BITS>
VMM_SMALL bool finite_v(double v) { return BITS ? finite_bits(v) : finite_d(v); }

// ---- layouts: the index of entry (i, j), i >= j -------------------------------------------------

struct Packed {
    VMM_SMALL int operator()(int i, int j) const { return tri6(i, j); }
};

template <int LD>
struct RowMajor {
    VMM_SMALL int operator()(int i, int j) const { return LD * i + j; }
};

// ---- pivot policies: policy(j, d) sees the pivot before its square root, may replace it, returns whether it is good ----

template <bool BITS>
struct PivotPositive {
    VMM_SMALL bool operator()(int, double& d) const { return d > 0.0 && finite_v<BITS>(d); }
};

// No test per pivot: the caller tests what the factor produces (spd_inverse).
struct PivotUnchecked {
    VMM_SMALL bool operator()(int, double&) const { return true; }
};

// The pivot of a scaled matrix, judged in another scaling: d weight[j] must exceed min_pivot.
struct PivotWeighted {
    const double* weight;
    double min_pivot;
    VMM_SMALL bool operator()(int j, double& d) const { return d * weight[j] > min_pivot && finite_bits(d); }
};

// A bad pivot becomes 1 and the factorisation goes on with finite numbers; the caller reports the failure.
struct PivotOrOne {
    VMM_SMALL bool operator()(int, double& d) const
    {
        if (!(d > 0.0) || !finite_bits(d)) {
            d = 1.0;
            return false;
        }
        return true;
    }
};

// ---- factorisation -------------------------------------------------------------------------------

// L L^T = A for the lower triangle of an N x N A; A and L: anything indexable, and they may be the same array.  false:
// the policy refused a pivot (what L then holds is the policy's business).
template <int N, typename Layout, typename In, typename Out, typename Pivot>
VMM_SMALL bool cholesky(const In& A, Out& L, const Layout at, Pivot&& pivot)
{
    bool ok = true;
    VMM_UNROLL
    for (int j = 0; j < N; ++j) {
        double d = A[at(j, j)];
        VMM_UNROLL
        for (int k = 0; k < j; ++k)
            d -= L[at(j, k)] * L[at(j, k)];
        const bool good = pivot(j, d);
        ok = ok && good;
        const double s = sqrt(d);
        L[at(j, j)] = s;
        const double is = 1.0 / s;
        VMM_UNROLL
        for (int i = j + 1; i < N; ++i) {
            double v = A[at(i, j)];
            VMM_UNROLL
            for (int k = 0; k < j; ++k)
                v -= L[at(i, k)] * L[at(j, k)];
            L[at(i, j)] = v * is;
        }
    }
    return ok;
}

// ---- substitutions -------------------------------------------------------------------------------

// L y = b in ascending rows: y_i = (b(i) - sum_{k < i} L_ik y_k) / L_ii, handed to store(i, y_i) as it is found (a
// strided column, an array; b may read the array that store writes, row i is read before it is written).
template <int N, typename Layout, typename Lower, typename Rhs, typename Store>
VMM_SMALL void forward_substitute(const Lower& L, const Layout at, Rhs&& b, Store&& store)
{
    double y[N];
    VMM_UNROLL
    for (int i = 0; i < N; ++i) {
        double v = b(i);
        VMM_UNROLL
        for (int k = 0; k < i; ++k)
            v -= L[at(i, k)] * y[k];
        y[i] = v / L[at(i, i)];
        store(i, y[i]);
    }
}

// L^T x = y in descending rows: x_i = (y(i) - sum_{k > i} L_ki x_k) / L_ii; x may be the array y reads.
template <int N, typename Layout, typename Lower, typename Rhs>
VMM_SMALL void backward_substitute(const Lower& L, const Layout at, Rhs&& y, double* x)
{
    VMM_UNROLL
    for (int i = N - 1; i >= 0; --i) {
        double v = y(i);
        VMM_UNROLL
        for (int k = i + 1; k < N; ++k)
            v -= L[at(k, i)] * x[k];
        x[i] = v / L[at(i, i)];
    }
}

// X <- L^-1 X for a row-major N x NC X in place, a row at a time with one reciprocal per row.
template <int N, int NC, typename Layout, typename Lower>
VMM_SMALL void forward_block(const Lower& L, const Layout at, double (&X)[N * NC])
{
    VMM_UNROLL
    for (int r = 0; r < N; ++r) {
        const double inv = 1.0 / L[at(r, r)];
        VMM_UNROLL
        for (int c = 0; c < NC; ++c) {
            double t = X[NC * r + c];
            VMM_UNROLL
            for (int k = 0; k < r; ++k)
                t -= L[at(r, k)] * X[NC * k + c];
            X[NC * r + c] = t * inv;
        }
    }
}

// (A + lam diag(max(A_ii, 1e-12))) step = -g by Cholesky; A packed lower.  false: not positive definite, or the step is
// not finite.  BITS: test finiteness with finite_bits instead of finite_d.
template <int N, bool BITS>
VMM_SMALL bool damped_solve(const double (&A)[N * (N + 1) / 2], const double (&g)[N], const double lam, double (&step)[N])
{
    double L[N * (N + 1) / 2];
    VMM_UNROLL
    for (int k = 0; k < N * (N + 1) / 2; ++k)
        L[k] = A[k];
    VMM_UNROLL
    for (int a = 0; a < N; ++a) {
        const double d = A[tri6(a, a)];
        L[tri6(a, a)] = d + lam * (d > 1e-12 ? d : 1e-12);
    }
    bool ok = cholesky<N>(L, L, Packed{}, PivotPositive<BITS>{});
    double y[N];
    forward_substitute<N>(L, Packed{}, [&](const int i) { return -g[i]; }, [&](const int i, const double v) { y[i] = v; });
    backward_substitute<N>(L, Packed{}, [&](const int i) { return y[i]; }, step);
    VMM_UNROLL
    for (int i = 0; i < N; ++i)
        ok = ok && finite_v<BITS>(step[i]);
    return ok;
}

// ---- inverses --------------------------------------------------------------------------------------

// M = L^-1 for a packed lower N x N factor L (tri6 indexing; L: anything indexable, registers or memory).
template <int N, typename Lower>
VMM_SMALL void lower_inverse(const Lower& L, double (&M)[N * (N + 1) / 2])
{
    VMM_UNROLL
    for (int j = 0; j < N; ++j) {
        M[tri6(j, j)] = 1.0 / L[tri6(j, j)];
        VMM_UNROLL
        for (int i = j + 1; i < N; ++i) {
            double v = 0.0;
            VMM_UNROLL
            for (int k = j; k < i; ++k)
                v -= L[tri6(i, k)] * M[tri6(k, j)];
            M[tri6(i, j)] = v / L[tri6(i, i)];
        }
    }
}

// C = M^T M (packed lower) for a packed lower N x N M; returns sum |C_ab| over the packed entries: finite exactly when
// every entry is.
template <int N>
VMM_SMALL double lower_gram(const double (&M)[N * (N + 1) / 2], double (&C)[N * (N + 1) / 2])
{
    double sum = 0.0;
    VMM_UNROLL
    for (int a = 0; a < N; ++a)
        VMM_UNROLL
        for (int b = 0; b <= a; ++b) {
            double v = 0.0;
            VMM_UNROLL
            for (int k = a; k < N; ++k)
                v += M[tri6(k, a)] * M[tri6(k, b)];
            C[tri6(a, b)] = v;
            sum += fabs(v);
        }
    return sum;
}

// C = A^-1 for a packed lower N x N A by Cholesky, in registers; false: not positive definite (C is not valid).
// One test at the end covers every pivot that is negative, zero or NaN: a negative pivot makes its square root a NaN and
// a zero pivot its reciprocal an infinity, and either reaches the last entry of every later row of L^-1 and from there
// C.  It does not cover a pivot of +inf (a diagonal entry of +inf: the square root is +inf, its reciprocal zero, and the
// row and column come out as zeros): a caller whose sums can overflow passes PivotPositive<true> and gets the test per
// pivot as well, as the point covariance of kernels_triangulate.hip does.
template <int N, typename Pivot = PivotUnchecked>
VMM_SMALL bool spd_inverse(const double (&A)[N * (N + 1) / 2], double (&C)[N * (N + 1) / 2])
{
    double L[N * (N + 1) / 2], M[N * (N + 1) / 2];   // A = L L^T, M = L^-1 (lower)
    const bool ok = cholesky<N>(A, L, Packed{}, Pivot{});
    lower_inverse<N>(L, M);
    return finite_bits(lower_gram<N>(M, C)) && ok;
}

// T = L^-1 as a full N x N matrix (zeros above the diagonal) for a lower factor in any layout, column by column.
template <int N, typename Layout, typename Lower>
VMM_SMALL void lower_inverse_full(const Lower& L, const Layout at, double (&T)[N][N])
{
    for (int c = 0; c < N; ++c)
        for (int r = 0; r < N; ++r) {
            if (r < c) {
                T[r][c] = 0.0;
                continue;
            }
            double s = (r == c) ? 1.0 : 0.0;
            for (int m = c; m < r; ++m)
                s -= L[at(r, m)] * T[m][c];
            T[r][c] = s / L[at(r, r)];
        }
}

// ---- the Levenberg-Marquardt trial loop ---------------------------------------------------------------

template <int N>
VMM_SMALL double max_abs(const double (&s)[N])
{
    double m = 0.0;
    VMM_UNROLL
    for (int k = 0; k < N; ++k)
        m = fabs(s[k]) > m ? fabs(s[k]) : m;
    return m;
}

// A rejected LM trial whose cost equals the current one to rounding (pixel coordinates of a few thousand carry 1e-12
// relative noise into a squared residual): the minimum is reached; raising the damping further would only repeat it.
VMM_SMALL bool cost_at_floor(const double cost, const double cand)
{
    return cand - cost <= 1e-10 * cost + 1e-20;
}

// Levenberg-Marquardt over N unknowns of a state x of NS doubles (in place), at most max_trials trials (accepted +
// rejected); returns the trials spent.  sums(jac, x, A, g) returns the cost at x (+inf: not admissible, the trial is
// rejected) and, when jac is std::true_type, fills J^T J (packed lower) and J^T r; plus(x, step, cand) applies a step.
// cost receives the cost of the last evaluation with Jacobians: that of x, except after the STOP_SMALL exit, where it is
// the cost before the last accepted step.
// STOP_SMALL: also stop after an accepted step below 1e-9 (an initial guess for the bundle adjustment needs no more).
// BITS: test finiteness with finite_bits instead of finite_d.
// The invariant every caller keeps: all threads that run the driver together (a lane alone, a wave, or a workgroup when
// sums contains a barrier) hold the same sums, so they take the same branches and reach the same barriers.
template <int N, int NS, bool BITS, bool STOP_SMALL, typename State, typename Sums, typename Plus>
VMM_SMALL int lm_trials(State&& x, const int max_trials, Sums&& sums, Plus&& plus, double& cost)
{
    double cand[NS], A[N * (N + 1) / 2], g[N], step[N];
    double lam = kLamInit;
    cost = sums(std::true_type{}, x, A, g);
    int it = 0;
    for (; it < max_trials; ++it) {
        if (!finite_v<BITS>(cost) || lam > kLamMax)
            break;
        if (!damped_solve<N, BITS>(A, g, lam, step)) {
            lam *= 10.0;
            continue;
        }
        const double sm = max_abs<N>(step);
        if (sm < 1e-14)
            break;
        plus(x, step, cand);
        double A2[N * (N + 1) / 2], g2[N];
        const double cc = sums(std::false_type{}, cand, A2, g2);
        if (finite_v<BITS>(cc) && cc < cost) {
            VMM_UNROLL
            for (int k = 0; k < NS; ++k)
                x[k] = cand[k];
            lam = lam * 0.1 > kLamMin ? lam * 0.1 : kLamMin;
            if (STOP_SMALL && sm < 1e-9)
                break;
            cost = sums(std::true_type{}, x, A, g);
        } else {
            if (sm < 1e-10 || cost_at_floor(cost, cc))
                break;
            lam *= 10.0;
        }
    }
    return it;
}

} // namespace vmm
