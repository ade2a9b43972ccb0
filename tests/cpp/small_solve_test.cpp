// The small dense algebra of visual_marker_mapping_amd/csrc/small_solve.hpp on the CPU, from the header alone (no HIP,
// no libvmm_ba).  Reads cases on stdin, one per line, and prints one line of results per case with 17 significant
// digits; tests/test_small_solve_cpu.py generates the cases and compares with numpy.  A matrix is given as the N x N
// doubles of its rows; only the lower triangle is read.
//   factor <N> <p|r> A               -> ok, L (N x N rows, zeros above)         PivotPositive<true>; p: packed, r: row-major
//   solve <N> <p|r> A b              -> ok, x                                   cholesky + forward + backward substitution
//   block A X                        -> L^-1 X (6 x 6 rows)                     row-major cholesky + forward_block<6, 6>
//   invfull A                        -> L^-1 (6 x 6 rows)                       row-major cholesky + lower_inverse_full<6>
//   inverse <N> A                    -> ok (spd_inverse), ok (per pivot as well), ok (the rule inverse3 had), C (N x N rows)
//   damped <N> <lam> A g             -> ok (BITS), ok (not BITS), step
//   policy <N> <name> A [w.. min]    -> ok, 1 when every entry of L is finite   positive | bits | orone | weighted
//   lm <N> <stop_small> <mode> <max_trials> <m> J (m x N rows) b x0
//                                    -> trials, cost, the cost evaluated again at the returned x, x
//                                       sums: |J x - b|^2, J^T J, J^T (J x - b); mode inf: +inf for every candidate
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "small_solve.hpp"

using namespace vmm;

namespace {

void put(const double v) { std::printf(" %.17g", v); }

// operator>> does not read "nan" and "inf"; strtod does
double get()
{
    std::string t;
    std::cin >> t;
    return std::strtod(t.c_str(), nullptr);
}

template <int N>
void read_packed(double (&A)[N * (N + 1) / 2], double (&full)[N * N])
{
    for (int k = 0; k < N * N; ++k)
        full[k] = get();
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j)
            A[tri6(i, j)] = full[N * i + j];
}

template <int N>
void put_lower(const double* L, const bool packed)
{
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            put(j <= i ? L[packed ? tri6(i, j) : N * i + j] : 0.0);
}

template <int N>
void factor_case(const bool packed, const bool solve)
{
    double A[N * (N + 1) / 2], full[N * N], b[N], x[N], y[N];
    read_packed<N>(A, full);
    if (solve)
        for (int k = 0; k < N; ++k)
            b[k] = get();
    bool ok;
    if (packed) {
        double L[N * (N + 1) / 2];
        ok = cholesky<N>(A, L, Packed{}, PivotPositive<true>{});
        std::printf("%d", ok ? 1 : 0);
        if (!solve)
            return put_lower<N>(L, true);
        forward_substitute<N>(L, Packed{}, [&](const int i) { return b[i]; }, [&](const int i, const double v) { y[i] = v; });
        backward_substitute<N>(L, Packed{}, [&](const int i) { return y[i]; }, x);
    } else {   // in place, as k_form_z factors
        ok = cholesky<N>(full, full, RowMajor<N>{}, PivotPositive<true>{});
        std::printf("%d", ok ? 1 : 0);
        if (!solve)
            return put_lower<N>(full, false);
        forward_substitute<N>(full, RowMajor<N>{}, [&](const int i) { return b[i]; }, [&](const int i, const double v) { b[i] = v; });
        backward_substitute<N>(full, RowMajor<N>{}, [&](const int i) { return b[i]; }, x);
    }
    for (int k = 0; k < N; ++k)
        put(x[k]);
}

void block_case(const bool inverse)
{
    double L[36], X[36], T[6][6];
    for (int k = 0; k < 36; ++k)
        L[k] = get();
    if (!inverse)
        for (int k = 0; k < 36; ++k)
            X[k] = get();
    const bool ok = cholesky<6>(L, L, RowMajor<6>{}, PivotOrOne{});
    std::printf("%d", ok ? 1 : 0);
    if (inverse) {
        lower_inverse_full<6>(L, RowMajor<6>{}, T);
        for (int k = 0; k < 36; ++k)
            put(T[k / 6][k % 6]);
    } else {
        forward_block<6, 6>(L, RowMajor<6>{}, X);
        for (int k = 0; k < 36; ++k)
            put(X[k]);
    }
}

template <int N>
void inverse_case()
{
    constexpr int T = N * (N + 1) / 2;
    double A[T], full[N * N], C[T], C2[T], L[T], M[T], G[T];
    read_packed<N>(A, full);
    const bool one_rule = spd_inverse<N>(A, C);
    const bool per_pivot = spd_inverse<N, PivotPositive<true>>(A, C2);
    // what inverse3 did: its own pivot tests next to the test of the Gram sum
    const bool ok = cholesky<N>(A, L, Packed{}, PivotPositive<true>{});
    lower_inverse<N>(L, M);
    const bool old_rule = finite_bits(lower_gram<N>(M, G)) && ok;
    std::printf("%d %d %d", one_rule ? 1 : 0, per_pivot ? 1 : 0, old_rule ? 1 : 0);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            put(i >= j ? C[tri6(i, j)] : C[tri6(j, i)]);
}

template <int N>
void damped_case()
{
    double lam, A[N * (N + 1) / 2], full[N * N], g[N], step[N], step2[N];
    lam = get();
    read_packed<N>(A, full);
    for (int k = 0; k < N; ++k)
        g[k] = get();
    const bool ok = damped_solve<N, true>(A, g, lam, step);
    const bool ok2 = damped_solve<N, false>(A, g, lam, step2);
    std::printf("%d %d", ok ? 1 : 0, ok2 ? 1 : 0);
    for (int k = 0; k < N; ++k)
        put(step[k]);
}

template <int N>
void policy_case()
{
    constexpr int T = N * (N + 1) / 2;
    std::string name;
    std::cin >> name;
    double A[T], full[N * N], L[T], w[N], min_pivot = 0.0;
    read_packed<N>(A, full);
    bool ok = false;
    if (name == "positive")
        ok = cholesky<N>(A, L, Packed{}, PivotPositive<false>{});
    else if (name == "bits")
        ok = cholesky<N>(A, L, Packed{}, PivotPositive<true>{});
    else if (name == "orone")
        ok = cholesky<N>(A, L, Packed{}, PivotOrOne{});
    else {
        for (int k = 0; k < N; ++k)
            w[k] = get();
        min_pivot = get();
        ok = cholesky<N>(A, L, Packed{}, PivotWeighted{ w, min_pivot });
    }
    bool finite = true;
    for (int k = 0; k < T; ++k)
        finite = finite && finite_bits(L[k]);
    std::printf("%d %d", ok ? 1 : 0, finite ? 1 : 0);
}

template <int N, bool STOP_SMALL>
void lm_case()
{
    std::string mode;
    int max_trials, m;
    std::cin >> mode >> max_trials >> m;
    std::vector<double> J(m * N), b(m);
    double x[N];
    for (double& v : J)
        v = get();
    for (double& v : b)
        v = get();
    for (int k = 0; k < N; ++k)
        x[k] = get();
    auto sums = [&](auto jac, const double (&at)[N], double (&A)[N * (N + 1) / 2], double (&g)[N]) {
        if (mode == "inf" && !decltype(jac)::value)
            return (double)__builtin_huge_val();
        double cost = 0.0;
        for (int k = 0; k < N * (N + 1) / 2; ++k)
            A[k] = 0.0;
        for (int k = 0; k < N; ++k)
            g[k] = 0.0;
        for (int r = 0; r < m; ++r) {
            double res = -b[r];
            for (int k = 0; k < N; ++k)
                res += J[N * r + k] * at[k];
            cost += res * res;
            if (decltype(jac)::value)
                for (int i = 0; i < N; ++i) {
                    g[i] += J[N * r + i] * res;
                    for (int k = 0; k <= i; ++k)
                        A[tri6(i, k)] += J[N * r + i] * J[N * r + k];
                }
        }
        return cost;
    };
    double cost;
    const int trials = lm_trials<N, N, true, STOP_SMALL>(
        x, max_trials, sums,
        [](const double (&at)[N], const double (&step)[N], double (&cand)[N]) {
            for (int k = 0; k < N; ++k)
                cand[k] = at[k] + step[k];
        },
        cost);
    double A[N * (N + 1) / 2], g[N];
    std::printf("%d", trials);
    put(cost);
    put(sums(std::true_type{}, x, A, g));
    for (int k = 0; k < N; ++k)
        put(x[k]);
}

template <int N>
void dispatch(const std::string& cmd)
{
    std::string layout;
    int stop_small;
    if (cmd == "factor" || cmd == "solve") {
        std::cin >> layout;
        factor_case<N>(layout == "p", cmd == "solve");
    } else if (cmd == "inverse") {
        inverse_case<N>();
    } else if (cmd == "damped") {
        damped_case<N>();
    } else if (cmd == "policy") {
        policy_case<N>();
    } else if (cmd == "lm") {
        std::cin >> stop_small;
        if (stop_small)
            lm_case<N, true>();
        else
            lm_case<N, false>();
    }
}

} // namespace

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "block" || cmd == "invfull") {
            block_case(cmd == "invfull");
        } else {
            int n;
            std::cin >> n;
            if (n == 3)
                dispatch<3>(cmd);
            else if (n == 6)
                dispatch<6>(cmd);
            else if (n == 9)
                dispatch<9>(cmd);
            else
                return 2;
        }
        std::printf("\n");
        if (!std::cin)
            return 3;
    }
    return 0;
}
