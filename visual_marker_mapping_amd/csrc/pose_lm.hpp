// The single-pose solver shared by kernels_init.hip (map initialisation), kernels_localize.hip (localisation against
// a finished map) and, through image_sums.hpp and the pieces named below, kernels_calibrate.hip: fit one
// 6-degree-of-freedom pose to pixel corners after picking the best of a list of candidates.
//   lm_refine               the Levenberg-Marquardt trial loop; the caller supplies the sums (cost, J^T J, J^T r)
//   project_camera_point    camera-side projection of a rotated point with its 2 x 6 Jacobian over the pose's tangent
//   project_camera_point_intrinsics   the same with the 2 x 9 Jacobian over the camera model (kernels_calibrate.hip)
//   better / wave_winner    the candidate winner rule and its wave butterfly
//   zero_normal / wave_sum_normal, accumulate_rows, solve6   the 21 + 6 sums of the normal equations and their solve
//   lower_inverse / lower_gram   L^-1 and M^T M of packed lower matrices: the covariances of kernels_localize.hip (6 x 6)
//                                and kernels_calibrate.hip (6 x 6 and 9 x 9)
//   inverse6                the 6 x 6 covariance of one pose (kernels_localize.hip, kernels_rig.hip)
//   chain_camera / chain_tag, quat_from_R                    candidates chained through a placed pose
// Everything is __forceinline__ and lives in registers.
#pragma once
#include <type_traits>

#include "geom.hpp"

namespace vmm {

constexpr double kInf = __builtin_huge_val();
constexpr double kLamInit = 1e-3, kLamMin = 1e-12, kLamMax = 1e12;

__device__ __forceinline__ int tri6(int a, int b) { return a * (a + 1) / 2 + b; }   // a >= b: packed lower, any order

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// The same question asked of the bits.  finite_d's subtraction may be contracted with the arithmetic that produced v
// (v = a * b + c: v - v becomes fma(a, b, c - v), the rounding error of v instead of zero), which reports a perfectly
// finite v as non-finite; where that would be wrong rather than merely slow, ask this one.
__device__ __forceinline__ bool finite_bits(double v) { return __builtin_isfinite(v); }

template <bool BITS>
__device__ __forceinline__ bool finite_v(double v) { return BITS ? finite_bits(v) : finite_d(v); }

// Eigen::Quaterniond(R) (trace test), normalised; R row-major.
__device__ __forceinline__ void quat_from_R(const double* R, double* q)
{
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z;
    if (tr > 0.0) {
        const double s = sqrt(tr + 1.0) * 2.0;
        w = 0.25 * s;
        x = (R[7] - R[5]) / s;
        y = (R[2] - R[6]) / s;
        z = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = sqrt(R[0] - R[4] - R[8] + 1.0) * 2.0;
        w = (R[7] - R[5]) / s;
        x = 0.25 * s;
        y = (R[3] + R[1]) / s;
        z = (R[6] + R[2]) / s;
    } else if (R[4] >= R[8]) {
        const double s = sqrt(R[4] - R[8] - R[0] + 1.0) * 2.0;
        w = (R[2] - R[6]) / s;
        x = (R[3] + R[1]) / s;
        y = 0.25 * s;
        z = (R[7] + R[5]) / s;
    } else {
        const double s = sqrt(R[8] - R[0] - R[4] + 1.0) * 2.0;
        w = (R[3] - R[1]) / s;
        x = (R[6] + R[2]) / s;
        y = (R[7] + R[5]) / s;
        z = 0.25 * s;
    }
    const double n = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    q[0] = w * n;
    q[1] = x * n;
    q[2] = y * n;
    q[3] = z * n;
}

// T_cam = T_rel o T_tag^-1 (rel: tag->camera, tag: tag->world, result: world->camera)
__device__ __forceinline__ void chain_camera(const Rigid& rel, const Rigid& tag, Rigid& cam)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            cam.R[3 * i + j] = rel.R[3 * i] * tag.R[3 * j] + rel.R[3 * i + 1] * tag.R[3 * j + 1] + rel.R[3 * i + 2] * tag.R[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        cam.t[i] = rel.t[i] - (cam.R[3 * i] * tag.t[0] + cam.R[3 * i + 1] * tag.t[1] + cam.R[3 * i + 2] * tag.t[2]);
}

// T_tag = T_cam^-1 o T_rel
__device__ __forceinline__ void chain_tag(const Rigid& rel, const Rigid& cam, Rigid& tag)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            tag.R[3 * i + j] = cam.R[i] * rel.R[j] + cam.R[3 + i] * rel.R[3 + j] + cam.R[6 + i] * rel.R[6 + j];
    const double d0 = rel.t[0] - cam.t[0], d1 = rel.t[1] - cam.t[1], d2 = rel.t[2] - cam.t[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        tag.t[i] = cam.R[i] * d0 + cam.R[3 + i] * d1 + cam.R[6 + i] * d2;
}

// (A + lam diag(max(A_ii, 1e-12))) step = -g by Cholesky; A packed lower (tri6).  false: not positive definite.
// BITS: test finiteness with finite_bits instead of finite_d.
template <bool BITS>
__device__ __forceinline__ bool solve6(const double (&A)[21], const double (&g)[6], const double lam, double (&step)[6])
{
    double L[21];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        L[k] = A[k];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double d = A[tri6(a, a)];
        L[tri6(a, a)] = d + lam * (d > 1e-12 ? d : 1e-12);
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = L[tri6(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k)
            d -= L[tri6(j, k)] * L[tri6(j, k)];
        ok = ok && d > 0.0 && finite_v<BITS>(d);
        const double s = sqrt(d);
        L[tri6(j, j)] = s;
        const double is = 1.0 / s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = L[tri6(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k)
                v -= L[tri6(i, k)] * L[tri6(j, k)];
            L[tri6(i, j)] = v * is;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k)
            v -= L[tri6(i, k)] * y[k];
        y[i] = v / L[tri6(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k)
            v -= L[tri6(k, i)] * step[k];
        step[i] = v / L[tri6(i, i)];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
        ok = ok && finite_v<BITS>(step[i]);
    return ok;
}

// M = L^-1 for a packed lower N x N factor L (tri6 indexing; L: anything indexable, registers or memory).
template <int N, typename Lower>
__device__ __forceinline__ void lower_inverse(const Lower& L, double (&M)[N * (N + 1) / 2])
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        M[tri6(j, j)] = 1.0 / L[tri6(j, j)];
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k)
                v -= L[tri6(i, k)] * M[tri6(k, j)];
            M[tri6(i, j)] = v / L[tri6(i, i)];
        }
    }
}

// C = M^T M (packed lower) for a packed lower N x N M; returns sum |C_ab| over the packed entries: finite exactly when
// every entry is.
template <int N>
__device__ __forceinline__ double lower_gram(const double (&M)[N * (N + 1) / 2], double (&C)[N * (N + 1) / 2])
{
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            double v = 0.0;
#pragma unroll
            for (int k = a; k < N; ++k)
                v += M[tri6(k, a)] * M[tri6(k, b)];
            C[tri6(a, b)] = v;
            sum += fabs(v);
        }
    return sum;
}

// C = A^-1 for a packed lower 6 x 6 A by Cholesky, in registers; false: not positive definite (C is not valid).
// One test at the end covers every pivot: a negative pivot makes its square root a NaN and a zero pivot its reciprocal
// an infinity, and either reaches the last entry of every later row of L^-1 and from there C.
__device__ __forceinline__ bool inverse6(const double (&A)[21], double (&C)[21])
{
    double L[21], M[21];   // A = L L^T, M = L^-1 (lower)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[tri6(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k)
            d -= L[tri6(j, k)] * L[tri6(j, k)];
        const double s = sqrt(d);
        L[tri6(j, j)] = s;
        const double is = 1.0 / s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[tri6(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k)
                v -= L[tri6(i, k)] * L[tri6(j, k)];
            L[tri6(i, j)] = v * is;
        }
    }
    lower_inverse<6>(L, M);
    return finite_bits(lower_gram<6>(M, C));
}

__device__ __forceinline__ void accumulate_rows(const double (&j)[2][6], const double ru, const double rv, double (&A)[21],
                                                double (&g)[6])
{
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        g[a] += j[0][a] * ru + j[1][a] * rv;
#pragma unroll
        for (int b = 0; b <= a; ++b)
            A[tri6(a, b)] += j[0][a] * j[0][b] + j[1][a] * j[1][b];
    }
}

__device__ __forceinline__ void zero_normal(double (&A)[21], double (&g)[6])
{
#pragma unroll
    for (int k = 0; k < 21; ++k)
        A[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        g[k] = 0.0;
}

// every lane ends with the wave's totals (wave_sum's fixed butterfly)
__device__ __forceinline__ void wave_sum_normal(double (&A)[21], double (&g)[6])
{
#pragma unroll
    for (int k = 0; k < 21; ++k)
        A[k] = wave_sum(A[k]);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        g[k] = wave_sum(g[k]);
}

__device__ __forceinline__ double max_abs6(const double (&s)[6])
{
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        m = fabs(s[k]) > m ? fabs(s[k]) : m;
    return m;
}

// A rejected LM trial whose cost equals the current one to rounding (pixel coordinates of a few thousand carry 1e-12
// relative noise into a squared residual): the minimum is reached; raising the damping further would only repeat it.
__device__ __forceinline__ bool cost_at_floor(const double cost, const double cand)
{
    return cand - cost <= 1e-10 * cost + 1e-20;
}

// Levenberg-Marquardt over the 6 tangent degrees of freedom of q (in place), at most max_trials trials (accepted +
// rejected); returns the trials spent.  sums(jac, q, A, g) returns the cost at q and, when jac is std::true_type, fills
// J^T J (packed lower) and J^T r.  cost receives the cost of the last evaluation with Jacobians: that of q, except
// after the STOP_SMALL exit, where it is the cost before the last accepted step.
// STOP_SMALL: also stop after an accepted step below 1e-9 (an initial guess for the bundle adjustment needs no more).
// BITS: test finiteness with finite_bits instead of finite_d.
// The invariant every caller keeps: all threads that run the driver together (a lane alone, a wave, or a workgroup when
// sums contains __syncthreads) hold the same sums, so they take the same branches and reach the same barriers.
template <bool BITS, bool STOP_SMALL, typename Sums>
__device__ __forceinline__ int lm_refine(double* q, const int max_trials, Sums&& sums, double& cost)
{
    double cand[7], A[21], g[6], step[6];
    double lam = kLamInit;
    cost = sums(std::true_type{}, q, A, g);
    int it = 0;
    for (; it < max_trials; ++it) {
        if (!finite_v<BITS>(cost) || lam > kLamMax)
            break;
        if (!solve6<BITS>(A, g, lam, step)) {
            lam *= 10.0;
            continue;
        }
        const double sm = max_abs6(step);
        if (sm < 1e-14)
            break;
        pose_plus(q, step, cand);
        double A2[21], g2[6];
        const double cc = sums(std::false_type{}, cand, A2, g2);
        if (finite_v<BITS>(cc) && cc < cost) {
#pragma unroll
            for (int k = 0; k < 7; ++k)
                q[k] = cand[k];
            lam = lam * 0.1 > kLamMin ? lam * 0.1 : kLamMin;
            if (STOP_SMALL && sm < 1e-9)
                break;
            cost = sums(std::true_type{}, q, A, g);
        } else {
            if (sm < 1e-10 || cost_at_floor(cost, cc))
                break;
            lam *= 10.0;
        }
    }
    return it;
}

// The camera half of eval_corner (geom.hpp) on a point already rotated into the camera frame, b = R P: residual of
// the projection of b + t against the observed pixel and, with JAC, the 2 x 6 Jacobian over the pose's tangent
// (translation, half-angle rotation).  CAMERA_MODEL: project like CameraModel::projectPoint (src/CameraModel.cpp:6-26,
// what vmm_ba_project_points computes); eval_corner has no Jacobian for that projection -- it is the functor's with the
// two entries of d(yd)/d(x, y) that the aliased term 2 p2 (xd - x) y adds.
template <bool CAMERA_MODEL, bool JAC>
__device__ __forceinline__ void project_camera_point(const Intrinsics& K, const double b0, const double b1, const double b2,
                                                     const double (&t)[3], const double u_obs, const double v_obs, double& ru,
                                                     double& rv, double (&j)[2][6])
{
    const double iz = 1.0 / (b2 + t[2]);
    const double x = (b0 + t[0]) * iz, y = (b1 + t[1]) * iz;
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (K.k1 + r2 * (K.k2 + r2 * K.k3));
    double xd, yd;
    distort(K, CAMERA_MODEL, x, y, r2, rad, xd, yd);
    ru = K.fx * xd + K.cx - u_obs;
    rv = K.fy * yd + K.cy - v_obs;
    if (!JAC)
        return;
    const double dr = K.k1 + r2 * (2.0 * K.k2 + 3.0 * K.k3 * r2);
    const double D00 = rad + 2.0 * x * x * dr + 2.0 * K.p1 * y + 6.0 * K.p2 * x;
    const double D01 = 2.0 * x * y * dr + 2.0 * K.p1 * x + 2.0 * K.p2 * y;
    double D10 = D01, D11 = rad + 2.0 * y * y * dr + 2.0 * K.p2 * x + 6.0 * K.p1 * y;
    if (CAMERA_MODEL) {
        D10 = D01 + 2.0 * K.p2 * y * (D00 - 1.0);
        D11 = D11 + 2.0 * K.p2 * (xd - x) + 2.0 * K.p2 * y * D01;
    }
    const double g[2][3] = { { K.fx * D00 * iz, K.fx * D01 * iz, -K.fx * (D00 * x + D01 * y) * iz },
                             { K.fy * D10 * iz, K.fy * D11 * iz, -K.fy * (D10 * x + D11 * y) * iz } };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        j[r][0] = g[r][0];
        j[r][1] = g[r][1];
        j[r][2] = g[r][2];
        j[r][3] = 2.0 * (b1 * g[r][2] - b2 * g[r][1]);
        j[r][4] = 2.0 * (b2 * g[r][0] - b0 * g[r][2]);
        j[r][5] = 2.0 * (b0 * g[r][1] - b1 * g[r][0]);
    }
}

// project_camera_point<false, true> and, next to it, the 2 x 9 Jacobian of the same residual over the camera model in
// the order of Intrinsics (fx, fy, cx, cy, k1, k2, p1, p2, k3).  The residual and the pose Jacobian are the existing
// function's; the normalised point is formed again with the same expressions for the intrinsic columns.
__device__ __forceinline__ void project_camera_point_intrinsics(const Intrinsics& K, const double b0, const double b1,
                                                                const double b2, const double (&t)[3], const double u_obs,
                                                                const double v_obs, double& ru, double& rv,
                                                                double (&j)[2][6], double (&jk)[2][9])
{
    project_camera_point<false, true>(K, b0, b1, b2, t, u_obs, v_obs, ru, rv, j);
    const double iz = 1.0 / (b2 + t[2]);
    const double x = (b0 + t[0]) * iz, y = (b1 + t[1]) * iz;
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (K.k1 + r2 * (K.k2 + r2 * K.k3));
    double xd, yd;
    distort(K, false, x, y, r2, rad, xd, yd);
    const double r4 = r2 * r2, r6 = r4 * r2, xy2 = 2.0 * x * y;
    const double fxx = K.fx * x, fyy = K.fy * y;
    jk[0][0] = xd;
    jk[1][0] = 0.0;
    jk[0][1] = 0.0;
    jk[1][1] = yd;
    jk[0][2] = 1.0;
    jk[1][2] = 0.0;
    jk[0][3] = 0.0;
    jk[1][3] = 1.0;
    jk[0][4] = fxx * r2;
    jk[1][4] = fyy * r2;
    jk[0][5] = fxx * r4;
    jk[1][5] = fyy * r4;
    jk[0][6] = K.fx * xy2;
    jk[1][6] = K.fy * (r2 + 2.0 * y * y);
    jk[0][7] = K.fx * (r2 + 2.0 * x * x);
    jk[1][7] = K.fy * xy2;
    jk[0][8] = fxx * r6;
    jk[1][8] = fyy * r6;
}

// The candidate winner rule: the lowest score wins, ties go to the lowest index, NaN and +inf lose (a thread that found
// no candidate holds (kInf, INT_MAX)).  better: whether (score, index) beats (other_score, other_index).
__device__ __forceinline__ bool better(const double score, const int index, const double other_score, const int other_index)
{
    return score < other_score || (score == other_score && index < other_index);
}

// the wave's winner in every lane; the waves of a workgroup then meet in LDS and are taken in wave order
__device__ __forceinline__ void wave_winner(double& best, int& best_c)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(best, m, 64);
        const int oc = __shfl_xor(best_c, m, 64);
        if (better(os, oc, best, best_c)) {
            best = os;
            best_c = oc;
        }
    }
}

__device__ __forceinline__ double corner_sx(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }   // LL, LR, UR, UL
__device__ __forceinline__ double corner_sy(int k) { return k >= 2 ? 1.0 : -1.0; }

} // namespace vmm
