// The single-pose solver shared by kernels_init.hip (map initialisation), kernels_localize.hip (localisation against
// a finished map), kernels_locate.hip (a tag from known cameras) and, through image_sums.hpp and the pieces named below,
// kernels_calibrate.hip: fit one 6-degree-of-freedom pose to pixel corners after picking the best of a list of candidates.
//   lm_refine               the Levenberg-Marquardt trial loop over a pose's six tangent unknowns (small_solve.hpp's
//                           lm_trials with pose_plus as the update); the caller supplies the sums (cost, J^T J, J^T r)
//   project_camera_point    camera-side projection of a rotated point with its 2 x 6 Jacobian over the pose's tangent
//   project_camera_point_intrinsics   the same with the 2 x 9 Jacobian over the camera model (kernels_calibrate.hip)
//   better / wave_winner    the candidate winner rule and its wave butterfly
//   zero_normal / wave_sum_normal, accumulate_rows   the 21 + 6 sums of the normal equations
//   chain_camera / chain_tag, quat_from_R                    candidates chained through a placed pose
//   sym6 / sandwich6        C S C of two packed symmetric 6 x 6 matrices (kernels_locate.hip, kernels_predict.hip)
// The algebra under it is small_solve.hpp's: tri6 and the tests of finiteness, the damped solve of the normal equations
// (damped_solve<6, BITS>), the covariance of one pose (spd_inverse<6>: kernels_localize.hip, kernels_rig.hip) and
// lower_inverse / lower_gram (kernels_calibrate.hip, arrowhead.hpp).
// Everything is __forceinline__ and lives in registers.
#pragma once
#include "geom.hpp"
#include "small_solve.hpp"

namespace vmm {

constexpr double kInf = __builtin_huge_val();

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

// Levenberg-Marquardt over the 6 tangent degrees of freedom of q (7 doubles, in place): lm_trials (small_solve.hpp)
// with pose_plus as the update; sums(jac, q, A, g) as described there.
template <bool BITS, bool STOP_SMALL, typename Sums>
__device__ __forceinline__ int lm_refine(double* q, const int max_trials, Sums&& sums, double& cost)
{
    return lm_trials<6, 7, BITS, STOP_SMALL>(q, max_trials, sums,
                                             [](const double* at, const double (&step)[6], double (&cand)[7]) { pose_plus(at, step, cand); }, cost);
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

// entry (r, c) of a symmetric 6 x 6 matrix held packed lower
__device__ __forceinline__ double sym6(const double (&P)[21], const int r, const int c) { return r >= c ? P[tri6(r, c)] : P[tri6(c, r)]; }

// C S C (packed lower) of two symmetric 6 x 6 matrices; entry (r, c) is averaged with its mirror image, so that the
// stored matrix is symmetric whatever the rounding.  Returns whether every entry is finite.
__device__ __forceinline__ bool sandwich6(const double (&C)[21], const double (&S)[21], double (&CC)[21])
{
    double T[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                t += sym6(C, r, k) * sym6(S, k, c);
            T[r][c] = t;
        }
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double x = 0.0, y = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                x += T[r][k] * sym6(C, k, c);
                y += T[c][k] * sym6(C, k, r);
            }
            CC[tri6(r, c)] = 0.5 * (x + y);
            sum += fabs(CC[tri6(r, c)]);
        }
    return finite_bits(sum);
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
