// The single-point solver of kernels_triangulate.hip: the 3-degree-of-freedom sibling of pose_lm.hpp's single-pose
// solver.  Fit one world point to its pixels in cameras that are known.
//   undistort_pixel        pixel -> undistorted normalised image point (fixed-point iteration of the functor's distortion)
//   project_world_point    residual of a world point in one camera frame, the depth, and with JAC the 2 x 6 camera
//                          Jacobian (project_camera_point<false, true>'s columns) and the 2 x 3 point Jacobian
//   spd3_solve             A x = b for a packed lower 3 x 3 A by Cholesky with a floor on the pivots (the ray intersections)
//   lm_refine3             the Levenberg-Marquardt trial loop over the three coordinates (small_solve.hpp's lm_trials)
// The covariance is small_solve.hpp's spd_inverse<3, PivotPositive<true>>.
//   wave_count             butterfly sum of an int over the wave
// Every test of finiteness asks the bits (finite_bits, small_solve.hpp): v - v == 0 misfires when the compiler contracts
// the subtraction with the arithmetic that produced v.
// Everything is __forceinline__ and lives in registers.  Packed lower 3 x 3 matrices use tri6's indexing.
#pragma once
#include "pose_lm.hpp"

namespace vmm {

constexpr int kPointUndistortIters = 20;

// (u, v) -> (x, y) with distort(K, false, x, y, ...) = ((u - cx) / fx, (v - cy) / fy): the iteration x <- (x0 - dx) / rad
// that k_quad_pose (kernels_init.hip) runs on a tag's corners, written anew here.
__device__ __forceinline__ void undistort_pixel(const Intrinsics& K, const double u, const double v, double& x, double& y)
{
    const double x0 = (u - K.cx) / K.fx, y0 = (v - K.cy) / K.fy;
    x = x0;
    y = y0;
    for (int it = 0; it < kPointUndistortIters; ++it) {
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (K.k1 + r2 * (K.k2 + r2 * K.k3));
        const double dx = 2.0 * K.p1 * x * y + K.p2 * (r2 + 2.0 * x * x);
        const double dy = K.p1 * (r2 + 2.0 * y * y) + 2.0 * K.p2 * x * y;
        x = (x0 - dx) / rad;
        y = (y0 - dy) / rad;
    }
}

// World point X in the camera frame f = R (9, row-major) | t (3): the residual of the functor's projection of R X + t
// against (u_obs, v_obs), the depth z of the point in that camera, and with JAC jc = d r / d (camera tangent) and
// jp = d r / d X = (d r / d P_c) R.  z <= 0: the residual is not meaningful (it may be non-finite); the caller decides.
template <bool JAC>
__device__ __forceinline__ void project_world_point(const Intrinsics& K, const double* __restrict__ f, const double (&X)[3],
                                                    const double u_obs, const double v_obs, double& ru, double& rv, double& z,
                                                    double (&jc)[2][6], double (&jp)[2][3])
{
    const double b0 = f[0] * X[0] + f[1] * X[1] + f[2] * X[2];
    const double b1 = f[3] * X[0] + f[4] * X[1] + f[5] * X[2];
    const double b2 = f[6] * X[0] + f[7] * X[1] + f[8] * X[2];
    const double t[3] = { f[9], f[10], f[11] };
    z = b2 + t[2];
    project_camera_point<false, JAC>(K, b0, b1, b2, t, u_obs, v_obs, ru, rv, jc);
    if (!JAC)
        return;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            jp[r][c] = jc[r][0] * f[c] + jc[r][1] * f[3 + c] + jc[r][2] * f[6 + c];
}

__device__ __forceinline__ int wave_count(int n)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        n += __shfl_xor(n, s, 64);
    return n;
}

// A x = b for a packed lower symmetric 3 x 3 A.  false: A is not positive definite beyond rounding, or x is not finite.
// A sum of projectors I - d d^T has entries of order one, and two parallel rays leave a last pivot of rounding size that
// may come out positive: a pivot below kSpdFloor times the largest diagonal entry counts as zero.
constexpr double kSpdFloor = 1e-13;
__device__ __forceinline__ bool spd3_solve(const double (&A)[6], const double (&b)[3], double (&x)[3])
{
    double L[6], y[3];
    bool ok = cholesky<3>(A, L, Packed{}, PivotPositive<true>{});
    const double dmax = fmax(A[0], fmax(A[2], A[5]));
#pragma unroll
    for (int j = 0; j < 3; ++j)
        ok = ok && L[tri6(j, j)] * L[tri6(j, j)] > kSpdFloor * dmax;
    forward_substitute<3>(L, Packed{}, [&](const int i) { return b[i]; }, [&](const int i, const double v) { y[i] = v; });
    backward_substitute<3>(L, Packed{}, [&](const int i) { return y[i]; }, x);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        ok = ok && finite_bits(x[i]);
    return ok;
}

// Levenberg-Marquardt over the 3 coordinates of X (in place): lm_trials (small_solve.hpp) with addition as the update.
// cost receives the cost at the returned X.  The invariant holds here too: all lanes that run the driver together hold
// the same sums (every lane ends a wave_sum with the total), so they run the same 3 x 3 solve and every branch is
// wave-uniform.
template <typename Sums>
__device__ __forceinline__ int lm_refine3(double (&X)[3], const int max_trials, Sums&& sums, double& cost)
{
    return lm_trials<3, 3, true, false>(X, max_trials, sums,
                                        [](const double (&at)[3], const double (&step)[3], double (&cand)[3]) {
#pragma unroll
                                            for (int k = 0; k < 3; ++k)
                                                cand[k] = at[k] + step[k];
                                        },
                                        cost);
}

} // namespace vmm
