// One-pose Levenberg-Marquardt building blocks shared by kernels_init.hip (map initialisation) and
// kernels_localize.hip (localisation against a finished map): everything is __forceinline__ and lives in registers.
#pragma once
#include "geom.hpp"

namespace vmm {

constexpr double kInf = __builtin_huge_val();
constexpr double kLamInit = 1e-3, kLamMin = 1e-12, kLamMax = 1e12;

__device__ __forceinline__ int tri6(int a, int b) { return a * (a + 1) / 2 + b; }   // a >= b

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// The same question asked of the bits.  finite_d's subtraction may be contracted with the arithmetic that produced v
// (v = a * b + c: v - v becomes fma(a, b, c - v), the rounding error of v instead of zero), which reports a perfectly
// finite v as non-finite; where that would be wrong rather than merely slow, ask this one.
__device__ __forceinline__ bool finite_bits(double v) { return __builtin_isfinite(v); }

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
template <bool BITS = false>
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
        ok = ok && d > 0.0 && (BITS ? finite_bits(d) : finite_d(d));
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
        ok = ok && (BITS ? finite_bits(step[i]) : finite_d(step[i]));
    return ok;
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

__device__ __forceinline__ double corner_sx(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }   // LL, LR, UR, UL
__device__ __forceinline__ double corner_sy(int k) { return k >= 2 ? 1.0 : -1.0; }

} // namespace vmm
