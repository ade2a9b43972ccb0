// What k_predict (kernels_predict.hip) and k_predict_joint (kernels_predict_joint.hip) share: the visibility rules, the
// tag Jacobian of a corner, the fetch of wave_sum32's totals, and the tail from the wave's sums to the stored result.
// Everything is __forceinline__ and lives in registers; nothing here touches LDS.
#pragma once

#include "engine.hpp"
#include "image_sums.hpp"

namespace vmm {

// the value wave_sum32 left for index k (lanes 2 m and 2 m + 1 hold index bit-reverse(m)), in every lane
__device__ __forceinline__ double wave_sum32_fetch(const double tot, const int k)
{
    const int m = ((k & 1) << 4) | ((k & 2) << 2) | (k & 4) | ((k & 8) >> 2) | ((k & 16) >> 4);
    return __shfl(tot, 2 * m, 64);
}

// Whether the tag with world corners w (4 x 3) and face f is visible from the pose `cam` with centre C; the rules and
// their words are include/vmm_ba.h's.
__device__ __forceinline__ bool tag_visible(const PredictArgs& a, const Intrinsics& K, const Rigid& cam, const double (&C)[3],
                                            const double (&w)[12], const double (&f)[kTagFace])
{
    const double d0 = C[0] - f[3], d1 = C[1] - f[4], d2 = C[2] - f[5];
    if (!(f[0] * d0 + f[1] * d1 + f[2] * d2 >= a.cos_max_angle * sqrt(d0 * d0 + d1 * d1 + d2 * d2)))
        return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        ok = ok && (cam.R[6] * w[3 * k] + cam.R[7] * w[3 * k + 1] + cam.R[8] * w[3 * k + 2]) + cam.t[2] > a.min_depth;
    if (!ok)
        return false;
    double u[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double b0, b1, b2, j[2][6];
        rotate_world(cam, w[3 * k], w[3 * k + 1], w[3 * k + 2], b0, b1, b2);
        const double iz = 1.0 / (b2 + cam.t[2]);
        const double x = (b0 + cam.t[0]) * iz, y = (b1 + cam.t[1]) * iz;
        const double r2 = x * x + y * y;
        ok = ok && 1.0 + r2 * (3.0 * K.k1 + r2 * (5.0 * K.k2 + r2 * (7.0 * K.k3))) > 0.0;
        project_camera_point<false, false>(K, b0, b1, b2, cam.t, 0.0, 0.0, u[k], v[k], j);
        ok = ok && u[k] >= a.u_lo && u[k] <= a.u_hi && v[k] >= a.v_lo && v[k] <= a.v_hi;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double du = u[(k + 1) & 3] - u[k], dv = v[(k + 1) & 3] - v[k];
        ok = ok && du * du + dv * dv >= a.min_side2;
    }
    return ok;
}

// The 2 x 6 Jacobian jt of a corner's residual over its tag's tangent, from the camera Jacobian jc of the same corner:
// eval_corner<true, true>'s (geom.hpp).  The translation columns are g^T R_cam, the rotation columns 2 (a x h) with
// a = (a0, a1, a2) = world corner - tag centre.
__device__ __forceinline__ void corner_tag_jacobian(const Rigid& cam, const double (&jc)[2][6], const double a0, const double a1,
                                                    const double a2, double (&jt)[2][6])
{
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double h0 = jc[r][0] * cam.R[0] + jc[r][1] * cam.R[3] + jc[r][2] * cam.R[6];
        const double h1 = jc[r][0] * cam.R[1] + jc[r][1] * cam.R[4] + jc[r][2] * cam.R[7];
        const double h2 = jc[r][0] * cam.R[2] + jc[r][1] * cam.R[5] + jc[r][2] * cam.R[8];
        jt[r][0] = h0;
        jt[r][1] = h1;
        jt[r][2] = h2;
        jt[r][3] = 2.0 * (a1 * h2 - a2 * h1);
        jt[r][4] = 2.0 * (a2 * h0 - a0 * h2);
        jt[r][5] = 2.0 * (a0 * h1 - a1 * h0);
    }
}

// What lane 0 stores for pose p; have false: zero matrices and sigmas.
__device__ __forceinline__ void store_pose(const PredictArgs& a, const int p, const bool have, const double (&P)[21],
                                           const double (&Q)[21], const vmm_ba_predict_result& res)
{
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (a.cov_px)
                a.cov_px[36 * (int64_t)p + 6 * r + c] = have ? sym6(P, r, c) : 0.0;
            if (a.cov_map)
                a.cov_map[36 * (int64_t)p + 6 * r + c] = have ? sym6(Q, r, c) : 0.0;
        }
    if (a.res)
        a.res[p] = res;
}

// The result of pose p from the wave's totals H, M (with MAP) and n_visible, which every lane holds alike, so that every
// lane takes the same way: the statuses, spd_inverse<6>, the sandwich H^-1 M H^-1, the two sigmas; lane 0 stores.
// usable false: a pose with enough tags that is SINGULAR whatever its sums say.
template <bool MAP>
__device__ __forceinline__ void finish_pose(const PredictArgs& a, const int p, const int lane, const Rigid& cam,
                                            const double (&H)[21], const double (&M)[21], const int n_visible, const bool usable)
{
    vmm_ba_predict_result res;
    res.n_visible = n_visible;
    res.sigma_pos_m = 0.0;
    res.sigma_rot_rad = 0.0;
    double P[21], Q[21];
    bool have = false;
    if (res.n_visible == 0)
        res.status = VMM_BA_PRED_NO_VISIBLE_TAG;
    else if (res.n_visible < a.min_tags)
        res.status = VMM_BA_PRED_TOO_FEW_TAGS;
    else {
        res.status = VMM_BA_PRED_SINGULAR;
        double Cv[21];
        have = spd_inverse<6>(H, Cv) && usable;
        if (MAP)
            have = sandwich6(Cv, M, Q) && have;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            P[k] = a.sigma2 * Cv[k];
            if (!MAP)
                Q[k] = 0.0;
            sum += fabs(P[k]);
        }
        have = have && finite_bits(sum);
        // dC = -R^T (dt + 2 [t]x dr): R is orthogonal, so the trace of the centre's covariance is that of A V A^T with
        // A = [I | 2 [t]x] and V = cov_px + cov_map; radians are twice the tangent's rotation part
        const double tx = 2.0 * cam.t[0], ty = 2.0 * cam.t[1], tz = 2.0 * cam.t[2];
        const double A[3][6] = { { 1.0, 0.0, 0.0, 0.0, -tz, ty }, { 0.0, 1.0, 0.0, tz, 0.0, -tx }, { 0.0, 0.0, 1.0, -ty, tx, 0.0 } };
        double pos = 0.0, rot = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    if ((r == i || r >= 3) && (c == i || c >= 3))
                        pos += A[i][r] * (sym6(P, r, c) + sym6(Q, r, c)) * A[i][c];
            rot += sym6(P, 3 + i, 3 + i) + sym6(Q, 3 + i, 3 + i);
        }
        rot *= 4.0;
        have = have && finite_bits(pos) && finite_bits(rot) && pos >= 0.0 && rot >= 0.0;
        if (have) {
            res.status = VMM_BA_PRED_OK;
            res.sigma_pos_m = sqrt(pos);
            res.sigma_rot_rad = sqrt(rot);
        }
    }
    if (lane == 0)
        store_pose(a, p, have, P, Q, res);
}

} // namespace vmm
