// One-shot map initialisation from the tag detections (gfx950): vmm_ba_quad_poses / vmm_ba_initialize.
//
// Replaces the pose initialisations the reference's incremental driver does one item at a time on the host:
//   solvePnPEigen on a tag's own four corners      src/TagReconstructor.cpp:208, src/EigenCVConversions.cpp:38-63
//   solvePnPRansacEigen on a camera's corners      src/TagReconstructor.cpp:280-312, src/EigenCVConversions.cpp:65-106
// with three data-parallel steps:
//   k_quad_pose    lane = observation: both planar tag->camera poses from the observation's own four corners
//   k_init_score   workgroup = pose: every candidate (quad pose chained through a placed pose of the other family) is
//                  scored by the truncated squared reprojection error over ALL the pose's corners on placed
//                  counterparts; the lowest sum wins
//   k_init_refine  wave = pose: Levenberg-Marquardt on that pose alone against its fixed placed counterparts
// The single-pose solver all three are built from lives in pose_lm.hpp and is shared with kernels_localize.hip: the
// Levenberg-Marquardt trial loop (lm_refine: quad_refine and k_init_refine supply their sums as a lambda), the camera-side
// projection with its Jacobian (project_camera_point: quad_corner forms the rotated point and calls it), the candidate
// winner rule (better, wave_winner: k_init_score), the 21 + 6 sums (zero_normal, wave_sum_normal, accumulate_rows; small_solve.hpp solves them)
// and the chaining of candidates (chain_camera, chain_tag, quat_from_R).  What is here is what differs: how a quad's
// rotated point is formed (z = 0), which observations a pose sums over, and the bookkeeping of the growth rounds.
// All f64, the projections of geom.hpp: k_quad_pose fits CameraModel::projectPoint (what vmm_ba_project_points computes,
// aliased tangential term included), scoring and refinement use the functor the bundle adjustment minimises (the two
// differ by up to 0.02 px with the README distortion, geom.hpp: distort).  Every loop is bounded by a
// constant or by a list length, no workgroup waits on another, every sum has a fixed order (lane-private sums in
// list order, then wave_sum's butterfly): results are bit-identical from run to run.
#include <limits.h>

#include "engine.hpp"
#include "pose_lm.hpp"

namespace vmm {

namespace {

constexpr int kQuadTrials = 60;        // LM trials (accepted + rejected) of one planar solution
constexpr int kUndistortIters = 20;    // fixed-point iterations of the undistortion (as cv::undistortPoints)

// ---- k_quad_pose ---------------------------------------------------------------------------------------------------

// One corner (X0, X1, 0) of the quad under the tag->camera pose T, projected like CameraModel::projectPoint, with the
// 2 x 6 Jacobian over T's tangent (project_camera_point<true, .>, pose_lm.hpp).  z = 0: two columns of R form b.
template <bool JAC>
__device__ __forceinline__ void quad_corner(const Intrinsics& K, const Rigid& T, const double X0, const double X1,
                                            const double u_obs, const double v_obs, double& ru, double& rv, double (&j)[2][6])
{
    const double b0 = T.R[0] * X0 + T.R[1] * X1, b1 = T.R[3] * X0 + T.R[4] * X1, b2 = T.R[6] * X0 + T.R[7] * X1;
    project_camera_point<true, JAC>(K, b0, b1, b2, T.t, u_obs, v_obs, ru, rv, j);
}

// Sum of the 8 squared pixel residuals of the quad under the tag->camera pose q; with JAC also J^T J and J^T r.
template <bool JAC>
__device__ __forceinline__ double quad_cost(const Intrinsics& K, const double* q, const double hw, const double hh,
                                            const double (&px)[8], double (&A)[21], double (&g)[6])
{
    Rigid cam;
    load_rigid<true>(q, cam);
    if (JAC)
        zero_normal(A, g);
    double cost = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double ru, rv, j[2][6];
        quad_corner<JAC>(K, cam, corner_sx(k) * hw, corner_sy(k) * hh, px[2 * k], px[2 * k + 1], ru, rv, j);
        cost += ru * ru + rv * rv;
        if (JAC)
            accumulate_rows(j, ru, rv, A, g);
    }
    return cost;
}

// Levenberg-Marquardt on the tag->camera pose q (in place) of one quad; returns the final cost, trials: the trials spent.
// lm_trials returns its loop counter, not the counter + 1: a stopping rule that fires in the last trial gives
// kQuadTrials - 1, and kQuadTrials means that no rule ended the run.
__device__ __forceinline__ double quad_refine(const Intrinsics& K, double* q, const double hw, const double hh,
                                              const double (&px)[8], int& trials)
{
    double cost;
    trials = lm_refine<false, false>(q, kQuadTrials, [&](auto jac, const double* at, double (&A)[21], double (&g)[6]) {
        return quad_cost<decltype(jac)::value>(K, at, hw, hh, px, A, g);
    }, cost);
    return cost;
}

// The two planar poses that the homography's first order at the tag centre allows (h1, h2, h3: its columns in the tag's
// metric frame).  With the camera turned so that the line of sight to the centre is its axis (Q, the minimal rotation),
// the 2 x 2 Jacobian of the image point over the tag's coordinates is the upper left block of the rotation over the
// distance: its larger singular value gives the distance, the unit length of the two columns |r1z| and |r2z|, their
// orthogonality the sign of r1z r2z, and the sign of r1z is the planar ambiguity itself.  Unlike the decomposition in
// k_quad_pose, which averages the two solutions of a weak-perspective quad into the saddle between them, neither of
// these starts lies there.
__device__ __forceinline__ void quad_weak_starts(const double (&h1)[3], const double (&h2)[3], const double (&h3)[3],
                                                 double (&w)[2][7])
{
    const double p0x = h3[0] / h3[2], p0y = h3[1] / h3[2];
    const double j1x = (h1[0] - p0x * h1[2]) / h3[2], j1y = (h1[1] - p0y * h1[2]) / h3[2];
    const double j2x = (h2[0] - p0x * h2[2]) / h3[2], j2y = (h2[1] - p0y * h2[2]) / h3[2];
    const double m = sqrt(p0x * p0x + p0y * p0y + 1.0);
    const double v[3] = { p0x / m, p0y / m, 1.0 / m };
    const double kx = v[1], ky = -v[0], f = 1.0 / (1.0 + v[2]);   // Q = I + [k]x + [k]x^2 / (1 + v_z), k = v x e_z
    const double Q[9] = { 1.0 - f * ky * ky, f * kx * ky, ky, f * kx * ky, 1.0 - f * kx * kx, -kx,
                          -ky, kx, 1.0 - f * (kx * kx + ky * ky) };
    const double a1x = (Q[0] * j1x + Q[1] * j1y) / m, a1y = (Q[3] * j1x + Q[4] * j1y) / m;
    const double a2x = (Q[0] * j2x + Q[1] * j2y) / m, a2y = (Q[3] * j2x + Q[4] * j2y) / m;
    const double sxx = a1x * a1x + a2x * a2x, syy = a1y * a1y + a2y * a2y, sxy = a1x * a1y + a2x * a2y;
    const double lam = 0.5 * (sxx + syy) + sqrt(0.25 * (sxx - syy) * (sxx - syy) + sxy * sxy);
    const double dist = 1.0 / sqrt(lam);
    const double b1x = a1x * dist, b1y = a1y * dist, b2x = a2x * dist, b2y = a2y * dist;
    const double u1 = 1.0 - (b1x * b1x + b1y * b1y), u2 = 1.0 - (b2x * b2x + b2y * b2y);
    const double z1 = sqrt(u1 > 0.0 ? u1 : 0.0);
    const double z2 = sqrt(u2 > 0.0 ? u2 : 0.0) * (b1x * b2x + b1y * b2y > 0.0 ? -1.0 : 1.0);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double sg = k ? -1.0 : 1.0;
        const double r1[3] = { b1x, b1y, sg * z1 }, r2[3] = { b2x, b2y, sg * z2 };
        const double r3[3] = { r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0] };
        double R[9];   // Q^T [r1 r2 r3]
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            R[3 * i] = Q[i] * r1[0] + Q[3 + i] * r1[1] + Q[6 + i] * r1[2];
            R[3 * i + 1] = Q[i] * r2[0] + Q[3 + i] * r2[1] + Q[6 + i] * r2[2];
            R[3 * i + 2] = Q[i] * r3[0] + Q[3 + i] * r3[1] + Q[6 + i] * r3[2];
        }
        quat_from_R(R, w[k]);
        w[k][4] = v[0] * dist;
        w[k][5] = v[1] * dist;
        w[k][6] = v[2] * dist;
    }
}

struct QuadArgs {
    Intrinsics K;
    int64_t n;
    const double* px;          // element k of observation i at px[k * stride_k + i * stride_i]
    int64_t stride_k, stride_i;
    const double* tag_wh;      // [2 * .]: row wh_index[i], or i when wh_index is null
    const int32_t* wh_index;
    const int32_t* out_index;  // where observation i's results go (null: i)
    const uint8_t* mask;       // by out index; null: all on.  Switched-off observations get RMS = +inf
    double* qt2;               // [14 * n]
    double* rms2;              // [2 * n]
};

__global__ __launch_bounds__(64) void k_quad_pose(const QuadArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    const int64_t o = a.out_index ? a.out_index[i] : i;
    double q[2][7] = { { 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 }, { 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 } };
    double rms[2] = { kInf, kInf };
    if (!a.mask || a.mask[o]) {
        const Intrinsics K = a.K;
        const int64_t w = a.wh_index ? a.wh_index[i] : i;
        const double hw = 0.5 * a.tag_wh[2 * w], hh = 0.5 * a.tag_wh[2 * w + 1];
        double px[8], xn[4], yn[4];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            px[k] = a.px[k * a.stride_k + i * a.stride_i];
        // undistorted normalised image points (fixed-point iteration of the functor's distortion model)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x0 = (px[2 * k] - K.cx) / K.fx, y0 = (px[2 * k + 1] - K.cy) / K.fy;
            double x = x0, y = y0;
            for (int it = 0; it < kUndistortIters; ++it) {
                const double r2 = x * x + y * y;
                const double rad = 1.0 + r2 * (K.k1 + r2 * (K.k2 + r2 * K.k3));
                const double dx = 2.0 * K.p1 * x * y + K.p2 * (r2 + 2.0 * x * x);
                const double dy = K.p1 * (r2 + 2.0 * y * y) + 2.0 * K.p2 * x * y;
                x = (x0 - dx) / rad;
                y = (y0 - dy) / rad;
            }
            xn[k] = x;
            yn[k] = y;
        }
        // homography unit square -> image quad in closed form, then the change of variables u = X / w + 1/2, v = Y / h + 1/2
        const double dx1 = xn[1] - xn[2], dx2 = xn[3] - xn[2], sx = xn[0] - xn[1] + xn[2] - xn[3];
        const double dy1 = yn[1] - yn[2], dy2 = yn[3] - yn[2], sy = yn[0] - yn[1] + yn[2] - yn[3];
        const double den = dx1 * dy2 - dx2 * dy1;
        const double hg = (sx * dy2 - dx2 * sy) / den, hh2 = (dx1 * sy - sx * dy1) / den;
        const double c0[3] = { xn[1] - xn[0] + hg * xn[1], yn[1] - yn[0] + hg * yn[1], hg };
        const double c1[3] = { xn[3] - xn[0] + hh2 * xn[3], yn[3] - yn[0] + hh2 * yn[3], hh2 };
        const double c2[3] = { xn[0], yn[0], 1.0 };
        double h1[3], h2[3], h3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h1[k] = c0[k] / (2.0 * hw);
            h2[k] = c1[k] / (2.0 * hh);
            h3[k] = 0.5 * c0[k] + 0.5 * c1[k] + c2[k];
        }
        // decomposition (the planar branch of OpenCV's iterative PnP): scale from the two column norms, the plane in
        // front of the camera, the two unit columns made orthogonal symmetrically (the polar factor of [r1 r2])
        const double n1 = sqrt(h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2]);
        const double n2 = sqrt(h2[0] * h2[0] + h2[1] * h2[1] + h2[2] * h2[2]);
        double s = 2.0 / (n1 + n2);
        if (h3[2] * s < 0.0)
            s = -s;
        const double sg = s < 0.0 ? -1.0 : 1.0;
        double r1[3], r2[3], cs[3], df[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r1[k] = h1[k] / n1 * sg;
            r2[k] = h2[k] / n2 * sg;
            cs[k] = r1[k] + r2[k];
            df[k] = r1[k] - r2[k];
        }
        const double nc = 1.0 / sqrt(2.0 * (cs[0] * cs[0] + cs[1] * cs[1] + cs[2] * cs[2]));
        const double nd = 1.0 / sqrt(2.0 * (df[0] * df[0] + df[1] * df[1] + df[2] * df[2]));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r1[k] = cs[k] * nc + df[k] * nd;
            r2[k] = cs[k] * nc - df[k] * nd;
        }
        const double r3[3] = { r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0] };
        const double R[9] = { r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2] };
        quat_from_R(R, q[0]);
        q[0][4] = h3[0] * s;
        q[0][5] = h3[1] * s;
        q[0][6] = h3[2] * s;
        double cost[2];
        int trials[2];
        cost[0] = quad_refine(K, q[0], hw, hh, px, trials[0]);
        // the second planar solution: the tag normal mirrored about the line of sight to the tag centre
        {
            Rigid T;
            load_rigid<true>(q[0], T);
            const double tn = 1.0 / sqrt(T.t[0] * T.t[0] + T.t[1] * T.t[1] + T.t[2] * T.t[2]);
            const double v[3] = { T.t[0] * tn, T.t[1] * tn, T.t[2] * tn };
            const double nrm[3] = { T.R[2], T.R[5], T.R[8] };
            const double nv = nrm[0] * v[0] + nrm[1] * v[1] + nrm[2] * v[2];
            const double m[3] = { 2.0 * nv * v[0] - nrm[0], 2.0 * nv * v[1] - nrm[1], 2.0 * nv * v[2] - nrm[2] };
            const double ax[3] = { nrm[1] * m[2] - nrm[2] * m[1], nrm[2] * m[0] - nrm[0] * m[2], nrm[0] * m[1] - nrm[1] * m[0] };
            const double sn = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
            const double c = nrm[0] * m[0] + nrm[1] * m[1] + nrm[2] * m[2];
            // minimal rotation taking the normal to its mirror image, as a quaternion (half angle from cos)
            double z0 = 1.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
            if (sn > 1e-12) {
                const double ch = sqrt(0.5 * (1.0 + c) > 0.0 ? 0.5 * (1.0 + c) : 0.0);
                const double sh = sqrt(0.5 * (1.0 - c) > 0.0 ? 0.5 * (1.0 - c) : 0.0) / sn;
                z0 = ch;
                z1 = sh * ax[0];
                z2 = sh * ax[1];
                z3 = sh * ax[2];
            }
            const double w0 = q[0][0], w1 = q[0][1], w2 = q[0][2], w3 = q[0][3];
            q[1][0] = z0 * w0 - z1 * w1 - z2 * w2 - z3 * w3;
            q[1][1] = z0 * w1 + z1 * w0 + z2 * w3 - z3 * w2;
            q[1][2] = z0 * w2 - z1 * w3 + z2 * w0 + z3 * w1;
            q[1][3] = z0 * w3 + z1 * w2 - z2 * w1 + z3 * w0;
            q[1][4] = q[0][4];
            q[1][5] = q[0][5];
            q[1][6] = q[0][6];
        }
        cost[1] = quad_refine(K, q[1], hw, hh, px, trials[1]);
        // The fallback.  The start above lies at the saddle between the two planar minima when the perspective is weak;
        // the gradient along the tilt is nearly zero there and the loop crawls.  A solution that spent all its trials is
        // replaced by a weak-perspective start refined the same way, where that ends lower: both starts when both
        // stalled, otherwise the one whose normal lies further from the solution that is kept.
        const bool stall0 = trials[0] == kQuadTrials, stall1 = trials[1] == kQuadTrials;
        if (stall0 || stall1) {
            double w[2][7], wc[2];
            quad_weak_starts(h1, h2, h3, w);
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                int spent;
                wc[k] = quad_refine(K, w[k], hw, hh, px, spent);
            }
            int pick0 = 0, pick1 = 1;
            if (!(stall0 && stall1)) {
                Rigid keep, w0, w1;
                load_rigid<true>(stall0 ? q[1] : q[0], keep);
                load_rigid<true>(w[0], w0);
                load_rigid<true>(w[1], w1);
                const double d0 = w0.R[2] * keep.R[2] + w0.R[5] * keep.R[5] + w0.R[8] * keep.R[8];
                const double d1 = w1.R[2] * keep.R[2] + w1.R[5] * keep.R[5] + w1.R[8] * keep.R[8];
                pick0 = pick1 = d1 < d0 ? 1 : 0;
            }
            if (stall0 && finite_bits(wc[pick0]) && wc[pick0] < cost[0]) {
                cost[0] = wc[pick0];
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    q[0][k] = pick0 ? w[1][k] : w[0][k];
            }
            if (stall1 && finite_bits(wc[pick1]) && wc[pick1] < cost[1]) {
                cost[1] = wc[pick1];
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    q[1][k] = pick1 ? w[1][k] : w[0][k];
            }
        }
#pragma unroll
        for (int sidx = 0; sidx < 2; ++sidx) {
            const double qn = 1.0 / sqrt(q[sidx][0] * q[sidx][0] + q[sidx][1] * q[sidx][1] + q[sidx][2] * q[sidx][2]
                                         + q[sidx][3] * q[sidx][3]);
            // finite_bits, not finite_d: the compiler contracted finite_d's v - v with the product q * qn just above it
            // into fma(q, qn, -v), the product's rounding error, for two components of the second solution, which then
            // came back as +inf unless both products happened to be exact
            bool ok = finite_bits(cost[sidx]) && finite_bits(qn);
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                if (k < 4)
                    q[sidx][k] *= qn;
                ok = ok && finite_bits(q[sidx][k]);
            }
            if (ok) {
                rms[sidx] = sqrt(0.25 * cost[sidx]);   // RMS corner distance in pixels
            } else {
                q[sidx][0] = 1.0;
                q[sidx][1] = q[sidx][2] = q[sidx][3] = q[sidx][4] = q[sidx][5] = 0.0;
                q[sidx][6] = 1.0;
            }
        }
    }
    const int first = rms[1] < rms[0] ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        a.qt2[14 * o + k] = first ? q[1][k] : q[0][k];
        a.qt2[14 * o + 7 + k] = first ? q[0][k] : q[1][k];
    }
    a.rms2[2 * o] = first ? rms[1] : rms[0];
    a.rms2[2 * o + 1] = first ? rms[0] : rms[1];
}

// ---- k_init_score / k_init_refine ----------------------------------------------------------------------------------

struct InitArgs {
    Intrinsics K;
    int n_own;
    const int32_t* start;      // [n_own + 1] observation range of every pose of this family
    const int32_t* other;      // [n_obs] pose of the other family
    const int32_t* caller;     // [n_obs] caller's observation index
    const double* px;          // [8][n_pad]
    int64_t n_pad;
    const uint8_t* mask;       // [n_obs] caller order
    double* own_qt;            // this family's poses (written for the poses that are placed)
    const double* other_qt;
    const double* tag_wh;
    int32_t* own_placed;
    const int32_t* other_placed;
    int32_t* todo;             // [n_own] k_init_score -> k_init_refine: a candidate was selected for this pose
    const double* quad_qt;     // [14 * n_obs] caller order
    const double* quad_rms;    // [2 * n_obs]
    int sweep;                 // 0: place poses that are not placed yet; 1: redo every placed pose
    const uint8_t* own_const;  // [n_own] non-zero: the pose is constant -- placed from the start, never touched
    int min_obs;               // active observations a pose needs to be placed
    double cap2;               // score_cap_px^2
    int max_trials;            // LM trials of the refinement
    int32_t* counter;          // poses newly placed (growth rounds)
};

__device__ __forceinline__ bool obs_usable(const InitArgs& a, const int d)
{
    return a.mask[a.caller[d]] != 0 && a.other_placed[a.other[d]] != 0;
}

// Truncated score of pose `own` over the usable observations [b, e) of pose p.
template <bool CAM>
__device__ __forceinline__ double score_pose(const InitArgs& a, const Rigid& own, const int p, const int b, const int e)
{
    double sum = 0.0;
    for (int d = b; d < e; ++d) {
        if (!obs_usable(a, d))
            continue;
        const int o = a.other[d];
        Rigid oth;
        load_rigid<true>(a.other_qt + 7 * (int64_t)o, oth);
        const int t = CAM ? o : p;
        const double hw = 0.5 * a.tag_wh[2 * t], hh = 0.5 * a.tag_wh[2 * t + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<false, false>(a.K, CAM ? own : oth, CAM ? oth : own, corner_sx(k) * hw, corner_sy(k) * hh,
                                      a.px[(2 * k) * a.n_pad + d], a.px[(2 * k + 1) * a.n_pad + d], ev);
            const double e2 = ev.ru * ev.ru + ev.rv * ev.rv;
            sum += e2 < a.cap2 ? e2 : (finite_bits(e2) ? a.cap2 : kInf);   // not finite_d: e2 is a sum of two products (k_quad_pose's final tests)
        }
    }
    return sum;
}

// Candidate c of pose p: solution c & 1 of observation b + (c >> 1), chained through that observation's counterpart.
template <bool CAM>
__device__ __forceinline__ bool candidate_pose(const InitArgs& a, const int b, const int c, Rigid& out)
{
    const int d = b + (c >> 1), s = c & 1;
    if (!obs_usable(a, d))
        return false;
    const int64_t i = a.caller[d];
    if (!(a.quad_rms[2 * i + s] < kInf))
        return false;
    Rigid rel, oth;
    load_rigid<true>(a.quad_qt + 14 * i + 7 * s, rel);
    load_rigid<true>(a.other_qt + 7 * (int64_t)a.other[d], oth);
    if (CAM)
        chain_camera(rel, oth, out);
    else
        chain_tag(rel, oth, out);
    return true;
}

// One workgroup of kScoreThreads per pose: thread = candidate (strided), so that the 2 m candidates of a pose with m
// observations (each of them m x 4 reprojections) spread over 16 waves; the waves' winners meet in LDS and thread 0 takes
// them in wave order.
constexpr int kScoreThreads = 1024;

template <bool CAM>
__global__ __launch_bounds__(kScoreThreads) void k_init_score(const InitArgs a)
{
    __shared__ double s_best[kScoreThreads / 64];
    __shared__ int s_c[kScoreThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x;
    if (threadIdx.x == 0)
        a.todo[p] = 0;
    // everything up to the barrier depends on the pose alone: the whole workgroup leaves together or not at all
    const bool placed = a.own_placed[p] != 0;
    if (a.own_const[p] != 0 || (a.sweep ? !placed : placed))
        return;
    const int b = a.start[p], e = a.start[p + 1];
    int n_act = 0, n_use = 0;
    for (int d = b + lane; d < e; d += 64) {
        n_act += a.mask[a.caller[d]] != 0;
        n_use += obs_usable(a, d);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        n_act += __shfl_xor(n_act, m, 64);
        n_use += __shfl_xor(n_use, m, 64);
    }
    if (n_use == 0 || n_act < a.min_obs)
        return;
    double best = kInf;
    int best_c = INT_MAX;
    for (int c = threadIdx.x; c < 2 * (e - b); c += kScoreThreads) {
        Rigid cand;
        if (!candidate_pose<CAM>(a, b, c, cand))
            continue;
        const double sc = score_pose<CAM>(a, cand, p, b, e);
        if (sc < best) {   // NaN and +inf lose
            best = sc;
            best_c = c;
        }
    }
    if (a.sweep && threadIdx.x == kScoreThreads - 1) {   // the pose as it stands competes too and wins ties
        Rigid cur;
        load_rigid<true>(a.own_qt + 7 * (int64_t)p, cur);
        const double sc = score_pose<CAM>(a, cur, p, b, e);
        if (sc <= best) {
            best = sc;
            best_c = -1;
        }
    }
    wave_winner(best, best_c);
    if (lane == 0) {
        s_best[wave] = best;
        s_c[wave] = best_c;
    }
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (int w = 1; w < kScoreThreads / 64; ++w)
        if (better(s_best[w], s_c[w], best, best_c)) {
            best = s_best[w];
            best_c = s_c[w];
        }
    if (!(best < kInf))
        return;
    if (best_c >= 0) {
        Rigid win;
        candidate_pose<CAM>(a, b, best_c, win);
        double* q = a.own_qt + 7 * (int64_t)p;
        quat_from_R(win.R, q);
        q[4] = win.t[0];
        q[5] = win.t[1];
        q[6] = win.t[2];
    }
    a.todo[p] = 1;
}

// Cost (and with JAC the normal equations) of pose q of family CAM over the usable observations of p, lanes striding
// over the list; every lane returns the wave's totals.
template <bool CAM, bool JAC>
__device__ __forceinline__ double refine_sums(const InitArgs& a, const double* q, const int p, const int b, const int e,
                                              const int lane, double (&A)[21], double (&g)[6])
{
    Rigid own;
    load_rigid<true>(q, own);
    double cost = 0.0;
    if (JAC)
        zero_normal(A, g);
    for (int d = b + lane; d < e; d += 64) {
        if (!obs_usable(a, d))
            continue;
        const int o = a.other[d];
        Rigid oth;
        load_rigid<true>(a.other_qt + 7 * (int64_t)o, oth);
        const int t = CAM ? o : p;
        const double hw = 0.5 * a.tag_wh[2 * t], hh = 0.5 * a.tag_wh[2 * t + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<JAC && CAM, JAC && !CAM>(a.K, CAM ? own : oth, CAM ? oth : own, corner_sx(k) * hw, corner_sy(k) * hh,
                                                 a.px[(2 * k) * a.n_pad + d], a.px[(2 * k + 1) * a.n_pad + d], ev);
            cost += ev.ru * ev.ru + ev.rv * ev.rv;
            if (JAC)
                accumulate_rows(CAM ? ev.jc : ev.jt, ev.ru, ev.rv, A, g);
        }
    }
    cost = wave_sum(cost);
    if (JAC)
        wave_sum_normal(A, g);
    return cost;
}

template <bool CAM>
__global__ __launch_bounds__(256) void k_init_refine(const InitArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.n_own || a.todo[p] == 0)
        return;
    const int b = a.start[p], e = a.start[p + 1];
    double q[7], cost;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        q[k] = a.own_qt[7 * (int64_t)p + k];
    // refine_sums gives every lane the wave's totals: the wave runs lm_refine as one
    lm_refine<false, true>(q, a.max_trials, [&](auto jac, const double* at, double (&A)[21], double (&g)[6]) {
        return refine_sums<CAM, decltype(jac)::value>(a, at, p, b, e, lane, A, g);
    }, cost);
    if (lane == 0) {
        const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        double* out = a.own_qt + 7 * (int64_t)p;
#pragma unroll
        for (int k = 0; k < 7; ++k)
            out[k] = k < 4 ? q[k] * qn : q[k];
        a.todo[p] = 0;
        if (a.own_placed[p] == 0) {
            a.own_placed[p] = 1;
            atomicAdd(a.counter, 1);   // an integer count: the order of the additions does not matter
        }
    }
}

// placed flags: cameras [0, n_cams), tags behind them; the constant poses (the origin tag among them) start placed
__global__ void k_init_begin(int32_t* placed, int n_pose, const uint8_t* __restrict__ pose_const)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pose)
        placed[i] = pose_const[i] != 0 ? 1 : 0;
}

// Mean corner reprojection distance (pixels) over the active observations whose camera and tag are both placed, and
// their number.  k_init_stats: one workgroup per camera, thread-private sums in list order, then a fixed tree in LDS,
// part[2 p] = sum, part[2 p + 1] = corners; k_init_stats_sum adds the cameras' partials the same way into out[0..1].
__device__ __forceinline__ void block_sum2(double sum, double cnt, double* out)
{
    __shared__ double s_sum[256], s_cnt[256];
    s_sum[threadIdx.x] = sum;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + m];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = s_sum[0];
        out[1] = s_cnt[0];
    }
}

__global__ __launch_bounds__(256) void k_init_stats(const InitArgs a, double* part)
{
    const int p = blockIdx.x;
    double sum = 0.0, cnt = 0.0;
    if (a.own_placed[p] != 0) {
        Rigid own;
        load_rigid<true>(a.own_qt + 7 * (int64_t)p, own);
        for (int d = a.start[p] + (int)threadIdx.x; d < a.start[p + 1]; d += 256) {
            if (!obs_usable(a, d))
                continue;
            const int o = a.other[d];
            Rigid oth;
            load_rigid<true>(a.other_qt + 7 * (int64_t)o, oth);
            const double hw = 0.5 * a.tag_wh[2 * o], hh = 0.5 * a.tag_wh[2 * o + 1];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                CornerEval ev;
                eval_corner<false, false>(a.K, own, oth, corner_sx(k) * hw, corner_sy(k) * hh, a.px[(2 * k) * a.n_pad + d],
                                          a.px[(2 * k + 1) * a.n_pad + d], ev);
                sum += sqrt(ev.ru * ev.ru + ev.rv * ev.rv);
                cnt += 1.0;
            }
        }
    }
    block_sum2(sum, cnt, part + 2 * (int64_t)p);
}

__global__ __launch_bounds__(256) void k_init_stats_sum(const double* part, int n, double* out)
{
    double sum = 0.0, cnt = 0.0;
    for (int p = (int)threadIdx.x; p < n; p += 256) {
        sum += part[2 * p];
        cnt += part[2 * p + 1];
    }
    block_sum2(sum, cnt, out);
}

InitArgs make_init_args(Engine& e, bool cam, const InitPass& s)
{
    const ObsOrder& ord = (cam == e.elim_cams) ? e.ordE : e.ordF;
    InitArgs a;
    a.K = e.K;
    a.n_own = cam ? e.n_cams : e.n_tags;
    a.start = ord.start;
    a.other = ord.other;
    a.caller = ord.caller;
    a.px = ord.px;
    a.n_pad = ord.n_pad;
    a.mask = e.obs_mask;
    a.own_qt = cam ? e.cam_qt : e.tag_qt;
    a.other_qt = cam ? e.tag_qt : e.cam_qt;
    a.tag_wh = e.tag_wh;
    a.own_placed = cam ? e.init_placed : e.init_placed + e.n_cams;
    a.other_placed = cam ? e.init_placed + e.n_cams : e.init_placed;
    a.todo = cam ? e.init_todo : e.init_todo + e.n_cams;
    a.quad_qt = e.init_quad_qt;
    a.quad_rms = e.init_quad_rms;
    a.sweep = s.sweep ? 1 : 0;
    a.own_const = cam ? e.pose_const : e.pose_const + e.n_cams;
    a.min_obs = cam ? 1 : s.min_tag_observations;
    a.cap2 = s.score_cap_px * s.score_cap_px;
    a.max_trials = s.refine_iterations;
    a.counter = e.init_counter;
    return a;
}

} // namespace

void launch_quad_poses(hipStream_t st, const Intrinsics& K, int64_t n, const double* tag_wh, const double* obs_px, double* qt2,
                       double* rms2, const int32_t* wh_index, const int32_t* out_index)
{
    if (n <= 0)
        return;
    QuadArgs a;
    a.K = K;
    a.n = n;
    a.px = obs_px;
    a.stride_k = 1;
    a.stride_i = 8;
    a.tag_wh = tag_wh;
    a.wh_index = wh_index;
    a.out_index = out_index;
    a.mask = nullptr;
    a.qt2 = qt2;
    a.rms2 = rms2;
    hipLaunchKernelGGL(k_quad_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
}

// quad poses of the handle's observations, results in the caller's observation order
void launch_init_quad(Engine& e)
{
    if (e.n_obs <= 0)
        return;
    const ObsOrder& ord = e.elim_cams ? e.ordF : e.ordE;   // sorted by tag: own = the tag whose size is needed
    QuadArgs a;
    a.K = e.K;
    a.n = e.n_obs;
    a.px = ord.px;
    a.stride_k = ord.n_pad;
    a.stride_i = 1;
    a.tag_wh = e.tag_wh;
    a.wh_index = ord.own;
    a.out_index = ord.caller;
    a.mask = e.obs_mask;
    a.qt2 = e.init_quad_qt;
    a.rms2 = e.init_quad_rms;
    hipLaunchKernelGGL(k_quad_pose, dim3((unsigned)((e.n_obs + 63) / 64)), dim3(64), 0, e.stream, a);
}

void launch_init_begin(Engine& e)
{
    const int n_pose = e.n_cams + e.n_tags;
    hipLaunchKernelGGL(k_init_begin, dim3((unsigned)((n_pose + 255) / 256)), dim3(256), 0, e.stream, e.init_placed, n_pose,
                       (const uint8_t*)e.pose_const);
}

// score + select + refine for one family
void launch_init_pass(Engine& e, bool cam, const InitPass& s)
{
    const InitArgs a = make_init_args(e, cam, s);
    const dim3 grid((unsigned)((a.n_own + 3) / 4)), block(256);
    const dim3 sgrid((unsigned)a.n_own), sblock(kScoreThreads);
    if (cam) {
        hipLaunchKernelGGL(k_init_score<true>, sgrid, sblock, 0, e.stream, a);
        hipLaunchKernelGGL(k_init_refine<true>, grid, block, 0, e.stream, a);
    } else {
        hipLaunchKernelGGL(k_init_score<false>, sgrid, sblock, 0, e.stream, a);
        hipLaunchKernelGGL(k_init_refine<false>, grid, block, 0, e.stream, a);
    }
}

// out[0] = sum of the corner errors, out[1] = corners; out[2 ..] holds the cameras' partials (2 each)
void launch_init_stats(Engine& e, double* out)
{
    InitPass s;
    const InitArgs a = make_init_args(e, true, s);
    hipLaunchKernelGGL(k_init_stats, dim3((unsigned)e.n_cams), dim3(256), 0, e.stream, a, out + 2);
    hipLaunchKernelGGL(k_init_stats_sum, dim3(1), dim3(256), 0, e.stream, out + 2, e.n_cams, out);
}

int preload_init_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_quad_pose)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_score<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_score<false>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_refine<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_refine<false>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_begin)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_stats)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_init_stats_sum)) != hipSuccess;
    return bad;
}

} // namespace vmm
