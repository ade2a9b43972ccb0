// Free points from known cameras (gfx950): vmm_ba_triangulate, the dual of the localisation.
//   k_cam_frames    thread = camera: R, t and the centre c = -R^T t of q / |q| (load_rigid<true>), once per call
//   k_triangulate   wave = point, four points per 256-thread workgroup, one launch from rays to covariances:
//                   rays        lanes stride the point's observations: pixel -> undistorted world ray through c
//                   candidates  candidate 0: the least-squares point of all rays (6 + 3 wave sums, one 3 x 3 Cholesky);
//                               candidates 1..: lane = pair (a, b), a < b < min(m, max_pair), the same solve on two rays
//                               fetched from lanes a and b; every candidate scored over ALL the point's observations
//                   winner      most observations within inlier_px, then the lowest truncated sum, then the lowest index
//                   passes      classify, then Levenberg-Marquardt on the 3 coordinates over the inliers (lm_refine3,
//                               point_lm.hpp): lanes stride the observations, 6 + 3 + 2 wave sums per evaluation, every
//                               lane runs the same 3 x 3 solve
//                   result      flags at the returned point, H^-1 and H^-1 (sum G C G^T) H^-1 by a 3 x 3 Cholesky
// No LDS, no barrier, no atomic.  A wave never waits on another, nothing but the selection of the point depends on the
// wave's place in the grid, and every sum has a fixed order (a lane's own sum in list order, then wave_sum's butterfly):
// a point gives the same bits alone, anywhere in any batch and from run to run.  Every branch that holds a shuffle is
// wave-uniform: the loops over candidates and observations run whole strides of 64 with the spare lanes masked.
#include <limits.h>

#include "engine.hpp"
#include "point_lm.hpp"

namespace vmm {

namespace {

constexpr int kTriThreads = 256;
constexpr int kTriPoints = kTriThreads / 64;   // points (waves) per workgroup

__global__ __launch_bounds__(256) void k_cam_frames(int n_cams, const double* __restrict__ cam_qt, double* __restrict__ frames)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cams)
        return;
    Rigid cam;
    load_rigid<true>(cam_qt + 7 * (int64_t)i, cam);
    double* const f = frames + kCamFrame * (int64_t)i;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        f[k] = cam.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[9 + k] = cam.t[k];
        f[12 + k] = -(cam.R[k] * cam.t[0] + cam.R[3 + k] * cam.t[1] + cam.R[6 + k] * cam.t[2]);
    }
}

// One point's observations as its wave sees them.
struct Track {
    int m;
    const int32_t* cam;   // obs_cam + first observation
    const double* uv;     // obs_uv + 2 * first observation
    const double* frames;
    __device__ __forceinline__ const double* frame(const int d) const { return frames + kCamFrame * (int64_t)cam[d]; }
};

// The world ray of observation d: unit direction dir through the camera centre c.
__device__ __forceinline__ void world_ray(const Intrinsics& K, const Track& t, const int d, double (&dir)[3], double (&c)[3])
{
    const double* const f = t.frame(d);
    double x, y;
    undistort_pixel(K, t.uv[2 * (int64_t)d], t.uv[2 * (int64_t)d + 1], x, y);
    const double r0 = f[0] * x + f[3] * y + f[6], r1 = f[1] * x + f[4] * y + f[7], r2 = f[2] * x + f[5] * y + f[8];
    const double n = 1.0 / sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    dir[0] = r0 * n;
    dir[1] = r1 * n;
    dir[2] = r2 * n;
    c[0] = f[12];
    c[1] = f[13];
    c[2] = f[14];
}

// A += I - d d^T (packed lower), b += (I - d d^T) c
__device__ __forceinline__ void add_ray(const double (&dir)[3], const double (&c)[3], double (&A)[6], double (&b)[3])
{
    const double dc = dir[0] * c[0] + dir[1] * c[1] + dir[2] * c[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        b[i] += c[i] - dir[i] * dc;
#pragma unroll
        for (int j = 0; j <= i; ++j)
            A[tri6(i, j)] += (i == j ? 1.0 : 0.0) - dir[i] * dir[j];
    }
}

// What one lane knows of a candidate X: observations within inlier_px and in front of their camera, and
// sum min(e^2, cap^2) over all the point's observations (cap^2 for one behind its camera or with a non-finite distance).
__device__ __forceinline__ void score_point(const Intrinsics& K, const Track& t, const double (&X)[3], const double inlier2,
                                            const double cap2, int& count, double& score)
{
    count = 0;
    score = 0.0;
    for (int d = 0; d < t.m; ++d) {
        double ru, rv, z, jc[2][6], jp[2][3];
        project_world_point<false>(K, t.frame(d), X, t.uv[2 * (int64_t)d], t.uv[2 * (int64_t)d + 1], ru, rv, z, jc, jp);
        const double e2 = ru * ru + rv * rv;
        const bool front = z > 0.0;
        count += (front && e2 <= inlier2) ? 1 : 0;
        score += (front && e2 < cap2) ? e2 : cap2;
    }
}

// The winner rule: more inliers, then the lower truncated sum, then the lower index.  A lane without a finite candidate
// holds (-1, kInf, INT_MAX) and loses to every finite one.
__device__ __forceinline__ bool better_point(const int count, const double score, const int index, const int other_count,
                                             const double other_score, const int other_index)
{
    return count > other_count || (count == other_count && better(score, index, other_score, other_index));
}

// Flags the observations within sqrt(inlier2) of X and in front of their camera (a non-finite distance is an outlier);
// every lane returns their number.  The lane that writes flag d is the lane that reads it in point_sums.
__device__ __forceinline__ int classify_point(const Intrinsics& K, const Track& t, const double (&X)[3], const double inlier2,
                                              uint8_t* flags, const int lane)
{
    int n = 0;
    for (int d = lane; d < t.m; d += 64) {
        double ru, rv, z, jc[2][6], jp[2][3];
        project_world_point<false>(K, t.frame(d), X, t.uv[2 * (int64_t)d], t.uv[2 * (int64_t)d + 1], ru, rv, z, jc, jp);
        const bool in = z > 0.0 && ru * ru + rv * rv <= inlier2;
        flags[d] = in ? 1 : 0;
        n += in ? 1 : 0;
    }
    return wave_count(n);
}

// Sums over the flagged observations at X: returns the 1/2-free cost sum rho(|r|^2), +inf when a flagged observation is
// not in front of its camera; with JAC also J^T J (packed lower) and J^T r with the Huber corrector applied (rows and
// residuals scaled by sqrt(rho')) and raw2 = sum |r|^2 without the loss.  Every lane returns the same totals.
template <bool JAC>
__device__ __forceinline__ double point_sums(const Intrinsics& K, const Track& t, const double (&X)[3], const uint8_t* flags,
                                             const bool robust, const double huber_a, const int lane, double (&A)[6],
                                             double (&g)[3], double& raw2)
{
    double cost = 0.0, raw = 0.0;
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            A[k] = 0.0;
        g[0] = g[1] = g[2] = 0.0;
    }
    for (int d = lane; d < t.m; d += 64) {
        if (flags[d] == 0)
            continue;
        double ru, rv, z, jc[2][6], jp[2][3];
        project_world_point<JAC>(K, t.frame(d), X, t.uv[2 * (int64_t)d], t.uv[2 * (int64_t)d + 1], ru, rv, z, jc, jp);
        const double s = ru * ru + rv * rv;
        double rho0, wgt;
        huber(robust, huber_a, s, rho0, wgt);
        cost += z > 0.0 ? rho0 : kInf;
        if (JAC) {
            raw += s;
            ru *= wgt;
            rv *= wgt;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                jp[0][a] *= wgt;
                jp[1][a] *= wgt;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                g[a] += jp[0][a] * ru + jp[1][a] * rv;
#pragma unroll
                for (int b = 0; b <= a; ++b)
                    A[tri6(a, b)] += jp[0][a] * jp[0][b] + jp[1][a] * jp[1][b];
            }
        }
    }
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            A[k] = wave_sum(A[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            g[k] = wave_sum(g[k]);
        raw2 = wave_sum(raw);
    }
    return wave_sum(cost);
}

// sum_i G_i C_i G_i^T over the flagged observations (packed lower 3 x 3), G_i = rho'_i Jp_i^T Jc_i, C_i camera i's 6 x 6
// block of cam_cov.  Every lane returns the same totals.
__device__ __forceinline__ void camera_part(const Intrinsics& K, const Track& t, const double (&X)[3], const uint8_t* flags,
                                            const bool robust, const double huber_a, const double* __restrict__ cam_cov,
                                            const int lane, double (&S)[6])
{
#pragma unroll
    for (int k = 0; k < 6; ++k)
        S[k] = 0.0;
    for (int d = lane; d < t.m; d += 64) {
        if (flags[d] == 0)
            continue;
        double ru, rv, z, jc[2][6], jp[2][3];
        project_world_point<true>(K, t.frame(d), X, t.uv[2 * (int64_t)d], t.uv[2 * (int64_t)d + 1], ru, rv, z, jc, jp);
        double rho0, wgt;
        huber(robust, huber_a, ru * ru + rv * rv, rho0, wgt);
        const double w2 = wgt * wgt;
        const double* const C = cam_cov + 36 * (int64_t)t.cam[d];
        double G[3][6], T[3][6];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                G[a][c] = w2 * (jp[0][a] * jc[0][c] + jp[1][a] * jc[1][c]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    v += G[a][k] * C[6 * k + c];
                T[a][c] = v;
            }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    v += T[a][k] * G[b][k];
                S[tri6(a, b)] += v;
            }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        S[k] = wave_sum(S[k]);
}

__device__ __forceinline__ double sym3(const double (&P)[6], const int r, const int c) { return r >= c ? P[tri6(r, c)] : P[tri6(c, r)]; }

// What lane 0 stores for point p; have_cov / have_cams false: a zero matrix.
__device__ __forceinline__ void store_point(const TriangulateArgs& a, const int p, const double (&X)[3], const double (&C)[6],
                                            const bool have_cov, const double (&CC)[6], const bool have_cams,
                                            const vmm_ba_triangulate_result& res)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
        a.xyz[3 * (int64_t)p + k] = X[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = r >= c ? tri6(r, c) : tri6(c, r);
            a.cov[9 * (int64_t)p + 3 * r + c] = have_cov ? C[k] : 0.0;
            a.cov_cams[9 * (int64_t)p + 3 * r + c] = have_cams ? CC[k] : 0.0;
        }
    a.res[p] = res;
}

// TOO_FEW_VIEWS / NO_CANDIDATE: the origin, zero covariances, zero flags
__device__ __forceinline__ void store_no_point(const TriangulateArgs& a, const int p, const int m, uint8_t* flags, const int status,
                                               const int trials, const int lane)
{
    for (int d = lane; d < m; d += 64)
        flags[d] = 0;
    if (lane != 0)
        return;
    const double X[3] = { 0.0, 0.0, 0.0 };
    vmm_ba_triangulate_result res;
    res.status = status;
    res.n_obs = m;
    res.n_inlier_obs = 0;
    res.trials = trials;
    res.rms_px = 0.0;
    res.cost = 0.0;
    const double Z[6] = {};
    store_point(a, p, X, Z, false, Z, false, res);
}

__global__ __launch_bounds__(kTriThreads) void k_triangulate(const TriangulateArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kTriPoints + (threadIdx.x >> 6);
    // every decision to leave depends on the point alone or on values all lanes of its wave hold alike
    if (p >= a.n_pts)
        return;
    const int64_t first = a.pt_start[p];
    Track t;
    t.m = (int)(a.pt_start[p + 1] - first);
    t.cam = a.obs_cam + first;
    t.uv = a.obs_uv + 2 * first;
    t.frames = a.frames;
    uint8_t* const flags = a.obs_inlier + first;
    const int m = t.m;
    if (m < 2) {
        store_no_point(a, p, m, flags, VMM_BA_TRI_TOO_FEW_VIEWS, 0, lane);
        return;
    }
    const Intrinsics K = a.K;
    // ---- rays: lane l keeps the ray of observation l (the pairs are formed among the first views) ----
    double dir[3] = { 0.0, 0.0, 1.0 }, cen[3] = { 0.0, 0.0, 0.0 };
    double X0[3];
    {
        double A[6] = {}, b[3] = {};
        for (int d = lane; d < m; d += 64) {
            double dd[3], cc[3];
            world_ray(K, t, d, dd, cc);
            add_ray(dd, cc, A, b);
            if (d == lane) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    dir[k] = dd[k];
                    cen[k] = cc[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            A[k] = wave_sum(A[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            b[k] = wave_sum(b[k]);
        if (!spd3_solve(A, b, X0))
            X0[0] = X0[1] = X0[2] = kInf;
    }
    // ---- candidates: lane = candidate, whole strides of 64 ----
    const int mp = m < a.max_pair ? m : a.max_pair;
    const int n_cand = 1 + mp * (mp - 1) / 2;
    int best_n = -1, best_c = INT_MAX;
    double best = kInf;
    double X[3] = { 0.0, 0.0, 0.0 };
    for (int base = 0; base < n_cand; base += 64) {
        const int c = base + lane;
        const bool pair = c >= 1 && c < n_cand;
        int va = 0, vb = 1;
        if (pair) {   // pair c - 1 in lexicographic order
            int rem = c - 1;
            while (rem >= mp - 1 - va) {
                rem -= mp - 1 - va;
                ++va;
            }
            vb = va + 1 + rem;
        }
        double da[3], ca[3], db[3], cb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // all 64 lanes take part in the exchange
            da[k] = __shfl(dir[k], va, 64);
            ca[k] = __shfl(cen[k], va, 64);
            db[k] = __shfl(dir[k], vb, 64);
            cb[k] = __shfl(cen[k], vb, 64);
        }
        double Xc[3] = { X0[0], X0[1], X0[2] };
        if (pair) {
            double A[6] = {}, b[3] = {};
            add_ray(da, ca, A, b);
            add_ray(db, cb, A, b);
            if (!spd3_solve(A, b, Xc))
                Xc[0] = kInf;
        }
        if (c < n_cand && finite_bits(Xc[0]) && finite_bits(Xc[1]) && finite_bits(Xc[2])) {
            int n;
            double sc;
            score_point(K, t, Xc, a.inlier2, a.cap2, n, sc);
            if (finite_bits(sc) && better_point(n, sc, c, best_n, best, best_c)) {
                best_n = n;
                best = sc;
                best_c = c;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    X[k] = Xc[k];
            }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int on = __shfl_xor(best_n, s, 64), oc = __shfl_xor(best_c, s, 64);
        const double os = __shfl_xor(best, s, 64);
        if (better_point(on, os, oc, best_n, best, best_c)) {
            best_n = on;
            best = os;
            best_c = oc;
        }
    }
    if (best_n < 0) {
        store_no_point(a, p, m, flags, VMM_BA_TRI_NO_CANDIDATE, 0, lane);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)   // candidate c was lane c mod 64's, and that lane's own best is the wave's
        X[k] = __shfl(X[k], best_c & 63, 64);
    // ---- classify -> refine on the inliers ----
    const bool robust = a.robustify != 0;
    int trials = 0;
    double cost, raw2;
    auto sums = [&](auto jac, const double (&at)[3], double (&A)[6], double (&g)[3]) {
        return point_sums<decltype(jac)::value>(K, t, at, flags, robust, a.huber_a, lane, A, g, raw2);
    };
    if (a.passes == 0 && classify_point(K, t, X, kInf, flags, lane) > 0)   // everything in front of its camera
        trials += lm_refine3(X, a.max_trials, sums, cost);
    for (int pass = 0; pass < a.passes; ++pass) {
        if (classify_point(K, t, X, a.inlier2, flags, lane) < a.min_inliers)
            break;
        trials += lm_refine3(X, a.max_trials, sums, cost);
    }
    // ---- the result: flags, statistics and covariances at the returned point ----
    if (!(finite_bits(X[0]) && finite_bits(X[1]) && finite_bits(X[2]))) {   // cannot happen with finite inputs; keeps the no-NaN promise
        store_no_point(a, p, m, flags, VMM_BA_TRI_NO_CANDIDATE, trials, lane);
        return;
    }
    vmm_ba_triangulate_result res;
    res.status = VMM_BA_TRI_OK;
    res.n_obs = m;
    res.trials = trials;
    res.rms_px = 0.0;
    res.cost = 0.0;
    res.n_inlier_obs = classify_point(K, t, X, a.inlier2, flags, lane);
    double C[6], CC[6];
    bool have_cov = false, have_cams = false;
    if (res.n_inlier_obs > 0) {
        double H[6], g[3];
        cost = point_sums<true>(K, t, X, flags, robust, a.huber_a, lane, H, g, raw2);
        if (finite_bits(cost) && finite_bits(raw2)) {
            res.cost = 0.5 * cost;
            res.rms_px = sqrt(raw2 / res.n_inlier_obs);
        }
        if (res.n_inlier_obs >= a.min_inliers) {
            have_cov = spd_inverse<3, PivotPositive<true>>(H, C);
            if (!have_cov)
                res.status = VMM_BA_TRI_SINGULAR;
        }
        if (have_cov && a.cam_cov) {
            double S[6], T[3][3];
            camera_part(K, t, X, flags, robust, a.huber_a, a.cam_cov, lane, S);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    T[r][c] = sym3(C, r, 0) * sym3(S, 0, c) + sym3(C, r, 1) * sym3(S, 1, c) + sym3(C, r, 2) * sym3(S, 2, c);
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) {
                    // the symmetric part: row r of C S against column c of C, averaged with its mirror image
                    const double v = T[r][0] * sym3(C, 0, c) + T[r][1] * sym3(C, 1, c) + T[r][2] * sym3(C, 2, c);
                    const double w = T[c][0] * sym3(C, 0, r) + T[c][1] * sym3(C, 1, r) + T[c][2] * sym3(C, 2, r);
                    CC[tri6(r, c)] = 0.5 * (v + w);
                    sum += fabs(CC[tri6(r, c)]);
                }
            have_cams = finite_bits(sum);
        }
    }
    if (res.n_inlier_obs < a.min_inliers)
        res.status = VMM_BA_TRI_TOO_FEW_INLIERS;
    if (lane == 0)
        store_point(a, p, X, C, have_cov, CC, have_cams, res);
}

} // namespace

void launch_cam_frames(hipStream_t st, int n_cams, const double* cam_qt, double* frames)
{
    if (n_cams <= 0)
        return;
    hipLaunchKernelGGL(k_cam_frames, dim3((unsigned)((n_cams + 255) / 256)), dim3(256), 0, st, n_cams, cam_qt, frames);
}

void launch_triangulate(hipStream_t st, const TriangulateArgs& a)
{
    if (a.n_pts <= 0)
        return;
    hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((a.n_pts + kTriPoints - 1) / kTriPoints)), dim3(kTriThreads), 0, st, a);
}

int preload_triangulate_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_cam_frames)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_triangulate)) != hipSuccess;
    return bad;
}

} // namespace vmm
