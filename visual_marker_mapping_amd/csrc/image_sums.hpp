// One image of a batch against a fixed map, as a 256-thread workgroup sees it: shared by kernels_localize.hip
// (k_localize), kernels_calibrate.hip (k_calib_classify, k_calib_image, k_calib_try) and kernels_rig.hip (k_rig_localize,
// whose frame is the images of all the rig's cameras).
//   ImageView        element k of local observation d: pixels and world corners, from LDS or from global memory
//   rotate_world / world_corner   a world corner under a world->camera pose, projected by project_camera_point (pose_lm.hpp)
//   classify_image   the inlier flags of the image's observations at a pose, and their number
//   image_sums       the cost over the active observations and, with JAC, J^T J, J^T r and sum |r|^2 over the pose
//   workgroup_count / workgroup_normal / workgroup_cost   the reductions behind them
//   store_result / store_failure   what a localisation writes for one image
// The two sums are workgroup functions: threads stride the observation list, one butterfly per wave, the waves combined
// in order through LDS (s_cnt: kImageWaves ints; s_red: 32 kImageWaves doubles with JAC, kImageWaves without); they
// hold barriers, so all kImageThreads threads call them together.
// kernels_locate.hip (k_locate_tags: a tag against fixed cameras) takes the three reductions as they are for its own sums.
#pragma once
#include "engine.hpp"
#include "pose_lm.hpp"

namespace vmm {

constexpr int kImageThreads = 256;   // the workgroup size of every kernel that calls classify_image or image_sums
constexpr int kImageWaves = kImageThreads / 64;

// A world point rotated into the camera frame, b = R w.
__device__ __forceinline__ void rotate_world(const Rigid& cam, const double w0, const double w1, const double w2, double& b0,
                                             double& b1, double& b2)
{
    b0 = cam.R[0] * w0 + cam.R[1] * w1 + cam.R[2] * w2;
    b1 = cam.R[3] * w0 + cam.R[4] * w1 + cam.R[5] * w2;
    b2 = cam.R[6] * w0 + cam.R[7] * w1 + cam.R[8] * w2;
}

// A world corner under the world->camera pose `cam`, projected like the functor the bundle adjustment minimises
// (project_camera_point<false, .>, pose_lm.hpp): residual and, with JAC, the 2 x 6 camera Jacobian.
template <bool JAC>
__device__ __forceinline__ void world_corner(const Intrinsics& K, const Rigid& cam, const double w0, const double w1,
                                             const double w2, const double u_obs, const double v_obs, double& ru, double& rv,
                                             double (&j)[2][6])
{
    double b0, b1, b2;
    rotate_world(cam, w0, w1, w2, b0, b1, b2);
    project_camera_point<false, JAC>(K, b0, b1, b2, cam.t, u_obs, v_obs, ru, rv, j);
}

// One image's observations: element k (0..7 pixels, 8..19 world corners) of local observation d.
template <bool STAGED>
struct ImageView {
    const double* lds;        // STAGED: [20][m]
    int m;
    const double* px;         // obs_px + 8 * first observation
    const int32_t* tag;       // obs_tag + first observation
    const double* corners;
    __device__ __forceinline__ double pixel(const int d, const int k) const
    {
        return STAGED ? lds[k * m + d] : px[8 * (int64_t)d + k];
    }
    __device__ __forceinline__ double world(const int d, const int k) const
    {
        return STAGED ? lds[(8 + k) * m + d] : corners[12 * (int64_t)tag[d] + k];
    }
};

// The workgroup's total of a per-thread count, in every thread: one butterfly per wave, the waves in order.
__device__ __forceinline__ int workgroup_count(int n, int* s_cnt)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        n += __shfl_xor(n, s, 64);
    if ((threadIdx.x & 63) == 0)
        s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();   // also orders the flags (global memory, this workgroup only) before their readers
    n = 0;
#pragma unroll
    for (int w = 0; w < kImageWaves; ++w)
        n += s_cnt[w];
    __syncthreads();
    return n;
}

// The workgroup's totals of the thread-private normal equations, cost and sum |r|^2, in every thread: A, g and raw2
// receive them, the cost is returned.
__device__ __forceinline__ double workgroup_normal(double (&A)[21], double (&g)[6], const double cost, const double raw,
                                                   double* s_red, double& raw2)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[32];   // 0..20 J^T J, 21..26 J^T r, 27 cost, 28 raw2
#pragma unroll
    for (int k = 0; k < 21; ++k)
        acc[k] = A[k];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        acc[21 + k] = g[k];
    acc[27] = cost;
    acc[28] = raw;
    acc[29] = acc[30] = acc[31] = 0.0;
    const double tot = wave_sum32(acc, lane);
    s_red[wave * 32 + wave_sum32_index(lane)] = tot;   // lanes 2 m and 2 m + 1 hold (and store) the same value
    __syncthreads();
    double r[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) {
        double t = s_red[k];
#pragma unroll
        for (int w = 1; w < kImageWaves; ++w)
            t += s_red[w * 32 + k];
        r[k] = t;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 21; ++k)
        A[k] = r[k];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        g[k] = r[21 + k];
    raw2 = r[28];
    return r[27];
}

// The workgroup's total of a thread-private cost, in every thread.
__device__ __forceinline__ double workgroup_cost(double cost, double* s_red)
{
    cost = wave_sum(cost);
    if ((threadIdx.x & 63) == 0)
        s_red[threadIdx.x >> 6] = cost;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < kImageWaves; ++w)
        t += s_red[w];
    __syncthreads();
    return t;
}

// Flags the observations whose largest corner distance under q is at most sqrt(inlier2); every thread returns their
// number.  A non-finite distance is an outlier.
template <bool STAGED>
__device__ __forceinline__ int classify_image(const Intrinsics& K, const ImageView<STAGED>& v, const double* q,
                                              const double inlier2, uint8_t* flags, int* s_cnt)
{
    Rigid cam;
    load_rigid<true>(q, cam);
    int n = 0;
    for (int d = threadIdx.x; d < v.m; d += kImageThreads) {
        bool in = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ru, rv, j[2][6];
            world_corner<false>(K, cam, v.world(d, 3 * k), v.world(d, 3 * k + 1), v.world(d, 3 * k + 2), v.pixel(d, 2 * k),
                                v.pixel(d, 2 * k + 1), ru, rv, j);
            in = in && (ru * ru + rv * rv <= inlier2);
        }
        flags[d] = in ? 1 : 0;
        n += in ? 1 : 0;
    }
    return workgroup_count(n, s_cnt);
}

// Sums over the active observations (flags null: all) at pose q: returns 1/2-free cost sum rho(|r_corner|^2); with JAC
// also J^T J (packed lower) and J^T r with the Huber corrector applied, and raw2 = sum |r|^2 without the loss.
// Every thread returns the same totals.
template <bool STAGED, bool JAC>
__device__ __forceinline__ double image_sums(const Intrinsics& K, const ImageView<STAGED>& v, const double* q,
                                             const uint8_t* flags, const bool robust, const double huber_a, double* s_red,
                                             double (&A)[21], double (&g)[6], double& raw2)
{
    Rigid cam;
    load_rigid<true>(q, cam);
    double cost = 0.0, raw = 0.0;
    if (JAC)
        zero_normal(A, g);
    for (int d = threadIdx.x; d < v.m; d += kImageThreads) {
        if (flags && flags[d] == 0)
            continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ru, rv, j[2][6];
            world_corner<JAC>(K, cam, v.world(d, 3 * k), v.world(d, 3 * k + 1), v.world(d, 3 * k + 2), v.pixel(d, 2 * k),
                              v.pixel(d, 2 * k + 1), ru, rv, j);
            const double s = ru * ru + rv * rv;
            double rho0, wgt;
            huber(robust, huber_a, s, rho0, wgt);
            cost += rho0;
            if (JAC) {
                raw += s;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    j[0][c] *= wgt;
                    j[1][c] *= wgt;
                }
                accumulate_rows(j, ru * wgt, rv * wgt, A, g);
            }
        }
    }
    if (JAC)
        return workgroup_normal(A, g, cost, raw, s_red, raw2);
    return workgroup_cost(cost, s_red);
}

// What thread 0 of k_localize / k_rig_localize stores for image (frame) p; have_cov false: a zero covariance.
__device__ __forceinline__ void store_result(const LocalizeArgs& a, const int p, const double (&q)[7], const double (&C)[21],
                                             const bool have_cov, const vmm_ba_localize_result& res)
{
    double* const out_q = a.cam_qt + 7 * (int64_t)p;
    double* const out_cov = a.cam_cov + 36 * (int64_t)p;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        out_q[k] = q[k];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c)
            out_cov[6 * r + c] = have_cov ? (r >= c ? C[tri6(r, c)] : C[tri6(c, r)]) : 0.0;
    a.res[p] = res;
}

// NO_OBSERVATIONS / NO_CANDIDATE: the identity pose, a zero covariance (the flags are zero already)
__device__ __forceinline__ void store_failure(const LocalizeArgs& a, const int p, const int m, const int status, const int trials)
{
    const double q[7] = { 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    vmm_ba_localize_result res;
    res.status = status;
    res.n_obs = m;
    res.n_inlier_obs = 0;
    res.trials = trials;
    res.rms_px = 0.0;
    res.cost = 0.0;
    const double C[21] = {};
    store_result(a, p, q, C, false, res);
}

} // namespace vmm
