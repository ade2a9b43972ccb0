// Localisation of images against a finished map (gfx950): vmm_ba_localize.
//
// Batch form of TagReconstructor::computeRelativeCameraPoseFromImg (src/TagReconstructor.cpp:280-312,
// solvePnPRansacEigen, src/EigenCVConversions.cpp:65-106), which the host mirror runs one image at a time:
//   k_quad_pose     (kernels_init.hip, as it is) both planar tag->camera poses of every observation
//   k_map_corners   thread = tag: the four world corners of every map tag, once per call -- eval_corner's tag half
//                   hoisted out of the per-observation, per-trial arithmetic
//   k_localize      workgroup = image, one launch from candidates to covariance:
//                   scoring   thread = candidate (two per observation, chained through the map tag), truncated squared
//                             reprojection error over all the image's corners; the waves' winners meet in LDS and are
//                             taken in wave order (better / wave_winner, pose_lm.hpp: the rule k_init_score uses)
//                   passes    classify the observations at the pose, Levenberg-Marquardt over the inliers: threads
//                             stride the observation list, 21 + 6 + 2 sums reduced by one butterfly per wave
//                             (wave_sum32) and combined in LDS in wave order; every thread runs the same 6 x 6 solve
//                   result    flags at the returned pose, (J^T J)^-1 by a 6 x 6 Cholesky in registers
// The single-pose solver is pose_lm.hpp's, shared with kernels_init.hip: lm_refine (refine_image supplies image_sums as a
// lambda; the sums hold barriers, so the workgroup runs the driver as one), better / wave_winner, chain_camera,
// quat_from_R, over small_solve.hpp's damped_solve<6> and spd_inverse<6>.  The image view (LDS or global), world_corner,
// classify_image and image_sums with their workgroup reductions and the stores of an image's result are image_sums.hpp's, shared with kernels_calibrate.hip and
// kernels_rig.hip.  Here: the staging, the candidate scoring and the passes.
// An image's pixels and world corners (20 doubles per observation) are staged in LDS when the image has at most
// kStage observations (k_localize<true>); larger images read them from global memory (k_localize<false>).  Both run the
// same arithmetic in the same order, and which one an image takes depends on its own length alone.
// Nothing but the selection of the image depends on blockIdx, no workgroup waits on another, there is no floating-point
// atomic and every sum has a fixed order (thread-private sums in list order, the wave butterfly, the waves in order):
// an image gives the same bits alone, in any batch and from run to run.
//
// Registers (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, the .s file's .vgpr_count / .vgpr_spill_count /
// .private_segment_fixed_size): k_localize<true> takes 350 and k_localize<false> 302 registers per lane with no spill and
// a zero private segment, like k_quad_pose (kernels_init.hip).  The compiler keeps a thread's own observation (20
// doubles and their LDS addresses) in registers across the passes, next to the 29 running sums, the pose and the 6 x 6
// system; asked for two waves per SIMD (__launch_bounds__(256, 2), 256 registers) it spills about 40 of them to scratch,
// so the kernel runs one wave per SIMD = one 256-thread workgroup per CU, and the 40 KiB of LDS never limit it.
#include <limits.h>

#include "engine.hpp"
#include "image_sums.hpp"

namespace vmm {

namespace {

constexpr int kLocThreads = kImageThreads;
constexpr int kLocWaves = kImageWaves;
constexpr int kStage = 256;   // observations staged in LDS: 20 x 8 B x 256 = 40 KiB per workgroup

__global__ __launch_bounds__(256) void k_map_corners(int n_tags, const double* __restrict__ tag_qt,
                                                     const double* __restrict__ tag_wh, double* __restrict__ corners)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tags)
        return;
    Rigid tag;
    load_rigid<true>(tag_qt + 7 * (int64_t)t, tag);
    const double hw = 0.5 * tag_wh[2 * t], hh = 0.5 * tag_wh[2 * t + 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // a = R_t p_l (p_l.z == 0), P_w = a + t_t, exactly as eval_corner (geom.hpp)
        const double sxhw = corner_sx(k) * hw, syhh = corner_sy(k) * hh;
        corners[12 * (int64_t)t + 3 * k] = (tag.R[0] * sxhw + tag.R[1] * syhh) + tag.t[0];
        corners[12 * (int64_t)t + 3 * k + 1] = (tag.R[3] * sxhw + tag.R[4] * syhh) + tag.t[1];
        corners[12 * (int64_t)t + 3 * k + 2] = (tag.R[6] * sxhw + tag.R[7] * syhh) + tag.t[2];
    }
}

// Truncated score of camera pose `cam` over all the image's corners.
template <bool STAGED>
__device__ __forceinline__ double score_image(const Intrinsics& K, const ImageView<STAGED>& v, const Rigid& cam,
                                              const double cap2)
{
    double sum = 0.0;
    for (int d = 0; d < v.m; ++d) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ru, rv, j[2][6];
            world_corner<false>(K, cam, v.world(d, 3 * k), v.world(d, 3 * k + 1), v.world(d, 3 * k + 2), v.pixel(d, 2 * k),
                                v.pixel(d, 2 * k + 1), ru, rv, j);
            const double e2 = ru * ru + rv * rv;
            sum += e2 < cap2 ? e2 : (finite_bits(e2) ? cap2 : kInf);
        }
    }
    return sum;
}

// Levenberg-Marquardt on q (in place) over the active observations; returns the trials spent.  image_sums gives every
// thread the workgroup's totals (and holds the barriers): the workgroup runs lm_refine as one.
template <bool STAGED>
__device__ __forceinline__ int refine_image(const Intrinsics& K, const ImageView<STAGED>& v, double (&q)[7],
                                            const uint8_t* flags, const bool robust, const double huber_a,
                                            const int max_trials, double* s_red)
{
    double cost, raw2;
    return lm_refine<true, false>(q, max_trials, [&](auto jac, const double* at, double (&A)[21], double (&g)[6]) {
        return image_sums<STAGED, decltype(jac)::value>(K, v, at, flags, robust, huber_a, s_red, A, g, raw2);
    }, cost);
}

template <bool STAGED>
__global__ __launch_bounds__(kLocThreads) void k_localize(const LocalizeArgs a)
{
    __shared__ double s_img[STAGED ? 20 * kStage : 1];
    __shared__ double s_red[kLocWaves * 32];
    __shared__ double s_best[kLocWaves];
    __shared__ int s_c[kLocWaves];
    __shared__ int s_cnt[kLocWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int64_t b = a.img_start[p];
    const int m = (int)(a.img_start[p + 1] - b);
    // every decision to leave depends on the image alone or on values all threads hold alike: the whole workgroup
    // reaches the same barriers and leaves together
    if ((m <= kStage) != STAGED)
        return;
    if (m == 0) {
        if (tid == 0)
            store_failure(a, p, m, VMM_BA_LOC_NO_OBSERVATIONS, 0);
        return;
    }
    uint8_t* const flags = a.obs_inlier + b;
    const Intrinsics K = a.K;
    ImageView<STAGED> v;
    v.lds = s_img;
    v.m = m;
    v.px = a.obs_px + 8 * b;
    v.tag = a.obs_tag + b;
    v.corners = a.corners;
    for (int d = tid; d < m; d += kLocThreads)
        flags[d] = 0;
    if (STAGED) {
        for (int i = tid; i < 8 * m; i += kLocThreads)   // coalesced read of the image's pixels, transposed store
            s_img[(i & 7) * m + (i >> 3)] = v.px[i];
        for (int i = tid; i < 12 * m; i += kLocThreads) {
            const int d = i / 12, k = i - 12 * d;
            s_img[(8 + k) * m + d] = a.corners[12 * (int64_t)v.tag[d] + k];
        }
        __syncthreads();
    }
    // ---- candidates ----
    double best = kInf;
    int best_c = INT_MAX;
    for (int c = tid; c < 2 * m; c += kLocThreads) {
        const int d = c >> 1, s = c & 1;
        if (!(a.quad_rms[2 * (b + d) + s] < kInf))
            continue;
        Rigid rel, tag, cand;
        load_rigid<true>(a.quad_qt + 14 * (b + d) + 7 * s, rel);
        load_rigid<true>(a.tag_qt + 7 * (int64_t)v.tag[d], tag);
        chain_camera(rel, tag, cand);
        const double sc = score_image<STAGED>(K, v, cand, a.cap2);
        if (sc < best) {   // NaN and +inf lose; within a thread c ascends, so ties keep the lowest
            best = sc;
            best_c = c;
        }
    }
    wave_winner(best, best_c);
    if (lane == 0) {
        s_best[wave] = best;
        s_c[wave] = best_c;
    }
    __syncthreads();
    best = s_best[0];
    best_c = s_c[0];
#pragma unroll
    for (int w = 1; w < kLocWaves; ++w)
        if (better(s_best[w], s_c[w], best, best_c)) {
            best = s_best[w];
            best_c = s_c[w];
        }
    if (!(best < kInf)) {
        if (tid == 0)
            store_failure(a, p, m, VMM_BA_LOC_NO_CANDIDATE, 0);
        return;
    }
    double q[7];
    {
        const int d = best_c >> 1, s = best_c & 1;
        Rigid rel, tag, win;
        load_rigid<true>(a.quad_qt + 14 * (b + d) + 7 * s, rel);
        load_rigid<true>(a.tag_qt + 7 * (int64_t)v.tag[d], tag);
        chain_camera(rel, tag, win);
        quat_from_R(win.R, q);
        q[4] = win.t[0];
        q[5] = win.t[1];
        q[6] = win.t[2];
    }
    // ---- classify -> refine on the inliers ----
    const bool robust = a.robustify != 0;
    int trials = 0;
    if (a.passes == 0)
        trials += refine_image<STAGED>(K, v, q, nullptr, robust, a.huber_a, a.max_trials, s_red);
    for (int pass = 0; pass < a.passes; ++pass) {
        const int n_in = classify_image<STAGED>(K, v, q, a.inlier2, flags, s_cnt);
        if (n_in < a.min_inliers)
            break;
        trials += refine_image<STAGED>(K, v, q, flags, robust, a.huber_a, a.max_trials, s_red);
    }
    // ---- the result: flags, covariance and statistics at the returned pose ----
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    bool ok = finite_bits(qn);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (k < 4)
            q[k] *= qn;
        ok = ok && finite_bits(q[k]);
    }
    if (!ok) {   // cannot happen with finite inputs; keeps the no-NaN promise for any input
        for (int d = tid; d < m; d += kLocThreads)
            flags[d] = 0;
        if (tid == 0)
            store_failure(a, p, m, VMM_BA_LOC_NO_CANDIDATE, trials);
        return;
    }
    vmm_ba_localize_result res;
    res.status = VMM_BA_LOC_OK;
    res.n_obs = m;
    res.trials = trials;
    res.rms_px = 0.0;
    res.cost = 0.0;
    res.n_inlier_obs = classify_image<STAGED>(K, v, q, a.inlier2, flags, s_cnt);
    double C[21];
    bool have_cov = false;
    if (res.n_inlier_obs > 0) {
        double A[21], g[6], raw2;
        const double cost = image_sums<STAGED, true>(K, v, q, flags, robust, a.huber_a, s_red, A, g, raw2);
        res.cost = 0.5 * cost;
        res.rms_px = sqrt(raw2 / (4.0 * res.n_inlier_obs));
        if (res.n_inlier_obs >= a.min_inliers) {
            have_cov = spd_inverse<6>(A, C);
            if (!have_cov)
                res.status = VMM_BA_LOC_SINGULAR;
        }
    }
    if (res.n_inlier_obs < a.min_inliers)
        res.status = VMM_BA_LOC_TOO_FEW_INLIERS;
    if (tid == 0)
        store_result(a, p, q, C, have_cov, res);
}

} // namespace

void launch_map_corners(hipStream_t st, int n_tags, const double* tag_qt, const double* tag_wh, double* corners)
{
    if (n_tags <= 0)
        return;
    hipLaunchKernelGGL(k_map_corners, dim3((unsigned)((n_tags + 255) / 256)), dim3(256), 0, st, n_tags, tag_qt, tag_wh, corners);
}

int localize_stage_capacity() { return kStage; }

// any_staged / any_unstaged: whether the batch holds an image of at most / more than localize_stage_capacity()
// observations; every workgroup of a launch whose kind its image is not leaves at once
void launch_localize(hipStream_t st, const LocalizeArgs& a, bool any_staged, bool any_unstaged)
{
    if (a.n_imgs <= 0)
        return;
    if (any_staged)
        hipLaunchKernelGGL(k_localize<true>, dim3((unsigned)a.n_imgs), dim3(kLocThreads), 0, st, a);
    if (any_unstaged)
        hipLaunchKernelGGL(k_localize<false>, dim3((unsigned)a.n_imgs), dim3(kLocThreads), 0, st, a);
}

int preload_localize_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_map_corners)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_localize<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_localize<false>)) != hipSuccess;
    return bad;
}

} // namespace vmm
