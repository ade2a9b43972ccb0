// Tag poses from known cameras (gfx950): vmm_ba_locate_tags, the dual of the localisation.
//   k_quad_pose       (kernels_init.hip, as it is) both planar tag->camera poses of every observation
//   k_camera_rigids   thread = camera: R | t of q / |q| (load_rigid<true>), once per call -- eval_corner's camera half
//                     hoisted out of the per-observation, per-trial arithmetic, as k_map_corners hoists the tag half
//   k_locate_tags     workgroup = tag, one launch from candidates to covariances:
//                     scoring   thread = candidate (two per observation, chained through the observing camera, chain_tag),
//                               truncated squared reprojection error over all the tag's corners in all its observations;
//                               the waves' winners meet in LDS and are taken in wave order (better / wave_winner)
//                     passes    classify the observations at the pose, Levenberg-Marquardt over the inliers: threads
//                               stride the observation list, 21 + 6 + 2 sums reduced by one butterfly per wave
//                               (wave_sum32) and combined in LDS in wave order; every thread runs the same 6 x 6 solve
//                     result    flags at the returned pose, H^-1 by a 6 x 6 Cholesky in registers, and once, behind the
//                               trial loop, sum G C G^T (camera_part: 21 sums through the same reduction)
// The single-pose solver is pose_lm.hpp's (lm_refine, better / wave_winner, chain_tag, quat_from_R, sandwich6) over small_solve.hpp's
// damped_solve<6> and spd_inverse<6>; the workgroup reductions are image_sums.hpp's (workgroup_count, workgroup_normal,
// workgroup_cost); the corner arithmetic is eval_corner<false, true> (geom.hpp), the residual and tag Jacobian of the
// bundle adjustment.  The tag's own pose is workgroup-uniform and expanded once per evaluation.  Here: the view of a
// tag's observations, the staging, the scoring, the sums over the tag's tangent and the propagation.
// A tag's pixels and camera rigids (20 doubles per observation) are staged in LDS when the tag has at most kStage
// observations (k_locate_tags<true>); longer tags read them from global memory (k_locate_tags<false>).  Both run the same
// arithmetic in the same order, and which one a tag takes depends on its own length alone.
// Nothing but the selection of the tag depends on blockIdx, no workgroup waits on another, there is no floating-point
// atomic and every sum has a fixed order (thread-private sums in list order, the wave butterfly, the waves in order):
// a tag gives the same bits alone, in any batch, at any position and from run to run.
//
// Registers (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, the .s file's .vgpr_count / .vgpr_spill_count /
// .private_segment_fixed_size): k_locate_tags<true> takes 354 and k_locate_tags<false> 334 registers per lane with no spill
// and a zero private segment, k_camera_rigids 34.  As in k_localize the compiler keeps a thread's own observation next to
// the 29 running sums, the pose and the 6 x 6 system, so the kernel runs one wave per SIMD = one 256-thread workgroup
// per CU, and the 41 KiB of LDS never limit it.  The propagation (camera_part: G, a row of G C and the 21 sums) runs
// once behind the trial loop and stays inside that budget with its corner loop rolled.
#include <limits.h>

#include "engine.hpp"
#include "image_sums.hpp"

namespace vmm {

namespace {

constexpr int kTagThreads = kImageThreads;
constexpr int kTagWaves = kImageWaves;
constexpr int kStage = 256;   // observations staged in LDS: 20 x 8 B x 256 = 40 KiB per workgroup

__global__ __launch_bounds__(256) void k_camera_rigids(int n_cams, const double* __restrict__ cam_qt, double* __restrict__ rigids)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cams)
        return;
    Rigid cam;
    load_rigid<true>(cam_qt + 7 * (int64_t)i, cam);
    double* const r = rigids + 12 * (int64_t)i;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        r[k] = cam.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        r[9 + k] = cam.t[k];
}

// One tag's observations: element k (0..7 pixels, 8..19 the observing camera's R | t) of local observation d.
template <bool STAGED>
struct TagView {
    const double* lds;        // STAGED: [20][m]
    int m;
    const double* px;         // obs_px + 8 * first observation
    const int32_t* cam;       // obs_cam + first observation
    const double* rigids;
    __device__ __forceinline__ double pixel(const int d, const int k) const
    {
        return STAGED ? lds[k * m + d] : px[8 * (int64_t)d + k];
    }
    __device__ __forceinline__ void camera(const int d, Rigid& c) const
    {
        const double* const r = rigids + (STAGED ? 0 : 12 * (int64_t)cam[d]);
#pragma unroll
        for (int k = 0; k < 9; ++k)
            c.R[k] = STAGED ? lds[(8 + k) * m + d] : r[k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            c.t[k] = STAGED ? lds[(17 + k) * m + d] : r[9 + k];
    }
};

// Truncated score of tag pose `tag` over all the tag's corners in all its observations.
template <bool STAGED>
__device__ __forceinline__ double score_tag(const Intrinsics& K, const TagView<STAGED>& v, const Rigid& tag, const double hw,
                                            const double hh, const double cap2)
{
    double sum = 0.0;
    for (int d = 0; d < v.m; ++d) {
        Rigid cam;
        v.camera(d, cam);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<false, false>(K, cam, tag, corner_sx(k) * hw, corner_sy(k) * hh, v.pixel(d, 2 * k), v.pixel(d, 2 * k + 1), ev);
            const double e2 = ev.ru * ev.ru + ev.rv * ev.rv;
            sum += e2 < cap2 ? e2 : (finite_bits(e2) ? cap2 : kInf);
        }
    }
    return sum;
}

// Flags the observations whose largest corner distance under tag pose q is at most sqrt(inlier2); every thread returns
// their number.  A non-finite distance is an outlier.
template <bool STAGED>
__device__ __forceinline__ int classify_tag(const Intrinsics& K, const TagView<STAGED>& v, const double* q, const double hw,
                                            const double hh, const double inlier2, uint8_t* flags, int* s_cnt)
{
    Rigid tag;
    load_rigid<true>(q, tag);
    int n = 0;
    for (int d = threadIdx.x; d < v.m; d += kTagThreads) {
        Rigid cam;
        v.camera(d, cam);
        bool in = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<false, false>(K, cam, tag, corner_sx(k) * hw, corner_sy(k) * hh, v.pixel(d, 2 * k), v.pixel(d, 2 * k + 1), ev);
            in = in && (ev.ru * ev.ru + ev.rv * ev.rv <= inlier2);
        }
        flags[d] = in ? 1 : 0;
        n += in ? 1 : 0;
    }
    return workgroup_count(n, s_cnt);
}

// Sums over the active observations (flags null: all) at tag pose q: returns the 1/2-free cost sum rho(|r_corner|^2); with
// JAC also Jt^T Jt (packed lower) and Jt^T r over the tag's tangent with the Huber corrector applied, and raw2 = sum |r|^2
// without the loss.  Every thread returns the same totals.
template <bool STAGED, bool JAC>
__device__ __forceinline__ double tag_sums(const Intrinsics& K, const TagView<STAGED>& v, const double* q, const double hw,
                                           const double hh, const uint8_t* flags, const bool robust, const double huber_a,
                                           double* s_red, double (&A)[21], double (&g)[6], double& raw2)
{
    Rigid tag;
    load_rigid<true>(q, tag);
    double cost = 0.0, raw = 0.0;
    if (JAC)
        zero_normal(A, g);
    for (int d = threadIdx.x; d < v.m; d += kTagThreads) {
        if (flags && flags[d] == 0)
            continue;
        Rigid cam;
        v.camera(d, cam);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<false, JAC>(K, cam, tag, corner_sx(k) * hw, corner_sy(k) * hh, v.pixel(d, 2 * k), v.pixel(d, 2 * k + 1), ev);
            const double s = ev.ru * ev.ru + ev.rv * ev.rv;
            double rho0, wgt;
            huber(robust, huber_a, s, rho0, wgt);
            cost += rho0;
            if (JAC) {
                raw += s;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    ev.jt[0][c] *= wgt;
                    ev.jt[1][c] *= wgt;
                }
                accumulate_rows(ev.jt, ev.ru * wgt, ev.rv * wgt, A, g);
            }
        }
    }
    if (JAC)
        return workgroup_normal(A, g, cost, raw, s_red, raw2);
    return workgroup_cost(cost, s_red);
}

// Levenberg-Marquardt on q (in place) over the active observations; returns the trials spent.  tag_sums gives every
// thread the workgroup's totals (and holds the barriers): the workgroup runs lm_refine as one.
template <bool STAGED>
__device__ __forceinline__ int refine_tag(const Intrinsics& K, const TagView<STAGED>& v, double (&q)[7], const double hw,
                                          const double hh, const uint8_t* flags, const bool robust, const double huber_a,
                                          const int max_trials, double* s_red)
{
    double cost, raw2;
    return lm_refine<true, false>(q, max_trials, [&](auto jac, const double* at, double (&A)[21], double (&g)[6]) {
        return tag_sums<STAGED, decltype(jac)::value>(K, v, at, hw, hh, flags, robust, huber_a, s_red, A, g, raw2);
    }, cost);
}

// sum_i G_i C_i G_i^T over the flagged observations (packed lower 6 x 6), G_i = sum over the four corners of
// rho' Jt^T Jc and C_i the observing camera's 6 x 6 block of cam_cov.  Runs once, at the returned pose, behind the trial
// loop; every thread returns the same totals.
template <bool STAGED>
__device__ __forceinline__ void camera_part(const Intrinsics& K, const TagView<STAGED>& v, const double* q, const double hw,
                                            const double hh, const uint8_t* flags, const bool robust, const double huber_a,
                                            const double* __restrict__ cam_cov, double* s_red, double (&S)[21])
{
    Rigid tag;
    load_rigid<true>(q, tag);
    double g[6];
    zero_normal(S, g);
    for (int d = threadIdx.x; d < v.m; d += kTagThreads) {
        if (flags[d] == 0)
            continue;
        Rigid cam;
        v.camera(d, cam);
        double G[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                G[a][c] = 0.0;
#pragma unroll 1   // rolled: unrolled, the four corners' Jacobians next to G cost the staged kernel four spilled registers
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<true, true>(K, cam, tag, corner_sx(k) * hw, corner_sy(k) * hh, v.pixel(d, 2 * k), v.pixel(d, 2 * k + 1), ev);
            double rho0, wgt;
            huber(robust, huber_a, ev.ru * ev.ru + ev.rv * ev.rv, rho0, wgt);
            const double w2 = wgt * wgt;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    G[a][c] += w2 * (ev.jt[0][a] * ev.jc[0][c] + ev.jt[1][a] * ev.jc[1][c]);
        }
        const double* const C = cam_cov + 36 * (int64_t)v.cam[d];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double T[6];   // row a of G C
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    t += G[a][k] * C[6 * k + c];
                T[c] = t;
            }
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    t += T[k] * G[b][k];
                S[tri6(a, b)] += t;
            }
        }
    }
    double raw2;
    workgroup_normal(S, g, 0.0, 0.0, s_red, raw2);
}

// What thread 0 stores for tag p; have_cov / have_cams false: a zero matrix.
__device__ __forceinline__ void store_tag(const LocateArgs& a, const int p, const double (&q)[7], const double (&C)[21],
                                          const bool have_cov, const double (&CC)[21], const bool have_cams,
                                          const vmm_ba_localize_result& res)
{
    double* const out_q = a.tag_qt + 7 * (int64_t)p;
    double* const out_cov = a.tag_cov + 36 * (int64_t)p;
    double* const out_cams = a.tag_cov_cams + 36 * (int64_t)p;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        out_q[k] = q[k];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            out_cov[6 * r + c] = have_cov ? sym6(C, r, c) : 0.0;
            out_cams[6 * r + c] = have_cams ? sym6(CC, r, c) : 0.0;
        }
    a.res[p] = res;
}

// NO_OBSERVATIONS / NO_CANDIDATE: the identity pose, zero covariances (the flags are zero already)
__device__ __forceinline__ void store_no_tag(const LocateArgs& a, const int p, const int m, const int status, const int trials)
{
    const double q[7] = { 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    vmm_ba_localize_result res;
    res.status = status;
    res.n_obs = m;
    res.n_inlier_obs = 0;
    res.trials = trials;
    res.rms_px = 0.0;
    res.cost = 0.0;
    const double Z[21] = {};
    store_tag(a, p, q, Z, false, Z, false, res);
}

template <bool STAGED>
__global__ __launch_bounds__(kTagThreads) void k_locate_tags(const LocateArgs a)
{
    __shared__ double s_obs[STAGED ? 20 * kStage : 1];
    __shared__ double s_red[kTagWaves * 32];
    __shared__ double s_best[kTagWaves];
    __shared__ int s_c[kTagWaves];
    __shared__ int s_cnt[kTagWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int64_t b = a.tag_start[p];
    const int m = (int)(a.tag_start[p + 1] - b);
    // every decision to leave depends on the tag alone or on values all threads hold alike: the whole workgroup
    // reaches the same barriers and leaves together
    if ((m <= kStage) != STAGED)
        return;
    if (m == 0) {
        if (tid == 0)
            store_no_tag(a, p, m, VMM_BA_LOC_NO_OBSERVATIONS, 0);
        return;
    }
    uint8_t* const flags = a.obs_inlier + b;
    const Intrinsics K = a.K;
    const double hw = 0.5 * a.tag_wh[2 * (int64_t)p], hh = 0.5 * a.tag_wh[2 * (int64_t)p + 1];
    TagView<STAGED> v;
    v.lds = s_obs;
    v.m = m;
    v.px = a.obs_px + 8 * b;
    v.cam = a.obs_cam + b;
    v.rigids = a.rigids;
    for (int d = tid; d < m; d += kTagThreads)
        flags[d] = 0;
    if (STAGED) {
        for (int i = tid; i < 8 * m; i += kTagThreads)   // coalesced read of the tag's pixels, transposed store
            s_obs[(i & 7) * m + (i >> 3)] = v.px[i];
        for (int i = tid; i < 12 * m; i += kTagThreads) {
            const int d = i / 12, k = i - 12 * d;
            s_obs[(8 + k) * m + d] = a.rigids[12 * (int64_t)v.cam[d] + k];
        }
        __syncthreads();
    }
    // ---- candidates ----
    double best = kInf;
    int best_c = INT_MAX;
    for (int c = tid; c < 2 * m; c += kTagThreads) {
        const int d = c >> 1, s = c & 1;
        if (!(a.quad_rms[2 * (b + d) + s] < kInf))
            continue;
        Rigid rel, cam, cand;
        load_rigid<true>(a.quad_qt + 14 * (b + d) + 7 * s, rel);
        v.camera(d, cam);
        chain_tag(rel, cam, cand);
        const double sc = score_tag<STAGED>(K, v, cand, hw, hh, a.cap2);
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
    for (int w = 1; w < kTagWaves; ++w)
        if (better(s_best[w], s_c[w], best, best_c)) {
            best = s_best[w];
            best_c = s_c[w];
        }
    if (!(best < kInf)) {
        if (tid == 0)
            store_no_tag(a, p, m, VMM_BA_LOC_NO_CANDIDATE, 0);
        return;
    }
    double q[7];
    {
        const int d = best_c >> 1, s = best_c & 1;
        Rigid rel, cam, win;
        load_rigid<true>(a.quad_qt + 14 * (b + d) + 7 * s, rel);
        v.camera(d, cam);
        chain_tag(rel, cam, win);
        quat_from_R(win.R, q);
        q[4] = win.t[0];
        q[5] = win.t[1];
        q[6] = win.t[2];
    }
    // ---- classify -> refine on the inliers ----
    const bool robust = a.robustify != 0;
    int trials = 0;
    if (a.passes == 0)
        trials += refine_tag<STAGED>(K, v, q, hw, hh, nullptr, robust, a.huber_a, a.max_trials, s_red);
    for (int pass = 0; pass < a.passes; ++pass) {
        const int n_in = classify_tag<STAGED>(K, v, q, hw, hh, a.inlier2, flags, s_cnt);
        if (n_in < a.min_inliers)
            break;
        trials += refine_tag<STAGED>(K, v, q, hw, hh, flags, robust, a.huber_a, a.max_trials, s_red);
    }
    // ---- the result: flags, covariances and statistics at the returned pose ----
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    bool ok = finite_bits(qn);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (k < 4)
            q[k] *= qn;
        ok = ok && finite_bits(q[k]);
    }
    if (!ok) {   // cannot happen with finite inputs; keeps the no-NaN promise for any input
        for (int d = tid; d < m; d += kTagThreads)
            flags[d] = 0;
        if (tid == 0)
            store_no_tag(a, p, m, VMM_BA_LOC_NO_CANDIDATE, trials);
        return;
    }
    vmm_ba_localize_result res;
    res.status = VMM_BA_LOC_OK;
    res.n_obs = m;
    res.trials = trials;
    res.rms_px = 0.0;
    res.cost = 0.0;
    res.n_inlier_obs = classify_tag<STAGED>(K, v, q, hw, hh, a.inlier2, flags, s_cnt);
    double C[21], CC[21];
    bool have_cov = false, have_cams = false;
    if (res.n_inlier_obs > 0) {
        double H[21], g[6], raw2;
        const double cost = tag_sums<STAGED, true>(K, v, q, hw, hh, flags, robust, a.huber_a, s_red, H, g, raw2);
        if (finite_bits(cost) && finite_bits(raw2)) {
            res.cost = 0.5 * cost;
            res.rms_px = sqrt(raw2 / (4.0 * res.n_inlier_obs));
        }
        if (res.n_inlier_obs >= a.min_inliers) {
            have_cov = spd_inverse<6>(H, C);
            if (!have_cov)
                res.status = VMM_BA_LOC_SINGULAR;
        }
        if (have_cov && a.cam_cov) {   // workgroup-uniform: every thread holds the same H
            double S[21];
            camera_part<STAGED>(K, v, q, hw, hh, flags, robust, a.huber_a, a.cam_cov, s_red, S);
            have_cams = sandwich6(C, S, CC);
        }
    }
    if (res.n_inlier_obs < a.min_inliers)
        res.status = VMM_BA_LOC_TOO_FEW_INLIERS;
    if (tid == 0)
        store_tag(a, p, q, C, have_cov, CC, have_cams, res);
}

} // namespace

void launch_camera_rigids(hipStream_t st, int n_cams, const double* cam_qt, double* rigids)
{
    if (n_cams <= 0)
        return;
    hipLaunchKernelGGL(k_camera_rigids, dim3((unsigned)((n_cams + 255) / 256)), dim3(256), 0, st, n_cams, cam_qt, rigids);
}

int locate_stage_capacity() { return kStage; }

// any_staged / any_unstaged: whether the batch holds a tag of at most / more than locate_stage_capacity() observations;
// every workgroup of a launch whose kind its tag is not leaves at once
void launch_locate_tags(hipStream_t st, const LocateArgs& a, bool any_staged, bool any_unstaged)
{
    if (a.n_tags <= 0)
        return;
    if (any_staged)
        hipLaunchKernelGGL(k_locate_tags<true>, dim3((unsigned)a.n_tags), dim3(kTagThreads), 0, st, a);
    if (any_unstaged)
        hipLaunchKernelGGL(k_locate_tags<false>, dim3((unsigned)a.n_tags), dim3(kTagThreads), 0, st, a);
}

int preload_locate_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_camera_rigids)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_locate_tags<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_locate_tags<false>)) != hipSuccess;
    return bad;
}

} // namespace vmm
