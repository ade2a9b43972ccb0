// A rigid multi-camera rig against a finished map (gfx950): vmm_ba_rig_localize, and below it the kernels of
// vmm_ba_rig_calibrate.
//
// A frame is what the rig's K cameras saw at one instant: the images f K .. f K + K - 1 of the batch, whose
// observations lie next to each other, camera by camera.  Camera c of frame f stands at ext_c o rig_f (R = R_c R_f,
// t = R_c t_f + t_c), and the frame's only unknown is the world->rig pose rig_f.  k_rig_localize is k_localize
// (kernels_localize.hip) with that composed pose and the observing camera's own model behind every corner:
//   k_quad_pose     (kernels_init.hip, as it is) one launch per camera over that camera's observations
//   k_map_corners   (kernels_localize.hip, as it is)
//   k_rig_localize  workgroup = frame, one launch from candidates to covariance:
//                   scoring   thread = candidate (two per observation): the planar pose chained through the map tag to
//                             the observing camera and from there to the rig, T_c^-1 o T_rel o T_tag^-1, scored over the
//                             corners of all the frame's cameras
//                   passes    classify at the rig pose, Levenberg-Marquardt on its 6 degrees of freedom over the inliers
//                   result    flags at the returned pose, (J^T J)^-1 in the rig's tangent
// The Jacobian over the rig's tangent is the camera Jacobian of project_camera_point (pose_lm.hpp) turned into the rig
// frame: a step (dt, dtheta) of the rig moves camera c by (R_c dt, R_c dtheta), so both halves of a row are multiplied
// by R_c from the right.
// The solver (lm_refine, better / wave_winner, chain_camera / chain_tag) is pose_lm.hpp's over small_solve.hpp (the
// damped 6 x 6 solve, spd_inverse<6>) and the reductions and the stores of a result are image_sums.hpp's, as in k_localize.  The localisation's body and its four
// per-observation loops stay a copy of kernels_localize.hip's with the camera looked up per observation: as one
// template over both (tried: DESIGN.md section 9) the same arithmetic compiled to other bits.  The K camera models and extrinsics
// (21 doubles each) are expanded into LDS once per workgroup; a thread reads the ones of its observation's camera from
// there, so nothing is indexed at run time in registers.  Pixels and world corners are read from global memory (the
// view k_localize<false> uses): a frame is read by its own workgroup only and stays in the CU's cache, and one code
// path serves frames of every length.
// Nothing but the selection of the frame depends on blockIdx, no workgroup waits on another, there is no floating-point
// atomic and every sum has a fixed order (thread-private sums in list order, the wave butterfly, the waves in order):
// a frame gives the same bits alone, in any batch and from run to run.
//
// Registers (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, the .s file's .vgpr_count / .vgpr_spill_count /
// .private_segment_fixed_size): k_rig_localize takes 326 registers per lane with no spill and a zero private
// segment; one 256-thread workgroup per CU, as k_localize.
#include <limits.h>

#include "arrowhead.hpp"

namespace vmm {

namespace {

constexpr int kRigModel = 21;   // doubles of a camera in LDS: fx fy cx cy k1 k2 p1 p2 k3 | R_c (9, row-major) | t_c (3)

// A frame as its workgroup sees it.
struct RigView {
    ImageView<false> v;     // the observations of all the frame's cameras, camera by camera
    const double* model;    // LDS [kRigModel * K]
    const int* end;         // LDS [VMM_BA_RIG_MAX_CAMS]: where camera c's observations end in the frame; INT_MAX from K on
    // the camera that made local observation d
    __device__ __forceinline__ int camera(const int d) const
    {
        int c = 0;
#pragma unroll
        for (int k = 0; k < VMM_BA_RIG_MAX_CAMS - 1; ++k)
            c += d >= end[k] ? 1 : 0;
        return c;
    }
    __device__ __forceinline__ Intrinsics intrinsics(const int c) const
    {
        const double* m = model + kRigModel * c;
        return Intrinsics{ m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8] };
    }
    __device__ __forceinline__ void extrinsic(const int c, Rigid& ext) const
    {
        const double* m = model + kRigModel * c + 9;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            ext.R[k] = m[k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            ext.t[k] = m[9 + k];
    }
};

// Frame p as its workgroup sees it: the K models and the extrinsics of ext_qt expanded into s_model, the ends of the
// cameras' ranges into s_end.  The caller's next barrier publishes them.
__device__ __forceinline__ RigView open_frame(const RigArgs& ra, const double* ext_qt, const int p, double* s_model, int* s_end)
{
    const LocalizeArgs& a = ra.loc;
    const int tid = threadIdx.x, n_cams = ra.n_rig_cams;
    const int64_t* const start = a.img_start + (int64_t)p * n_cams;
    const int64_t b = start[0];
    if (tid < n_cams) {
        double* const mdl = s_model + kRigModel * tid;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            mdl[k] = k < 4 ? ra.intr[4 * tid + k] : ra.dist[5 * tid + k - 4];
        Rigid ext;
        load_rigid<true>(ext_qt + 7 * tid, ext);
#pragma unroll
        for (int k = 0; k < 9; ++k)
            mdl[9 + k] = ext.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            mdl[18 + k] = ext.t[k];
    }
    if (tid < VMM_BA_RIG_MAX_CAMS)
        s_end[tid] = tid < n_cams ? (int)(start[tid + 1] - b) : INT_MAX;
    RigView f;
    f.v.lds = nullptr;
    f.v.m = (int)(start[n_cams] - b);
    f.v.px = a.obs_px + 8 * b;
    f.v.tag = a.obs_tag + b;
    f.v.corners = a.corners;
    f.model = s_model;
    f.end = s_end;
    return f;
}

// T_cam = T_ext o T_rig
__device__ __forceinline__ void compose_camera(const Rigid& ext, const Rigid& rig, Rigid& cam)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            cam.R[3 * i + j] = ext.R[3 * i] * rig.R[j] + ext.R[3 * i + 1] * rig.R[3 + j] + ext.R[3 * i + 2] * rig.R[6 + j];
        cam.t[i] = (ext.R[3 * i] * rig.t[0] + ext.R[3 * i + 1] * rig.t[1] + ext.R[3 * i + 2] * rig.t[2]) + ext.t[i];
    }
}

// Corner k of local observation d under the rig pose `rig`: the residual in the observing camera and, with JAC, its
// 2 x 6 Jacobian over the rig's tangent.  K, ext, cam: the observing camera's model, extrinsic and composed pose.
template <bool JAC>
__device__ __forceinline__ void rig_corner(const RigView& f, const Intrinsics& K, const Rigid& ext, const Rigid& cam, const int d,
                                           const int k, double& ru, double& rv, double (&j)[2][6])
{
    double jc[2][6];
    world_corner<JAC>(K, cam, f.v.world(d, 3 * k), f.v.world(d, 3 * k + 1), f.v.world(d, 3 * k + 2), f.v.pixel(d, 2 * k),
                      f.v.pixel(d, 2 * k + 1), ru, rv, jc);
    if (!JAC)
        return;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int h = 0; h < 6; h += 3)
#pragma unroll
            for (int a = 0; a < 3; ++a)
                j[r][h + a] = jc[r][h] * ext.R[a] + jc[r][h + 1] * ext.R[3 + a] + jc[r][h + 2] * ext.R[6 + a];
}

// Truncated score of the rig pose `rig` over all the frame's corners.
__device__ __forceinline__ double score_frame(const RigView& f, const Rigid& rig, const double cap2)
{
    double sum = 0.0;
    for (int d = 0; d < f.v.m; ++d) {
        const int c = f.camera(d);
        const Intrinsics K = f.intrinsics(c);
        Rigid ext, cam;
        f.extrinsic(c, ext);
        compose_camera(ext, rig, cam);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ru, rv, j[2][6];
            rig_corner<false>(f, K, ext, cam, d, k, ru, rv, j);
            const double e2 = ru * ru + rv * rv;
            sum += e2 < cap2 ? e2 : (finite_bits(e2) ? cap2 : kInf);
        }
    }
    return sum;
}

// classify_image (image_sums.hpp) for a frame at the rig pose q
__device__ __forceinline__ int classify_frame(const RigView& f, const double* q, const double inlier2, uint8_t* flags, int* s_cnt)
{
    Rigid rig;
    load_rigid<true>(q, rig);
    int n = 0;
    for (int d = threadIdx.x; d < f.v.m; d += kImageThreads) {
        const int c = f.camera(d);
        const Intrinsics K = f.intrinsics(c);
        Rigid ext, cam;
        f.extrinsic(c, ext);
        compose_camera(ext, rig, cam);
        bool in = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ru, rv, j[2][6];
            rig_corner<false>(f, K, ext, cam, d, k, ru, rv, j);
            in = in && (ru * ru + rv * rv <= inlier2);
        }
        flags[d] = in ? 1 : 0;
        n += in ? 1 : 0;
    }
    return workgroup_count(n, s_cnt);
}

// image_sums (image_sums.hpp) for a frame at the rig pose q, over the rig's tangent
template <bool JAC>
__device__ __forceinline__ double frame_sums(const RigView& f, const double* q, const uint8_t* flags, const bool robust,
                                             const double huber_a, double* s_red, double (&A)[21], double (&g)[6], double& raw2)
{
    Rigid rig;
    load_rigid<true>(q, rig);
    double cost = 0.0, raw = 0.0;
    if (JAC)
        zero_normal(A, g);
    for (int d = threadIdx.x; d < f.v.m; d += kImageThreads) {
        if (flags && flags[d] == 0)
            continue;
        const int c = f.camera(d);
        const Intrinsics K = f.intrinsics(c);
        Rigid ext, cam;
        f.extrinsic(c, ext);
        compose_camera(ext, rig, cam);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ru, rv, j[2][6];
            rig_corner<JAC>(f, K, ext, cam, d, k, ru, rv, j);
            const double s = ru * ru + rv * rv;
            double rho0, wgt;
            huber(robust, huber_a, s, rho0, wgt);
            cost += rho0;
            if (JAC) {
                raw += s;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    j[0][a] *= wgt;
                    j[1][a] *= wgt;
                }
                accumulate_rows(j, ru * wgt, rv * wgt, A, g);
            }
        }
    }
    if (JAC)
        return workgroup_normal(A, g, cost, raw, s_red, raw2);
    return workgroup_cost(cost, s_red);
}

// Levenberg-Marquardt on the rig pose q (in place) over the active observations; returns the trials spent.  The
// workgroup runs lm_refine as one, as refine_image of kernels_localize.hip.
__device__ __forceinline__ int refine_frame(const RigView& f, double (&q)[7], const uint8_t* flags, const bool robust,
                                            const double huber_a, const int max_trials, double* s_red)
{
    double cost, raw2;
    return lm_refine<true, false>(q, max_trials, [&](auto jac, const double* at, double (&A)[21], double (&g)[6]) {
        return frame_sums<decltype(jac)::value>(f, at, flags, robust, huber_a, s_red, A, g, raw2);
    }, cost);
}

// The rig pose that candidate c of the frame (solution c & 1 of local observation c >> 1) stands for.
__device__ __forceinline__ void candidate_rig(const RigArgs& ra, const RigView& f, const int64_t b, const int c, Rigid& rig)
{
    const LocalizeArgs& a = ra.loc;
    const int d = c >> 1, s = c & 1;
    Rigid rel, tag, cam, ext;
    load_rigid<true>(a.quad_qt + 14 * (b + d) + 7 * s, rel);
    load_rigid<true>(a.tag_qt + 7 * (int64_t)f.v.tag[d], tag);
    chain_camera(rel, tag, cam);
    f.extrinsic(f.camera(d), ext);
    chain_tag(cam, ext, rig);   // T_ext^-1 o T_cam
}

__global__ __launch_bounds__(kImageThreads) void k_rig_localize(const RigArgs ra)
{
    __shared__ double s_model[kRigModel * VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_end[VMM_BA_RIG_MAX_CAMS];
    __shared__ double s_red[kImageWaves * 32];
    __shared__ double s_best[kImageWaves];
    __shared__ int s_c[kImageWaves];
    __shared__ int s_cnt[kImageWaves];
    const LocalizeArgs& a = ra.loc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x, n_cams = ra.n_rig_cams;
    const int64_t* const start = a.img_start + (int64_t)p * n_cams;
    const int64_t b = start[0];
    const int m = (int)(start[n_cams] - b);
    // every decision to leave depends on the frame alone or on values all threads hold alike: the whole workgroup
    // reaches the same barriers and leaves together
    if (m == 0) {
        if (tid == 0)
            store_failure(a, p, m, VMM_BA_LOC_NO_OBSERVATIONS, 0);
        return;
    }
    uint8_t* const flags = a.obs_inlier + b;
    const RigView f = open_frame(ra, ra.ext_qt, p, s_model, s_end);
    for (int d = tid; d < m; d += kImageThreads)
        flags[d] = 0;
    __syncthreads();
    // ---- candidates ----
    double best = kInf;
    int best_c = INT_MAX;
    for (int c = tid; c < 2 * m; c += kImageThreads) {
        if (!(a.quad_rms[2 * b + c] < kInf))
            continue;
        Rigid cand;
        candidate_rig(ra, f, b, c, cand);
        const double sc = score_frame(f, cand, a.cap2);
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
    for (int w = 1; w < kImageWaves; ++w)
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
        Rigid win;
        candidate_rig(ra, f, b, best_c, win);
        quat_from_R(win.R, q);
        q[4] = win.t[0];
        q[5] = win.t[1];
        q[6] = win.t[2];
    }
    // ---- classify -> refine on the inliers ----
    const bool robust = a.robustify != 0;
    int trials = 0;
    if (a.passes == 0)
        trials += refine_frame(f, q, nullptr, robust, a.huber_a, a.max_trials, s_red);
    for (int pass = 0; pass < a.passes; ++pass) {
        const int n_in = classify_frame(f, q, a.inlier2, flags, s_cnt);
        if (n_in < a.min_inliers)
            break;
        trials += refine_frame(f, q, flags, robust, a.huber_a, a.max_trials, s_red);
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
        for (int d = tid; d < m; d += kImageThreads)
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
    res.n_inlier_obs = classify_frame(f, q, a.inlier2, flags, s_cnt);
    double C[21];
    bool have_cov = false;
    if (res.n_inlier_obs > 0) {
        double A[21], g[6], raw2;
        const double cost = frame_sums<true>(f, q, flags, robust, a.huber_a, s_red, A, g, raw2);
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

// ---- vmm_ba_rig_calibrate: the extrinsics and one rig pose per frame, refined together ---------------------------------
// The arrowhead of arrowhead.hpp with the 6 K extrinsic parameters as the shared unknowns: every frame eliminates its own
// 6 x 6 block and what is left is P x P, P = 6 K.  What the kernels below share with kernels_calibrate.hip is that
// header's (the list is at its top); their own: one corner's 2 x 12 rows, spreading a camera's sums over the frame's
// blocks, and the P x P system in LDS.  One Levenberg-Marquardt trial:
//   k_rigcal_frame    workgroup = frame.  An observation touches the rig pose and ONE extrinsic, so the frame's sums are
//                     formed camera by camera as 12 x 12 packed blocks (78 + 12 + 2 sums: thread-private in list order,
//                     one butterfly per wave -- wave_sum32, three times --, the waves in order through LDS) and spread
//                     over A (cameras added in order), B, the block-diagonal C and the gradients; then L = chol(A + lam
//                     diag), Y = L^-1 B, y = L^-1 g and the record: C - Y'Y, g_e - Y'y, diag(C), cost, L, Y, y
//   k_rigcal_solve    one workgroup: the records summed in a fixed order (four interleaved chains, combined in order),
//                     damped with lam diag(sum C), Jacobi-scaled, unit rows for the extrinsics that are held or have no
//                     inlier observation, P x P Cholesky in LDS (every entry's updates in column order), the step and
//                     the candidate extrinsics
//   k_rigcal_try      workgroup = frame: d rig = -L^-T (y + Y d ext), candidate pose, cost-only pass at the candidates
//   k_rigcal_control  one workgroup: lm_refine's accept / stop rules on the whole problem (arrow_control)
// At the result k_rigcal_frame and k_rigcal_solve run once more with lam = 0 (cov_mode): S^-1 = ext_cov, and
// k_rigcal_cov_pose forms rig_cov_f = L^-T (I + Y S^-1 Y') L^-1.  Every sum has a fixed order; the sum over the frames
// makes the bits depend on the order of the batch.
//                         .vgpr_count  .vgpr_spill_count  .private_segment_fixed_size
//   k_rigcal_frame        364          0                  0      (92 running sums = 184 registers, one corner's 2 x 12 rows)
//   k_rigcal_solve        56           0                  0      (the 48 x 48 system lives in 30 KiB of LDS)
//   k_rigcal_try          152          0                  0
//   k_rigcal_classify 100, k_rigcal_cov_pose 86, k_rigcal_control 18, k_rigcal_begin 6: no spill, no private segment

using RcSums = Wide<12>;        // 92 sums: 78 (12 x 12 packed lower: rig 0..5, extrinsic 6..11) + 12 gradient + cost + sum |r|^2
constexpr int kRcThreads = kImageThreads;

static_assert(RcSums::kSums == 92 && RcSums::kChunks == 3, "the layout k_rigcal_frame spreads");

__global__ __launch_bounds__(64) void k_rigcal_begin(const RigCalArgs a)
{
    arrow_begin(a.w, a.rig.loc.res, a.rig.loc.n_imgs);
}

// workgroup = frame: the localisation's classification under the current extrinsics, for the localised frames
__global__ __launch_bounds__(kRcThreads) void k_rigcal_classify(const RigCalArgs a)
{
    __shared__ double s_model[kRigModel * VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_end[VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_cnt[kImageWaves];
    const int p = blockIdx.x;
    const LocalizeArgs& la = a.rig.loc;
    if (la.res[p].status != VMM_BA_LOC_OK)
        return;
    const RigView f = open_frame(a.rig, a.ctl->ext, p, s_model, s_end);
    __syncthreads();
    const int n = classify_frame(f, la.cam_qt + 7 * (int64_t)p, a.w.inlier2,
                                 la.obs_inlier + la.img_start[(int64_t)p * a.rig.n_rig_cams], s_cnt);
    if (threadIdx.x == 0) {
        a.w.n_in[p] = n;
        a.w.part[p] = n >= a.w.min_inliers;
    }
}

// The sums of camera c's inlier observations of a frame into s_tot: the packed lower triangle of the 12 x 12 normal
// matrix over (rig pose, extrinsic c) (0..77), the gradient (78..89), the cost (90) and sum |r|^2 (91), the Huber
// corrector applied.  free_c false: the extrinsic is held and its columns are zero.
__device__ __forceinline__ void camera_normal_sums(const RigView& f, const uint8_t* flags, const int c, const Rigid& rig,
                                                   const bool free_c, const bool robust, const double huber_a, double* s_red,
                                                   double* s_tot)
{
    const int tid = threadIdx.x;
    RcSums sums;
    sums.zero();
    const Intrinsics K = f.intrinsics(c);
    Rigid ext, cam;
    f.extrinsic(c, ext);
    compose_camera(ext, rig, cam);
    const double v0 = cam.t[0] - ext.t[0], v1 = cam.t[1] - ext.t[1], v2 = cam.t[2] - ext.t[2];   // R_c t_f
    const int lo = c > 0 ? f.end[c - 1] : 0, hi = f.end[c];
    for (int d = lo + tid; d < hi; d += kRcThreads) {
        if (flags[d] == 0)
            continue;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {   // not unrolled, as in k_calib_image: the sums need the registers
            double ru, rv, jc[2][6];
            world_corner<true>(K, cam, f.v.world(d, 3 * k), f.v.world(d, 3 * k + 1), f.v.world(d, 3 * k + 2), f.v.pixel(d, 2 * k),
                               f.v.pixel(d, 2 * k + 1), ru, rv, jc);
            const double s = ru * ru + rv * rv;
            double rho0, wgt;
            huber(robust, huber_a, s, rho0, wgt);
            double J[2][12];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                // the rig: both halves of the camera row turned into the rig frame
#pragma unroll
                for (int h = 0; h < 6; h += 3)
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        J[r][h + e] = (jc[r][h] * ext.R[e] + jc[r][h + 1] * ext.R[3 + e] + jc[r][h + 2] * ext.R[6 + e]) * wgt;
                // the extrinsic: a step (ds, dphi) moves the camera by (ds + 2 dphi x (R_c t_f), dphi)
                const double g0 = jc[r][0], g1 = jc[r][1], g2 = jc[r][2];
                J[r][6] = free_c ? g0 * wgt : 0.0;
                J[r][7] = free_c ? g1 * wgt : 0.0;
                J[r][8] = free_c ? g2 * wgt : 0.0;
                J[r][9] = free_c ? (jc[r][3] + 2.0 * (v1 * g2 - v2 * g1)) * wgt : 0.0;
                J[r][10] = free_c ? (jc[r][4] + 2.0 * (v2 * g0 - v0 * g2)) * wgt : 0.0;
                J[r][11] = free_c ? (jc[r][5] + 2.0 * (v0 * g1 - v1 * g0)) * wgt : 0.0;
            }
            ru *= wgt;
            rv *= wgt;
            sums.add(J, ru, rv, rho0, s);
        }
    }
    sums.reduce(s_red, s_tot);
}

__global__ __launch_bounds__(kRcThreads) void k_rigcal_frame(const RigCalArgs a, const int cov_mode)
{
    __shared__ double s_model[kRigModel * VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_end[VMM_BA_RIG_MAX_CAMS];
    __shared__ double s_red[kImageWaves * 32 * RcSums::kChunks];
    __shared__ double s_tot[32 * RcSums::kChunks];
    __shared__ double s_A[21], s_g[6], s_stat[2], s_L[21];
    __shared__ double s_B[6][kRigDof], s_C[VMM_BA_RIG_MAX_CAMS][21], s_gk[kRigDof];
    __shared__ double s_Y[6][kRigDof + 1];   // column P: y
    __shared__ int s_bad;
    const RigCalCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->lm.done)
        return;
    const LocalizeArgs& la = a.rig.loc;
    const int tid = threadIdx.x, p = blockIdx.x, n_cams = a.rig.n_rig_cams;
    const int P = 6 * n_cams, n_rec = arrow_rec_doubles(P), n_el = arrow_elim_doubles(P);
    double* const rec = a.w.rec + n_rec * (int64_t)p;
    double* const el = a.w.elim + n_el * (int64_t)p;
    if (!a.w.part[p]) {
        for (int e = tid; e < n_rec; e += kRcThreads)
            rec[e] = 0.0;
        return;
    }
    const RigView f = open_frame(a.rig, ctl->ext, p, s_model, s_end);
    if (tid < 21)
        s_A[tid] = 0.0;
    if (tid < 6)
        s_g[tid] = 0.0;
    if (tid < 2)
        s_stat[tid] = 0.0;
    __syncthreads();
    const uint8_t* const flags = la.obs_inlier + la.img_start[(int64_t)p * n_cams];
    const int mask = ctl->lm.refine_mask;
    Rigid rig;
    load_rigid<true>(la.cam_qt + 7 * (int64_t)p, rig);
    for (int c = 0; c < n_cams; ++c) {
        camera_normal_sums(f, flags, c, rig, (mask >> c) & 1, a.w.robustify != 0, a.w.huber_a, s_red, s_tot);
        // every LDS entry below has one writer per camera
        if (tid < 78) {
            const int i = packed_row(tid), j = tid - tri6(i, 0);
            const double v = s_tot[tid];
            if (i < 6)
                s_A[tid] += v;
            else if (j < 6)
                s_B[j][6 * c + i - 6] = v;
            else
                s_C[c][tri6(i - 6, j - 6)] = v;
        } else if (tid < 84) {
            s_g[tid - 78] += s_tot[tid];
        } else if (tid < 90) {
            s_gk[6 * c + tid - 84] = s_tot[tid];
        } else if (tid < 92) {
            s_stat[tid - 90] += s_tot[tid];
        }
        __syncthreads();
    }
    if (tid == 0)
        s_bad = damped_chol6(s_A, cov_mode ? 0.0 : ctl->lm.lam, s_L) ? 0 : 1;
    __syncthreads();
    // column c of Y = L^-1 B (c < P) and y = L^-1 g (c == P)
    if (tid <= P)
        forward_column6(s_L, [&](const int i) { return tid < P ? s_B[i][tid] : s_g[i]; }, &s_Y[0][tid], kRigDof + 1);
    __syncthreads();
    const double cost = s_stat[0], raw2 = s_stat[1];
    const bool bad = s_bad != 0;
    const int n_in = a.w.n_in[p];
    for (int e = tid; e < n_rec; e += kRcThreads)   // C is block-diagonal
        rec[e] = arrow_record_entry(e, P, [&](const int i, const int j) { return i / 6 == j / 6 ? s_C[i / 6][tri6(i % 6, j % 6)] : 0.0; },
                                    [&](const int c) { return s_gk[c]; }, &s_Y[0][0], kRigDof + 1, cost, raw2, bad, n_in);
    for (int e = tid; e < n_el; e += kRcThreads)
        el[e] = arrow_elim_entry(e, P, s_L, &s_Y[0][0], kRigDof + 1);
}

__global__ __launch_bounds__(kRcThreads) void k_rigcal_solve(const RigCalArgs a, const int cov_mode)
{
    constexpr int kMaxTri = kRigDof * (kRigDof + 1) / 2;
    __shared__ double s_tot[kMaxTri + 2 * kRigDof + 5];
    __shared__ double s_M[kMaxTri], s_W[kMaxTri];
    __shared__ double s_sc[kRigDof], s_wt[kRigDof], s_z[kRigDof];
    __shared__ int s_act[kRigDof];
    __shared__ int s_go, s_ok;
    RigCalCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->lm.done)
        return;
    const int tid = threadIdx.x, n_cams = a.rig.n_rig_cams, n_frames = a.rig.loc.n_imgs;
    const int P = 6 * n_cams, T = P * (P + 1) / 2, n_rec = arrow_rec_doubles(P);
    for (int e = tid; e < n_rec; e += kRcThreads) {
        double t[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int i = 0; i < n_frames; i += 4)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (i + g < n_frames)
                    t[g] += a.w.rec[n_rec * (int64_t)(i + g) + e];
        s_tot[e] = ((t[0] + t[1]) + t[2]) + t[3];
    }
    __syncthreads();
    const double* const st = s_tot + arrow_rec_stat(P);
    const double lam = cov_mode ? 0.0 : ctl->lm.lam;
    if (tid == 0) {
        s_go = arrow_solve_begin(ctl->lm, st, cov_mode, lam) ? 1 : 0;
        s_ok = st[2] == 0.0 ? 1 : 0;
    }
    __syncthreads();
    if (!s_go)
        return;
    // damp, give the extrinsics that are held or unobserved unit rows, scale to a unit diagonal
    const int mask = ctl->lm.refine_mask;
    if (tid < P) {
        const bool act = ((mask >> (tid / 6)) & 1) && s_tot[arrow_rec_diag(P) + 6 * (tid / 6)] > 0.0;
        const double cjj = s_tot[arrow_rec_diag(P) + tid];
        const double d = act ? s_tot[tri6(tid, tid)] + lam * cjj : 1.0;
        if (!(d > 0.0 && finite_bits(d)))
            s_ok = 0;   // every writer writes 0
        s_act[tid] = act ? 1 : 0;
        s_sc[tid] = act ? 1.0 / sqrt(d) : 1.0;
        s_wt[tid] = cov_mode && act ? d / cjj : 1.0;   // S_jj / C_jj
    }
    __syncthreads();
    for (int e = tid; e < T; e += kRcThreads) {
        const int i = packed_row(e), j = e - tri6(i, 0);
        s_M[e] = i == j ? 1.0 : (s_act[i] && s_act[j] ? s_tot[e] * s_sc[i] * s_sc[j] : 0.0);
    }
    __syncthreads();
    // Cholesky in place, column by column: every entry receives its updates in column order
    const double min_pivot = cov_mode ? kMinPivot : 0.0;
    for (int j = 0; j < P; ++j) {
        if (tid == 0) {
            const double d = s_M[tri6(j, j)];
            if (!(d * s_wt[j] > min_pivot && finite_bits(d)))
                s_ok = 0;
            s_M[tri6(j, j)] = sqrt(d);
        }
        __syncthreads();
        const double is = 1.0 / s_M[tri6(j, j)];
        for (int i = j + 1 + tid; i < P; i += kRcThreads)
            s_M[tri6(i, j)] *= is;
        __syncthreads();
        const int n = P - 1 - j;
        for (int e = tid; e < n * (n + 1) / 2; e += kRcThreads) {
            const int r = packed_row(e), i = j + 1 + r, k = j + 1 + e - tri6(r, 0);
            s_M[tri6(i, k)] -= s_M[tri6(i, j)] * s_M[tri6(k, j)];
        }
        __syncthreads();
    }
    if (cov_mode) {
        // S^-1 = D (L L')^-1 D with the rows and columns of the inactive extrinsics zero: W = L^-1 column by column,
        // then W'W
        if (tid < P) {
            const int j = tid;
            s_W[tri6(j, j)] = 1.0 / s_M[tri6(j, j)];
            for (int i = j + 1; i < P; ++i) {
                double v = 0.0;
                for (int k = j; k < i; ++k)
                    v -= s_M[tri6(i, k)] * s_W[tri6(k, j)];
                s_W[tri6(i, j)] = v / s_M[tri6(i, i)];
            }
        }
        __syncthreads();
        for (int e = tid; e < T; e += kRcThreads) {
            const int i = packed_row(e), j = e - tri6(i, 0);
            double v = 0.0;
            for (int k = i; k < P; ++k)
                v += s_W[tri6(k, i)] * s_W[tri6(k, j)];
            s_M[e] = s_act[i] && s_act[j] ? v * s_sc[i] * s_sc[j] : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int e = 0; e < T; ++e)
                sum += fabs(s_M[e]);
            if (!finite_bits(sum))
                s_ok = 0;
            ctl->lm.cov_ok = s_ok;
        }
        __syncthreads();
        const bool ok = s_ok != 0;
        for (int e = tid; e < P * P; e += kRcThreads) {
            const int i = e / P, j = e - P * i;
            a.ext_cov[e] = ok ? (i >= j ? s_M[tri6(i, j)] : s_M[tri6(j, i)]) : 0.0;
        }
        return;
    }
    // (L L') z = -D g_e, d ext = D z
    if (tid == 0) {
        bool ok = s_ok != 0;
        for (int i = 0; i < P; ++i) {
            double v = s_act[i] ? -s_tot[arrow_rec_grad(P) + i] * s_sc[i] : 0.0;
            for (int k = 0; k < i; ++k)
                v -= s_M[tri6(i, k)] * s_z[k];
            s_z[i] = v / s_M[tri6(i, i)];
        }
        for (int i = P - 1; i >= 0; --i) {
            double v = s_z[i];
            for (int k = i + 1; k < P; ++k)
                v -= s_M[tri6(k, i)] * s_z[k];
            s_z[i] = v / s_M[tri6(i, i)];
        }
        for (int i = 0; i < P; ++i) {
            const double d = s_act[i] ? s_z[i] * s_sc[i] : 0.0;
            ok = ok && finite_bits(d);
            ctl->dext[i] = d;
        }
        for (int c = 0; c < n_cams; ++c) {
            double cand[7];
            pose_plus(ctl->ext + 7 * c, ctl->dext + 6 * c, cand);
#pragma unroll
            for (int k = 0; k < 7; ++k)   // an inactive extrinsic keeps its bits
                ctl->ext_cand[7 * c + k] = s_act[6 * c] ? cand[k] : ctl->ext[7 * c + k];
        }
        ctl->lm.solve_ok = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(kRcThreads) void k_rigcal_try(const RigCalArgs a)
{
    __shared__ double s_model[kRigModel * VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_end[VMM_BA_RIG_MAX_CAMS];
    __shared__ double s_red[kImageWaves];
    const RigCalCtl* const ctl = a.ctl;
    if (ctl->lm.done || !ctl->lm.solve_ok)
        return;
    const LocalizeArgs& la = a.rig.loc;
    const int p = blockIdx.x, n_cams = a.rig.n_rig_cams, P = 6 * n_cams;
    if (!a.w.part[p]) {
        if (threadIdx.x == 0)
            a.w.trial[2 * p] = a.w.trial[2 * p + 1] = 0.0;
        return;
    }
    double dp[6], cand[7];
    arrow_pose_step(a.w.elim + arrow_elim_doubles(P) * (int64_t)p, P, ctl->dext, dp);
    pose_plus(la.cam_qt + 7 * (int64_t)p, dp, cand);
    const RigView f = open_frame(a.rig, ctl->ext_cand, p, s_model, s_end);
    __syncthreads();
    double A[21], g[6], raw2;   // not filled by the cost-only sum
    const double cost = frame_sums<false>(f, cand, la.obs_inlier + la.img_start[(int64_t)p * n_cams], a.w.robustify != 0,
                                          a.w.huber_a, s_red, A, g, raw2);
    if (threadIdx.x == 0)
        arrow_store_trial(a.w, p, cand, cost, dp);
}

// arrow_control with the extrinsics' step measured like a pose's: its largest tangent component
__global__ __launch_bounds__(kRcThreads) void k_rigcal_control(const RigCalArgs a)
{
    __shared__ double s_sum[kImageWaves], s_max[kImageWaves];
    RigCalCtl* const ctl = a.ctl;
    const int n_cams = a.rig.n_rig_cams;
    arrow_control(a.w, ctl->lm, a.rig.loc.n_imgs, a.rig.loc.cam_qt, s_sum, s_max,
                  [&](double sm) {
                      for (int j = 0; j < 6 * n_cams; ++j) {
                          const double s = fabs(ctl->dext[j]);
                          sm = s > sm ? s : sm;
                      }
                      return sm;
                  },
                  [&] {
                      for (int j = 0; j < 7 * n_cams; ++j)
                          ctl->ext[j] = ctl->ext_cand[j];
                  });
}

// workgroup (one wave) = frame, after k_rigcal_frame and k_rigcal_solve in cov_mode: the joint marginal of the rig pose
// and the frame's statistics at the result
__global__ __launch_bounds__(64) void k_rigcal_cov_pose(const RigCalArgs a)
{
    __shared__ double s_T[6][kRigDof];   // Y S^-1
    __shared__ double s_Mx[21];
    const LocalizeArgs& la = a.rig.loc;
    const int tid = threadIdx.x, p = blockIdx.x, P = 6 * a.rig.n_rig_cams;
    double* const out = la.cam_cov + 36 * (int64_t)p;
    if (!a.w.part[p]) {
        if (tid < 36)
            out[tid] = 0.0;
        return;
    }
    const double* const el = a.w.elim + arrow_elim_doubles(P) * (int64_t)p;
    if (tid == 0)
        arrow_result_update(la.res, p, a.w.n_in[p], a.w.rec + arrow_rec_doubles(P) * (int64_t)p + arrow_rec_stat(P));
    if (!a.ctl->lm.cov_ok) {
        if (tid < 36)
            out[tid] = 0.0;
        return;
    }
    for (int e = tid; e < 6 * P; e += 64) {
        const int i = e / P, c = e - P * i;
        double v = 0.0;
        for (int d = 0; d < P; ++d)
            v += el[arrow_elim_Y(P, i) + d] * a.ext_cov[P * d + c];
        s_T[i][c] = v;
    }
    __syncthreads();
    if (tid < 21) {   // M = I + Y S^-1 Y' (6 x 6, packed lower)
        const int i = packed_row(tid), j = tid - tri6(i, 0);
        double v = i == j ? 1.0 : 0.0;
        for (int c = 0; c < P; ++c)
            v += s_T[i][c] * el[arrow_elim_Y(P, j) + c];
        s_Mx[tid] = v;
    }
    __syncthreads();
    if (tid != 0)
        return;
    double M[21];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        M[k] = s_Mx[k];
    arrow_marginal_store(el, M, out);
}

} // namespace

void launch_rig_localize(hipStream_t st, const RigArgs& a)
{
    if (a.loc.n_imgs <= 0)
        return;
    hipLaunchKernelGGL(k_rig_localize, dim3((unsigned)a.loc.n_imgs), dim3(kImageThreads), 0, st, a);
}

void launch_rigcal_begin(hipStream_t st, const RigCalArgs& a)
{
    hipLaunchKernelGGL(k_rigcal_begin, dim3((unsigned)((a.rig.loc.n_imgs + 63) / 64)), dim3(64), 0, st, a);
}

void launch_rigcal_classify(hipStream_t st, const RigCalArgs& a)
{
    hipLaunchKernelGGL(k_rigcal_classify, dim3((unsigned)a.rig.loc.n_imgs), dim3(kRcThreads), 0, st, a);
}

void launch_rigcal_trial(hipStream_t st, const RigCalArgs& a)
{
    hipLaunchKernelGGL(k_rigcal_frame, dim3((unsigned)a.rig.loc.n_imgs), dim3(kRcThreads), 0, st, a, 0);
    hipLaunchKernelGGL(k_rigcal_solve, dim3(1), dim3(kRcThreads), 0, st, a, 0);
    hipLaunchKernelGGL(k_rigcal_try, dim3((unsigned)a.rig.loc.n_imgs), dim3(kRcThreads), 0, st, a);
    hipLaunchKernelGGL(k_rigcal_control, dim3(1), dim3(kRcThreads), 0, st, a);
}

void launch_rigcal_covariance(hipStream_t st, const RigCalArgs& a)
{
    hipLaunchKernelGGL(k_rigcal_frame, dim3((unsigned)a.rig.loc.n_imgs), dim3(kRcThreads), 0, st, a, 1);
    hipLaunchKernelGGL(k_rigcal_solve, dim3(1), dim3(kRcThreads), 0, st, a, 1);
    hipLaunchKernelGGL(k_rigcal_cov_pose, dim3((unsigned)a.rig.loc.n_imgs), dim3(64), 0, st, a);
}

int preload_rig_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rig_localize)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_begin)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_classify)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_frame)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_solve)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_try)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_control)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_rigcal_cov_pose)) != hipSuccess;
    return bad;
}

} // namespace vmm
