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
// The solver (lm_refine, solve6, inverse6, better / wave_winner, chain_camera / chain_tag) is pose_lm.hpp's and the
// reductions and the stores of a result are image_sums.hpp's, as in k_localize.  The K camera models and extrinsics
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

#include "engine.hpp"
#include "image_sums.hpp"

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
            have_cov = inverse6(A, C);
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
// The arrowhead of kernels_calibrate.hip with the 6 K extrinsic parameters in the place of the camera model: every frame
// eliminates its own 6 x 6 block and what is left is P x P, P = 6 K.  One Levenberg-Marquardt trial:
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
//   k_rigcal_control  one workgroup: lm_refine's accept / stop rules on the whole problem
// At the result k_rigcal_frame and k_rigcal_solve run once more with lam = 0 (cov_mode): S^-1 = ext_cov, and
// k_rigcal_cov_pose forms rig_cov_f = L^-T (I + Y S^-1 Y') L^-1.  Every sum has a fixed order; the sum over the frames
// makes the bits depend on the order of the batch.
//                         .vgpr_count  .vgpr_spill_count  .private_segment_fixed_size
//   k_rigcal_frame        364          0                  0      (92 running sums = 184 registers, one corner's 2 x 12 rows)
//   k_rigcal_solve        56           0                  0      (the 48 x 48 system lives in 30 KiB of LDS)
//   k_rigcal_try          152          0                  0
//   k_rigcal_classify 100, k_rigcal_cov_pose 86, k_rigcal_control 18, k_rigcal_begin 6: no spill, no private segment

constexpr int kRcSums = 92;     // 78 (12 x 12 packed lower: rig 0..5, extrinsic 6..11) + 12 gradient + cost + sum |r|^2
constexpr int kRcChunks = 3;    // wave_sum32 calls that cover them
constexpr int kRcThreads = kImageThreads;

// row of packed-lower entry e (tri6 indexing)
__device__ __forceinline__ int packed_row(const int e)
{
    int r = 0;
    while (tri6(r + 1, 0) <= e)
        ++r;
    return r;
}

__global__ __launch_bounds__(64) void k_rigcal_begin(const RigCalArgs a)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.rig.loc.n_imgs)
        return;
    const vmm_ba_localize_result r = a.rig.loc.res[p];
    a.n_in[p] = r.n_inlier_obs;
    a.part[p] = r.status == VMM_BA_LOC_OK && r.n_inlier_obs >= a.min_inliers;
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
    const int n = classify_frame(f, la.cam_qt + 7 * (int64_t)p, a.inlier2,
                                 la.obs_inlier + la.img_start[(int64_t)p * a.rig.n_rig_cams], s_cnt);
    if (threadIdx.x == 0) {
        a.n_in[p] = n;
        a.part[p] = n >= a.min_inliers;
    }
}

// The sums of camera c's inlier observations of a frame into s_tot: the packed lower triangle of the 12 x 12 normal
// matrix over (rig pose, extrinsic c) (0..77), the gradient (78..89), the cost (90) and sum |r|^2 (91), the Huber
// corrector applied.  free_c false: the extrinsic is held and its columns are zero.
__device__ __forceinline__ void camera_normal_sums(const RigView& f, const uint8_t* flags, const int c, const Rigid& rig,
                                                   const bool free_c, const bool robust, const double huber_a, double* s_red,
                                                   double* s_tot)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[kRcChunks][32];
#pragma unroll
    for (int h = 0; h < kRcChunks; ++h)
#pragma unroll
        for (int k = 0; k < 32; ++k)
            acc[h][k] = 0.0;
#define VMM_ACC(i) acc[(i) >> 5][(i) & 31]
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
            VMM_ACC(90) += rho0;
            VMM_ACC(91) += s;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                VMM_ACC(78 + i) += J[0][i] * ru + J[1][i] * rv;
#pragma unroll
                for (int e = 0; e <= i; ++e)
                    VMM_ACC(tri6(i, e)) += J[0][i] * J[0][e] + J[1][i] * J[1][e];
            }
        }
    }
#undef VMM_ACC
#pragma unroll
    for (int h = 0; h < kRcChunks; ++h) {
        const double tot = wave_sum32(acc[h], lane);
        s_red[(wave * kRcChunks + h) * 32 + wave_sum32_index(lane)] = tot;   // lanes 2 m and 2 m + 1 store the same value
    }
    __syncthreads();
    if (tid < kRcSums) {
        double t = s_red[tid];
#pragma unroll
        for (int w = 1; w < kImageWaves; ++w)
            t += s_red[w * 32 * kRcChunks + tid];
        s_tot[tid] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kRcThreads) void k_rigcal_frame(const RigCalArgs a, const int cov_mode)
{
    __shared__ double s_model[kRigModel * VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_end[VMM_BA_RIG_MAX_CAMS];
    __shared__ double s_red[kImageWaves * 32 * kRcChunks];
    __shared__ double s_tot[32 * kRcChunks];
    __shared__ double s_A[21], s_g[6], s_stat[2], s_L[21];
    __shared__ double s_B[6][kRigDof], s_C[VMM_BA_RIG_MAX_CAMS][21], s_gk[kRigDof];
    __shared__ double s_Y[6][kRigDof + 1];   // column P: y
    __shared__ int s_bad;
    const RigCalCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->done)
        return;
    const LocalizeArgs& la = a.rig.loc;
    const int tid = threadIdx.x, p = blockIdx.x, n_cams = a.rig.n_rig_cams;
    const int P = 6 * n_cams, T = P * (P + 1) / 2, n_rec = rig_rec_doubles(P), n_el = rig_elim_doubles(P);
    double* const rec = a.rec + n_rec * (int64_t)p;
    double* const el = a.elim + n_el * (int64_t)p;
    if (!a.part[p]) {
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
    const int mask = ctl->refine_mask;
    Rigid rig;
    load_rigid<true>(la.cam_qt + 7 * (int64_t)p, rig);
    for (int c = 0; c < n_cams; ++c) {
        camera_normal_sums(f, flags, c, rig, (mask >> c) & 1, a.robustify != 0, a.huber_a, s_red, s_tot);
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
    // L = chol(A + lam diag(max(A_ii, 1e-12))), as solve6 damps
    if (tid == 0) {
        const double lam = cov_mode ? 0.0 : ctl->lam;
        double L[21];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double ajj = s_A[tri6(j, j)];
            double d = ajj + lam * (ajj > 1e-12 ? ajj : 1e-12);
#pragma unroll
            for (int k = 0; k < j; ++k)
                d -= L[tri6(j, k)] * L[tri6(j, k)];
            ok = ok && d > 0.0 && finite_bits(d);
            const double sq = sqrt(d);
            L[tri6(j, j)] = sq;
            const double is = 1.0 / sq;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double v = s_A[tri6(i, j)];
#pragma unroll
                for (int k = 0; k < j; ++k)
                    v -= L[tri6(i, k)] * L[tri6(j, k)];
                L[tri6(i, j)] = v * is;
            }
        }
#pragma unroll
        for (int k = 0; k < 21; ++k)
            s_L[k] = L[k];
        s_bad = ok ? 0 : 1;
    }
    __syncthreads();
    // column c of Y = L^-1 B (c < P) and y = L^-1 g (c == P)
    if (tid <= P) {
        double col[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = tid < P ? s_B[i][tid] : s_g[i];
#pragma unroll
            for (int k = 0; k < i; ++k)
                v -= s_L[tri6(i, k)] * col[k];
            col[i] = v / s_L[tri6(i, i)];
            s_Y[i][tid] = col[i];
        }
    }
    __syncthreads();
    for (int e = tid; e < n_rec; e += kRcThreads) {
        double v;
        if (e < T) {   // C - Y'Y, packed lower; C is block-diagonal
            const int i = packed_row(e), j = e - tri6(i, 0);
            v = i / 6 == j / 6 ? s_C[i / 6][tri6(i % 6, j % 6)] : 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                v -= s_Y[k][i] * s_Y[k][j];
        } else if (e < T + P) {   // g_e - Y'y
            const int c = e - T;
            v = s_gk[c];
#pragma unroll
            for (int k = 0; k < 6; ++k)
                v -= s_Y[k][c] * s_Y[k][P];
        } else if (e < T + 2 * P) {
            const int c = e - T - P;
            v = s_C[c / 6][tri6(c % 6, c % 6)];
        } else {
            const int k = e - T - 2 * P;
            v = k == 0 ? s_stat[0] : k == 1 ? s_stat[1] : k == 2 ? (s_bad ? 1.0 : 0.0) : k == 3 ? (double)a.n_in[p] : 1.0;
        }
        rec[e] = v;
    }
    for (int e = tid; e < n_el; e += kRcThreads) {
        double v;
        if (e < 21)
            v = s_L[e];
        else if (e < 21 + 6 * P)
            v = s_Y[(e - 21) / P][(e - 21) % P];
        else
            v = s_Y[e - 21 - 6 * P][P];
        el[e] = v;
    }
}

// As kernels_calibrate.hip's: a pivot of the undamped S, scaled by diag(sum C), within a factor 100 of its rounding
// noise is taken for the zero of a singular matrix.
constexpr double kRcMinPivot = 1e-13;

__global__ __launch_bounds__(kRcThreads) void k_rigcal_solve(const RigCalArgs a, const int cov_mode)
{
    constexpr int kMaxTri = kRigDof * (kRigDof + 1) / 2;
    __shared__ double s_tot[kMaxTri + 2 * kRigDof + 5];
    __shared__ double s_M[kMaxTri], s_W[kMaxTri];
    __shared__ double s_sc[kRigDof], s_wt[kRigDof], s_z[kRigDof];
    __shared__ int s_act[kRigDof];
    __shared__ int s_go, s_ok;
    RigCalCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->done)
        return;
    const int tid = threadIdx.x, n_cams = a.rig.n_rig_cams, n_frames = a.rig.loc.n_imgs;
    const int P = 6 * n_cams, T = P * (P + 1) / 2, n_rec = rig_rec_doubles(P);
    for (int e = tid; e < n_rec; e += kRcThreads) {
        double t[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int i = 0; i < n_frames; i += 4)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (i + g < n_frames)
                    t[g] += a.rec[n_rec * (int64_t)(i + g) + e];
        s_tot[e] = ((t[0] + t[1]) + t[2]) + t[3];
    }
    __syncthreads();
    const double* const st = s_tot + T + 2 * P;   // cost | raw2 | bad frames | inlier observations | frames
    const double lam = cov_mode ? 0.0 : ctl->lam;
    if (tid == 0) {
        const double cost = st[0], raw2 = st[1];
        const int n_used = (int)st[4], n_obs_used = (int)st[3];
        int go = 1;
        ctl->cost = cost;
        ctl->raw2 = raw2;
        ctl->n_used = n_used;
        ctl->n_obs_used = n_obs_used;
        if (ctl->first) {
            ctl->first = 0;
            ctl->initial_cost = cost;
            ctl->initial_raw2 = raw2;
            ctl->initial_n_obs = n_obs_used;
        }
        if (!cov_mode) {
            if (n_used == 0 || !finite_bits(cost) || lam > kLamMax) {
                ctl->done = 1;
                ctl->stop = 1;
                go = 0;
            } else if (ctl->trials >= ctl->max_trials) {
                ctl->done = 1;
                ctl->stop = 2;
                go = 0;
            } else {
                ctl->trials += 1;
            }
        }
        s_go = go;
        s_ok = st[2] == 0.0 ? 1 : 0;
    }
    __syncthreads();
    if (!s_go)
        return;
    // damp, give the extrinsics that are held or unobserved unit rows, scale to a unit diagonal
    const int mask = ctl->refine_mask;
    if (tid < P) {
        const double cjj = s_tot[T + P + tid];
        const bool act = ((mask >> (tid / 6)) & 1) && s_tot[T + P + 6 * (tid / 6)] > 0.0;
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
    const double min_pivot = cov_mode ? kRcMinPivot : 0.0;
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
            ctl->cov_ok = s_ok;
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
            double v = s_act[i] ? -s_tot[T + i] * s_sc[i] : 0.0;
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
        ctl->solve_ok = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(kRcThreads) void k_rigcal_try(const RigCalArgs a)
{
    __shared__ double s_model[kRigModel * VMM_BA_RIG_MAX_CAMS];
    __shared__ int s_end[VMM_BA_RIG_MAX_CAMS];
    __shared__ double s_red[kImageWaves];
    const RigCalCtl* const ctl = a.ctl;
    if (ctl->done || !ctl->solve_ok)
        return;
    const LocalizeArgs& la = a.rig.loc;
    const int p = blockIdx.x, n_cams = a.rig.n_rig_cams, P = 6 * n_cams;
    if (!a.part[p]) {
        if (threadIdx.x == 0)
            a.trial[2 * p] = a.trial[2 * p + 1] = 0.0;
        return;
    }
    const double* const el = a.elim + rig_elim_doubles(P) * (int64_t)p;
    // d rig = -L^-T (y + Y d ext); every thread computes it
    double w[6], dp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = el[21 + 6 * P + k];
        for (int c = 0; c < P; ++c)
            v += el[21 + P * k + c] * ctl->dext[c];
        w[k] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = -w[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k)
            v -= el[tri6(k, i)] * dp[k];
        dp[i] = v / el[tri6(i, i)];
    }
    double cand[7];
    pose_plus(la.cam_qt + 7 * (int64_t)p, dp, cand);
    const RigView f = open_frame(a.rig, ctl->ext_cand, p, s_model, s_end);
    __syncthreads();
    double A[21], g[6], raw2;   // not filled by the cost-only sum
    const double cost = frame_sums<false>(f, cand, la.obs_inlier + la.img_start[(int64_t)p * n_cams], a.robustify != 0, a.huber_a,
                                          s_red, A, g, raw2);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
            a.rig_cand[7 * (int64_t)p + k] = cand[k];
        a.trial[2 * p] = cost;
        a.trial[2 * p + 1] = max_abs6(dp);
    }
}

// lm_refine's decision (pose_lm.hpp) on the whole problem.  The step's size: the largest tangent component of any rig
// pose or extrinsic.
__global__ __launch_bounds__(kRcThreads) void k_rigcal_control(const RigCalArgs a)
{
    __shared__ double s_sum[kImageWaves], s_max[kImageWaves];
    RigCalCtl* const ctl = a.ctl;
    if (ctl->done)
        return;
    const int tid = threadIdx.x, n_frames = a.rig.loc.n_imgs, n_cams = a.rig.n_rig_cams;
    if (!ctl->solve_ok) {   // a trial spent on a system that was not positive definite
        if (tid == 0)
            ctl->lam *= 10.0;
        return;
    }
    double cc = 0.0, sm = 0.0;
    for (int i = tid; i < n_frames; i += kRcThreads) {
        cc += a.trial[2 * i];
        const double s = a.trial[2 * i + 1];
        sm = s > sm ? s : sm;
    }
    cc = wave_sum(cc);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double o = __shfl_xor(sm, s, 64);
        sm = o > sm ? o : sm;
    }
    if ((tid & 63) == 0) {
        s_sum[tid >> 6] = cc;
        s_max[tid >> 6] = sm;
    }
    __syncthreads();
    cc = s_sum[0];
    sm = s_max[0];
#pragma unroll
    for (int w = 1; w < kImageWaves; ++w) {
        cc += s_sum[w];
        sm = s_max[w] > sm ? s_max[w] : sm;
    }
    for (int j = 0; j < 6 * n_cams; ++j) {
        const double s = fabs(ctl->dext[j]);
        sm = s > sm ? s : sm;
    }
    const double cost = ctl->cost, lam = ctl->lam;
    __syncthreads();   // every thread has read the control block before thread 0 writes it
    if (sm < 1e-14) {
        if (tid == 0) {
            ctl->done = 1;
            ctl->stop = 1;
        }
        return;
    }
    if (finite_bits(cc) && cc < cost) {
        double* const rig_qt = a.rig.loc.cam_qt;
        for (int i = tid; i < n_frames; i += kRcThreads)
            if (a.part[i])
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    rig_qt[7 * (int64_t)i + k] = a.rig_cand[7 * (int64_t)i + k];
        if (tid == 0) {
            for (int j = 0; j < 7 * n_cams; ++j)
                ctl->ext[j] = ctl->ext_cand[j];
            ctl->lam = lam * 0.1 > kLamMin ? lam * 0.1 : kLamMin;
            ctl->accepted += 1;
        }
    } else if (tid == 0) {
        if (sm < 1e-10 || cost_at_floor(cost, cc)) {
            ctl->done = 1;
            ctl->stop = 1;
        } else {
            ctl->lam = lam * 10.0;
        }
    }
}

// workgroup (one wave) = frame, after k_rigcal_frame and k_rigcal_solve in cov_mode: the joint marginal of the rig pose
// and the frame's statistics at the result
__global__ __launch_bounds__(64) void k_rigcal_cov_pose(const RigCalArgs a)
{
    __shared__ double s_T[6][kRigDof];   // Y S^-1
    __shared__ double s_Mx[21];
    const LocalizeArgs& la = a.rig.loc;
    const int tid = threadIdx.x, p = blockIdx.x, P = 6 * a.rig.n_rig_cams, T = P * (P + 1) / 2;
    double* const out = la.cam_cov + 36 * (int64_t)p;
    if (!a.part[p]) {
        if (tid < 36)
            out[tid] = 0.0;
        return;
    }
    const double* const rec = a.rec + rig_rec_doubles(P) * (int64_t)p;
    const double* const el = a.elim + rig_elim_doubles(P) * (int64_t)p;
    if (tid == 0) {
        const int n_in = a.n_in[p];
        vmm_ba_localize_result r = la.res[p];
        r.n_inlier_obs = n_in;
        r.cost = 0.5 * rec[T + 2 * P];
        r.rms_px = sqrt(rec[T + 2 * P + 1] / (4.0 * n_in));
        la.res[p] = r;
    }
    if (!a.ctl->cov_ok) {
        if (tid < 36)
            out[tid] = 0.0;
        return;
    }
    for (int e = tid; e < 6 * P; e += 64) {
        const int i = e / P, c = e - P * i;
        double v = 0.0;
        for (int d = 0; d < P; ++d)
            v += el[21 + P * i + d] * a.ext_cov[P * d + c];
        s_T[i][c] = v;
    }
    __syncthreads();
    if (tid < 21) {   // M = I + Y S^-1 Y' (6 x 6, packed lower)
        const int i = packed_row(tid), j = tid - tri6(i, 0);
        double v = i == j ? 1.0 : 0.0;
        for (int c = 0; c < P; ++c)
            v += s_T[i][c] * el[21 + P * j + c];
        s_Mx[tid] = v;
    }
    __syncthreads();
    if (tid != 0)
        return;
    double M[21], W[21];   // W = L^-1, lower
#pragma unroll
    for (int k = 0; k < 21; ++k)
        M[k] = s_Mx[k];
    lower_inverse<6>(el, W);
    // cov = W' M W: Q = M W (full 6 x 6), cov[r][c] = sum_k W[k][r] Q[k][c]
    double Q[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
#pragma unroll
            for (int k = c; k < 6; ++k)
                v += (i >= k ? M[tri6(i, k)] : M[tri6(k, i)]) * W[tri6(k, c)];
            Q[i][c] = v;
        }
    double sum = 0.0, C[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double v = 0.0;
#pragma unroll
            for (int k = r; k < 6; ++k)
                v += W[tri6(k, r)] * Q[k][c];
            C[tri6(r, c)] = v;
            sum += fabs(v);
        }
    const bool ok = finite_bits(sum);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c)
            out[6 * r + c] = ok ? (r >= c ? C[tri6(r, c)] : C[tri6(c, r)]) : 0.0;
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
