// Calibration of a camera against a finished map (gfx950): the kernels of vmm_ba_calibrate.
//
// Unknowns: the nine numbers of the camera model (fx, fy, cx, cy, k1, k2, p1, p2, k3) shared by all images and one
// 6-degree-of-freedom pose per image; the map is fixed.  The normal equations are an arrowhead,
//     [ A_i  B_i ] [dp_i]     [ g_i ]
//     [ B_i' C   ] [dk  ] = - [ g_k ],   C = sum_i C_i, g_k = sum_i g_k,i
// so every image eliminates its own 6 x 6 block and what is left is 9 x 9.  One Levenberg-Marquardt trial:
//   k_calib_image    workgroup = image: the 15 x 15 packed normal matrix of the image (A, B, C_i), its gradient, cost and
//                    sum |r|^2 over the inlier observations with the Huber corrector applied -- thread-private sums in
//                    list order, one butterfly per wave (wave_sum32, five times), the waves combined in order through
//                    LDS, no floating-point atomic -- then L = chol(A + lam diag), Y = L^-1 B, y = L^-1 g, and the
//                    image's record: C_i - Y'Y, g_k,i - Y'y, diag(C_i), cost (kCalRec), L, Y, y (kCalElim)
//   k_calib_solve    one workgroup: the records summed in a fixed order (four interleaved chains, combined in order),
//                    damped with lam diag(sum C), Jacobi-scaled, unit rows for the parameters outside the mask, 9 x 9
//                    Cholesky, dk; holds the control block (cost, lam, counters, done)
//   k_calib_try      workgroup = image: dp_i = -L^-T (y + Y dk), candidate pose by pose_plus, candidate model k + dk,
//                    cost-only pass
//   k_calib_control  one workgroup: the candidate costs summed in a fixed order, lm_refine's accept / stop rules
//                    (pose_lm.hpp), the accepted candidates copied over the state
// Every one of them returns at once when CalibCtl::done is set.  At the result k_calib_image and k_calib_solve run once
// more with lam = 0 (cov_mode): S^-1 = intr_cov, and k_calib_cov_pose (thread = image) forms
// cam_cov_i = L^-T (I + Y S^-1 Y') L^-1 = A_i^-1 + A_i^-1 B_i S^-1 B_i' A_i^-1.
// Nothing but the selection of the image depends on blockIdx and every sum has a fixed order: the same batch gives the
// same bits from run to run.  The sum over the images makes the bits depend on the order of the batch.
// Every kernel reads pixels and world corners from global memory (ImageView<false>; no LDS staging: one variant).
// Shared with kernels_rig.hip through arrowhead.hpp, once each: the wide sums and their reduction (Wide<15>), the damped
// 6 x 6 factorisation and the forward solve of a column, the layouts of a record and an elimination, the solve kernel's
// bookkeeping on the control block, dp from an elimination, the accept / stop rules of the control kernel, the result
// update and the joint marginal, the begin rule and kMinPivot.  Shared with kernels_localize.hip through image_sums.hpp:
// the image view, the rotation of a world corner, the classification (k_calib_classify is classify_image under the
// current model) and the cost-only sum (k_calib_try's candidate cost is image_sums<false, false>); from pose_lm.hpp:
// project_camera_point_intrinsics; from small_solve.hpp: tri6, cholesky<9>, forward_substitute<9>, lower_inverse /
// lower_gram.  The camera model is loaded by
// engine.hpp's make_intrinsics.  Calibration's own: one corner's 2 x 15 rows (image_normal_sums), the 9 x 9 system in one
// thread's registers (chol9, the solve and the inverse behind it) and the step size of the model in k_calib_control.
//
// Registers (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, the .s file's .vgpr_count / .vgpr_spill_count /
// .private_segment_fixed_size): the table at k_calib_image below.
#include "arrowhead.hpp"

namespace vmm {

namespace {

constexpr int kCalThreads = 256;
constexpr int kCalWaves = kCalThreads / 64;
constexpr int kCalP = 9;          // the shared unknowns: the camera model
using CalSums = Wide<6 + kCalP>;  // 137 sums: 120 (15 x 15 packed lower: pose 0..5, model 6..14) + 15 gradient + cost + sum |r|^2
constexpr int kSolveThreads = 512;

static_assert(kCalThreads == kImageThreads, "classify_image, image_sums and the arrowhead stride by kImageThreads");
static_assert(CalSums::kSums == 137 && CalSums::kChunks == 5 && kCalRec == 68 && arrow_elim_doubles(kCalP) <= kCalElim, "the layouts of DESIGN.md");

// image p's observations, read from global memory
__device__ __forceinline__ ImageView<false> image_view(const CalibArgs& a, const int p)
{
    const int64_t b = a.img_start[p];
    ImageView<false> v;
    v.lds = nullptr;
    v.m = (int)(a.img_start[p + 1] - b);
    v.px = a.obs_px + 8 * b;
    v.tag = a.obs_tag + b;
    v.corners = a.corners;
    return v;
}

// thread = image: who takes part in the first refinement, from the localisation's results and flags
__global__ __launch_bounds__(64) void k_calib_begin(const CalibArgs a)
{
    arrow_begin(a.w, a.res, a.n_imgs);
}

// workgroup = image: k_localize's classification (classify_image, image_sums.hpp) under the current camera model, for
// the localised images
__global__ __launch_bounds__(kCalThreads) void k_calib_classify(const CalibArgs a)
{
    __shared__ int s_cnt[kCalWaves];
    const int p = blockIdx.x;
    if (a.res[p].status != VMM_BA_LOC_OK)
        return;
    const ImageView<false> v = image_view(a, p);
    const int n = classify_image<false>(make_intrinsics(a.ctl->k), v, a.cam_qt + 7 * (int64_t)p, a.w.inlier2,
                                        a.flags + a.img_start[p], s_cnt);
    if (threadIdx.x == 0) {
        a.w.n_in[p] = n;
        a.w.part[p] = n >= a.w.min_inliers;
    }
}

// An image's sums into s_tot: the packed lower triangle of its 15 x 15 normal matrix (pose 0..5, model 6..14: A, B and
// C_i; entries 0..119), the gradient (120..134), the cost (135) and sum |r|^2 (136), the Huber corrector applied.
__device__ __forceinline__ void image_normal_sums(const ImageView<false>& v, const uint8_t* flags, const Intrinsics& K,
                                                  const Rigid& cam, const int mask, const bool robust, const double huber_a,
                                                  double* s_red, double* s_tot)
{
    CalSums sums;
    sums.zero();
    for (int d = threadIdx.x; d < v.m; d += kCalThreads) {
        if (flags[d] == 0)
            continue;
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {   // not unrolled: four corners in flight at once cost registers the sums need
            double b0, b1, b2, ru, rv, jp[2][6], jk[2][9];
            rotate_world(cam, v.world(d, 3 * c), v.world(d, 3 * c + 1), v.world(d, 3 * c + 2), b0, b1, b2);
            project_camera_point_intrinsics(K, b0, b1, b2, cam.t, v.pixel(d, 2 * c), v.pixel(d, 2 * c + 1), ru, rv, jp, jk);
            const double s = ru * ru + rv * rv;
            double rho0, wgt;
            huber(robust, huber_a, s, rho0, wgt);
            double J[2][15];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    J[r][k] = jp[r][k] * wgt;
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    J[r][6 + k] = ((mask >> k) & 1) ? jk[r][k] * wgt : 0.0;   // a fixed parameter has zero columns
            }
            ru *= wgt;
            rv *= wgt;
            sums.add(J, ru, rv, rho0, s);
        }
    }
    sums.reduce(s_red, s_tot);
}

// The image's sums and its elimination.
//                         .vgpr_count  .vgpr_spill_count  .private_segment_fixed_size
//   k_calib_image         390          0                  0
//   k_calib_try           120          0                  0
// One 256-thread workgroup per CU = one wave per SIMD, 512 registers per lane: the 137 running sums (274 registers) stay
// in registers next to one corner's 2 x 15 Jacobian, so one pass over the image is enough.  With the corner loop unrolled
// the compiler kept four corners in flight and spilled 162 registers to 268 bytes of scratch, and split into two passes (A, g
// and the cost, then B, C and g_k) it still took 510 registers and spilled 4; with the loop rolled neither happens.
__global__ __launch_bounds__(kCalThreads) void k_calib_image(const CalibArgs a, const int cov_mode)
{
    constexpr int P = kCalP, kTri = CalSums::kTri;
    __shared__ double s_red[kCalWaves * 32 * CalSums::kChunks];
    __shared__ double s_tot[CalSums::kSums];
    __shared__ double s_L[21];
    __shared__ double s_Y[6][P + 1];   // column P: y
    __shared__ int s_bad;
    const CalibCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->lm.done)
        return;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    double* const rec = a.w.rec + kCalRec * (int64_t)p;
    double* const el = a.w.elim + kCalElim * (int64_t)p;
    if (!a.w.part[p]) {
        if (tid < kCalRec)
            rec[tid] = 0.0;
        return;
    }
    const Intrinsics K = make_intrinsics(ctl->k);
    const int mask = ctl->lm.refine_mask;
    const bool robust = a.w.robustify != 0;
    Rigid cam;
    load_rigid<true>(a.cam_qt + 7 * (int64_t)p, cam);
    image_normal_sums(image_view(a, p), a.flags + a.img_start[p], K, cam, mask, robust, a.w.huber_a, s_red, s_tot);
    if (tid == 0)   // A: the first 21 sums
        s_bad = damped_chol6(s_tot, cov_mode ? 0.0 : ctl->lm.lam, s_L) ? 0 : 1;
    __syncthreads();
    // column c of Y = L^-1 B (c < P: B[.][c] = row 6 + c of the packed matrix) and y = L^-1 g (c == P)
    if (tid <= P)
        forward_column6(s_L, [&](const int i) { return tid < P ? s_tot[tri6(6 + tid, i)] : s_tot[kTri + i]; }, &s_Y[0][tid], P + 1);
    __syncthreads();
    if (tid < kCalRec) {
        rec[tid] = arrow_record_entry(tid, P, [&](const int i, const int j) { return s_tot[tri6(6 + i, 6 + j)]; },
                                      [&](const int c) { return s_tot[kTri + 6 + c]; }, &s_Y[0][0], P + 1, s_tot[kTri + 15],
                                      s_tot[kTri + 16], s_bad != 0, a.w.n_in[p]);
    } else if (tid >= 128 && tid < 128 + arrow_elim_doubles(P)) {
        el[tid - 128] = arrow_elim_entry(tid - 128, P, s_L, &s_Y[0][0], P + 1);
    }
}

// 9 x 9 packed lower M (unit diagonal after the caller's scaling) -> its Cholesky factor in place; false: a pivot times
// its weight is not above min_pivot, or not finite
__device__ __forceinline__ bool chol9(double (&M)[45], const double (&weight)[9], const double min_pivot)
{
    return cholesky<9>(M, M, Packed{}, PivotWeighted{ weight, min_pivot });
}

__global__ __launch_bounds__(kSolveThreads) void k_calib_solve(const CalibArgs a, const int cov_mode)
{
    __shared__ double s_part[4][kCalRec];
    __shared__ double s_tot[kCalRec];
    CalibCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->lm.done)
        return;
    const int tid = threadIdx.x, e = tid & 127, grp = tid >> 7;
    if (e < kCalRec) {
        double t = 0.0;
        for (int i = grp; i < a.n_imgs; i += 4)
            t += a.w.rec[kCalRec * (int64_t)i + e];
        s_part[grp][e] = t;
    }
    __syncthreads();
    if (tid < kCalRec)
        s_tot[tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
    __syncthreads();
    if (tid != 0)
        return;
    constexpr int P = kCalP;
    const double* const st = s_tot + arrow_rec_stat(P);
    const double lam = cov_mode ? 0.0 : ctl->lm.lam;
    if (!arrow_solve_begin(ctl->lm, st, cov_mode, lam))
        return;
    const int mask = ctl->lm.refine_mask;
    // damp, give the fixed parameters unit rows, scale to a unit diagonal
    double M[45], sc[9], weight[9];
    bool ok = st[2] == 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const bool free_j = (mask >> j) & 1;
        const double d = free_j ? s_tot[tri6(j, j)] + lam * s_tot[arrow_rec_diag(P) + j] : 1.0;
        ok = ok && d > 0.0 && finite_bits(d);
        sc[j] = free_j ? 1.0 / sqrt(d) : 1.0;
        weight[j] = cov_mode && free_j ? d / s_tot[arrow_rec_diag(P) + j] : 1.0;   // S_jj / C_jj
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const bool both = ((mask >> i) & 1) && ((mask >> j) & 1);
            M[tri6(i, j)] = i == j ? 1.0 : (both ? s_tot[tri6(i, j)] * sc[i] * sc[j] : 0.0);
        }
    ok = chol9(M, weight, cov_mode ? kMinPivot : 0.0) && ok;
    if (cov_mode) {
        // S^-1 = D (L L')^-1 D with the rows and columns of the fixed parameters zero
        double W[45], G[45];   // L^-1 (lower), its Gram matrix
        lower_inverse<9>(M, W);
        lower_gram<9>(W, G);
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const bool both = ((mask >> i) & 1) && ((mask >> j) & 1);
                const double v = both ? G[tri6(i, j)] * sc[i] * sc[j] : 0.0;
                sum += fabs(v);
                M[tri6(i, j)] = v;
            }
        ok = ok && finite_bits(sum);
        ctl->lm.cov_ok = ok ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j)
                a.intr_cov[9 * i + j] = ok ? (i >= j ? M[tri6(i, j)] : M[tri6(j, i)]) : 0.0;
        return;
    }
    // (L L') z = -D g_k, dk = D z
    double z[9];
    forward_substitute<9>(M, Packed{}, [&](const int i) { return ((mask >> i) & 1) ? -s_tot[arrow_rec_grad(P) + i] * sc[i] : 0.0; },
                          [&](const int i, const double v) { z[i] = v; });
#pragma unroll
    for (int i = 8; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int k = i + 1; k < 9; ++k)
            v -= M[tri6(k, i)] * z[k];
        z[i] = v / M[tri6(i, i)];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const bool free_i = (mask >> i) & 1;
        const double dk = free_i ? z[i] * sc[i] : 0.0;
        ok = ok && finite_bits(dk);
        ctl->dk[i] = dk;
        ctl->k_cand[i] = free_i ? ctl->k[i] + dk : ctl->k[i];   // a fixed parameter keeps its bits
    }
    ctl->lm.solve_ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(kCalThreads) void k_calib_try(const CalibArgs a)
{
    __shared__ double s_red[kCalWaves];
    const CalibCtl* const ctl = a.ctl;
    if (ctl->lm.done || !ctl->lm.solve_ok)
        return;
    const int p = blockIdx.x;
    if (!a.w.part[p]) {
        if (threadIdx.x == 0)
            a.w.trial[2 * p] = a.w.trial[2 * p + 1] = 0.0;
        return;
    }
    double dp[6], cand[7];
    arrow_pose_step(a.w.elim + kCalElim * (int64_t)p, kCalP, ctl->dk, dp);
    pose_plus(a.cam_qt + 7 * (int64_t)p, dp, cand);
    double A[21], g[6], raw2;   // not filled by the cost-only sum
    const double cost = image_sums<false, false>(make_intrinsics(ctl->k_cand), image_view(a, p), cand, a.flags + a.img_start[p],
                                                 a.w.robustify != 0, a.w.huber_a, s_red, A, g, raw2);
    if (threadIdx.x == 0)
        arrow_store_trial(a.w, p, cand, cost, dp);
}

// arrow_control with the model's step measured relative to max(|k_j|, 1)
__global__ __launch_bounds__(kCalThreads) void k_calib_control(const CalibArgs a)
{
    __shared__ double s_sum[kCalWaves], s_max[kCalWaves];
    CalibCtl* const ctl = a.ctl;
    arrow_control(a.w, ctl->lm, a.n_imgs, a.cam_qt, s_sum, s_max,
                  [&](double sm) {
#pragma unroll
                      for (int j = 0; j < 9; ++j) {
                          const double kj = fabs(ctl->k[j]);
                          const double s = fabs(ctl->dk[j]) / (kj > 1.0 ? kj : 1.0);
                          sm = s > sm ? s : sm;
                      }
                      return sm;
                  },
                  [&] {
#pragma unroll
                      for (int j = 0; j < 9; ++j)
                          ctl->k[j] = ctl->k_cand[j];
                  });
}

// thread = image, after k_calib_image and k_calib_solve in cov_mode: the joint marginal of the pose and the image's
// statistics at the result
__global__ __launch_bounds__(64) void k_calib_cov_pose(const CalibArgs a)
{
    constexpr int P = kCalP;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_imgs)
        return;
    double* const out = a.cam_cov + 36 * (int64_t)p;
    if (!a.w.part[p]) {
#pragma unroll
        for (int k = 0; k < 36; ++k)
            out[k] = 0.0;
        return;
    }
    const double* const el = a.w.elim + kCalElim * (int64_t)p;
    arrow_result_update(a.res, p, a.w.n_in[p], a.w.rec + kCalRec * (int64_t)p + arrow_rec_stat(P));
    if (!a.ctl->lm.cov_ok) {
#pragma unroll
        for (int k = 0; k < 36; ++k)
            out[k] = 0.0;
        return;
    }
    // M = I + Y S^-1 Y' (6 x 6, packed lower)
    double M[21];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double T[P];   // row i of Y S^-1
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double v = 0.0;
#pragma unroll
            for (int d = 0; d < P; ++d)
                v += el[arrow_elim_Y(P, i) + d] * a.intr_cov[P * d + c];
            T[c] = v;
        }
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double v = i == j ? 1.0 : 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c)
                v += T[c] * el[arrow_elim_Y(P, j) + c];
            M[tri6(i, j)] = v;
        }
    }
    arrow_marginal_store(el, M, out);
}

} // namespace

void launch_calib_begin(hipStream_t st, const CalibArgs& a)
{
    hipLaunchKernelGGL(k_calib_begin, dim3((unsigned)((a.n_imgs + 63) / 64)), dim3(64), 0, st, a);
}

void launch_calib_classify(hipStream_t st, const CalibArgs& a)
{
    hipLaunchKernelGGL(k_calib_classify, dim3((unsigned)a.n_imgs), dim3(kCalThreads), 0, st, a);
}

void launch_calib_trial(hipStream_t st, const CalibArgs& a)
{
    hipLaunchKernelGGL(k_calib_image, dim3((unsigned)a.n_imgs), dim3(kCalThreads), 0, st, a, 0);
    hipLaunchKernelGGL(k_calib_solve, dim3(1), dim3(kSolveThreads), 0, st, a, 0);
    hipLaunchKernelGGL(k_calib_try, dim3((unsigned)a.n_imgs), dim3(kCalThreads), 0, st, a);
    hipLaunchKernelGGL(k_calib_control, dim3(1), dim3(kCalThreads), 0, st, a);
}

void launch_calib_covariance(hipStream_t st, const CalibArgs& a)
{
    hipLaunchKernelGGL(k_calib_image, dim3((unsigned)a.n_imgs), dim3(kCalThreads), 0, st, a, 1);
    hipLaunchKernelGGL(k_calib_solve, dim3(1), dim3(kSolveThreads), 0, st, a, 1);
    hipLaunchKernelGGL(k_calib_cov_pose, dim3((unsigned)((a.n_imgs + 63) / 64)), dim3(64), 0, st, a);
}

int preload_calibrate_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_begin)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_classify)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_image)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_solve)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_try)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_control)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_calib_cov_pose)) != hipSuccess;
    return bad;
}

} // namespace vmm
