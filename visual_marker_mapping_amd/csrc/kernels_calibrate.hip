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
// Shared with kernels_localize.hip through image_sums.hpp: the image view, the rotation of a world corner, the
// classification (k_calib_classify is classify_image under the current model) and the cost-only sum (k_calib_try's
// candidate cost is image_sums<false, false>); from pose_lm.hpp: tri6, project_camera_point_intrinsics, the accept /
// stop rules and lower_inverse / lower_gram (both covariances).  The camera model is loaded by engine.hpp's
// make_intrinsics.  Calibration's own: the 15-wide sums (image_normal_sums) and the three small Cholesky loops, whose
// pivot tests differ (damped in k_calib_image, weighted in chol9).
//
// Registers (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, the .s file's .vgpr_count / .vgpr_spill_count /
// .private_segment_fixed_size): the table at k_calib_image below.
#include "engine.hpp"
#include "image_sums.hpp"

namespace vmm {

namespace {

constexpr int kCalThreads = 256;
constexpr int kCalWaves = kCalThreads / 64;
constexpr int kCalSums = 137;     // 120 (15 x 15 packed lower: pose 0..5, model 6..14) + 15 gradient + cost + sum |r|^2
constexpr int kCalChunks = 5;     // wave_sum32 calls that cover them
constexpr int kSolveThreads = 512;

static_assert(kCalThreads == kImageThreads, "classify_image and image_sums stride by kImageThreads");

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
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_imgs)
        return;
    const vmm_ba_localize_result r = a.res[p];
    a.n_in[p] = r.n_inlier_obs;
    a.part[p] = r.status == VMM_BA_LOC_OK && r.n_inlier_obs >= a.min_inliers;
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
    const int n = classify_image<false>(make_intrinsics(a.ctl->k), v, a.cam_qt + 7 * (int64_t)p, a.inlier2,
                                        a.flags + a.img_start[p], s_cnt);
    if (threadIdx.x == 0) {
        a.n_in[p] = n;
        a.part[p] = n >= a.min_inliers;
    }
}

// An image's sums into s_tot: the packed lower triangle of its 15 x 15 normal matrix (pose 0..5, model 6..14: A, B and
// C_i; entries 0..119), the gradient (120..134), the cost (135) and sum |r|^2 (136), the Huber corrector applied.
// Each thread sums privately in list order, then one butterfly per wave (wave_sum32, five of them for the 137 sums),
// then the waves in order through LDS.
__device__ __forceinline__ void image_normal_sums(const ImageView<false>& v, const uint8_t* flags, const Intrinsics& K,
                                                  const Rigid& cam, const int mask, const bool robust, const double huber_a,
                                                  double* s_red, double* s_tot)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[kCalChunks][32];
#pragma unroll
    for (int c = 0; c < kCalChunks; ++c)
#pragma unroll
        for (int k = 0; k < 32; ++k)
            acc[c][k] = 0.0;
#define VMM_ACC(i) acc[(i) >> 5][(i) & 31]
    for (int d = tid; d < v.m; d += kCalThreads) {
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
            VMM_ACC(135) += rho0;
            VMM_ACC(136) += s;
#pragma unroll
            for (int i = 0; i < 15; ++i) {
                VMM_ACC(120 + i) += J[0][i] * ru + J[1][i] * rv;
#pragma unroll
                for (int k = 0; k <= i; ++k)
                    VMM_ACC(tri6(i, k)) += J[0][i] * J[0][k] + J[1][i] * J[1][k];
            }
        }
    }
#undef VMM_ACC
#pragma unroll
    for (int c = 0; c < kCalChunks; ++c) {
        const double tot = wave_sum32(acc[c], lane);
        s_red[(wave * kCalChunks + c) * 32 + wave_sum32_index(lane)] = tot;   // lanes 2 m and 2 m + 1 store the same value
    }
    __syncthreads();
    if (tid < kCalSums) {
        double t = s_red[tid];
#pragma unroll
        for (int w = 1; w < kCalWaves; ++w)
            t += s_red[w * 32 * kCalChunks + tid];
        s_tot[tid] = t;
    }
    __syncthreads();
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
    __shared__ double s_red[kCalWaves * 32 * kCalChunks];
    __shared__ double s_tot[kCalSums];
    __shared__ double s_L[21];
    __shared__ double s_Y[6][10];   // column 9: y
    __shared__ int s_bad;
    const CalibCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->done)
        return;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    double* const rec = a.rec + kCalRec * (int64_t)p;
    double* const el = a.elim + kCalElim * (int64_t)p;
    if (!a.part[p]) {
        if (tid < kCalRec)
            rec[tid] = 0.0;
        return;
    }
    const Intrinsics K = make_intrinsics(ctl->k);
    const int mask = ctl->refine_mask;
    const bool robust = a.robustify != 0;
    Rigid cam;
    load_rigid<true>(a.cam_qt + 7 * (int64_t)p, cam);
    image_normal_sums(image_view(a, p), a.flags + a.img_start[p], K, cam, mask, robust, a.huber_a, s_red, s_tot);
    // L = chol(A + lam diag(max(A_ii, 1e-12))), as solve6 damps
    if (tid == 0) {
        const double lam = cov_mode ? 0.0 : ctl->lam;
        double L[21];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double ajj = s_tot[tri6(j, j)];
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
                double v = s_tot[tri6(i, j)];
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
    // column c of Y = L^-1 B (c < 9: B[.][c] = row 6 + c of the packed matrix) and y = L^-1 g (c == 9)
    if (tid < 10) {
        double col[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = tid < 9 ? s_tot[tri6(6 + tid, i)] : s_tot[120 + i];
#pragma unroll
            for (int k = 0; k < i; ++k)
                v -= s_L[tri6(i, k)] * col[k];
            col[i] = v / s_L[tri6(i, i)];
            s_Y[i][tid] = col[i];
        }
    }
    __syncthreads();
    if (tid < kCalRec) {
        double v;
        if (tid < 45) {   // C_i - Y'Y, packed lower
            int r = 0;
            while (tri6(r + 1, 0) <= tid)
                ++r;
            const int c = tid - tri6(r, 0);
            v = s_tot[tri6(6 + r, 6 + c)];
#pragma unroll
            for (int k = 0; k < 6; ++k)
                v -= s_Y[k][r] * s_Y[k][c];
        } else if (tid < 54) {   // g_k,i - Y'y
            const int c = tid - 45;
            v = s_tot[120 + 6 + c];
#pragma unroll
            for (int k = 0; k < 6; ++k)
                v -= s_Y[k][c] * s_Y[k][9];
        } else if (tid < 63) {
            const int c = tid - 54;
            v = s_tot[tri6(6 + c, 6 + c)];
        } else if (tid == 63) {
            v = s_tot[135];
        } else if (tid == 64) {
            v = s_tot[136];
        } else if (tid == 65) {
            v = s_bad ? 1.0 : 0.0;
        } else if (tid == 66) {
            v = (double)a.n_in[p];
        } else {
            v = 1.0;
        }
        rec[tid] = v;
    } else if (tid >= 128 && tid < 128 + 21) {
        el[tid - 128] = s_L[tid - 128];
    } else if (tid >= 160 && tid < 160 + 60) {
        const int e = tid - 160, k = e / 10, c = e - 10 * k;
        el[c < 9 ? 21 + 9 * k + c : 75 + k] = s_Y[k][c];
    }
}

// 9 x 9 packed lower M (unit diagonal after the caller's scaling) -> its Cholesky factor in place; false: a pivot times
// its weight is not above min_pivot, or not finite
__device__ __forceinline__ bool chol9(double (&M)[45], const double (&weight)[9], const double min_pivot)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        double d = M[tri6(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k)
            d -= M[tri6(j, k)] * M[tri6(j, k)];
        ok = ok && d * weight[j] > min_pivot && finite_bits(d);
        const double sq = sqrt(d);
        M[tri6(j, j)] = sq;
        const double is = 1.0 / sq;
#pragma unroll
        for (int i = j + 1; i < 9; ++i) {
            double v = M[tri6(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k)
                v -= M[tri6(i, k)] * M[tri6(j, k)];
            M[tri6(i, j)] = v * is;
        }
    }
    return ok;
}

// When is the undamped S = sum (C_i - Y'Y) singular?  Its entries come out of a cancellation and carry rounding errors
// of a few eps sqrt(C_aa C_bb), C = sum C_i: scaled by diag(C) they are known to about 1e-15, and so are the pivots of
// that scaling (the factorisation runs on the unit-diagonal scaling by diag(S); a pivot of one scaling is the other's
// times S_jj / C_jj).  A pivot within a factor 100 of that noise is taken for the zero of a singular matrix.
constexpr double kCalMinPivot = 1e-13;

__global__ __launch_bounds__(kSolveThreads) void k_calib_solve(const CalibArgs a, const int cov_mode)
{
    __shared__ double s_part[4][kCalRec];
    __shared__ double s_tot[kCalRec];
    CalibCtl* const ctl = a.ctl;
    if (!cov_mode && ctl->done)
        return;
    const int tid = threadIdx.x, e = tid & 127, grp = tid >> 7;
    if (e < kCalRec) {
        double t = 0.0;
        for (int i = grp; i < a.n_imgs; i += 4)
            t += a.rec[kCalRec * (int64_t)i + e];
        s_part[grp][e] = t;
    }
    __syncthreads();
    if (tid < kCalRec)
        s_tot[tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
    __syncthreads();
    if (tid != 0)
        return;
    const double cost = s_tot[63], raw2 = s_tot[64];
    const bool images_ok = s_tot[65] == 0.0;
    const int n_used = (int)s_tot[67], n_obs_used = (int)s_tot[66];
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
    const int mask = ctl->refine_mask;
    const double lam = cov_mode ? 0.0 : ctl->lam;
    if (!cov_mode) {
        if (n_used == 0 || !finite_bits(cost) || lam > kLamMax) {
            ctl->done = 1;
            ctl->stop = 1;
            return;
        }
        if (ctl->trials >= ctl->max_trials) {
            ctl->done = 1;
            ctl->stop = 2;
            return;
        }
        ctl->trials += 1;
    }
    // damp, give the fixed parameters unit rows, scale to a unit diagonal
    double M[45], sc[9], weight[9];
    bool ok = images_ok;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const bool free_j = (mask >> j) & 1;
        const double d = free_j ? s_tot[tri6(j, j)] + lam * s_tot[54 + j] : 1.0;
        ok = ok && d > 0.0 && finite_bits(d);
        sc[j] = free_j ? 1.0 / sqrt(d) : 1.0;
        weight[j] = cov_mode && free_j ? d / s_tot[54 + j] : 1.0;   // S_jj / C_jj
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const bool both = ((mask >> i) & 1) && ((mask >> j) & 1);
            M[tri6(i, j)] = i == j ? 1.0 : (both ? s_tot[tri6(i, j)] * sc[i] * sc[j] : 0.0);
        }
    ok = chol9(M, weight, cov_mode ? kCalMinPivot : 0.0) && ok;
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
        ctl->cov_ok = ok ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j)
                a.intr_cov[9 * i + j] = ok ? (i >= j ? M[tri6(i, j)] : M[tri6(j, i)]) : 0.0;
        return;
    }
    // (L L') z = -D g_k, dk = D z
    double z[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double v = ((mask >> i) & 1) ? -s_tot[45 + i] * sc[i] : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k)
            v -= M[tri6(i, k)] * z[k];
        z[i] = v / M[tri6(i, i)];
    }
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
    ctl->solve_ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(kCalThreads) void k_calib_try(const CalibArgs a)
{
    __shared__ double s_red[kCalWaves];
    const CalibCtl* const ctl = a.ctl;
    if (ctl->done || !ctl->solve_ok)
        return;
    const int p = blockIdx.x;
    if (!a.part[p]) {
        if (threadIdx.x == 0)
            a.trial[2 * p] = a.trial[2 * p + 1] = 0.0;
        return;
    }
    const double* const el = a.elim + kCalElim * (int64_t)p;
    // dp = -L^-T (y + Y dk); every thread computes it
    double w[6], dp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = el[75 + k];
#pragma unroll
        for (int c = 0; c < 9; ++c)
            v += el[21 + 9 * k + c] * ctl->dk[c];
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
    pose_plus(a.cam_qt + 7 * (int64_t)p, dp, cand);
    double A[21], g[6], raw2;   // not filled by the cost-only sum
    const double cost = image_sums<false, false>(make_intrinsics(ctl->k_cand), image_view(a, p), cand, a.flags + a.img_start[p],
                                                 a.robustify != 0, a.huber_a, s_red, A, g, raw2);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
            a.cam_cand[7 * (int64_t)p + k] = cand[k];
        a.trial[2 * p] = cost;
        a.trial[2 * p + 1] = max_abs6(dp);
    }
}

// lm_refine's decision (pose_lm.hpp) on the whole problem.  The step's size: the largest pose-tangent component and
// the largest model component relative to max(|k_j|, 1).
__global__ __launch_bounds__(kCalThreads) void k_calib_control(const CalibArgs a)
{
    __shared__ double s_sum[kCalWaves], s_max[kCalWaves];
    CalibCtl* const ctl = a.ctl;
    if (ctl->done)
        return;
    const int tid = threadIdx.x;
    if (!ctl->solve_ok) {   // a trial spent on a system that was not positive definite
        if (tid == 0)
            ctl->lam *= 10.0;
        return;
    }
    double cc = 0.0, sm = 0.0;
    for (int i = tid; i < a.n_imgs; i += kCalThreads) {
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
    for (int w = 1; w < kCalWaves; ++w) {
        cc += s_sum[w];
        sm = s_max[w] > sm ? s_max[w] : sm;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double kj = fabs(ctl->k[j]);
        const double s = fabs(ctl->dk[j]) / (kj > 1.0 ? kj : 1.0);
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
        for (int i = tid; i < a.n_imgs; i += kCalThreads)
            if (a.part[i])
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    a.cam_qt[7 * (int64_t)i + k] = a.cam_cand[7 * (int64_t)i + k];
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j)
                ctl->k[j] = ctl->k_cand[j];
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

// thread = image, after k_calib_image and k_calib_solve in cov_mode: the joint marginal of the pose and the image's
// statistics at the result
__global__ __launch_bounds__(64) void k_calib_cov_pose(const CalibArgs a)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_imgs)
        return;
    double* const out = a.cam_cov + 36 * (int64_t)p;
    if (!a.part[p]) {
#pragma unroll
        for (int k = 0; k < 36; ++k)
            out[k] = 0.0;
        return;
    }
    const double* const rec = a.rec + kCalRec * (int64_t)p;
    const double* const el = a.elim + kCalElim * (int64_t)p;
    const int n_in = a.n_in[p];
    vmm_ba_localize_result r = a.res[p];
    r.n_inlier_obs = n_in;
    r.cost = 0.5 * rec[63];
    r.rms_px = sqrt(rec[64] / (4.0 * n_in));
    a.res[p] = r;
    if (!a.ctl->cov_ok) {
#pragma unroll
        for (int k = 0; k < 36; ++k)
            out[k] = 0.0;
        return;
    }
    // M = I + Y S^-1 Y' (6 x 6, packed lower)
    double M[21];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double T[9];   // row i of Y S^-1
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            double v = 0.0;
#pragma unroll
            for (int d = 0; d < 9; ++d)
                v += el[21 + 9 * i + d] * a.intr_cov[9 * d + c];
            T[c] = v;
        }
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double v = i == j ? 1.0 : 0.0;
#pragma unroll
            for (int c = 0; c < 9; ++c)
                v += T[c] * el[21 + 9 * j + c];
            M[tri6(i, j)] = v;
        }
    }
    double W[21];   // L^-1, lower
    lower_inverse<6>(el, W);
    // cov = W' M W: P = M W (full 6 x 6), cov[r][c] = sum_k W[k][r] P[k][c]
    double P[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
#pragma unroll
            for (int k = c; k < 6; ++k)
                v += (i >= k ? M[tri6(i, k)] : M[tri6(k, i)]) * W[tri6(k, c)];
            P[i][c] = v;
        }
    double sum = 0.0, C[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double v = 0.0;
#pragma unroll
            for (int k = r; k < 6; ++k)
                v += W[tri6(k, r)] * P[k][c];
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
