// The border of the arrowhead system of the joint problem "poses + camera model" (gfx950), for
// vmm_ba_intrinsics_system.  With A the pose normal matrix (cameras and tags), k the nine numbers of the camera model
// (fx, fy, cx, cy, k1, k2, p1, p2, k3), J_k the Jacobian of the residuals over them:
//     [ A   B ] [dx]     [ g  ]        B   = one 6 x 9 block sum J_pose^T J_k per pose
//     [ B^T C ] [dk] = - [ g_k]        C   = J_k^T J_k,  g_k = J_k^T r
// and the reduced camera-model system S_k = C - B^T A^-1 B, r_k = g_k - B^T A^-1 g.
//
// Evaluation: the layout of kernels_eval.hip -- one wave = one Task = up to 64 consecutive observations of ONE pose in a
// family-sorted order, lane = observation -- in one launch of three ranges of workgroups: the eliminated family's order
// (that family's B blocks), the kept family's order (its B blocks), and the eliminated family's order again for the 45 +
// 9 + 1 global sums (C, g_k, cost).  One range with all 109 sums would need 218 accumulator registers per lane next to
// the corner's temporaries; three ranges of at most 55 fit two waves per SIMD like the evaluation.  Wave partials by the
// shared butterfly (wave_sum32), per-pose sums in task order, the global sums by a fixed tree: no floating-point atomics,
// the same bits on every run.
//
// Elimination (kernels_cov.hip's notation; L_e, Z and the factor L of S come from the covariance preamble):
//     Y_E = L_e^-1 [B_e | g_e],   R = [B_F | g_F] - Z^T Y_E,   Y_F = L^-1 R   (launch_cov_trsm_mfma, one 64-column chunk)
//     [B | g]^T A^-1 [B | g] = Y_E^T Y_E + Y_F^T Y_F   (10 x 10; forward substitution only)
#include "engine.hpp"
#include "pose_lm.hpp"

namespace vmm {

constexpr int kBorderPart = 64;    // doubles of a task partial: 54 (B block, row-major 6 x 9) or 45 + 9 + 1 (C lower | g_k | cost), padded
constexpr int kBorderY = 10;       // columns of [B | g]

struct BorderEvalArgs {
    Intrinsics K;
    const Task* tasks;
    int n_tasks;
    const int32_t* other;
    const double* px;
    int64_t n_pad;
    const double* own_pose;
    const double* other_pose;
    const double* tag_wh;
    const uint8_t* cam_const;
    const uint8_t* tag_const;
    int robustify;
    double huber_a;
    double* part;              // [n_tasks][kBorderPart]
    const int32_t* caller;
    const uint8_t* mask;
};

// GLOBAL: the sums that belong to no pose (C, g_k, cost) instead of the own pose's B block.
template <bool OWN_IS_CAM, bool GLOBAL>
__device__ __forceinline__ void border_body(const BorderEvalArgs& a, const int wave)
{
    const int lane = threadIdx.x & 63;
    if (wave >= a.n_tasks)
        return;
    const Task t = a.tasks[wave];
    const int64_t i = (int64_t)t.begin + lane;
    const bool valid = i < t.end;
    const int64_t is = valid ? i : t.begin;
    const int o = a.other[is];
    const int tag_idx = OWN_IS_CAM ? o : t.pose;
    const int cam_idx = OWN_IS_CAM ? t.pose : o;
    Rigid cam, tag;
    load_rigid<true>((OWN_IS_CAM ? a.own_pose : a.other_pose) + 7 * (int64_t)cam_idx, cam);
    load_rigid<true>((OWN_IS_CAM ? a.other_pose : a.own_pose) + 7 * (int64_t)tag_idx, tag);
    const double hw = 0.5 * a.tag_wh[2 * tag_idx], hh = 0.5 * a.tag_wh[2 * tag_idx + 1];
    const bool own_c = (OWN_IS_CAM ? a.cam_const[cam_idx] : a.tag_const[tag_idx]) != 0;
    const bool on = valid && a.mask[a.caller[is]];
    // a switched-off observation is evaluated on the optical axis of an identity camera (its poses are parked defaults
    // and may put the corner on the camera plane) and weighted zero
    const double ct[3] = { on ? cam.t[0] : 0.0, on ? cam.t[1] : 0.0, on ? cam.t[2] : 0.0 };

    constexpr int NACC = GLOBAL ? 55 : 54;
    double acc[64];
#pragma unroll
    for (int k = 0; k < 64; ++k)
        acc[k] = 0.0;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        const double sx = (c == 1 || c == 2) ? hw : -hw;
        const double sy = (c >= 2) ? hh : -hh;
        const double u = a.px[(2 * c) * a.n_pad + is];
        const double v = a.px[(2 * c + 1) * a.n_pad + is];
        // eval_corner's chain (geom.hpp): a = R_t p_l, P_w = a + t_t, b = R_c P_w
        const double a0 = tag.R[0] * sx + tag.R[1] * sy;
        const double a1 = tag.R[3] * sx + tag.R[4] * sy;
        const double a2 = tag.R[6] * sx + tag.R[7] * sy;
        const double w0 = a0 + tag.t[0], w1 = a1 + tag.t[1], w2 = a2 + tag.t[2];
        const double b0 = on ? cam.R[0] * w0 + cam.R[1] * w1 + cam.R[2] * w2 : 0.0;
        const double b1 = on ? cam.R[3] * w0 + cam.R[4] * w1 + cam.R[5] * w2 : 0.0;
        const double b2 = on ? cam.R[6] * w0 + cam.R[7] * w1 + cam.R[8] * w2 : 1.0;
        double ru, rv, jc[2][6], jk[2][9];
        project_camera_point_intrinsics(a.K, b0, b1, b2, ct, u, v, ru, rv, jc, jk);
        double rho0, wgt;
        huber(a.robustify != 0, a.huber_a, ru * ru + rv * rv, rho0, wgt);
        wgt = on ? wgt : 0.0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double jkw[9];
#pragma unroll
            for (int q = 0; q < 9; ++q)
                jkw[q] = jk[r][q] * wgt;
            if (GLOBAL) {
                const double res = (r == 0 ? ru : rv) * wgt;
#pragma unroll
                for (int p = 0; p < 9; ++p) {
                    acc[45 + p] += jkw[p] * res;
#pragma unroll
                    for (int q = 0; q <= p; ++q)
                        acc[tri6(p, q)] += jkw[p] * jkw[q];
                }
            } else {
                double jo[6];
                if (OWN_IS_CAM) {
#pragma unroll
                    for (int k = 0; k < 6; ++k)
                        jo[k] = jc[r][k];
                } else {
                    // the tag half of eval_corner: h = g R_c, rotation about a
                    const double g0 = jc[r][0], g1 = jc[r][1], g2 = jc[r][2];
                    const double h0 = g0 * cam.R[0] + g1 * cam.R[3] + g2 * cam.R[6];
                    const double h1 = g0 * cam.R[1] + g1 * cam.R[4] + g2 * cam.R[7];
                    const double h2 = g0 * cam.R[2] + g1 * cam.R[5] + g2 * cam.R[8];
                    jo[0] = h0;
                    jo[1] = h1;
                    jo[2] = h2;
                    jo[3] = 2.0 * (a1 * h2 - a2 * h1);
                    jo[4] = 2.0 * (a2 * h0 - a0 * h2);
                    jo[5] = 2.0 * (a0 * h1 - a1 * h0);
                }
                const double w_own = own_c ? 0.0 : wgt;
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    const double jp = jo[p] * w_own;
#pragma unroll
                    for (int q = 0; q < 9; ++q)
                        acc[9 * p + q] += jp * jkw[q];
                }
            }
        }
        if (GLOBAL)
            acc[54] += on ? 0.5 * rho0 : 0.0;
    }
    static_assert(NACC <= 64, "two butterflies of 32");
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        double red[32];
#pragma unroll
        for (int k = 0; k < 32; ++k)
            red[k] = acc[32 * half + k];
        const double mine = wave_sum32(red, lane);
        const int slot = wave_sum32_index(lane);
        if (!(lane & 1))
            a.part[(int64_t)wave * kBorderPart + 32 * half + slot] = mine;
    }
}

// workgroups [0, nb_e): B blocks of the eliminated family; [nb_e, nb_e + nb_f): of the kept family; the rest: global sums
template <bool E_IS_CAM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_border_eval(const BorderEvalArgs aE, const BorderEvalArgs aF, const BorderEvalArgs aG, const int nb_e, const int nb_f)
{
    const int b = (int)blockIdx.x;
    if (b < nb_e)
        border_body<E_IS_CAM, false>(aE, (int)((b * blockDim.x + threadIdx.x) >> 6));
    else if (b < nb_e + nb_f)
        border_body<!E_IS_CAM, false>(aF, (int)(((b - nb_e) * blockDim.x + threadIdx.x) >> 6));
    else
        border_body<E_IS_CAM, true>(aG, (int)(((b - nb_e - nb_f) * blockDim.x + threadIdx.x) >> 6));
}

// B[p][k] = sum of the pose's task partials in task order; one thread per (pose, k); family E first
__global__ void k_border_reduce(int n_e, const int32_t* __restrict__ task_e, const double* __restrict__ part_e,
                                double* __restrict__ B_e, int n_f, const int32_t* __restrict__ task_f,
                                const double* __restrict__ part_f, double* __restrict__ B_f)
{
    int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool first = tid < 64 * n_e;
    if (!first)
        tid -= 64 * n_e;
    const int p = tid >> 6, k = tid & 63;
    if (p >= (first ? n_e : n_f) || k >= 54)
        return;
    const int32_t* pt = first ? task_e : task_f;
    const double* part = first ? part_e : part_f;
    double s = 0.0;
    for (int t = pt[p]; t < pt[p + 1]; ++t)
        s += part[(int64_t)t * kBorderPart + k];
    (first ? B_e : B_f)[54 * (int64_t)p + k] = s;
}

// glob[k] = sum over the tasks of partial k (k_sum's tree: a serial prefix per thread, then pairwise); one workgroup per k
__global__ __launch_bounds__(256) void k_border_global(const double* __restrict__ part, int n_tasks, double* __restrict__ glob)
{
    __shared__ double sh[256];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_tasks; i += 256)
        s += part[(int64_t)i * kBorderPart + k];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m)
            sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        glob[k] = sh[0];
}

// Y_E[6 e + r][0..9] = L_e^-1 [B_e | g_e]; one thread per eliminated pose.  An inactive pose (constant, or without an
// active observation: zero B and g, and nobody may have written its L_e) gets zeros.
__global__ __launch_bounds__(64) void k_border_ye(int n_e, const double* __restrict__ Le, const double* __restrict__ B_e,
                            const double* __restrict__ g_e, const int32_t* __restrict__ active_e, double* __restrict__ YE)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_e)
        return;
    double* out = YE + (int64_t)6 * e * kBorderY;
    if (!active_e[e]) {
        for (int k = 0; k < 6 * kBorderY; ++k)
            out[k] = 0.0;
        return;
    }
    const double* L = Le + 36 * (int64_t)e;
#pragma unroll   // as the compiler unrolled the written-out loop by itself: ten independent columns in flight
    for (int c = 0; c < kBorderY; ++c) {
        forward_substitute<6>(
            L, RowMajor<6>{}, [&](const int r) { return c < 9 ? B_e[54 * (int64_t)e + 9 * r + c] : g_e[6 * (int64_t)e + r]; },
            [&](const int r, const double t) { out[r * kBorderY + c] = t; });
    }
}

// R[r][0..63] = [B_F | g_F | 0] - (Z^T Y_E)[r]: one thread per row of the (padded) reduced system, the rows of Z in
// ascending order, ten accumulators.  Lanes read consecutive doubles of a row of Z; Y_E's row is uniform.
__global__ __launch_bounds__(256) void k_border_rhs(int n_red, int n_pad, int k_dim, const double* __restrict__ Z, int ldz,
                                                     const double* __restrict__ YE, const double* __restrict__ B_f,
                                                     const double* __restrict__ g_f, double* __restrict__ R)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pad)
        return;
    double acc[kBorderY];
#pragma unroll
    for (int c = 0; c < kBorderY; ++c)
        acc[c] = 0.0;
    if (r < n_red) {
        const int f = r / 6, a = r - 6 * f;
#pragma unroll
        for (int c = 0; c < 9; ++c)
            acc[c] = B_f[54 * (int64_t)f + 9 * a + c];
        acc[9] = g_f[r];
        for (int k = 0; k < k_dim; ++k) {
            const double z = Z[(int64_t)k * ldz + r];
            const double* y = YE + (int64_t)k * kBorderY;
#pragma unroll
            for (int c = 0; c < kBorderY; ++c)
                acc[c] -= z * y[c];
        }
    }
    double* out = R + (int64_t)r * 64;
#pragma unroll
    for (int c = 0; c < kBorderY; ++c)
        out[c] = acc[c];
    for (int c = kBorderY; c < 64; ++c)
        out[c] = 0.0;
}

// out = cost | g_k[9] | C[81] | r_k[9] | S_k[81] from glob (C lower | g_k | cost) and the 10 x 10 Gram matrix
// Y_E^T Y_E + Y_F^T Y_F: one workgroup; a thread sums its rows (Y_E first, ascending), a wave meets in wave_sum's
// butterfly, the four waves are added in wave order.
__global__ __launch_bounds__(256) void k_border_gram(int k_dim, const double* __restrict__ YE, int n_pad,
                                                      const double* __restrict__ YF, const double* __restrict__ glob,
                                                      double* __restrict__ out)
{
    __shared__ double sh[4][56];
    __shared__ double G[56];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double g[55];
#pragma unroll
    for (int q = 0; q < 55; ++q)
        g[q] = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        const double* Y = pass ? YF : YE;
        const int n = pass ? n_pad : k_dim, ld = pass ? 64 : kBorderY;
        for (int r = tid; r < n; r += 256) {
            double y[kBorderY];
#pragma unroll
            for (int c = 0; c < kBorderY; ++c)
                y[c] = Y[(int64_t)r * ld + c];
            int q = 0;
#pragma unroll
            for (int a = 0; a < kBorderY; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b)
                    g[q++] += y[a] * y[b];
        }
    }
#pragma unroll
    for (int q = 0; q < 55; ++q) {
        const double s = wave_sum(g[q]);
        if (lane == 0)
            sh[wave][q] = s;
    }
    __syncthreads();
    if (tid < 55)
        G[tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    __syncthreads();
    if (tid < 81) {
        const int i = tid / 9, j = tid - 9 * i;
        const int lo = i >= j ? tri6(i, j) : tri6(j, i);
        const double c = glob[lo];
        out[10 + tid] = c;
        out[100 + tid] = c - G[lo];
    } else if (tid < 90) {
        const int j = tid - 81;
        out[1 + j] = glob[45 + j];
        out[91 + j] = glob[45 + j] - G[tri6(9, j)];
    } else if (tid == 90) {
        out[0] = glob[54];
    }
}

// ---- launchers -------------------------------------------------------------------------------------

size_t border_workspace_doubles(const Engine& e)
{
    return (size_t)kBorderPart * (2 * (size_t)e.ordE.n_tasks + (size_t)e.ordF.n_tasks) + 54 * (size_t)(e.n_e + e.n_f) + 64
        + (size_t)kBorderY * e.k_dim + 64 * (size_t)e.n_pad + kBorderOut;
}

static BorderEvalArgs make_border_args(Engine& e, const ObsOrder& ord, bool own_is_cam, int robustify, double huber_a,
                                       double* part)
{
    BorderEvalArgs a;
    a.K = e.K;
    a.tasks = ord.tasks;
    a.n_tasks = ord.n_tasks;
    a.other = ord.other;
    a.px = ord.px;
    a.n_pad = ord.n_pad;
    a.own_pose = own_is_cam ? e.cam_qt : e.tag_qt;
    a.other_pose = own_is_cam ? e.tag_qt : e.cam_qt;
    a.tag_wh = e.tag_wh;
    a.cam_const = e.pose_const;
    a.tag_const = e.pose_const + e.n_cams;
    a.robustify = robustify;
    a.huber_a = huber_a;
    a.part = part;
    a.caller = ord.caller;
    a.mask = e.obs_mask;
    return a;
}

// ws: border_workspace_doubles(e) doubles.  The evaluation at the current poses and the handle's camera model, then the
// elimination against the factors the covariance preamble left behind; the result is the last kBorderOut doubles of ws
// (returned).
double* launch_border(Engine& e, int robustify, double huber_a, double* ws)
{
    const int nt_e = e.ordE.n_tasks, nt_f = e.ordF.n_tasks;
    double* part_e = ws;
    double* part_f = part_e + (size_t)kBorderPart * nt_e;
    double* part_g = part_f + (size_t)kBorderPart * nt_f;
    double* B_e = part_g + (size_t)kBorderPart * nt_e;
    double* B_f = B_e + 54 * (size_t)e.n_e;
    double* glob = B_f + 54 * (size_t)e.n_f;
    double* YE = glob + 64;
    double* R = YE + (size_t)kBorderY * e.k_dim;
    double* out = R + 64 * (size_t)e.n_pad;
    const bool e_is_cam = e.elim_cams;
    const BorderEvalArgs aE = make_border_args(e, e.ordE, e_is_cam, robustify, huber_a, part_e);
    const BorderEvalArgs aF = make_border_args(e, e.ordF, !e_is_cam, robustify, huber_a, part_f);
    const BorderEvalArgs aG = make_border_args(e, e.ordE, e_is_cam, robustify, huber_a, part_g);
    const int nb_e = (nt_e + 3) / 4, nb_f = (nt_f + 3) / 4;
    if (2 * nb_e + nb_f > 0) {
        if (e_is_cam)
            hipLaunchKernelGGL((k_border_eval<true>), dim3(2 * nb_e + nb_f), dim3(256), 0, e.stream, aE, aF, aG, nb_e, nb_f);
        else
            hipLaunchKernelGGL((k_border_eval<false>), dim3(2 * nb_e + nb_f), dim3(256), 0, e.stream, aE, aF, aG, nb_e, nb_f);
    }
    hipLaunchKernelGGL(k_border_reduce, dim3(((e.n_e + e.n_f) * 64 + 255) / 256), dim3(256), 0, e.stream, e.n_e,
                       (const int32_t*)e.ordE.pose_task, (const double*)part_e, B_e, e.n_f,
                       (const int32_t*)e.ordF.pose_task, (const double*)part_f, B_f);
    hipLaunchKernelGGL(k_border_global, dim3(55), dim3(256), 0, e.stream, (const double*)part_g, nt_e, glob);
    const int e_off = e_is_cam ? 0 : e.n_cams;   // cameras first in `active`
    hipLaunchKernelGGL(k_border_ye, dim3((e.n_e + 63) / 64), dim3(64), 0, e.stream, e.n_e, (const double*)e.Le,
                       (const double*)B_e, (const double*)(e_is_cam ? e.g_cam : e.g_tag),
                       (const int32_t*)(e.active + e_off), YE);
    hipLaunchKernelGGL(k_border_rhs, dim3((e.n_pad + 255) / 256), dim3(256), 0, e.stream, e.n_red, e.n_pad, e.k_dim,
                       (const double*)e.Z, e.ldz, (const double*)YE, (const double*)B_f,
                       (const double*)(e_is_cam ? e.g_tag : e.g_cam), R);
    launch_cov_trsm_mfma(e, R, 64, std::vector<int>((size_t)e.n_blk, 1));
    hipLaunchKernelGGL(k_border_gram, dim3(1), dim3(256), 0, e.stream, e.k_dim, (const double*)YE, e.n_pad,
                       (const double*)R, (const double*)glob, out);
    return out;
}

int preload_border_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_eval<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_eval<false>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_reduce)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_global)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_ye)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_rhs)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_border_gram)) != hipSuccess;
    return bad;
}

} // namespace vmm
