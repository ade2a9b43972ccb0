// The localisation accuracy a pose would have against a finished map (gfx950): vmm_ba_predict_localization.
//   k_map_corners   (kernels_localize.hip, as it is) the four world corners of every map tag, once per call
//   k_tag_faces     thread = tag: the normal n = R e_z and the centre of every map tag, once per call
//   k_cam_frames    (kernels_triangulate.hip, as it is) R, t and the centre C = -R^T t of every pose
//   k_predict<MAP>  wave = pose, four poses per 256-thread workgroup:
//                   tags     lanes stride the tag list (lane l takes tags l, l + 64, ...): the visibility rules of
//                            include/vmm_ba.h with the cheap tests first (facing, the four depths, then per corner the
//                            monotone test and the pixel, then the sides); only for a visible tag the 21 packed
//                            entries of H = sum Jc^T Jc (world_corner<true>, accumulate_rows) and, with MAP, the tag's
//                            G = sum Jc^T Jt and the 21 packed entries of G S G^T
//                   sums     one wave_sum32 butterfly for H and the count, one more for M with MAP; every lane then
//                            fetches the totals from the lanes that hold them
//                   result   every lane runs the same spd_inverse<6>, the sandwich H^-1 M H^-1 and the two sigmas;
//                            lane 0 stores 36 + 36 doubles and the record, all lanes store their visible bytes
// The tag Jacobian is eval_corner<true, true>'s (geom.hpp) formed from the tables: the translation columns are
// g^T R_cam, the rotation columns 2 (a x h) with a = world corner - centre.  The rules, the fetch of the totals and the
// store are in predict_common.hpp, which k_predict_joint (kernels_predict_joint.hip) shares; the tag Jacobian and the
// tail below stand there a second time, because calling them from here changed this kernel's register allocation and
// the last bits of cov_map.
// No LDS, no barrier, no atomic.  A wave never waits on another, nothing but the selection of the pose depends on the
// wave's place in the grid, and every sum has a fixed order (a lane's own sum in list order, then the butterfly): a pose
// gives the same bits alone, anywhere in any batch and from run to run.  The tables (200 tags x 144 B) stay in L2; a
// pose's frame is wave-uniform and read through the scalar cache.
//
// Registers (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the kernel table of DESIGN.md
// section 9.
#include "predict_common.hpp"

namespace vmm {

namespace {

constexpr int kPredThreads = 256;
constexpr int kPredPoses = kPredThreads / 64;   // poses per workgroup

__global__ __launch_bounds__(256) void k_tag_faces(int n_tags, const double* __restrict__ tag_qt, double* __restrict__ faces)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tags)
        return;
    Rigid tag;
    load_rigid<true>(tag_qt + 7 * (int64_t)t, tag);
    double* const f = faces + kTagFace * (int64_t)t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[k] = tag.R[3 * k + 2];
        f[3 + k] = tag.t[k];
    }
}

template <bool MAP>
__global__ __launch_bounds__(kPredThreads) void k_predict(const PredictArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kPredPoses + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= a.n_poses)   // the whole wave
        return;
    const Intrinsics K = a.K;
    const double* const fr = a.frames + kCamFrame * (int64_t)p;
    Rigid cam;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        cam.R[k] = fr[k];
    double C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cam.t[k] = fr[9 + k];
        C[k] = fr[12 + k];
    }
    double H[21], g[6], M[21];
    zero_normal(H, g);
    if (MAP)
        zero_normal(M, g);
    int n = 0;
    for (int t = lane; t < a.n_tags; t += 64) {
        double w[12], f[kTagFace];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            w[k] = a.corners[12 * (int64_t)t + k];
#pragma unroll
        for (int k = 0; k < kTagFace; ++k)
            f[k] = a.faces[kTagFace * (int64_t)t + k];
        const bool vis = tag_visible(a, K, cam, C, w, f);
        if (a.visible)
            a.visible[(int64_t)p * a.n_tags + t] = vis ? 1 : 0;
        if (!vis)
            continue;
        ++n;
        double G[6][6];
        if (MAP) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    G[r][c] = 0.0;
        }
#pragma unroll 1   // rolled: four corners' Jacobians next to H, M and G would only cost registers
        for (int k = 0; k < 4; ++k) {
            double ru, rv, jc[2][6];
            world_corner<true>(K, cam, w[3 * k], w[3 * k + 1], w[3 * k + 2], 0.0, 0.0, ru, rv, jc);
            accumulate_rows(jc, 0.0, 0.0, H, g);
            if (MAP) {
                const double a0 = w[3 * k] - f[3], a1 = w[3 * k + 1] - f[4], a2 = w[3 * k + 2] - f[5];
                double jt[2][6];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const double h0 = jc[r][0] * cam.R[0] + jc[r][1] * cam.R[3] + jc[r][2] * cam.R[6];
                    const double h1 = jc[r][0] * cam.R[1] + jc[r][1] * cam.R[4] + jc[r][2] * cam.R[7];
                    const double h2 = jc[r][0] * cam.R[2] + jc[r][1] * cam.R[5] + jc[r][2] * cam.R[8];
                    jt[r][0] = h0;
                    jt[r][1] = h1;
                    jt[r][2] = h2;
                    jt[r][3] = 2.0 * (a1 * h2 - a2 * h1);
                    jt[r][4] = 2.0 * (a2 * h0 - a0 * h2);
                    jt[r][5] = 2.0 * (a0 * h1 - a1 * h0);
                }
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        G[r][c] += jc[0][r] * jt[0][c] + jc[1][r] * jt[1][c];
            }
        }
        if (MAP) {
            const double* const S = a.tag_cov + 36 * (int64_t)t;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double T[6];   // row r of G S
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k)
                        s += G[r][k] * S[6 * k + c];
                    T[c] = s;
                }
#pragma unroll
                for (int b = 0; b <= r; ++b) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k)
                        s += T[k] * G[b][k];
                    M[tri6(r, b)] += s;
                }
            }
        }
    }
    // ---- the wave's totals, in every lane ----
    double acc[32];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        acc[k] = H[k];
    acc[21] = (double)n;   // exact: a count below 2^53
#pragma unroll
    for (int k = 22; k < 32; ++k)
        acc[k] = 0.0;
    double tot = wave_sum32(acc, lane);
#pragma unroll
    for (int k = 0; k < 21; ++k)
        H[k] = wave_sum32_fetch(tot, k);
    vmm_ba_predict_result res;
    res.n_visible = (int)wave_sum32_fetch(tot, 21);
    res.sigma_pos_m = 0.0;
    res.sigma_rot_rad = 0.0;
    if (MAP) {
#pragma unroll
        for (int k = 0; k < 32; ++k)
            acc[k] = k < 21 ? M[k] : 0.0;
        tot = wave_sum32(acc, lane);
#pragma unroll
        for (int k = 0; k < 21; ++k)
            M[k] = wave_sum32_fetch(tot, k);
    }
    // ---- the result: every lane holds the same sums and takes the same way ----
    double P[21], Q[21];
    bool have = false;
    if (res.n_visible == 0)
        res.status = VMM_BA_PRED_NO_VISIBLE_TAG;
    else if (res.n_visible < a.min_tags)
        res.status = VMM_BA_PRED_TOO_FEW_TAGS;
    else {
        res.status = VMM_BA_PRED_SINGULAR;
        double Cv[21];
        have = spd_inverse<6>(H, Cv);
        if (MAP)
            have = sandwich6(Cv, M, Q) && have;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            P[k] = a.sigma2 * Cv[k];
            if (!MAP)
                Q[k] = 0.0;
            sum += fabs(P[k]);
        }
        have = have && finite_bits(sum);
        // dC = -R^T (dt + 2 [t]x dr): R is orthogonal, so the trace of the centre's covariance is that of A V A^T with
        // A = [I | 2 [t]x] and V = cov_px + cov_map; radians are twice the tangent's rotation part
        const double tx = 2.0 * cam.t[0], ty = 2.0 * cam.t[1], tz = 2.0 * cam.t[2];
        const double A[3][6] = { { 1.0, 0.0, 0.0, 0.0, -tz, ty }, { 0.0, 1.0, 0.0, tz, 0.0, -tx }, { 0.0, 0.0, 1.0, -ty, tx, 0.0 } };
        double pos = 0.0, rot = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    if ((r == i || r >= 3) && (c == i || c >= 3))
                        pos += A[i][r] * (sym6(P, r, c) + sym6(Q, r, c)) * A[i][c];
            rot += sym6(P, 3 + i, 3 + i) + sym6(Q, 3 + i, 3 + i);
        }
        rot *= 4.0;
        have = have && finite_bits(pos) && finite_bits(rot) && pos >= 0.0 && rot >= 0.0;
        if (have) {
            res.status = VMM_BA_PRED_OK;
            res.sigma_pos_m = sqrt(pos);
            res.sigma_rot_rad = sqrt(rot);
        }
    }
    if (lane == 0)
        store_pose(a, p, have, P, Q, res);
}

} // namespace

void launch_tag_faces(hipStream_t st, int n_tags, const double* tag_qt, double* faces)
{
    if (n_tags <= 0)
        return;
    hipLaunchKernelGGL(k_tag_faces, dim3((unsigned)((n_tags + 255) / 256)), dim3(256), 0, st, n_tags, tag_qt, faces);
}

void launch_predict(hipStream_t st, const PredictArgs& a)
{
    if (a.n_poses <= 0)
        return;
    const dim3 grid((unsigned)(((int64_t)a.n_poses + kPredPoses - 1) / kPredPoses));
    if (a.tag_cov)
        hipLaunchKernelGGL(k_predict<true>, grid, dim3(kPredThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_predict<false>, grid, dim3(kPredThreads), 0, st, a);
}

int preload_predict_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_tag_faces)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_predict<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_predict<false>)) != hipSuccess;
    return bad;
}

} // namespace vmm
