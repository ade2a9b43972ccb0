// The localisation accuracy a pose would have against a finished map whose tags are correlated (gfx950):
// vmm_ba_predict_localization_joint.  k_map_corners, k_tag_faces and k_cam_frames as for k_predict (kernels_predict.hip),
// then
//   k_predict_joint<GIVEN>  wave = pose, two poses per 128-thread workgroup; lane l owns the tags l, l + 64, ... (tag
//                           64 a + l in round a), in both sweeps
//     sweep 1   k_predict<false>'s pass, statement by statement: the visibility rules (GIVEN: the caller's visible_in
//               instead, and whether a selected tag has a corner at z_cam <= 0), the visible bytes, the 21 packed entries
//               of H = sum Jc^T Jc and the count; one wave_sum32 butterfly.  A pose without enough tags ends here.
//     sweep 2   M = sum_s G_s S_ss G_s^T + sum_s sum_{t < s} (X_st + X_st^T), X_st = G_s S_st G_t^T, over the selected tags.
//               For every round a with a selected tag the lane forms the G_s of its own tag once and keeps it in
//               registers.  For every round b <= a the wave stages the G_t of round b's selected tags in LDS, compacted
//               in ascending tag order (ballot + prefix popcount, no atomic; round a's own are stored from the
//               registers, an earlier round's are formed again: four Jacobians per tag are cheap next to the pairs), the
//               list of their tag indices beside them.  A lane with a selected s then walks the list (t < s only when
//               a == b: the entries below its own rank): the 288-byte block S_st straight from global memory
//               (contiguous for the lane, 64-bit index), U = G_s S_st, and X_st = U G_t^T row of G_t by row from LDS, all
//               lanes reading the same address (a broadcast); entry (r, c) of X goes to M[tri6(max, min)], a diagonal
//               entry twice.  The diagonal term G_s S_ss G_s^T follows in round pair (a, a), with k_predict<true>'s
//               statements.
//     result    one more wave_sum32 butterfly for M, then finish_pose<true> (predict_common.hpp), k_predict<true>'s tail.
// Order of every sum: a lane's own in (round a, round b, list) order, then the butterfly: no floating-point atomic, and
// nothing but the selection of the pose depends on the wave's place in the grid.  A pose gives the same bits alone,
// anywhere in any batch and from run to run.
// LDS: 64 x 288 B of G, 64 indices and the 21 entries of H (parked during sweep 2) per wave, 37,712 B per workgroup
// (static).  A wave's stage is written and read by
// that wave alone and a wave's LDS operations complete in order, so a workgroup barrier is not needed (and with one, a
// wave whose pose is beyond n_poses could not leave early): between the write of a stage and its reads, and between the
// reads and the next write, stands a wavefront-scope fence with a wave barrier, which costs no instruction beyond the
// s_waitcnt the reads need anyway and only keeps the compiler from moving LDS accesses across it.
// n_tags is unbounded: nothing is sized by it but the loops.
// The pair work is v (v + 1) / 2 terms of 432 f64 FMAs on the VALU for a pose with v selected tags, spread over the v
// lanes that own them: a wave is busy for about v terms, and a lane in round pair (a, a) for its rank's share.
//
// Registers (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the kernel table of DESIGN.md
// section 9.
#include "predict_common.hpp"

namespace vmm {

namespace {

constexpr int kJointThreads = 128;
constexpr int kJointPoses = kJointThreads / 64;   // poses per workgroup

// orders a wave's LDS writes and reads of its own stage for the compiler; the hardware keeps them in order
__device__ __forceinline__ void wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// G = sum over the four corners of Jc^T Jt of tag t under `cam`: k_predict<true>'s statements
__device__ __forceinline__ void tag_response(const PredictArgs& a, const Intrinsics& K, const Rigid& cam, const int t, double (&G)[6][6])
{
    const double* const w = a.corners + 12 * (int64_t)t;   // read corner by corner in the rolled loop: no indexed private array
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        c[k] = a.faces[kTagFace * (int64_t)t + 3 + k];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q)
            G[r][q] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        double ru, rv, jc[2][6], jt[2][6];
        const double w0 = w[3 * k], w1 = w[3 * k + 1], w2 = w[3 * k + 2];
        world_corner<true>(K, cam, w0, w1, w2, 0.0, 0.0, ru, rv, jc);
        corner_tag_jacobian(cam, jc, w0 - c[0], w1 - c[1], w2 - c[2], jt);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                G[r][q] += jc[0][r] * jt[0][q] + jc[1][r] * jt[1][q];
    }
}

// M += X + X^T, X = Gs S Gt^T; S: a row-major 6 x 6 block in global memory, Gt: a staged G in LDS
__device__ __forceinline__ void pair_term(const double (&Gs)[6][6], const double* __restrict__ S, const double* Gt, double (&M)[21])
{
    double U[6][6];   // Gs S
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double row[6];
#pragma unroll
        for (int c = 0; c < 6; ++c)
            row[c] = S[6 * k + c];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                U[r][c] = k == 0 ? Gs[r][0] * row[c] : U[r][c] + Gs[r][k] * row[c];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double g[6];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            g[k] = Gt[6 * c + k];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double x = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                x += U[r][k] * g[k];
            if (r == c)
                M[tri6(r, r)] += x + x;
            else
                M[r > c ? tri6(r, c) : tri6(c, r)] += x;
        }
    }
}

// M += G S G^T, the lower triangle: k_predict<true>'s statements
__device__ __forceinline__ void diagonal_term(const double (&G)[6][6], const double* __restrict__ S, double (&M)[21])
{
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

// the wave's stage: the G of the round's selected tags in ascending tag order and their indices
__device__ __forceinline__ void stage_round(const bool sel, const int rank, const int t, const double (&G)[6][6], double* s_G, int* s_tag)
{
    wave_fence();   // the reads of the stage before are done
    if (sel) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                s_G[36 * rank + 6 * r + c] = G[r][c];
        s_tag[rank] = t;
    }
    wave_fence();
}

template <bool GIVEN>
__global__ __launch_bounds__(kJointThreads) void k_predict_joint(const PredictJointArgs ja)
{
    __shared__ double s_stage[kJointPoses][64 * 36];
    __shared__ int s_list[kJointPoses][64];
    __shared__ double s_H[kJointPoses][21];
    const PredictArgs& a = ja.p;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = blockIdx.x * kJointPoses + wave;
    if (p >= a.n_poses)   // the whole wave; no workgroup barrier follows
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
    uint8_t* const vis_p = a.visible + (int64_t)p * a.n_tags;
    // ---- sweep 1: the selection, H and the count ----
    double H[21], g[6];
    zero_normal(H, g);
    int n = 0, n_behind = 0;
    for (int t = lane; t < a.n_tags; t += 64) {
        double w[12], f[kTagFace];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            w[k] = a.corners[12 * (int64_t)t + k];
        bool vis;
        if (GIVEN) {
            vis = ja.visible_in[(int64_t)p * a.n_tags + t] != 0;
            if (vis) {
                bool front = true;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    front = front && (cam.R[6] * w[3 * k] + cam.R[7] * w[3 * k + 1] + cam.R[8] * w[3 * k + 2]) + cam.t[2] > 0.0;
                n_behind += front ? 0 : 1;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kTagFace; ++k)
                f[k] = a.faces[kTagFace * (int64_t)t + k];
            vis = tag_visible(a, K, cam, C, w, f);
        }
        vis_p[t] = vis ? 1 : 0;
        if (!vis)
            continue;
        ++n;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            double ru, rv, jc[2][6];
            world_corner<true>(K, cam, w[3 * k], w[3 * k + 1], w[3 * k + 2], 0.0, 0.0, ru, rv, jc);
            accumulate_rows(jc, 0.0, 0.0, H, g);
        }
    }
    double acc[32];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        acc[k] = H[k];
    acc[21] = (double)n;          // exact: counts below 2^53
    acc[22] = (double)n_behind;
#pragma unroll
    for (int k = 23; k < 32; ++k)
        acc[k] = 0.0;
    double tot = wave_sum32(acc, lane);
#pragma unroll
    for (int k = 0; k < 21; ++k)
        H[k] = wave_sum32_fetch(tot, k);
    const int n_visible = (int)wave_sum32_fetch(tot, 21);
    const bool usable = wave_sum32_fetch(tot, 22) == 0.0;
    // ---- sweep 2: M over the pairs of selected tags ----
    double M[21];
    zero_normal(M, g);
    if (n_visible >= a.min_tags && usable) {   // wave-uniform; min_tags >= 1
        // H waits in LDS: next to Gs, U and M it would not fit the register file
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 21; ++k)
                s_H[wave][k] = H[k];
        }
        double* const s_G = s_stage[wave];
        int* const s_tag = s_list[wave];
        const int rounds = (a.n_tags + 63) / 64;
#pragma unroll 1
        for (int ra = 0; ra < rounds; ++ra) {
            const int s = 64 * ra + lane;
            const bool sel_s = s < a.n_tags && vis_p[s] != 0;   // the byte this lane wrote in sweep 1
            const uint64_t mask_s = __ballot(sel_s);
            if (mask_s == 0)
                continue;
            double Gs[6][6];
            if (sel_s)
                tag_response(a, K, cam, s, Gs);
            const double* const S_s = ja.tag_cov_joint + 36 * (int64_t)s * a.n_tags;   // block row s
#pragma unroll 1
            for (int rb = 0; rb <= ra; ++rb) {
                int limit;   // the staged entries this lane pairs with
                if (rb == ra) {
                    limit = __popcll(mask_s & ((1ull << lane) - 1ull));
                    stage_round(sel_s, limit, s, Gs, s_G, s_tag);
                } else {
                    const int t = 64 * rb + lane;   // < n_tags: rb < ra
                    const bool sel_t = vis_p[t] != 0;
                    const uint64_t mask_t = __ballot(sel_t);
                    if (mask_t == 0)
                        continue;
                    double Gt[6][6];
                    if (sel_t)
                        tag_response(a, K, cam, t, Gt);
                    stage_round(sel_t, __popcll(mask_t & ((1ull << lane) - 1ull)), t, Gt, s_G, s_tag);
                    limit = __popcll(mask_t);
                }
                if (!sel_s)
                    continue;
#pragma unroll 1
                for (int j = 0; j < limit; ++j)
                    pair_term(Gs, S_s + 36 * (int64_t)s_tag[j], s_G + 36 * j, M);
                if (rb == ra)
                    diagonal_term(Gs, S_s + 36 * (int64_t)s, M);
            }
        }
#pragma unroll
        for (int k = 0; k < 32; ++k)
            acc[k] = k < 21 ? M[k] : 0.0;
        tot = wave_sum32(acc, lane);
        wave_fence();
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            M[k] = wave_sum32_fetch(tot, k);
            H[k] = s_H[wave][k];
        }
    }
    finish_pose<true>(a, p, lane, cam, H, M, n_visible, usable);
}

} // namespace

void launch_predict_joint(hipStream_t st, const PredictJointArgs& a)
{
    if (a.p.n_poses <= 0)
        return;
    const dim3 grid((unsigned)(((int64_t)a.p.n_poses + kJointPoses - 1) / kJointPoses));
    if (a.visible_in)
        hipLaunchKernelGGL(k_predict_joint<true>, grid, dim3(kJointThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_predict_joint<false>, grid, dim3(kJointThreads), 0, st, a);
}

int preload_predict_joint_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_predict_joint<true>)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_predict_joint<false>)) != hipSuccess;
    return bad;
}

} // namespace vmm
