// The arrowhead solver of the two joint refinements against a fixed map (gfx950): vmm_ba_calibrate (kernels_calibrate.hip:
// the nine numbers of the camera model and one pose per image) and vmm_ba_rig_calibrate (kernels_rig.hip: the 6 K
// extrinsic parameters and one rig pose per frame).  An item is an image or a frame; its pose has 6 degrees of freedom,
// the shared unknowns are P (9; 6 K).  The normal equations are
//     [ A_i  B_i ] [dp_i]     [ g_i ]
//     [ B_i' C   ] [ds  ] = - [ g_s ],   C = sum_i C_i, g_s = sum_i g_s,i
// so every item eliminates its own 6 x 6 block and what is left is P x P.  Both kernel files run one Levenberg-Marquardt
// trial as item kernel -> solve -> try -> control and, at the result, item kernel -> solve (lam = 0) -> cov_pose.  What
// those kernels have in common exists here once; ArrowCtl, ArrowArgs and the sizes of a record are engine.hpp's.
//   Wide<N>               the thread-private sums of weighted 2 x N row pairs (packed lower J'J, J'r, cost, sum |r|^2)
//                         and their reduction into LDS: one butterfly per 32 sums and wave (wave_sum32), the waves in order
//   damped_chol6          L = chol(A + lam diag(max(A_ii, 1e-12))) with its `ok`: the damped diagonal in front of
//                         small_solve.hpp's cholesky<6>, and the copy to LDS
//   forward_column6       one column of Y = L^-1 B or y = L^-1 g (small_solve.hpp's forward_substitute<6>)
//   arrow_record_entry / arrow_elim_entry   the layout of an item's record and elimination, entry by entry
//   arrow_solve_begin     the solve kernel's bookkeeping on the control block; false: nothing to solve
//   arrow_pose_step       dp = -L^-T (y + Y ds) from an item's elimination
//   arrow_store_trial     what a try kernel stores
//   arrow_control         lm_refine's accept / stop rules (pose_lm.hpp) on the whole problem
//   arrow_result_update, arrow_marginal_store   an item's statistics and its joint marginal L^-T (I + Y S^-1 Y') L^-1
//   arrow_begin           who takes part in the first refinement
// The two factorisations of the reduced system stay apart: chol9 (kernels_calibrate.hip) holds the 9 x 9 matrix in one
// thread's registers, k_rigcal_solve factors up to 48 x 48 in LDS with a barrier per column.  They are different
// algorithms for different sizes, and one body for both would change k_calib_solve's speed.  chol9 is small_solve.hpp's
// cholesky<9> under its own pivot policy (PivotWeighted), like every other register-resident factorisation here.  The
// four-line rule in front of the two factorisations stays written out twice (damping by lam C_jj, a unit row for an
// inactive unknown, the Jacobi scale, the weight S_jj / C_jj): as a function of its own, in any of four shapes, it cost
// k_calib_solve 55 to 58 registers (167 -> 222 .. 225).  So does the back substitution behind chol9: through
// backward_substitute<9> one fused multiply-add of k_calib_solve became an add.
// Every sum has a fixed order and nothing here depends on blockIdx.
#pragma once
#include "engine.hpp"
#include "image_sums.hpp"

namespace vmm {

// When is the undamped S = sum (C_i - Y'Y) singular?  Its entries come out of a cancellation and carry rounding errors
// of a few eps sqrt(C_aa C_bb), C = sum C_i: scaled by diag(C) they are known to about 1e-15, and so are the pivots of
// that scaling (the factorisation runs on the unit-diagonal scaling by diag(S); a pivot of one scaling is the other's
// times S_jj / C_jj).  A pivot within a factor 100 of that noise is taken for the zero of a singular matrix.
constexpr double kMinPivot = 1e-13;

// where the parts of a record and of an elimination begin (engine.hpp: arrow_rec_doubles, arrow_elim_doubles)
__device__ __forceinline__ constexpr int arrow_rec_grad(const int P) { return P * (P + 1) / 2; }
__device__ __forceinline__ constexpr int arrow_rec_diag(const int P) { return P * (P + 1) / 2 + P; }
__device__ __forceinline__ constexpr int arrow_rec_stat(const int P) { return P * (P + 1) / 2 + 2 * P; }   // cost | raw2 | bad | obs | 1
__device__ __forceinline__ constexpr int arrow_elim_Y(const int P, const int row) { return 21 + P * row; }
__device__ __forceinline__ constexpr int arrow_elim_y(const int P) { return 21 + 6 * P; }

// row of packed-lower entry e (tri6 indexing)
__device__ __forceinline__ int packed_row(const int e)
{
    int r = 0;
    while (tri6(r + 1, 0) <= e)
        ++r;
    return r;
}

// thread = item
__device__ __forceinline__ void arrow_begin(const ArrowArgs& w, const vmm_ba_localize_result* res, const int n)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n)
        return;
    const vmm_ba_localize_result r = res[p];
    w.n_in[p] = r.n_inlier_obs;
    w.part[p] = r.status == VMM_BA_LOC_OK && r.n_inlier_obs >= w.min_inliers;
}

// A thread's running sums over weighted 2 x N row pairs: the packed lower triangle of J'J (0 .. kTri - 1), J'r (kTri ..),
// the cost and sum |r|^2.  They live in registers (2 kSums of them), so the loop over a tag's corners around add() stays
// rolled in its caller: four corners in flight at once cost registers the sums need.
template <int N>
struct Wide {
    static constexpr int kTri = N * (N + 1) / 2, kSums = kTri + N + 2, kChunks = (kSums + 31) / 32;
    double acc[kChunks][32];
    __device__ __forceinline__ double& at(const int i) { return acc[i >> 5][i & 31]; }
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int c = 0; c < kChunks; ++c)
#pragma unroll
            for (int k = 0; k < 32; ++k)
                acc[c][k] = 0.0;
    }
    // J and (ru, rv) carry the weight already; s = |r|^2 without it
    __device__ __forceinline__ void add(const double (&J)[2][N], const double ru, const double rv, const double rho0, const double s)
    {
        at(kTri + N) += rho0;
        at(kTri + N + 1) += s;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            at(kTri + i) += J[0][i] * ru + J[1][i] * rv;
#pragma unroll
            for (int k = 0; k <= i; ++k)
                at(tri6(i, k)) += J[0][i] * J[0][k] + J[1][i] * J[1][k];
        }
    }
    // the workgroup's totals into s_tot [kSums]: one butterfly per chunk and wave, then the waves in order through
    // s_red [kImageWaves * 32 * kChunks]; ends with a barrier
    __device__ __forceinline__ void reduce(double* s_red, double* s_tot)
    {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            const double tot = wave_sum32(acc[c], lane);
            s_red[(wave * kChunks + c) * 32 + wave_sum32_index(lane)] = tot;   // lanes 2 m and 2 m + 1 store the same value
        }
        __syncthreads();
        if (tid < kSums) {
            double t = s_red[tid];
#pragma unroll
            for (int w = 1; w < kImageWaves; ++w)
                t += s_red[w * 32 * kChunks + tid];
            s_tot[tid] = t;
        }
        __syncthreads();
    }
};

// One thread: L = chol(A + lam diag(max(A_ii, 1e-12))), as damped_solve damps, into s_L; A packed lower.  false: a pivot was
// not positive or not finite.
__device__ __forceinline__ bool damped_chol6(const double* A, const double lam, double* s_L)
{
    double L[21];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        L[k] = A[k];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double ajj = A[tri6(j, j)];
        L[tri6(j, j)] = ajj + lam * (ajj > 1e-12 ? ajj : 1e-12);
    }
    const bool ok = cholesky<6>(L, L, Packed{}, PivotPositive<true>{});
#pragma unroll
    for (int k = 0; k < 21; ++k)
        s_L[k] = L[k];
    return ok;
}

// One thread: L^-1 b for the column b = (rhs(0) .. rhs(5)), stored at out[ld * i]
template <typename Rhs>
__device__ __forceinline__ void forward_column6(const double* s_L, Rhs&& rhs, double* out, const int ld)
{
    forward_substitute<6>(s_L, Packed{}, rhs, [&](const int i, const double v) { out[ld * i] = v; });
}

// Entry e of an item's record.  c_entry(i, j), i >= j: the item's C; grad(c): its g_s; Y [6][ld]: L^-1 B with y = L^-1 g
// in column P.
template <typename CEntry, typename Grad>
__device__ __forceinline__ double arrow_record_entry(const int e, const int P, CEntry&& c_entry, Grad&& grad, const double* Y,
                                                     const int ld, const double cost, const double raw2, const bool bad,
                                                     const int n_in)
{
    double v;
    if (e < arrow_rec_grad(P)) {   // C - Y'Y, packed lower
        const int i = packed_row(e), j = e - tri6(i, 0);
        v = c_entry(i, j);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            v -= Y[ld * k + i] * Y[ld * k + j];
    } else if (e < arrow_rec_diag(P)) {   // g_s - Y'y
        const int c = e - arrow_rec_grad(P);
        v = grad(c);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            v -= Y[ld * k + c] * Y[ld * k + P];
    } else if (e < arrow_rec_stat(P)) {
        const int c = e - arrow_rec_diag(P);
        v = c_entry(c, c);
    } else {
        const int k = e - arrow_rec_stat(P);
        v = k == 0 ? cost : k == 1 ? raw2 : k == 2 ? (bad ? 1.0 : 0.0) : k == 3 ? (double)n_in : 1.0;
    }
    return v;
}

// Entry e of an item's elimination: L | Y row by row | y
__device__ __forceinline__ double arrow_elim_entry(const int e, const int P, const double* s_L, const double* Y, const int ld)
{
    if (e < 21)
        return s_L[e];
    if (e < arrow_elim_y(P))
        return Y[ld * ((e - 21) / P) + (e - 21) % P];
    return Y[ld * (e - arrow_elim_y(P)) + P];
}

// Thread 0 of a solve kernel, the records summed: st = the sums' cost | raw2 | bad items | inlier observations | items.
// Books them on the control block and decides whether a trial (or, in cov_mode, the covariance) is solved for.
__device__ __forceinline__ bool arrow_solve_begin(ArrowCtl& c, const double* st, const int cov_mode, const double lam)
{
    const double cost = st[0], raw2 = st[1];
    const int n_used = (int)st[4], n_obs_used = (int)st[3];
    c.cost = cost;
    c.raw2 = raw2;
    c.n_used = n_used;
    c.n_obs_used = n_obs_used;
    if (c.first) {
        c.first = 0;
        c.initial_cost = cost;
        c.initial_raw2 = raw2;
        c.initial_n_obs = n_obs_used;
    }
    if (!cov_mode) {
        if (n_used == 0 || !finite_bits(cost) || lam > kLamMax) {
            c.done = 1;
            c.stop = 1;
            return false;
        }
        if (c.trials >= c.max_trials) {
            c.done = 1;
            c.stop = 2;
            return false;
        }
        c.trials += 1;
    }
    return true;
}

// dp = -L^-T (y + Y ds) from an item's elimination; every thread computes it
__device__ __forceinline__ void arrow_pose_step(const double* el, const int P, const double* ds, double (&dp)[6])
{
    double w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = el[arrow_elim_y(P) + k];
        for (int c = 0; c < P; ++c)
            v += el[arrow_elim_Y(P, k) + c] * ds[c];
        w[k] = v;
    }
    backward_substitute<6>(el, Packed{}, [&](const int i) { return -w[i]; }, dp);
}

// thread 0 of a try kernel
__device__ __forceinline__ void arrow_store_trial(const ArrowArgs& w, const int p, const double (&cand)[7], const double cost,
                                                  const double (&dp)[6])
{
#pragma unroll
    for (int k = 0; k < 7; ++k)
        w.cand[7 * (int64_t)p + k] = cand[k];
    w.trial[2 * p] = cost;
    w.trial[2 * p + 1] = max_abs<6>(dp);
}

// lm_refine's decision (pose_lm.hpp) on the whole problem, by one workgroup of kImageThreads.  The step's size is the
// largest tangent component of any pose, folded with the shared unknowns' by shared_step(size so far); on acceptance
// thread 0 books it, the candidate poses are copied over `poses` and thread 0 calls take_shared(), which copies the
// shared candidate (as one block behind the booking, k_calib_control needed a register more than it had).  s_sum, s_max:
// LDS [kImageWaves].
template <typename SharedStep, typename TakeShared>
__device__ __forceinline__ void arrow_control(const ArrowArgs& w, ArrowCtl& c, const int n, double* poses, double* s_sum,
                                              double* s_max, SharedStep&& shared_step, TakeShared&& take_shared)
{
    if (c.done)
        return;
    const int tid = threadIdx.x;
    if (!c.solve_ok) {   // a trial spent on a system that was not positive definite
        if (tid == 0)
            c.lam *= 10.0;
        return;
    }
    double cc = 0.0, sm = 0.0;
    for (int i = tid; i < n; i += kImageThreads) {
        cc += w.trial[2 * i];
        const double s = w.trial[2 * i + 1];
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
    for (int k = 1; k < kImageWaves; ++k) {
        cc += s_sum[k];
        sm = s_max[k] > sm ? s_max[k] : sm;
    }
    sm = shared_step(sm);
    const double cost = c.cost, lam = c.lam;
    const int accepted = c.accepted;
    __syncthreads();   // every thread has read the control block before thread 0 writes it
    if (sm < 1e-14) {
        if (tid == 0) {
            c.done = 1;
            c.stop = 1;
        }
        return;
    }
    if (finite_bits(cc) && cc < cost) {
        if (tid == 0) {
            c.lam = lam * 0.1 > kLamMin ? lam * 0.1 : kLamMin;
            c.accepted = accepted + 1;
        }
        for (int i = tid; i < n; i += kImageThreads)
            if (w.part[i])
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    poses[7 * (int64_t)i + k] = w.cand[7 * (int64_t)i + k];
        if (tid == 0)
            take_shared();
    } else if (tid == 0) {
        if (sm < 1e-10 || cost_at_floor(cost, cc)) {
            c.done = 1;
            c.stop = 1;
        } else {
            c.lam = lam * 10.0;
        }
    }
}

// One thread, at the result: the statistics of item p from its record (stat: the record at arrow_rec_stat)
__device__ __forceinline__ void arrow_result_update(vmm_ba_localize_result* res, const int p, const int n_in, const double* stat)
{
    vmm_ba_localize_result r = res[p];
    r.n_inlier_obs = n_in;
    r.cost = 0.5 * stat[0];
    r.rms_px = sqrt(stat[1] / (4.0 * n_in));
    res[p] = r;
}

// One thread: the joint marginal of an item's pose, cov = W' M W with W = L^-1 (el: the item's elimination) and
// M = I + Y S^-1 Y' (packed lower), mirrored into out [36]; all zero when an entry is not finite.
__device__ __forceinline__ void arrow_marginal_store(const double* el, const double (&M)[21], double* out)
{
    double W[21];
    lower_inverse<6>(el, W);
    // Q = M W (full 6 x 6), cov[r][c] = sum_k W[k][r] Q[k][c]
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

} // namespace vmm
