// k_small_ba (gfx950): a whole bundle adjustment in one workgroup, a batch of them in one launch (vmm_ba_solve_small).
// The grid is the batch, workgroup b solves problem b from the first evaluation to the policy's own stop; nothing is
// handed between workgroups and nothing depends on blockIdx but the problem and its slice of the scratch.
//
// The objective is vmm_ba_solve's (eval_corner and huber of geom.hpp; a constant pose has zero columns) and so is the
// trust-region policy, stage for stage as k_control (kernels_lm.hip) and the oracle's vo_solve state it.  Per pass:
//   evaluation   one thread per observation: 4 corners, both 2 x 6 Jacobians, the Huber weight; its shares of both
//                poses' J^T J (packed lower) and J^T r, W = J_e^T J_f and the cost go to the problem's scratch; one thread
//                per (pose, entry) then adds the shares in the order of the pose's observation list
//   elimination  one thread per eliminated pose: the damped, scaled 6 x 6 block and its Cholesky factor (small_solve.hpp),
//                z = L^-1 g; one thread per (observation, column): Y = L^-1 (s_e W s_f)
//   reduced      one thread per entry of the lower block triangle of S in LDS: the kept pose's own block, minus
//                Y_a^T Y_b over the block's list of observation pairs that share an eliminated pose (made on the host),
//                in ascending order of the eliminated pose
//   factor       blocked by 6 in LDS: thread 0 factors the diagonal block, one thread per row solves the panel, one thread
//                per entry updates the rest; the right-hand side travels as one more row, so the forward solve is done
//                when the factor is; then the backward solve, block by block
//   step         one thread per eliminated pose back-substitutes; one thread per pose forms Plus(x, delta) and its terms
//                of the model cost and the norms; the cross term d_e^T W d_f is summed over the observations
//   control      thread 0 runs the policy on a block in LDS; all threads read its decisions behind a barrier
// Every sum has a fixed order (strided partial sums, one butterfly per wave, the four wave totals added in wave order), so a
// problem gives the same bits alone, in any batch, at any position and from run to run.  No floating-point atomics.
#include <float.h>

#include "pose_lm.hpp"
#include "small_ba.hpp"
#include "small_solve.hpp"

namespace vmm {

namespace {

constexpr int kWaves = kSmallThreads / 64;

struct SmallCtl {
    double radius, decrease_factor, x_cost, x_norm, initial_cost;
    int reuse_diagonal, reuse_now, num_invalid, stop, accept, valid, termination;
    int records, num_successful, num_unsuccessful, num_lm_iterations, num_jac_evals, num_cost_evals;
    vmm_ba_iteration cur;
};

// one problem: the batch arrays moved to its first pose / observation
struct Prob {
    Intrinsics K;
    int n_cams, n_tags, n_pose, n_obs, n_e, n_f, e_base, f_base;
    double *x, *cand;
    const double* wh;
    const uint8_t* is_const;
    double* Hg;
    int64_t hg_stride;
    double *scale, *diag, *D2, *delta, *ysol, *Le, *ze;
    int32_t* active;
    const int32_t *obs_e, *obs_f;
    const double* px;
    double* W;
    int64_t w_stride;
    double *Y, *opart;
    const int32_t *e_start, *f_start, *f_list, *pair_start, *pairs;
};

__device__ __forceinline__ Prob make_prob(const SmallArgs& a, const SmallDesc& d)
{
    Prob P;
    P.K = d.K;
    P.n_cams = d.n_cams;
    P.n_tags = d.n_tags;
    P.n_pose = d.n_cams + d.n_tags;
    P.n_obs = d.n_obs;
    P.n_e = d.n_e;
    P.n_f = d.n_f;
    P.e_base = d.elim_cams ? 0 : d.n_cams;
    P.f_base = d.elim_cams ? d.n_cams : 0;
    const int64_t po = d.pose_off, oo = d.obs_off;
    P.x = a.x + 7 * po;
    P.cand = a.cand + 7 * po;
    P.wh = a.wh + 2 * po;
    P.is_const = a.is_const + po;
    P.Hg = a.Hg + kSmallPosePart * po;
    P.hg_stride = a.hg_stride;
    P.scale = a.scale + 6 * po;
    P.diag = a.diag + 6 * po;
    P.D2 = a.D2 + 6 * po;
    P.delta = a.delta + 6 * po;
    P.ysol = a.ysol + 6 * po;
    P.Le = a.Le + 21 * po;
    P.ze = a.ze + 6 * po;
    P.active = a.active + po;
    P.obs_e = a.obs_e + oo;
    P.obs_f = a.obs_f + oo;
    P.px = a.px + 8 * oo;
    P.W = a.W + 36 * oo;
    P.w_stride = a.w_stride;
    P.Y = a.Y + 36 * oo;
    P.opart = a.opart + kSmallObsPart * oo;
    P.e_start = a.e_start + d.e_start_off;
    P.f_start = a.f_start + d.f_start_off;
    P.f_list = a.f_list + oo;
    P.pair_start = a.pair_start + d.pair_start_off;
    P.pairs = a.pairs + 2 * d.pair_off;
    return P;
}

// Sums (or maxima) over the workgroup with a fixed tree; every thread ends with the totals.  sh: [kWaves][NV].
template <int NV, bool MAX>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double* sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        if (MAX) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1)
                v[k] = fmax(v[k], __shfl_xor(v[k], m, 64));
        } else {
            v[k] = wave_sum(v[k]);
        }
    }
    __syncthreads();   // the readers of the previous reduction are done with sh
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            sh[wave * NV + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double r = sh[k];
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            r = MAX ? fmax(r, sh[w * NV + k]) : r + sh[w * NV + k];
        v[k] = r;
    }
}

// One thread per observation: everything it contributes at `poses`, to the scratch.
template <bool ELIM_CAMS>
__device__ __forceinline__ void eval_observations(const Prob& P, const double* __restrict__ poses, double* __restrict__ Wb,
                                                  const bool robust, const double huber_a)
{
    for (int i = (int)threadIdx.x; i < P.n_obs; i += kSmallThreads) {
        const int pe = P.e_base + P.obs_e[i], pf = P.f_base + P.obs_f[i];
        const int pc = ELIM_CAMS ? pe : pf, pt = ELIM_CAMS ? pf : pe;
        Rigid cam, tag;
        load_rigid<true>(poses + 7 * (int64_t)pc, cam);
        load_rigid<true>(poses + 7 * (int64_t)pt, tag);
        const double hw = 0.5 * P.wh[2 * (int64_t)pt], hh = 0.5 * P.wh[2 * (int64_t)pt + 1];
        // a constant pose has zero columns: its own block, its gradient and W
        const double me = P.is_const[pe] ? 0.0 : 1.0, mf = P.is_const[pf] ? 0.0 : 1.0;
        const double* __restrict__ px = P.px + 8 * (int64_t)i;
        double He[21], Hf[21], ge[6], gf[6], Wm[36], cost = 0.0;
#pragma unroll
        for (int k = 0; k < 21; ++k)
            He[k] = Hf[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            ge[k] = gf[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 36; ++k)
            Wm[k] = 0.0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            CornerEval ev;
            eval_corner<true, true>(P.K, cam, tag, corner_sx(k) * hw, corner_sy(k) * hh, px[2 * k], px[2 * k + 1], ev);
            double rho0, wgt;
            huber(robust, huber_a, ev.ru * ev.ru + ev.rv * ev.rv, rho0, wgt);
            cost += 0.5 * rho0;
            // the corrector: rows of the Jacobian and the residual scaled by sqrt(rho')
            const double we = wgt * me, wf = wgt * mf;
            const double r0 = wgt * ev.ru, r1 = wgt * ev.rv;
            double je[2][6], jf[2][6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                je[0][a] = we * (ELIM_CAMS ? ev.jc[0][a] : ev.jt[0][a]);
                je[1][a] = we * (ELIM_CAMS ? ev.jc[1][a] : ev.jt[1][a]);
                jf[0][a] = wf * (ELIM_CAMS ? ev.jt[0][a] : ev.jc[0][a]);
                jf[1][a] = wf * (ELIM_CAMS ? ev.jt[1][a] : ev.jc[1][a]);
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                ge[a] += je[0][a] * r0 + je[1][a] * r1;
                gf[a] += jf[0][a] * r0 + jf[1][a] * r1;
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    He[tri6(a, b)] += je[0][a] * je[0][b] + je[1][a] * je[1][b];
                    Hf[tri6(a, b)] += jf[0][a] * jf[0][b] + jf[1][a] * jf[1][b];
                }
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    Wm[6 * a + q] += je[0][a] * jf[0][q] + je[1][a] * jf[1][q];
            }
        }
        double* __restrict__ op = P.opart + kSmallObsPart * (int64_t)i;
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            op[k] = He[k];
            op[kSmallPosePart + k] = Hf[k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            op[21 + k] = ge[k];
            op[kSmallPosePart + 21 + k] = gf[k];
        }
        op[2 * kSmallPosePart] = cost;
        double* __restrict__ w = Wb + 36 * (int64_t)i;
#pragma unroll
        for (int k = 0; k < 36; ++k)
            w[k] = Wm[k];
    }
}

// The evaluation at `poses` into copy `buf` of the blocks; returns the cost (every thread).  Contains barriers.
__device__ __forceinline__ double evaluate(const Prob& P, const bool elim_cams, const double* __restrict__ poses,
                                           const int buf, const vmm_ba_options& o, double* sh)
{
    double* const Wb = P.W + buf * P.w_stride;
    if (elim_cams)
        eval_observations<true>(P, poses, Wb, o.robustify != 0, o.huber_a);
    else
        eval_observations<false>(P, poses, Wb, o.robustify != 0, o.huber_a);
    __syncthreads();
    // per pose, in the order of its observation list
    double* __restrict__ Hgb = P.Hg + buf * P.hg_stride;
    for (int64_t t = threadIdx.x; t < (int64_t)kSmallPosePart * P.n_pose; t += kSmallThreads) {
        const int p = (int)(t / kSmallPosePart), k = (int)(t - (int64_t)kSmallPosePart * p);
        double s = 0.0;
        if (p >= P.e_base && p < P.e_base + P.n_e) {
            const int e = p - P.e_base;
            for (int i = P.e_start[e]; i < P.e_start[e + 1]; ++i)
                s += P.opart[kSmallObsPart * (int64_t)i + k];
        } else {
            const int f = p - P.f_base;
            for (int j = P.f_start[f]; j < P.f_start[f + 1]; ++j)
                s += P.opart[kSmallObsPart * (int64_t)P.f_list[j] + kSmallPosePart + k];
        }
        Hgb[t] = s;
    }
    double c[1] = { 0.0 };
    for (int i = (int)threadIdx.x; i < P.n_obs; i += kSmallThreads)
        c[0] += P.opart[kSmallObsPart * (int64_t)i + 2 * kSmallPosePart];
    block_reduce<1, false>(c, sh);   // its barriers also publish Hgb
    return c[0];
}

// |Plus(x, -g) - x|_inf and |x|^2 over the active poses at `poses` with the blocks of copy `buf` (every thread)
__device__ __forceinline__ void gradient_and_norm(const Prob& P, const double* __restrict__ poses, const int buf, double* sh,
                                                  double& gmax, double& xnorm2)
{
    const double* __restrict__ Hgb = P.Hg + buf * P.hg_stride;
    double m[1] = { 0.0 }, n[1] = { 0.0 };
    for (int p = (int)threadIdx.x; p < P.n_pose; p += kSmallThreads) {
        if (!P.active[p])
            continue;
        const double* x = poses + 7 * (int64_t)p;
        double ng[6], xp[7];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            ng[k] = -Hgb[kSmallPosePart * (int64_t)p + 21 + k];
        pose_plus(x, ng, xp);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            m[0] = fmax(m[0], fabs(x[k] - xp[k]));
            n[0] += x[k] * x[k];
        }
    }
    block_reduce<1, true>(m, sh);
    block_reduce<1, false>(n, sh);
    gmax = m[0];
    xnorm2 = n[0];
}

__device__ __forceinline__ int blk(int fa, int fb) { return 36 * (fa * (fa + 1) / 2 + fb); }

} // namespace

__global__ __launch_bounds__(kSmallThreads) void k_small_ba(const SmallArgs a)
{
    __shared__ double S[36 * kSmallBlocks];   // the lower block triangle of the reduced system, block (fa, fb) row-major
    __shared__ double sb[6 * kSmallMaxKept];  // its right-hand side, then the solution
    __shared__ double sh[kWaves * 8];
    __shared__ uint16_t tab[kSmallBlocks];    // block index -> (fa << 8) | fb
    __shared__ SmallCtl ctl;
    __shared__ int s_fail;

    const int tid = (int)threadIdx.x;
    const SmallDesc& d = a.desc[blockIdx.x];
    const Prob P = make_prob(a, d);
    const bool elim_cams = d.elim_cams != 0;
    const vmm_ba_options& o = a.o;
    vmm_ba_iteration* const trace = a.trace + d.trace_off;
    const int trace_capacity = d.trace_capacity;
    const int n_f = P.n_f, n_e = P.n_e;

    for (int fa = tid; fa < n_f; fa += kSmallThreads)
        for (int fb = 0; fb <= fa; ++fb)
            tab[fa * (fa + 1) / 2 + fb] = (uint16_t)((fa << 8) | fb);

    // One evaluation per turn of the outer loop: at x itself in iteration zero, at the candidate afterwards, into the
    // copy of the blocks that does not belong to x.  `which` (the copy that belongs to x) and `first` are the same in
    // every thread: they follow decisions read from LDS behind a barrier.
    int which = 1;
    bool first = true;
    double red[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };   // d.g, d^T H d, |x - x+|^2, |x+|^2, cross term of the last step
    for (;;) {
        const double* const at = first ? P.x : P.cand;
        const double ccost = evaluate(P, elim_cams, at, which ^ 1, o, sh);
        if (first) {
            // iteration zero: activity and Jacobi scaling
            const double* Hg0 = P.Hg + (which ^ 1) * P.hg_stride;
            for (int p = tid; p < P.n_pose; p += kSmallThreads) {
                const double* Hp = Hg0 + kSmallPosePart * (int64_t)p;
                // blocks with zero Jacobian columns (constant poses, poses without observations) are not part of the program
                P.active[p] = (Hp[tri6(0, 0)] + Hp[tri6(1, 1)] + Hp[tri6(2, 2)]) > 0.0 ? 1 : 0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    P.scale[6 * (int64_t)p + k] = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(Hp[tri6(k, k)])) : 1.0;
            }
            __syncthreads();
        }
        double gm, xn;
        gradient_and_norm(P, at, which ^ 1, sh, gm, xn);
        if (tid == 0 && first) {
            SmallCtl& c = ctl;
            c.radius = o.initial_trust_region_radius;
            c.decrease_factor = 2.0;
            c.x_cost = ccost;
            c.initial_cost = ccost;
            c.x_norm = sqrt(xn);
            c.reuse_diagonal = 0;
            c.reuse_now = 0;
            c.num_invalid = 0;
            c.stop = 0;
            c.accept = 1;   // the evaluation at x: its blocks are the blocks at x
            c.valid = 0;
            c.termination = VMM_BA_NO_CONVERGENCE;
            c.records = c.num_successful = c.num_unsuccessful = c.num_lm_iterations = c.num_cost_evals = 0;
            c.num_jac_evals = 1;
            vmm_ba_iteration z;
            z.iteration = 0;
            z.step_is_valid = 1;
            z.step_is_successful = 1;
            z.reserved = 0;
            z.cost = ccost;
            z.cost_change = 0.0;
            z.gradient_max_norm = gm;
            z.step_norm = 0.0;
            z.relative_decrease = 0.0;
            z.trust_region_radius = 0.0;
            z.model_cost_change = 0.0;
            c.cur = z;
            if (!finite_bits(ccost)) {
                c.stop = 1;
                c.termination = VMM_BA_FAILURE;
            }
        }
        if (tid == 0 && !first) {
            SmallCtl& c = ctl;
            double cand = ccost;
            c.num_cost_evals++;
            if (!finite_bits(cand))
                cand = DBL_MAX;
            const double step_norm = sqrt(red[2]);
            c.cur.step_norm = step_norm;
            const double x_cost = c.x_cost;
            const double cost_change = x_cost - cand;
            if (step_norm <= o.parameter_tolerance * (c.x_norm + o.parameter_tolerance)) {
                c.stop = 1;   // ParameterToleranceReached: return without pushing this record
                c.termination = VMM_BA_CONVERGENCE;
            } else if (fabs(cost_change) <= o.function_tolerance * x_cost) {
                c.cur.cost_change = cost_change;
                c.stop = 1;   // FunctionToleranceReached
                c.termination = VMM_BA_CONVERGENCE;
            } else {
                c.cur.cost_change = cost_change;
                const double rd = (cand >= DBL_MAX) ? -DBL_MAX : cost_change / c.cur.model_cost_change;
                c.cur.relative_decrease = rd;
                if (rd > o.min_relative_decrease) {
                    // HandleSuccessfulStep, LevenbergMarquardtStrategy::StepAccepted
                    c.accept = 1;
                    const double q = 2.0 * rd - 1.0;
                    double den = 1.0 - q * q * q;
                    den = den < 1.0 / 3.0 ? 1.0 / 3.0 : den;
                    const double r = c.radius / den;
                    c.radius = r > o.max_trust_region_radius ? o.max_trust_region_radius : r;
                    c.decrease_factor = 2.0;
                    c.reuse_diagonal = 0;
                    c.x_norm = sqrt(xn);
                    c.x_cost = ccost;
                    c.num_jac_evals++;
                    c.cur.step_is_successful = 1;
                    c.cur.cost = ccost;
                    c.cur.gradient_max_norm = gm;
                } else {
                    // HandleUnsuccessfulStep, StepRejected
                    c.cur.step_is_successful = 0;
                    c.cur.cost = cand;
                    c.radius = c.radius / c.decrease_factor;
                    c.decrease_factor *= 2.0;
                    c.reuse_diagonal = 1;
                }
            }
        }
        __syncthreads();
        if (ctl.accept) {
            which ^= 1;   // the blocks evaluated at the candidate become the blocks at x
            if (!first)
                for (int64_t i = tid; i < 7 * (int64_t)P.n_pose; i += kSmallThreads)
                    P.x[i] = P.cand[i];
        }
        first = false;
        __syncthreads();
        // ---- passes of the trust-region loop until a step is valid (its candidate is evaluated above) or the loop ends ----
        bool stopped = false;
        for (;;) {
            // ---- FinalizeIterationAndCheckIfMinimizerCanContinue ----
            if (tid == 0 && !ctl.stop) {
                SmallCtl& c = ctl;
                vmm_ba_iteration cur = c.cur;
                cur.trust_region_radius = c.radius;
                if (cur.step_is_successful)
                    c.num_successful++;
                else
                    c.num_unsuccessful++;
                if (c.records < trace_capacity)
                    trace[c.records] = cur;
                c.records++;
                int stop = 0;
                if (cur.iteration >= o.max_num_iterations) {
                    stop = 1;
                    c.termination = VMM_BA_NO_CONVERGENCE;
                } else if (cur.step_is_successful && cur.gradient_max_norm <= o.gradient_tolerance) {
                    stop = 1;
                    c.termination = VMM_BA_CONVERGENCE;
                } else if (c.radius <= o.min_trust_region_radius) {
                    stop = 1;
                    c.termination = VMM_BA_CONVERGENCE;
                }
                c.stop = stop;
                if (!stop) {
                    vmm_ba_iteration z;
                    z.iteration = cur.iteration + 1;
                    z.step_is_valid = 0;
                    z.step_is_successful = 0;
                    z.reserved = 0;
                    z.cost = c.x_cost;
                    z.cost_change = 0.0;
                    z.gradient_max_norm = cur.gradient_max_norm;   // carried until the next successful step
                    z.step_norm = 0.0;
                    z.relative_decrease = 0.0;
                    z.trust_region_radius = 0.0;
                    z.model_cost_change = 0.0;
                    c.cur = z;
                    c.num_lm_iterations++;
                    c.reuse_now = c.reuse_diagonal;
                    c.reuse_diagonal = 1;
                }
                s_fail = 0;
            }
            __syncthreads();
            if (ctl.stop) {
                stopped = true;
                break;
            }
            const double* __restrict__ Hx = P.Hg + which * P.hg_stride;   // the blocks at x
            const double* __restrict__ Wx = P.W + which * P.w_stride;

            // ---- LevenbergMarquardtStrategy::ComputeStep: the LM diagonal ----
            {
                const bool reuse = ctl.reuse_now != 0;
                const double radius = ctl.radius;
                for (int64_t q = tid; q < 6 * (int64_t)P.n_pose; q += kSmallThreads) {
                    double dg;
                    if (!reuse) {
                        const int64_t p = q / 6;
                        const int k = (int)(q - 6 * p);
                        const double sc = P.scale[q];
                        dg = sc * sc * Hx[kSmallPosePart * p + tri6(k, k)];   // squared column norm of the scaled Jacobian
                        dg = fmin(fmax(dg, o.min_lm_diagonal), o.max_lm_diagonal);
                        P.diag[q] = dg;
                    } else {
                        dg = P.diag[q];
                    }
                    const double lm = sqrt(dg / radius);   // lm_diagonal_ = sqrt(diagonal_ / radius_)
                    P.D2[q] = lm * lm;
                }
            }
            __syncthreads();

            // ---- elimination: the damped block of every eliminated pose, its factor, z = L^-1 g ----
            for (int e = tid; e < n_e; e += kSmallThreads) {
                const int64_t p = P.e_base + e;
                if (!P.active[p])
                    continue;
                const double* Hp = Hx + kSmallPosePart * p;
                const double* s = P.scale + 6 * p;
                double M[21];
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j)
                        M[tri6(i, j)] = s[i] * s[j] * Hp[tri6(i, j)] + (i == j ? P.D2[6 * p + i] : 0.0);
                if (!cholesky<6>(M, M, Packed{}, PivotPositive<true>{}))
                    s_fail = 1;
                forward_substitute<6>(M, Packed{}, [&](const int i) { return s[i] * Hp[21 + i]; },
                                      [&](const int i, const double v) { P.ze[6 * p + i] = v; });
#pragma unroll
                for (int k = 0; k < 21; ++k)
                    P.Le[21 * p + k] = M[k];
            }
            __syncthreads();
            if (!s_fail) {
                // Y = L_e^-1 (s_e W s_f), a column per thread
                for (int64_t t = tid; t < 6 * (int64_t)P.n_obs; t += kSmallThreads) {
                    const int64_t i = t / 6;
                    const int q = (int)(t - 6 * i);
                    const int64_t pe = P.e_base + P.obs_e[i], pf = P.f_base + P.obs_f[i];
                    double* __restrict__ Yi = P.Y + 36 * i;
                    if (!P.active[pe] || !P.active[pf]) {
#pragma unroll
                        for (int r = 0; r < 6; ++r)
                            Yi[6 * r + q] = 0.0;
                        continue;
                    }
                    const double* L = P.Le + 21 * pe;
                    const double* se = P.scale + 6 * pe;
                    const double sf = P.scale[6 * pf + q];
                    const double* Wi = Wx + 36 * i;
                    forward_substitute<6>(L, Packed{}, [&](const int r) { return se[r] * Wi[6 * r + q] * sf; },
                                          [&](const int r, const double v) { Yi[6 * r + q] = v; });
                }
                __syncthreads();
                // ---- the reduced system: S = (s_f H_f s_f + D2_f) - sum_e Y^T Y, b = s_f g_f - sum_e Y^T z ----
                const int nblk = n_f * (n_f + 1) / 2;
                for (int t = tid; t < 36 * nblk; t += kSmallThreads) {
                    const int u = t / 36, w = t - 36 * u;
                    const int fa = tab[u] >> 8, fb = tab[u] & 255;
                    const int r = w / 6, q = w - 6 * r;
                    double acc = 0.0;
                    if (fa == fb) {
                        const int64_t p = P.f_base + fa;
                        if (P.active[p]) {
                            const int hi = r > q ? r : q, lo = r > q ? q : r;
                            acc = P.scale[6 * p + r] * P.scale[6 * p + q] * Hx[kSmallPosePart * p + tri6(hi, lo)]
                                + (r == q ? P.D2[6 * p + r] : 0.0);
                        } else {
                            acc = r == q ? 1.0 : 0.0;   // outside the program: unit diagonal, zero step
                        }
                    }
                    // the block products of the pairs of observations that share an eliminated pose, in its order
                    const double* Yr = P.Y + r;
                    const double* Yq = P.Y + q;
                    for (int j = P.pair_start[u]; j < P.pair_start[u + 1]; ++j) {
                        const double* Ya = Yr + 36 * (int64_t)P.pairs[2 * (int64_t)j];
                        const double* Yb = Yq + 36 * (int64_t)P.pairs[2 * (int64_t)j + 1];
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m)
                            s += Ya[6 * m] * Yb[6 * m];
                        acc -= s;
                    }
                    S[t] = acc;
                }
                for (int t = tid; t < 6 * n_f; t += kSmallThreads) {
                    const int f = t / 6, r = t - 6 * f;
                    const int64_t p = P.f_base + f;
                    double acc = P.active[p] ? P.scale[6 * p + r] * Hx[kSmallPosePart * p + 21 + r] : 0.0;
                    for (int j = P.f_start[f]; j < P.f_start[f + 1]; ++j) {
                        const int i = P.f_list[j];
                        const double* Yi = P.Y + 36 * (int64_t)i + r;
                        const double* z = P.ze + 6 * (int64_t)(P.e_base + P.obs_e[i]);
                        if (!P.active[P.e_base + P.obs_e[i]])
                            continue;
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m)
                            s += Yi[6 * m] * z[m];
                        acc -= s;
                    }
                    sb[t] = acc;
                }
                __syncthreads();
                // ---- Cholesky blocked by 6, the right-hand side as one more row: sb ends as L^-1 b ----
                for (int k = 0; k < n_f; ++k) {
                    double* const Dk = S + blk(k, k);
                    if (tid == 0) {
                        if (!cholesky<6>(Dk, Dk, RowMajor<6>{}, PivotPositive<true>{}))
                            s_fail = 1;
                    }
                    __syncthreads();
                    const int nrows = 6 * (n_f - k - 1);
                    for (int r = tid; r <= nrows; r += kSmallThreads) {
                        double* const X = r < nrows ? S + blk(k + 1 + r / 6, k) + 6 * (r % 6) : sb + 6 * k;
                        forward_substitute<6>(Dk, RowMajor<6>{}, [&](const int i) { return X[i]; },
                                              [&](const int i, const double v) { X[i] = v; });
                    }
                    __syncthreads();
                    const int u0 = (k + 1) * (k + 2) / 2;
                    for (int t = tid; t < 36 * (nblk - u0); t += kSmallThreads) {
                        const int u = u0 + t / 36, w = t % 36;
                        const int fa = tab[u] >> 8, fb = tab[u] & 255;
                        if (fb <= k)
                            continue;
                        const int r = w / 6, q = w - 6 * r;
                        const double* La = S + blk(fa, k) + 6 * r;
                        const double* Lb = S + blk(fb, k) + 6 * q;
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m)
                            s += La[m] * Lb[m];
                        S[36 * u + w] -= s;
                    }
                    for (int t = tid; t < nrows; t += kSmallThreads) {
                        const int fb = k + 1 + t / 6, q = t % 6;
                        const double* Lb = S + blk(fb, k) + 6 * q;
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m)
                            s += sb[6 * k + m] * Lb[m];
                        sb[6 * fb + q] -= s;
                    }
                    __syncthreads();
                }
            }
            if (!s_fail) {
                // ---- L^T y = sb, block by block from the last ----
                for (int k = n_f - 1; k >= 0; --k) {
                    if (tid == 0) {
                        const double* Dk = S + blk(k, k);
                        double xk[6];
                        backward_substitute<6>(Dk, RowMajor<6>{}, [&](const int i) { return sb[6 * k + i]; }, xk);
#pragma unroll
                        for (int i = 0; i < 6; ++i)
                            sb[6 * k + i] = xk[i];
                    }
                    __syncthreads();
                    for (int t = tid; t < 6 * k; t += kSmallThreads) {
                        const int fb = t / 6, q = t - 6 * fb;
                        const double* L = S + blk(k, fb) + q;
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m)
                            s += L[6 * m] * sb[6 * k + m];
                        sb[t] -= s;
                    }
                    __syncthreads();
                }
                // ---- back-substitution of the eliminated poses: y_e = L_e^-T (z_e - sum_f Y_ef y_f) ----
                for (int t = tid; t < 6 * n_f; t += kSmallThreads)
                    P.ysol[6 * (int64_t)P.f_base + t] = sb[t];
                for (int e = tid; e < n_e; e += kSmallThreads) {
                    const int64_t p = P.e_base + e;
                    double v[6];
                    if (!P.active[p]) {
#pragma unroll
                        for (int i = 0; i < 6; ++i)
                            P.ysol[6 * p + i] = 0.0;
                        continue;
                    }
#pragma unroll
                    for (int i = 0; i < 6; ++i)
                        v[i] = P.ze[6 * p + i];
                    for (int i = P.e_start[e]; i < P.e_start[e + 1]; ++i) {
                        const double* Yi = P.Y + 36 * (int64_t)i;
                        const double* yf = sb + 6 * P.obs_f[i];
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            double s = 0.0;
#pragma unroll
                            for (int q = 0; q < 6; ++q)
                                s += Yi[6 * r + q] * yf[q];
                            v[r] -= s;
                        }
                    }
                    const double* L = P.Le + 21 * p;
                    double out[6];
                    backward_substitute<6>(L, Packed{}, [&](const int i) { return v[i]; }, out);
#pragma unroll
                    for (int i = 0; i < 6; ++i)
                        P.ysol[6 * p + i] = out[i];
                }
                __syncthreads();
            }
            // ---- the candidate x+ = Plus(x, delta) and the terms of the model cost and of the norms ----
            red[0] = red[1] = red[2] = red[3] = red[4] = 0.0;
            double bad[1] = { 0.0 };
            if (!s_fail) {
                for (int p = tid; p < P.n_pose; p += kSmallThreads) {
                    const double* x = P.x + 7 * (int64_t)p;
                    double* cnd = P.cand + 7 * (int64_t)p;
                    if (!P.active[p]) {   // outside the program: the pose keeps its bits
#pragma unroll
                        for (int k = 0; k < 7; ++k)
                            cnd[k] = x[k];
#pragma unroll
                        for (int k = 0; k < 6; ++k)
                            P.delta[6 * (int64_t)p + k] = 0.0;
                        continue;
                    }
                    double dl[6], out[7];
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        dl[k] = -P.ysol[6 * (int64_t)p + k] * P.scale[6 * (int64_t)p + k];
                        P.delta[6 * (int64_t)p + k] = dl[k];
                        if (!finite_bits(dl[k]))
                            bad[0] = 1.0;
                    }
                    pose_plus(x, dl, out);
#pragma unroll
                    for (int k = 0; k < 7; ++k) {
                        cnd[k] = out[k];
                        const double df = x[k] - out[k];
                        red[2] += df * df;
                        red[3] += out[k] * out[k];
                    }
                    const double* Hp = Hx + kSmallPosePart * (int64_t)p;
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        red[0] += dl[i] * Hp[21 + i];
                        double r = 0.0;
#pragma unroll
                        for (int j = 0; j < 6; ++j)
                            r += Hp[i > j ? tri6(i, j) : tri6(j, i)] * dl[j];
                        red[1] += dl[i] * r;
                    }
                }
                __syncthreads();
                for (int i = tid; i < P.n_obs; i += kSmallThreads) {
                    const double* de = P.delta + 6 * (int64_t)(P.e_base + P.obs_e[i]);
                    const double* df = P.delta + 6 * (int64_t)(P.f_base + P.obs_f[i]);
                    const double* Wi = Wx + 36 * (int64_t)i;
                    double s = 0.0;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        double v = 0.0;
#pragma unroll
                        for (int q = 0; q < 6; ++q)
                            v += Wi[6 * r + q] * df[q];
                        s += de[r] * v;
                    }
                    red[4] += s;
                }
            }
            block_reduce<5, false>(red, sh);
            block_reduce<1, true>(bad, sh);
            // ---- ComputeTrustRegionStep: the model cost, the validity of the step ----
            if (tid == 0) {
                SmallCtl& c = ctl;
                const bool lin_fail = s_fail != 0 || bad[0] != 0.0;
                // model_cost_change = -(J d)^T (r + J d / 2) = -d^T g - 1/2 d^T H d   (unscaled coordinates)
                const double mcc = lin_fail ? 0.0 : -red[0] - 0.5 * (red[1] + 2.0 * red[4]);
                c.cur.model_cost_change = mcc;
                const bool valid = !lin_fail && (mcc > 0.0);
                c.cur.step_is_valid = valid ? 1 : 0;
                c.valid = valid ? 1 : 0;
                c.accept = 0;
                if (!valid) {
                    // HandleInvalidStep
                    c.num_invalid++;
                    if (c.num_invalid >= o.max_num_consecutive_invalid_steps) {
                        c.stop = 1;
                        c.termination = VMM_BA_FAILURE;
                    } else {
                        c.radius = c.radius / c.decrease_factor;
                        c.decrease_factor *= 2.0;
                        c.reuse_diagonal = 1;
                        c.cur.cost = c.x_cost;
                        c.cur.step_is_successful = 0;
                    }
                } else {
                    c.num_invalid = 0;
                }
            }
            __syncthreads();
            if (ctl.valid)
                break;   // an invalid step goes round: the stop (if any) is seen at the head of the loop
        }
        if (stopped)
            break;
    }

    if (tid == 0) {
        const SmallCtl& c = ctl;
        SmallResult r;
        r.termination = c.termination;
        r.records = c.records;
        r.num_successful = c.num_successful;
        r.num_unsuccessful = c.num_unsuccessful;
        r.num_lm_iterations = c.num_lm_iterations;
        r.num_jac_evals = c.num_jac_evals;
        r.num_cost_evals = c.num_cost_evals;
        r.reserved = 0;
        r.initial_cost = c.initial_cost;
        r.final_cost = c.x_cost;
        a.res[blockIdx.x] = r;
    }
}

void launch_small_ba(hipStream_t st, int n_problems, const SmallArgs& a)
{
    hipLaunchKernelGGL(k_small_ba, dim3((unsigned)n_problems), dim3(kSmallThreads), 0, st, a);
}

int preload_small_kernels()
{
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_small_ba)) != hipSuccess;
}

} // namespace vmm
