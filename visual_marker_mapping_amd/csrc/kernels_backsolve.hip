// Back-substitution L^T y = w of the reduced system (gfx950): the one-launch chain (dense and tree-ordered factors) and the
// per-block fallback k_backsolve_step.  (The three paths and the matrix layout: kernels_chol.hip.)
#include "chol_common.hpp"

namespace vmm {

// One step of L^T y = w (w lives in row n_pad of S).  Launched for kb = n_blk-1 .. 0 with kb+1
// workgroups of 256 threads: workgroup m first applies y_{kb+1} to w_m (64x64 transposed GEMV split
// over the four waves), then workgroup kb solves its diagonal block four unknowns per round.
__global__ __launch_bounds__(256) void k_backsolve_step(const LmCtl* ctl, double* __restrict__ S, int ld,
                                                        int n_pad, int n_blk, int kb, double* __restrict__ y,
                                                        const double* __restrict__ dinv,
                                                        const double* __restrict__ Ld)
{
    if (ctl->done || ctl->lin_fail)
        return;
    __shared__ double red[4][64];
    __shared__ double L[64 * kLd];
    __shared__ double ws[64];
    __shared__ double di[64];
    const int m = blockIdx.x;
    const int tid = threadIdx.x;
    const int c = tid & 63, part = tid >> 6;
    double* w = S + (int64_t)n_pad * ld;
    double wc = 0.0;
    if (kb + 1 < n_blk) {
        const int R0 = (kb + 1) * kNB + part * 16;
        const double* Lb = S + (int64_t)R0 * ld + m * kNB + c;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc += Lb[(int64_t)r * ld] * y[R0 + r];
        red[part][c] = acc;
    }
    if (m == kb) {
        // stage the diagonal block while the partial sums settle
        const int K0 = kb * kNB;
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, cc = idx & 63;
            L[r * kLd + cc] = (cc <= r) ? Ld[(int64_t)kb * 4096 + r * 64 + cc] : 0.0;
        }
        if (tid < 64)
            di[tid] = dinv[K0 + tid];
    }
    __syncthreads();
    if (part == 0) {
        wc = w[m * kNB + c];
        if (kb + 1 < n_blk) {
            wc -= (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
            w[m * kNB + c] = wc;
        }
    }
    if (m != kb)
        return;
    // single wave from here on (part == 0); other waves only keep the barriers company
    double yj = 0.0;
    for (int j0 = 60; j0 >= 0; j0 -= 4) {
        if (part == 0)
            ws[c] = wc;
        __syncthreads();
        if (part == 0) {
            // L4^T v = w4 with L4 the lower 4x4 pivot block at (j0, j0)
            const double* D = L + j0 * kLd + j0;
            const double v3 = ws[j0 + 3] * di[j0 + 3];
            const double v2 = (ws[j0 + 2] - D[3 * kLd + 2] * v3) * di[j0 + 2];
            const double v1 = (ws[j0 + 1] - D[2 * kLd + 1] * v2 - D[3 * kLd + 1] * v3) * di[j0 + 1];
            const double v0 = (ws[j0] - D[kLd] * v1 - D[2 * kLd] * v2 - D[3 * kLd] * v3) * di[j0];
            if (c >= j0 && c < j0 + 4)
                yj = (c == j0) ? v0 : (c == j0 + 1 ? v1 : (c == j0 + 2 ? v2 : v3));
            if (c < j0)
                wc -= L[j0 * kLd + c] * v0 + L[(j0 + 1) * kLd + c] * v1 + L[(j0 + 2) * kLd + c] * v2
                    + L[(j0 + 3) * kLd + c] * v3;
        }
        __syncthreads();
    }
    if (part == 0)
        y[kb * kNB + c] = yj;
}

// Whole back-substitution L^T y = w in ONE launch: workgroup p owns block m = n_blk-1-p and depends on
// the workgroups before it (dispatched earlier), which publish their 64 unknowns as self-validating
// granules (cdna_hip_programming.md Guideline 16, R2: "the data IS the flag"): every double travels as two
// 8-byte {tag = epoch, 32 value bits} words written by ONE aligned agent-scope (sc1) store each; one wave
// of the consumer re-reads its 128 granules with sc1 loads until every tag carries this solve's epoch and
// hands the values to the other waves through LDS.  One L2 round trip per hop instead of two (flag, then
// payload), no drain + flag store on the producer side; the kernel boundaries of the per-block version disappear.
//
// What a hop costs (tools/gpu_chain_stamps.sh): ~0.45 us from a block's publication to its successor seeing it, and
// -- before this form -- ~0.95 us of work behind it: the product with L(m+1,m)^T, a reduction over the four waves,
// the product with the inverse of the diagonal block, another reduction (four barriers).  Only ONE product has to
// wait for y_{m+1}:
//     y_m = Linv_m^T (w_m - sum_{j>m+1} L(j,m)^T y_j)  -  (L(m+1,m) Linv_m)^T y_{m+1}  =  u_m - B_m^T y_{m+1},
// u_m is finished one hop earlier and B_m (a 64x64x64 product) while the workgroup waits for the chain to reach it.
// (Two blocks per workgroup, 10 hops instead of 19, was built first and changed nothing: the work, not the hand-off,
// was the larger part of a hop.)
// Every spin is bounded: a workgroup that gives up raises LmCtl::sync_timeout (NOT lin_fail: a stalled workgroup is
// not an indefinite matrix) and pauses the loop (done = 2); it still publishes, so that no other workgroup is left
// waiting.  The host then redoes this pass's factorisation on the path without inter-workgroup waits.
int backsolve_chain_workgroups(int n_blk) { return n_blk; }

// Tree chain: the workgroup that finishes LAST retires the epoch (every workgroup has read the old value at its start by
// then; with a tree ordering block 0 is not the last to finish any more) and leaves the counter at zero for the next launch.
// (dense chains end with block 0 by construction: it retires the epoch with a plain store -- the returning atomic costs
// the last workgroup, i.e. the launch, ~1-2 us)
__device__ __forceinline__ void chain_block_done(unsigned* n_done, int n_blk, unsigned* epoch_word, unsigned epoch)
{
    if (atomicAdd(n_done, 1u) == (unsigned)n_blk - 1u) {
        *n_done = 0u;
        *epoch_word = epoch;
    }
}

#ifdef VMM_STAMPS
__device__ unsigned long long g_chain_stamps[128][4];   // [block]: start, last dependency seen, published
#define CH_RT(blk, slot)                                                                  \
    do {                                                                                  \
        if (threadIdx.x == 0)                                                             \
            g_chain_stamps[(blk) & 127][slot] = __builtin_amdgcn_s_memrealtime();         \
    } while (0)
extern "C" int vmm_ba_debug_read_chain_stamps(unsigned long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_stamps), sizeof(unsigned long long) * 128 * 4);
}
#else
#define CH_RT(blk, slot)
#endif

// ONE body for both chains.  k_backsolve_chain (TREE = false) is the dense chain: block m waits for every block behind it
// and its hop is on m + 1.  k_backsolve_chain_tree (TREE = true) is the chain of a factor with a block structure (tree
// orderings of the kept family, `nz` as in DfArgs): block m waits only for the blocks j > m with L(j, m) != 0, its hop is on
// the nearest of them (jp, the parent in the elimination tree) instead of m + 1, and the workgroup that finishes LAST
// retires the epoch (block 0 is no longer the last).
// Shared: the arithmetic, the order of every sum, the barriers, the granule protocol, the bounded spin and its report.
// What differs is decided at COMPILE time -- `if constexpr (TREE)` or a constant operand: which blocks are visited
// (below, has_parent), which ys[] buffer a trip uses, and who retires the epoch (skip path, single-wave last block, end).
// Nothing is decided at run time in the dense instantiation.  (An earlier merge behind a RUN-time flag cost the dense chain
// ~2 us per launch, which is why there were two copies of this text for a while.)
// Against the two copies: the same VGPRs (144), LDS and no scratch, 2375 -> 2357 (dense) and 2625 -> 2553 (tree)
// instructions, only moves, compares and scalar control flow changed.  TIMING NOT MEASURED: no GPU run could be had for
// this change; the ~2 us above refers to the run-time merge.
template <bool TREE>
__device__ __forceinline__ void backsolve_chain_body(LmCtl* ctl, const double* __restrict__ S, int ld, int n_pad, int n_blk,
                                                     double* y, const double* __restrict__ dinv, unsigned long long* gran,
                                                     unsigned* epoch_word, const double* __restrict__ Ld,
                                                     const double* __restrict__ Linv,
                                                     const unsigned long long* __restrict__ nz, unsigned* n_done)
{
    // (a give-up inside the dataflow factorisation before this launch has set done = 2: every workgroup that stops
    // waiting raises it itself, report_give_up)
    // (the abort word itself is not looked at here: the epoch it is compared with is being retired by this very launch, and
    // every workgroup of the factorisation that gave up has raised done = 2 itself before that kernel ended)
    if (ctl->done || ctl->lin_fail) {
        // the factorisation before this launch may have tagged granules with the current epoch: retire it even
        // when the solve is skipped (every workgroup of this launch leaves here, so nobody needs the old value)
        if constexpr (TREE) {
            if (threadIdx.x == 0)
                chain_block_done(n_done, n_blk, epoch_word, *epoch_word + 1u);
        } else {
            if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
                *epoch_word = *epoch_word + 1u;
        }
        return;
    }
    const unsigned spin_limit = (ctl->spin_limit_chain && (ctl->spin_wg < 0 || ctl->spin_wg == (int)blockIdx.x))
                                    ? ctl->spin_limit_chain : kSpinLimit;
    __shared__ double L[64 * kLd];    // L(jp, m) for the product B_m
    __shared__ double Li[64 * kLd];   // Linv_m
    __shared__ double red[4][64];
    __shared__ double ws[64];
    __shared__ double ys[2][64];
    __shared__ double sB[16][256];    // B_m: [row within a wave's 16][thread that owns the column]
    __shared__ int s_timeout;
    const int m = n_blk - 1 - (int)blockIdx.x;
    const int tid = threadIdx.x;
    const int c = tid & 63, part = tid >> 6;
    const unsigned epoch = *epoch_word + 1u;   // every workgroup reads it before the one that retires it bumps it
    const int K0 = m * kNB;
    if (tid == 0)
        s_timeout = 0;
    CH_RT(m, 0);
    // wave 0 sweeps block j's granules into ysj: lane c owns unknown c (two granules)
    auto receive = [&](const int j, double* ysj) {
        if (part == 0) {
            const unsigned long long* g = gran + 2 * (int64_t)(j * kNB + c);
            unsigned long long x0, x1;
            for (unsigned n = 0;;) {
                x0 = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x1 = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool ok = (unsigned)(x0 >> 32) == epoch && (unsigned)(x1 >> 32) == epoch;
                if (__all(ok) && spin_limit != 1u)   // a limit of 1 (debugging) gives up even on valid data
                    break;
                __builtin_amdgcn_s_sleep(1);
                if (++n >= spin_limit) {   // wave-uniform give-up: reported as a synchronisation time-out below
                    s_timeout = 1;
                    break;
                }
            }
            ysj[c] = __longlong_as_double((long long)(((x1 & 0xffffffffull) << 32) | (x0 & 0xffffffffull)));
        }
    };
    auto publish = [&](const double yv) {   // wave 0
        const unsigned long long bits = (unsigned long long)__double_as_longlong(yv);
        const unsigned long long tag = (unsigned long long)epoch << 32;
        unsigned long long* g = gran + 2 * (int64_t)(K0 + c);
        __hip_atomic_store(g, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(g + 1, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        y[K0 + c] = yv;   // for the kernels after this launch
    };
    if (m == n_blk - 1) {
        // The last block is the first in the chain and has no inverse (nothing runs beside its factorisation).  ONE
        // wave solves L^T y = w by columns, lane c holding w[c]: 64 steps of (broadcast y_j from lane j, one
        // multiply-add per lane) on registers only -- no barrier, no LDS in the dependent chain.
        if (part == 0) {
            double lcol[64];
#pragma unroll
            for (int jj = 0; jj < 64; ++jj)
                lcol[jj] = (c <= jj) ? Ld[(int64_t)m * 4096 + jj * 64 + c] : 0.0;
            const double dic = dinv[K0 + c];
            double wv = S[(int64_t)n_pad * ld + K0 + c];
            double yv = 0.0;
#pragma unroll
            for (int jj = 63; jj >= 0; --jj) {
                // v_readlane (jj is a constant), not a cross-lane permute through the LDS
                const long long wb = __double_as_longlong(wv * dic);
                const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)wb, jj);
                const unsigned w1 = (unsigned)__builtin_amdgcn_readlane((int)(wb >> 32), jj);
                const double yj = __longlong_as_double((long long)(((unsigned long long)w1 << 32) | w0));
                yv = (c == jj) ? yj : yv;
                wv = (c < jj) ? wv - lcol[jj] * yj : wv;
            }
            publish(yv);
        }
        CH_RT(m, 2);
        if constexpr (TREE) {
            if (tid == 0)
                chain_block_done(n_done, n_blk, epoch_word, epoch);
        } else {
            if (tid == 0 && m == 0)
                *epoch_word = epoch;   // a single block: also the end of the chain
        }
        return;   // no wait, so no timeout
    }
    // The blocks of column m below the diagonal.  Dense: all of m+1 .. n_blk-1, and the hop waits for y_{m+1}.  With the
    // factor's block structure (tree ordering): only those with L(j, m) != 0; the nearest one, jp, is the block whose
    // unknowns arrive last (the parent in the elimination tree) and takes the place of m+1; without any, y_m = u_m.
    auto below = [&](int jj) {   // L(jj, m) may be non-zero (a tree chain without a structure: all)
        if constexpr (TREE)
            return !nz || nz_bit(nz, jj, m);
        else
            return true;
    };
    int jp = m + 1;
    while (jp < n_blk && !below(jp))
        ++jp;
    const bool has_parent = !TREE || jp < n_blk;
    // ---- B_m = L(jp, m) Linv_m on the matrix cores: wave `part` computes rows part*16 .. part*16+15 ----
    // (as 16 x 64 dot products per thread with broadcast LDS reads it took 15 us: every workgroup was late for its hop)
    double li[16];
    {
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, cc = idx & 63;
            L[r * kLd + cc] = has_parent ? S[(int64_t)(jp * kNB + r) * ld + K0 + cc] : 0.0;
            Li[r * kLd + cc] = Linv[(int64_t)m * 4096 + r * 64 + cc];   // lower triangular, zero above the diagonal
        }
        __syncthreads();
        // li: my 16 rows of column c of Linv_m, for u_m = Linv_m^T t
#pragma unroll
        for (int r = 0; r < 16; ++r)
            li[r] = Li[(part * 16 + r) * kLd + c];
        // v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
        // C[row = (lane >> 4) + 4 reg][col = lane & 15]
        const int fi = c & 15, fk = c >> 4;
        double4_t accB[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            accB[t] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const double av = L[(part * 16 + fi) * kLd + 4 * ks + fk];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                accB[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Li[(4 * ks + fk) * kLd + 16 * t + fi], accB[t], 0, 0, 0);
        }
        // to the layout the hop reads: sB[row within my 16][workgroup thread that owns the column]
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sB[fk + 4 * r][part * 64 + 16 * t + fi] = accB[t][r];
        __syncthreads();
    }
    // ---- the blocks behind jp: acc = sum_j L(j, m)^T y_j, highest block first ----
    double acc = 0.0;
    double lt[16], ln[16];
    auto next_down = [&](int from) {   // the highest block below `from` (exclusive) and above jp with an entry; jp: none
        int jj = from - 1;
        while (jj > jp && !below(jj))
            --jj;
        return jj;
    };
    int j = has_parent ? next_down(n_blk) : jp;
    if (j > jp) {
        const double* Lb = S + (int64_t)(j * kNB + part * 16) * ld + K0 + c;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            lt[r] = Lb[(int64_t)r * ld];
    }
    for (int parity = 0; j > jp; parity ^= 1) {
        const int jn = next_down(j);
        if (jn > jp) {   // next tile requested before the wait
            const double* Lb = S + (int64_t)(jn * kNB + part * 16) * ld + K0 + c;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ln[r] = Lb[(int64_t)r * ld];
        }
        double* ysj = ys[TREE ? parity : j & 1];
        receive(j, ysj);
        __syncthreads();   // also orders the reuse of this ys[] buffer two trips later
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc += lt[r] * ysj[part * 16 + r];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            lt[r] = ln[r];
        j = jn;
    }
    // ---- u_m = Linv_m^T (w_m - acc): one hop ahead of the value it will be combined with ----
    red[part][c] = acc;
    __syncthreads();
    if (part == 0)
        ws[c] = S[(int64_t)n_pad * ld + K0 + c] - ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c]));
    __syncthreads();
    double a2 = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        a2 += li[r] * ws[part * 16 + r];
    __syncthreads();   // everyone has read red[] above
    red[part][c] = a2;
    __syncthreads();
    double u = 0.0;
    if (part == 0)
        u = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    // ---- the hop: y_m = u_m - B_m^T y_jp ----
    double* ysj = ys[TREE ? 0 : (m + 1) & 1];   // (every earlier use of ys[] is behind the barriers above)
    if (has_parent)
        receive(jp, ysj);
    else if (part == 0)
        ysj[c] = 0.0;
    __syncthreads();   // also: everyone has read red[] above
    CH_RT(m, 1);
    double a3 = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        a3 += sB[r][tid] * ysj[part * 16 + r];
    red[part][c] = a3;
    __syncthreads();
    if (part == 0)
        publish(u - ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])));
    CH_RT(m, 2);
    if (tid == 0) {
        if (s_timeout)
            raise_sync_timeout(ctl, 2);
        if constexpr (TREE)
            chain_block_done(n_done, n_blk, epoch_word, epoch);
        else if (m == 0)
            *epoch_word = epoch;   // block 0 is the end of the dense chain: every other workgroup has read the old value
    }
}

__global__ __launch_bounds__(256) void k_backsolve_chain(LmCtl* ctl, const double* __restrict__ S, int ld,
                                                         int n_pad, int n_blk, double* y,
                                                         const double* __restrict__ dinv, unsigned long long* gran,
                                                         unsigned* epoch_word, const double* __restrict__ Ld,
                                                         const double* __restrict__ Linv)
{
    backsolve_chain_body<false>(ctl, S, ld, n_pad, n_blk, y, dinv, gran, epoch_word, Ld, Linv, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_backsolve_chain_tree(LmCtl* ctl, const double* __restrict__ S, int ld,
                                                         int n_pad, int n_blk, double* y,
                                                         const double* __restrict__ dinv, unsigned long long* gran,
                                                         unsigned* epoch_word, const double* __restrict__ Ld,
                                                         const double* __restrict__ Linv,
                                                         const unsigned long long* __restrict__ nz, unsigned* n_done)
{
    backsolve_chain_body<true>(ctl, S, ld, n_pad, n_blk, y, dinv, gran, epoch_word, Ld, Linv, nz, n_done);
}

void launch_backsolve_chain(Engine& e, double* S, int n_pad, int ld, double* y, LmCtl* ctl)
{
    const int n_blk = n_pad / kNB;
    if (e.chol_nz_on)
        hipLaunchKernelGGL(k_backsolve_chain_tree, dim3(backsolve_chain_workgroups(n_blk)), dim3(256), 0, e.stream, ctl, S, ld,
                           n_pad, n_blk, y, e.dinv, e.gran, e.flags + 256, (const double*)e.Ldiag, (const double*)e.Linv,
                           (const unsigned long long*)e.chol_nz, e.flags + 261);
    else
        hipLaunchKernelGGL(k_backsolve_chain, dim3(backsolve_chain_workgroups(n_blk)), dim3(256), 0, e.stream, ctl, S, ld,
                           n_pad, n_blk, y, e.dinv, e.gran, e.flags + 256, (const double*)e.Ldiag, (const double*)e.Linv);
}

// The fallback without inter-workgroup waits: one launch per block, last block first.
void launch_backsolve_steps(Engine& e, double* S, int n_pad, int ld, double* y, LmCtl* ctl)
{
    const int n_blk = n_pad / kNB;
    for (int kb = n_blk - 1; kb >= 0; --kb)
        hipLaunchKernelGGL(k_backsolve_step, dim3(kb + 1), dim3(256), 0, e.stream, ctl, S, ld, n_pad, n_blk, kb, y,
                           e.dinv, (const double*)e.Ldiag);
}

int preload_backsolve_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_backsolve_step)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_backsolve_chain)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_backsolve_chain_tree)) != hipSuccess;
    return bad;
}

} // namespace vmm
