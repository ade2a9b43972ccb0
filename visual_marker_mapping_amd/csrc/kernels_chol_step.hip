// Launch-per-column Cholesky factorisation (gfx950): k_chol_step (panel workgroups, trailing-update workgroups and the inverse
// of the previous diagonal factor in one launch per block column), its host schedule, and k_chol_inverse.
// (The three paths and the matrix layout: kernels_chol.hip.)
#include "chol_common.hpp"

namespace vmm {

#ifdef VMM_STAMPS
__device__ unsigned long long g_stamps[64];
#define STAMP(slot)                                                                  \
    do {                                                                             \
        if (blockIdx.x == 1 && threadIdx.x == 0 && k == 1) {                         \
            g_stamps[slot] = __builtin_amdgcn_s_memtime();                           \
            g_stamps[16 + slot] = __builtin_amdgcn_s_memrealtime();                  \
        }                                                                            \
    } while (0)
#define USTAMP(slot)                                                                 \
    do {                                                                             \
        if (u == 0 && threadIdx.x == 0 && k == 1 && t == u + n_wg)                   \
            g_stamps[(slot)] = __builtin_amdgcn_s_memtime();                         \
    } while (0)
#else
#define USTAMP(slot)
#define STAMP(slot)
#endif

// NOTE on the diagonal factor: L_kk goes to its own buffer Ld[k][64][64], never back into S(k,k): every
// workgroup of the launch reads S(k,k) when it starts, and a workgroup that starts late (busy GPU, more
// workgroups than CUs) must still find the unfactored block there.
//
// Panel of block column k as ONE right-looking factorisation of the tall matrix [A_kk; A_ik]:
// workgroup 0 owns only the diagonal block, workgroup b >= 1 the diagonal block (re-factored
// redundantly, cheaper than a dependent launch) plus 64 rows below it (the rhs row n_pad is just one
// more row).  Both 64x64 blocks live in v_mfma_f64_16x16x4_f64 accumulators for the whole kernel:
// wave w holds the 16-row tile row w (tiles (w,0..3); for the diagonal block only tj <= w).
// Eight rounds of eight columns:
//   1. the lanes that hold columns J0..J0+7 publish them to a small LDS panel buffer
//   2. wave 0 (diagonal rows) and wave 1 (rows below) each factor the 8x8 pivot block in registers
//      (eight dependent rsqrt chains, no barrier in between) and scale "their" row: x = a L8^{-T},
//      written back in place
//   3. every wave applies the rank-8 update C -= X X_d^T to its tiles with two MFMAs per tile
// The panel buffers ping-pong between rounds, so two barriers per round suffice and there is no
// separate triangular-solve phase: after the last round the scaled columns ARE L_ik.
// (Four columns per round cost 16 x (2 barriers + 2 LDS round trips); eight halve that overhead for
// the same pivot chain.)
template <int J0, bool HAS_T>
__device__ __forceinline__ void panel_round(const int w, const int lane,
                                            double4_t (&Dacc)[4], double4_t (&Tacc)[4], double* __restrict__ Pd,
                                            double* __restrict__ Pt, double* __restrict__ At,
                                            double* __restrict__ R, double* __restrict__ invd, bool& ok)
{
    constexpr int tc = J0 >> 4, cj = J0 & 15;
    const int fr = lane & 15, fk = lane >> 4;
    double* pd = Pd + ((J0 >> 3) & 1) * 64 * kPs;
    double* pt = Pt + ((J0 >> 3) & 1) * 64 * kPs;
    // 1. publish columns J0..J0+7 (rows of my tile row) from the accumulators
    if (fr >= cj && fr < cj + kPw) {
        const int q = fr - cj;
        const int row = 16 * w + fk;
        if (w >= tc) {
            pd[(row + 0) * kPs + q] = Dacc[tc][0];
            pd[(row + 4) * kPs + q] = Dacc[tc][1];
            pd[(row + 8) * kPs + q] = Dacc[tc][2];
            pd[(row + 12) * kPs + q] = Dacc[tc][3];
        }
        if (HAS_T) {
            pt[(row + 0) * kPs + q] = Tacc[tc][0];
            pt[(row + 4) * kPs + q] = Tacc[tc][1];
            pt[(row + 8) * kPs + q] = Tacc[tc][2];
            pt[(row + 12) * kPs + q] = Tacc[tc][3];
        }
    }
    __syncthreads();
    // 2. pivot block + row scaling (wave 0: diagonal rows, wave 1: rows below)
    if (w == 0 || (w == 1 && HAS_T)) {
        double* row = (w == 0 ? pd : pt) + lane * kPs;
        double x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            x[q] = row[q];
        Piv8 p;
        chol8(pd + J0 * kPs, p);
        scale8(x, p);   // x = a L8^{-T}
        if (w == 0) {
            ok = ok && p.ok;
            const int r = lane - J0;
            const bool below = r >= kPw, above = r < 0;
            if (below) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    row[q] = x[q];
            }
            if (!HAS_T) {
                // keep L^T for the write-back: x below the pivot block, the factor inside, zero above
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    double inside = 0.0;
#pragma unroll
                    for (int rr = q; rr < 8; ++rr)
                        inside = (r == rr) ? p.l[tri8(rr, q)] : inside;
                    At[(J0 + q) * kLdT + lane] = below ? x[q] : (above ? 0.0 : inside);
                }
                if (r >= 0 && r < kPw) {
                    double iv = 0.0;
#pragma unroll
                    for (int rr = 0; rr < 8; ++rr)
                        iv = (r == rr) ? p.inv[rr] : iv;
                    invd[lane] = iv;
                }
            }
        } else {
            double* rr = R + lane * kLd + J0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                row[q] = x[q];
                rr[q] = x[q];
            }
        }
    }
    __syncthreads();
    // 3. rank-8 update of the tiles right of the pivot columns.  MFMA f64 maps: A[i = lane&15][k = lane>>4],
    //    B[k = lane>>4][j = lane&15], C row = (lane>>4) + 4*reg, col = lane&15.
    if (J0 + kPw < 64) {
        constexpr int t0 = (J0 + kPw) >> 4;
        const int ra = 16 * w + fr;
        const bool ma = ra >= J0 + kPw;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const double adv = pd[ra * kPs + 4 * ks + fk];
            const double ad = ma ? -adv : 0.0;
            const double at = HAS_T ? -pt[ra * kPs + 4 * ks + fk] : 0.0;
            // the tile that holds the next pivot columns goes first: the next round's publish waits on it
#pragma unroll
            for (int tj = t0; tj < 4; ++tj) {
                const int rb = 16 * tj + fr;
                const double bv = pd[rb * kPs + 4 * ks + fk];
                const double b = (rb >= J0 + kPw) ? bv : 0.0;
                // tiles above the diagonal (tj > w) get a zero operand instead of a branch
                const double adm = (tj <= w) ? ad : 0.0;
                Dacc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(adm, b, Dacc[tj], 0, 0, 0);
                if (HAS_T)
                    Tacc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(at, b, Tacc[tj], 0, 0, 0);
            }
        }
    }
}

template <bool HAS_T>
__device__ __forceinline__ void panel_body(LmCtl* ctl, double* __restrict__ S, int ld, int n_pad, int k,
                                           double* __restrict__ P, const double* __restrict__ Pprev,
                                           const double* __restrict__ Pprev2, double* __restrict__ dinv,
                                           double* __restrict__ Ld, double* RA, double* Pd, double* Pt, double* invd,
                                           double* Ads, double* Ats)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fk = lane >> 4;
    const int K0 = k * kNB;
    const int R0 = K0 + kNB + ((int)blockIdx.x - 1) * 64;
    STAMP(0);
    // accumulator-layout loads straight from global memory: for fixed (tile, reg) 16 lanes read 128
    // contiguous bytes of one row
    double4_t Dacc[4], Tacc[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        Dacc[tj] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
        Tacc[tj] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * w + fk + 4 * r;
            const double dv = S[(int64_t)(K0 + row) * ld + K0 + 16 * tj + fr];
            Dacc[tj][r] = (tj <= w) ? dv : 0.0;
            if (HAS_T) {
                const int grow = (R0 + row <= n_pad) ? R0 + row : n_pad;   // clamp: always in bounds
                const double tv = S[(int64_t)grow * ld + K0 + 16 * tj + fr];
                Tacc[tj][r] = (R0 + row <= n_pad) ? tv : 0.0;
            }
        }
    }
    // Look-ahead: the trailing updates skip this block column (chol_update2_wg starts one or two columns further), so
    // this kernel does not have to wait for them; the missing rank-64 updates of the tiles (k,k) and (i,k) are applied
    // here from the transposed panels that are still pending: Pprev2 (block column k-2; even k only, the pair of
    // panels k-2, k-1 is applied to the rest of the matrix by this launch and the next) and Pprev (k-1).
    STAMP(6);
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
        const double* __restrict__ Pq = pp == 0 ? Pprev2 : Pprev;
        if (!Pq)
            continue;
        if (pp == 1 && Pprev2)
            __syncthreads();   // the first panel's operands are consumed
        // stage Pq[:, K0..K0+63] (diagonal rows; also the B operand) and Pq[:, R0..R0+63] k-major
        double2 va[8], vt[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int mm = idx >> 5, c = (idx & 31) * 2;
            va[it] = *reinterpret_cast<const double2*>(Pq + (int64_t)mm * ld + K0 + c);
            if (HAS_T)
                vt[it] = *reinterpret_cast<const double2*>(Pq + (int64_t)mm * ld + R0 + c);
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int mm = idx >> 5, c = (idx & 31) * 2;
            *reinterpret_cast<double2*>(&Ads[mm * kLdsRow + c]) = va[it];
            if (HAS_T)
                *reinterpret_cast<double2*>(&Ats[mm * kLdsRow + c]) = vt[it];
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < 16; ++ks) {
            const int row = (ks * 4 + fk) * kLdsRow;
            const double ad = -Ads[row + 16 * w + fr];
            const double at = HAS_T ? -Ats[row + 16 * w + fr] : 0.0;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                const double b = Ads[row + 16 * tj + fr];
                const double adm = (tj <= w) ? ad : 0.0;
                Dacc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(adm, b, Dacc[tj], 0, 0, 0);
                if (HAS_T)
                    Tacc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(at, b, Tacc[tj], 0, 0, 0);
            }
        }
    }
    STAMP(1);
    bool ok = true;
    panel_round<0, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<8, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<16, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<24, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<32, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<40, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<48, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    panel_round<56, HAS_T>(w, lane, Dacc, Tacc, Pd, Pt, RA, RA, invd, ok);
    __syncthreads();
    STAMP(2);
    if (!HAS_T) {
        // `ok` is meaningful in wave 0 only
        if (tid == 0 && !ok)
            ctl->lin_fail = 1;
        if (tid < 64)
            dinv[K0 + tid] = invd[tid];
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            if (c <= r)
                Ld[(int64_t)k * 4096 + r * 64 + c] = RA[c * kLdT + r];
        }
        return;
    }
    STAMP(4);
    // L_ik = the scaled columns collected in R: coalesced stores to S and, transposed, to P
    const double* R = RA;
    for (int idx = tid; idx < 64 * 32; idx += 256) {
        const int rr = idx >> 5, c = (idx & 31) * 2;
        if (R0 + rr <= n_pad)
            *reinterpret_cast<double2*>(S + (int64_t)(R0 + rr) * ld + K0 + c)
                = make_double2(R[rr * kLd + c], R[rr * kLd + c + 1]);
    }
    {
        const int rr = tid & 63;
        if (R0 + rr <= n_pad)
            for (int c = tid >> 6; c < 64; c += 4)
                P[(int64_t)c * ld + R0 + rr] = R[rr * kLd + c];
    }
    STAMP(5);
}

constexpr int kPanelSmem = 64 * kLdT + 4 * 64 * kPs + 64 + 2 * 64 * kLdsRow;   // doubles (kPs = 9: 4 x 576)
constexpr int kUpdateSmem = 4 * 64 * kLdsRow;   // two operand slices, double-buffered: exactly the 160 KB of a CU
constexpr int kStepSmem = kPanelSmem > kUpdateSmem ? kPanelSmem : kUpdateSmem;

__device__ __forceinline__ void chol_panel_wg(LmCtl* ctl, double* __restrict__ S, int ld, int n_pad, int k,
                                              double* __restrict__ P, const double* __restrict__ Pprev,
                                              const double* __restrict__ Pprev2, double* __restrict__ dinv,
                                              double* __restrict__ Ld, double* smem)
{
    double* RA = smem;                     // workgroup 0: L^T (stride kLdT); others: result tile R (stride kLd)
    double* Pd = RA + 64 * kLdT;
    double* Pt = Pd + 2 * 64 * kPs;
    double* invd = Pt + 2 * 64 * kPs;
    double* Ads = invd + 64;               // previous panel, diagonal rows (k-major); 16-byte aligned offsets
    double* Ats = Ads + 64 * kLdsRow;      // previous panel, this workgroup's rows
    if (blockIdx.x == 0)
        panel_body<false>(ctl, S, ld, n_pad, k, P, Pprev, Pprev2, dinv, Ld, RA, Pd, Pt, invd, Ads, Ats);
    else
        panel_body<true>(ctl, S, ld, n_pad, k, P, Pprev, Pprev2, dinv, Ld, RA, Pd, Pt, invd, Ads, Ats);
}

#ifdef VMM_STAMPS
extern "C" int vmm_ba_debug_read_stamps(unsigned long long* out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * (n < 64 ? n : 64));
}
#endif

// Trailing update of block column k: A_ij -= L_ik L_jk^T for k+1 < j <= i (the rhs row block included;
// block column k+1 is left to the next panel kernel, see the look-ahead note there)
// with K = 64 taken from the transposed panel P (64 x ld, row m = panel column m).  One workgroup per
// 64x64 tile; the whole K extent of both operands (2 x 32 KB) and the C tile are requested up front
// so the kernel pays one memory latency, then 16 k-steps of four v_mfma_f64_16x16x4_f64 per wave.
typedef double double2v __attribute__((ext_vector_type(2)));

__host__ __device__ __forceinline__ void update_tile_index(int n_blk, int k, int t, int& bi, int& bj)
{
    // tile index -> (bi, bj): columns k+2..min(bi, n_blk-1) (block column k+1 is updated lazily by the
    // panel of that column), rows k+2..n_blk.  Row q = bi - (k+2) holds q + 1 tiles, except the last row (the
    // right-hand side, bi = n_blk), which has as many as the row before it: closed form, no search (a search
    // from the first row costs ~50 cycles per row, 2 us at 94 rows -- as much as the tile's MFMAs).
    const int n_rows = n_blk - (k + 2) + 1;                 // rows k+2 .. n_blk
    const int before_last = (n_rows - 1) * n_rows / 2;      // tiles in front of the last row
    int q;
    if (t >= before_last) {
        q = n_rows - 1;
        t -= before_last;
    } else {
        q = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        // guard the rounding of the square root
        while (q * (q + 1) / 2 > t)
            --q;
        while ((q + 1) * (q + 2) / 2 <= t)
            ++q;
        t -= q * (q + 1) / 2;
    }
    bi = k + 2 + q;
    bj = k + 2 + t;
}

// The tiles of a launch's trailing update are handed out through a counter (one atomic per tile, fetched two tiles
// ahead of its use): the dedicated update workgroups start at once, the panel workgroups of the same launch join when
// their panel is stored -- at n = 6000 a panel takes ~26 us of a launch that lasts up to 150 us, and the 95 CUs of the
// panel workgroups used to idle for the rest of it.  With more tiles than compute units the operands of the NEXT tile
// are requested before the MFMAs of the current one and parked in the other half of the LDS, and the C tile is
// requested at the start of its own iteration and only added after the 16 k-steps: a tile costs its MFMAs plus one
// barrier instead of a full memory latency.  No register array lives across the loop back-edge (those end up in
// scratch).  The order in which workgroups take tiles does not touch the result: a tile is updated by exactly one.
__device__ __forceinline__ void chol_update_wg(double* __restrict__ S, int ld, int n_blk, int k, unsigned* counter,
                                               int n_tiles, const double* __restrict__ P, double* smem)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int fk = lane >> 4, fi = lane & 15;
    // four ints in the padding columns of the first LDS row (the operand tiles use columns 0..63 of every row)
    volatile int* slot = reinterpret_cast<volatile int*>(smem + 64);
    if (tid == 0) {
        slot[0] = (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slot[1] = (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    int t = slot[0], tn = slot[1];
    const int u = t, n_wg = 0;   // (names the diagnostic stamps refer to)
    (void)u;
    (void)n_wg;
    if (t >= n_tiles)
        return;
    int bi, bj;
    update_tile_index(n_blk, k, t, bi, bj);
    {
        double2 va[8], vb[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            va[it] = *reinterpret_cast<const double2*>(P + (int64_t)m * ld + bi * kNB + c);
            vb[it] = *reinterpret_cast<const double2*>(P + (int64_t)m * ld + bj * kNB + c);   // diagonal tile: same lines
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            *reinterpret_cast<double2*>(&smem[m * kLdsRow + c]) = va[it];
            *reinterpret_cast<double2*>(&smem[(64 + m) * kLdsRow + c]) = vb[it];
        }
    }
    __syncthreads();
    int cur = 0;
    for (int iter = 0;; ++iter) {
        const double* As = smem + cur * 128 * kLdsRow;
        const double* Bs = As + 64 * kLdsRow;
        const int I0 = bi * kNB, J0 = bj * kNB;
        // the tile after the next one, read by everybody behind this iteration's closing barrier
        if (tid == 0)
            slot[2 + (iter & 1)] = (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // The requests of this tile's C values and of the NEXT tile's operands are issued as volatile asm:
        // written as plain loads, LLVM sinks them below the MFMA loop to their first use (measured: the
        // memory latency then adds to the MFMA time, 6.6 us per tile instead of ~3).  The results are only
        // touched after the matching s_waitcnt below, which takes them as read-write operands.
        USTAMP(40);
        double creg[2][2][4];
        const double* pc[16];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pc[8 * a + 4 * b + r] = S + (int64_t)(I0 + wi * 32 + a * 16 + fk + 4 * r) * ld + J0 + wj * 32 + b * 16 + fi;
        const bool more = tn < n_tiles;   // workgroup-uniform
        // The last tile re-requests itself (result unused).
        int nbi = bi, nbj = bj;
        if (more)
            update_tile_index(n_blk, k, tn, nbi, nbj);
        double2v va[8], vb[8];
        const double* pa[8];
        const double* pb[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            pa[it] = P + (int64_t)m * ld + nbi * kNB + c;
            pb[it] = P + (int64_t)m * ld + nbj * kNB + c;
        }
        USTAMP(41);
        double4_t acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                acc[a][b] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
        // 16 k-steps; the LDS operands of step ks+1 are read before the MFMAs of step ks, and one of the 16
        // operand requests of the next tile is issued per step (VMEM issue slots beside the MFMAs)
        double a0 = -As[fk * kLdsRow + wi * 32 + fi], a1 = -As[fk * kLdsRow + wi * 32 + 16 + fi];
        double b0 = Bs[fk * kLdsRow + wj * 32 + fi], b1 = Bs[fk * kLdsRow + wj * 32 + 16 + fi];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            // one pair of requests per k-step (issuing all 32 in the first four steps was measured slower: 4.02 against
            // 3.69 ms per factorisation at n = 6000 -- the loop is bound by the memory system's throughput, not by latency)
            if (ks < 8) {   // this tile's C values (HBM, the longer latency) first ...
                __asm__ volatile("global_load_dwordx2 %0, %1, off nt"
                                 : "=&v"(creg[(2 * ks) >> 3][((2 * ks) >> 2) & 1][(2 * ks) & 3]) : "v"(pc[2 * ks]) : "memory");
                __asm__ volatile("global_load_dwordx2 %0, %1, off nt"
                                 : "=&v"(creg[(2 * ks + 1) >> 3][((2 * ks + 1) >> 2) & 1][(2 * ks + 1) & 3]) : "v"(pc[2 * ks + 1]) : "memory");
            } else {        // ... then the next tile's operands (L2)
                __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=&v"(va[ks - 8]) : "v"(pa[ks - 8]) : "memory");
                __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=&v"(vb[ks - 8]) : "v"(pb[ks - 8]) : "memory");
            }
            double na0 = 0.0, na1 = 0.0, nb0 = 0.0, nb1 = 0.0;
            if (ks < 15) {
                const int row = ((ks + 1) * 4 + fk) * kLdsRow;
                na0 = -As[row + wi * 32 + fi];
                na1 = -As[row + wi * 32 + 16 + fi];
                nb0 = Bs[row + wj * 32 + fi];
                nb1 = Bs[row + wj * 32 + 16 + fi];
            }
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            a0 = na0;
            a1 = na1;
            b0 = nb0;
            b1 = nb1;
        }
#ifdef VMM_STAMPS
        __asm__ volatile("" ::"v"(acc[0][0][0]), "v"(acc[1][1][3]) : "memory");
#endif
        USTAMP(42);
        __asm__ volatile("s_waitcnt vmcnt(0)"
                         : "+v"(creg[0][0][0]), "+v"(creg[0][0][1]), "+v"(creg[0][0][2]), "+v"(creg[0][0][3]),
                           "+v"(creg[0][1][0]), "+v"(creg[0][1][1]), "+v"(creg[0][1][2]), "+v"(creg[0][1][3]),
                           "+v"(creg[1][0][0]), "+v"(creg[1][0][1]), "+v"(creg[1][0][2]), "+v"(creg[1][0][3])
                         :
                         : "memory");
        __asm__ volatile("s_waitcnt vmcnt(0)"
                         : "+v"(creg[1][1][0]), "+v"(creg[1][1][1]), "+v"(creg[1][1][2]), "+v"(creg[1][1][3]),
                           "+v"(va[0]), "+v"(va[1]), "+v"(va[2]), "+v"(va[3]), "+v"(va[4]), "+v"(va[5]), "+v"(va[6]),
                           "+v"(va[7])
                         :
                         : "memory");
        __asm__ volatile("s_waitcnt vmcnt(0)"
                         : "+v"(vb[0]), "+v"(vb[1]), "+v"(vb[2]), "+v"(vb[3]), "+v"(vb[4]), "+v"(vb[5]), "+v"(vb[6]),
                           "+v"(vb[7])
                         :
                         : "memory");
        USTAMP(43);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    // non-temporal, like the loads of these values: a tile of C is touched once per launch, and kept out
                    // of the L2 it leaves the transposed panel (3 MB, read by every workgroup for every tile) resident --
                    // the update is bound by memory traffic (16 B of C + 16 B of operands per 128 flops), not by the MFMAs
                    __builtin_nontemporal_store(creg[a][b][r] + acc[a][b][r],
                                                &S[(int64_t)(I0 + wi * 32 + a * 16 + fk + 4 * r) * ld + J0 + wj * 32 + b * 16 + fi]);
        USTAMP(44);
        // park the next tile's operands in the other half (nobody reads it during this iteration)
        double* An = smem + (cur ^ 1) * 128 * kLdsRow;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            *reinterpret_cast<double2v*>(&An[m * kLdsRow + c]) = va[it];
            *reinterpret_cast<double2v*>(&An[(64 + m) * kLdsRow + c]) = vb[it];
        }
        USTAMP(45);
        __syncthreads();
        USTAMP(46);
        cur ^= 1;
        bi = nbi;
        bj = nbj;
        t = tn;
        tn = slot[2 + (iter & 1)];
        if (t >= n_tiles)
            break;
    }
}

// Rank-128 trailing update: the transposed panels PA (block column c0-3) and PB (c0-2) applied in ONE visit of each C tile
// of the block columns >= c0 (rows >= column, the right-hand side row included).  A rank-64 visit moves 16 B of C per
// 128 flops and the launch is bound by that traffic (measured at n = 6000: the MFMA work of two updates in one visit
// costs 1.35x one visit, not 2x); the pair halves it.  Tile t of the pair's list: first block column c0 (needed by the
// next panel), then the triangle of the columns > c0 in update_tile_index order; the list is worked off by two
// consecutive launches (tiles [t0, t1) each, handed out by `counter` as in chol_update_wg).
// One loop iteration = one tile = two halves of 16 k-steps: half 0 multiplies the PA operands (parked in LDS half `0`)
// while the tile's C values (non-temporal) and its PB operands are requested, half 1 multiplies the PB operands
// (LDS half `1`) while the NEXT tile's PA operands are requested; C is added and stored behind half 1.  As in
// chol_update_wg the requests are volatile asm, touched only behind the matching s_waitcnt (tools/check_chol_asm.py).
__host__ __device__ __forceinline__ void pair_tile_index(int n_blk, int c0, int t, int& bi, int& bj)
{
    const int n_first = n_blk - c0 + 1;   // block column c0: rows c0 .. n_blk
    if (t < n_first) {
        bi = c0 + t;
        bj = c0;
    } else {
        update_tile_index(n_blk, c0 - 1, t - n_first, bi, bj);
    }
}

__device__ __forceinline__ void chol_update2_wg(double* __restrict__ S, int ld, int n_blk, int c0, unsigned* counter,
                                                int t0, int t1, const double* __restrict__ PA,
                                                const double* __restrict__ PB, double* smem)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int fk = lane >> 4, fi = lane & 15;
    volatile int* slot = reinterpret_cast<volatile int*>(smem + 64);   // padding columns of the first LDS row
    if (tid == 0) {
        slot[0] = t0 + (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slot[1] = t0 + (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    int t = slot[0], tn = slot[1];
    if (t >= t1)
        return;
    int bi, bj;
    pair_tile_index(n_blk, c0, t, bi, bj);
    double* const L0 = smem;                    // PA operands: A rows 0..63, B rows 64..127 (k-major)
    double* const L1 = smem + 128 * kLdsRow;    // PB operands
    {
        double2 va[8], vb[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            va[it] = *reinterpret_cast<const double2*>(PA + (int64_t)m * ld + bi * kNB + c);
            vb[it] = *reinterpret_cast<const double2*>(PA + (int64_t)m * ld + bj * kNB + c);
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            *reinterpret_cast<double2*>(&L0[m * kLdsRow + c]) = va[it];
            *reinterpret_cast<double2*>(&L0[(64 + m) * kLdsRow + c]) = vb[it];
        }
    }
    __syncthreads();
    for (int iter = 0;; ++iter) {
        const int I0 = bi * kNB, J0 = bj * kNB;
        if (tid == 0)   // the tile after the next one, read by everybody behind this iteration's closing barrier
            slot[2 + (iter & 1)] = t0 + (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double creg[2][2][4];
        double2v va[8], vb[8];
        const double* pa[8];
        const double* pb[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            pa[it] = PB + (int64_t)m * ld + bi * kNB + c;
            pb[it] = PB + (int64_t)m * ld + bj * kNB + c;
        }
        double4_t acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                acc[a][b] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
        // ---- half 0: PA operands; requests: this tile's PB operands, then its C values.  The C values (HBM, the longer
        // latency) are only needed behind half 1: the wait at the end of this half leaves the 16 most recent requests --
        // exactly them -- in flight (loads return in order), so they have both halves to arrive
        {
            // (the addresses of the C values only live in this half: they are recomputed for the stores -- kept across
            // half 1 their 32 registers push the compiler into copying `creg` while its loads are still in flight)
            const double* pc[16];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        pc[8 * a + 4 * b + r] = S + (int64_t)(I0 + wi * 32 + a * 16 + fk + 4 * r) * ld + J0 + wj * 32 + b * 16 + fi;
            const double* As = L0;
            const double* Bs = L0 + 64 * kLdsRow;
            double a0 = -As[fk * kLdsRow + wi * 32 + fi], a1 = -As[fk * kLdsRow + wi * 32 + 16 + fi];
            double b0 = Bs[fk * kLdsRow + wj * 32 + fi], b1 = Bs[fk * kLdsRow + wj * 32 + 16 + fi];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (ks < 8) {
                    __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=&v"(va[ks]) : "v"(pa[ks]) : "memory");
                    __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=&v"(vb[ks]) : "v"(pb[ks]) : "memory");
                } else {
                    const int q = 2 * (ks - 8);
                    __asm__ volatile("global_load_dwordx2 %0, %1, off nt"
                                     : "=&v"(creg[q >> 3][(q >> 2) & 1][q & 3]) : "v"(pc[q]) : "memory");
                    __asm__ volatile("global_load_dwordx2 %0, %1, off nt"
                                     : "=&v"(creg[(q + 1) >> 3][((q + 1) >> 2) & 1][(q + 1) & 3]) : "v"(pc[q + 1]) : "memory");
                }
                double na0 = 0.0, na1 = 0.0, nb0 = 0.0, nb1 = 0.0;
                if (ks < 15) {
                    const int row = ((ks + 1) * 4 + fk) * kLdsRow;
                    na0 = -As[row + wi * 32 + fi];
                    na1 = -As[row + wi * 32 + 16 + fi];
                    nb0 = Bs[row + wj * 32 + fi];
                    nb1 = Bs[row + wj * 32 + 16 + fi];
                }
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
                a0 = na0;
                a1 = na1;
                b0 = nb0;
                b1 = nb1;
            }
        }
        __asm__ volatile("s_waitcnt vmcnt(16)"
                         : "+v"(va[0]), "+v"(va[1]), "+v"(va[2]), "+v"(va[3]), "+v"(va[4]), "+v"(va[5]), "+v"(va[6]),
                           "+v"(va[7])
                         :
                         : "memory");
        __asm__ volatile("s_waitcnt vmcnt(16)"
                         : "+v"(vb[0]), "+v"(vb[1]), "+v"(vb[2]), "+v"(vb[3]), "+v"(vb[4]), "+v"(vb[5]), "+v"(vb[6]),
                           "+v"(vb[7])
                         :
                         : "memory");
        // park the PB operands in the other half (its last readers finished before the previous closing barrier)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            *reinterpret_cast<double2v*>(&L1[m * kLdsRow + c]) = va[it];
            *reinterpret_cast<double2v*>(&L1[(64 + m) * kLdsRow + c]) = vb[it];
        }
        __syncthreads();
        // ---- half 1: PB operands; requests: the NEXT tile's PA operands (the last tile re-requests itself, unused)
        const bool more = tn < t1;   // workgroup-uniform
        int nbi = bi, nbj = bj;
        if (more)
            pair_tile_index(n_blk, c0, tn, nbi, nbj);
        double2v wa[8], wb[8];
        const double* qa[8];
        const double* qb[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            qa[it] = PA + (int64_t)m * ld + nbi * kNB + c;
            qb[it] = PA + (int64_t)m * ld + nbj * kNB + c;
        }
        {
            const double* As = L1;
            const double* Bs = L1 + 64 * kLdsRow;
            double a0 = -As[fk * kLdsRow + wi * 32 + fi], a1 = -As[fk * kLdsRow + wi * 32 + 16 + fi];
            double b0 = Bs[fk * kLdsRow + wj * 32 + fi], b1 = Bs[fk * kLdsRow + wj * 32 + 16 + fi];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (ks < 8) {
                    __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=&v"(wa[ks]) : "v"(qa[ks]) : "memory");
                    __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=&v"(wb[ks]) : "v"(qb[ks]) : "memory");
                }
                double na0 = 0.0, na1 = 0.0, nb0 = 0.0, nb1 = 0.0;
                if (ks < 15) {
                    const int row = ((ks + 1) * 4 + fk) * kLdsRow;
                    na0 = -As[row + wi * 32 + fi];
                    na1 = -As[row + wi * 32 + 16 + fi];
                    nb0 = Bs[row + wj * 32 + fi];
                    nb1 = Bs[row + wj * 32 + 16 + fi];
                }
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
                a0 = na0;
                a1 = na1;
                b0 = nb0;
                b1 = nb1;
            }
        }
        __asm__ volatile("s_waitcnt vmcnt(0)"
                         : "+v"(creg[0][0][0]), "+v"(creg[0][0][1]), "+v"(creg[0][0][2]), "+v"(creg[0][0][3]),
                           "+v"(creg[0][1][0]), "+v"(creg[0][1][1]), "+v"(creg[0][1][2]), "+v"(creg[0][1][3]),
                           "+v"(creg[1][0][0]), "+v"(creg[1][0][1]), "+v"(creg[1][0][2]), "+v"(creg[1][0][3])
                         :
                         : "memory");
        __asm__ volatile("s_waitcnt vmcnt(0)"
                         : "+v"(creg[1][1][0]), "+v"(creg[1][1][1]), "+v"(creg[1][1][2]), "+v"(creg[1][1][3]),
                           "+v"(wa[0]), "+v"(wa[1]), "+v"(wa[2]), "+v"(wa[3]), "+v"(wa[4]), "+v"(wa[5]), "+v"(wa[6]),
                           "+v"(wa[7])
                         :
                         : "memory");
        __asm__ volatile("s_waitcnt vmcnt(0)"
                         : "+v"(wb[0]), "+v"(wb[1]), "+v"(wb[2]), "+v"(wb[3]), "+v"(wb[4]), "+v"(wb[5]), "+v"(wb[6]),
                           "+v"(wb[7])
                         :
                         : "memory");
        // (stores behind the wait: on gfx9 they count in vmcnt too)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    __builtin_nontemporal_store(creg[a][b][r] + acc[a][b][r],
                                                &S[(int64_t)(I0 + wi * 32 + a * 16 + fk + 4 * r) * ld + J0 + wj * 32 + b * 16 + fi]);
        // park the next tile's PA operands (half 0 was last read before the barrier in the middle of this iteration)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 256 + tid;
            const int m = idx >> 5, c = (idx & 31) * 2;
            *reinterpret_cast<double2v*>(&L0[m * kLdsRow + c]) = wa[it];
            *reinterpret_cast<double2v*>(&L0[(64 + m) * kLdsRow + c]) = wb[it];
        }
        __syncthreads();
        bi = nbi;
        bj = nbj;
        t = tn;
        tn = slot[2 + (iter & 1)];
        if (t >= t1)
            break;
    }
}

// One launch per block column k: workgroups [0, n_panel) factor panel k (with the lazy update of their own column
// from the pending panels k-1 and, for even k of the paired launches, k-2), the others apply a trailing update.  While
// the update is what a launch waits for (more than kPairMinBlocks block columns left) it is a rank-128 one: launches 2m
// and 2m+1 share the update of the panels 2m-2 and 2m-1 (PA, PB) on the block columns >= c0 = 2m+1 (tiles [t0, t1) of
// pair_tile_index each; launch 2m takes block column 2m+1, which the next panel needs, and about half of the rest).
// Near the end a launch is as long as its panel chain and the second lazy panel of the paired form (+6 us on every other
// launch) costs more than the saved traffic: PB == nullptr = the rank-64 update of panel k-1 (PA) on the columns >= k+1.
// The two parts of a launch touch disjoint tiles and both only need results of earlier launches, so the update
// (throughput work) runs beside the latency-bound panel instead of in front of it.
__global__ __launch_bounds__(256) void k_chol_step(LmCtl* ctl, double* __restrict__ S, int ld, int n_pad, int n_blk,
                                                   int k, int n_panel, double* __restrict__ Pcur,
                                                   const double* __restrict__ Pprev, const double* __restrict__ Pprev2,
                                                   double* __restrict__ dinv, double* __restrict__ Ld,
                                                   double* __restrict__ Linv, const double* __restrict__ PA,
                                                   const double* __restrict__ PB, int c0, int t0, int t1, int n_upd_wg,
                                                   unsigned* tile_ctr)
{
    if (ctl->done)
        return;
    if (k == 0)
        phase_stamp(ctl, 3);
    if (ctl->lin_fail)
        return;
    // the tile counter of launch k is word k & 1; launch k resets the other word for launch k + 1 (launches 0 and 1
    // have no trailing update: whatever an earlier factorisation left behind, word k & 1 is zero at launch k)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        tile_ctr[(k + 1) & 1] = 0u;
    __shared__ __attribute__((aligned(16))) double smem[kStepSmem];
    if ((int)blockIdx.x < n_panel) {
        chol_panel_wg(ctl, S, ld, n_pad, k, Pcur, Pprev, Pprev2, dinv, Ld, smem);
        if (t1 > t0) {   // the panel is stored: help with the trailing update
            __syncthreads();
            if (PB)
                chol_update2_wg(S, ld, n_blk, c0, tile_ctr + (k & 1), t0, t1, PA, PB, smem);
            else
                chol_update_wg(S, ld, n_blk, c0 - 2, tile_ctr + (k & 1), t1, PA, smem);
        }
    } else if ((int)blockIdx.x < n_panel + n_upd_wg) {
        if (PB)
            chol_update2_wg(S, ld, n_blk, c0, tile_ctr + (k & 1), t0, t1, PA, PB, smem);
        else   // rank-64 update of the single panel PA on the block columns >= c0 (tiles [0, t1))
            chol_update_wg(S, ld, n_blk, c0 - 2, tile_ctr + (k & 1), t1, PA, smem);
    } else   // last workgroup of launches k >= 1: invert the diagonal factor of block k-1
        chol_inverse_wg(Ld + (int64_t)(k - 1) * 4096, dinv + (k - 1) * kNB, Linv + (int64_t)(k - 1) * 4096, smem);
}

// The look-ahead launches leave the last diagonal block uninverted (the chain solves it directly); the
// covariance forward substitution needs all of them.
__global__ __launch_bounds__(256) void k_chol_inverse(const LmCtl* ctl, const double* __restrict__ Ld,
                                                      const double* __restrict__ dinv, double* __restrict__ Linv, int k)
{
    if (ctl->done || ctl->lin_fail)
        return;
    __shared__ __attribute__((aligned(16))) double smem[64 * kLd + 64];
    chol_inverse_wg(Ld + (int64_t)k * 4096, dinv + k * kNB, Linv + (int64_t)k * 4096, smem);
}

void launch_chol_inverse(Engine& e, int k)
{
    hipLaunchKernelGGL(k_chol_inverse, dim3(1), dim3(256), 0, e.stream, (const LmCtl*)e.ctl, (const double*)e.Ldiag,
                       (const double*)e.dinv, e.Linv, k);
}

constexpr int kPairMinBlocks = 46;   // block columns left below which the launches stop pairing their trailing updates

static int update_tiles(int n_blk, int k)   // tiles of the trailing update of panel k: columns >= k+2
{
    int tiles = 0;
    for (int r = k + 2; r <= n_blk; ++r)
        tiles += ((r < n_blk) ? r : n_blk - 1) - (k + 1);
    return tiles;
}

// The k_chol_step launches that factor the leading n_blk - n_df block columns (and, when a dataflow tail follows, hand
// the rest of the matrix over with every update applied).  Pure host logic, also exported for the schedule test
// (vmm_ba_debug_chol_schedule): tests/test_host_cpu.py replays it for every size and checks that each tile receives
// each panel exactly once, from a panel of an earlier launch, before its block column is factored.
//   launches k < k_pair are paired (rank-128 updates: launches 2m and 2m+1 share the pair of panels 2m-2, 2m-1 on the
//   block columns >= 2m+1), launch k_pair finishes the last pair alone, later ones are single (rank-64: panel k-1 on the
//   columns >= k+1): measured at n = 6000, the pair wins while more than ~46 block columns are left.
std::vector<CholLaunch> chol_step_schedule(int n_blk, int n_df)
{
    std::vector<CholLaunch> out;
    const int n_step = n_blk - n_df;   // even when a tail follows (dataflow_blocks)
    int k_pair = 0;
    while (n_blk - k_pair > kPairMinBlocks)
        k_pair += 2;
    if (k_pair > n_step)
        k_pair = n_step;       // the hand-over launch then finishes the last pair
    for (int k = 0; k < n_step; ++k) {
        CholLaunch L = { k, { -1, k > 0 ? k - 1 : -1 }, { -1, -1 }, k + 1, 0, 0 };
        if (k >= 2 && k <= k_pair) {
            const int m = k / 2;
            L.c0 = 2 * m + 1;
            L.upd[0] = 2 * m - 2;
            L.upd[1] = 2 * m - 1;
            if (!(k & 1))
                L.lazy[0] = k - 2;
            if (L.c0 <= n_blk - 1) {
                const int n_first = n_blk - L.c0 + 1;
                const int total = n_first + update_tiles(n_blk, L.c0 - 1);
                // launch 2m takes block column 2m+1 (the next panel needs it) and about half of the rest
                const int half = k == k_pair ? total : std::max(n_first, (total + 1) / 2);
                L.t0 = (k & 1) ? half : 0;
                L.t1 = (k & 1) ? total : half;
            }
        } else if (k >= 1 && k > k_pair) {
            L.upd[0] = k - 1;
            L.t1 = update_tiles(n_blk, k - 1);
        }
        out.push_back(L);
    }
    if (n_df > 0) {
        // hand-over to the one-launch kernel: what is still pending on every block column >= n_step (the pair of panels
        // n_step-2, n_step-1 when the last launch was a paired one, else panel n_step-1) in one update-only launch (it
        // also inverts diagonal block n_step-1)
        const bool pair = n_step <= k_pair;
        CholLaunch L = { -1, { -1, -1 }, { n_step - (pair ? 2 : 1), pair ? n_step - 1 : -1 }, n_step, 0, 0 };
        L.t1 = pair ? (n_blk - L.c0 + 1) + update_tiles(n_blk, L.c0 - 1) : update_tiles(n_blk, L.c0 - 2);
        out.push_back(L);
    }
    return out;
}

// tile t of a launch's update list (host copy of what the kernel computes)
void chol_schedule_tile(int n_blk, const CholLaunch& L, int t, int* bi, int* bj)
{
    if (L.upd[1] >= 0)
        pair_tile_index(n_blk, L.c0, t, *bi, *bj);
    else
        update_tile_index(n_blk, L.c0 - 2, t, *bi, *bj);
}

// Launches the schedule: the leading n_blk - n_df block columns, one k_chol_step launch each (+ the hand-over launch).
void launch_chol_steps(Engine& e, double* S, int n_pad, int ld, LmCtl* ctl, int n_df)
{
    const int n_blk = n_pad / kNB;
    for (const CholLaunch& L : chol_step_schedule(n_blk, n_df)) {
        const int k = L.k >= 0 ? L.k : n_blk - n_df;   // (the hand-over launch carries the number of the first tail column)
        int n_panel = 0;
        if (L.k >= 0) {
            const int rows_below = n_pad + 1 - (k + 1) * kNB;
            n_panel = 1 + (rows_below + 63) / 64;
        }
        auto panel = [&](int p) { return p >= 0 ? (const double*)e.P4[p & 3] : (const double*)nullptr; };
        const int n_upd = L.t1 - L.t0;
        // all workgroups of a launch resident at once (one per CU: 160 KB of LDS): the update workgroups
        // share the CUs the panel leaves free and loop over the tiles
        const int n_upd_wg = L.k >= 0 ? std::min(n_upd, std::max(e.n_cu - n_panel - 1, e.n_cu / 4))
                                      : std::min(n_upd, e.n_cu - 1);
        const int grid = n_panel + n_upd_wg + (k > 0 ? 1 : 0);
        hipLaunchKernelGGL(k_chol_step, dim3(grid), dim3(256), 0, e.stream, ctl, S, ld, n_pad, n_blk, k, n_panel,
                           L.k >= 0 ? e.P4[k & 3] : (double*)nullptr, panel(L.lazy[1]), panel(L.lazy[0]), e.dinv, e.Ldiag,
                           e.Linv, panel(L.upd[0]), panel(L.upd[1]), L.c0, L.t0, L.t1, n_upd_wg, e.flags + 258);
        if (e.sw.debug) {
            const hipError_t le = hipPeekAtLastError();
            if (le != hipSuccess)
                fprintf(stderr, "[vmm_ba debug] k_chol_step k=%d grid=%d: %s\n", k, grid, hipGetErrorString(le));
        }
    }
}

int preload_chol_step_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_chol_step)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_chol_inverse)) != hipSuccess;
    return bad;
}

} // namespace vmm
