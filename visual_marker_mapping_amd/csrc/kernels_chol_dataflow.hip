#include <type_traits>
#include <utility>

#include "chol_common.hpp"

namespace vmm {

// ------------------------------------------------------------------------------------------------
// Dataflow factorisation (k_chol_dataflow and its _bulk, _tree, _tree_help forms): the whole Cholesky + forward substitution
// of a reduced system in ONE launch (the three paths and the matrix layout: kernels_chol.hip).  Every (block column j, row
// block R > j) pair is a workgroup (`role`; the right-hand side row is row block n_blk) that keeps its two 64x64 blocks -- a
// replica of the diagonal block (j,j) and the block (R,j) -- in MFMA accumulators from the first to the last instruction
// (left-looking): it first subtracts the contributions of the panels k < j, eight columns at a time, as those columns are
// published by the workgroups (k,j) and (k,R), then factors its own panel (eight rounds of eight columns) and publishes its
// scaled columns round by round.  One more workgroup per block column holds only the diagonal block; it writes the diagonal
// factor, its reciprocals and its inverse (back-substitution, covariance).
//
// A published slice (64 rows x 8 columns) travels as self-validating {epoch, 32 value bits} granules
// (cdna_hip_programming.md Guideline 16, R2: the data is the flag): layout [half][column][row], written by ONE
// wave with one aligned agent-scope 8-byte store per granule, swept by the consumers with agent-scope loads
// until every tag carries this factorisation's epoch (wait_slice, wait_slice_pair).  S is read at the start (written by the
// previous kernel) and L, Ld, dinv, Linv are written for the kernels that follow.
//
// What this buys at 19 blocks against one k_chol_step launch per block column (21 us each): the accumulators
// never leave the registers between panels (no load / rank-64 update / store per step: 9.4 us), the update of
// column j+1 by panel j is applied eight columns behind the panel's own rounds on OTHER compute units, and the
// 19 launch boundaries go.  Measured time line (tools/gpu_df_stamps.sh): 1.05-1.2 us per 8-column round (the
// pivot chain: 8x8 Cholesky ~1200 cycles + row scaling ~750 + hand-offs), ~3 us from the last round of a block
// column to the first pivot block of the next (granule latency + the consumer's backlog: a slice costs a worker
// 26 MFMAs = 0.7 us + operand loads, about the rate at which slices are produced), 11.7 us per block column.
//
// The waves are specialised, each alone on its SIMD (f64 MFMA and f64 VALU share a SIMD's FP64 pipe):
//   wave 0 (P0) is the pivot chain: 8x8 pivot block, rows of the diagonal block scaled, and the NEXT pivot block formed by
//     itself (the block before this round's update, left in Nd by the workers, minus the Gram product of the rows just scaled);
//   wave 1 (P1) factors the same pivot block, scales the rows below and publishes them (granules);
//   waves 2, 3 (W0, W1) own ALL accumulator tiles (13 each) and issue every MFMA.
// While the panels before its own are consumed, P0/P1 sweep the slices and stage them in the LDS, one barrier per slice
// (pivot_path), and W0/W1 apply them (worker_path).  Round r of the own panel is pivot_round beside worker_round, the same
// barriers in both: A (round 0 only) the first pivot block is in Pb; B all rows of columns 8r..8r+7 and the next diagonal
// block (Nd) are in the LDS; C the scaled columns and the next pivot block are.  P0/P1 run the 8x8 Cholesky in front of B and
// scale between B and C.  The workers apply, during round r, the rank-8 update with the columns of round r-1 (round 0 of a
// block column > 0: the last slice of the previous panel); phase_of sorts a worker's tiles into the phases of that update:
// 1 in front of A (the tile with the first pivot block), 2 in front of B, beside the 8x8 Cholesky (first what the pivot waves
// need before they scale, urgent_tile, then others until the worker has kFill2 in all), 3 between B and C (the rest).
// Helper waves (MODE bit 1: k_chol_dataflow_tree_help, six waves): waves 4, 5 hold six of each worker's tiles while the
// earlier panels are applied and hand them over through the LDS before the last slice (helper_path); the same bits.
// Compact copies (MODE bit 0, BULK: _bulk, _tree, _tree_help): a finished workgroup writes its block once more as plain
// doubles (DfArgs::Gc) and then a completion word (DfArgs::done[slot] = epoch, release); a consumer asks for that word one
// panel ahead and reads a panel that is complete by then from its copy (half the bytes, no validity test), any other
// through its granules.
//
// Variants built and measured at 19 blocks, then removed: every wave owning a 16-row strip
// of both blocks with waves 0/1 also carrying the pivot chain (233 us against 223 us); the pivot waves applying
// the previous round's rank-8 update to whole columns themselves so that a round is one barrier (rounds 1.45 us:
// 64 LDS reads + 64 FMAs per lane and round cost more than the wait they remove; 253 us); the pivot waves fixing
// up only the 8x8 pivot block from an early copy (230 us: the workers' slice backlog, not the pivot chain, sets
// the pace).
//
// Used (launch_cholesky_solve, dataflow_blocks) for dense systems of up to 48 block columns (1224 workgroups, more than the
// chip holds at one per CU), for the last 33 or 34 block columns of a larger system of at most n_cu block columns, and for
// every tree-ordered factor (k_chol_dataflow_tree: only the non-zero blocks have workgroups; _tree_help from 64 block
// columns on; _bulk on request only).  The measurements behind these choices: launch_dataflow.
//
// Progress: blockIdx is panel-major, so a workgroup only waits for workgroups with smaller blockIdx; with the in-order
// dispatch observed on this hardware the earliest unfinished workgroup is always resident and never waits for an
// undispatched one.  HIP does not promise that order, so every spin is bounded (DfArgs::spin_limit).  A wait that gives up
// stages NaN and raises the abort word (= epoch), which ends every other spin; each workgroup that gave up or saw the abort
// word reports it (report_give_up): bit 0 of LmCtl::sync_timeout and done = 2 -- NOT lin_fail, which stays what a non-positive
// pivot raises.  The host redoes the pass on the launch-per-column path (recover_sync_timeout): slow, not wrong.
// ------------------------------------------------------------------------------------------------
constexpr int kDfSlice = 2 * 8 * 64;         // granules (8 bytes each) per published slice
// LDS row stride (doubles) of the dataflow kernel's 64x8 panel buffers and 8x8 blocks: EVEN, so a row starts 16-byte
// aligned and is read / written two entries per instruction (the pivot waves' LDS round trips are on the critical path:
// 4 instead of 8 per row); 10: a 16-lane group of ds_read_b128 covers all 64 banks, the workers' ds_read_b64 operand
// fetches (16 rows x 2 columns per half wave) stay conflict-free
constexpr int kPsD = 10;
constexpr unsigned kDfSpinDefault = 1u << 21;   // polls of ~0.3 us each before giving up
constexpr int kDfXs = 8 * kLdsRow;            // doubles per staged slice, k-major [8][kLdsRow]
// doubles: 73 KB used, declared as 84 KB.  The copy of the diagonal factor that the block inverse reads (64 x kLd + 64,
// diagonal-only role, after the last round) lives in the panel / slice buffers, which are dead by then.  84 KB: two
// of these workgroups never share a CU (every wave alone on its SIMD), while a rank-k update workgroup (72 KB) still
// fits on the same CU beside a factorisation workgroup that is waiting for its block column (156 of 160 KB).
constexpr int kDfSmemUsed = 64 * kLdT + 4 * 64 * kPsD + 64 + 2 * 8 * kPsD + 4 * kDfXs;
constexpr int kDfSmem = 84 * 1024 / 8;
static_assert(kDfSmemUsed <= kDfSmem, "dataflow LDS layout");
static_assert(4 * 64 * kPsD + 64 + 4 * kDfXs >= 64 * kLd + 64, "the inverse's staging area must fit into the dead buffers");

struct DfArgs {
    LmCtl* ctl;
    double* S;
    int ld, n_pad, n_blk;
    double* dinv;
    double* Ld;
    double* Linv;
    unsigned long long* G;       // [n_blk (n_blk + 1) / 2][8][kDfSlice]
    const unsigned* epoch_word;  // bumped by the back-substitution chain that follows
    unsigned* abort_word;        // == epoch: some workgroup gave up waiting
    unsigned spin_limit;         // polls before a wait gives up (set per launch from LmCtl::spin_limit_df)
    const unsigned long long* nz;   // block structure of the factor: bit k of row i (kDfMaskWords words per row, up to 255
                                    // block columns) = L(i, k) may be non-zero (after fill); null: dense.  A workgroup then only
                                    // consumes the panels its row and column share, a structurally zero tile has no workgroup
                                    // and no slot for its slices (tree orderings)
    const unsigned char* order;     // with nz: [n_blk][kDfMaxBlk] the panels of block column j in the order they are expected
                                    // to be finished (a column of a separator takes the panels of the subtree that is done
                                    // first first, instead of waiting for panel 9 with panels 12-14 already there)
    const int32_t* wg;              // with nz: [gridDim.x][2] (block column, block row) of every workgroup, panel-major: the
                                    // non-zero blocks below the diagonal of a column (the right-hand side row last), then the
                                    // diagonal-only workgroup
    const int32_t* slot;            // with nz: [n_blk][n_blk + 1] slot of block (k, rb)'s slices in G, -1: structurally zero
    double* Gc;                     // BULK kernels: [slot][64 columns][64 rows] the block once more, as plain doubles, written when
    unsigned* done;                 // the workgroup is finished; done[slot] == epoch says so (release / acquire, agent scope)
};

// number of panels k < j that block column j of the factor has an entry in (dense: all of them)
__device__ __forceinline__ int df_num_panels(const DfArgs& a, const int j)
{
    if (!a.nz)
        return j;
    int n = 0;
#pragma unroll
    for (int w = 0; w < kDfMaskWords; ++w) {
        const int lo = 64 * w;
        if (j <= lo)
            break;
        const unsigned long long below = (j - lo >= 64) ? ~0ull : ((1ull << (j - lo)) - 1ull);
        n += __popcll(a.nz[kDfMaskWords * j + w] & below);
    }
    return n;
}

__device__ __forceinline__ double df_value(const unsigned long long lo, const unsigned long long hi)
{
    return __longlong_as_double((long long)(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull)));
}

#ifdef VMM_STAMPS
__device__ unsigned long long g_df_stamps[32][128];   // [block column][slot]: s_memrealtime (100 MHz) / s_memtime
#define DF_RT(slot)                                                                              \
    do {                                                                                         \
        if (stamp_on && lane == 0)                                                               \
            g_df_stamps[stamp_j][slot] = __builtin_amdgcn_s_memrealtime();                       \
    } while (0)
#define DF_CY(slot)                                                                              \
    do {                                                                                         \
        if (stamp_cy && lane == 0)                                                               \
            g_df_stamps[stamp_j][(slot) - stamp_off] = __builtin_amdgcn_s_memtime();             \
    } while (0)
extern "C" int vmm_ba_debug_read_df_stamps(unsigned long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_df_stamps), sizeof(unsigned long long) * 32 * 128);
}
#else
#define DF_RT(slot)
#define DF_CY(slot)
#endif

namespace df2 {

// chol8 (above) for the dataflow kernel: the block at D has row stride kPsD and is read two entries at a time; the
// validity test is off the chain altogether -- a non-positive or non-finite pivot gives NaN (v_rsq_f64 of a negative
// number, 0 * inf in the correction), every later entry of the factor inherits it, and ok is read off the last reciprocal
__device__ __forceinline__ void chol8_df(const double* __restrict__ D, Piv8& p)
{
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c <= r; c += 2) {
            const double2 v = *reinterpret_cast<const double2*>(D + r * kPsD + c);
            p.l[tri8(r, c)] = v.x;
            if (c + 1 <= r)
                p.l[tri8(r, c + 1)] = v.y;
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double t = p.l[tri8(j, j)];
        const double y0 = __builtin_amdgcn_rsq(t);
        const double e = fma(-t * y0, y0, 1.0);
        const double inv = fma(y0 * e, fma(e, 0.375, 0.5), y0);
        p.inv[j] = inv;
        p.l[tri8(j, j)] = t * inv;
#pragma unroll
        for (int i = j + 1; i < 8; ++i)
            p.l[tri8(i, j)] *= inv;
#pragma unroll
        for (int c = j + 1; c < 8; ++c)
#pragma unroll
            for (int i = c; i < 8; ++i)
                p.l[tri8(i, c)] = fma(-p.l[tri8(i, j)], p.l[tri8(c, j)], p.l[tri8(i, c)]);
    }
    p.ok = isfinite(p.inv[7]);
}

// tile tables: worker 0 = D lower tiles (row-major) + T(0,0..2); worker 1 = T(0,3) + T(1..3, 0..3)
__device__ __forceinline__ constexpr bool is_t(int wk, int i) { return wk == 0 ? i >= 10 : true; }
__device__ __forceinline__ constexpr int tile_i(int wk, int i)
{
    if (wk == 0)
        return i >= 10 ? 0 : (i >= 6 ? 3 : (i >= 3 ? 2 : (i >= 1 ? 1 : 0)));
    return i == 0 ? 0 : 1 + (i - 1) / 4;
}
__device__ __forceinline__ constexpr int tile_j(int wk, int i)
{
    if (wk == 0)
        return i >= 10 ? i - 10 : i - tile_i(0, i) * (tile_i(0, i) + 1) / 2;
    return i == 0 ? 3 : (i - 1) % 4;
}
// Round r factors columns J0 = 8 r .. J0 + 7 of the block column.  The pivot waves form the NEXT pivot block themselves
// (pivot_round: the 8x8 Gram product of the eight scaled rows below the pivot block), so what the pivot chain needs from
// the workers before it can scale its rows is: the columns of this round for all rows below the pivot block (the tiles of
// the pivot tile column tc = r >> 1) and the diagonal 8x8 block of round r + 1 as it is BEFORE this round's update (the
// Gram product is subtracted from it).  That block sits in the pivot tile for even r and in the next diagonal tile for
// odd r.
// Phase of tile i in the rank-8 update with the columns of round r - 1, applied during round r:
//   0  not touched (left of the pivot tile column; the diagonal tile of an odd round: what is left of it is the pivot
//      block the pivot waves compute themselves)
//   1  round 0 only: the tile that holds the first pivot block (one more barrier: the 8x8 Cholesky starts behind it)
//   2  needed by the pivot waves before they scale, then as many of the others as fit beside the 8x8 Cholesky
//   3  the others, beside the scaling
#ifndef VMM_DF_FILL2
#define VMM_DF_FILL2 4
#endif
constexpr int kFill2 = VMM_DF_FILL2;
__device__ __forceinline__ constexpr bool urgent_tile(int wk, int i, int r)
{
    const int tc = r >> 1, tj = tile_j(wk, i), ti = tile_i(wk, i);
    const bool diag = !is_t(wk, i) && ti == tj;
    if (tj == tc)
        return !(diag && (r & 1));
    return (r & 1) && diag && tj == tc + 1;
}
__device__ __forceinline__ constexpr int phase_of(int wk, int i, int r, bool has_t)
{
    if (is_t(wk, i) && !has_t)
        return 0;
    const int tc = r >> 1, tj = tile_j(wk, i), ti = tile_i(wk, i);
    const bool diag = !is_t(wk, i) && ti == tj;
    if (tj < tc || (tj == tc && diag && (r & 1)))
        return 0;
    if (urgent_tile(wk, i, r))
        return (r == 0 && diag) ? 1 : 2;
    // remaining tiles: fill phase 2 up to kFill2 tiles per worker: operand loads + 2 MFMAs per tile + the publication of
    // the urgent ones must end before the 8x8 Cholesky beside them does (~1100 cycles), or the pivot chain waits
    int n_urgent = 0, rank = 0;
    for (int k = 0; k < 13; ++k) {
        if (is_t(wk, k) && !has_t)
            continue;
        if (urgent_tile(wk, k, r))
            ++n_urgent;
        else if (tile_j(wk, k) >= tc && !(tile_j(wk, k) == tc) && k < i)
            ++rank;
    }
    return (n_urgent + rank < kFill2) ? 2 : 3;
}

struct Ops {   // MFMA operands of one k-step: A of the diagonal block's tile rows, A of the block below, B
    double ad[4], at[4], b[4];
};

// operands of the rank-8 update with the scaled columns in pd / pt (row-major, stride kPsD); rows < m are masked
template <int WK, bool HAS_T>
__device__ __forceinline__ void load_ops_panel(const double* pd, const double* pt, const int m, const int fr, const int fk,
                                               Ops (&o)[2])
{
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = 16 * t + fr;
            const double v = pd[row * kPsD + 4 * ks + fk];
            const double vm = (row >= m) ? v : 0.0;
            o[ks].b[t] = vm;
            o[ks].ad[t] = (WK == 0) ? -vm : 0.0;
            o[ks].at[t] = (HAS_T && (WK == 1 || t == 0)) ? -pt[row * kPsD + 4 * ks + fk] : 0.0;
        }
}

// operands from staged slices (k-major, stride kLdsRow)
template <int WK, bool HAS_T>
__device__ __forceinline__ void load_ops_slice(const double* XJ, const double* XR, const int fr, const int fk, Ops (&o)[2])
{
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int off = (4 * ks + fk) * kLdsRow + 16 * t + fr;
            const double v = XJ[off];
            o[ks].b[t] = v;
            o[ks].ad[t] = (WK == 0) ? -v : 0.0;
            o[ks].at[t] = (HAS_T && (WK == 1 || t == 0)) ? -XR[off] : 0.0;
        }
}

template <int WK, int I>
__device__ __forceinline__ void mfma_tile(double4_t (&acc)[13], const Ops (&o)[2])
{
    constexpr int ti = tile_i(WK, I), tj = tile_j(WK, I);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const double a = is_t(WK, I) ? o[ks].at[ti] : o[ks].ad[ti];
        acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, o[ks].b[tj], acc[I], 0, 0, 0);
    }
}

// columns cj..cj+7 of tile I -> the panel buffers (rows of the diagonal block -> pd, rows below -> pt)
template <int WK, int I>
__device__ __forceinline__ void publish_tile(const double4_t (&acc)[13], double* pd, double* pt, const int cj, const int fr,
                                             const int fk)
{
    constexpr int ti = tile_i(WK, I);
    if (fr >= cj && fr < cj + kPw) {
        double* dst = (is_t(WK, I) ? pt : pd) + (16 * ti + fk) * kPsD + (fr - cj);
        dst[0] = acc[I][0];
        dst[4 * kPsD] = acc[I][1];
        dst[8 * kPsD] = acc[I][2];
        dst[12 * kPsD] = acc[I][3];
    }
}

// 8x8 quadrant (QR, QC) of tile I -> dst (row stride kPsD): the first pivot block of a panel and the diagonal block the
// pivot waves subtract their Gram product from
template <int I, int QR, int QC>
__device__ __forceinline__ void publish_quadrant(const double4_t (&acc)[13], double* dst, const int fr, const int fk)
{
    if (fr >= 8 * QC && fr < 8 * QC + 8) {
        double* d = dst + fk * kPsD + (fr - 8 * QC);
        d[0] = acc[I][2 * QR];
        d[4 * kPsD] = acc[I][2 * QR + 1];
    }
}

// one phase of a worker in round R8 (columns 8 R8 ..): the tiles of that phase are updated (UPDATE: not in the first round
// of a panel, whose accumulators are complete); the tiles of the pivot tile column are published, and so are the first
// pivot block (round 0, -> pb) and the diagonal block of the next round before this round's update (-> nd)
template <int WK, bool HAS_T, int R8, int PHASE, bool UPDATE, int... Is>
__device__ __forceinline__ void worker_phase(double4_t (&acc)[13], const Ops (&o)[2], double* pd, double* pt, double* pb,
                                             double* nd, const int fr, const int fk, std::integer_sequence<int, Is...>)
{
    constexpr int tc = R8 >> 1;
    // all MFMAs of the phase first, the urgent tiles leading: a publication right behind its own tile's MFMAs would wait
    // for the matrix pipeline to drain once per tile
    auto upd = [&](auto idx, auto urgent_pass) {
        constexpr int I = decltype(idx)::value;
        constexpr bool U = decltype(urgent_pass)::value;
        if constexpr (UPDATE && phase_of(WK, I, R8, HAS_T) == PHASE && urgent_tile(WK, I, R8) == U)
            mfma_tile<WK, I>(acc, o);
    };
    (upd(std::integral_constant<int, Is>{}, std::true_type{}), ...);
    (upd(std::integral_constant<int, Is>{}, std::false_type{}), ...);
    auto pub = [&](auto idx) {
        constexpr int I = decltype(idx)::value;
        if constexpr (phase_of(WK, I, R8, HAS_T) == PHASE) {
            constexpr int ti = tile_i(WK, I), tj = tile_j(WK, I);
            constexpr bool diag = !is_t(WK, I) && ti == tj;
            if constexpr (tj == tc)
                publish_tile<WK, I>(acc, pd, pt, (8 * R8) & 15, fr, fk);
            if constexpr (diag && R8 == 0 && tj == 0)
                publish_quadrant<I, 0, 0>(acc, pb, fr, fk);
            if constexpr (diag && R8 < 7 && !(R8 & 1) && tj == tc)
                publish_quadrant<I, 1, 1>(acc, nd, fr, fk);
            if constexpr (diag && R8 < 7 && (R8 & 1) && tj == tc + 1)
                publish_quadrant<I, 0, 0>(acc, nd, fr, fk);
        }
    };
    (pub(std::integral_constant<int, Is>{}), ...);
}

template <int WK, bool HAS_T, int... Is>
__device__ __forceinline__ void worker_apply_slice(double4_t (&acc)[13], const Ops (&o)[2], std::integer_sequence<int, Is...>)
{
    auto one = [&](auto idx) {
        constexpr int I = decltype(idx)::value;
        if constexpr (HAS_T || !is_t(WK, I))
            mfma_tile<WK, I>(acc, o);
    };
    (one(std::integral_constant<int, Is>{}), ...);
}

using Seq13 = std::make_integer_sequence<int, 13>;

template <typename F, int... Is>
__device__ __forceinline__ void for_tiles(F&& f, std::integer_sequence<int, Is...>)
{
    (f(std::integral_constant<int, Is>{}), ...);
}

// a pivot wave's whole slice: sixteen granules per lane (lane = row)
struct SliceRegs {
    unsigned long long lo[8], hi[8];
};

__device__ __forceinline__ void issue_slice(const unsigned long long* sl, const int lane, SliceRegs& g)
{
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        g.lo[q] = __hip_atomic_load(sl + q * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g.hi[q] = __hip_atomic_load(sl + 512 + q * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ bool slice_valid(const SliceRegs& g, const unsigned epoch)
{
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        ok = ok && (unsigned)(g.lo[q] >> 32) == epoch && (unsigned)(g.hi[q] >> 32) == epoch;
    return ok;
}

// direct: the slice is expected any moment (the panel right before mine): sweep it again instead of probing one
// granule first
__device__ __forceinline__ bool wait_slice(const unsigned long long* sl, const int lane, const unsigned epoch,
                                           const unsigned* abort_word, const bool direct, SliceRegs& g,
                                           const unsigned kDfSpinLimit, bool* spun = nullptr)
{
    for (unsigned n = 0;;) {
        if (kDfSpinLimit != 1u && __all(slice_valid(g, epoch)))   // a limit of 1 (debugging) gives up even on valid data
            return true;
        if (spun)
            *spun = true;   // the first look came back stale: this slice was not there yet
        if (!direct) {
            for (;;) {
                const unsigned long long pv
                    = __hip_atomic_load(sl + 512 + 7 * 64 + 63, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((unsigned)(pv >> 32) == epoch)
                    break;
                if (++n >= kDfSpinLimit)
                    return false;
                if ((n & 63u) == 0u
                    && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch)
                    return false;
                __builtin_amdgcn_s_sleep(2);
            }
        } else {
            if ((n & 63u) == 63u
                && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch)
                return false;
            __builtin_amdgcn_s_sleep(1);
        }
        if (++n >= kDfSpinLimit)
            return false;
        issue_slice(sl, lane, g);
    }
}

// The slices a workgroup waits for while their producer is still at work (the panel right before mine).  A look at a slice
// is a round trip to the level the XCDs share (~1.1 us under this kernel's traffic) and the producer publishes one every
// ~0.85 us, so ONE look at a time cannot keep up: the look at slice s+1 must be on its way before slice s has been seen.
// Both the slice waited for (g) and the next one (gn, requested ahead by the caller) are looked at again each time their
// previous look comes back stale, alternately, so each is sampled once per round trip, half a round trip apart, and the
// next slice is usually complete in its registers when the current one has been staged.
// (Measured before: the copy requested two slices ahead was always stale, every slice then cost a fresh round trip after its
// predecessor, and each block column started 2.3 us behind the last slice of the previous one, 3 us with shorter rounds.)
__device__ __forceinline__ bool wait_slice_pair(const unsigned long long* sl, const unsigned long long* sl_next, const int lane,
                                                const unsigned epoch, const unsigned* abort_word, SliceRegs& g, SliceRegs& gn,
                                                const unsigned kDfSpinLimit, bool* spun = nullptr)
{
    for (unsigned n = 0;;) {
        if (kDfSpinLimit != 1u && __all(slice_valid(g, epoch)))   // a limit of 1 (debugging) gives up even on valid data
            return true;
        if (spun)
            *spun = true;
        if (++n >= kDfSpinLimit)
            return false;
        if ((n & 63u) == 63u && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch)
            return false;
        issue_slice(sl, lane, g);
        if (sl_next && !__all(slice_valid(gn, epoch)))
            issue_slice(sl_next, lane, gn);
    }
}

struct Lds {
    double* RA;     // D-only role: L^T (stride kLdT); others: result tile (stride kLd)
    double* Pd;     // [2][64][kPsD] panel columns of the diagonal block's rows (ping-pong between rounds)
    double* Pt;     // the same for the rows below
    double* invd;
    double* Pb;     // [8][kPsD] the pivot block of the current round (round 0: from the workers; then from the pivot waves)
    double* Nd;     // [8][kPsD] the diagonal block of the next round before this round's update (from the workers)
    double* Xs;     // [2 buffers][J | R][8][kLdsRow] staged slices of earlier panels
    int stamp_j;    // diagnostic build: block column whose (j, j+1) workgroup records time stamps (else -1)
};

struct SliceMap {
    unsigned long long* G;
    int n_blk;
    const int32_t* slot;   // tree orderings: [n_blk][n_blk + 1] slot of block (k, rb), only the non-zero blocks have one
    __device__ __forceinline__ int64_t index(int k, int rb) const
    {
        return slot ? (int64_t)slot[k * (n_blk + 1) + rb] : (int64_t)k * n_blk - (int64_t)k * (k - 1) / 2 + (rb - k - 1);
    }
    __device__ __forceinline__ unsigned long long* at(int k, int rb, int r) const
    {
        return G + (index(k, rb) * 8 + r) * kDfSlice;
    }
};

// ---- the pivot waves' program: sweeps during the earlier panels, then 8 x (8x8 Cholesky, scale rows, next pivot block) ----
// Barriers: one per consumed slice, then per round (A, round 0 only) B, C -- the same sequence as worker_path.
//   A  the first pivot block of the panel is in Pb (from the workers' accumulators)
//   B  all rows below the pivot block, columns J0..J0+7, are in pdc / ptc and the next diagonal block in Nd
//   C  the scaled columns are in pdc / ptc, the next pivot block in Pb
// The pivot chain is 8x8 Cholesky -> B -> scale the rows -> next pivot block = Nd - X X^T for the eight scaled rows X right
// below the pivot block (wave 0, lane = one entry of the block, the rows exchanged through pdc: same wave, no barrier)
// -> C -> 8x8 Cholesky; the workers' rank-8 update of the pivot tile column runs beside the 8x8 Cholesky instead of in
// front of it (until round 3 this was a third phase of ~640 cycles per round: MFMA update of the pivot tile, LDS, barrier).
template <int J0, bool HAS_T>
__device__ __forceinline__ void pivot_round(const int w, const int lane, const Lds& m, bool& ok, unsigned long long* gs,
                                            const unsigned epoch)
{
    double* pdc = m.Pd + ((J0 >> 3) & 1) * 64 * kPsD;
    double* ptc = m.Pt + ((J0 >> 3) & 1) * 64 * kPsD;
    const bool active = w == 0 || HAS_T;
#ifdef VMM_STAMPS
    const bool stamp_on = m.stamp_j >= 0 && w == 0;
    const bool stamp_cy = m.stamp_j >= 0;
    const int stamp_off = w == 0 ? 0 : 8;
    const int stamp_j = m.stamp_j;
#endif
    if (J0 == 0)
        __syncthreads();   // A: the first pivot block is in Pb
    if (J0 == 16) DF_CY(40);
    Piv8 p;
    if (active) {
        chol8_df(m.Pb, p);
        // the factor is complete BEFORE the barrier: left alone, the compiler sinks its arithmetic behind the barrier
        // and the 8x8 Cholesky no longer overlaps with the workers' phase 2 (measured with the stamps build)
#pragma unroll
        for (int k = 0; k < 36; ++k)
            asm volatile("" : "+v"(p.l[k]));
#pragma unroll
        for (int k = 0; k < 8; ++k)
            asm volatile("" : "+v"(p.inv[k]));
    }
    if (J0 == 16) DF_CY(41);
    __syncthreads();   // B: all rows of columns J0..J0+7 are in pdc / ptc, the next diagonal block in Nd
    if (J0 == 16) DF_CY(42);
    if (active) {
        double* row = (w == 0 ? pdc : ptc) + lane * kPsD;
        double x[8];
#pragma unroll
        for (int q = 0; q < 8; q += 2) {
            const double2 v = *reinterpret_cast<const double2*>(row + q);
            x[q] = v.x;
            x[q + 1] = v.y;
        }
        if (w == 1) {
            scale8(x, p);   // x = a L8^{-T}
            // the rows below leave for the other workgroups first (the longest latency of the round; holding them
            // back behind the barrier in all rounds but the last was measured slower) ...
            const unsigned long long tag = (unsigned long long)epoch << 32;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(x[q]);
                __hip_atomic_store(gs + q * 64 + lane, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(gs + 512 + q * 64 + lane, tag | (bits >> 32), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int q = 0; q < 8; q += 2)
                *reinterpret_cast<double2*>(row + q) = make_double2(x[q], x[q + 1]);
        } else {
            ok = ok && p.ok;
            // Wave 0 is the pivot chain.  The next pivot block: entry (gi, gj) = Nd - sum_q X[gi][q] X[gj][q] over the
            // scaled rows X = rows J0+8 .. J0+15, which lanes J0+8 .. J0+15 of this very wave produce (LDS operations of a
            // wave stay in order: no barrier).  Column q of a row is final after step q of the scaling, so it is written
            // and the two entries of it a lane needs are requested back right there: the LDS round trips run beside the
            // remaining steps instead of behind the last one.  Every lane writes its row -- rows up to the pivot block hold
            // nothing anybody reads (the workers mask them, load_ops_panel).
            constexpr bool NEXT = J0 + kPw < 64;
            const int gi = lane >> 3, gj = lane & 7;
            const double* xi = pdc + (J0 + kPw + gi) * kPsD;
            const double* xj = pdc + (J0 + kPw + gj) * kPsD;
            double sacc = NEXT ? m.Nd[gi * kPsD + gj] : 0.0;
            double vi[8], vj[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                x[q] *= p.inv[q];
#pragma unroll
                for (int c = q + 1; c < 8; ++c)
                    x[c] = fma(-x[q], p.l[tri8(c, q)], x[c]);
                row[q] = x[q];
                if (NEXT) {
                    vi[q] = xi[q];
                    vj[q] = xj[q];
                }
            }
#ifdef VMM_STAMPS
#pragma unroll
            for (int q = 0; q < 8; ++q)
                asm volatile("" : "+v"(x[q]));
            if (J0 == 16) DF_CY(56);
#endif
            if (NEXT) {
                if (J0 == 16) DF_CY(57);
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    sacc = fma(-vi[q], vj[q], sacc);
#ifdef VMM_STAMPS
                asm volatile("" : "+v"(sacc));
                if (J0 == 16) DF_CY(58);
#endif
                m.Pb[gi * kPsD + gj] = sacc;
            }
        }
        if (J0 == 16) DF_CY(43);
        __syncthreads();   // C: the scaled columns are in pdc / ptc, the next pivot block in Pb
        if (J0 == 16) DF_CY(44);
        DF_RT(2 + (J0 >> 3));
        // ... what only this workgroup's final write-back needs is stored behind the barrier, beside the next 8x8 Cholesky
        if (w == 1) {
            double* rr = m.RA + lane * kLd + J0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                rr[q] = x[q];
        } else if (!HAS_T) {
            // keep L^T for the write-back: x below the pivot block, the factor inside, zero above
            const int r = lane - J0;
            const bool below = r >= kPw, above = r < 0;
            double* At = m.RA;
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
                m.invd[lane] = iv;
            }
        }
    } else {
        __syncthreads();   // C (idle pivot wave of the diagonal-only role)
    }
}

// TREE: the factor has a block structure (DfArgs::nz, tree orderings): only the panels this block column depends on are
// consumed, in DfArgs::order.  !TREE is the dense kernel: panels 0 .. j-1 in ascending order.
// BULK: panels that are COMPLETE when this workgroup gets to them -- it works off a backlog: a separator column of a tree
// ordering, a late block column of a system with more workgroups than compute units -- are read from the producers' compact
// copies (DfArgs::Gc: plain doubles behind a completion word) instead of swept as granules: half the bytes and half the
// loads of a look, no validity test, two slices per register set, requested across panel boundaries.  A panel still in
// production is tracked through its granules as before; once a look has come back stale the workgroup has caught up
// with production and stops asking for completion words.  !BULK is the kernel of round 4, instruction for instruction.
// MODE bit 1 (HELP): the workgroup has six waves -- two more workers (waves 4, 5) on the pivot waves' SIMDs, which hold six of
// each worker's thirteen tiles while the EARLIER panels are applied (the pivot waves only sweep then: loads and integer
// work, nothing on the f64 pipe an MFMA of another wave would block) and hand them to the workers through the LDS right
// before the last slice, where they end.  A tile sees the same MFMAs in the same order whoever issues them: the same bits.
template <bool HAS_T, bool TREE, int MODE>
__device__ __forceinline__ void pivot_path(const DfArgs& a, const int w, const int lane, const int j, const int R,
                                           const Lds& m, const SliceMap& sm, const unsigned epoch, int* s_timeout, bool& ok)
{
    constexpr bool BULK = (MODE & 1) != 0, HELP = (MODE & 2) != 0;
    const int n_it = TREE ? 8 * df_num_panels(a, j) : 8 * j;   // a multiple of 8
    if (n_it > 0) {
        // Two slices are on their way at any time (two register sets): a slice read costs a round trip to the level all
        // XCDs share (~1.0-1.3 us) and with one request in flight that was the pace of a workgroup working off panels that are
        // long complete -- slower than they are produced since the rounds got shorter, so every block column started later
        // behind its predecessor than the one before
        SliceRegs ga, gb;
        const bool sweeper = w == 0 || HAS_T;
        const int my_rb = (w == 0) ? j : R;
        const unsigned char* const ord = TREE ? a.order + kDfMaxBlk * j : nullptr;
        // TREE: wave 1 sweeps the slices of block row R; where L(R, k) is structurally zero nobody publishes one -- zeros
        const bool mine_all = !TREE || w == 0 || R >= a.n_blk;
        // What a tree ordering keeps in tables in global memory -- which panel comes at position it >> 3 of this block column's
        // list, whether block row R has an entry in it, where block (k, my_rb) publishes its slices -- is looked up once per
        // PANEL (two panels are in use around a panel boundary), not once per slice: three dependent loads in front of every
        // request cost ~15 % of the slice rate.
        struct PanelInfo {
            int pos, k;
            bool has;
            unsigned long long* base;
        };
        PanelInfo c0{ -1, 0, false, nullptr }, c1{ -1, 0, false, nullptr };
        auto panel_at = [&](const int it) -> const PanelInfo& {
            const int pos = it >> 3;
            if (!TREE) {   // dense: panel `pos`, every block there, its place is arithmetic
                c0.pos = c0.k = pos;
                c0.has = true;
                c0.base = sm.at(pos, my_rb, 0);
                return c0;
            }
            if (pos == c0.pos)
                return c0;
            if (pos == c1.pos)
                return c1;
            c1 = c0;
            c0.pos = pos;
            c0.k = TREE ? (int)ord[pos] : pos;
            c0.has = mine_all || nz_bit(a.nz, R, c0.k);
            c0.base = c0.has ? sm.at(c0.k, my_rb, 0) : nullptr;
            return c0;
        };
        auto request = [&](const int it, SliceRegs& g) {
            if (sweeper && it < n_it) {
                const PanelInfo& pi = panel_at(it);
                if (pi.has)
                    issue_slice(pi.base + (it & 7) * kDfSlice, lane, g);
            }
        };
        // HELP: the helpers' tiles reach the workers behind one more barrier, right before the last slice
        auto help_before = [&](const int it) {
            if (HELP && it == n_it - 1)
                __syncthreads();
        };
        auto consume = [&](const int it, SliceRegs& g, SliceRegs& gn) {
            help_before(it);
            const PanelInfo pi = sweeper ? panel_at(it) : PanelInfo{ it >> 3, 0, true, nullptr };
            const int k = pi.k;
            const bool have = pi.has;
            if (sweeper) {
                // the panel expected last (dense: the one right before mine) is swept directly instead of probed
                const bool last_panel = TREE ? it + 8 >= n_it : k == j - 1;
                bool got = true;
                if (have && last_panel) {
                    // the next slice belongs to the same panel unless this is the panel's last one
                    const bool next_too = (it & 7) != 7;
                    unsigned long long* const sl = pi.base + (it & 7) * kDfSlice;
                    got = wait_slice_pair(sl, next_too ? sl + kDfSlice : nullptr, lane, epoch,
                                          a.abort_word, g, gn, a.spin_limit, nullptr);
                } else if (have) {
                    got = wait_slice(pi.base + (it & 7) * kDfSlice, lane, epoch, a.abort_word, false, g, a.spin_limit,
                                     nullptr);
                }
#ifdef VMM_STAMPS
                if (m.stamp_j >= 0 && w == 0 && lane == 0 && it >= n_it - 2)
                    g_df_stamps[m.stamp_j][12 + (it - (n_it - 2))] = __builtin_amdgcn_s_memrealtime();
                if (m.stamp_j >= 0 && w == 0 && lane == 0 && it >= n_it - 8)   // the last panel's slices, one by one
                    g_df_stamps[m.stamp_j][14 + (it - (n_it - 8))] = __builtin_amdgcn_s_memrealtime();
                if (m.stamp_j >= 0 && w == 1 && lane == 0 && it >= n_it - 8)
                    g_df_stamps[m.stamp_j][64 + (it - (n_it - 8))] = __builtin_amdgcn_s_memrealtime();
#endif
                double* X = m.Xs + (it & 1) * 2 * kDfXs + (w == 0 ? 0 : kDfXs);
                const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const double xv = got ? df_value(g.lo[q], g.hi[q]) : nan;
                    X[q * kLdsRow + lane] = (TREE && !have) ? 0.0 : xv;
                }
                if (!got && lane == 0) {
                    *s_timeout = 1;
                    __hip_atomic_store(a.abort_word, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __syncthreads();
#ifdef VMM_STAMPS
            if (m.stamp_j >= 0 && w == 0 && lane == 0 && it >= n_it - 8)
                g_df_stamps[m.stamp_j][80 + (it - (n_it - 8))] = __builtin_amdgcn_s_memrealtime();
#endif
        };
        if constexpr (!BULK) {
            request(0, ga);
            request(1, gb);
            for (int it = 0; it < n_it; it += 2) {
                consume(it, ga, gb);
                request(it + 2, ga);   // requested while the workers apply slice it
                consume(it + 1, gb, ga);
                request(it + 3, gb);
            }
        } else {
            const int n_pan = n_it >> 3;
            // one register set = two slices of a compact copy: lo[q] = column q of slice 2p, hi[q] = of slice 2p + 1
            auto issue_pair = [&](const double* cb, const int p, SliceRegs& g) {
                const unsigned long long* src = reinterpret_cast<const unsigned long long*>(cb) + p * 1024 + lane;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    g.lo[q] = __hip_atomic_load(src + q * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    g.hi[q] = __hip_atomic_load(src + 512 + q * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            };
            auto stage = [&](const int it, const unsigned long long (&v)[8]) {
                help_before(it);
                double* X = m.Xs + (it & 1) * 2 * kDfXs + (w == 0 ? 0 : kDfXs);
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    X[q * kLdsRow + lane] = __longlong_as_double((long long)v[q]);
                __syncthreads();
            };
            // Is block (k, my_rb)'s compact copy written?  The completion word of a panel is requested one panel ahead (at the
            // start of the panel in front of it), so that looking at it never waits: a panel that completes later than that is
            // taken through its granules like one that is still in production.
            auto flag_of = [&](const int pos, const double*& cb) -> unsigned {
                cb = nullptr;
                if (!sweeper || pos >= n_pan)
                    return epoch + 1u;
                const PanelInfo pi = panel_at(8 * pos);
                if (!pi.has)
                    return epoch + 1u;
                const int64_t si = sm.index(pi.k, my_rb);
                cb = a.Gc + si * 4096;
                return __hip_atomic_load(a.done + si, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            };
            bool pre = false;               // the coming panel's first two pairs are already in ga / gb
            const double* cb_cur = nullptr;
            const double* cb_next = nullptr;
            unsigned fl_next = flag_of(0, cb_next);
            for (int pos = 0; pos < n_pan; ++pos) {
                const int it0 = 8 * pos;
                const unsigned fl = fl_next;
                cb_cur = cb_next;
                fl_next = flag_of(pos + 1, cb_next);   // on its way while this panel is applied
                const bool bulk = pre || fl == epoch;
                if (bulk) {
                    if (!pre) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        issue_pair(cb_cur, 0, ga);
                        issue_pair(cb_cur, 1, gb);
                    }
                    pre = false;
                    stage(it0 + 0, ga.lo);
                    stage(it0 + 1, ga.hi);
                    issue_pair(cb_cur, 2, ga);
                    stage(it0 + 2, gb.lo);
                    stage(it0 + 3, gb.hi);
                    issue_pair(cb_cur, 3, gb);
                    stage(it0 + 4, ga.lo);
                    stage(it0 + 5, ga.hi);
                    const bool nbulk = fl_next == epoch;   // (requested eight slices ago)
                    if (nbulk) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        issue_pair(cb_next, 0, ga);
                    }
                    stage(it0 + 6, gb.lo);
                    stage(it0 + 7, gb.hi);
                    if (nbulk) {
                        issue_pair(cb_next, 1, gb);
                        pre = true;
                    }
                } else {
                    // granules: the panel is in production, structurally zero for my block row (zeros are staged), or this
                    // wave only keeps the barriers
                    request(it0, ga);
                    request(it0 + 1, gb);
#pragma unroll 1
                    for (int it = it0; it < it0 + 8; it += 2) {
                        consume(it, ga, gb);
                        if (it + 2 < it0 + 8)
                            request(it + 2, ga);
                        consume(it + 1, gb, ga);
                        if (it + 3 < it0 + 8)
                            request(it + 3, gb);
                    }
                }
            }
        }
    }
#ifdef VMM_STAMPS
    const bool stamp_on = m.stamp_j >= 0 && w == 0;
    const int stamp_j = m.stamp_j;
#endif
    DF_RT(1);
    unsigned long long* g0 = HAS_T ? sm.at(j, R, 0) : sm.G;
    pivot_round<0, HAS_T>(w, lane, m, ok, g0, epoch);
    pivot_round<8, HAS_T>(w, lane, m, ok, g0 + 1 * kDfSlice, epoch);
    pivot_round<16, HAS_T>(w, lane, m, ok, g0 + 2 * kDfSlice, epoch);
    pivot_round<24, HAS_T>(w, lane, m, ok, g0 + 3 * kDfSlice, epoch);
    pivot_round<32, HAS_T>(w, lane, m, ok, g0 + 4 * kDfSlice, epoch);
    pivot_round<40, HAS_T>(w, lane, m, ok, g0 + 5 * kDfSlice, epoch);
    pivot_round<48, HAS_T>(w, lane, m, ok, g0 + 6 * kDfSlice, epoch);
    pivot_round<56, HAS_T>(w, lane, m, ok, g0 + 7 * kDfSlice, epoch);
}

// ---- a worker wave's program ----
// SLICE (round 0 of a block column > 0 only): the "previous round" is the last slice of the previous panel, staged
// at XJ / XR and not applied yet -- its update of the first pivot tile column comes first like any round's, so the
// pivot waves start on the panel 2 MFMAs after the slice has arrived instead of 26 + a round.
template <int WK, int J0, bool HAS_T, bool SLICE = false>
__device__ __forceinline__ void worker_round(const int lane, double4_t (&acc)[13], const Lds& m, const double* XJ = nullptr,
                                             const double* XR = nullptr)
{
    static_assert(!SLICE || J0 == 0, "only the first round takes a slice");
    const int fr = lane & 15, fk = lane >> 4;
    constexpr int R8 = J0 >> 3;
    double* pdc = m.Pd + (R8 & 1) * 64 * kPsD;
    double* ptc = m.Pt + (R8 & 1) * 64 * kPsD;
    const double* pdp = m.Pd + ((R8 & 1) ^ 1) * 64 * kPsD;
    const double* ptp = m.Pt + ((R8 & 1) ^ 1) * 64 * kPsD;
    constexpr bool UPD = J0 > 0 || SLICE;
#ifdef VMM_STAMPS
    const bool stamp_cy = m.stamp_j >= 0;
    const int stamp_off = WK == 0 ? 0 : 24;
    const int stamp_j = m.stamp_j;
#endif
    Ops o[2];
    if (J0 == 16) DF_CY(48);
    if (SLICE)
        load_ops_slice<WK, HAS_T>(XJ, XR, fr, fk, o);
    else if (UPD)
        load_ops_panel<WK, HAS_T>(pdp, ptp, J0, fr, fk, o);
    if (J0 == 0) {
        worker_phase<WK, HAS_T, R8, 1, UPD>(acc, o, pdc, ptc, m.Pb, m.Nd, fr, fk, Seq13{});
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();   // A
        __builtin_amdgcn_sched_barrier(0);
    }
    worker_phase<WK, HAS_T, R8, 2, UPD>(acc, o, pdc, ptc, m.Pb, m.Nd, fr, fk, Seq13{});
    if (J0 == 16) DF_CY(49);
    // MFMAs touch no memory, so the compiler is free to sink them behind a barrier -- and did: the rest of a round's
    // update ran in front of the next round's urgent tiles, on the in-order matrix pipeline, ~700 cycles of every round
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // B
    __builtin_amdgcn_sched_barrier(0);
    if (J0 == 16) DF_CY(50);
    worker_phase<WK, HAS_T, R8, 3, UPD>(acc, o, pdc, ptc, m.Pb, m.Nd, fr, fk, Seq13{});
    if (J0 == 16) DF_CY(51);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // C
    __builtin_amdgcn_sched_barrier(0);
    if (J0 == 16) DF_CY(52);
}

constexpr int kHelpSplit = 7;   // HELP: a worker keeps its tiles 0..6 while earlier panels are applied, its helper holds 7..12

// one tile of a worker, straight from global memory in accumulator layout
template <int WK, int I, bool HAS_T>
__device__ __forceinline__ void load_tile(double4_t (&acc)[13], const double* __restrict__ S, const int ld, const int n_pad,
                                          const int K0, const int R0, const int fr, const int fk)
{
    constexpr int ti = tile_i(WK, I), tj = tile_j(WK, I);
    acc[I] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
    if constexpr (!is_t(WK, I)) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[I][r] = S[(int64_t)(K0 + 16 * ti + fk + 4 * r) * ld + K0 + 16 * tj + fr];
    } else if constexpr (HAS_T) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = R0 + 16 * ti + fk + 4 * r;
            const int grow = (row <= n_pad) ? row : n_pad;   // clamp: always in bounds
            const double tv = S[(int64_t)grow * ld + K0 + 16 * tj + fr];
            acc[I][r] = (row <= n_pad) ? tv : 0.0;
        }
    }
}

template <int WK, bool HAS_T, bool TREE, bool HELP = false>
__device__ __forceinline__ void worker_path(const DfArgs& a, const int lane, const int j, const int R, const Lds& m)
{
    const int fr = lane & 15, fk = lane >> 4;
    const int K0 = j * kNB, R0 = R * kNB;
    const int ld = a.ld, n_pad = a.n_pad;
    const double* __restrict__ S = a.S;
    const int n_it = TREE ? 8 * df_num_panels(a, j) : 8 * j;
    // accumulator tiles straight from global memory, in accumulator layout (HELP: the helper's tiles arrive later, unless
    // there is no earlier panel and hence no helper at work)
    double4_t acc[13];
    for_tiles([&](auto idx) {
        constexpr int I = decltype(idx)::value;
        if (!HELP || I < kHelpSplit || n_it == 0)
            load_tile<WK, I, HAS_T>(acc, S, ld, n_pad, K0, R0, fr, fk);
        else
            acc[I] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
    }, Seq13{});
    for (int it = 0; it + 1 < n_it; ++it) {
        const double* XJ = m.Xs + (it & 1) * 2 * kDfXs;
        const double* XR = XJ + kDfXs;
        __syncthreads();
        if (WK == 0 || HAS_T) {
            Ops o[2];
            load_ops_slice<WK, HAS_T>(XJ, XR, fr, fk, o);
            for_tiles([&](auto idx) {
                constexpr int I = decltype(idx)::value;
                if constexpr ((HAS_T || !is_t(WK, I)) && (!HELP || I < kHelpSplit))
                    mfma_tile<WK, I>(acc, o);
            }, Seq13{});
        }
#ifdef VMM_STAMPS
        if (m.stamp_j >= 0 && lane == 0 && it >= n_it - 8)
            g_df_stamps[m.stamp_j][(WK == 0 ? 72 : 88) + (it - (n_it - 8))] = __builtin_amdgcn_s_memrealtime();
#endif
    }
    if (n_it > 0) {
        if (HELP) {
            __syncthreads();   // the helper's tiles are in the LDS (the result tile's area, dead until the rounds)
            const double* M = m.RA + WK * (13 - kHelpSplit) * 256;
            for_tiles([&](auto idx) {
                constexpr int I = decltype(idx)::value;
                if constexpr (I >= kHelpSplit) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc[I][r] = M[((I - kHelpSplit) * 4 + r) * 64 + lane];
                }
            }, Seq13{});
        }
        const double* XJ = m.Xs + ((n_it - 1) & 1) * 2 * kDfXs;
        __syncthreads();   // the last slice is staged
        worker_round<WK, 0, HAS_T, true>(lane, acc, m, XJ, XJ + kDfXs);
    } else {
        worker_round<WK, 0, HAS_T>(lane, acc, m);
    }
    worker_round<WK, 8, HAS_T>(lane, acc, m);
    worker_round<WK, 16, HAS_T>(lane, acc, m);
    worker_round<WK, 24, HAS_T>(lane, acc, m);
    worker_round<WK, 32, HAS_T>(lane, acc, m);
    worker_round<WK, 40, HAS_T>(lane, acc, m);
    worker_round<WK, 48, HAS_T>(lane, acc, m);
    worker_round<WK, 56, HAS_T>(lane, acc, m);
}

// HELP: waves 4 and 5.  Worker WK's tiles kHelpSplit..12 from the start of the workgroup until the earlier panels are
// applied (all slices but the last one), then into the LDS for the worker, and out.
template <int WK, bool HAS_T, bool TREE>
__device__ __forceinline__ void helper_path(const DfArgs& a, const int lane, const int j, const int R, const Lds& m)
{
    const int n_it = TREE ? 8 * df_num_panels(a, j) : 8 * j;
    if (n_it == 0)
        return;   // no earlier panel: the workers hold all their tiles from the start
    const int fr = lane & 15, fk = lane >> 4;
    const int K0 = j * kNB, R0 = R * kNB;
    double4_t acc[13];
    for_tiles([&](auto idx) {
        constexpr int I = decltype(idx)::value;
        if constexpr (I >= kHelpSplit)
            load_tile<WK, I, HAS_T>(acc, a.S, a.ld, a.n_pad, K0, R0, fr, fk);
        else
            acc[I] = (double4_t){ 0.0, 0.0, 0.0, 0.0 };
    }, Seq13{});
    for (int it = 0; it + 1 < n_it; ++it) {
        const double* XJ = m.Xs + (it & 1) * 2 * kDfXs;
        const double* XR = XJ + kDfXs;
        __syncthreads();
        if (WK == 0 || HAS_T) {
            Ops o[2];
            load_ops_slice<WK, HAS_T>(XJ, XR, fr, fk, o);
            for_tiles([&](auto idx) {
                constexpr int I = decltype(idx)::value;
                if constexpr ((HAS_T || !is_t(WK, I)) && I >= kHelpSplit)
                    mfma_tile<WK, I>(acc, o);
            }, Seq13{});
        }
    }
    double* M = m.RA + WK * (13 - kHelpSplit) * 256;
    for_tiles([&](auto idx) {
        constexpr int I = decltype(idx)::value;
        if constexpr (I >= kHelpSplit) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                M[((I - kHelpSplit) * 4 + r) * 64 + lane] = acc[I][r];
        }
    }, Seq13{});
    __syncthreads();   // (the workers read behind this barrier; a wave that has ended no longer counts for the later ones)
}

// A give-up anywhere is a synchronisation failure, not an indefinite matrix: the pass pauses (LmCtl::done = 2) and the host
// redoes the factorisation without the dataflow.  EVERY workgroup reports for itself -- the one that gave up, and any that
// ends after somebody raised the abort word.  (Until round 3 only the last block column's workgroup did, on the grounds that
// it ends after everybody else; with a tree ordering of a kept family whose co-observation graph is not connected that is
// not true -- the last column depends on its own component only -- and a give-up in the other component went unreported.)
__device__ __forceinline__ void report_give_up(const DfArgs& a, const unsigned epoch, const int& s_timeout)
{
    if (threadIdx.x == 0
        && (s_timeout || __hip_atomic_load(a.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch))
        raise_sync_timeout(a.ctl, 1);
}

template <bool HAS_T, bool TREE, int MODE>
__device__ __forceinline__ void role(const DfArgs& a, const int j, const int R, double* smem)
{
    constexpr bool BULK = (MODE & 1) != 0, HELP = (MODE & 2) != 0;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K0 = j * kNB;
    const int R0 = R * kNB;
    const int n_blk = a.n_blk, ld = a.ld, n_pad = a.n_pad;
    if (TREE && HAS_T && R < n_blk && !nz_bit(a.nz, R, j))
        return;   // L(R, j) is structurally zero: nothing to compute, nothing to publish (its consumers know)
    const unsigned epoch = *a.epoch_word + 1u;
    Lds m;
    m.RA = smem;
    m.Pd = m.RA + 64 * kLdT;
    m.Pt = m.Pd + 2 * 64 * kPsD;
    m.invd = m.Pt + 2 * 64 * kPsD;
    m.Pb = m.invd + 64;
    m.Nd = m.Pb + 8 * kPsD;
    m.Xs = m.Nd + 8 * kPsD;
    m.stamp_j = -1;
#ifdef VMM_STAMPS
    if (TREE ? !HAS_T : (HAS_T && R == j + 1))   // tree orderings: the diagonal-only workgroup (block (j+1, j) may be empty)
        m.stamp_j = j;
    {
        const bool stamp_on = m.stamp_j >= 0 && w == 0;
        const int stamp_j = m.stamp_j;
        DF_RT(0);
    }
#endif
    double* Li = m.Pd;                       // diagonal factor, row stride kLd, for the block inverse: over the panel
    double* di = Li + 64 * kLd;              // and slice buffers (Pd, Pt, invd, Xs), dead after the last round
    __shared__ int s_timeout;
    if (tid == 0)
        s_timeout = 0;
    SliceMap sm;
    sm.G = a.G;
    sm.n_blk = n_blk;
    sm.slot = TREE ? a.slot : nullptr;
    __syncthreads();   // s_timeout
    bool ok = true;
    if (w < 2)
        pivot_path<HAS_T, TREE, MODE>(a, w, lane, j, R, m, sm, epoch, &s_timeout, ok);
    else if (w == 2)
        worker_path<0, HAS_T, TREE, HELP>(a, lane, j, R, m);
    else if (w == 3)
        worker_path<1, HAS_T, TREE, HELP>(a, lane, j, R, m);
    else {   // HELP only (six waves)
        if (w == 4)
            helper_path<0, HAS_T, TREE>(a, lane, j, R, m);
        else
            helper_path<1, HAS_T, TREE>(a, lane, j, R, m);
        return;
    }
    __syncthreads();   // the pivot waves store their rows of the result tile behind the last round's barrier
    // results for the kernels after this launch
    if (!HAS_T) {
        const double iv = tid < 64 ? m.invd[tid] : 0.0;   // invd is about to be overwritten by Li
        __syncthreads();
        if (tid < 64)
            a.dinv[K0 + tid] = iv;
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            const double v = (c <= r) ? m.RA[c * kLdT + r] : 0.0;
            if (c <= r)
                a.Ld[(int64_t)j * 4096 + r * 64 + c] = v;
            Li[r * kLd + c] = v;
        }
        if (tid < 64)
            di[tid] = iv;
        __syncthreads();
        if (j < n_blk - 1)   // the chain solves the last block directly
            chol_inverse_lds(Li, di, a.Linv + (int64_t)j * 4096);
        report_give_up(a, epoch, s_timeout);
        return;
    }
    for (int idx = tid; idx < 64 * 32; idx += 256) {
        const int rr = idx >> 5, c = (idx & 31) * 2;
        if (R0 + rr <= n_pad)
            *reinterpret_cast<double2*>(a.S + (int64_t)(R0 + rr) * ld + K0 + c)
                = make_double2(m.RA[rr * kLd + c], m.RA[rr * kLd + c + 1]);
    }
    if (BULK) {
        // the block once more for the workgroups that get to this panel when it is long complete: [column][row], what a
        // consumer stages slice by slice (the granules carried the same values), then the completion word -- every thread's
        // stores made visible (release at agent scope), then one thread says so
        double* cb = a.Gc + sm.index(j, R) * 4096;
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int c = idx >> 6, rr = idx & 63;
            cb[idx] = m.RA[rr * kLd + c];
        }
        __threadfence();
        __syncthreads();
        if (tid == 0)
            __hip_atomic_store(a.done + sm.index(j, R), epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (j == n_blk - 1 && tid == 0 && !ok)
        a.ctl->lin_fail = 1;   // (with a give-up the result is NaN-poisoned and `ok` says nothing: the pass is redone anyway)
    report_give_up(a, epoch, s_timeout);
}

} // namespace df2

template <bool TREE, int MODE>
__device__ __forceinline__ void chol_dataflow_body(DfArgs& a)
{
    if (a.ctl->done)
        return;
    a.spin_limit = (a.ctl->spin_limit_df && (a.ctl->spin_wg < 0 || a.ctl->spin_wg == (int)blockIdx.x)) ? a.ctl->spin_limit_df
                                                                                                          : kDfSpinDefault;
    phase_stamp(a.ctl, 3);
    if (a.ctl->lin_fail)
        return;
    __shared__ __attribute__((aligned(16))) double smem[kDfSmem];
    if (TREE) {
        // only the non-zero blocks of the factor have a workgroup (listed panel-major by the host)
        const int j = a.wg[2 * (int)blockIdx.x], R = a.wg[2 * (int)blockIdx.x + 1];
        if (R > j)
            df2::role<true, TREE, MODE>(a, j, R, smem);
        else
            df2::role<false, TREE, MODE>(a, j, j, smem);
        return;
    }
    int b = (int)blockIdx.x, j = 0;
    for (; j < a.n_blk; ++j) {
        const int cnt = a.n_blk - j + 1;
        if (b < cnt)
            break;
        b -= cnt;
    }
    if (j >= a.n_blk)
        return;
    if (b < a.n_blk - j)
        df2::role<true, TREE, MODE>(a, j, j + 1 + b, smem);
    else
        df2::role<false, TREE, MODE>(a, j, j, smem);
}

__global__ __launch_bounds__(256) void k_chol_dataflow(DfArgs a)
{
    chol_dataflow_body<false, 0>(a);
}

// the same launch with the compact-copy path of pivot_path (BULK) for dense systems: workgroups that are dispatched late (22 to
// 48 block columns, the 34-column tail of a large system) read the panels that are complete by then from their compact
// copies.  Not faster there (launch_dataflow), kept as the tested dense form of what the tree-ordered kernel uses
__global__ __launch_bounds__(256) void k_chol_dataflow_bulk(DfArgs a)
{
    chol_dataflow_body<false, 1>(a);
}

// the same launch for a factor with a block structure (DfArgs::nz / order: tree orderings of the kept family)
__global__ __launch_bounds__(256) void k_chol_dataflow_tree(DfArgs a)
{
    chol_dataflow_body<true, 1>(a);
}

// six waves per workgroup: two helper workers while earlier panels are applied (pivot_path, HELP)
__global__ __launch_bounds__(384) void k_chol_dataflow_tree_help(DfArgs a)
{
    chol_dataflow_body<true, 3>(a);
}

void launch_dataflow(Engine& e, double* S, int n_pad, int ld, LmCtl* ctl, int first_blk, int n_blk)
{
    DfArgs a;
    a.ctl = ctl;
    a.S = S + (int64_t)first_blk * kNB * (ld + 1);
    a.ld = ld;
    a.n_pad = n_pad - first_blk * kNB;
    a.n_blk = n_blk - first_blk;
    a.dinv = e.dinv + first_blk * kNB;
    a.Ld = e.Ldiag + (int64_t)first_blk * 4096;
    a.Linv = e.Linv + (int64_t)first_blk * 4096;
    a.G = e.df_gran;
    a.epoch_word = e.flags + 256;
    a.abort_word = e.flags + 257;
    a.spin_limit = 0;
    a.nz = (first_blk == 0 && e.chol_nz_on) ? e.chol_nz : nullptr;
    a.order = a.nz ? e.chol_order : nullptr;
    a.wg = a.nz ? e.df_wg : nullptr;
    a.slot = a.nz ? e.df_slot : nullptr;
    a.Gc = e.df_compact;
    a.done = e.df_done;
    // Dense systems: measured (MI355X, us per factorisation, granules only / compact copies): 24 block columns 278 / 295,
    // 30: 387 / 390, 38: 582 / 583, 47: 896 / 891, the 34-column tail at n = 6000: 3023 / 3041 -- a late workgroup there is
    // bound by its two worker waves (26 MFMAs per slice each), not by its sweeps; so only on request (VMM_BA_DF_BULK=1, tested).
    // Tree orderings (k_chol_dataflow_tree) always: 2000 x 1000 close-up 1004 -> 874 us, 500 x 200 close-up 205 -> 200.
    const bool bulk = e.df_compact && e.df_done && e.sw.df_bulk;
    // Helper waves (six waves per workgroup, the same bits): measured (MI355X, factorisation + solve, four / six waves) --
    // tree orderings: 2000 x 1000 close-up (109 block columns) 876 / 810 us, 500 x 200 close-up (22) 202 / 202, corridor
    // 120 / 124; dense: 19 block columns 226 / 238, 24: 281 / 294, 30: 389 / 410, 38: 582 / 617, 47: 892 / 954, the 34-column
    // tail at n = 6000 3042 / 3070.  So: large tree-ordered factors only (VMM_BA_DF_HELP=0 / 1 decides otherwise; the dense
    // kernels were measured with an instantiation that is not kept).
    const bool help = e.sw.df_help >= 0 ? e.sw.df_help == 1 : a.n_blk >= 64;
    if (a.nz && help)
        hipLaunchKernelGGL(k_chol_dataflow_tree_help, dim3(e.n_df_wg), dim3(384), 0, e.stream, a);
    else if (a.nz)
        hipLaunchKernelGGL(k_chol_dataflow_tree, dim3(e.n_df_wg), dim3(256), 0, e.stream, a);
    else if (bulk)
        hipLaunchKernelGGL(k_chol_dataflow_bulk, dim3(dataflow_workgroups(a.n_blk)), dim3(256), 0, e.stream, a);
    else
        hipLaunchKernelGGL(k_chol_dataflow, dim3(dataflow_workgroups(a.n_blk)), dim3(256), 0, e.stream, a);
}

int preload_chol_dataflow_kernels()
{
    hipFuncAttributes at;
    int bad = 0;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_chol_dataflow)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_chol_dataflow_bulk)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_chol_dataflow_tree)) != hipSuccess;
    bad += hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_chol_dataflow_tree_help)) != hipSuccess;
    return bad;
}

} // namespace vmm
