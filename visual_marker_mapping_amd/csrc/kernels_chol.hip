// Dense Cholesky factorisation + triangular solves of the reduced system (gfx950): which path factors what.
//
// Replaces the numeric Cholesky of the linear solver Ceres runs inside ceres::Solve for the reference
// (src/TagReconstructor.cpp:737-738; SPARSE_NORMAL_CHOLESKY / DENSE_QR by default, both exact).
//
// Matrix layout: row-major, leading dimension ld, only the lower block triangle is used.  Order
// n_pad = 64 * n_blk; the right-hand side is stored as ROW n_pad of the same array, so the blocked
// right-looking factorisation also performs the forward substitution (row n_pad ends as (L^-1 b)^T).
//
// Three paths, one source file each (what they share: chol_common.hpp):
//   * kernels_chol_dataflow.hip -- the whole factorisation in ONE launch (k_chol_dataflow and its bulk / tree / tree_help
//     forms): a workgroup per 64x64 block of the factor, the panels handed between workgroups as self-validating
//     granules.  Dense systems of up to 48 block columns, the last 33 or 34 block columns of a larger one of at most
//     n_cu block columns, and every tree-ordered factor (dataflow_blocks below);
//   * kernels_chol_step.hip -- one launch per block column (k_chol_step: panel, trailing update and the inverse of the
//     previous diagonal factor side by side) with its host schedule: the leading block columns of a large system, and
//     everything when a pass is redone without inter-workgroup waits (`safe`) or the dataflow kernels are switched off;
//   * kernels_backsolve.hip -- the back-substitution L^T y = w: ONE launch of n_blk workgroups handing their 64 unknowns
//     on through granules (k_backsolve_chain / k_backsolve_chain_tree, one body), or k_backsolve_step per block as the
//     fallback without waits.
// This file holds the host side that chooses between them: launch_cholesky_solve.
#include <algorithm>

#include "engine.hpp"

namespace vmm {

int dataflow_workgroups(int n_blk) { return n_blk * (n_blk + 1) / 2 + n_blk; }

// How many workgroups the one-launch factorisation may have.  Up to 48 block columns (1224 workgroups) -- more than the
// chip holds at one per CU.  Workgroups are panel-major; a tile only waits for lower-numbered workgroups and for the
// diagonal workgroup of its own column (fewer than n_blk + 1 <= n_cu numbers ahead), so with the in-order dispatch of
// the hardware the lowest unfinished workgroup always has its producers resident or finished and the launch drains with
// only a prefix resident.  HIP does not promise that order: the bounded spins and the redo of a pass that gave up
// waiting (k_chol_step) make a wrong guess slow, not wrong.  Measured (MI355X, us per factorisation, this kernel vs one
// k_chol_step launch per column): 24 blocks 328 vs 584, 30: 461 vs 744, 38: 701 vs 975, 47: 1097 vs 1232,
// 60: 1948 vs 1711, 94: 6254 vs 3713 -- hence 48.  VMM_BA_DF_MAX_WG overrides the limit (experiments).
int dataflow_max_workgroups(int n_cu, const Switches& sw)
{
    if (sw.df_max_wg > 0)
        return sw.df_max_wg;
    const int kMaxBlocks = 48;
    return n_cu > kMaxBlocks ? std::max(n_cu, dataflow_workgroups(kMaxBlocks)) : n_cu;
}

// How many of the LAST block columns of an n_blk-column system the one-launch kernel factors: all of them when it may
// (dataflow_max_workgroups), else a tail -- the launches of k_chol_step near the end are bound by their panel chain
// (~25-31 us per block column at n = 6000, whatever the trailing update costs) while the dataflow kernel needs ~14 us
// per column at 24 to 38 columns.  VMM_BA_CHOL_TAIL sets the tail length (0: none).
int dataflow_blocks(int n_blk, int n_cu, const Switches& sw)
{
    if (dataflow_workgroups(n_blk) <= dataflow_max_workgroups(n_cu, sw))
        return n_blk;
    int tail = sw.chol_tail >= 0 ? sw.chol_tail : 34;
    if (dataflow_workgroups(tail) > dataflow_max_workgroups(n_cu, sw) || n_blk > n_cu)
        return 0;
    tail = std::min(tail, n_blk - 2);
    return tail - ((n_blk - tail) & 1);   // the step launches come in pairs: an even number of them in front
}

void launch_cholesky_solve(Engine& e, double* S, int n_pad, int ld, double* y, LmCtl* ctl, bool safe)
{
    const int n_blk = n_pad / kNB;
    const bool chain = n_blk <= e.n_cu && e.flags && e.gran && !e.sw.no_chain && !safe;
    // a tree-ordered handle: the one-launch kernel whatever the size (only the non-zero blocks have workgroups)
    const int n_df = (chain && e.df_gran && !e.sw.no_dataflow) ? (e.chol_nz_on ? n_blk : dataflow_blocks(n_blk, e.n_cu, e.sw)) : 0;
    if (n_df == n_blk) {
        // one launch for the factorisation + forward substitution, one for the back-substitution chain (which
        // bumps the epoch both kernels tag their granules with)
        launch_dataflow(e, S, n_pad, ld, ctl, 0, n_blk);
        launch_backsolve_chain(e, S, n_pad, ld, y, ctl);
        return;
    }
    launch_chol_steps(e, S, n_pad, ld, ctl, n_df);
    if (n_df > 0)   // the trailing n_df x n_df blocks (+ right-hand side row) in one launch
        launch_dataflow(e, S, n_pad, ld, ctl, n_blk - n_df, n_blk);
    // one chained launch while every workgroup of the chain is certainly resident (one per CU); the per-block
    // kernels otherwise
    if (chain)
        launch_backsolve_chain(e, S, n_pad, ld, y, ctl);
    else
        launch_backsolve_steps(e, S, n_pad, ld, y, ctl);
}

// Touches every Cholesky kernel once (vmm_ba_create): the code object is loaded and the kernel's resources
// are known before any launch is recorded into a hipGraph (nothing may be loaded lazily under stream capture).
int preload_chol_kernels()
{
    return preload_chol_step_kernels() + preload_chol_dataflow_kernels() + preload_backsolve_kernels();
}

} // namespace vmm
