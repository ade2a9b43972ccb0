// Internal layout of the bundle-adjustment engine (host + device views).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/vmm_ba.h"
#include "geom.hpp"
#include "plan.hpp"

namespace vmm {

constexpr int kLdsRow = 80;        // LDS row stride (doubles) for 64-wide tiles: rows k, k+1 land in
                                   // opposite 32-bank halves for ds_read_b64 (MI355X_MICROARCH LDS)

// Observations sorted by one pose family ("own"); SoA so that lane = observation is coalesced.
struct ObsOrder {
    int64_t n = 0;          // observations
    int64_t n_pad = 0;      // SoA stride (multiple of 64)
    int32_t* own = nullptr;     // [n] pose index in the sorted family
    int32_t* other = nullptr;   // [n] pose index in the other family
    int32_t* caller = nullptr;  // [n] position in the caller's observation order
    double* px = nullptr;       // [8][n_pad]
    Task* tasks = nullptr;
    int32_t n_tasks = 0;
    int32_t* pose_task = nullptr;  // [n_pose+1] task range per pose
    double* part = nullptr;        // [n_tasks][kPart]
    int32_t* start = nullptr;      // [n_pose+1] observation range per pose
};

// Device control block of the trust-region loop (Ceres TrustRegionMinimizer +
// LevenbergMarquardtStrategy state).  Lives in device memory; the host only polls it.
struct LmCtl {
    // options (copied at solve start)
    int32_t max_num_iterations, robustify, jacobi_scaling, max_invalid;
    double huber_a, function_tolerance, gradient_tolerance, parameter_tolerance;
    double max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
    // strategy
    double radius, decrease_factor;
    int32_t reuse_diagonal, num_invalid;
    // minimizer
    double x_cost, cand_cost, model_cost_change, x_norm, initial_cost;
    int32_t iteration;         // index of the iteration record being built
    int32_t first_eval;        // the pending evaluation is iteration zero
    int32_t done, termination; // done: 0 = running, 1 = the loop is over, 2 = paused: this pass's factorisation gave up
                               // waiting on another workgroup (sync_timeout), the host redoes it on the launch-per-
                               // block-column path and resumes (every kernel of a pass returns at once while done != 0)
    int32_t lin_fail;          // a Cholesky pivot was not positive in this iteration (numerical failures ONLY)
    // Spin give-ups of the two one-launch kernels that hand data between workgroups.  They are NOT numerical
    // failures: the trust-region policy never sees them.  sync_timeout: bit 0 k_chol_dataflow, bit 1
    // k_backsolve_chain, bit 2 another rank reported one (world > 1) -- of the pass that paused; the host clears it.
    int32_t sync_timeout;
    int32_t num_sync_timeouts; // passes of this solve redone on the fallback path
    int32_t sync_kernels;      // OR of sync_timeout over the solve
    uint32_t spin_limit_df, spin_limit_chain;   // 0 = the kernels' defaults (VMM_BA_DEBUG_SPIN_LIMIT shrinks them)
    int32_t spin_wg;           // debugging: the shrunk limit applies to this workgroup (blockIdx.x) only; < 0: to all
    int32_t records;           // trace rows pushed (== Ceres summary.iterations.size())
    int32_t num_successful, num_unsuccessful, num_lm_iterations, num_jac_evals, num_cost_evals;
    int32_t trace_capacity;
    int32_t w_which;           // which copy of W and of the small blocks (H, g) belongs to x; the evaluation at the
                               // candidate writes the other one and an accepted step flips this
    vmm_ba_iteration cur;      // record under construction
    // phase report (vmm_ba_summary.time_*_s): s_memrealtime (100 MHz) stamps written by thread 0 of the first
    // kernel of each group -- 0 evaluation at the candidate, 1 unused, 2 k_form_z, 3 Cholesky, 4 k_backsub, 5 k_control --
    // and their differences accumulated per solve: 0 evaluation, 1 control, 2 eliminate + rank-k update,
    // 3 factor + triangular solves, 4 step (back-substitution, candidate, cost at the candidate)
    unsigned long long stamp[6];
    unsigned long long phase_ticks[5];
};

// Offset (doubles) of the copy of the small blocks that belongs to x.
__device__ __forceinline__ int64_t small_sel(const LmCtl* ctl, const int64_t alt_off) { return ctl->w_which ? alt_off : 0; }

// Start-of-group stamp by one thread of the launch (costs one s_memrealtime + one 8-byte store).
__device__ __forceinline__ void phase_stamp(const LmCtl* ctl, int slot)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        const_cast<LmCtl*>(ctl)->stamp[slot] = __builtin_amdgcn_s_memrealtime();
}

// Stream-K decomposition of the rank-k update (kernels_schur.hip): device arrays + sizes.
struct SyrkPlan {
    int n_tiles = 0, n_kt = 0, n_wg = 0, n_segments = 0;
    int32_t *tile_bi = nullptr, *tile_bj = nullptr, *wg_seg0 = nullptr, *tile_seg0 = nullptr;
    int64_t *wg_u0 = nullptr, *wg_u1 = nullptr;   // [n_wg] unit range of each workgroup (by blockIdx)
    double* partials = nullptr;   // [n_segments][kST*kST]
    bool wide = false;            // k_syrk_wide: one 8-wave workgroup per CU, one tile per workgroup (few tiles)
};

struct Engine {
    int device = 0;
    int n_cu = 256;                 // compute units of the device (workgroup counts of the persistent loops)
    hipStream_t stream = nullptr;
    int rank = 0, world = 1;
    Switches sw;                    // environment switches, read at create (read_switches)
    bool multi = false;             // world > 1 (or forced for tests): staging buffers, eager launches, all-reduces
    vmm_ba_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    void* rccl_comm = nullptr;      // ncclComm_t of vmm_ba_enable_rccl: the all-reduces are ncclAllReduce on `stream`
    bool rccl_graph = true;         // ... recorded into the iteration's hipGraph (VMM_BA_RCCL_GRAPH=0: enqueued between graphs)

    Intrinsics K;
    int n_cams = 0, n_tags = 0, fixed_tag = -1;
    // point landmarks (VMM_BA_LANDMARK_POINTS): the "tag" family holds 2 * n_tags_user point pairs, the observation
    // arrays 2 * n_obs_user pair observations; fixed_tag stays the caller's tag index (block >> 1 is compared)
    bool points = false;
    int n_tags_user = 0;
    int64_t n_obs_user = 0;
    std::vector<double> user_tag_wh;   // [2 * n_tags_user]: vmm_ba_set_state turns tag poses into corners again
    int64_t n_obs = 0;
    bool elim_cams = true;          // eliminated family E = cameras (else tags)
    int n_e = 0, n_f = 0;           // pose counts of the eliminated / kept family

    // poses: cameras then tags, 7 doubles each
    double* cam_qt = nullptr;
    double* tag_qt = nullptr;
    double* cam_cand = nullptr;
    double* tag_cand = nullptr;
    double* tag_wh = nullptr;

    ObsOrder ordE, ordF;            // observations sorted by the eliminated / kept family

    // normal-equation blocks ("small" buffer, contiguous for one all-reduce):
    //   H_cam[36*n_cams] | H_tag[36*n_tags] | g_cam[6*n_cams] | g_tag[6*n_tags] | cost | pad
    double* small = nullptr;
    size_t small_count = 0;
    double *H_cam = nullptr, *H_tag = nullptr, *g_cam = nullptr, *g_tag = nullptr, *cost_slot = nullptr;
    // where the evaluation kernels write (== the pointers above on one GPU, a staging copy that is
    // all-reduced first when world > 1)
    double* small_stage = nullptr;
    // one GPU: the staging copy IS the second copy of the small blocks (offset from `small` in doubles; kernels add it
    // when LmCtl::w_which is set); world > 1: 0 -- the all-reduced staging copy is copied into `small` on acceptance
    int64_t small_alt_off = 0;
    double *ev_H_cam = nullptr, *ev_H_tag = nullptr, *ev_g_cam = nullptr, *ev_g_tag = nullptr, *ev_cost = nullptr;
    double* ev_pose_cost = nullptr;   // [n_e] behind the staging copy: per-pose costs of the evaluation (world > 1)
    double* W = nullptr;            // [36][ordE.n_pad]: J_e^T J_f per observation, E order (f64 precision)
    double* W2 = nullptr;           // second buffer: every LM iteration evaluates at the candidate, LmCtl::w_which says
                                    // which one belongs to x
    float* Wf2 = nullptr;
    uint8_t* obs_mask = nullptr;    // [n_obs] caller order, 1 = observation active (vmm_ba_set_observation_mask)
    // [n_cams + n_tags] cameras then landmark blocks, non-zero = the pose is held constant: the evaluation zeroes its
    // Jacobian columns, the initialisation starts from it.  Holds the problem's fixed_tag from create on;
    // vmm_ba_set_constant_poses adds the caller's flags (point landmarks: both pair blocks of a constant tag)
    uint8_t* pose_const = nullptr;
    bool any_const = false;         // some pose is constant: vmm_ba_initialize has a seed
    float* Wf = nullptr;            // the same in f32 (VMM_BA_PRECISION_F32_ACCUM); exactly one of the two exists
    bool f32_accum = false;

    // Fused evaluation (k_eval_fused): one evaluation per observation, lane = kept pose, the wave walks `fused_group`
    // eliminated poses.  On when most (e, f) pairs are observed (VMM_BA_EVAL=fused|twopass overrides).
    bool fused_eval = false;
    int32_t* pair_obs = nullptr;      // [n_e][fused_f_pad]
    int32_t* fused_e_list = nullptr;  // [fused_n_e_act] eliminated poses with observations
    int32_t* fused_e_part0 = nullptr; // [n_e] first partial of each eliminated pose
    int32_t* fused_pose_task = nullptr;   // [n_e + 1] partial range per eliminated pose (k_reduce_pose)
    double* fused_partE = nullptr;    // [fused_n_e_act * fused_chunks][kPart]
    double* fused_partF = nullptr;    // [fused_groups][28][fused_f_pad]
    int fused_n_e_act = 0, fused_f_pad = 0, fused_chunks = 0, fused_group = 1, fused_groups = 0;

    // tangent-space vectors, cameras first then tags (6 each)
    double *scale = nullptr, *diag = nullptr, *D2 = nullptr, *delta = nullptr;
    int32_t* active = nullptr;      // per pose (cameras then tags)

    // elimination
    double* Le = nullptr;           // [n_e][36] Cholesky factors of the damped E blocks
    double* ze = nullptr;           // [n_e][6]  L_e^{-1} g_e
    double* Z = nullptr;            // [k_pad][ldz] dense L_e^{-1} W (+ z column), row-major
    int k_dim = 0, k_pad = 0;
    int n_red = 0, n_pad = 0, ldz = 0, n_blk = 0;   // reduced order, padded, leading dim, blocks
    // Block-sparse elimination (kernels_schur.hip: k_schur_pairs): Z holds only the 6x6 blocks of co-observed (e, f) pairs and
    // S -= Z^T Z runs over pairs that share an eliminated pose.  Chosen at create by a cost model (VMM_BA_SCHUR=
    // dense|sparse overrides): at full visibility the dense MFMA rank-k update is the faster one.
    bool sparse_schur = false;
    double* Zc = nullptr;           // [n_obs][36]: one column-major 6x6 block per observation, E order
    int32_t* f2e = nullptr;         // [n_obs] F-order position -> E-order position of the same observation
    // the symbolic structure of S -= Z^T Z (built once at create): pairs of kept poses (row f: f' = 0..f, then the rhs),
    // the terms of every pair, and the work items of k_schur_pairs (row | first pair; up to 42 pairs of one row each)
    int32_t* pair_start = nullptr;  // [n_f + 1]
    int32_t* pair_tstart = nullptr; // [n_pairs + 1]
    int32_t* pair_terms = nullptr;  // [n_terms][2] position of the left block in the row's observation list | E-order
                                    // index of the right block (rhs pair: the eliminated pose)
    int32_t* row_items = nullptr;   // [2][n_row_items]
    double co_terms = 0.0;          // sum over the eliminated poses of (observations)^2: size of the host's pair bookkeeping
    bool explicit_pairs = false;    // only the pairs that share an eliminated pose are listed (pair_col), S zero-filled first
    int32_t* pair_col = nullptr;    // [n_pairs] first column of the pair's block in S (-1: the row's right-hand side entry)
    int32_t* row_of = nullptr;      // [n_f] first row of every kept pose in the reduced system (explicit form only)
    int32_t* pose_of_row = nullptr; // [n_pad] world > 1 with a tree ordering: kept pose of a row of the reduced system, -1: padding
    std::vector<int32_t> h_row_of;  // host copy; empty: kept pose f sits at row 6 f
    unsigned long long* chol_nz = nullptr;    // [n_blk + 1][kDfMaskWords] block structure of the factor (tree ordering), see DfArgs::nz
    unsigned char* chol_order = nullptr;      // [n_blk][kDfMaxBlk] panel order per block column, see DfArgs::order
    int32_t* df_wg = nullptr;                 // [n_df_wg][2] (block column, block row) of the tree-ordered launch's workgroups
    int32_t* df_slot = nullptr;               // [n_blk][n_blk + 1] slot of a block's slices in df_gran, -1: structurally zero
    int n_df_wg = 0;
    size_t df_tree_slots = 0;                 // blocks with published slices under the tree ordering
    bool chol_nz_on = false;                  // off while a call factors the dense, naturally ordered system (covariance)
    std::vector<int32_t> nd_node_first_blk;   // tree ordering: first 64-row block of every node, in elimination order
    int n_row_items = 0;
    double schur_flops = 0.0;       // algorithmic flops of the reduced-system formation on the path in use
    double chol_flops = 0.0;        // tree-ordered factor: flops over its non-zero blocks (0: dense factor)
    SyrkPlan syrk;                  // stream-K plan of S = Z^T Z
    double* S = nullptr;            // [ldz][ldz] reduced system (lower) + rhs row at n_pad
    double* S_packed = nullptr;     // world > 1: rows 0..n_pad of the lower triangle, packed, for the all-reduce
    double* P = nullptr;            // [4][kNB][ldz] transposed Cholesky panels (ring: panel k in slot k & 3)
    double* P4[4] = { nullptr, nullptr, nullptr, nullptr };
    double* dinv = nullptr;         // [ldz] reciprocals of the Cholesky diagonal
    double* Ldiag = nullptr;        // [n_blk][64][64] Cholesky factors of the diagonal blocks
    double* Linv = nullptr;         // [n_blk][64][64] their inverses (all but the last block)
    unsigned* flags = nullptr;      // [256] unused | epoch word | abort word | two tile counters of k_chol_step | agreement word
    unsigned long long* gran = nullptr;   // [2 * ld] {epoch, 32 value bits} granules of the chain's hand-offs
    unsigned long long* df_gran = nullptr;   // published 64x8 slices of the dataflow factorisation: [slot][8][kDfSlice], DfArgs::G
    double* df_compact = nullptr;            // the same blocks once they are COMPLETE, as plain doubles [slot][column][row]
    unsigned* df_done = nullptr;             // [slot] == factorisation epoch: the block's compact copy is written
    double* yf = nullptr;           // [ldz] solution of the reduced system (scaled coordinates)
    double* step_comm = nullptr;    // [7*n_e + 1]: delta of the eliminated family | per-pose cross terms | votes
    double* cost_comm = nullptr;    // [2] candidate cost (all-reduced)
    double* part_cost = nullptr;    // [ordE.n_tasks]
    double* part_cross = nullptr;   // [ordE.n_tasks] cross-term wave partials
    double* part_k1 = nullptr;      // [ordE.n_tasks] candidate-cost wave partials
    double* pose_part = nullptr;    // [n_pose][5] per-pose terms of the step decision
    double* pose_gm = nullptr;      // [n_pose] per-pose gradient max-norm terms of the evaluation at the candidate

    // reprojection statistics (vmm_ba_reprojection_stats): per-task partials, per-pose sums | counts
    double* stats_part = nullptr;   // [n_tasks by camera + n_tasks by tag]
    int32_t* stats_cnt = nullptr;   // same layout: active observations per task
    double* stats_pose = nullptr;   // [2 * (n_cams + n_tags)]
    double* stats_corner = nullptr; // [8 * n_obs], allocated by the first call that asks for per-corner errors

    // vmm_ba_initialize (kernels_init.hip), allocated by the first call
    double* init_quad_qt = nullptr;   // [14 * n_obs] both planar tag->camera poses per observation, caller's order
    double* init_quad_rms = nullptr;  // [2 * n_obs] their RMS reprojection errors (+inf: unusable)
    int32_t* init_placed = nullptr;   // [n_cams + n_tags] pose has been placed (cameras first)
    int32_t* init_todo = nullptr;     // [n_cams + n_tags] k_init_score -> k_init_refine
    int32_t* init_counter = nullptr;  // poses placed in the current round
    double* init_stats = nullptr;     // [2 + 2 * n_cams] sum of the corner errors | corners | the same per camera
    double* init_host = nullptr;      // pinned, 4 doubles: the round's counter and the statistics as the host reads them

    LmCtl* ctl = nullptr;           // device
    LmCtl* ctl_host = nullptr;      // pinned
    // vmm_ba_set_state: the caller's poses are staged here (pinned) and copied on the stream without waiting for it
    double* pose_stage = nullptr;   // [7 * (n_cams + n_tags)]
    hipEvent_t pose_ev = nullptr;   // recorded behind the copies: the staging buffer is free again
    bool pose_ev_pending = false;
    double* pose_stage_dev = nullptr;   // the staging buffer as the device sees it (k_begin_loop reads it directly)
    bool dirty_cam = false, dirty_tag = false;   // staged by vmm_ba_set_state, not yet on the device
    vmm_ba_iteration* trace = nullptr;  // device
    int trace_capacity = 0;

    // one LM iteration captured as a hipGraph (single GPU; collectives are host calls)
    hipGraphExec_t iter_graph = nullptr;
    hipGraphExec_t iter_graph_seg[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };   // world > 1: the groups between the all-reduces
    int graph_robustify = -1;
    double graph_huber_a = 0.0;
    int last_passes = 1;            // passes the last run_iteration enqueued (sw.graph_passes per graph; 2 measured best)
    bool launched_eagerly = false;

    std::vector<void*> allocs;
};

void set_error(const std::string& s);

__host__ __device__ inline Intrinsics make_intrinsics(const double intr[4], const double dist[5])
{
    Intrinsics K;
    K.fx = intr[0]; K.fy = intr[1]; K.cx = intr[2]; K.cy = intr[3];
    K.k1 = dist[0]; K.k2 = dist[1]; K.p1 = dist[2]; K.p2 = dist[3]; K.k3 = dist[4];
    return K;
}
// the nine numbers in one array (fx, fy, cx, cy, k1, k2, p1, p2, k3), as CalibCtl holds them
__host__ __device__ inline Intrinsics make_intrinsics(const double k[9]) { return make_intrinsics(k, k + 4); }

// The device memory of an entry point that works without a handle: one allocation, released on every way out, and the
// first HIP error of the steps made through it -- after a failure the later copies are skipped.  The pieces are
// described once, by a function that takes them in order: layout() runs it without memory to learn the size, allocates,
// and runs it again to hand out the pointers.
struct Arena {
    char* base = nullptr;
    size_t used = 0;
    hipError_t err = hipSuccess;
    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    ~Arena()
    {
        if (base)
            (void)hipFree(base);
    }
    hipError_t alloc(size_t bytes)
    {
        err = hipMalloc((void**)&base, bytes);
        if (err != hipSuccess)
            base = nullptr;
        return err;
    }
    static size_t round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    template <typename T>
    T* take(size_t count)   // the next 256-byte aligned piece (null while layout() is sizing)
    {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += round(count * sizeof(T));
        return p;
    }
    template <typename Carve>
    hipError_t layout(Carve&& carve)
    {
        carve(*this);
        const size_t total = used;
        used = 0;
        if (alloc(total) == hipSuccess)
            carve(*this);
        return err;
    }
    // blocking, on the null stream: ordered with the kernels launched there
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
    {
        if (err == hipSuccess)
            err = hipMemcpy(dst, src, bytes, kind);
    }
};

// one per .hip file: hipFuncGetAttributes on every kernel (returns the number of failures)
int preload_eval_kernels();
int preload_schur_kernels();
int preload_chol_kernels();
int preload_lm_kernels();
int preload_cov_kernels();
int preload_init_kernels();

// ---- kernel launchers (defined in the .hip files) ----
// kernels_eval.hip
void launch_eval_passes(Engine& e, int robustify, double huber_a, bool use_ctl);
void launch_cost_kernel(Engine& e, const double* cam, const double* tag, bool guard, int robustify, double huber_a);
void launch_cost(Engine& e, const double* cam, const double* tag, bool guard, int robustify, double huber_a,
                 double* out_scalar);
void launch_stats(Engine& e, double* per_corner_dev);
void launch_project(hipStream_t st, const Intrinsics& K, int64_t n, const double* pc, double* uv);
void launch_sum(Engine& e, bool guard, const double* in, int n, double* out);
// kernels_schur.hip
void launch_elim(Engine& e);
void launch_schur_rows(Engine& e, bool add_diag);   // block-sparse: S from the pair lists (k_schur_pairs)
void launch_syrk_only(Engine& e);
void launch_syrk_reduced(Engine& e);
void launch_pack_lower(Engine& e, bool unpack);
void launch_syrk_plan(hipStream_t st, const LmCtl* ctl, const double* Z, int ldz, const SyrkPlan& p);
void launch_reduce_plan(hipStream_t st, const LmCtl* ctl, const SyrkPlan& p, int ld, int n_rows, double* S);
// kernels_chol.hip: which path factors what
// safe: the launch-per-block-column factorisation and the per-block back-substitution (no workgroup waits on another)
void launch_cholesky_solve(Engine& e, double* S, int n_pad, int ld, double* y, LmCtl* ctl, bool safe = false);
int dataflow_workgroups(int n_blk);   // workgroups of the dense one-launch factorisation of n_blk block columns
int dataflow_max_workgroups(int n_cu, const Switches& sw);
int dataflow_blocks(int n_blk, int n_cu, const Switches& sw);   // trailing block columns factored by k_chol_dataflow (n_blk: all; 0: none)
// kernels_chol_step.hip
void launch_chol_inverse(Engine& e, int k);
struct CholLaunch {   // one k_chol_step launch of the launch-per-column factorisation
    int k;            // block column its panel workgroups factor; -1: the update-only hand-over launch
    int lazy[2];      // panels those workgroups first apply to their own column (older first; -1: none)
    int upd[2];       // panels of the launch's trailing update (-1: none; both: rank-128)
    int c0, t0, t1;   // first block column of the update's tile list, and the range of that list this launch takes
};
std::vector<CholLaunch> chol_step_schedule(int n_blk, int n_df);
void chol_schedule_tile(int n_blk, const CholLaunch& L, int t, int* bi, int* bj);
void launch_chol_steps(Engine& e, double* S, int n_pad, int ld, LmCtl* ctl, int n_df);   // the schedule's launches
int preload_chol_step_kernels();
// kernels_chol_dataflow.hip: block columns first_blk .. n_blk-1 (+ the right-hand side row) in one launch
void launch_dataflow(Engine& e, double* S, int n_pad, int ld, LmCtl* ctl, int first_blk, int n_blk);
int preload_chol_dataflow_kernels();
// kernels_backsolve.hip
void launch_backsolve_chain(Engine& e, double* S, int n_pad, int ld, double* y, LmCtl* ctl);   // one launch
void launch_backsolve_steps(Engine& e, double* S, int n_pad, int ld, double* y, LmCtl* ctl);   // one launch per block
int preload_backsolve_kernels();
// kernels_cov.hip
void launch_cov_prepare(Engine& e);
void launch_cov_rhs(Engine& e, double* B, int ldb, bool identity_rhs);
void launch_cov_trsm(Engine& e, double* B, int ldb, int n_chunks, bool identity_rhs);
void launch_cov_gram(Engine& e, const double* X, int ldb, double* cov_dev);
void launch_cov_rhs_slots(Engine& e, const int32_t* slot_src, int n_slots, double* B, int ldb);
void launch_cov_trsm_mfma(Engine& e, double* B, int ldb, const std::vector<int>& chunks_at);
void launch_cov_pairs(Engine& e, const double* X, int ldb, const int32_t* pair, int64_t n_pairs, double* cov_dev);
// kernels_border.hip: the border of the joint system "poses + camera model" and its reduction to 9 x 9
constexpr int kBorderOut = 181;   // cost | g_k[9] | C[81] | r_k[9] | S_k[81]
size_t border_workspace_doubles(const Engine& e);
double* launch_border(Engine& e, int robustify, double huber_a, double* ws);   // behind the covariance preamble
int preload_border_kernels();
// kernels_init.hip
struct InitPass {   // one score + select + refine pass over a family
    bool sweep = false;             // false: place what is not placed yet; true: redo every placed pose
    int min_tag_observations = 2;
    double score_cap_px = 100.0;
    int refine_iterations = 30;
};
// wh_index: row of tag_wh that holds observation i's size (null: row i); out_index: where in qt2 / rms2 observation i's
// results go (null: i)
void launch_quad_poses(hipStream_t st, const Intrinsics& K, int64_t n, const double* tag_wh, const double* obs_px, double* qt2,
                       double* rms2, const int32_t* wh_index = nullptr, const int32_t* out_index = nullptr);
// kernels_localize.hip
struct LocalizeArgs {
    Intrinsics K;
    int n_imgs;
    const int64_t* img_start;  // [n_imgs + 1]
    const int32_t* obs_tag;    // [n_obs]
    const double* obs_px;      // [8 * n_obs]
    const double* tag_qt;      // [7 * n_tags]
    const double* corners;     // [12 * n_tags] world corners (k_map_corners)
    const double* quad_qt;     // [14 * n_obs] planar tag->camera poses (k_quad_pose)
    const double* quad_rms;    // [2 * n_obs]
    int max_trials, robustify, passes, min_inliers;
    double huber_a, cap2, inlier2;
    double* cam_qt;            // [7 * n_imgs]
    double* cam_cov;           // [36 * n_imgs]
    uint8_t* obs_inlier;       // [n_obs]: the active set of every pass, the final flags at the end
    vmm_ba_localize_result* res;
};
void launch_map_corners(hipStream_t st, int n_tags, const double* tag_qt, const double* tag_wh, double* corners);
void launch_localize(hipStream_t st, const LocalizeArgs& a, bool any_staged, bool any_unstaged);
int localize_stage_capacity();   // observations of one image that k_localize stages in LDS
int preload_localize_kernels();
// localize.hip: the host stage that vmm_ba_localize and vmm_ba_calibrate share (vmm_ba_rig_localize takes its checks,
// memory and uploads) -- a batch of images against a map, from
// the argument checks to the localisation's results.  `who` is the entry point's name, for the error text; the checks
// are separate functions because the two entry points make them in different orders.
struct MapBatch {
    // the caller's arrays (check_batch)
    int32_t n_tags = 0, n_imgs = 0;
    int64_t n_obs = 0;
    const double *h_tag_qt = nullptr, *h_tag_wh = nullptr, *h_px = nullptr;
    const int64_t* h_start = nullptr;
    const int32_t* h_obs_tag = nullptr;
    bool any_staged = false, any_unstaged = false;   // an image of at most / more than localize_stage_capacity() observations
    // their device copies and what the three kernels write (carve)
    double *tag_qt = nullptr, *tag_wh = nullptr, *corners = nullptr, *px = nullptr, *quad_qt = nullptr, *quad_rms = nullptr;
    int64_t* start = nullptr;
    int32_t* obs_tag = nullptr;
    double *cam = nullptr, *cov = nullptr;
    uint8_t* inl = nullptr;
    vmm_ba_localize_result* res = nullptr;

    void carve(Arena& ar);   // the twelve pieces, in this order; the caller's own go behind them
    LocalizeArgs args(const double intr[4], const double dist[5], const vmm_ba_localize_options& o) const;
    void upload(Arena& ar) const;   // the five copies to the device
    // the uploads, then k_quad_pose -> k_map_corners -> k_localize and `then()` (the caller's further launches) on the
    // null stream, in order, then one hipGetLastError; the blocking copies back wait for the kernels
    template <typename Then>
    void run(Arena& ar, const LocalizeArgs& a, Then&& then) const
    {
        upload(ar);
        if (ar.err != hipSuccess)
            return;
        launch_quad_poses(nullptr, a.K, n_obs, tag_wh, px, quad_qt, quad_rms, obs_tag);
        launch_map_corners(nullptr, n_tags, tag_qt, tag_wh, corners);
        launch_localize(nullptr, a, any_staged, any_unstaged);
        then();
        ar.err = hipGetLastError();
    }
    void results(Arena& ar, double* cam_qt, double* cam_cov, uint8_t* obs_inlier, vmm_ba_localize_result* res_out) const;
};
// arrowhead.hpp: what the two joint refinements against a fixed map share (vmm_ba_calibrate: the camera model and one pose
// per image; vmm_ba_rig_calibrate: the extrinsics and one rig pose per frame).  An item is an image or a frame, P the
// number of shared unknowns (9; 6 n_rig_cams).
// An item's record: reduced P x P block (packed lower) | reduced gradient (P) | diag(C) (P) | cost | sum |r|^2 | 1 if
// A + lam diag was not positive definite | inlier observations | 1 (the item takes part); all zero for one that does not
__host__ __device__ constexpr int arrow_rec_doubles(int P) { return P * (P + 1) / 2 + 2 * P + 5; }
// An item's elimination: L (21, packed lower) | Y = L^-1 B (6 x P) | y = L^-1 g (6)
__host__ __device__ constexpr int arrow_elim_doubles(int P) { return 27 + 6 * P; }
struct ArrowCtl {                    // the control block of the LM loop behind the shared unknowns' current, candidate, step
    double lam, cost, raw2;          // damping; sum rho and sum |r|^2 over the inliers at the current state
    double initial_cost, initial_raw2;
    int32_t refine_mask, max_trials;
    int32_t trials, accepted;
    int32_t done, stop;              // done: every kernel returns at once; stop: 1 converged, 2 max_trials ran out
    int32_t solve_ok, first;         // first: the next evaluation is the start of the whole call (initial_*)
    int32_t n_used, n_obs_used;      // items that take part, their inlier observations
    int32_t cov_ok, initial_n_obs;
};
struct ArrowArgs {                   // n: the number of items
    double* cand;                    // [7 * n] candidate poses
    int32_t* part;                   // [n] the item takes part
    int32_t* n_in;                   // [n] its inlier observations
    double* rec;                     // [arrow_rec_doubles(P) * n]
    double* elim;                    // [arrow_elim_doubles(P) * n]
    double* trial;                   // [2 * n] candidate cost | max |pose step|
    int robustify, min_inliers;
    double huber_a, inlier2;
};
// kernels_rig.hip: a rig of rigidly mounted cameras against a fixed map (vmm_ba_rig_localize)
struct RigArgs {
    LocalizeArgs loc;          // per frame what it holds per image: n_imgs frames, img_start [n_rig_cams * n_imgs + 1] (image
                               // (f, c) is slot f * n_rig_cams + c), cam_qt / cam_cov / res per frame; K is not used
    int n_rig_cams;
    const double* intr;        // [4 * n_rig_cams]
    const double* dist;        // [5 * n_rig_cams]
    const double* ext_qt;      // [7 * n_rig_cams] rig->camera
};
void launch_rig_localize(hipStream_t st, const RigArgs& a);
// the joint refinement of the extrinsics and one rig pose per frame (vmm_ba_rig_calibrate); P = 6 n_rig_cams.  The
// control block's common part, the per-frame buffers and the record layouts are the arrowhead's (above)
constexpr int kRigDof = 6 * VMM_BA_RIG_MAX_CAMS;
struct RigCalCtl {
    double ext[7 * VMM_BA_RIG_MAX_CAMS], ext_cand[7 * VMM_BA_RIG_MAX_CAMS], dext[kRigDof];   // current, candidate, step
    ArrowCtl lm;
};
struct RigCalArgs {
    RigArgs rig;                   // the batch; loc.cam_qt: current rig poses, loc.obs_inlier: the inlier set of the refinement,
                                   // loc.res: the localisation's results, loc.cam_cov: the joint marginals; ext_qt is not used
                                   // (the extrinsics are RigCalCtl's)
    ArrowArgs w;                   // per frame; P = 6 n_rig_cams
    RigCalCtl* ctl;
    double* ext_cov;               // [P * P]
};
void launch_rigcal_begin(hipStream_t st, const RigCalArgs& a);
void launch_rigcal_classify(hipStream_t st, const RigCalArgs& a);
void launch_rigcal_trial(hipStream_t st, const RigCalArgs& a);
void launch_rigcal_covariance(hipStream_t st, const RigCalArgs& a);
int preload_rig_kernels();
// kernels_triangulate.hip: free points from known cameras (vmm_ba_triangulate)
constexpr int kCamFrame = 15;   // doubles of a camera's frame: R (9, row-major, of q / |q|) | t (3) | c = -R^T t (3)
struct TriangulateArgs {
    Intrinsics K;
    int n_pts;
    const double* frames;      // [kCamFrame * n_cams] (k_cam_frames)
    const double* cam_cov;     // [36 * n_cams] or null
    const int64_t* pt_start;   // [n_pts + 1]
    const int32_t* obs_cam;    // [n_obs]
    const double* obs_uv;      // [2 * n_obs]
    int max_trials, robustify, passes, min_inliers, max_pair;
    double huber_a, cap2, inlier2;
    double* xyz;               // [3 * n_pts]
    double* cov;               // [9 * n_pts]
    double* cov_cams;          // [9 * n_pts]
    uint8_t* obs_inlier;       // [n_obs]: the active set of every pass, the final flags at the end
    vmm_ba_triangulate_result* res;
};
void launch_cam_frames(hipStream_t st, int n_cams, const double* cam_qt, double* frames);
void launch_triangulate(hipStream_t st, const TriangulateArgs& a);
int preload_triangulate_kernels();
// kernels_locate.hip: tag poses from known cameras (vmm_ba_locate_tags)
struct LocateArgs {
    Intrinsics K;
    int n_tags;
    const double* rigids;      // [12 * n_cams] R | t of every camera (k_camera_rigids)
    const double* cam_cov;     // [36 * n_cams] or null
    const double* tag_wh;      // [2 * n_tags]
    const int64_t* tag_start;  // [n_tags + 1]
    const int32_t* obs_cam;    // [n_obs]
    const double* obs_px;      // [8 * n_obs]
    const double* quad_qt;     // [14 * n_obs] planar tag->camera poses (k_quad_pose)
    const double* quad_rms;    // [2 * n_obs]
    int max_trials, robustify, passes, min_inliers;
    double huber_a, cap2, inlier2;
    double* tag_qt;            // [7 * n_tags]
    double* tag_cov;           // [36 * n_tags]
    double* tag_cov_cams;      // [36 * n_tags]
    uint8_t* obs_inlier;       // [n_obs]: the active set of every pass, the final flags at the end
    vmm_ba_localize_result* res;
};
void launch_camera_rigids(hipStream_t st, int n_cams, const double* cam_qt, double* rigids);
void launch_locate_tags(hipStream_t st, const LocateArgs& a, bool any_staged, bool any_unstaged);
int locate_stage_capacity();   // observations of one tag that k_locate_tags stages in LDS
int preload_locate_kernels();
// kernels_predict.hip: the localisation accuracy a pose would have against a finished map (vmm_ba_predict_localization)
constexpr int kTagFace = 6;   // doubles of a tag's face: n = R e_z (3) | centre (3)
struct PredictArgs {
    Intrinsics K;
    int n_tags, n_poses;
    const double* corners;     // [12 * n_tags] world corners (k_map_corners)
    const double* faces;       // [kTagFace * n_tags] (k_tag_faces)
    const double* tag_cov;     // [36 * n_tags] or null (k_predict<false>)
    const double* frames;      // [kCamFrame * n_poses] (k_cam_frames)
    double u_lo, u_hi, v_lo, v_hi;   // margin_px, width - margin_px, margin_px, height - margin_px
    double min_depth, cos_max_angle, min_side2, sigma2;   // min_side_px^2, sigma_px^2
    int min_tags;
    double* cov_px;            // [36 * n_poses] or null
    double* cov_map;           // [36 * n_poses] or null
    uint8_t* visible;          // [n_poses * n_tags] or null
    vmm_ba_predict_result* res;   // [n_poses] or null
};
void launch_tag_faces(hipStream_t st, int n_tags, const double* tag_qt, double* faces);
void launch_predict(hipStream_t st, const PredictArgs& a);
int preload_predict_kernels();
// kernels_predict_joint.hip: the same with the map's joint covariance (vmm_ba_predict_localization_joint)
struct PredictJointArgs {
    PredictArgs p;                 // tag_cov unused; visible is never null: the kernel's second sweep reads what its first wrote
    const double* tag_cov_joint;   // [36 * n_tags * n_tags] block-major, blocks s >= t read
    const uint8_t* visible_in;     // [n_poses * n_tags] or null: the selection instead of the visibility rules
};
void launch_predict_joint(hipStream_t st, const PredictJointArgs& a);
int preload_predict_joint_kernels();
// kernels_calibrate.hip: the joint refinement of the camera model and one pose per image against a fixed map
constexpr int kCalRec = arrow_rec_doubles(9);     // 68
constexpr int kCalElim = 84;                        // the stride of an image's elimination: arrow_elim_doubles(9) = 81 of it are used
struct CalibCtl {              // control block of the LM loop: k_calib_solve and k_calib_control write it, the host polls it
    double k[9], k_cand[9], dk[9];   // (fx, fy, cx, cy, k1, k2, p1, p2, k3): current, candidate, step
    ArrowCtl lm;
};
struct CalibArgs {
    int n_imgs;
    const int64_t* img_start;
    const int32_t* obs_tag;
    const double* obs_px;
    const double* corners;         // [12 * n_tags] world corners (k_map_corners)
    uint8_t* flags;                // [n_obs] the inlier set of the refinement
    vmm_ba_localize_result* res;   // [n_imgs] the localisation's results; k_calib_cov_pose updates the images that took part
    double* cam_qt;                // [7 * n_imgs] current poses
    ArrowArgs w;                   // per image; P = 9
    CalibCtl* ctl;
    double* intr_cov;              // [81]
    double* cam_cov;               // [36 * n_imgs]
};
void launch_calib_begin(hipStream_t st, const CalibArgs& a);      // who takes part, from the localisation's results
void launch_calib_classify(hipStream_t st, const CalibArgs& a);   // new inlier flags under the current camera model
void launch_calib_trial(hipStream_t st, const CalibArgs& a);      // one LM trial: image sums -> solve -> try -> control
void launch_calib_covariance(hipStream_t st, const CalibArgs& a); // undamped system at the result: intr_cov, cam_cov, res
int preload_calibrate_kernels();
void launch_init_quad(Engine& e);
void launch_init_begin(Engine& e);
void launch_init_pass(Engine& e, bool cam, const InitPass& s);
void launch_init_stats(Engine& e, double* out);
// kernels_lm.hip
void launch_control(Engine& e);
void launch_begin_loop(Engine& e, const LmCtl& init);
void launch_pose_plus(hipStream_t st, int64_t n, const double* qt, const double* delta, double* out);
void launch_backsub(Engine& e);
void launch_candidate(Engine& e);

} // namespace vmm
