// Host-side plan of a bundle-adjustment handle: everything vmm_ba_create decides before it touches the device --
// observation orders, the rank-k schedule, the form, ordering and symbolic structure of the reduced system -- and the
// environment switches.  Plain C++17: no HIP header, no Engine, no device call (tests/cpp/plan_test.cpp builds it with
// g++ alone).  engine.hpp and the kernels take the shared constants from here.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/vmm_ba.h"

namespace vmm {

constexpr int kWave = 64;          // gfx950 wavefront
constexpr int kPart = 32;          // doubles per task partial: 21 (H lower) + 6 (g) + 1 (cost) + pad
constexpr int kNB = 64;            // dense block size of the reduced system
constexpr int kDfMaskWords = 4;    // 64-bit words of a block row's structure mask (tree orderings): up to 255 block columns
constexpr int kDfMaxBlk = 256;
constexpr int kKT = 16;            // K tile of the MFMA f64 rank-k update (rows of Z per LDS stage)
constexpr int kST = 128;           // output tile of the rank-k update (the leading dimension is a multiple of it)

// k_schur_pairs (kernels_schur.hip): workgroup size, lanes that share one output column, and so pairs per work item
#ifndef VMM_PAIR_NS
#define VMM_PAIR_NS 2
#endif
#ifndef VMM_PAIR_THREADS
#define VMM_PAIR_THREADS 256
#endif
constexpr int kPairSplit = VMM_PAIR_NS;                  // lanes that share one output column: each takes every
                                                         // kPairSplit-th term, the partial sums meet in a fixed shuffle tree
constexpr int kPairThreads = VMM_PAIR_THREADS;           // workgroup size of k_schur_pairs
constexpr int kPairsPerItem = kPairThreads / (6 * kPairSplit);    // 6 x kPairSplit lanes per pair

inline int round_up(int64_t v, int m) { return (int)(((v + m - 1) / m) * m); }

// One wave's work: up to 64 consecutive observations of one pose in a family-sorted order.
struct Task {
    int32_t pose;
    int32_t begin;
    int32_t end;
};

// The environment switches of DESIGN.md section 10 (debugging and A/B only).  read_switches() holds the library's only
// getenv calls; a handle reads them once, at create, and keeps them.
struct Switches {
    bool debug = false;             // VMM_BA_DEBUG (set): diagnostics on stderr
    bool force_collectives = false; // VMM_BA_FORCE_COLLECTIVES=1: one rank, but the world > 1 code paths
    bool no_preload = false;        // VMM_BA_NO_PRELOAD=1
    bool eager_first = false;       // VMM_BA_EAGER_FIRST=1
    bool rccl_graph = true;         // VMM_BA_RCCL_GRAPH=0: collectives enqueued between graphs
    bool use_graph = true;          // VMM_BA_NO_GRAPH=1
    int graph_passes = 2;           // VMM_BA_GRAPH_PASSES (1..8)
    bool no_chain = false;          // VMM_BA_NO_CHAIN=1
    bool no_dataflow = false;       // VMM_BA_NO_DATAFLOW=1
    int capture_fail_rank = -1;     // VMM_BA_DEBUG_CAPTURE_FAIL=<rank>
    // VMM_BA_DEBUG_SPIN_LIMIT=<polls> [VMM_BA_DEBUG_SPIN_KERNEL=df|chain|both] [VMM_BA_DEBUG_SPIN_ONCE=1] [VMM_BA_DEBUG_SPIN_WG=<b>]
    uint32_t spin_df = 0, spin_chain = 0;
    bool spin_once = false;
    int spin_wg = -1;
    // plan of the reduced system
    bool eval_fused = false;        // VMM_BA_EVAL=fused
    int fused_group = 0;            // VMM_BA_FUSED_GROUP (1..64; 0: from the size)
    int schur = 0;                  // VMM_BA_SCHUR: 0 cost model, 1 dense, 2 sparse
    bool order_nd = false;          // VMM_BA_ORDER=nd
    bool order_natural = false;     // VMM_BA_ORDER=natural
    int nd_leaf = 42;               // VMM_BA_ND_LEAF
    int tree_max_wg = 16384;        // VMM_BA_TREE_MAX_WG
    bool tree_model_r3 = false;     // VMM_BA_TREE_MODEL=r3
    int pairs = -1;                 // VMM_BA_PAIRS: -1 cost model, 1 explicit, 0 anything else (implicit)
    // rank-k schedule
    int syrk_wg_per_cu = 0;         // VMM_BA_SYRK_WG_PER_CU (>= 1; 0: unset)
    int syrk_slices = 0;            // VMM_BA_SYRK_SLICES (>= 1; 0: unset)
    bool syrk_no_xcd = false;       // VMM_BA_SYRK_NO_XCD=1
    bool syrk_wide = true;          // VMM_BA_SYRK_WIDE=0
    // factorisation
    int df_max_wg = 0;              // VMM_BA_DF_MAX_WG (> 0 overrides)
    int chol_tail = -1;             // VMM_BA_CHOL_TAIL (>= 0 overrides)
    bool df_bulk = false;           // VMM_BA_DF_BULK=<n > 0>
    int df_help = -1;               // VMM_BA_DF_HELP: -1 by size, 0 / 1
};
Switches read_switches();

// Point landmarks: the caller's problem with every tag turned into two point pairs, every tag observation into two
// corner-pair observations.  `problem` points into the vectors.
struct PointProblem {
    std::vector<double> tag_qt, tag_wh, px;
    std::vector<int32_t> cam, tag;
    vmm_ba_problem problem;
};
void expand_points(const vmm_ba_problem& user, PointProblem& x);
// caller's tag poses -> the device's point pairs [2 * n_tags][7] (slot 6 unused)
std::vector<double> pairs_from_tags(const double* tag_qt, const double* tag_wh, int n_tags);

// Observations sorted by one pose family ("own", stable counting sort), each pose's run cut into wave-sized tasks.
struct OrderPlan {
    int64_t n = 0;
    int64_t n_pad = 0;                  // SoA stride (multiple of 64)
    std::vector<int32_t> own, other, caller;
    std::vector<double> px;             // [8][n_pad]
    std::vector<Task> tasks;
    std::vector<int32_t> pose_task;     // [n_own + 1]
    std::vector<int32_t> start;         // [n_own + 1]
};
OrderPlan plan_order(int n_own, const int32_t* own_idx, const int32_t* other_idx, const double* px, int64_t n);

// Work plan of the rank-k update (see plan.cpp), host half of SyrkPlan.
struct SyrkSchedule {
    int n_tiles = 0, n_kt = 0, n_wg = 0, n_segments = 0;
    bool wide = false;
    std::vector<int32_t> tile_bi, tile_bj, wg_seg0, tile_seg0;
    std::vector<int64_t> wg_u0, wg_u1;
};
SyrkSchedule plan_syrk(int n_row_blk, int n_col_blk, int k_pad, int n_cu, const Switches& sw);

// Everything vmm_ba_create uploads besides the poses, and the decisions behind it.  The fields mirror Engine's.
struct Plan {
    std::string error;              // not empty: the problem cannot be planned (VMM_BA_ERR_ARGUMENT)
    int n_e = 0, n_f = 0;
    OrderPlan ordE, ordF;           // observations sorted by the eliminated / kept family
    // fused evaluation (k_eval_fused)
    bool fused_eval = false;
    int fused_n_e_act = 0, fused_f_pad = 0, fused_chunks = 0, fused_group = 1, fused_groups = 0, fused_slots = 0;
    std::vector<int32_t> pair_obs, fused_e_list, fused_e_part0, fused_pose_task;
    // reduced system
    int n_red = 0, n_pad = 0, n_blk = 0, ldz = 0, k_dim = 0, k_pad = 0;
    bool sparse_schur = false;
    double co_terms = 0.0, schur_flops = 0.0;
    std::vector<int32_t> h_row_of;              // tree ordering: first row of every kept pose; empty: 6 f
    std::vector<int32_t> nd_node_first_blk;     // tree ordering: first block of every node, in elimination order
    // block-sparse elimination: the symbolic structure of S -= Z^T Z
    std::vector<int32_t> f2e, pair_start, pair_tstart;
    std::vector<int32_t> pair_terms;            // [n_terms][2]
    std::vector<int32_t> row_items;             // [2][n_row_items]
    int n_row_items = 0;
    bool explicit_pairs = false;
    std::vector<int32_t> pair_col, row_of, pose_of_row;
    // tree-ordered factor
    std::vector<unsigned long long> chol_nz;    // [n_blk + 1][kDfMaskWords]
    std::vector<unsigned char> chol_order;      // [n_blk][kDfMaxBlk]
    std::vector<int32_t> df_wg, df_slot;
    int n_df_wg = 0;
    size_t df_tree_slots = 0;
    double chol_flops = 0.0;
};
// p: the (expanded) problem; co: for the structure of all ranks (world > 1).
Plan make_plan(const vmm_ba_problem& p, const vmm_ba_create_options& co, bool elim_cams, bool multi, int world,
               bool points, const Switches& sw);

} // namespace vmm
