// vmm_ba_solve_small (include/vmm_ba.h): what its host side (small_ba.hip) and its kernel (kernels_small.hip) share.
// A batch of independent bundle adjustments, each small enough for one workgroup: the kept family (the one that is not
// eliminated) has at most VMM_BA_SMALL_MAX_KEPT poses, so the reduced system fits in LDS as its lower block triangle.
//
// Layout of a problem on the device.  Poses are numbered cameras first, then tags (the order of scale / D2 / active in
// the handle path), and every per-pose array of the batch holds the problems one after the other (pose_off).  The
// observations are sorted by (eliminated pose, kept pose, caller's order) and every per-observation array holds the
// problems one after the other (obs_off); e_start cuts them by eliminated pose, f_list / f_start lists them by kept pose
// in ascending order.  pair_start cuts `pairs` by block (fa, fb), fb <= fa, of the reduced system's lower block triangle
// (block fa (fa + 1) / 2 + fb): the pairs (ia, ib) of observations of kept poses fa and fb that share an eliminated pose, in
// ascending order of that pose -- the block products Y_ia^T Y_ib the block subtracts.
#pragma once

#include "engine.hpp"

namespace vmm {

constexpr int kSmallThreads = 256;                                     // one workgroup = one problem
constexpr int kSmallMaxKept = VMM_BA_SMALL_MAX_KEPT;
constexpr int kSmallBlocks = kSmallMaxKept * (kSmallMaxKept + 1) / 2;  // 6 x 6 blocks of the lower block triangle
constexpr int kSmallPosePart = 27;                                     // packed lower 6 x 6 (21) + gradient (6)
constexpr int kSmallObsPart = 2 * kSmallPosePart + 1;                  // eliminated pose's share, kept pose's share, cost

struct SmallDesc {
    Intrinsics K;
    int32_t n_cams, n_tags, n_obs, n_e, n_f, elim_cams, trace_capacity, reserved;
    int64_t pose_off, obs_off, e_start_off, f_start_off, pair_start_off, pair_off, trace_off;
};

struct SmallResult {   // the part of vmm_ba_summary the device decides
    int32_t termination, records, num_successful, num_unsuccessful, num_lm_iterations, num_jac_evals, num_cost_evals, reserved;
    double initial_cost, final_cost;
};

struct SmallArgs {
    const SmallDesc* desc;
    SmallResult* res;
    vmm_ba_options o;
    // per pose
    double* x;                // [7] the state: in = the start, out = the result
    double* cand;             // [7]
    const double* wh;         // [2] tag width, height (unused for cameras)
    const uint8_t* is_const;  // constant flag, the fixed tag included
    double* Hg;               // two copies (hg_stride apart) of [27]: J^T J packed lower, J^T r; one at x, one at the candidate
    int64_t hg_stride;
    double *scale, *diag, *D2, *delta, *ysol;   // [6]
    double* part;             // [5] d.g, d^T H d, |x - x+|^2, |x+|^2, non-finite flag
    double* gm;               // [1] |Plus(x, -g) - x|_inf
    double *Le, *ze;          // [21] factor of the damped block, [6] L^-1 g (eliminated poses)
    int32_t* active;
    // per observation (sorted)
    const int32_t *obs_e, *obs_f;
    const double* px;         // [8]
    double* W;                // two copies (w_stride apart) of [36]: J_e^T J_f, row = eliminated pose's tangent
    int64_t w_stride;
    double* Y;                // [36] L_e^-1 (s_e W s_f)
    double* opart;            // [kSmallObsPart]
    const int32_t *e_start, *f_start, *f_list;
    const int32_t* pair_start;   // [blocks + 1] per problem, into pairs (from the problem's pair_off)
    const int32_t* pairs;        // [2]: ia, ib
    vmm_ba_iteration* trace;
};

void launch_small_ba(hipStream_t st, int n_problems, const SmallArgs& a);
int preload_small_kernels();

} // namespace vmm
