/*
 * vmm_ba.h -- C-ABI of libvmm_ba.so: the MI355X (gfx950) bundle-adjustment engine behind
 * visual_marker_mapping's TagReconstructor hot path.
 *
 * Plain C: pointers and sizes only, no Eigen/torch types.  Each entry point names the reference
 * interface it replaces (file:line relative to /root/reference).  Host arrays are owned by the
 * caller; the handle owns device memory; nothing is thrown across this boundary -- every call
 * returns a status and vmm_ba_last_error() holds the text of the last failure on this thread.
 *
 * Data conventions (reference: include/visual_marker_mapping/Camera.h:13-17,
 * TagReconstructor.h:19-52, DetectionResults.h:10-37):
 *   pose      = 7 doubles: quaternion (w,x,y,z), translation (x,y,z)
 *   camera    = world->camera, tag = tag->world (TagReconstructionCostFunction.h:107-122)
 *   tag quad  = LL,LR,UR,UL = (-w/2,-h/2,0),(w/2,-h/2,0),(w/2,h/2,0),(-w/2,h/2,0)
 *   obs_px    = 8 doubles per tag observation: the four corners' (u,v) in that order
 *   tangent   = 6 per pose: translation(3), then the half-angle rotation vector(3) of
 *               ceres::QuaternionParameterization (src/TagReconstructor.cpp:661)
 */
#ifndef VMM_BA_H_
#define VMM_BA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMM_BA_ABI_VERSION 6

typedef struct vmm_ba_handle_s* vmm_ba_handle;

/* status codes */
enum {
    VMM_BA_OK = 0,
    VMM_BA_ERR_ARGUMENT = 1,   /* bad sizes / indices / null pointers */
    VMM_BA_ERR_HIP = 2,        /* a HIP runtime call failed (no device, OOM, launch failure) */
    VMM_BA_ERR_COLLECTIVE = 3, /* the user-supplied all-reduce callback reported failure */
    VMM_BA_ERR_STATE = 4,      /* call sequence error */
    VMM_BA_ERR_NUMERIC = 5     /* rank-deficient Jacobian: no covariance (ceres::Covariance::Compute == false) */
};

/* which pose family is eliminated by block Gaussian elimination before the dense reduced solve.
 * The reference puts tags in Ceres ordering group 0 and cameras in group 1
 * (src/TagReconstructor.cpp:675-676,695-696) but keeps Ceres' default exact solver; any exact
 * elimination yields the same LM step. */
enum {
    VMM_BA_ELIM_AUTO = 0,    /* eliminate the larger family -> smaller reduced system */
    VMM_BA_ELIM_TAGS = 1,    /* reduced camera system (the reference's ordering) */
    VMM_BA_ELIM_CAMERAS = 2  /* reduced tag system */
};

/* Ceres termination_type as printed by src/TagReconstructor.cpp:740 */
enum { VMM_BA_CONVERGENCE = 0, VMM_BA_NO_CONVERGENCE = 1, VMM_BA_FAILURE = 2 };

/* The problem TagReconstructor::doBundleAdjustment assembles at src/TagReconstructor.cpp:646-724:
 * reconstructed tags, reconstructed cameras with >= 1 reconstructed tag, and the observations
 * whose camera and tag are both reconstructed, with dense 0-based indices. */
typedef struct vmm_ba_problem {
    double intr[4];          /* fx, fy, cx, cy           CameraModel.h:14-17 */
    double dist[5];          /* k1, k2, p1, p2, k3       CameraModel.cpp:11-16 */
    int32_t n_cams;
    int32_t n_tags;
    const double* cam_qt;    /* [7*n_cams] initial camera poses (src/TagReconstructor.cpp:692-693) */
    const double* tag_qt;    /* [7*n_tags] initial tag poses    (src/TagReconstructor.cpp:665-666) */
    const double* tag_wh;    /* [2*n_tags] tag width, height    (src/TagReconstructor.cpp:713,718) */
    int32_t fixed_tag;       /* dense index of the origin tag, or -1 (src/TagReconstructor.cpp:669-673) */
    int64_t n_obs;
    const int32_t* obs_cam;  /* [n_obs] */
    const int32_t* obs_tag;  /* [n_obs] */
    const double* obs_px;    /* [8*n_obs] (src/DetectionIO.cpp:45-51) */
} vmm_ba_problem;

#define VMM_BA_PRECISION_F64 0
#define VMM_BA_PRECISION_F32_ACCUM 1

/* Landmark model.  TAG_POSES: TagReconstructionCostFunction (CostFunction.h:88-184), one 7-parameter pose per tag
 * -- the live doBundleAdjustment (src/TagReconstructor.cpp:646-743).  POINTS: OpenCVReprojectionError
 * (CostFunction.h:9-84), four free 3-D points per tag, 3x3 landmark blocks -- doBundleAdjustment_points
 * (src/TagReconstructor.cpp:457-644, `#if 0` in the reference): the tag poses handed to vmm_ba_create become their
 * four world corners (:483-491), the origin tag's corners are constant (:494-497), no loss function (:556).
 * vmm_ba_get_state then returns tag poses rebuilt from the optimised corners (:608-639), vmm_ba_get_points the
 * corners themselves. */
#define VMM_BA_LANDMARK_TAG_POSES 0
#define VMM_BA_LANDMARK_POINTS 1

typedef struct vmm_ba_create_options {
    int32_t device;          /* HIP device ordinal */
    int32_t elimination;     /* VMM_BA_ELIM_* */
    /* Multi-GPU: one process per GPU.  Every rank passes ALL poses and only ITS shard of the
     * observations (sharded by the eliminated family, cameras by default); rank/world are
     * informational, the exchange itself goes through vmm_ba_set_allreduce(). */
    int32_t rank;
    int32_t world_size;
    /* VMM_BA_PRECISION_F64 (default): everything in f64, as the reference.
     * VMM_BA_PRECISION_F32_ACCUM (BASELINE.json configs[3]): the Gauss-Newton blocks J^T J (per-pose 6x6
     * and per-observation J_e^T J_f) are accumulated and stored in f32; residuals, cost, the gradient
     * J^T r, the reduced system S, its factorisation and every LM decision stay f64.  The fixed point
     * (zero gradient) is unchanged, the LM trajectory is that of a slightly perturbed Gauss-Newton model. */
    int32_t precision;
    int32_t landmarks;       /* VMM_BA_LANDMARK_* */
    /* world_size > 1 only, optional (ABI 4): the (camera, tag) index pairs of the observations of ALL ranks -- the same
     * arrays on every rank, structure only, no pixels; the caller keeps them alive during vmm_ba_create only.  The
     * reduced systems of the ranks are summed and must share one layout: with the global structure every rank orders the
     * kept family by the same nested dissection (tree ordering, vmm_ba_summary.tree_ordering); without it world_size > 1
     * keeps the natural order.  The reference is a single process (src/TagReconstructor.cpp:646-743): no counterpart. */
    int64_t n_structure_obs;
    const int32_t* structure_obs_cam;
    const int32_t* structure_obs_tag;
} vmm_ba_create_options;

/* Solver::Options fields the reference sets (src/TagReconstructor.cpp:725-735) plus the Ceres
 * defaults that are in force because it does not set them. */
typedef struct vmm_ba_options {
    int32_t max_num_iterations;        /* 400 / 1500: src/TagReconstructor.cpp:233,271,277 */
    int32_t robustify;                 /* HuberLoss(huber_a) per corner block, :721 */
    double huber_a;                    /* 1.0 */
    double function_tolerance;         /* 1e-6  */
    double gradient_tolerance;         /* 1e-10 */
    double parameter_tolerance;        /* 1e-8  */
    double initial_trust_region_radius;/* 1e4   */
    double max_trust_region_radius;    /* 1e16  */
    double min_trust_region_radius;    /* 1e-32 */
    double min_relative_decrease;      /* 1e-3  */
    double min_lm_diagonal;            /* 1e-6  */
    double max_lm_diagonal;            /* 1e32  */
    int32_t max_num_consecutive_invalid_steps; /* 5 */
    int32_t jacobi_scaling;            /* 1 */
    int32_t num_threads;               /* accepted for signature parity (:733); the GPU path ignores it */
    int32_t poll_interval;             /* iteration-graph launches (two LM passes each) enqueued between host
                                          polls of the device control block (>=1); does not change results */
} vmm_ba_options;

/* One row of Ceres' Solver::Summary::iterations. */
typedef struct vmm_ba_iteration {
    int32_t iteration;
    int32_t step_is_valid;
    int32_t step_is_successful;
    int32_t reserved;
    double cost;
    double cost_change;
    double gradient_max_norm;
    double step_norm;
    double relative_decrease;
    double trust_region_radius;
    double model_cost_change;
} vmm_ba_iteration;

typedef struct vmm_ba_summary {
    int32_t termination_type;       /* VMM_BA_CONVERGENCE / NO_CONVERGENCE / FAILURE */
    int32_t iterations;             /* == Ceres summary.iterations.size() */
    int32_t num_successful_steps;
    int32_t num_unsuccessful_steps;
    int32_t num_lm_iterations;      /* passes of the trust-region loop (each = 1 linear solve) */
    int32_t num_jacobian_evals;
    int32_t num_cost_evals;
    int32_t elimination;            /* the VMM_BA_ELIM_* actually used */
    double initial_cost;
    double final_cost;
    double time_solve_s;            /* host wall time of vmm_ba_solve */
    vmm_ba_iteration* trace;        /* optional caller buffer, filled up to trace_capacity rows */
    int32_t trace_capacity;
    int32_t reserved;
    /* Where the device time of the solve went (the per-phase part of Ceres' Summary::FullReport(),
     * src/TagReconstructor.cpp:741-742), measured ON the device: the first kernel of every group stamps the
     * 100 MHz s_memrealtime counter and the control kernel sums the differences.  Their sum is <= time_solve_s. */
    double time_eval_s;             /* residual + Jacobian evaluation, J^T J / J^T r blocks (Ceres: "Jacobian & residual evaluation") */
    double time_eliminate_s;        /* block elimination, Z, rank-k update, reduced system */
    double time_factor_solve_s;     /* dense Cholesky + triangular solves (Ceres: "Linear solver") */
    double time_step_s;             /* back-substitution, candidate, cost at the candidate */
    double time_control_s;          /* trust-region control kernels */
    /* The one-launch factorisation (k_chol_dataflow) and back-substitution (k_backsolve_chain) hand data between
     * workgroups with bounded spins.  A spin that gives up (a GPU time-sliced between processes, a profiler
     * serialising workgroups) is NOT a numerical failure and never reaches the trust-region policy: the library
     * redoes that pass's factorisation on the launch-per-block-column path and goes on, so the trajectory is the
     * one of an undisturbed run.  These two fields report that it happened. */
    int32_t num_sync_timeouts;      /* LM passes of this solve whose factorisation was redone on the fallback path */
    int32_t sync_timeout_kernels;   /* OR over those passes: 1 = k_chol_dataflow, 2 = k_backsolve_chain gave up,
                                       4 = another rank reported a give-up (world_size > 1) */
    int32_t block_sparse;           /* 1: the elimination ran over co-observed (camera, tag) pairs only (compressed Z,
                                       k_schur_pairs) -- what the handle chose at create from its block structure,
                                       VMM_BA_SCHUR=dense|sparse overrides; 0: dense Z + MFMA rank-k update */
    int32_t tree_ordering;          /* block-sparse handles only: number of nodes of the nested-dissection tree the kept
                                       family is ordered by (their block columns of the reduced system's factor are
                                       computed independently of each other where the tree says so); 0: natural order.
                                       Chosen at create when the longest chain of dependent block columns shrinks enough;
                                       VMM_BA_ORDER=nd|natural overrides */
} vmm_ba_summary;

/* Sum-all-reduce of `count` doubles in DEVICE memory, in place, ordered on `hip_stream`
 * (a hipStream_t).  Return 0 on success.  Called by vmm_ba_solve / vmm_ba_cost on every rank in
 * the same order.  The default (none set) is the single-GPU identity. */
typedef int (*vmm_ba_allreduce_fn)(void* user, void* device_buffer, size_t count, void* hip_stream);

/* Average duration of each device kernel of one LM iteration, measured with HIP events on the
 * engine's own stream (bench.py's roofline leg). */
typedef struct vmm_ba_kernel_times {
    double eval_elim_ms;     /* residual+Jacobian+accumulate as an LM iteration runs it: both family passes in
                              * one launch (k_eval_both, the eliminated family's pass writes W) + the per-pose sums */
    double eval_keep_ms;     /* 0 since the two passes share a launch (kept for layout compatibility) */
    double cost_ms;          /* cost-only residual pass */
    double form_z_ms;        /* block factor + Z = L^-1 W */
    double syrk_ms;          /* reduced system: S -= Z^T Z (dense: f64 MFMA rank-k update; block-sparse: k_schur_rows) */
    double cholesky_ms;      /* dense Cholesky + triangular solves of the reduced system */
    double backsub_ms;       /* back-substitution + Plus + model cost */
    double lm_iteration_ms;  /* one whole LM iteration as enqueued by vmm_ba_solve */
    int64_t n_obs;
    int32_t reduced_dim;     /* order of the dense reduced system (without padding) */
    int32_t elim_dim;        /* 6 * number of eliminated poses */
    int32_t schur_sparse;    /* 1: the reduced system is formed over co-observed (e, f) pairs only (compressed Z) */
    int32_t syrk_wide;       /* 1: the dense rank-k update runs k_syrk_wide (one 8-wave workgroup per CU; few tiles) */
    double schur_flops;      /* algorithmic flops of that formation: dense (n+1)(n+2) K; block-sparse 432 per pair of
                                observations sharing an eliminated pose (lower triangle) + the right-hand side */
    double chol_flops;       /* ABI 5.  Tree-ordered factor (vmm_ba_summary.tree_ordering > 0): flops of the Cholesky
                                factorisation + the two triangular solves over the NON-ZERO 64 x 64 blocks of the factor
                                (after fill); 0 for a dense factor, whose count is n^3 / 3 + 2 n^2 */
} vmm_ba_kernel_times;

const char* vmm_ba_last_error(void);
int vmm_ba_abi_version(void);
void vmm_ba_default_options(vmm_ba_options* o);
void vmm_ba_default_create_options(vmm_ba_create_options* o);

/* Replaces the ceres::Problem construction of src/TagReconstructor.cpp:657-724: uploads poses and
 * observations, sorts them by pose family, builds the block structure.  Done once per problem. */
int vmm_ba_create(const vmm_ba_problem* problem, const vmm_ba_create_options* copt,
                  vmm_ba_handle* out);
void vmm_ba_destroy(vmm_ba_handle h);

/* Poses live on the device between calls (the reference mutates map nodes in place through raw
 * double*, src/TagReconstructor.cpp:665-666,692-693,722).  vmm_ba_set_state copies the caller's arrays into
 * pinned staging memory and issues no device command: the caller's buffers are free at once, and the next call that
 * needs the poses on the device uploads them (vmm_ba_solve inside the one launch that starts its loop).  Either
 * pointer may be NULL (that family is left alone).
 * VMM_BA_LANDMARK_POINTS handles: get_state followed by set_state is NOT the identity on the tag family --
 * get_state returns poses rebuilt (and re-orthogonalised) from the optimised corners, set_state regenerates exact
 * rectangles from pose and tag_wh, as vmm_ba_create does (src/TagReconstructor.cpp:483-491 / :608-639); the free
 * corners themselves are read with vmm_ba_get_points. */
int vmm_ba_set_state(vmm_ba_handle h, const double* cam_qt, const double* tag_qt);
int vmm_ba_get_state(vmm_ba_handle h, double* cam_qt, double* tag_qt);

/* VMM_BA_LANDMARK_POINTS handles: points[12 * n_tags] = the four world corners (LL, LR, UR, UL) of every tag,
 * the parameter blocks of doBundleAdjustment_points (src/TagReconstructor.cpp:485-492). */
int vmm_ba_get_points(vmm_ba_handle h, double* points);

int vmm_ba_set_allreduce(vmm_ba_handle h, vmm_ba_allreduce_fn fn, void* user);

/* Native collective path (BASELINE.json north_star: "RCCL all-reduce over xGMI of the reduced camera system"):
 * the library resolves librccl.so itself (dlopen) and issues ncclAllReduce(ncclDouble, ncclSum) in place on its
 * own stream, recorded into the LM iteration's hipGraph, so that world > 1 runs one graph per iteration with no
 * host callback.  Rank 0 draws an id, the host side hands the same 128 bytes to every rank by whatever means it
 * has (MPI, torch.distributed, a file), and every rank calls vmm_ba_enable_rccl -- a collective call; rank and
 * world size are those of vmm_ba_create_options.  Takes precedence over a vmm_ba_set_allreduce callback. */
#define VMM_BA_RCCL_ID_BYTES 128
/* 1 when librccl.so and every entry point the library uses were resolved in this process, else 0 (no device call).
 * Launchers ask every rank for this and agree on the answer BEFORE any rank enters vmm_ba_enable_rccl: a rank that
 * cannot load RCCL would otherwise leave the others blocked inside ncclCommInitRank. */
int vmm_ba_rccl_available(void);
int vmm_ba_rccl_unique_id(void* id128);
int vmm_ba_enable_rccl(vmm_ba_handle h, const void* id128);

/* Switches observations off and on without rebuilding the handle: mask[i] != 0 keeps observation i (the
 * caller's order), NULL keeps all.  This is how the incremental driver (src/TagReconstructor.cpp:86-278: one
 * more image per bundle adjustment, observations of unreconstructed tags skipped at :699-708) grows its problem
 * on the device: one handle for the whole detection set, a mask per step.  A pose left without an active
 * observation drops out of the reduced program exactly like a pose without observations.  The poses of
 * switched-off observations must still be finite numbers (they are evaluated and weighted 0). */
int vmm_ba_set_observation_mask(vmm_ba_handle h, const uint8_t* mask);

/* ABI 6, additive.  cam_const[n_cams], tag_const[n_tags]: non-zero = hold that pose constant
 * (ceres::Problem::SetParameterBlockConstant, as src/TagReconstructor.cpp:669-673 does for the origin tag).  NULL = no
 * pose of that family.  Replaces any earlier set; the problem's fixed_tag stays constant regardless.  Callable between
 * solves like vmm_ba_set_observation_mask, and orthogonal to it.
 *   - The observations of a constant pose still add their residuals to the cost, and to the OTHER pose's J^T J and J^T r.
 *   - The constant pose's own columns are zero: its H block, its gradient, and W of every observation touching it.
 *   - An observation between two constant poses adds to the cost and the statistics only.
 *   - vmm_ba_solve never moves a constant pose: with H = 0 it is outside the reduced program exactly like the origin
 *     tag (unit diagonal, zero step); vmm_ba_get_state returns its bits unchanged.
 *   - VMM_BA_LANDMARK_POINTS handles: a constant tag fixes both of its pair blocks (its four corners,
 *     src/TagReconstructor.cpp:494-497); vmm_ba_get_points returns them unchanged.
 *   - world_size > 1: every rank passes the same arrays.  The flag is local to the evaluation and adds no collective.
 *   - vmm_ba_eval_blocks reports the zeros described above.
 *   - vmm_ba_tag_translation_covariance returns zeros for constant tags, as it does for the origin; the other tags'
 *     blocks are the covariance conditional on the constants.
 *   - vmm_ba_initialize grows the map from every constant pose (see there).
 *   - VMM_BA_ELIM_AUTO was decided at create and does not change; a constant pose keeps its (unit-diagonal) rows.
 * VMM_BA_ERR_ARGUMENT for a null handle; nothing else can be invalid. */
int vmm_ba_set_constant_poses(vmm_ba_handle h, const uint8_t* cam_const, const uint8_t* tag_const);

/* Replaces ceres::Solve at src/TagReconstructor.cpp:737-738. */
int vmm_ba_solve(vmm_ba_handle h, const vmm_ba_options* opt, vmm_ba_summary* summary);

/* ABI 6, additive.  Solves n_problems independent small bundle adjustments in ONE launch: the grid is the batch, one
 * workgroup runs the whole Levenberg-Marquardt loop of one problem (the shape of vmm_ba_localize), with no host round
 * trip and no hand-off between workgroups.  Stateless.  The reference's mapping step runs many bundle adjustments of a
 * few dozen poses (src/TagReconstructor.cpp:233,236,271-277: N + 2 of them, growing from one image and one tag); so do
 * sub-maps per room, resampled detection sets and leave-one-out re-solves.
 *   problem     every problems[i] is an independent vmm_ba_problem, with its own camera model, sizes, fixed_tag and
 *               observations, and is solved as vmm_ba_create + vmm_ba_solve would solve it with VMM_BA_PRECISION_F64 and
 *               VMM_BA_LANDMARK_TAG_POSES: the same objective, and the same trust-region policy stage for stage.
 *   constants   cam_const / tag_const: the flags of all problems one after the other (sum n_cams, sum n_tags), or NULL;
 *               they act as vmm_ba_set_constant_poses: a constant pose comes back bit for bit.
 *   elimination VMM_BA_ELIM_* for every problem; AUTO picks per problem what vmm_ba_create would pick.  The family that
 *               is NOT eliminated must have at most VMM_BA_SMALL_MAX_KEPT poses (its reduced system lives in LDS); the
 *               eliminated family and the observations are bounded only by int32.
 *   options     every field of vmm_ba_options but num_threads and poll_interval, which are ignored.
 *   results     cam_qt / tag_qt: the poses of all problems one after the other.  summaries[i]: termination_type,
 *               iterations, the step and evaluation counts, elimination, initial_cost, final_cost and (where
 *               summaries[i].trace is set on entry) the trace rows as vmm_ba_solve fills them; time_solve_s is the host
 *               wall time of the call, the same in every summary; the device phase times, num_sync_timeouts,
 *               sync_timeout_kernels, block_sparse and tree_ordering are 0.
 * No output is NaN unless the input poses made the first cost non-finite (VMM_BA_FAILURE, the poses returned as given).
 * A problem gives the same bits alone, in any batch, at any position and from run to run.  n_problems == 0 returns
 * VMM_BA_OK without a device call.  VMM_BA_ERR_ARGUMENT (before any device call, vmm_ba_last_error() names the problem):
 * null pointers, what vmm_ba_create rejects in a problem, a kept family above the limit, an elimination outside the
 * enum, what vmm_ba_solve rejects in the options.  VMM_BA_ERR_HIP with the byte count if the scratch cannot be allocated. */
#define VMM_BA_SMALL_MAX_KEPT 24   /* poses of the family that is NOT eliminated: reduced order <= 144 */
int vmm_ba_solve_small(int32_t n_problems, const vmm_ba_problem* problems, const uint8_t* cam_const, const uint8_t* tag_const,
                       const vmm_ba_options* o, int32_t elimination, double* cam_qt, double* tag_qt,
                       vmm_ba_summary* summaries, int device);

/* Cost-only evaluation 1/2 sum rho(|r|^2) at the current state (Ceres Evaluator, cost only). */
int vmm_ba_cost(vmm_ba_handle h, int robustify, double huber_a, double* cost);

/* Replaces computeReprojectionErrorPerImg / PerTag / PerCorner (src/TagReconstructor.cpp:340-455):
 * per_cam_mean[n_cams] (-1 for a camera without observations, :379-383), per_tag_mean[n_tags]
 * (NaN for a tag without observations), *avg (:416-426), per_corner[8*n_obs] signed pixel errors in
 * the caller's observation order (:447-451).  Any output may be NULL. */
int vmm_ba_reprojection_stats(vmm_ba_handle h, double* per_cam_mean, double* per_tag_mean,
                              double* avg, double* per_corner);

/* Replaces the ceres::Covariance block of doBundleAdjustment (src/TagReconstructor.cpp:744-783):
 * cov[9*t .. 9*t+8] = row-major 3x3 covariance of tag t's translation = the corresponding block of
 * (J^T J)^-1 in tangent coordinates at the current state, J with the loss applied when robustify != 0
 * (Covariance::Options::apply_loss_function defaults to true).  Constant (origin) and residual-free tags
 * get zeros, as Ceres reports for constant blocks.  Computed from the Schur factor of the undamped,
 * unscaled normal equations; VMM_BA_ERR_NUMERIC if they are not positive definite.  Single-GPU handles. */
int vmm_ba_tag_translation_covariance(vmm_ba_handle h, int robustify, double huber_a, double* cov);

/* ABI 6 (additive).  Any 6x6 marginal or cross block of the pose covariance.
 * cov[36*p ..] = row-major 6x6 block (pose_a[p], pose_b[p]) of (J^T J)^-1 in tangent coordinates at the current
 * state (translation, then half-angle rotation), J with the loss applied when robustify != 0.
 * Pose index space: cameras 0 .. n_cams-1, then tags n_cams .. n_cams+n_tags-1 (the order of scale / D2 / active).
 * Ceres: Covariance::Compute(covariance_blocks) + GetCovarianceBlockInTangentSpace.
 *   - The call leaves the state alone and is idempotent; a handle on the block-sparse or tree-ordered path switches to
 *     the dense, naturally ordered system for the call and back, like vmm_ba_tag_translation_covariance.
 *   - Pairs may repeat and come in any order; a == b is the marginal (symmetric in its bits).
 *   - A pair that names an inactive pose (constant, origin, or without an active observation) gets 36 zeros, the
 *     cross block included.
 *   - The bits of a block depend neither on what else is in the request nor on the call.
 *   - n_obs == 0: zeros.  n_pairs == 0: VMM_BA_OK without a device call.
 * VMM_BA_ERR_ARGUMENT (before any device call) for null pointers with n_pairs > 0 or an index outside
 * [0, n_cams + n_tags); VMM_BA_ERR_STATE for world_size > 1 or VMM_BA_LANDMARK_POINTS handles; VMM_BA_ERR_NUMERIC if
 * the normal equations are not positive definite; VMM_BA_ERR_HIP (with the byte count in the message) if the
 * n_pad x 6 (distinct poses, rounded up to 64 columns) right-hand side cannot be allocated. */
int vmm_ba_covariance_blocks(vmm_ba_handle h, int robustify, double huber_a, int64_t n_pairs,
                             const int32_t* pose_a, const int32_t* pose_b, double* cov);

/* Replaces CameraModel::projectPoint (src/CameraModel.cpp:6-26) for n camera-frame points. */
int vmm_ba_project_points(const double intr[4], const double dist[5], int64_t n,
                          const double* points_cam, double* uv, int device);

/* ABI 6.  n independent planar tag poses from each tag's own four corners; stateless like vmm_ba_project_points.
 * Replaces solvePnPEigen on a tag's own four corners (src/TagReconstructor.cpp:208, src/EigenCVConversions.cpp:38-63):
 * closed-form homography of the quad, decomposition, Levenberg-Marquardt on the 8 pixel residuals of
 * CameraModel::projectPoint -- and then the second planar solution (the tag normal mirrored about the line of sight to
 * the tag centre, refined the same way), which a small or distant tag makes nearly as good as the first.
 * A solution whose refinement spends all its trials (a weak-perspective quad, whose decomposition lies at the saddle
 * between the two solutions) is replaced by the refined first-order planar pose of its side, where that ends lower.
 * tag_wh[2*n]: width, height of observation i's tag; obs_px[8*n].
 * qt2[14*n]: two tag->camera poses per observation, lower RMS first; rms2[2*n]: their RMS corner distance in pixels.
 * A degenerate observation yields RMS = +inf and the pose (1,0,0,0, 0,0,1), never NaN. */
int vmm_ba_quad_poses(const double intr[4], const double dist[5], int64_t n, const double* tag_wh,
                      const double* obs_px, double* qt2, double* rms2, int device);

/* ABI 6.  Initial poses for the bundle adjustment from the detections alone (the reference gets them from its
 * incremental driver, src/TagReconstructor.cpp:86-278: one PnP + one bundle adjustment per image). */
typedef struct vmm_ba_init_options {
    int32_t sweeps;                /* 1: passes over all placed poses after the map stopped growing */
    int32_t min_tag_observations;  /* 2: active observations a tag needs to be placed (src/TagReconstructor.cpp:192) */
    double score_cap_px;           /* 100: a corner adds min(e^2, cap^2) to a candidate's score */
    int32_t refine_iterations;     /* 30: Levenberg-Marquardt trials (accepted + rejected) of one pose's refinement */
    int32_t reserved;
} vmm_ba_init_options;
typedef struct vmm_ba_init_report {
    int32_t rounds;                /* growth rounds run, the last one (which placed nothing) included */
    int32_t cams_reached, tags_reached, reserved;
    double avg_reprojection_px;    /* mean corner distance over the active observations between reached poses */
    double time_s;                 /* host wall time of the call */
} vmm_ba_init_report;
void vmm_ba_default_init_options(vmm_ba_init_options* o);
/* Overwrites the device state of every pose reachable from the constant poses: the fixed (origin) tag and whatever
 * vmm_ba_set_constant_poses names, cameras included.  The constant poses keep their current values.  They count as
 * placed from round 0, are never overwritten, are skipped by the sweeps and are reported reached.
 * The steps: planar poses of all active observations; then rounds -- every camera with an active observation of a placed tag,
 * then every tag with >= min_tag_observations active observations that a placed camera sees (the count is over all the
 * tag's active observations, whoever made them; one of them from a placed camera is enough): among the candidates
 * (two per such observation, chained through the placed pose) the one with the lowest truncated squared reprojection
 * error over all the pose's corners on placed counterparts, refined on its own -- until a round places nothing;
 * then `sweeps` passes that redo selection and refinement for every placed pose except the constant ones.
 * cam_reached[n_cams] / tag_reached[n_tags] (optional) receive 0/1; unreached poses keep their state.  Results are
 * bit-identical from run to run.  VMM_BA_ERR_STATE for world_size > 1 or VMM_BA_LANDMARK_POINTS handles,
 * VMM_BA_ERR_ARGUMENT for a handle with neither a fixed tag nor a constant pose. */
int vmm_ba_initialize(vmm_ba_handle h, const vmm_ba_init_options* o, vmm_ba_init_report* r,
                      uint8_t* cam_reached, uint8_t* tag_reached);

/* ABI 6, additive: new functions and structs only, no existing struct or signature changes.
 * Localises n_imgs images against a finished map; stateless like the quad poses above, every image independent of the
 * others in the batch.  Batch form of TagReconstructor::computeRelativeCameraPoseFromImg (src/TagReconstructor.cpp:
 * 280-312: every correspondence between one image and the reconstructed tags, RANSAC PnP).  Per image:
 *   candidates  the two planar solutions of each of its observations chained through the map tag, T_rel o T_tag^-1;
 *               each scored by sum min(e^2, score_cap_px^2) over ALL the image's corners with the residual the bundle
 *               adjustment minimises; lowest wins, ties to the lowest observation then solution 0, non-finite loses
 *   passes      reclassify_passes times: an observation is an inlier when its largest corner distance is at most
 *               inlier_px; then Levenberg-Marquardt on the 6 tangent degrees of freedom over the inliers, minimising
 *               1/2 sum rho(|r_corner|^2), until the cost is at its rounding floor or refine_iterations trials are spent.
 *               A pass that finds fewer than min_inlier_tags inliers ends the passes.  reclassify_passes == 0: one
 *               refinement over all observations.
 *   result      obs_inlier = the classification at the returned pose; cam_cov = row-major 6x6 (J^T J)^-1 in tangent
 *               order over those inliers, the loss applied when robustify != 0 (as the tag translation covariance above).
 * NO_OBSERVATIONS / NO_CANDIDATE: pose (1,0,0,0, 0,0,0), zero covariance, zero flags.  TOO_FEW_INLIERS (fewer than
 * min_inlier_tags at the returned pose): the best-effort pose and its flags, zero covariance.  SINGULAR: J^T J is not
 * positive definite; pose and flags are returned, the covariance is zeros.  No output is ever NaN; results are
 * bit-identical from run to run and do not depend on what else is in the batch.
 * VMM_BA_ERR_ARGUMENT (before any device call): null pointers, img_start not starting at 0 or decreasing, obs_tag
 * outside [0, n_tags), non-finite map poses or sizes, bad options.  n_imgs == 0 returns VMM_BA_OK without a device call. */
typedef struct vmm_ba_localize_options {
    int32_t refine_iterations;   /* 30: LM trials (accepted + rejected) of one refinement */
    int32_t robustify;           /* 1: HuberLoss(huber_a) per corner block, as doBundleAdjustment (:721) */
    double  huber_a;             /* 1.0 */
    double  score_cap_px;        /* 100: as vmm_ba_init_options */
    double  inlier_px;           /* 8.0: solvePnPRansac's reprojectionError (pnp.py default) */
    int32_t reclassify_passes;   /* 2: classify -> refine on the inliers, repeated this often */
    int32_t min_inlier_tags;     /* 1 */
} vmm_ba_localize_options;

typedef struct vmm_ba_localize_result {   /* one per image */
    int32_t status;              /* VMM_BA_LOC_* */
    int32_t n_obs, n_inlier_obs, trials;
    double  rms_px;              /* RMS corner distance over the inlier observations */
    double  cost;                /* 1/2 sum rho(|r|^2) over the inlier observations at the result */
} vmm_ba_localize_result;

enum { VMM_BA_LOC_OK = 0, VMM_BA_LOC_NO_OBSERVATIONS = 1, VMM_BA_LOC_NO_CANDIDATE = 2,
       VMM_BA_LOC_TOO_FEW_INLIERS = 3, VMM_BA_LOC_SINGULAR = 4 };

void vmm_ba_default_localize_options(vmm_ba_localize_options* o);
int vmm_ba_localize(const double intr[4], const double dist[5],
                    int32_t n_tags, const double* tag_qt, const double* tag_wh,      /* the map */
                    int32_t n_imgs, const int64_t* img_start,                         /* [n_imgs+1], CSR */
                    const int32_t* obs_tag, const double* obs_px,                     /* [n_obs], [8*n_obs] */
                    const vmm_ba_localize_options* o,
                    double* cam_qt,              /* [7*n_imgs] world->camera */
                    double* cam_cov,             /* [36*n_imgs] or NULL */
                    uint8_t* obs_inlier,         /* [n_obs] or NULL */
                    vmm_ba_localize_result* res, /* [n_imgs] or NULL */
                    int device);

/* ABI 6, additive.  Localises n_frames frames of a rig of n_rig_cams rigidly mounted cameras against a finished map:
 * vmm_ba_localize with one pose per frame instead of one per image.  Stateless like it, every frame independent of the
 * others in the batch.
 *   rig         camera c has its own model intr[4c .. 4c+3] / dist[5c .. 5c+4] and stands at ext_qt[7c .. 7c+6]
 *               (rig->camera) in the rig.  rig_qt[7f .. 7f+6] is world->rig of frame f, so camera c of frame f is
 *               ext_c o rig_f: R = R_c R_f, t = R_c t_f + t_c.  The rig pose moves in its own tangent (translation, then
 *               the half-angle rotation of vmm_ba_pose_plus), as every pose of this library.
 *   batch       image (f, c) is slot f * n_rig_cams + c of img_start[n_frames * n_rig_cams + 1]; a camera that saw
 *               nothing in a frame has an empty range.  obs_tag / obs_px as vmm_ba_localize.
 *   candidates  both planar solutions of every observation of the frame, computed under the observing camera's model and
 *               chained to the rig, T_c^-1 o T_rel o T_tag^-1; each scored by sum min(e^2, score_cap_px^2) over ALL the
 *               frame's corners in all cameras, the residual being the one the bundle adjustment minimises under the
 *               observing camera's model; lowest wins, ties to the lowest observation of the frame (camera-major) then
 *               solution 0, non-finite loses
 *   passes      as vmm_ba_localize, on the 6 degrees of freedom of the rig over the frame's inliers; min_inlier_tags
 *               counts over the frame
 *   result      obs_inlier = the classification at the returned pose; rig_cov = row-major 6x6 (J^T J)^-1 in the rig's
 *               tangent over those inliers, the loss applied when robustify != 0; res[f]: the VMM_BA_LOC_* statuses with
 *               the meanings and outputs vmm_ba_localize gives them, per frame.
 * No output is ever NaN; a frame gives the same bits alone, in any batch, at any position and from run to run.
 * VMM_BA_ERR_ARGUMENT (before any device call): what vmm_ba_localize rejects, n_rig_cams outside
 * [1, VMM_BA_RIG_MAX_CAMS], a non-finite or zero-quaternion extrinsic, a non-finite camera model.  n_frames == 0
 * returns VMM_BA_OK without a device call. */
#define VMM_BA_RIG_MAX_CAMS 8
int vmm_ba_rig_localize(int32_t n_rig_cams, const double* intr, const double* dist,   /* [4*K], [5*K] */
                        const double* ext_qt,                                         /* [7*K] rig->camera */
                        int32_t n_tags, const double* tag_qt, const double* tag_wh,   /* the map */
                        int32_t n_frames, const int64_t* img_start,                   /* [n_frames*K+1], CSR */
                        const int32_t* obs_tag, const double* obs_px,                 /* [n_obs], [8*n_obs] */
                        const vmm_ba_localize_options* o,
                        double* rig_qt,              /* [7*n_frames] world->rig */
                        double* rig_cov,             /* [36*n_frames] or NULL */
                        uint8_t* obs_inlier,         /* [n_obs] or NULL */
                        vmm_ba_localize_result* res, /* [n_frames] or NULL */
                        int device);

/* ABI 6, additive.  Calibrates a rig against a finished map: the extrinsics of its cameras and one rig pose per frame
 * are refined together, the map and the camera models held fixed.  The map of tags of known size is the calibration
 * target.  Stateless; the rig, the map and the batch exactly as vmm_ba_rig_localize takes them.  The semantics are
 * vmm_ba_calibrate's, with the 6 n_rig_cams extrinsic parameters (per camera: translation, then half-angle rotation, each
 * extrinsic moving in its own tangent as vmm_ba_pose_plus moves a pose) in the place of the nine numbers:
 *   start       vmm_ba_rig_localize's own steps under ext_qt0 and o->loc.  A frame that is not VMM_BA_LOC_OK, or has fewer
 *               than min_inlier_tags inliers, takes no part: it keeps what the localisation gave it and gets a zero rig_cov.
 *   refinement  Levenberg-Marquardt on 1/2 sum rho(|r_corner|^2) over the inlier observations, Marquardt damping on the
 *               frame blocks and on the extrinsic block; every frame eliminates its own 6 x 6 block, the reduced
 *               6K x 6K system is Jacobi-scaled.  An extrinsic outside refine_mask, or without an inlier observation in
 *               this refinement, has zero columns, a unit diagonal and a zero step: it comes back with the bits it went
 *               in with, and its rows and columns of ext_cov are zero.  Accept / reject, the stop rules,
 *               VMM_BA_CAL_NO_CONVERGENCE, the reclassify passes (classification at inlier_px under the current
 *               extrinsics, then a new refinement) and VMM_BA_CAL_SINGULAR (a pivot of the undamped reduced system at or
 *               below 1e-13 C_jj / S_jj) are vmm_ba_calibrate's.
 *   gauge       at least one camera must be held: a refine_mask with all n_rig_cams bits set, or with bits at or above
 *               n_rig_cams, is VMM_BA_ERR_ARGUMENT.  The default (a null o, or the value
 *               vmm_ba_default_rig_calibrate_options sets) is every camera of the rig but camera 0.
 *   result      ext_qt; ext_cov = S^-1, row-major 6K x 6K in the order of the cameras, cross blocks between cameras
 *               included; rig_cov_f = A_f^-1 + A_f^-1 B_f S^-1 B_f' A_f^-1, the marginal of the JOINT problem; both from
 *               the undamped system at the result with the loss applied.  rep->cams_refined: bit c = extrinsic c moved.
 * Results are bit-identical from run to run; the sum over the frames has a fixed order, so the bits DO depend on the
 * order of the frames in the batch.  n_frames == 0 returns VMM_BA_OK, ext_qt = ext_qt0 and VMM_BA_CAL_NO_IMAGES without a
 * device call. */
typedef struct vmm_ba_rig_calibrate_options {
    vmm_ba_localize_options loc; /* the initial localisation under the starting extrinsics */
    int32_t max_trials;          /* 100: LM trials (accepted + rejected) of one refinement */
    int32_t refine_mask;         /* bit c = extrinsic c is refined; default: every camera but 0 */
    int32_t robustify;           /* 1 */
    int32_t reclassify_passes;   /* 2 */
    int32_t min_inlier_tags;     /* 2: a frame with fewer inliers takes no part */
    int32_t reserved;
    double  huber_a;             /* 1.0 */
    double  inlier_px;           /* 8.0 */
} vmm_ba_rig_calibrate_options;
typedef struct vmm_ba_rig_calibrate_report {
    int32_t status;              /* VMM_BA_CAL_* */
    int32_t trials, accepted, passes, n_frames_used, n_obs_used, cams_refined, reserved;
    double  initial_cost, final_cost, initial_rms_px, final_rms_px, time_s;
} vmm_ba_rig_calibrate_report;
void vmm_ba_default_rig_calibrate_options(vmm_ba_rig_calibrate_options* o);
int vmm_ba_rig_calibrate(int32_t n_rig_cams, const double* intr, const double* dist, const double* ext_qt0,
                         int32_t n_tags, const double* tag_qt, const double* tag_wh,
                         int32_t n_frames, const int64_t* img_start,
                         const int32_t* obs_tag, const double* obs_px,
                         const vmm_ba_rig_calibrate_options* o,
                         double* ext_qt,               /* [7*K] */
                         double* ext_cov,              /* [(6K)*(6K)] or NULL */
                         double* rig_qt,               /* [7*n_frames] */
                         double* rig_cov,              /* [36*n_frames] or NULL: the joint marginals */
                         uint8_t* obs_inlier,          /* [n_obs] or NULL */
                         vmm_ba_localize_result* res,  /* [n_frames] or NULL */
                         vmm_ba_rig_calibrate_report* rep, /* or NULL */
                         int device);

/* ABI 6, additive.  Triangulates n_pts free points (anything that is not a tag: a drill hole, an LED, a clicked feature,
 * or a tag's own corners taken one by one) from the cameras of a finished map or of a localisation; the dual of
 * vmm_ba_localize and stateless like it, every point independent of the others in the batch.  Point p owns the
 * observations [pt_start[p], pt_start[p + 1]): obs_cam names the camera (strictly increasing within a point, so one
 * image appears at most once in a track and the caller's ordering cannot change a result), obs_uv the pixel.
 *   residual    the cost functor's projection of R X + t (q / |q| first) against the pixel: what the bundle adjustment
 *               and the localisation minimise, not CameraModel::projectPoint.  An observation whose point is not in front
 *               of its camera (Z <= 0) is never an inlier, adds score_cap_px^2 to a score, and makes the cost of a
 *               refinement trial +inf (the trial is rejected).
 *   rays        every pixel undistorted (20 fixed-point iterations of the functor's distortion) and turned into the world
 *               ray through the camera centre c = -R^T t.
 *   candidates  candidate 0: the least-squares point of all rays, sum (I - d d^T) X = sum (I - d d^T) c; candidates 1..:
 *               the same solve on the two rays (a, b), a < b < min(n_obs, max_pair_views), in lexicographic order.  A
 *               system that is not positive definite (parallel rays) gives no candidate.
 *   winner      most observations within inlier_px (and Z > 0); ties to the lowest sum min(e^2, score_cap_px^2) over ALL
 *               the point's observations; then to the lowest candidate index.  (The count comes first, unlike the
 *               localisation's rule: at low parallax a pair that contains a gross outlier can put the point at a depth
 *               where the clean views miss by only tens of pixels, and the truncated sum alone then prefers it.)
 *   passes      reclassify_passes times: an observation is an inlier when its distance is at most inlier_px and Z > 0;
 *               then Levenberg-Marquardt on the 3 coordinates over the inliers, minimising 1/2 sum rho(|r|^2), until the
 *               cost is at its rounding floor or refine_iterations trials are spent.  A pass that finds fewer than
 *               min_inlier_views inliers ends the passes.  reclassify_passes == 0: one refinement over all observations
 *               in front of their camera.
 *   result      obs_inlier = the classification at the returned point; rms_px and cost over those inliers;
 *               xyz_cov = H^-1 (row-major 3x3), H = sum rho'_i Jp_i^T Jp_i over the inliers, the loss applied when
 *               robustify != 0 (as the tag translation covariance above): the part the pixel noise (unit variance)
 *               causes, the cameras taken as exact.
 *               xyz_cov_cams = H^-1 (sum_i G_i C_i G_i^T) H^-1, G_i = rho'_i Jp_i^T Jc_i (3x6), Jc_i the 2x6 Jacobian over
 *               camera i's tangent (translation, then half-angle rotation) and C_i = cam_cov[36 i ..], camera i's 6x6
 *               marginal in that order (vmm_ba_covariance_blocks' or vmm_ba_localize's): first-order propagation of
 *               each camera's own uncertainty.  It IGNORES THE CORRELATIONS BETWEEN CAMERAS (the cross blocks of the
 *               map's covariance), which a bundle adjustment leaves positive between neighbours: treat it as the
 *               independent-cameras figure.  Zeros when cam_cov is NULL.  The total is the sum of the two parts.
 * Status per point: TOO_FEW_VIEWS (fewer than 2 observations): xyz = 0, zero covariances, zero flags.  NO_CANDIDATE
 * (every candidate non-finite): the same.  TOO_FEW_INLIERS (fewer than min_inlier_views at the returned point): the
 * best-effort point and its flags, zero covariances.  SINGULAR: H is not positive definite; point and flags are
 * returned, both covariances are zeros.  No output is ever NaN; results are bit-identical from run to run and do not
 * depend on what else is in the batch or on where the point sits in it.
 * VMM_BA_ERR_ARGUMENT (before any device call): null intr, dist, pt_start or xyz; negative sizes; pt_start not starting
 * at 0 or decreasing; null observations while n_obs > 0; obs_cam outside [0, n_cams) or not strictly increasing within
 * a point; a non-finite camera model, pose, pixel or cam_cov; a zero quaternion; bad options.  n_pts == 0 returns
 * VMM_BA_OK without a device call, and so does a batch in which no point has two observations. */
enum { VMM_BA_TRI_OK = 0, VMM_BA_TRI_TOO_FEW_VIEWS = 1, VMM_BA_TRI_NO_CANDIDATE = 2,
       VMM_BA_TRI_TOO_FEW_INLIERS = 3, VMM_BA_TRI_SINGULAR = 4 };

typedef struct vmm_ba_triangulate_options {
    int32_t refine_iterations;   /* 30: LM trials (accepted + rejected) of one refinement */
    int32_t robustify;           /* 1: HuberLoss(huber_a) per observation */
    double  huber_a;             /* 1.0 */
    double  score_cap_px;        /* 100 */
    double  inlier_px;           /* 8.0 */
    int32_t reclassify_passes;   /* 2 */
    int32_t min_inlier_views;    /* 2 */
    int32_t max_pair_views;      /* 16, in [2, 64]: two-ray candidates are formed among the first this-many observations */
    int32_t reserved;
} vmm_ba_triangulate_options;

typedef struct vmm_ba_triangulate_result {   /* one per point */
    int32_t status, n_obs, n_inlier_obs, trials;
    double  rms_px, cost;
} vmm_ba_triangulate_result;

void vmm_ba_default_triangulate_options(vmm_ba_triangulate_options* o);
int vmm_ba_triangulate(const double intr[4], const double dist[5],
                       int32_t n_cams, const double* cam_qt,      /* [7*n_cams] world->camera: the map's or the localisation's */
                       const double* cam_cov,                     /* [36*n_cams] 6x6 per camera, tangent order, or NULL */
                       int32_t n_pts, const int64_t* pt_start,    /* [n_pts+1], CSR */
                       const int32_t* obs_cam, const double* obs_uv,   /* [n_obs], [2*n_obs] */
                       const vmm_ba_triangulate_options* o,
                       double* xyz,                 /* [3*n_pts] */
                       double* xyz_cov,             /* [9*n_pts] or NULL: measurement part */
                       double* xyz_cov_cams,        /* [9*n_pts] or NULL: part propagated from cam_cov (zeros when cam_cov is NULL) */
                       uint8_t* obs_inlier,         /* [n_obs] or NULL */
                       vmm_ba_triangulate_result* res, /* [n_pts] or NULL */
                       int device);

/* ABI 6, additive.  Locates n_tags tags from cameras that are already known: the 6-DoF pose of every tag from its own
 * observations, with a covariance.  The dual of vmm_ba_localize (the roles of camera and tag swapped) and stateless like
 * it, every tag independent of the others in the batch.  Tag t owns the observations [tag_start[t], tag_start[t + 1]):
 * obs_cam names the camera (strictly increasing within a tag, so one image appears at most once and the caller's
 * ordering cannot change a result), obs_px the four corners.  It reuses vmm_ba_localize_options and
 * vmm_ba_localize_result with the VMM_BA_LOC_* statuses, one result per tag; min_inlier_tags counts the tag's inlier
 * observations.  Per tag:
 *   candidates  the two planar solutions of each of its observations chained through the observing camera,
 *               T_cam^-1 o T_rel; each scored by sum min(e^2, score_cap_px^2) over ALL the tag's corners in all its
 *               observations with the residual the bundle adjustment minimises; lowest wins, ties to the lowest
 *               observation then solution 0, non-finite loses
 *   passes      reclassify_passes times: an observation is an inlier when its largest corner distance is at most
 *               inlier_px; then Levenberg-Marquardt on the tag's 6 tangent degrees of freedom (translation, then
 *               half-angle rotation) over the inliers, minimising 1/2 sum rho(|r_corner|^2), until the cost is at its
 *               rounding floor or refine_iterations trials are spent.  A pass that finds fewer than min_inlier_tags
 *               inliers ends the passes.  reclassify_passes == 0: one refinement over all observations.
 *   result      tag_qt = tag->world, as the map stores it; obs_inlier = the classification at the returned pose; rms_px
 *               and cost over those inliers;
 *               tag_cov = H^-1 (row-major 6x6, the order vmm_ba_covariance_blocks uses for a tag), H = sum rho' Jt^T Jt
 *               over the inliers' corners, the loss applied when robustify != 0: the part the pixel noise (unit
 *               variance) causes, the cameras taken as exact.
 *               tag_cov_cams = H^-1 (sum_i G_i C_i G_i^T) H^-1, G_i = sum over observation i's four corners of
 *               rho' Jt^T Jc (6x6), Jc the 2x6 Jacobian over the observing camera's tangent and
 *               C_i = cam_cov[36 obs_cam[i] ..], that camera's 6x6 marginal in the same order (vmm_ba_covariance_blocks'
 *               or vmm_ba_localize's): first-order propagation of each camera's own uncertainty.  It IGNORES THE
 *               CORRELATIONS BETWEEN CAMERAS (the cross blocks of the map's covariance), which a bundle adjustment leaves
 *               positive between neighbours: treat it as the independent-cameras figure.  Zeros when cam_cov is NULL.
 *               The total is the sum of the two parts.  Both matrices are symmetric to the last bit.
 * NO_OBSERVATIONS / NO_CANDIDATE (every planar solution of the tag degenerate): pose (1,0,0,0, 0,0,0), zero covariances,
 * zero flags.  TOO_FEW_INLIERS (fewer than min_inlier_tags at the returned pose): the best-effort pose and its flags,
 * zero covariances.  SINGULAR: H is not positive definite; pose and flags are returned, both covariances are zeros.
 * No output is ever NaN; a tag gives the same bits alone, in any batch, at any position and from run to run.
 * VMM_BA_ERR_ARGUMENT (before any device call): null intr, dist, tag_start or tag_qt; negative sizes; tag_start not
 * starting at 0 or decreasing; null observations while n_obs > 0; obs_cam outside [0, n_cams) or not strictly increasing
 * within a tag; a non-finite camera model, pose, size, pixel or cam_cov; a zero quaternion; bad options.  n_tags == 0
 * returns VMM_BA_OK without a device call. */
int vmm_ba_locate_tags(const double intr[4], const double dist[5],
                       int32_t n_cams, const double* cam_qt,      /* [7*n_cams] world->camera: the map's or the localisation's */
                       const double* cam_cov,                     /* [36*n_cams] 6x6 per camera, tangent order, or NULL */
                       int32_t n_tags, const double* tag_wh,      /* [2*n_tags] width, height */
                       const int64_t* tag_start,                  /* [n_tags+1], CSR over tags */
                       const int32_t* obs_cam, const double* obs_px,   /* [n_obs], [8*n_obs] */
                       const vmm_ba_localize_options* o,
                       double* tag_qt,              /* [7*n_tags] tag->world */
                       double* tag_cov,             /* [36*n_tags] or NULL: measurement part */
                       double* tag_cov_cams,        /* [36*n_tags] or NULL: part propagated from cam_cov (zeros when cam_cov is NULL) */
                       uint8_t* obs_inlier,         /* [n_obs] or NULL */
                       vmm_ba_localize_result* res, /* [n_tags] or NULL */
                       int device);

/* ABI 6, additive.  Predicts how well a camera would be localised against a finished map at poses that have no image
 * behind them: which tags it would see, and the covariance vmm_ba_localize would report there.  Stateless like
 * vmm_ba_localize, every pose independent of the others in the batch.
 *   visibility  Tag t counts as visible from pose p when all of the following hold.
 *               - All four corners have z_cam > min_depth.
 *               - At all four corners the radial map is still rising at that radius: with r^2 the squared normalised
 *                 radius, 1 + 3 k1 r^2 + 5 k2 r^4 + 7 k3 r^6 > 0.  Without this, a corner far outside the field of view
 *                 of a lens with k1 < 0 folds back into the image.  (A model that folds and unfolds again inside that
 *                 radius is not detected.)
 *               - All four predicted pixels (u, v) satisfy margin_px <= u <= width - margin_px and
 *                 margin_px <= v <= height - margin_px.  The pixel is that of the functor the bundle adjustment
 *                 minimises, not CameraModel::projectPoint's aliased form.
 *               - The tag faces the camera.  Let n = R_tag e_z.  Corners run LL, LR, UR, UL, counter-clockwise seen from
 *                 +z, so +z is the printed side.  Let c be the tag's centre and C = -R^T t the camera centre.  Then
 *                 n.(C - c) >= cos(max_view_angle) |C - c|.
 *               - The shortest of the four projected sides is at least min_side_px.
 *               OCCLUSION IS NOT MODELLED: a tag hidden by a wall counts as visible.
 *   covariances The sums run over the visible tags, in the tangent every pose of the library moves in (translation,
 *               then the half-angle rotation of vmm_ba_pose_plus).
 *               cov_px = sigma_px^2 H^-1, H = sum Jc^T Jc over the 4 corners of every visible tag, Jc the 2x6 camera
 *               Jacobian of the residual the bundle adjustment minimises.  No loss is applied: the expected residual
 *               is zero and the Huber weight is 1 there.  Row-major 6x6, symmetric to the last bit.
 *               cov_map = H^-1 M H^-1, M = sum_t G_t S_t G_t^T, G_t = sum over tag t's corners of Jc^T Jt (6x6, Jt the 2x6
 *               Jacobian over the tag's tangent) and S_t = tag_cov[36 t ..], the tag's 6x6 marginal in the order
 *               vmm_ba_covariance_blocks uses: the first-order response of the minimiser,
 *               dx = -H^-1 sum_t G_t dy_t, with independent tags.  Like vmm_ba_triangulate's camera part, it ignores the
 *               correlations between tags.  Neighbouring tags far from the origin move together, so for them this errs
 *               towards too small.  Zeros when tag_cov is NULL.
 *               sigma_pos_m and sigma_rot_rad come from cov_px + cov_map: the rotation in radians is twice the
 *               tangent's rotation part, and the camera centre C = -R^T t answers a tangent step (dt, dr) with
 *               dC = -R^T (dt + 2 [t]x dr).
 *   statuses    NO_VISIBLE_TAG (n_visible == 0), TOO_FEW_TAGS (n_visible < min_tags) and SINGULAR (H is not positive
 *               definite, or a result would not be finite): zero covariances and zero sigmas; n_visible and the visible
 *               bytes are still those of the rules above.
 * The predicted covariance is local: with one visible tag it says nothing of the two-fold planar ambiguity of a single
 * tag's pose; min_tags is the caller's lever.
 * No output is ever NaN; a pose gives the same bits alone, in any batch, at any position and from run to run.
 * VMM_BA_ERR_ARGUMENT (before any device call): null intr, dist, cam_qt or o; negative sizes; a null map with
 * n_tags > 0; a non-finite camera model, map pose, size, pose or tag_cov; a zero quaternion; image_width or
 * image_height <= 0; sigma_px not finite or <= 0; a negative or non-finite margin_px, min_depth or min_side_px;
 * max_view_angle_deg outside (0, 90]; min_tags < 1.  n_poses == 0 returns VMM_BA_OK without a device call; so does
 * n_tags == 0, where every pose is NO_VISIBLE_TAG. */
enum { VMM_BA_PRED_OK = 0, VMM_BA_PRED_NO_VISIBLE_TAG = 1, VMM_BA_PRED_TOO_FEW_TAGS = 2, VMM_BA_PRED_SINGULAR = 3 };
typedef struct vmm_ba_predict_options {
    int32_t image_width, image_height;  /* no default: must be > 0 (CameraModel's horizontal/verticalResolution) */
    double  sigma_px;                   /* 1.0: standard deviation of one corner coordinate */
    double  margin_px;                  /* 0.0: a corner must lie this far inside the image */
    double  min_depth;                  /* 1e-3: a corner must have z_cam > min_depth */
    double  max_view_angle_deg;         /* 70: angle between the tag's normal and the line tag centre -> camera centre */
    double  min_side_px;                /* 10: shortest of the four projected sides */
    int32_t min_tags;                   /* 1: fewer visible tags -> TOO_FEW_TAGS */
    int32_t reserved;
} vmm_ba_predict_options;

typedef struct vmm_ba_predict_result {  /* one per pose */
    int32_t status;                     /* VMM_BA_PRED_* */
    int32_t n_visible;
    double  sigma_pos_m;                /* sqrt(trace of the camera CENTRE's 3x3 covariance in the world), cov_px + cov_map */
    double  sigma_rot_rad;              /* sqrt(trace of the rotation's 3x3 covariance in radians), cov_px + cov_map */
} vmm_ba_predict_result;

void vmm_ba_default_predict_options(vmm_ba_predict_options* o);
int vmm_ba_predict_localization(const double intr[4], const double dist[5],
                                int32_t n_tags, const double* tag_qt, const double* tag_wh,   /* the map, as vmm_ba_localize */
                                const double* tag_cov,       /* [36*n_tags] tangent order as vmm_ba_covariance_blocks, or NULL */
                                int32_t n_poses, const double* cam_qt,   /* [7*n_poses] world->camera */
                                const vmm_ba_predict_options* o,
                                double* cov_px,              /* [36*n_poses] or NULL */
                                double* cov_map,             /* [36*n_poses] or NULL */
                                uint8_t* visible,            /* [n_poses*n_tags] or NULL */
                                vmm_ba_predict_result* res,  /* [n_poses] or NULL */
                                int device);

/* ABI 6, additive.  vmm_ba_predict_localization with the map's tags correlated: what it says holds here word for word,
 * but for two arguments and for cov_map.
 *   tag_cov_joint  The tags' joint covariance, [36 * n_tags * n_tags] doubles block-major: block (s, t) is the row-major
 *               6x6 at 36 (s n_tags + t), which is what vmm_ba_covariance_blocks writes for the pair list
 *               (n_cams + s, n_cams + t) with s the outer loop.  Required when n_tags > 0.  Only the blocks with s >= t are
 *               read; S_ts is taken as S_st^T.  The diagonal blocks are read in full as given, as tag_cov is.  The upper
 *               block triangle may hold anything, NaN included: it is neither validated nor touched.
 *   visible_in  [n_poses * n_tags] or NULL.  When given, the visibility rules are not evaluated: tag t takes part in pose
 *               p exactly when visible_in[p n_tags + t] != 0, and `visible` repeats it as 0 / 1.  This is how the inlier
 *               set of a real localisation is fed in.  A pose with a selected tag that has a corner at or behind the
 *               camera's plane (z_cam <= 0, where the projection means nothing), or whose sums come out non-finite or
 *               with an indefinite H, is SINGULAR.
 *   cov_map     H^-1 M H^-1 with M = sum_{s in V} G_s S_ss G_s^T + sum_{s in V} sum_{t in V, t < s} (X_st + X_st^T),
 *               X_st = G_s S_st G_t^T, V the visible (selected) tags of the pose: the covariance of the first-order
 *               response dx = -H^-1 sum_t G_t dy_t under the joint covariance of the dy_t.  On a block-diagonal
 *               tag_cov_joint it is vmm_ba_predict_localization's cov_map up to rounding; cov_px is its cov_px bit for
 *               bit.  sigma_pos_m and sigma_rot_rad come from cov_px + cov_map by the same formulas.
 * OCCLUSION IS STILL NOT MODELLED.  With visible_in taken from a robust localisation, the response is that of the plain
 * least-squares minimiser over the selected tags (unit weights, no loss), not of the robust one.
 * No output is ever NaN; the matrices are symmetric to the last bit; a pose gives the same bits alone, in any batch, at
 * any position and from run to run.  Statuses, and the zero outputs that go with them, as above.
 * VMM_BA_ERR_ARGUMENT (before any device call): what vmm_ba_predict_localization rejects; a null tag_cov_joint with
 * n_tags > 0; a non-finite entry in a block with s >= t.  VMM_BA_ERR_HIP with the byte count in the message when the
 * device memory, 288 n_tags^2 bytes of it for tag_cov_joint, cannot be allocated.  n_poses == 0 and n_tags == 0 return
 * VMM_BA_OK without a device call, as above. */
int vmm_ba_predict_localization_joint(const double intr[4], const double dist[5],
                                      int32_t n_tags, const double* tag_qt, const double* tag_wh,
                                      const double* tag_cov_joint,   /* [36*n_tags*n_tags] block-major; blocks s >= t are read */
                                      int32_t n_poses, const double* cam_qt,   /* [7*n_poses] world->camera */
                                      const uint8_t* visible_in,     /* [n_poses*n_tags] or NULL: the selection */
                                      const vmm_ba_predict_options* o,
                                      double* cov_px,              /* [36*n_poses] or NULL */
                                      double* cov_map,             /* [36*n_poses] or NULL */
                                      uint8_t* visible,            /* [n_poses*n_tags] or NULL */
                                      vmm_ba_predict_result* res,  /* [n_poses] or NULL */
                                      int device);

/* ABI 6, additive.  Calibrates a camera against a finished map: the nine numbers of the camera model
 * (fx, fy, cx, cy, k1, k2, p1, p2, k3) and one pose per image, the map held fixed.  Stateless like vmm_ba_localize.
 *   objective   1/2 sum rho(|r_corner|^2) over the inlier observations of the images that take part, with the residual
 *               the bundle adjustment and the localisation minimise (the cost functor's projection, not
 *               CameraModel::projectPoint, which differs in the tangential y term).
 *   start       vmm_ba_localize's own steps under intr0 / dist0 and o->loc.  An image that is not VMM_BA_LOC_OK, or has
 *               fewer than min_inlier_tags inlier observations, takes no part: it keeps the pose, flags and result the
 *               localisation gave it and gets a zero cam_cov.
 *   refinement  Levenberg-Marquardt on all poses and the parameters in refine_mask at once, Marquardt damping
 *               lam diag on the pose blocks and on the 9 x 9 block; every image's 6 x 6 block is eliminated and the 9 x 9
 *               reduced system is solved Jacobi-scaled.  A trial with a strictly lower finite cost is accepted (lam x 0.1),
 *               any other rejected (lam x 10).  The loop stops when a rejected trial's cost equals the current one to
 *               rounding, when the step is negligible (every pose-tangent component and every |dk_j| / max(|k_j|, 1)
 *               below 1e-10 on a rejected trial, 1e-14 on any), or when lam passes 1e12; VMM_BA_CAL_NO_CONVERGENCE when
 *               max_trials (accepted + rejected) ran out first -- the best state is still returned.
 *               reclassify_passes times afterwards: every observation of the localised images is classified again under
 *               the current model and poses (inlier: largest corner distance at most inlier_px), who takes part is
 *               decided again from the new counts, and the refinement runs again.  The status is the last refinement's.
 *   mask        a parameter outside refine_mask has zero columns, a unit diagonal and a zero step: it comes back with
 *               the bits it went in with, and its rows and columns of intr_cov are zero.
 *   result      intr / dist; cam_qt; obs_inlier = the inlier set the last refinement minimised over; res = the
 *               localisation's results with n_inlier_obs, rms_px and cost of the images that took part taken at the result.
 *   covariance  at the result, from the undamped system with the loss applied (as the tag translation covariance above):
 *               intr_cov = S^-1 with S = sum_i (C_i - B_i' A_i^-1 B_i); cam_cov_i = A_i^-1 + A_i^-1 B_i S^-1 B_i' A_i^-1,
 *               the marginal of the JOINT problem (wider than vmm_ba_localize's, which takes the model as known).
 *               VMM_BA_CAL_SINGULAR: S or an A_i is not positive definite (S: a Cholesky pivot at or below 1e-13 of
 *               its entry of diag(sum C_i), the scale of S's rounding errors); both covariances are zeros, parameters
 *               and poses are still returned.
 * VMM_BA_CAL_NO_IMAGES: no image takes part; intr / dist are the start values, cam_cov and intr_cov zeros.
 * No output is ever NaN.  Results are bit-identical from run to run for the same batch; the sum over the images has a
 * fixed order, so the bits DO depend on the order of the images in the batch (unlike vmm_ba_localize).
 * VMM_BA_ERR_ARGUMENT (before any device call): what vmm_ba_localize rejects, a refine_mask outside [0, 0x1FF], bad
 * tolerances or counts, null intr / dist.  n_imgs == 0 returns VMM_BA_OK with intr / dist copied from the start
 * values and status NO_IMAGES, without a device call. */
enum { VMM_BA_CAL_OK = 0, VMM_BA_CAL_NO_IMAGES = 1, VMM_BA_CAL_SINGULAR = 2, VMM_BA_CAL_NO_CONVERGENCE = 3 };
typedef struct vmm_ba_calibrate_options {
    vmm_ba_localize_options loc; /* the initial localisation under the starting intrinsics, as vmm_ba_localize runs it */
    int32_t max_trials;          /* 100: LM trials (accepted + rejected) of one joint refinement */
    int32_t refine_mask;         /* 0x1FF: bit i set = parameter i of (fx,fy,cx,cy,k1,k2,p1,p2,k3) is refined */
    int32_t robustify;           /* 1 */
    int32_t reclassify_passes;   /* 2: after a joint refinement, reclassify every observation at inlier_px and refine again */
    int32_t min_inlier_tags;     /* 2: an image with fewer inlier observations takes no part */
    int32_t reserved;
    double  huber_a;             /* 1.0 */
    double  inlier_px;           /* 8.0 */
} vmm_ba_calibrate_options;
typedef struct vmm_ba_calibrate_report {
    int32_t status, trials, accepted, passes, n_images_used, n_obs_used;
    double initial_cost, final_cost, initial_rms_px, final_rms_px, time_s;
} vmm_ba_calibrate_report;
void vmm_ba_default_calibrate_options(vmm_ba_calibrate_options* o);
int vmm_ba_calibrate(const double intr0[4], const double dist0[5],
                     int32_t n_tags, const double* tag_qt, const double* tag_wh,
                     int32_t n_imgs, const int64_t* img_start, const int32_t* obs_tag, const double* obs_px,
                     const vmm_ba_calibrate_options* o,
                     double intr[4], double dist[5],       /* result */
                     double* intr_cov,                     /* [81] row-major 9x9, or NULL */
                     double* cam_qt,                       /* [7*n_imgs] */
                     double* cam_cov,                      /* [36*n_imgs] or NULL: the JOINT marginal */
                     uint8_t* obs_inlier,                  /* [n_obs] or NULL */
                     vmm_ba_localize_result* res,          /* [n_imgs] or NULL */
                     vmm_ba_calibrate_report* rep,         /* or NULL */
                     int device);

/* ABI 6, additive.  The camera model of a handle.  Every entry point takes it from vmm_ba_problem.intr / dist at create;
 * vmm_ba_set_intrinsics replaces it, after which every entry (cost, eval_blocks, solve, initialize, reprojection_stats,
 * the covariances) behaves as a handle created with the new numbers -- the captured iteration graph holds the model by
 * value and is dropped, the next solve captures again.  intr = fx, fy, cx, cy; dist = k1, k2, p1, p2, k3.
 * VMM_BA_ERR_ARGUMENT for null pointers or non-finite numbers; VMM_BA_ERR_STATE for world_size > 1 or
 * VMM_BA_LANDMARK_POINTS handles (as vmm_ba_covariance_blocks), after the argument checks.  vmm_ba_get_intrinsics
 * works on every handle and makes no device call. */
int vmm_ba_set_intrinsics(vmm_ba_handle h, const double intr[4], const double dist[5]);
int vmm_ba_get_intrinsics(vmm_ba_handle h, double intr[4], double dist[5]);

/* ABI 6, additive.  The camera-model part of the joint problem "cameras + tags + camera model" at the current state and
 * the handle's model, k = (fx, fy, cx, cy, k1, k2, p1, p2, k3), J_k the Jacobian of the residuals over k:
 *   cost          1/2 sum rho(|r|^2) over the active observations
 *   g_k[9], C[81] J_k^T r and J_k^T J_k (row-major) over the active observations
 *   r_k[9]        g_k - B^T A^-1 g      with A the pose normal matrix (cameras and tags), g the pose gradient and B the
 *   S_k[81]       C - B^T A^-1 B        stack of the 6 x 9 blocks sum J_pose^T J_k: the reduced system of the camera
 *                                       model with every pose eliminated (row-major, symmetric in its bits)
 * Undamped and unscaled, the loss applied when robustify != 0 as everywhere else (rows and residuals scaled by
 * sqrt(rho')).  The observation mask and the constant-pose flags are honoured: a switched-off observation contributes
 * nothing; a constant pose has a zero block of B, its observations still feed C, g_k and the other pose's block.
 * S_k^-1 is the covariance of the camera model with the poses marginalised; -S_k^-1 r_k its Gauss-Newton step.
 * The call leaves the state alone and is idempotent; a block-sparse or tree-ordered handle switches to the dense,
 * naturally ordered system for the call, as vmm_ba_covariance_blocks.  Every sum has a fixed order: the results are
 * bit-identical from run to run.  Any output may be NULL.
 * n_obs == 0 or no active observation: zeros.  VMM_BA_ERR_ARGUMENT for a null handle, VMM_BA_ERR_STATE for
 * world_size > 1 or VMM_BA_LANDMARK_POINTS handles, VMM_BA_ERR_NUMERIC if A is not positive definite. */
int vmm_ba_intrinsics_system(vmm_ba_handle h, int robustify, double huber_a, double* cost, double g_k[9], double C[81],
                             double r_k[9], double S_k[81]);

/* ABI 6, additive.  Bundle adjustment with the camera model refined: cameras, tags and the parameters of refine_mask at
 * one optimum of 1/2 sum rho(|r|^2), and the covariance of the model with the poses marginalised.
 *   start       one vmm_ba_solve(h, inner).  refine_mask == 0: that is all -- poses and *last_inner are those of a plain
 *               vmm_ba_solve, outer_iterations == 0.
 *   iteration   vmm_ba_intrinsics_system at the current state; a parameter outside refine_mask gets a unit row and a zero
 *               step (it comes back with the bits it went in with); (S_k + lam diag S_k) dk = -r_k is solved on the host,
 *               Jacobi-scaled; the poses are saved, the model becomes k + dk, vmm_ba_solve(h, inner) runs from the current
 *               poses.  A strictly lower finite cost: accepted, lam x 0.1 (from 1e-4).  Otherwise poses and model are
 *               restored exactly and lam x 10.
 *   stop        VMM_BA_CAL_OK: an accepted step with every |dk_j| / max(|k_j|, 1) below parameter_tolerance; an accepted
 *               step whose relative cost decrease is below function_tolerance; a rejected step whose cost equals the
 *               current one to rounding; lam past 1e12.  VMM_BA_CAL_NO_CONVERGENCE: max_outer_iterations (accepted +
 *               rejected) ran out; the best state is kept.  VMM_BA_CAL_SINGULAR: S_k is not positive definite (a Cholesky
 *               pivot of its unit-diagonal scaling at or below 1e-13 C_jj / S_jj, as vmm_ba_calibrate); poses and model
 *               are those of the first solve, intr_cov is zeros.
 *   result      the handle holds the returned poses (vmm_ba_get_state) and model (intr / dist, vmm_ba_get_intrinsics);
 *               intr_cov = S_k^-1 at the result over the free parameters, rows and columns of the others zero;
 *               *last_inner (optional) is the summary of the last vmm_ba_solve the call made, rejected trials included.
 *   inner       the outer loop compares the costs of consecutive solves: `inner` should stop well below the outer
 *               function_tolerance (the defaults of vmm_ba_default_options stop at a relative cost decrease of 1e-6,
 *               which leaves the model accurate to about that; function_tolerance 1e-14 and parameter_tolerance 1e-12
 *               are what TagReconstructor.doBundleAdjustment(refineCameraModel) passes).
 * No output is ever NaN.  Two calls from the same start give identical bytes (time_s aside).
 * The iteration graph is captured again after every change of the model: once per outer iteration.
 * VMM_BA_ERR_ARGUMENT: null handle, report, intr or dist; refine_mask outside [0, 0x1FF]; negative counts or tolerances.
 * VMM_BA_ERR_STATE: world_size > 1 or VMM_BA_LANDMARK_POINTS.  VMM_BA_ERR_NUMERIC: the pose system is not positive
 * definite at an iterate.  Errors of the inner solve are passed on. */
typedef struct vmm_ba_selfcal_options {
    int32_t max_outer_iterations;   /* 30: trials (accepted + rejected) of the outer loop */
    int32_t refine_mask;            /* 0x1FF: bit i set = parameter i of (fx,fy,cx,cy,k1,k2,p1,p2,k3) is refined */
    double parameter_tolerance;     /* 1e-10 */
    double function_tolerance;      /* 1e-12 */
} vmm_ba_selfcal_options;
typedef struct vmm_ba_selfcal_report {
    int32_t status;                 /* VMM_BA_CAL_OK / _SINGULAR / _NO_CONVERGENCE */
    int32_t outer_iterations;       /* trials of the outer loop */
    int32_t accepted;
    int32_t inner_lm_iterations;    /* num_lm_iterations summed over every vmm_ba_solve of the call */
    double initial_cost;            /* final cost of the first solve: the optimum under the starting model */
    double final_cost;
    double time_s;                  /* host wall time of the call */
} vmm_ba_selfcal_report;
void vmm_ba_default_selfcal_options(vmm_ba_selfcal_options* o);
int vmm_ba_solve_selfcal(vmm_ba_handle h, const vmm_ba_options* inner, const vmm_ba_selfcal_options* o,
                         vmm_ba_summary* last_inner, vmm_ba_selfcal_report* report, double intr[4], double dist[5],
                         double* intr_cov /* [81] row-major 9x9, or NULL */);

/* Test/diagnostic: one residual+Jacobian evaluation at the current state; copies out the
 * accumulated normal-equation blocks in the caller's index space.  Any output may be NULL.
 *   V[36*n_cams], U[36*n_tags]  row-major 6x6 J^T J diagonal blocks (Huber-corrected, unscaled)
 *   W[36*n_obs]                 row-major 6x6 J_cam^T J_tag per observation, caller's order
 *   g_cam[6*n_cams], g_tag[6*n_tags]  J^T r                                               */
int vmm_ba_eval_blocks(vmm_ba_handle h, int robustify, double huber_a, double* cost, double* V,
                       double* U, double* W, double* g_cam, double* g_tag);

/* Test/diagnostic: solves A x = b for a dense SPD A (row-major n x n, host memory) with the
 * engine's blocked Cholesky and triangular solves; reports failure through *info != 0. */
int vmm_ba_dense_spd_solve(int device, int n, const double* A, const double* b, double* x, int* info);

/* Test/diagnostic: C = Z^T Z (n x n, row-major, lower triangle valid) for a row-major k x n Z with
 * the engine's MFMA kernel. */
int vmm_ba_dense_syrk(int device, int k, int n, const double* Z, double* C);

/* Test/diagnostic: out[i] = Plus(qt[i], delta[i]) for n poses (7 doubles each, tangent 6 each) with the engine's own
 * device function -- QuaternionParameterization::Plus on the rotation, plain addition on the translation
 * (src/TagReconstructor.cpp:665-666,692-693 attach it to every q block; tangent order: translation, rotation). */
int vmm_ba_pose_plus(int64_t n, const double* qt, const double* delta, double* out, int device);

/* Diagnostic (can the reduced-system assembly hide behind the factorisation?): ms[0] rank-k update + sum
 * alone, ms[1] factorisation + triangular solves alone, ms[2] both back to back on one stream, ms[3] both at once on
 * two streams (no data dependency between them in this measurement), ms[4] the factorisation's own duration in that
 * concurrent run, ms[5] the rank-k update + sum's; ms[6], ms[7]: total and factorisation when the rank-k update is
 * enqueued first.  ms holds 8 doubles.  Dense elimination, one GPU. */
int vmm_ba_debug_overlap(vmm_ba_handle h, int reps, double* ms);

/* Test hook, host logic only (no device needed): the launch schedule of the launch-per-column Cholesky
 * (csrc/kernels_chol_step.hip, chol_step_schedule) for a system of n_blk 64-column blocks whose trailing n_df block columns go
 * to the one-launch kernel (n_df < 0: the library's own choice for a chip of n_cu compute units).  launches[i] =
 * { k (-1: update-only hand-over launch), lazy0, lazy1, upd0, upd1 (panel numbers, -1: none), c0, t0, t1 }; at most
 * `cap` rows are written, *n_launches is the full count, *n_df_used the tail length.  vmm_ba_debug_chol_tile returns the
 * (block row, block column) of tile t of such a launch's update list. */
int vmm_ba_debug_chol_schedule(int n_blk, int n_df, int n_cu, int32_t* launches, int cap, int* n_launches, int* n_df_used);
int vmm_ba_debug_chol_tile(int n_blk, const int32_t* launch, int t, int* bi, int* bj);

/* Times each kernel of an LM iteration at the current state (reps launches each). */
int vmm_ba_time_kernels(vmm_ba_handle h, const vmm_ba_options* opt, int reps, vmm_ba_kernel_times* out);

#ifdef __cplusplus
}
#endif
#endif
