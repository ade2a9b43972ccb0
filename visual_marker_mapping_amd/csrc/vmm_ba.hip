// libvmm_ba.so -- C-ABI (include/vmm_ba.h) and host driver of the device-resident LM loop.
//
// Replaces the body of TagReconstructor::doBundleAdjustment
// (/root/reference/src/TagReconstructor.cpp:646-743): vmm_ba_create() takes the place of the
// ceres::Problem construction (:657-724), vmm_ba_solve() of ceres::Solve (:737-738).  No CPU
// fallback exists: without a HIP device every entry point fails with VMM_BA_ERR_HIP.
//
// This file: the error text, the handle (create, destroy, collectives, state), the LM iteration with its graphs,
// vmm_ba_solve and the evaluation entries.  The other entry families have host files of their own -- covariance.hip,
// selfcal.hip, initialize.hip, standalone.hip, diagnostics.hip, localize.hip, calibrate.hip -- and take what they
// need from here through host.hpp.
#include <dlfcn.h>
#include <math.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl.so is resolved with dlopen when a communicator is asked for
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <functional>
#include <vector>

#include "host.hpp"

namespace vmm {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }

template <typename T>
static int upload(Engine& e, T* dst, const std::vector<T>& src)
{
    if (!src.empty())
        HIP_TRY(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, e.stream));
    return VMM_BA_OK;
}

// ---- optional libraries, resolved at run time (libvmm_ba.so itself links only the HIP runtime) ----
// roctx ranges around the solve and its iterations (rocprofv3 --marker-trace / the reference prints
// summary.FullReport(), src/TagReconstructor.cpp:741-742; the numeric phase report is in vmm_ba_summary).
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h)
            h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        }
    }
};
static Roctx& roctx()
{
    static Roctx r;
    return r;
}
Range::Range(const char* name)
{
    if (roctx().push)
        roctx().push(name);
}
Range::~Range()
{
    if (roctx().pop)
        roctx().pop();
}

// RCCL (north_star: "RCCL all-reduce over xGMI of the reduced camera system")
struct Rccl {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
    Rccl()
    {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h)
            h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h)
            h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h)
            return;
        GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
        CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(h, "ncclCommInitRank"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(h, "ncclAllReduce"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        ok = GetUniqueId && CommInitRank && AllReduce && CommDestroy && GetErrorString;
    }
};
static Rccl& rccl()
{
    static Rccl r;
    return r;
}

// ---- uploads of the host plan (plan.hpp) ----

static int upload_order(Engine& e, ObsOrder& o, const OrderPlan& p)
{
    o.n = p.n;
    o.n_pad = p.n_pad;
    o.n_tasks = (int32_t)p.tasks.size();
    int rc;
    if ((rc = dev_alloc(e, &o.own, (size_t)p.n))) return rc;
    if ((rc = dev_alloc(e, &o.other, (size_t)p.n))) return rc;
    if ((rc = dev_alloc(e, &o.caller, (size_t)p.n))) return rc;
    if ((rc = dev_alloc(e, &o.px, (size_t)8 * p.n_pad))) return rc;
    if ((rc = dev_alloc(e, &o.tasks, p.tasks.size()))) return rc;
    if ((rc = dev_alloc(e, &o.pose_task, p.pose_task.size()))) return rc;
    if ((rc = dev_alloc(e, &o.part, p.tasks.size() * kPart))) return rc;
    if ((rc = dev_alloc(e, &o.start, p.start.size()))) return rc;
    if ((rc = upload(e, o.start, p.start))) return rc;
    if ((rc = upload(e, o.own, p.own))) return rc;
    if ((rc = upload(e, o.other, p.other))) return rc;
    if ((rc = upload(e, o.caller, p.caller))) return rc;
    if ((rc = upload(e, o.px, p.px))) return rc;
    if ((rc = upload(e, o.tasks, p.tasks))) return rc;
    if ((rc = upload(e, o.pose_task, p.pose_task))) return rc;
    return VMM_BA_OK;
}

// The rank-k schedule of plan_syrk on the device: a fresh plan every time, and one partial tile per segment.
int make_syrk_plan(Engine& e, SyrkPlan& p, int n_row_blk, int n_col_blk, int k_pad)
{
    const SyrkSchedule s = plan_syrk(n_row_blk, n_col_blk, k_pad, e.n_cu, e.sw);
    p = SyrkPlan();
    p.n_tiles = s.n_tiles;
    p.n_kt = s.n_kt;
    p.n_wg = s.n_wg;
    p.n_segments = s.n_segments;
    p.wide = s.wide;
    int rc;
    if ((rc = dev_alloc(e, &p.tile_bi, s.tile_bi.size()))) return rc;
    if ((rc = dev_alloc(e, &p.tile_bj, s.tile_bj.size()))) return rc;
    if ((rc = dev_alloc(e, &p.wg_u0, s.wg_u0.size()))) return rc;
    if ((rc = dev_alloc(e, &p.wg_u1, s.wg_u1.size()))) return rc;
    if ((rc = dev_alloc(e, &p.wg_seg0, s.wg_seg0.size()))) return rc;
    if ((rc = dev_alloc(e, &p.tile_seg0, s.tile_seg0.size()))) return rc;
    if ((rc = dev_alloc(e, &p.partials, (size_t)std::max(s.n_segments, 1) * kST * kST, false))) return rc;
    if ((rc = upload(e, p.tile_bi, s.tile_bi))) return rc;
    if ((rc = upload(e, p.tile_bj, s.tile_bj))) return rc;
    if ((rc = upload(e, p.wg_u0, s.wg_u0))) return rc;
    if ((rc = upload(e, p.wg_u1, s.wg_u1))) return rc;
    if ((rc = upload(e, p.wg_seg0, s.wg_seg0))) return rc;
    if ((rc = upload(e, p.tile_seg0, s.tile_seg0))) return rc;
    HIP_TRY(hipStreamSynchronize(e.stream));   // the schedule goes out of scope
    return VMM_BA_OK;
}
// the two alternating transposed-panel buffers of the look-ahead Cholesky; P must be allocated
int setup_lookahead(Engine& e, int n_blk_max, int ld)
{
    (void)n_blk_max;
    for (int i = 0; i < 4; ++i)
        e.P4[i] = e.P + (size_t)i * kNB * ld;
    return VMM_BA_OK;
}

// ---- point landmarks: four world corners -> tag pose (the other way: pairs_from_tags, plan.cpp) ----
// The tag pose of four optimised corners, src/TagReconstructor.cpp:608-639: x along corner 0 -> 1, y along corner
// 0 -> 3, z = x cross y, t = the mean of the corners.  The dead code stores R.col(0) = y, R.col(1) = -x (its comments
// name the corners ul, ur, or, ol: an older corner order); with today's order LL, LR, UR, UL
// (TagReconstructor.h:47-50) the tag frame is (x, y, z), and y is re-orthogonalised (z cross x) so that the matrix is
// a rotation before it becomes the quaternion the current ReconstructedTag stores.
static void points_to_tag(const double* pts, double* qt)
{
    double ex[3], ey[3], ez[3];
    for (int a = 0; a < 3; ++a) {
        ex[a] = pts[3 + a] - pts[a];
        ey[a] = pts[9 + a] - pts[a];
    }
    auto normalise = [](double* v) {
        const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (n > 0.0)
            for (int a = 0; a < 3; ++a)
                v[a] /= n;
    };
    normalise(ex);
    normalise(ey);
    ez[0] = ex[1] * ey[2] - ex[2] * ey[1];
    ez[1] = ex[2] * ey[0] - ex[0] * ey[2];
    ez[2] = ex[0] * ey[1] - ex[1] * ey[0];
    normalise(ez);
    ey[0] = ez[1] * ex[2] - ez[2] * ex[1];
    ey[1] = ez[2] * ex[0] - ez[0] * ex[2];
    ey[2] = ez[0] * ex[1] - ez[1] * ex[0];
    const double m00 = ex[0], m01 = ey[0], m02 = ez[0], m10 = ex[1], m11 = ey[1], m12 = ez[1], m20 = ex[2], m21 = ey[2],
                 m22 = ez[2];
    // Eigen::Quaterniond(Matrix3d)
    double q[4];
    const double tr = m00 + m11 + m22;
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m21 - m12) * t;
        q[2] = (m02 - m20) * t;
        q[3] = (m10 - m01) * t;
    } else {
        const double m[3][3] = { { m00, m01, m02 }, { m10, m11, m12 }, { m20, m21, m22 } };
        int i = 0;
        if (m[1][1] > m[0][0])
            i = 1;
        if (m[2][2] > m[i][i])
            i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[k][j] - m[j][k]) * t;
        q[1 + j] = (m[j][i] + m[i][j]) * t;
        q[1 + k] = (m[k][i] + m[i][k]) * t;
    }
    for (int a = 0; a < 4; ++a)
        qt[a] = q[a];
    for (int a = 0; a < 3; ++a)
        qt[4 + a] = (pts[a] + pts[3 + a] + pts[6 + a] + pts[9 + a]) / 4.0;
}

// Dense Z and the plan of its rank-k update (the default at high visibility; a handle on the block-sparse path
// builds them the first time the covariance report asks for Z as a matrix).
int ensure_dense_schur(Engine& e)
{
    if (e.Z)
        return VMM_BA_OK;
    int rc;
    if ((rc = dev_alloc(e, &e.Z, (size_t)e.k_pad * e.ldz))) return rc;
    // 128-row blocks covering rows 0..n_pad (the last one holds the rhs row) and columns 0..n_pad-1
    return make_syrk_plan(e, e.syrk, (e.n_pad + kST) / kST, (e.n_pad + kST - 1) / kST, e.k_pad);
}

static int do_allreduce(Engine& e, double* buf, size_t count)
{
    if (!e.multi)
        return VMM_BA_OK;
    if (e.rccl_comm) {
        // in place, on the engine's stream: ordered behind the kernels that filled the buffer, capturable
        const ncclResult_t r = rccl().AllReduce(buf, buf, count, ncclDouble, ncclSum,
                                                reinterpret_cast<ncclComm_t>(e.rccl_comm), e.stream);
        if (r != ncclSuccess) {
            set_error(std::string("ncclAllReduce: ") + rccl().GetErrorString(r));
            return VMM_BA_ERR_COLLECTIVE;
        }
        return VMM_BA_OK;
    }
    if (!e.allreduce) {
        set_error("world_size > 1 but no all-reduce callback was set (vmm_ba_set_allreduce)");
        return VMM_BA_ERR_STATE;
    }
    if (e.allreduce(e.allreduce_user, buf, count, (void*)e.stream) != 0) {
        set_error("all-reduce callback failed");
        return VMM_BA_ERR_COLLECTIVE;
    }
    return VMM_BA_OK;
}

// World > 1 with the library's own communicator: the ranks agree (minimum) on a yes/no each of them holds, with an
// eager ncclAllReduce on the engine's stream.  Used where a per-rank decision would make the ranks enqueue different
// sequences of collectives (graph or no graph: ADVICE.md round 2).
static int rccl_agree(Engine& e, bool mine, bool* all)
{
    unsigned* word = e.flags + 260;
    const unsigned v = mine ? 1u : 0u;
    unsigned out = 0;
    HIP_TRY(hipMemcpyAsync(word, &v, sizeof(v), hipMemcpyHostToDevice, e.stream));
    const ncclResult_t r = rccl().AllReduce(word, word, 1, ncclUint32, ncclMin, reinterpret_cast<ncclComm_t>(e.rccl_comm),
                                            e.stream);
    if (r != ncclSuccess) {
        set_error(std::string("ncclAllReduce (agreement): ") + rccl().GetErrorString(r));
        return VMM_BA_ERR_COLLECTIVE;
    }
    HIP_TRY(hipMemcpyAsync(&out, word, sizeof(out), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    *all = out != 0;
    return VMM_BA_OK;
}

static void destroy_engine(Engine* e)
{
    if (!e)
        return;
    (void)hipSetDevice(e->device);
    if (e->stream)
        (void)hipStreamSynchronize(e->stream);
    if (e->iter_graph)
        (void)hipGraphExecDestroy(e->iter_graph);
    for (auto& g : e->iter_graph_seg)
        if (g)
            (void)hipGraphExecDestroy(g);
    if (e->rccl_comm)
        (void)rccl().CommDestroy(reinterpret_cast<ncclComm_t>(e->rccl_comm));
    for (void* p : e->allocs)
        (void)hipFree(p);
    if (e->ctl_host)
        (void)hipHostFree(e->ctl_host);
    if (e->pose_stage)
        (void)hipHostFree(e->pose_stage);
    if (e->init_host)
        (void)hipHostFree(e->init_host);
    if (e->pose_ev)
        (void)hipEventDestroy(e->pose_ev);
    if (e->stream)
        (void)hipStreamDestroy(e->stream);
    delete e;
}

// One LM iteration = four groups of kernels separated (world > 1) by the three sum-all-reduces.
//
// Every iteration evaluates residuals AND Jacobians at the CANDIDATE x + delta of the previous iteration (iteration
// zero: the candidate buffers start as a copy of x).  Its cost is the cost Ceres evaluates at the candidate; when the
// step is accepted its blocks simply become the blocks at the new x (staging copy -> working copy, the other W
// buffer), so an accepted step -- the common case -- costs one evaluation instead of a cost pass plus a Jacobian
// pass, and the accept/reject decision sits directly in front of the next iteration's set-up.  A rejected step
// wastes the Jacobian part of its evaluation (21 us of a 0.5 ms iteration at 500 x 200).
constexpr int kNumSeg = 4;
// redo: the host's recovery of a pass whose one-launch factorisation gave up waiting (LmCtl::sync_timeout): the
// reduced system is rebuilt from Z (the factorisation overwrote it) and factored on the path without
// inter-workgroup waits; the control kernel and the elimination of that pass have run and are not repeated.
static void enqueue_segment(Engine& e, const vmm_ba_options& o, int seg, bool redo = false)
{
    switch (seg) {
    case 0:
        if (!redo)
            launch_eval_passes(e, o.robustify, o.huber_a, true);
        break;
    case 1:
        if (!redo) {
            launch_control(e);
            launch_elim(e);
        }
        launch_syrk_reduced(e);
        launch_pack_lower(e, false);
        break;
    case 2:
        launch_pack_lower(e, true);   // world > 1: unpack + the kept family's diagonal blocks
        launch_cholesky_solve(e, e.S, e.n_pad, e.ldz, e.yf, e.ctl, redo);
        launch_backsub(e);
        break;
    default:
        launch_candidate(e);   // world > 1 only; one GPU forms the candidates in k_backsub
        break;
    }
}

// the all-reduce that follows segment `seg` when world > 1 (none after the last one)
static int allreduce_after(Engine& e, int seg)
{
    switch (seg) {
    case 0: return do_allreduce(e, e.small_stage, e.small_count + (size_t)e.n_e);   // blocks, gradient, per-pose costs at the candidate
    case 1: return do_allreduce(e, e.S_packed, (size_t)(e.n_pad + 1) * (e.n_pad + 2) / 2);
    case 2: return do_allreduce(e, e.step_comm, 7 * (size_t)e.n_e + 1);   // steps | per-pose cross terms | sync-time-out votes
    default: return VMM_BA_OK;
    }
}

int enqueue_iteration(Engine& e, const vmm_ba_options& o)
{
    static const char* const names[kNumSeg] = { "vmm_ba evaluation at the candidate", "vmm_ba decide + eliminate + rank-k",
                                                "vmm_ba factor + solve + step", "vmm_ba candidate" };
    int rc;
    for (int seg = 0; seg < kNumSeg; ++seg) {
        if (seg == kNumSeg - 1 && !e.multi)
            break;   // one GPU: the candidates are formed by k_backsub
        Range r(names[seg]);
        enqueue_segment(e, o, seg);
        if (e.multi && (rc = allreduce_after(e, seg)))
            return rc;
    }
    HIP_TRY(hipGetLastError());
    return VMM_BA_OK;
}

// Records `body` (kernel launches, and ncclAllReduce calls when a communicator is attached) into a hipGraph.
// Nothing may fail silently here: a sticky error from before the capture, or a call that invalidates the capture,
// is reported with the place where it was noticed (`where` is set by the body after every group).
static int capture_graph(Engine& e, hipGraphExec_t* out, const std::function<int(const char**)>& body)
{
    const hipError_t pre = hipGetLastError();
    if (pre != hipSuccess) {
        set_error(std::string("error pending before hipStreamBeginCapture: ") + hipGetErrorString(pre));
        return VMM_BA_ERR_HIP;
    }
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(e.stream, hipStreamCaptureModeThreadLocal));
    const char* where = "start";
    const int rc = body(&where);
    const hipError_t ee = hipStreamEndCapture(e.stream, &g);
    if (rc != VMM_BA_OK) {
        if (g)
            (void)hipGraphDestroy(g);
        return rc;
    }
    if (ee != hipSuccess || !g) {
        set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ee) + " (capture invalidated at or before: " + where
                  + ")");
        (void)hipGetLastError();
        return VMM_BA_ERR_HIP;
    }
    const hipError_t ei = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
        *out = nullptr;
        set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
        return VMM_BA_ERR_HIP;
    }
    return VMM_BA_OK;
}

// after a group of launches under capture: is the capture still alive?
static bool capture_alive(Engine& e)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(e.stream, &st) != hipSuccess)
        return false;
    return st == hipStreamCaptureStatusActive;
}

void drop_graphs(Engine& e)
{
    for (auto& g : e.iter_graph_seg)
        if (g) {
            (void)hipGraphExecDestroy(g);
            g = nullptr;
        }
    if (e.iter_graph) {
        (void)hipGraphExecDestroy(e.iter_graph);
        e.iter_graph = nullptr;
    }
}

static const char* const kSegName[kNumSeg] = { "evaluation at the candidate", "decide + control + eliminate + rank-k update",
                                               "factor + solve + back-substitution", "candidate" };

// The iteration is captured once into hipGraphs and replayed (eager enqueueing is host-bound).
//   one GPU:                      one graph;
//   world > 1, RCCL communicator: one graph, the three ncclAllReduce calls recorded between the kernel groups
//                                 (VMM_BA_RCCL_GRAPH=0: four graphs with the collectives enqueued between them);
//   world > 1, host callback:     the callbacks are host calls, so the four kernel groups around them are four graphs.
// No kernel is launched for the first time under capture: vmm_ba_create touches every kernel (preload_*_kernels).
// Round 1 ran the first iteration of a handle eagerly because of an intermittent "operation failed due to a previous
// error during capture" at 2000 x 1000; VMM_BA_EAGER_FIRST=1 brings that back.
int run_iteration(Engine& e, const vmm_ba_options& o)
{
    e.last_passes = 1;
    if (!e.sw.use_graph)
        return enqueue_iteration(e, o);
    if (e.sw.eager_first && !e.launched_eagerly) {
        e.launched_eagerly = true;
        return enqueue_iteration(e, o);
    }
    const bool one_graph = !e.multi || (e.rccl_comm && e.rccl_graph);
    const bool have = one_graph ? e.iter_graph != nullptr : e.iter_graph_seg[0] != nullptr;
    if (!have || e.graph_robustify != o.robustify || e.graph_huber_a != o.huber_a) {
        drop_graphs(e);
        int rc;
        if (one_graph) {
            // graph_passes passes in one graph: nothing separates two passes inside a graph (~9 us between two graph
            // launches); the passes behind the terminating one find `done` set and return at once
            rc = capture_graph(e, &e.iter_graph, [&](const char** where) -> int {
                for (int pass = 0; pass < e.sw.graph_passes; ++pass)
                    for (int seg = 0; seg < kNumSeg; ++seg) {
                        enqueue_segment(e, o, seg);
                        int r;
                        if (e.multi && (r = allreduce_after(e, seg)))
                            return r;
                        if (capture_alive(e))
                            *where = kSegName[seg];
                    }
                return VMM_BA_OK;
            });
            if (e.multi && e.rccl_comm) {
                // Graph or eagerly enqueued collectives is ONE decision for all ranks: a rank that fell back on its own
                // would enqueue one pass per launch while the others enqueue graph_passes, and the surplus
                // ncclAllReduce calls of one side would never complete.  So the ranks agree on "everybody captured".
                bool all_ok = false;
                const std::string why = rc ? g_err : std::string();
                // VMM_BA_DEBUG_CAPTURE_FAIL=<rank>: that rank votes "my capture failed" although it did not -- the path of a
                // rank whose RCCL refuses the capture, without such an RCCL (tests/test_gpu_distributed.py)
                const bool mine = rc == VMM_BA_OK && e.sw.capture_fail_rank != e.rank;
                int arc;
                if ((arc = rccl_agree(e, mine, &all_ok)))
                    return arc;
                if (!all_ok) {
                    // a collective that cannot be recorded (here or on another rank): graphs around eagerly
                    // enqueued collectives, on every rank
                    drop_graphs(e);
                    e.rccl_graph = false;
                    if (e.sw.debug)
                        fprintf(stderr, "[vmm_ba debug] rank %d: RCCL not recorded into the iteration graph (%s)\n", e.rank,
                                rc ? why.c_str() : "another rank could not");
                    return run_iteration(e, o);
                }
            }
            if (rc)
                return rc;
        } else {
            for (int seg = 0; seg < kNumSeg; ++seg)
                if ((rc = capture_graph(e, &e.iter_graph_seg[seg], [&](const char** where) -> int {
                         enqueue_segment(e, o, seg);
                         if (capture_alive(e))
                             *where = kSegName[seg];
                         return VMM_BA_OK;
                     }))) {
                    drop_graphs(e);
                    return rc;
                }
        }
        e.graph_robustify = o.robustify;
        e.graph_huber_a = o.huber_a;
    }
    Range r("vmm_ba lm_iteration");
    if (one_graph) {
        HIP_TRY(hipGraphLaunch(e.iter_graph, e.stream));
        e.last_passes = e.sw.graph_passes;
        return VMM_BA_OK;
    }
    int rc;
    for (int seg = 0; seg < kNumSeg; ++seg) {
        HIP_TRY(hipGraphLaunch(e.iter_graph_seg[seg], e.stream));
        if ((rc = allreduce_after(e, seg)))
            return rc;
    }
    return VMM_BA_OK;
}

// The control block (already read back into e.ctl_host) says done == 2: a workgroup of k_chol_dataflow or
// k_backsolve_chain gave up waiting for another one in the pass that paused.  That is a scheduling event (several
// processes time-slicing one GPU, a profiler serialising workgroups), not a property of the matrix: the pass is
// completed here on the launch-per-block-column factorisation and the per-block back-substitution, which wait for
// nothing inside a launch, and the loop resumes -- the trust-region policy never learns of it.  Every kernel that
// was enqueued behind the give-up has returned at once (done != 0).  World > 1: all ranks pause in the same pass
// (the votes ride on the step all-reduce, k_candidate) and make the same collective calls here.
static int recover_sync_timeout(Engine& e, const vmm_ba_options& o)
{
    LmCtl& c = *e.ctl_host;
    c.num_sync_timeouts++;
    c.sync_kernels |= c.sync_timeout;
    c.sync_timeout = 0;
    c.lin_fail = 0;
    c.done = 0;
    if (e.sw.spin_once)
        c.spin_limit_df = c.spin_limit_chain = 0;
    HIP_TRY(hipMemcpyAsync(e.ctl, e.ctl_host, sizeof(LmCtl), hipMemcpyHostToDevice, e.stream));
    Range r("vmm_ba sync time-out recovery");
    int rc;
    for (int seg = 1; seg < kNumSeg; ++seg) {
        if (seg == kNumSeg - 1 && !e.multi)
            break;
        enqueue_segment(e, o, seg, true);
        if (e.multi && (rc = allreduce_after(e, seg)))
            return rc;
    }
    HIP_TRY(hipGetLastError());
    return VMM_BA_OK;
}

// Control block and candidate buffers at the start of an LM loop: iteration zero evaluates "the candidate" = x.
int begin_lm_loop(Engine& e, const vmm_ba_options& o, int trace_capacity)
{
    init_ctl(e, *e.ctl_host, o, trace_capacity);
    launch_begin_loop(e, *e.ctl_host);   // control block, staged poses -> state, state -> candidate: one launch
    HIP_TRY(hipGetLastError());
    if (e.dirty_cam || e.dirty_tag) {
        HIP_TRY(hipEventRecord(e.pose_ev, e.stream));   // the staging buffer is read by that launch
        e.pose_ev_pending = true;
        e.dirty_cam = e.dirty_tag = false;
    }
    return VMM_BA_OK;
}

// Poses staged by vmm_ba_set_state go to the device (every entry point that reads them there calls this first;
// vmm_ba_solve does it inside k_begin_loop).
int flush_state(Engine& e)
{
    if (!e.dirty_cam && !e.dirty_tag)
        return VMM_BA_OK;
    if (e.dirty_cam)
        HIP_TRY(hipMemcpyAsync(e.cam_qt, e.pose_stage, sizeof(double) * 7 * e.n_cams, hipMemcpyHostToDevice, e.stream));
    if (e.dirty_tag)
        HIP_TRY(hipMemcpyAsync(e.tag_qt, e.pose_stage + (size_t)7 * e.n_cams, sizeof(double) * 7 * e.n_tags,
                               hipMemcpyHostToDevice, e.stream));
    HIP_TRY(hipEventRecord(e.pose_ev, e.stream));
    e.pose_ev_pending = true;
    e.dirty_cam = e.dirty_tag = false;
    return VMM_BA_OK;
}

void init_ctl(Engine& e, LmCtl& c, const vmm_ba_options& o, int trace_capacity)
{
    memset(&c, 0, sizeof(c));
    c.spin_limit_df = e.sw.spin_df;
    c.spin_limit_chain = e.sw.spin_chain;
    c.spin_wg = e.sw.spin_wg;
    c.max_num_iterations = o.max_num_iterations;
    c.robustify = o.robustify;
    c.jacobi_scaling = o.jacobi_scaling;
    c.max_invalid = o.max_num_consecutive_invalid_steps;
    c.huber_a = o.huber_a;
    c.function_tolerance = o.function_tolerance;
    c.gradient_tolerance = o.gradient_tolerance;
    c.parameter_tolerance = o.parameter_tolerance;
    c.max_radius = o.max_trust_region_radius;
    c.min_radius = o.min_trust_region_radius;
    c.min_relative_decrease = o.min_relative_decrease;
    c.min_lm_diagonal = o.min_lm_diagonal;
    c.max_lm_diagonal = o.max_lm_diagonal;
    c.radius = o.initial_trust_region_radius;
    c.decrease_factor = 2.0;
    c.first_eval = 1;
    c.termination = VMM_BA_NO_CONVERGENCE;
    c.trace_capacity = trace_capacity;
}

// ---- vmm_ba_create: validate, expand, open the device, read the switches, plan, allocate and upload ----

// Everything that can be checked without a device (the caller's problem, before any point-landmark expansion).
static int validate_problem(const vmm_ba_problem* p, const vmm_ba_create_options& co)
{
    if (p->n_cams <= 0 || p->n_tags <= 0 || p->n_obs < 0 || !p->cam_qt || !p->tag_qt || !p->tag_wh
        || (p->n_obs > 0 && (!p->obs_cam || !p->obs_tag || !p->obs_px))) {
        set_error("problem needs >= 1 camera, >= 1 tag and non-null arrays");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (p->n_obs >= (int64_t)1 << 31) {
        set_error("n_obs must fit in 31 bits");
        return VMM_BA_ERR_ARGUMENT;
    }
    for (int64_t i = 0; i < p->n_obs; ++i)
        if (p->obs_cam[i] < 0 || p->obs_cam[i] >= p->n_cams || p->obs_tag[i] < 0 || p->obs_tag[i] >= p->n_tags) {
            set_error("observation " + std::to_string(i) + " references a camera or tag index out of range");
            return VMM_BA_ERR_ARGUMENT;
        }
    if (p->fixed_tag >= p->n_tags) {
        set_error("fixed_tag out of range");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (co.landmarks != VMM_BA_LANDMARK_TAG_POSES && co.landmarks != VMM_BA_LANDMARK_POINTS) {
        set_error("create_options.landmarks must be VMM_BA_LANDMARK_TAG_POSES or VMM_BA_LANDMARK_POINTS");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (co.landmarks == VMM_BA_LANDMARK_POINTS && co.precision != VMM_BA_PRECISION_F64) {
        set_error("point landmarks run in f64 only");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (co.landmarks == VMM_BA_LANDMARK_POINTS && (p->n_obs >= (int64_t)1 << 30 || p->n_tags >= 1 << 30)) {
        set_error("problem too large for point landmarks");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (co.precision != VMM_BA_PRECISION_F64 && co.precision != VMM_BA_PRECISION_F32_ACCUM) {
        set_error("create_options.precision must be VMM_BA_PRECISION_F64 or VMM_BA_PRECISION_F32_ACCUM");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (co.world_size < 1 || co.rank < 0 || co.rank >= co.world_size) {
        set_error("bad rank / world_size");
        return VMM_BA_ERR_ARGUMENT;
    }
    return VMM_BA_OK;
}

// Stream and compute units of the engine's device, and every kernel touched once per process and device before
// anything is captured.
static int open_device(Engine& e, int device)
{
    e.device = device;
    if (hipSetDevice(e.device) != hipSuccess || hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipSetDevice / hipStreamCreate failed");
        e.stream = nullptr;
        return VMM_BA_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e.device) == hipSuccess && prop.multiProcessorCount > 0)
        e.n_cu = prop.multiProcessorCount;
    static bool preloaded[64] = {};
    if (e.device < 64 && !preloaded[e.device] && !e.sw.no_preload) {
        const int bad = preload_eval_kernels() + preload_schur_kernels() + preload_chol_kernels() + preload_lm_kernels()
            + preload_cov_kernels() + preload_init_kernels() + preload_border_kernels();
        if (bad) {
            set_error("hipFuncGetAttributes failed for " + std::to_string(bad) + " kernels (code object not loadable on this device)");
            return VMM_BA_ERR_HIP;
        }
        preloaded[e.device] = true;
    }
    return VMM_BA_OK;
}

// The plan's sizes and decisions, kept by the engine.
static void take_plan(Engine& e, const Plan& P)
{
    e.n_e = P.n_e;
    e.n_f = P.n_f;
    e.fused_eval = P.fused_eval;
    e.fused_n_e_act = P.fused_n_e_act;
    e.fused_f_pad = P.fused_f_pad;
    e.fused_chunks = P.fused_chunks;
    e.fused_group = P.fused_group;
    e.fused_groups = P.fused_groups;
    e.n_red = P.n_red;
    e.n_pad = P.n_pad;
    e.n_blk = P.n_blk;
    e.ldz = P.ldz;
    e.k_dim = P.k_dim;
    e.k_pad = P.k_pad;
    e.sparse_schur = P.sparse_schur;
    e.co_terms = P.co_terms;
    e.schur_flops = P.schur_flops;
    e.h_row_of = P.h_row_of;
    e.nd_node_first_blk = P.nd_node_first_blk;
    e.explicit_pairs = P.explicit_pairs;
    e.n_row_items = P.n_row_items;
    e.chol_flops = P.chol_flops;
    e.n_df_wg = P.n_df_wg;
    e.df_tree_slots = P.df_tree_slots;
    e.chol_nz_on = !P.chol_nz.empty();
}

// Engine::pose_const from the caller's flags (either may be null) and the problem's fixed tag; point landmarks: a tag
// owns two landmark blocks.  Waits for the copy: the staging vector goes out of scope.
static int upload_pose_const(Engine& e, const uint8_t* cam_const, const uint8_t* tag_const)
{
    std::vector<uint8_t> c((size_t)e.n_cams + (size_t)e.n_tags, 0);
    const int rep = e.points ? 2 : 1;
    if (cam_const)
        for (int i = 0; i < e.n_cams; ++i)
            c[(size_t)i] = cam_const[i] ? 1 : 0;
    for (int t = 0; t < e.n_tags; ++t)
        c[(size_t)e.n_cams + t] = ((tag_const && tag_const[t / rep]) || t / rep == e.fixed_tag) ? 1 : 0;
    if (c.empty())
        return VMM_BA_OK;
    HIP_TRY(hipMemcpyAsync(e.pose_const, c.data(), c.size(), hipMemcpyHostToDevice, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    e.any_const = std::find(c.begin(), c.end(), (uint8_t)1) != c.end();
    return VMM_BA_OK;
}

// Device buffers of the engine, the plan's tables copied into them (the poses from the caller's problem `p`).
static int allocate_and_upload(Engine& e, const Plan& P, const vmm_ba_problem& p)
{
    const int n_pose = e.n_cams + e.n_tags;
    int rc;
    // poses
    if ((rc = dev_alloc(e, &e.cam_qt, (size_t)7 * e.n_cams))) return rc;
    if ((rc = dev_alloc(e, &e.tag_qt, (size_t)7 * e.n_tags))) return rc;
    if ((rc = dev_alloc(e, &e.cam_cand, (size_t)7 * e.n_cams))) return rc;
    if ((rc = dev_alloc(e, &e.tag_cand, (size_t)7 * e.n_tags))) return rc;
    if ((rc = dev_alloc(e, &e.tag_wh, (size_t)2 * e.n_tags))) return rc;
    if (hipMemcpyAsync(e.cam_qt, p.cam_qt, sizeof(double) * 7 * e.n_cams, hipMemcpyHostToDevice, e.stream) != hipSuccess
        || hipMemcpyAsync(e.tag_qt, p.tag_qt, sizeof(double) * 7 * e.n_tags, hipMemcpyHostToDevice, e.stream) != hipSuccess
        || hipMemcpyAsync(e.tag_wh, p.tag_wh, sizeof(double) * 2 * e.n_tags, hipMemcpyHostToDevice, e.stream) != hipSuccess
        || hipStreamSynchronize(e.stream) != hipSuccess) {
        set_error("pose upload failed");
        return VMM_BA_ERR_HIP;
    }
    // observation orders
    if ((rc = upload_order(e, e.ordE, P.ordE))) return rc;
    if ((rc = upload_order(e, e.ordF, P.ordF))) return rc;
    if (e.fused_eval) {
        if ((rc = dev_alloc(e, &e.pair_obs, P.pair_obs.size()))) return rc;
        if ((rc = dev_alloc(e, &e.fused_e_list, P.fused_e_list.size()))) return rc;
        if ((rc = dev_alloc(e, &e.fused_e_part0, P.fused_e_part0.size()))) return rc;
        if ((rc = dev_alloc(e, &e.fused_pose_task, P.fused_pose_task.size()))) return rc;
        if ((rc = dev_alloc(e, &e.fused_partE, (size_t)std::max(P.fused_slots, 1) * kPart))) return rc;
        if ((rc = dev_alloc(e, &e.fused_partF, (size_t)e.fused_groups * 28 * e.fused_f_pad))) return rc;
        if ((rc = upload(e, e.pair_obs, P.pair_obs))) return rc;
        if ((rc = upload(e, e.fused_e_list, P.fused_e_list))) return rc;
        if ((rc = upload(e, e.fused_e_part0, P.fused_e_part0))) return rc;
        if ((rc = upload(e, e.fused_pose_task, P.fused_pose_task))) return rc;
    }

    // normal-equation blocks
    e.small_count = (size_t)42 * n_pose + 2;
    if ((rc = dev_alloc(e, &e.small, e.small_count))) return rc;
    e.H_cam = e.small;
    e.H_tag = e.H_cam + (size_t)36 * e.n_cams;
    e.g_cam = e.H_tag + (size_t)36 * e.n_tags;
    e.g_tag = e.g_cam + (size_t)6 * e.n_cams;
    e.cost_slot = e.g_tag + (size_t)6 * e.n_tags;
    // the LM loop evaluates at the candidate into this staging copy (all-reduced when world > 1); it replaces the
    // working copy when the step is accepted
    // (+ n_e per-pose costs of the eliminated family behind it: world > 1 sums them over the ranks with the blocks)
    if ((rc = dev_alloc(e, &e.small_stage, e.small_count + (size_t)e.n_e))) return rc;
    e.ev_pose_cost = e.small_stage + e.small_count;
    e.small_alt_off = e.multi ? 0 : (int64_t)(e.small_stage - e.small);
    e.ev_H_cam = e.small_stage;
    e.ev_H_tag = e.ev_H_cam + (size_t)36 * e.n_cams;
    e.ev_g_cam = e.ev_H_tag + (size_t)36 * e.n_tags;
    e.ev_g_tag = e.ev_g_cam + (size_t)6 * e.n_cams;
    e.ev_cost = e.ev_g_tag + (size_t)6 * e.n_tags;
    if ((rc = dev_alloc(e, &e.obs_mask, (size_t)std::max<int64_t>(e.n_obs, 1), false))) return rc;
    if (hipMemsetAsync(e.obs_mask, 1, (size_t)std::max<int64_t>(e.n_obs, 1), e.stream) != hipSuccess) {
        set_error("hipMemsetAsync(obs_mask) failed");
        return VMM_BA_ERR_HIP;
    }
    if ((rc = dev_alloc(e, &e.pose_const, (size_t)n_pose))) return rc;
    if ((rc = upload_pose_const(e, nullptr, nullptr))) return rc;
    const size_t n_stat = (size_t)e.ordE.n_tasks + (size_t)e.ordF.n_tasks + 1;
    if ((rc = dev_alloc(e, &e.stats_part, n_stat))) return rc;
    if ((rc = dev_alloc(e, &e.stats_cnt, n_stat))) return rc;
    if ((rc = dev_alloc(e, &e.stats_pose, (size_t)2 * n_pose))) return rc;
    if (e.f32_accum) {
        if ((rc = dev_alloc(e, &e.Wf, (size_t)36 * e.ordE.n_pad))) return rc;
        if ((rc = dev_alloc(e, &e.Wf2, (size_t)36 * e.ordE.n_pad))) return rc;
    } else {
        if ((rc = dev_alloc(e, &e.W, (size_t)36 * e.ordE.n_pad))) return rc;
        if ((rc = dev_alloc(e, &e.W2, (size_t)36 * e.ordE.n_pad))) return rc;
    }
    if ((rc = dev_alloc(e, &e.scale, (size_t)6 * n_pose))) return rc;
    if ((rc = dev_alloc(e, &e.diag, (size_t)6 * n_pose))) return rc;
    if ((rc = dev_alloc(e, &e.D2, (size_t)6 * n_pose))) return rc;
    if ((rc = dev_alloc(e, &e.delta, (size_t)6 * n_pose))) return rc;
    if ((rc = dev_alloc(e, &e.active, (size_t)n_pose))) return rc;

    // elimination: block-sparse (the plan's pair lists, and the tree-ordered factor's structure) or dense Z
    if ((rc = dev_alloc(e, &e.Le, (size_t)36 * e.n_e))) return rc;
    if ((rc = dev_alloc(e, &e.ze, (size_t)6 * e.n_e))) return rc;
    if (e.sparse_schur) {
        if ((rc = dev_alloc(e, &e.Zc, (size_t)36 * std::max<int64_t>(e.n_obs, 1)))) return rc;
        if ((rc = dev_alloc(e, &e.f2e, P.f2e.size()))) return rc;
        if ((rc = dev_alloc(e, &e.pair_start, P.pair_start.size()))) return rc;
        if ((rc = dev_alloc(e, &e.pair_tstart, P.pair_tstart.size()))) return rc;
        if ((rc = dev_alloc(e, &e.pair_terms, P.pair_terms.size()))) return rc;
        if ((rc = dev_alloc(e, &e.row_items, P.row_items.size()))) return rc;
        if ((rc = upload(e, e.f2e, P.f2e))) return rc;
        if ((rc = upload(e, e.pair_start, P.pair_start))) return rc;
        if ((rc = upload(e, e.pair_tstart, P.pair_tstart))) return rc;
        if ((rc = upload(e, e.pair_terms, P.pair_terms))) return rc;
        if ((rc = upload(e, e.row_items, P.row_items))) return rc;
        if (e.chol_nz_on) {
            if ((rc = dev_alloc(e, &e.chol_nz, P.chol_nz.size()))) return rc;
            if ((rc = upload(e, e.chol_nz, P.chol_nz))) return rc;
            if ((rc = dev_alloc(e, &e.chol_order, P.chol_order.size()))) return rc;
            if ((rc = upload(e, e.chol_order, P.chol_order))) return rc;
            if ((rc = dev_alloc(e, &e.df_wg, P.df_wg.size()))) return rc;
            if ((rc = upload(e, e.df_wg, P.df_wg))) return rc;
            if ((rc = dev_alloc(e, &e.df_slot, P.df_slot.size()))) return rc;
            if ((rc = upload(e, e.df_slot, P.df_slot))) return rc;
        }
        if (e.explicit_pairs) {
            if ((rc = dev_alloc(e, &e.pair_col, P.pair_col.size()))) return rc;
            if ((rc = dev_alloc(e, &e.row_of, P.row_of.size()))) return rc;
            if ((rc = upload(e, e.pair_col, P.pair_col))) return rc;
            if ((rc = upload(e, e.row_of, P.row_of))) return rc;
            if (!P.pose_of_row.empty()) {
                if ((rc = dev_alloc(e, &e.pose_of_row, P.pose_of_row.size()))) return rc;
                if ((rc = upload(e, e.pose_of_row, P.pose_of_row))) return rc;
            }
        }
    } else {
        if ((rc = ensure_dense_schur(e))) return rc;
    }
    if ((rc = dev_alloc(e, &e.S, (size_t)e.ldz * e.ldz))) return rc;
    if (e.multi && (rc = dev_alloc(e, &e.S_packed, (size_t)(e.n_pad + 1) * (e.n_pad + 2) / 2))) return rc;
    if ((rc = dev_alloc(e, &e.P, (size_t)4 * kNB * e.ldz))) return rc;
    if ((rc = setup_lookahead(e, e.n_blk, e.ldz))) return rc;
    if ((rc = dev_alloc(e, &e.dinv, (size_t)e.ldz))) return rc;
    if ((rc = dev_alloc(e, &e.Ldiag, (size_t)(e.n_blk + 1) * 4096))) return rc;
    if ((rc = dev_alloc(e, &e.Linv, (size_t)(e.n_blk + 1) * 4096))) return rc;
    if ((rc = dev_alloc(e, &e.flags, 264))) return rc;
    if ((rc = dev_alloc(e, &e.gran, (size_t)2 * e.ldz))) return rc;
    {
        // published slices of the one-launch factorisation: 64 KB per block below the diagonal (dense: of the block columns
        // that kernel takes; tree ordering: of the non-zero blocks, and of the dense kernel's share when the handle is
        // switched to the natural dense system for a call)
        const size_t nd = e.sw.no_dataflow ? 0 : (size_t)dataflow_blocks(e.n_blk, e.n_cu, e.sw);
        const size_t slots = std::max(nd * (nd + 1) / 2, e.sw.no_dataflow ? (size_t)0 : e.df_tree_slots);
        if (slots > 0 && (rc = dev_alloc(e, &e.df_gran, slots * 8 * 1024)))
            return rc;
        if (slots > 0 && (rc = dev_alloc(e, &e.df_compact, slots * 4096, false)))
            return rc;
        if (slots > 0 && (rc = dev_alloc(e, &e.df_done, slots)))
            return rc;
    }
    if ((rc = dev_alloc(e, &e.yf, (size_t)e.ldz))) return rc;
    if ((rc = dev_alloc(e, &e.step_comm, (size_t)7 * e.n_e + 1))) return rc;
    if ((rc = dev_alloc(e, &e.cost_comm, 2))) return rc;
    const size_t n_part = (size_t)std::max<int>(e.ordE.n_tasks, e.n_e) + 1;
    if ((rc = dev_alloc(e, &e.part_cost, n_part))) return rc;
    if ((rc = dev_alloc(e, &e.part_cross, n_part))) return rc;
    if ((rc = dev_alloc(e, &e.part_k1, n_part))) return rc;
    if ((rc = dev_alloc(e, &e.pose_part, (size_t)5 * n_pose))) return rc;
    if ((rc = dev_alloc(e, &e.pose_gm, (size_t)n_pose))) return rc;
    if ((rc = dev_alloc(e, &e.ctl, 1))) return rc;
    if (hipHostMalloc((void**)&e.ctl_host, sizeof(LmCtl)) != hipSuccess) {
        set_error("hipHostMalloc failed");
        e.ctl_host = nullptr;
        return VMM_BA_ERR_HIP;
    }
    memset(e.ctl_host, 0, sizeof(LmCtl));
    if (hipHostMalloc((void**)&e.pose_stage, sizeof(double) * 7 * (size_t)n_pose, hipHostMallocMapped) != hipSuccess
        || hipHostGetDevicePointer((void**)&e.pose_stage_dev, e.pose_stage, 0) != hipSuccess
        || hipEventCreateWithFlags(&e.pose_ev, hipEventDisableTiming) != hipSuccess) {
        set_error("hipHostMalloc / hipEventCreate (pose staging) failed");
        return VMM_BA_ERR_HIP;
    }
    e.trace_capacity = 0;
    if (hipStreamSynchronize(e.stream) != hipSuccess) {   // the plan's vectors go out of scope
        set_error("create: device synchronisation failed");
        return VMM_BA_ERR_HIP;
    }
    return VMM_BA_OK;
}
} // namespace vmm

using namespace vmm;

extern "C" {

const char* vmm_ba_last_error(void) { return g_err.c_str(); }
int vmm_ba_abi_version(void) { return VMM_BA_ABI_VERSION; }

void vmm_ba_default_options(vmm_ba_options* o)
{
    // src/TagReconstructor.cpp:725-735 + Ceres Solver::Options defaults
    memset(o, 0, sizeof(*o));
    o->max_num_iterations = 400;
    o->robustify = 1;
    o->huber_a = 1.0;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->max_num_consecutive_invalid_steps = 5;
    o->jacobi_scaling = 1;
    o->num_threads = 1;
    o->poll_interval = 1;
}

void vmm_ba_default_create_options(vmm_ba_create_options* o)
{
    memset(o, 0, sizeof(*o));
    o->device = 0;
    o->elimination = VMM_BA_ELIM_AUTO;
    o->rank = 0;
    o->world_size = 1;
}

int vmm_ba_create(const vmm_ba_problem* p, const vmm_ba_create_options* copt, vmm_ba_handle* out)
{
    if (!p || !out) {
        set_error("null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    *out = nullptr;
    vmm_ba_create_options co;
    if (copt)
        co = *copt;
    else
        vmm_ba_default_create_options(&co);
    int rc;
    if ((rc = validate_problem(p, co)))
        return rc;
    // Point landmarks (expand_points): from here on `p` is the expanded problem, `user` the caller's.
    const vmm_ba_problem* const user = p;
    PointProblem expanded;
    if (co.landmarks == VMM_BA_LANDMARK_POINTS) {
        expand_points(*user, expanded);
        p = &expanded.problem;
    }
    int elim = co.elimination;
    if (elim == VMM_BA_ELIM_AUTO)
        elim = (p->n_cams >= p->n_tags) ? VMM_BA_ELIM_CAMERAS : VMM_BA_ELIM_TAGS;
    if (elim != VMM_BA_ELIM_CAMERAS && elim != VMM_BA_ELIM_TAGS) {
        set_error("bad elimination mode");
        return VMM_BA_ERR_ARGUMENT;
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libvmm_ba has no CPU fallback");
        return VMM_BA_ERR_HIP;
    }
    if (co.device < 0 || co.device >= ndev) {
        set_error("device ordinal out of range");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine* ep = new Engine();
    Engine& e = *ep;
    auto fail = [&](int code) {
        destroy_engine(ep);
        return code;
    };
    e.sw = read_switches();
    if ((rc = open_device(e, co.device)))
        return fail(rc);
    e.rank = co.rank;
    e.world = co.world_size;
    e.f32_accum = co.precision == VMM_BA_PRECISION_F32_ACCUM;
    e.multi = e.world > 1 || e.sw.force_collectives;   // test hook: one rank, but staging buffers + eager launches + all-reduce callbacks
    e.rccl_graph = e.sw.rccl_graph;
    e.K = make_intrinsics(p->intr, p->dist);
    e.n_cams = p->n_cams;
    e.n_tags = p->n_tags;
    e.fixed_tag = user->fixed_tag;
    e.n_obs = p->n_obs;
    e.points = co.landmarks == VMM_BA_LANDMARK_POINTS;
    e.n_tags_user = user->n_tags;
    e.n_obs_user = user->n_obs;
    if (e.points)
        std::vector<double>(user->tag_wh, user->tag_wh + 2 * (size_t)user->n_tags).swap(e.user_tag_wh);
    e.elim_cams = (elim == VMM_BA_ELIM_CAMERAS);

    const Plan plan = make_plan(*p, co, e.elim_cams, e.multi, e.world, e.points, e.sw);
    if (!plan.error.empty()) {
        set_error(plan.error);
        return fail(VMM_BA_ERR_ARGUMENT);
    }
    take_plan(e, plan);
    if ((rc = allocate_and_upload(e, plan, *p)))
        return fail(rc);
    *out = reinterpret_cast<vmm_ba_handle>(ep);
    return VMM_BA_OK;
}
void vmm_ba_destroy(vmm_ba_handle h) { destroy_engine(reinterpret_cast<Engine*>(h)); }

int vmm_ba_set_allreduce(vmm_ba_handle h, vmm_ba_allreduce_fn fn, void* user)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    e.allreduce = fn;
    e.allreduce_user = user;
    return VMM_BA_OK;
}

int vmm_ba_rccl_available(void) { return rccl().ok ? 1 : 0; }

int vmm_ba_rccl_unique_id(void* id128)
{
    if (!id128) {
        set_error("null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (!rccl().ok) {
        set_error("librccl.so could not be loaded");
        return VMM_BA_ERR_COLLECTIVE;
    }
    static_assert(sizeof(ncclUniqueId) == VMM_BA_RCCL_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    const ncclResult_t r = rccl().GetUniqueId(&id);
    if (r != ncclSuccess) {
        set_error(std::string("ncclGetUniqueId: ") + rccl().GetErrorString(r));
        return VMM_BA_ERR_COLLECTIVE;
    }
    memcpy(id128, &id, sizeof(id));
    return VMM_BA_OK;
}

int vmm_ba_enable_rccl(vmm_ba_handle h, const void* id128)
{
    if (!h || !id128) {
        set_error("null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!e.multi) {
        set_error("vmm_ba_enable_rccl: the handle was created with world_size 1");
        return VMM_BA_ERR_STATE;
    }
    if (!rccl().ok) {
        set_error("librccl.so could not be loaded");
        return VMM_BA_ERR_COLLECTIVE;
    }
    HIP_TRY(hipSetDevice(e.device));
    if (e.rccl_comm) {
        (void)rccl().CommDestroy(reinterpret_cast<ncclComm_t>(e.rccl_comm));
        e.rccl_comm = nullptr;
    }
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = rccl().CommInitRank(&comm, e.world, id, e.rank);
    if (r != ncclSuccess) {
        set_error(std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
        return VMM_BA_ERR_COLLECTIVE;
    }
    e.rccl_comm = comm;
    drop_graphs(e);
    return VMM_BA_OK;
}

int vmm_ba_set_state(vmm_ba_handle h, const double* cam_qt, const double* tag_qt)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    HIP_TRY(hipSetDevice(e.device));
    std::vector<double> pairs;
    if (tag_qt && e.points) {   // tag poses -> their corners, as at create
        pairs = pairs_from_tags(tag_qt, e.user_tag_wh.data(), e.n_tags_user);
        tag_qt = pairs.data();
    }
    // Staged in pinned memory only: the next call that needs the poses on the device uploads them (vmm_ba_solve inside
    // the launch that starts its loop), so the call costs a 39 KB memcpy on the host and no device command.
    if (e.pose_ev_pending) {
        HIP_TRY(hipEventSynchronize(e.pose_ev));   // an earlier upload has left the staging buffer
        e.pose_ev_pending = false;
    }
    if (cam_qt) {
        memcpy(e.pose_stage, cam_qt, sizeof(double) * 7 * e.n_cams);
        e.dirty_cam = true;
    }
    if (tag_qt) {
        memcpy(e.pose_stage + (size_t)7 * e.n_cams, tag_qt, sizeof(double) * 7 * e.n_tags);
        e.dirty_tag = true;
    }
    return VMM_BA_OK;
}

int vmm_ba_get_points(vmm_ba_handle h, double* points)
{
    if (!h || !points) {
        set_error("null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!e.points) {
        set_error("vmm_ba_get_points: the handle was not created with VMM_BA_LANDMARK_POINTS");
        return VMM_BA_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    std::vector<double> pairs((size_t)7 * e.n_tags);
    HIP_TRY(hipMemcpyAsync(pairs.data(), e.tag_qt, sizeof(double) * pairs.size(), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    for (int t = 0; t < e.n_tags_user; ++t)
        for (int k = 0; k < 6; ++k) {
            points[(size_t)12 * t + k] = pairs[(size_t)14 * t + k];
            points[(size_t)12 * t + 6 + k] = pairs[(size_t)14 * t + 7 + k];
        }
    return VMM_BA_OK;
}

int vmm_ba_get_state(vmm_ba_handle h, double* cam_qt, double* tag_qt)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    if (cam_qt)
        HIP_TRY(hipMemcpyAsync(cam_qt, e.cam_qt, sizeof(double) * 7 * e.n_cams, hipMemcpyDeviceToHost, e.stream));
    if (tag_qt && e.points) {   // tag poses rebuilt from the optimised corners (src/TagReconstructor.cpp:608-639)
        std::vector<double> pts((size_t)12 * e.n_tags_user);
        HIP_TRY(hipStreamSynchronize(e.stream));
        if ((rc = vmm_ba_get_points(h, pts.data()))) return rc;
        for (int t = 0; t < e.n_tags_user; ++t)
            points_to_tag(pts.data() + (size_t)12 * t, tag_qt + (size_t)7 * t);
        return VMM_BA_OK;
    }
    if (tag_qt)
        HIP_TRY(hipMemcpyAsync(tag_qt, e.tag_qt, sizeof(double) * 7 * e.n_tags, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    return VMM_BA_OK;
}

int vmm_ba_solve(vmm_ba_handle h, const vmm_ba_options* opt, vmm_ba_summary* s)
{
    if (!h || !s) {
        set_error("null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    vmm_ba_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_options(&o);
    if (o.max_num_iterations < 0 || o.poll_interval < 0 || !(o.initial_trust_region_radius > 0.0)) {
        set_error("bad solver options");
        return VMM_BA_ERR_ARGUMENT;
    }
    HIP_TRY(hipSetDevice(e.device));
    Range solve_range("vmm_ba_solve");
    const auto t0 = std::chrono::steady_clock::now();
    vmm_ba_iteration* user_trace = s->trace;
    const int user_cap = s->trace ? s->trace_capacity : 0;
    memset(s, 0, sizeof(*s));
    s->trace = user_trace;
    s->trace_capacity = user_cap;

    // device trace buffer sized for this call
    const int need_cap = std::max(user_cap, 1);
    int rc;
    if (need_cap > e.trace_capacity) {
        drop_graphs(e);   // the captured k_control holds the old trace pointer
        if (e.trace) {
            HIP_TRY(hipStreamSynchronize(e.stream));
            e.allocs.erase(std::remove(e.allocs.begin(), e.allocs.end(), (void*)e.trace), e.allocs.end());
            (void)hipFree(e.trace);
            e.trace = nullptr;
            e.trace_capacity = 0;
        }
        if ((rc = dev_alloc(e, &e.trace, (size_t)need_cap, false))) return rc;
        e.trace_capacity = need_cap;
    }
    if ((rc = begin_lm_loop(e, o, user_cap))) return rc;

    const int poll = std::max(1, o.poll_interval);
    const int64_t max_steps = (int64_t)o.max_num_iterations + 2;
    int64_t enq = 0;
    for (;;) {
        for (int k = 0; k < poll && enq < max_steps; ++k) {
            if ((rc = run_iteration(e, o))) return rc;
            enq += e.last_passes;
        }
        HIP_TRY(hipMemcpyAsync(e.ctl_host, e.ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, e.stream));
        HIP_TRY(hipStreamSynchronize(e.stream));
        if (e.ctl_host->done == 2) {
            // a spin give-up, not a numerical failure: finish that pass on the fallback path and go on
            if (e.ctl_host->num_sync_timeouts >= 1000) {
                set_error("the one-launch factorisation gave up waiting in 1000 passes of one solve (kernels: "
                          + std::to_string(e.ctl_host->sync_kernels | e.ctl_host->sync_timeout) + ")");
                return VMM_BA_ERR_HIP;
            }
            if ((rc = recover_sync_timeout(e, o))) return rc;
            enq = e.ctl_host->num_lm_iterations;   // the passes enqueued behind the paused one did nothing
            continue;
        }
        if (e.ctl_host->done)
            break;
        if (enq >= max_steps) {
            set_error("LM loop did not terminate within max_num_iterations + 2 passes");
            return VMM_BA_ERR_STATE;
        }
    }
    const LmCtl& c = *e.ctl_host;
    s->termination_type = c.termination;
    s->iterations = c.records;
    s->num_successful_steps = c.num_successful;
    s->num_unsuccessful_steps = c.num_unsuccessful;
    s->num_lm_iterations = c.num_lm_iterations;
    s->num_jacobian_evals = c.num_jac_evals;
    s->num_cost_evals = c.num_cost_evals;
    s->elimination = e.elim_cams ? VMM_BA_ELIM_CAMERAS : VMM_BA_ELIM_TAGS;
    s->initial_cost = c.initial_cost;
    s->final_cost = c.x_cost;
    s->time_eval_s = 1e-8 * (double)c.phase_ticks[0];          // 100 MHz ticks
    s->time_control_s = 1e-8 * (double)c.phase_ticks[1];
    s->time_eliminate_s = 1e-8 * (double)c.phase_ticks[2];
    s->time_factor_solve_s = 1e-8 * (double)c.phase_ticks[3];
    s->time_step_s = 1e-8 * (double)c.phase_ticks[4];
    s->num_sync_timeouts = c.num_sync_timeouts;
    s->sync_timeout_kernels = c.sync_kernels;
    s->block_sparse = e.sparse_schur ? 1 : 0;
    s->tree_ordering = (e.sparse_schur && !e.h_row_of.empty()) ? (int32_t)e.nd_node_first_blk.size() : 0;
    if (user_trace && user_cap > 0) {
        const int n = std::min(c.records, user_cap);
        if (n > 0) {
            HIP_TRY(hipMemcpyAsync(user_trace, e.trace, sizeof(vmm_ba_iteration) * n, hipMemcpyDeviceToHost, e.stream));
            HIP_TRY(hipStreamSynchronize(e.stream));
        }
    }
    s->time_solve_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return VMM_BA_OK;
}

int vmm_ba_cost(vmm_ba_handle h, int robustify, double huber_a, double* cost)
{
    if (!h || !cost) {
        set_error("null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    launch_cost(e, e.cam_qt, e.tag_qt, false, robustify, huber_a, e.cost_comm);
    if ((rc = do_allreduce(e, e.cost_comm, 1))) return rc;
    HIP_TRY(hipMemcpyAsync(cost, e.cost_comm, sizeof(double), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    return VMM_BA_OK;
}

int vmm_ba_set_observation_mask(vmm_ba_handle h, const uint8_t* mask)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    HIP_TRY(hipSetDevice(e.device));
    if (e.n_obs == 0)
        return VMM_BA_OK;
    if (mask) {
        std::vector<uint8_t> m((size_t)e.n_obs);
        const int rep = e.points ? 2 : 1;   // a tag observation is two point-pair observations
        for (int64_t i = 0; i < e.n_obs; ++i)
            m[(size_t)i] = mask[i / rep] ? 1 : 0;
        HIP_TRY(hipMemcpyAsync(e.obs_mask, m.data(), m.size(), hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipStreamSynchronize(e.stream));   // the staging vector goes out of scope
    } else {
        HIP_TRY(hipMemsetAsync(e.obs_mask, 1, (size_t)e.n_obs, e.stream));
    }
    return VMM_BA_OK;
}

int vmm_ba_set_constant_poses(vmm_ba_handle h, const uint8_t* cam_const, const uint8_t* tag_const)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    HIP_TRY(hipSetDevice(e.device));
    return upload_pose_const(e, cam_const, tag_const);
}

int vmm_ba_reprojection_stats(vmm_ba_handle h, double* per_cam_mean, double* per_tag_mean, double* avg,
                              double* per_corner)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.points) {
        set_error("reprojection_stats works on tag poses: read them with vmm_ba_get_state and use a tag-pose handle");
        return VMM_BA_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    const int n_pose = e.n_cams + e.n_tags;
    if (per_corner && e.n_obs > 0 && !e.stats_corner && (rc = dev_alloc(e, &e.stats_corner, (size_t)8 * e.n_obs, false)))
        return rc;
    launch_stats(e, (per_corner && e.n_obs > 0) ? e.stats_corner : nullptr);
    HIP_TRY(hipGetLastError());
    // per-pose sums and counts come back in one copy; the means and the average are formed here in the
    // reference's order (per tag, ascending: src/TagReconstructor.cpp:416-426)
    std::vector<double> pose((size_t)2 * n_pose);
    HIP_TRY(hipMemcpyAsync(pose.data(), e.stats_pose, sizeof(double) * pose.size(), hipMemcpyDeviceToHost, e.stream));
    if (per_corner && e.n_obs > 0)
        HIP_TRY(hipMemcpyAsync(per_corner, e.stats_corner, sizeof(double) * 8 * e.n_obs, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    const double* sc = pose.data();
    const double* st = sc + e.n_cams;
    const double* nc = sc + n_pose;
    const double* nt = nc + e.n_cams;
    if (per_cam_mean)
        for (int c = 0; c < e.n_cams; ++c)
            per_cam_mean[c] = nc[c] > 0.0 ? sc[c] / nc[c] : -1.0;   // :371-383
    double a = 0.0, tot = 0.0;
    for (int t = 0; t < e.n_tags; ++t) {
        if (nt[t] > 0.0) {
            a += st[t];
            tot += nt[t];
        }
        if (per_tag_mean)
            per_tag_mean[t] = nt[t] > 0.0 ? st[t] / nt[t] : NAN;
    }
    if (avg)
        *avg = tot > 0.0 ? a / tot : 0.0;                            // :416-426
    return VMM_BA_OK;
}

int vmm_ba_eval_blocks(vmm_ba_handle h, int robustify, double huber_a, double* cost, double* V, double* U,
                       double* W, double* g_cam, double* g_tag)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.points && (U || W || g_tag)) {
        set_error("eval_blocks: with point landmarks only cost, V and g_cam are in the caller's index space");
        return VMM_BA_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    launch_eval_passes(e, robustify, huber_a, false);
    HIP_TRY(hipGetLastError());
    if (cost) HIP_TRY(hipMemcpyAsync(cost, e.cost_slot, sizeof(double), hipMemcpyDeviceToHost, e.stream));
    if (V) HIP_TRY(hipMemcpyAsync(V, e.H_cam, sizeof(double) * 36 * e.n_cams, hipMemcpyDeviceToHost, e.stream));
    if (U) HIP_TRY(hipMemcpyAsync(U, e.H_tag, sizeof(double) * 36 * e.n_tags, hipMemcpyDeviceToHost, e.stream));
    if (g_cam) HIP_TRY(hipMemcpyAsync(g_cam, e.g_cam, sizeof(double) * 6 * e.n_cams, hipMemcpyDeviceToHost, e.stream));
    if (g_tag) HIP_TRY(hipMemcpyAsync(g_tag, e.g_tag, sizeof(double) * 6 * e.n_tags, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    if (W && e.n_obs > 0) {
        std::vector<double> w((size_t)36 * e.ordE.n_pad);
        std::vector<int32_t> caller((size_t)e.n_obs);
        if (e.f32_accum) {
            std::vector<float> wf(w.size());
            HIP_TRY(hipMemcpy(wf.data(), e.Wf, sizeof(float) * wf.size(), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < w.size(); ++q)
                w[q] = (double)wf[q];
        } else {
            HIP_TRY(hipMemcpy(w.data(), e.W, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
        }
        HIP_TRY(hipMemcpy(caller.data(), e.ordE.caller, sizeof(int32_t) * caller.size(), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < e.n_obs; ++i)
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) {
                    // device: rows = eliminated family's tangent, columns = kept family's
                    const double v = w[(size_t)(6 * a + b) * e.ordE.n_pad + i];
                    const int ca = e.elim_cams ? a : b, tb = e.elim_cams ? b : a;
                    W[(size_t)36 * caller[i] + 6 * ca + tb] = v;
                }
    }
    return VMM_BA_OK;
}

} // extern "C"
