// What the host files of libvmm_ba.so share (vmm_ba.hip, covariance.hip, selfcal.hip, initialize.hip, standalone.hip,
// diagnostics.hip, localize.hip, rig.hip, calibrate.hip, triangulate.hip, locate.hip).  No kernel; no kernels_*.hip includes this.
#pragma once

#include <algorithm>
#include <initializer_list>
#include <string>

#include <math.h>
#include <string.h>

#include "engine.hpp"
#include "pose_lm.hpp"

namespace vmm {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                         \
            return VMM_BA_ERR_HIP;                                                                 \
        }                                                                                          \
    } while (0)

template <typename T>
int dev_alloc(Engine& e, T** p, size_t count, bool zero = true)
{
    *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    HIP_TRY(hipMalloc((void**)p, bytes));
    e.allocs.push_back(*p);
    if (zero)
        HIP_TRY(hipMemsetAsync(*p, 0, bytes, e.stream));
    return VMM_BA_OK;
}

// ---- vmm_ba.hip ----
struct Range {   // a roctx range, where libroctx64.so is present
    explicit Range(const char* name);
    ~Range();
};
int make_syrk_plan(Engine& e, SyrkPlan& p, int n_row_blk, int n_col_blk, int k_pad);
int setup_lookahead(Engine& e, int n_blk_max, int ld);
int ensure_dense_schur(Engine& e);
int enqueue_iteration(Engine& e, const vmm_ba_options& o);
void drop_graphs(Engine& e);
int run_iteration(Engine& e, const vmm_ba_options& o);
void init_ctl(Engine& e, LmCtl& c, const vmm_ba_options& o, int trace_capacity);
int begin_lm_loop(Engine& e, const vmm_ba_options& o, int trace_capacity);
int flush_state(Engine& e);

// ---- covariance.hip ----
int tag_pose_handle(const Engine& e, const char* who);   // VMM_BA_ERR_STATE: "<who> needs a single-GPU handle with tag-pose landmarks"

// ---- localize.hip: `who` is the entry point's name, for the error text ----
int bad_argument(const char* who, const char* what);                 // VMM_BA_ERR_ARGUMENT, "<who>: <what>"
int hip_failure(const char* who, const char* step, hipError_t err);  // VMM_BA_ERR_HIP, "<who>: <step><error string>"
int check_camera_model(const char* who, const double intr[4], const double dist[5]);   // finite
// known cameras (vmm_ba_triangulate, vmm_ba_locate_tags): finite poses, no zero quaternion, a finite cam_cov (may be null)
int check_cameras(const char* who, int32_t n_cams, const double* cam_qt, const double* cam_cov);
int check_batch(const char* who, MapBatch& mb, int32_t n_tags, const double* tag_qt, const double* tag_wh, int32_t n_imgs,
                const int64_t* img_start, const int32_t* obs_tag, const double* obs_px, const double* cam_qt);
int check_map(const char* who, const MapBatch& mb);
int check_localize_options(const char* who, const vmm_ba_localize_options& o);
// n_obs == 0: every image reports NO_OBSERVATIONS, the identity pose and a zero covariance
void fill_no_observations(int32_t n_imgs, double* cam_qt, double* cam_cov, vmm_ba_localize_result* res);
// hipSetDevice, and on an entry point's first call on a device every preload_* of `preload` (`done`: the caller's flags)
int select_device(const char* who, int device, bool (&done)[64], std::initializer_list<int (*)()> preload);

// ---- the host side of an arrowhead refinement (arrowhead.hpp), shared by calibrate.hip and rig.hip ----
// the options both calibrations have; `who` as above
template <typename Options>
int check_arrow_options(const char* who, const Options& o)
{
    if (o.max_trials < 0 || o.reclassify_passes < 0 || o.min_inlier_tags < 1 || !(o.huber_a > 0.0) || !(o.inlier_px > 0.0)
        || !isfinite(o.huber_a) || !isfinite(o.inlier_px))
        return bad_argument(who, "bad options");
    return VMM_BA_OK;
}
// the options' part of ArrowArgs; the buffers are the caller's
template <typename Options>
void set_arrow_options(ArrowArgs& w, const Options& o)
{
    w.robustify = o.robustify != 0;
    w.min_inliers = o.min_inlier_tags;
    w.huber_a = o.huber_a;
    w.inlier2 = o.inlier_px * o.inlier_px;
}
struct ArrowRun {
    int passes = 0, trials = 0, accepted = 0, stop = 0;
};
// The refinement from the first trial to the covariances, on the null stream, in order; the blocking copies wait for the
// kernels.  Per pass: the control block (ctl: the shared unknowns and refine_mask, max_trials, first set by the caller)
// goes up, from the second pass on classify() flags the observations anew, and trial() runs until the block comes back
// done.  Then covariance(), unless no item takes part.  ctl holds the device's last block at the end; errors go to ar.err.
template <typename Ctl, typename Classify, typename Trial, typename Covariance>
ArrowRun run_arrow(Arena& ar, Ctl& ctl, Ctl* d_ctl, int reclassify_passes, Classify&& classify, Trial&& trial,
                   Covariance&& covariance)
{
    ArrowRun r;
    ArrowCtl& c = ctl.lm;
    for (int pass = 0; pass <= reclassify_passes && ar.err == hipSuccess; ++pass) {
        c.lam = kLamInit;
        c.trials = c.accepted = c.done = c.stop = c.solve_ok = 0;
        ar.copy(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice);
        if (pass > 0 && ar.err == hipSuccess)
            classify();
        // every trial either counts (the solve kernel stops at max_trials) or sets done
        for (int64_t t = 0; t <= (int64_t)c.max_trials + 1 && ar.err == hipSuccess; ++t) {
            trial();
            ar.err = hipGetLastError();
            ar.copy(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost);
            if (c.done)
                break;
        }
        ++r.passes;
        r.trials += c.trials;
        r.accepted += c.accepted;
        if (c.n_used == 0)
            break;
    }
    r.stop = c.stop;
    if (ar.err == hipSuccess && c.n_used > 0) {
        covariance();
        ar.err = hipGetLastError();
        ar.copy(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost);
    }
    return r;
}
// a report that says `status` and nothing else (rep may be null)
template <typename Report>
void empty_report(Report* rep, int status, double time_s)
{
    if (!rep)
        return;
    memset(rep, 0, sizeof(*rep));
    rep->status = status;
    rep->time_s = time_s;
}
inline double finite_or_zero(double v) { return isfinite(v) ? v : 0.0; }
// The report of a refinement in which items took part, but for the number of them (n_images_used / n_frames_used) and
// what else is the entry's own.  finite: the shared unknowns came back finite.
template <typename Report>
void fill_arrow_report(Report* rep, const ArrowCtl& c, const ArrowRun& r, bool finite, double time_s)
{
    memset(rep, 0, sizeof(*rep));
    rep->status = !c.cov_ok ? VMM_BA_CAL_SINGULAR : (r.stop == 2 || !finite ? VMM_BA_CAL_NO_CONVERGENCE : VMM_BA_CAL_OK);
    rep->trials = r.trials;
    rep->accepted = r.accepted;
    rep->passes = r.passes;
    rep->n_obs_used = c.n_obs_used;
    rep->initial_cost = finite_or_zero(0.5 * c.initial_cost);
    rep->final_cost = finite_or_zero(0.5 * c.cost);
    rep->initial_rms_px = c.initial_n_obs > 0 ? finite_or_zero(sqrt(c.initial_raw2 / (4.0 * c.initial_n_obs))) : 0.0;
    rep->final_rms_px = c.n_obs_used > 0 ? finite_or_zero(sqrt(c.raw2 / (4.0 * c.n_obs_used))) : 0.0;
    rep->time_s = time_s;
}

} // namespace vmm
