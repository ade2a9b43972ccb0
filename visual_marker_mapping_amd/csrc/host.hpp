// What the host files of libvmm_ba.so share (vmm_ba.hip, covariance.hip, selfcal.hip, initialize.hip, standalone.hip,
// diagnostics.hip, localize.hip, rig.hip, calibrate.hip, triangulate.hip, locate.hip, predict.hip, small_ba.hip): the error returns and
// argument checks (one walk over an item list, check_list, for images, points and tags), the option fields and the
// no-device answer that the stateless entries have in common, the host side of an arrowhead refinement, and
// KnownCameras, the stage of the two entries that take known cameras (MapBatch, the stage of those that take a map, is
// in engine.hpp).
// No kernel; no kernels_*.hip includes this.
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
// The one walk over an item list (images over tags, points or tags over cameras): start[0] == 0, no item of negative
// length or of more than 2^28 observations, ids and obs present where there are observations, every id in [0, n_ids),
// and where `ordered` the ids strictly increasing within an item.  The words of the error texts are the caller's.
struct ListWords {
    const char *start, *item, *ids, *count;   // "img_start", "an image", "obs_tag", "n_tags"
    bool ordered;
};
// shortest / longest: the extreme item lengths (INT64_MAX / 0 without items), for the caller's any_staged, any_pair
int check_list(const char* who, const ListWords& w, int32_t n_items, const int64_t* start, const int32_t* ids, const void* obs,
               int32_t n_ids, int64_t& shortest, int64_t& longest);
int check_batch(const char* who, MapBatch& mb, int32_t n_tags, const double* tag_qt, const double* tag_wh, int32_t n_imgs,
                const int64_t* img_start, const int32_t* obs_tag, const double* obs_px, const double* cam_qt);
int check_map(const char* who, const MapBatch& mb);
int check_localize_options(const char* who, const vmm_ba_localize_options& o);
// hipSetDevice, and on an entry point's first call on a device every preload_* of `preload` (`done`: the caller's flags)
int select_device(const char* who, int device, bool (&done)[64], std::initializer_list<int (*)()> preload);
// the seven option fields that LocalizeArgs, LocateArgs and TriangulateArgs have in common
template <typename Args, typename Options>
void set_refine_options(Args& a, const Options& o, int min_inliers)
{
    a.max_trials = o.refine_iterations;
    a.robustify = o.robustify != 0;
    a.passes = o.reclassify_passes;
    a.min_inliers = min_inliers;
    a.huber_a = o.huber_a;
    a.cap2 = o.score_cap_px * o.score_cap_px;
    a.inlier2 = o.inlier_px * o.inlier_px;
}
// The answer that needs no device: every item gets a zero value (width 7: the identity pose), zero covariances, zero
// flags and a record that says `status` and the item's observations.  start null: no item has any.
template <typename Result>
void fill_without_device(int32_t n, const int64_t* start, int value_width, int cov_width, int status, double* value, double* cov,
                         double* cov_cams, uint8_t* obs_inlier, Result* res)
{
    memset(value, 0, sizeof(double) * value_width * (size_t)n);
    for (int32_t i = 0; i < n && value_width == 7; ++i)
        value[7 * (int64_t)i] = 1.0;
    if (cov)
        memset(cov, 0, sizeof(double) * cov_width * (size_t)n);
    if (cov_cams)
        memset(cov_cams, 0, sizeof(double) * cov_width * (size_t)n);
    if (obs_inlier && start)
        memset(obs_inlier, 0, (size_t)start[n]);
    for (int32_t i = 0; i < n && res; ++i) {
        memset(&res[i], 0, sizeof(res[i]));
        res[i].status = status;
        res[i].n_obs = start ? (int32_t)(start[i + 1] - start[i]) : 0;
    }
}
// n_obs == 0: every image reports NO_OBSERVATIONS, the identity pose and a zero covariance
inline void fill_no_observations(int32_t n_imgs, double* cam_qt, double* cam_cov, vmm_ba_localize_result* res)
{
    fill_without_device(n_imgs, nullptr, 7, 36, VMM_BA_LOC_NO_OBSERVATIONS, cam_qt, cam_cov, nullptr, nullptr, res);
}

// ---- the host stage that vmm_ba_triangulate and vmm_ba_locate_tags share: items (points, tags) over known cameras, from
// the device memory to the copies back.  The entry fills in the caller's arrays and the four widths, carves its own
// pieces behind carve() in the same Arena::layout call, and launches its kernels between upload() and results().
template <typename Result>
struct KnownCameras {
    int32_t n_cams, n_items;
    const double *h_cam_qt, *h_cam_cov;   // h_cam_cov may be null
    const int64_t* h_start;
    const int32_t* h_obs_cam;
    const double* h_px;
    // doubles per camera of the buffer derived from cam_qt (12: k_camera_rigids, kCamFrame: k_cam_frames), per
    // observation of h_px (8, 2), per item of the value (7, 3) and of either covariance (36, 9)
    int cam_stride, px_width, value_width, cov_width;
    // the device copies, and what the kernels write
    double *cam_qt = nullptr, *derived = nullptr, *cam_cov = nullptr, *px = nullptr, *value = nullptr, *cov = nullptr,
           *cov_cams = nullptr;   // cam_cov stays null without h_cam_cov
    int64_t* start = nullptr;
    int32_t* obs_cam = nullptr;
    uint8_t* inl = nullptr;
    Result* res = nullptr;

    size_t n_obs() const { return (size_t)h_start[n_items]; }
    void carve(Arena& a)   // the eleven pieces, in this order
    {
        const size_t nc = (size_t)n_cams, ni = (size_t)n_items, no = n_obs();
        cam_qt = a.take<double>(7 * nc);
        derived = a.take<double>(cam_stride * nc);
        cam_cov = h_cam_cov ? a.take<double>(36 * nc) : nullptr;
        start = a.take<int64_t>(ni + 1);
        obs_cam = a.take<int32_t>(no);
        px = a.take<double>(px_width * no);
        value = a.take<double>(value_width * ni);
        cov = a.take<double>(cov_width * ni);
        cov_cams = a.take<double>(cov_width * ni);
        inl = a.take<uint8_t>(no);
        res = a.take<Result>(ni);
    }
    void upload(Arena& ar) const   // the five copies to the device
    {
        const size_t nc = (size_t)n_cams, no = n_obs();
        ar.copy(cam_qt, h_cam_qt, 8 * 7 * nc, hipMemcpyHostToDevice);
        if (h_cam_cov)
            ar.copy(cam_cov, h_cam_cov, 8 * 36 * nc, hipMemcpyHostToDevice);
        ar.copy(start, h_start, 8 * ((size_t)n_items + 1), hipMemcpyHostToDevice);
        ar.copy(obs_cam, h_obs_cam, 4 * no, hipMemcpyHostToDevice);
        ar.copy(px, h_px, 8 * px_width * no, hipMemcpyHostToDevice);
    }
    // the blocking copies back wait for the kernels; all but the value may be null
    void results(Arena& ar, double* value_out, double* cov_out, double* cov_cams_out, uint8_t* obs_inlier, Result* res_out) const
    {
        const size_t ni = (size_t)n_items;
        ar.copy(value_out, value, 8 * value_width * ni, hipMemcpyDeviceToHost);
        if (cov_out)
            ar.copy(cov_out, cov, 8 * cov_width * ni, hipMemcpyDeviceToHost);
        if (cov_cams_out)
            ar.copy(cov_cams_out, cov_cams, 8 * cov_width * ni, hipMemcpyDeviceToHost);
        if (obs_inlier)
            ar.copy(obs_inlier, inl, n_obs(), hipMemcpyDeviceToHost);
        if (res_out)
            ar.copy(res_out, res, sizeof(Result) * ni, hipMemcpyDeviceToHost);
    }
};

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
