// vmm_ba_calibrate (include/vmm_ba.h): host side.  Checks the arguments, uploads the map and the detections, localises
// the images under the starting camera model (k_quad_pose -> k_map_corners -> k_localize, as vmm_ba_localize runs them),
// then drives the joint Levenberg-Marquardt refinement of kernels_calibrate.hip one trial at a time, reading the small
// control block back after each, and copies the results back.
#include <math.h>
#include <string.h>

#include <chrono>
#include <string>

#include "engine.hpp"
#include "pose_lm.hpp"

using namespace vmm;

namespace {

int bad_argument(const char* what)
{
    set_error(std::string("vmm_ba_calibrate: ") + what);
    return VMM_BA_ERR_ARGUMENT;
}

void empty_report(vmm_ba_calibrate_report* rep, int status, double time_s)
{
    if (!rep)
        return;
    memset(rep, 0, sizeof(*rep));
    rep->status = status;
    rep->time_s = time_s;
}

double finite_or_zero(double v) { return isfinite(v) ? v : 0.0; }

} // namespace

extern "C" {

void vmm_ba_default_calibrate_options(vmm_ba_calibrate_options* o)
{
    if (!o)
        return;
    memset(o, 0, sizeof(*o));
    vmm_ba_default_localize_options(&o->loc);
    o->max_trials = 100;
    o->refine_mask = 0x1FF;
    o->robustify = 1;
    o->reclassify_passes = 2;
    o->min_inlier_tags = 2;
    o->huber_a = 1.0;
    o->inlier_px = 8.0;
}

int vmm_ba_calibrate(const double intr0[4], const double dist0[5], int32_t n_tags, const double* tag_qt, const double* tag_wh,
                     int32_t n_imgs, const int64_t* img_start, const int32_t* obs_tag, const double* obs_px,
                     const vmm_ba_calibrate_options* opt, double intr[4], double dist[5], double* intr_cov, double* cam_qt,
                     double* cam_cov, uint8_t* obs_inlier, vmm_ba_localize_result* res, vmm_ba_calibrate_report* rep, int device)
{
    const auto t_start = std::chrono::steady_clock::now();
    const auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    if (!intr0 || !dist0)
        return bad_argument("null camera model");
    if (!intr || !dist)
        return bad_argument("null result camera model");
    if (n_tags < 0 || n_imgs < 0)
        return bad_argument("negative size");
    for (int i = 0; i < 9; ++i)
        if (!isfinite(i < 4 ? intr0[i] : dist0[i - 4]))
            return bad_argument("non-finite camera model");
    vmm_ba_calibrate_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_calibrate_options(&o);
    const vmm_ba_localize_options& lo = o.loc;
    if (lo.refine_iterations < 0 || !(lo.huber_a > 0.0) || !(lo.score_cap_px > 0.0) || !(lo.inlier_px > 0.0)
        || lo.reclassify_passes < 0 || lo.min_inlier_tags < 1 || !isfinite(lo.huber_a) || !isfinite(lo.score_cap_px)
        || !isfinite(lo.inlier_px))
        return bad_argument("bad localisation options");
    if (o.refine_mask < 0 || o.refine_mask > 0x1FF)
        return bad_argument("refine_mask outside [0, 0x1FF]");
    if (o.max_trials < 0 || o.reclassify_passes < 0 || o.min_inlier_tags < 1 || !(o.huber_a > 0.0) || !(o.inlier_px > 0.0)
        || !isfinite(o.huber_a) || !isfinite(o.inlier_px))
        return bad_argument("bad options");
    if (n_imgs == 0) {
        memcpy(intr, intr0, 4 * sizeof(double));
        memcpy(dist, dist0, 5 * sizeof(double));
        if (intr_cov)
            memset(intr_cov, 0, 81 * sizeof(double));
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        return VMM_BA_OK;
    }
    if (!img_start || !cam_qt)
        return bad_argument("null img_start or cam_qt");
    if (n_tags > 0 && (!tag_qt || !tag_wh))
        return bad_argument("null map");
    if (img_start[0] != 0)
        return bad_argument("img_start[0] is not 0");
    bool any_staged = false, any_unstaged = false;
    const int cap = localize_stage_capacity();
    for (int32_t i = 0; i < n_imgs; ++i) {
        const int64_t m = img_start[i + 1] - img_start[i];
        if (m < 0)
            return bad_argument("img_start decreases");
        if (m > (int64_t)1 << 28)
            return bad_argument("an image has too many observations");
        (m <= cap ? any_staged : any_unstaged) = true;
    }
    const int64_t n_obs = img_start[n_imgs];
    if (n_obs > 0 && (!obs_tag || !obs_px))
        return bad_argument("null observations");
    for (int64_t i = 0; i < n_obs; ++i)
        if (obs_tag[i] < 0 || obs_tag[i] >= n_tags)
            return bad_argument("obs_tag outside [0, n_tags)");
    for (int32_t t = 0; t < n_tags; ++t) {
        const double* q = tag_qt + 7 * (int64_t)t;
        for (int k = 0; k < 7; ++k)
            if (!isfinite(q[k]))
                return bad_argument("non-finite map pose");
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0))
            return bad_argument("zero map quaternion");
        if (!isfinite(tag_wh[2 * t]) || !isfinite(tag_wh[2 * t + 1]))
            return bad_argument("non-finite tag size");
    }

    memcpy(intr, intr0, 4 * sizeof(double));
    memcpy(dist, dist0, 5 * sizeof(double));
    if (intr_cov)
        memset(intr_cov, 0, 81 * sizeof(double));
    if (n_obs == 0) {   // nothing to compute: every image reports NO_OBSERVATIONS
        for (int32_t i = 0; i < n_imgs; ++i) {
            double* q = cam_qt + 7 * (int64_t)i;
            q[0] = 1.0;
            q[1] = q[2] = q[3] = q[4] = q[5] = q[6] = 0.0;
            if (res) {
                memset(&res[i], 0, sizeof(res[i]));
                res[i].status = VMM_BA_LOC_NO_OBSERVATIONS;
            }
        }
        if (cam_cov)
            memset(cam_cov, 0, sizeof(double) * 36 * (size_t)n_imgs);
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        return VMM_BA_OK;
    }

    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        set_error(std::string("vmm_ba_calibrate: hipSetDevice: ") + hipGetErrorString(err));
        return VMM_BA_ERR_HIP;
    }
    static bool preloaded[64] = {};
    if (device >= 0 && device < 64 && !preloaded[device]) {
        if (preload_init_kernels() + preload_localize_kernels() + preload_calibrate_kernels() != 0) {
            set_error("vmm_ba_calibrate: hipFuncGetAttributes failed (code object not loadable on this device)");
            return VMM_BA_ERR_HIP;
        }
        preloaded[device] = true;
    }
    const size_t nt = (size_t)n_tags, ni = (size_t)n_imgs, no = (size_t)n_obs;
    Arena ar;
    const size_t total = Arena::round(8 * 7 * nt) + Arena::round(8 * 2 * nt) + Arena::round(8 * 12 * nt) + Arena::round(8 * (ni + 1))
        + Arena::round(4 * no) + Arena::round(8 * 8 * no) + Arena::round(8 * 14 * no) + Arena::round(8 * 2 * no)
        + 2 * Arena::round(8 * 7 * ni) + Arena::round(8 * 36 * ni) + Arena::round(no) + Arena::round(sizeof(vmm_ba_localize_result) * ni)
        + 2 * Arena::round(4 * ni) + Arena::round(8 * kCalRec * ni) + Arena::round(8 * kCalElim * ni) + Arena::round(8 * 2 * ni)
        + Arena::round(sizeof(CalibCtl)) + Arena::round(8 * 81);
    if ((err = ar.alloc(total)) != hipSuccess) {
        set_error(std::string("vmm_ba_calibrate: hipMalloc: ") + hipGetErrorString(err));
        return VMM_BA_ERR_HIP;
    }
    double* d_tag_qt = ar.take<double>(7 * nt);
    double* d_tag_wh = ar.take<double>(2 * nt);
    double* d_corners = ar.take<double>(12 * nt);
    int64_t* d_start = ar.take<int64_t>(ni + 1);
    int32_t* d_obs_tag = ar.take<int32_t>(no);
    double* d_px = ar.take<double>(8 * no);
    double* d_quad_qt = ar.take<double>(14 * no);
    double* d_quad_rms = ar.take<double>(2 * no);
    double* d_cam = ar.take<double>(7 * ni);
    double* d_cand = ar.take<double>(7 * ni);
    double* d_cov = ar.take<double>(36 * ni);
    uint8_t* d_inl = ar.take<uint8_t>(no);
    vmm_ba_localize_result* d_res = ar.take<vmm_ba_localize_result>(ni);
    int32_t* d_part = ar.take<int32_t>(ni);
    int32_t* d_n_in = ar.take<int32_t>(ni);
    double* d_rec = ar.take<double>(kCalRec * ni);
    double* d_elim = ar.take<double>(kCalElim * ni);
    double* d_trial = ar.take<double>(2 * ni);
    CalibCtl* d_ctl = ar.take<CalibCtl>(1);
    double* d_intr_cov = ar.take<double>(81);

    LocalizeArgs la;
    la.K = make_intrinsics(intr0, dist0);
    la.n_imgs = n_imgs;
    la.img_start = d_start;
    la.obs_tag = d_obs_tag;
    la.obs_px = d_px;
    la.tag_qt = d_tag_qt;
    la.corners = d_corners;
    la.quad_qt = d_quad_qt;
    la.quad_rms = d_quad_rms;
    la.max_trials = lo.refine_iterations;
    la.robustify = lo.robustify != 0;
    la.passes = lo.reclassify_passes;
    la.min_inliers = lo.min_inlier_tags;
    la.huber_a = lo.huber_a;
    la.cap2 = lo.score_cap_px * lo.score_cap_px;
    la.inlier2 = lo.inlier_px * lo.inlier_px;
    la.cam_qt = d_cam;
    la.cam_cov = d_cov;
    la.obs_inlier = d_inl;
    la.res = d_res;

    CalibArgs ca;
    ca.n_imgs = n_imgs;
    ca.img_start = d_start;
    ca.obs_tag = d_obs_tag;
    ca.obs_px = d_px;
    ca.corners = d_corners;
    ca.flags = d_inl;
    ca.res = d_res;
    ca.cam_qt = d_cam;
    ca.cam_cand = d_cand;
    ca.part = d_part;
    ca.n_in = d_n_in;
    ca.rec = d_rec;
    ca.elim = d_elim;
    ca.trial = d_trial;
    ca.ctl = d_ctl;
    ca.robustify = o.robustify != 0;
    ca.min_inliers = o.min_inlier_tags;
    ca.huber_a = o.huber_a;
    ca.inlier2 = o.inlier_px * o.inlier_px;
    ca.intr_cov = d_intr_cov;
    ca.cam_cov = d_cov;

    CalibCtl ctl;
    memset(&ctl, 0, sizeof(ctl));
    for (int i = 0; i < 9; ++i)
        ctl.k[i] = ctl.k_cand[i] = i < 4 ? intr0[i] : dist0[i - 4];
    ctl.refine_mask = o.refine_mask;
    ctl.max_trials = o.max_trials;
    ctl.first = 1;

    // everything on the null stream, in order; the blocking copies wait for the kernels
    ar.copy(d_tag_qt, tag_qt, 8 * 7 * nt, hipMemcpyHostToDevice);
    ar.copy(d_tag_wh, tag_wh, 8 * 2 * nt, hipMemcpyHostToDevice);
    ar.copy(d_start, img_start, 8 * (ni + 1), hipMemcpyHostToDevice);
    ar.copy(d_obs_tag, obs_tag, 4 * no, hipMemcpyHostToDevice);
    ar.copy(d_px, obs_px, 8 * 8 * no, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess) {
        launch_quad_poses(nullptr, la.K, n_obs, d_tag_wh, d_px, d_quad_qt, d_quad_rms, d_obs_tag);
        launch_map_corners(nullptr, n_tags, d_tag_qt, d_tag_wh, d_corners);
        launch_localize(nullptr, la, any_staged, any_unstaged);
        launch_calib_begin(nullptr, ca);
        ar.err = hipGetLastError();
    }
    int passes = 0, trials = 0, accepted = 0;
    for (int pass = 0; pass <= o.reclassify_passes && ar.err == hipSuccess; ++pass) {
        ctl.lam = kLamInit;
        ctl.trials = ctl.accepted = ctl.done = ctl.stop = ctl.solve_ok = 0;
        ar.copy(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice);
        if (pass > 0 && ar.err == hipSuccess)
            launch_calib_classify(nullptr, ca);
        // every trial either counts (k_calib_solve stops at max_trials) or sets done
        for (int64_t t = 0; t <= (int64_t)o.max_trials + 1 && ar.err == hipSuccess; ++t) {
            launch_calib_trial(nullptr, ca);
            ar.err = hipGetLastError();
            ar.copy(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost);
            if (ctl.done)
                break;
        }
        ++passes;
        trials += ctl.trials;
        accepted += ctl.accepted;
        if (ctl.n_used == 0)
            break;
    }
    const int stop = ctl.stop;
    if (ar.err == hipSuccess && ctl.n_used > 0) {
        launch_calib_covariance(nullptr, ca);
        ar.err = hipGetLastError();
        ar.copy(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost);
    }
    ar.copy(cam_qt, d_cam, 8 * 7 * ni, hipMemcpyDeviceToHost);
    if (cam_cov)
        ar.copy(cam_cov, d_cov, 8 * 36 * ni, hipMemcpyDeviceToHost);
    if (obs_inlier)
        ar.copy(obs_inlier, d_inl, no, hipMemcpyDeviceToHost);
    if (res)
        ar.copy(res, d_res, sizeof(vmm_ba_localize_result) * ni, hipMemcpyDeviceToHost);
    if (intr_cov && ctl.n_used > 0)
        ar.copy(intr_cov, d_intr_cov, 8 * 81, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess) {
        set_error(std::string("vmm_ba_calibrate: ") + hipGetErrorString(ar.err));
        return VMM_BA_ERR_HIP;
    }
    if (ctl.n_used == 0) {   // no image was localised well enough to take part: cam_cov holds the localisation's
        if (cam_cov)
            memset(cam_cov, 0, sizeof(double) * 36 * ni);
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        if (rep)
            rep->passes = passes;
        return VMM_BA_OK;
    }
    bool finite = true;
    for (int i = 0; i < 9; ++i)
        finite = finite && isfinite(ctl.k[i]);
    if (finite)
        for (int i = 0; i < 9; ++i)
            (i < 4 ? intr[i] : dist[i - 4]) = ctl.k[i];
    if (rep) {
        memset(rep, 0, sizeof(*rep));
        rep->status = !ctl.cov_ok ? VMM_BA_CAL_SINGULAR : (stop == 2 || !finite ? VMM_BA_CAL_NO_CONVERGENCE : VMM_BA_CAL_OK);
        rep->trials = trials;
        rep->accepted = accepted;
        rep->passes = passes;
        rep->n_images_used = ctl.n_used;
        rep->n_obs_used = ctl.n_obs_used;
        rep->initial_cost = finite_or_zero(0.5 * ctl.initial_cost);
        rep->final_cost = finite_or_zero(0.5 * ctl.cost);
        rep->initial_rms_px = ctl.initial_n_obs > 0 ? finite_or_zero(sqrt(ctl.initial_raw2 / (4.0 * ctl.initial_n_obs))) : 0.0;
        rep->final_rms_px = ctl.n_obs_used > 0 ? finite_or_zero(sqrt(ctl.raw2 / (4.0 * ctl.n_obs_used))) : 0.0;
        rep->time_s = elapsed();
    }
    return VMM_BA_OK;
}

} // extern "C"
