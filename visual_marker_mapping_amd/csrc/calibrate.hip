// vmm_ba_calibrate (include/vmm_ba.h): host side.  The checks, the device memory of the common buffers, the uploads,
// the localisation under the starting camera model and the copies back are the stage it shares with vmm_ba_localize
// (MapBatch, engine.hpp; defined in localize.hip).  Its own: the result arguments and the calibration options, seven
// more buffers behind the common ones, CalibArgs, the trial loop, which drives the joint Levenberg-Marquardt refinement
// of kernels_calibrate.hip one trial at a time and reads the small control block back after each, and the report.
#include <math.h>
#include <string.h>

#include <chrono>
#include <string>

#include "host.hpp"
#include "pose_lm.hpp"

using namespace vmm;

namespace {

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
    static const char who[] = "vmm_ba_calibrate";
    const auto t_start = std::chrono::steady_clock::now();
    const auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    if (!intr0 || !dist0)
        return bad_argument(who, "null camera model");
    if (!intr || !dist)
        return bad_argument(who, "null result camera model");
    if (n_tags < 0 || n_imgs < 0)
        return bad_argument(who, "negative size");
    vmm_ba_calibrate_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_calibrate_options(&o);
    int rc;
    if ((rc = check_camera_model(who, intr0, dist0)) != VMM_BA_OK || (rc = check_localize_options(who, o.loc)) != VMM_BA_OK)
        return rc;
    if (o.refine_mask < 0 || o.refine_mask > 0x1FF)
        return bad_argument(who, "refine_mask outside [0, 0x1FF]");
    if (o.max_trials < 0 || o.reclassify_passes < 0 || o.min_inlier_tags < 1 || !(o.huber_a > 0.0) || !(o.inlier_px > 0.0)
        || !isfinite(o.huber_a) || !isfinite(o.inlier_px))
        return bad_argument(who, "bad options");
    const auto start_values = [&]() {   // what comes back unless the refinement moves it
        memcpy(intr, intr0, 4 * sizeof(double));
        memcpy(dist, dist0, 5 * sizeof(double));
        if (intr_cov)
            memset(intr_cov, 0, 81 * sizeof(double));
    };
    if (n_imgs == 0) {
        start_values();
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        return VMM_BA_OK;
    }
    MapBatch mb;
    if ((rc = check_batch(who, mb, n_tags, tag_qt, tag_wh, n_imgs, img_start, obs_tag, obs_px, cam_qt)) != VMM_BA_OK
        || (rc = check_map(who, mb)) != VMM_BA_OK)
        return rc;
    start_values();
    if (mb.n_obs == 0) {
        fill_no_observations(n_imgs, cam_qt, cam_cov, res);
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        return VMM_BA_OK;
    }

    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_init_kernels, preload_localize_kernels, preload_calibrate_kernels }))
        != VMM_BA_OK)
        return rc;
    const size_t ni = (size_t)n_imgs;
    Arena ar;
    double *d_cand = nullptr, *d_rec = nullptr, *d_elim = nullptr, *d_trial = nullptr, *d_intr_cov = nullptr;
    int32_t *d_part = nullptr, *d_n_in = nullptr;
    CalibCtl* d_ctl = nullptr;
    const auto carve = [&](Arena& a) {
        mb.carve(a);
        d_cand = a.take<double>(7 * ni);
        d_part = a.take<int32_t>(ni);
        d_n_in = a.take<int32_t>(ni);
        d_rec = a.take<double>(kCalRec * ni);
        d_elim = a.take<double>(kCalElim * ni);
        d_trial = a.take<double>(2 * ni);
        d_ctl = a.take<CalibCtl>(1);
        d_intr_cov = a.take<double>(81);
    };
    if (ar.layout(carve) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    const LocalizeArgs la = mb.args(intr0, dist0, o.loc);

    CalibArgs ca;
    ca.n_imgs = n_imgs;
    ca.img_start = mb.start;
    ca.obs_tag = mb.obs_tag;
    ca.obs_px = mb.px;
    ca.corners = mb.corners;
    ca.flags = mb.inl;
    ca.res = mb.res;
    ca.cam_qt = mb.cam;
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
    ca.cam_cov = mb.cov;

    CalibCtl ctl;
    memset(&ctl, 0, sizeof(ctl));
    for (int i = 0; i < 9; ++i)
        ctl.k[i] = ctl.k_cand[i] = i < 4 ? intr0[i] : dist0[i - 4];
    ctl.refine_mask = o.refine_mask;
    ctl.max_trials = o.max_trials;
    ctl.first = 1;

    // everything on the null stream, in order; the blocking copies wait for the kernels
    mb.run(ar, la, [&] { launch_calib_begin(nullptr, ca); });
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
    mb.results(ar, cam_qt, cam_cov, obs_inlier, res);
    if (intr_cov && ctl.n_used > 0)
        ar.copy(intr_cov, d_intr_cov, 8 * 81, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
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
