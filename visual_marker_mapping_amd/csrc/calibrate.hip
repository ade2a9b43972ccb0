// vmm_ba_calibrate (include/vmm_ba.h): host side.  The checks, the device memory of the common buffers, the uploads,
// the localisation under the starting camera model and the copies back are the stage it shares with vmm_ba_localize
// (MapBatch, engine.hpp; defined in localize.hip).  The trial loop, which drives the joint Levenberg-Marquardt refinement
// of kernels_calibrate.hip one trial at a time and reads the small control block back after each, the check of the
// calibration options and the report are host.hpp's (run_arrow, check_arrow_options, fill_arrow_report), shared with
// rig.hip.  Its own: the arguments, the mask rule, seven more buffers behind the common ones, CalibArgs, the start
// values and writing back the camera model.
#include <math.h>
#include <string.h>

#include <chrono>
#include <string>

#include "host.hpp"
#include "pose_lm.hpp"

using namespace vmm;

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
    if ((rc = check_arrow_options(who, o)) != VMM_BA_OK)
        return rc;
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
    ca.w.cand = d_cand;
    ca.w.part = d_part;
    ca.w.n_in = d_n_in;
    ca.w.rec = d_rec;
    ca.w.elim = d_elim;
    ca.w.trial = d_trial;
    set_arrow_options(ca.w, o);
    ca.ctl = d_ctl;
    ca.intr_cov = d_intr_cov;
    ca.cam_cov = mb.cov;

    CalibCtl ctl;
    memset(&ctl, 0, sizeof(ctl));
    for (int i = 0; i < 9; ++i)
        ctl.k[i] = ctl.k_cand[i] = i < 4 ? intr0[i] : dist0[i - 4];
    ctl.lm.refine_mask = o.refine_mask;
    ctl.lm.max_trials = o.max_trials;
    ctl.lm.first = 1;

    mb.run(ar, la, [&] { launch_calib_begin(nullptr, ca); });
    const ArrowRun run = run_arrow(ar, ctl, d_ctl, o.reclassify_passes, [&] { launch_calib_classify(nullptr, ca); },
                                   [&] { launch_calib_trial(nullptr, ca); }, [&] { launch_calib_covariance(nullptr, ca); });
    const int n_used = ctl.lm.n_used;
    mb.results(ar, cam_qt, cam_cov, obs_inlier, res);
    if (intr_cov && n_used > 0)
        ar.copy(intr_cov, d_intr_cov, 8 * 81, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    if (n_used == 0) {   // no image was localised well enough to take part: cam_cov holds the localisation's
        if (cam_cov)
            memset(cam_cov, 0, sizeof(double) * 36 * ni);
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        if (rep)
            rep->passes = run.passes;
        return VMM_BA_OK;
    }
    bool finite = true;
    for (int i = 0; i < 9; ++i)
        finite = finite && isfinite(ctl.k[i]);
    if (finite)
        for (int i = 0; i < 9; ++i)
            (i < 4 ? intr[i] : dist[i - 4]) = ctl.k[i];
    if (rep) {
        fill_arrow_report(rep, ctl.lm, run, finite, elapsed());
        rep->n_images_used = n_used;
    }
    return VMM_BA_OK;
}

} // extern "C"
