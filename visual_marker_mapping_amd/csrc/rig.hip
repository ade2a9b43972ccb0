// vmm_ba_rig_localize and vmm_ba_rig_calibrate (include/vmm_ba.h): host side.  The batch is localize.hip's MapBatch with
// one image per (frame, camera) slot; its checks, device memory, uploads and k_map_corners are used as they are.
// RigBatch adds what both entries share: the checks on the rig, the quad poses camera by camera (k_quad_pose takes one
// camera model per launch, so the observations are sorted by camera for it and their results scattered back),
// k_rig_localize (kernels_rig.hip) and the copies back per frame.  vmm_ba_rig_calibrate's own: its arguments, the mask
// rules, eight more buffers, the start values and writing back the extrinsics; the trial loop around the kernels of the
// joint refinement, the check of the common options and the report are host.hpp's, shared with calibrate.hip.
#include <math.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "host.hpp"
#include "pose_lm.hpp"

namespace vmm {

namespace {

int check_rig(const char* who, int32_t n_rig_cams, const double* intr, const double* dist, const double* ext_qt)
{
    for (int32_t c = 0; c < n_rig_cams; ++c) {
        const int rc = check_camera_model(who, intr + 4 * c, dist + 5 * c);
        if (rc != VMM_BA_OK)
            return rc;
        const double* q = ext_qt + 7 * c;
        for (int k = 0; k < 7; ++k)
            if (!isfinite(q[k]))
                return bad_argument(who, "non-finite extrinsic");
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0))
            return bad_argument(who, "zero extrinsic quaternion");
    }
    return VMM_BA_OK;
}

// The observations sorted by camera (frames in order inside a camera): camera c owns [off[c], off[c + 1]).
struct ByCamera {
    std::vector<int64_t> off;
    std::vector<int32_t> index, tag;   // position in the caller's order; obs_tag there
    std::vector<double> px;
    ByCamera(const MapBatch& mb, int32_t n_rig_cams, int32_t n_frames) : off(n_rig_cams + 1, 0)
    {
        index.reserve((size_t)mb.n_obs);
        tag.reserve((size_t)mb.n_obs);
        px.reserve(8 * (size_t)mb.n_obs);
        for (int32_t c = 0; c < n_rig_cams; ++c) {
            for (int32_t f = 0; f < n_frames; ++f) {
                const int64_t slot = (int64_t)f * n_rig_cams + c;
                for (int64_t i = mb.h_start[slot]; i < mb.h_start[slot + 1]; ++i) {
                    index.push_back((int32_t)i);
                    tag.push_back(mb.h_obs_tag[i]);
                    px.insert(px.end(), mb.h_px + 8 * i, mb.h_px + 8 * i + 8);
                }
            }
            off[c + 1] = (int64_t)index.size();
        }
    }
};

// A batch of frames of a rig against a map, from the argument checks to the localisation's results.
struct RigBatch {
    MapBatch mb;
    int32_t n_rig_cams = 0, n_frames = 0;
    const double *h_intr = nullptr, *h_dist = nullptr;
    double *intr = nullptr, *dist = nullptr, *ext = nullptr, *px = nullptr;   // device: models, extrinsics, pixels by camera
    int32_t *index = nullptr, *tag = nullptr;

    // the sizes and what needs no batch; then n_frames == 0 is the caller's to answer
    int check_sizes(const char* who, int32_t K, const double* intr_, const double* dist_, const double* ext_qt, int32_t n_tags,
                    int32_t nf)
    {
        if (K < 1 || K > VMM_BA_RIG_MAX_CAMS)
            return bad_argument(who, "n_rig_cams outside [1, VMM_BA_RIG_MAX_CAMS]");
        if (!intr_ || !dist_ || !ext_qt)
            return bad_argument(who, "null camera models or extrinsics");
        if (n_tags < 0 || nf < 0)
            return bad_argument(who, "negative size");
        if (nf > INT32_MAX / VMM_BA_RIG_MAX_CAMS)
            return bad_argument(who, "too many frames");
        n_rig_cams = K;
        n_frames = nf;
        h_intr = intr_;
        h_dist = dist_;
        return VMM_BA_OK;
    }
    int check(const char* who, const double* ext_qt, int32_t n_tags, const double* tag_qt, const double* tag_wh,
              const int64_t* img_start, const int32_t* obs_tag, const double* obs_px, const double* rig_qt,
              const vmm_ba_localize_options& o)
    {
        int rc;
        if ((rc = check_batch(who, mb, n_tags, tag_qt, tag_wh, n_frames * n_rig_cams, img_start, obs_tag, obs_px, rig_qt))
                != VMM_BA_OK
            || (rc = check_rig(who, n_rig_cams, h_intr, h_dist, ext_qt)) != VMM_BA_OK || (rc = check_map(who, mb)) != VMM_BA_OK
            || (rc = check_localize_options(who, o)) != VMM_BA_OK)
            return rc;
        if (mb.n_obs > (int64_t)1 << 28)   // a frame's length and an observation's index are ints on the device
            return bad_argument(who, "too many observations");
        return VMM_BA_OK;
    }
    void carve(Arena& a)
    {
        const size_t nk = (size_t)n_rig_cams, no = (size_t)mb.n_obs;
        mb.carve(a);   // its per-image results are per slot here: the frames use the first n_frames of them
        intr = a.take<double>(4 * nk);
        dist = a.take<double>(5 * nk);
        ext = a.take<double>(7 * nk);
        px = a.take<double>(8 * no);
        index = a.take<int32_t>(no);
        tag = a.take<int32_t>(no);
    }
    // the uploads, then k_quad_pose per camera -> k_map_corners -> k_rig_localize and `then(args)` (the caller's further
    // launches) on the null stream, in order, then one hipGetLastError
    template <typename Then>
    RigArgs run(Arena& ar, const double* ext_qt, const vmm_ba_localize_options& o, Then&& then) const
    {
        const ByCamera by(mb, n_rig_cams, n_frames);
        const size_t nk = (size_t)n_rig_cams, no = (size_t)mb.n_obs;
        RigArgs a;
        a.loc = mb.args(h_intr, h_dist, o);
        a.loc.n_imgs = n_frames;
        a.n_rig_cams = n_rig_cams;
        a.intr = intr;
        a.dist = dist;
        a.ext_qt = ext;
        mb.upload(ar);
        ar.copy(intr, h_intr, 8 * 4 * nk, hipMemcpyHostToDevice);
        ar.copy(dist, h_dist, 8 * 5 * nk, hipMemcpyHostToDevice);
        ar.copy(ext, ext_qt, 8 * 7 * nk, hipMemcpyHostToDevice);
        ar.copy(px, by.px.data(), 8 * 8 * no, hipMemcpyHostToDevice);
        ar.copy(index, by.index.data(), 4 * no, hipMemcpyHostToDevice);
        ar.copy(tag, by.tag.data(), 4 * no, hipMemcpyHostToDevice);
        if (ar.err != hipSuccess)
            return a;
        for (int32_t c = 0; c < n_rig_cams; ++c) {
            const int64_t at = by.off[c];
            launch_quad_poses(nullptr, make_intrinsics(h_intr + 4 * c, h_dist + 5 * c), by.off[c + 1] - at, mb.tag_wh, px + 8 * at,
                              mb.quad_qt, mb.quad_rms, tag + at, index + at);
        }
        launch_map_corners(nullptr, mb.n_tags, mb.tag_qt, mb.tag_wh, mb.corners);
        launch_rig_localize(nullptr, a);
        then(a);
        ar.err = hipGetLastError();
        return a;
    }
    void results(Arena& ar, double* rig_qt, double* rig_cov, uint8_t* obs_inlier, vmm_ba_localize_result* res) const
    {
        const size_t nf = (size_t)n_frames;
        ar.copy(rig_qt, mb.cam, 8 * 7 * nf, hipMemcpyDeviceToHost);
        if (rig_cov)
            ar.copy(rig_cov, mb.cov, 8 * 36 * nf, hipMemcpyDeviceToHost);
        if (obs_inlier)
            ar.copy(obs_inlier, mb.inl, (size_t)mb.n_obs, hipMemcpyDeviceToHost);
        if (res)
            ar.copy(res, mb.res, sizeof(vmm_ba_localize_result) * nf, hipMemcpyDeviceToHost);
    }
};

} // namespace

} // namespace vmm

using namespace vmm;

extern "C" {

int vmm_ba_rig_localize(int32_t n_rig_cams, const double* intr, const double* dist, const double* ext_qt, int32_t n_tags,
                        const double* tag_qt, const double* tag_wh, int32_t n_frames, const int64_t* img_start,
                        const int32_t* obs_tag, const double* obs_px, const vmm_ba_localize_options* opt, double* rig_qt,
                        double* rig_cov, uint8_t* obs_inlier, vmm_ba_localize_result* res, int device)
{
    static const char who[] = "vmm_ba_rig_localize";
    RigBatch rb;
    int rc;
    if ((rc = rb.check_sizes(who, n_rig_cams, intr, dist, ext_qt, n_tags, n_frames)) != VMM_BA_OK)
        return rc;
    if (n_frames == 0)
        return VMM_BA_OK;
    vmm_ba_localize_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_localize_options(&o);
    if ((rc = rb.check(who, ext_qt, n_tags, tag_qt, tag_wh, img_start, obs_tag, obs_px, rig_qt, o)) != VMM_BA_OK)
        return rc;
    if (rb.mb.n_obs == 0) {
        fill_no_observations(n_frames, rig_qt, rig_cov, res);
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_init_kernels, preload_localize_kernels, preload_rig_kernels }))
        != VMM_BA_OK)
        return rc;
    Arena ar;
    if (ar.layout([&](Arena& a) { rb.carve(a); }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    rb.run(ar, ext_qt, o, [](const RigArgs&) {});
    rb.results(ar, rig_qt, rig_cov, obs_inlier, res);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

void vmm_ba_default_rig_calibrate_options(vmm_ba_rig_calibrate_options* o)
{
    if (!o)
        return;
    memset(o, 0, sizeof(*o));
    vmm_ba_default_localize_options(&o->loc);
    o->max_trials = 100;
    o->refine_mask = (1 << VMM_BA_RIG_MAX_CAMS) - 2;   // every camera but 0; the bits at or above n_rig_cams are dropped
    o->robustify = 1;
    o->reclassify_passes = 2;
    o->min_inlier_tags = 2;
    o->huber_a = 1.0;
    o->inlier_px = 8.0;
}

int vmm_ba_rig_calibrate(int32_t n_rig_cams, const double* intr, const double* dist, const double* ext_qt0, int32_t n_tags,
                         const double* tag_qt, const double* tag_wh, int32_t n_frames, const int64_t* img_start,
                         const int32_t* obs_tag, const double* obs_px, const vmm_ba_rig_calibrate_options* opt, double* ext_qt,
                         double* ext_cov, double* rig_qt, double* rig_cov, uint8_t* obs_inlier, vmm_ba_localize_result* res,
                         vmm_ba_rig_calibrate_report* rep, int device)
{
    static const char who[] = "vmm_ba_rig_calibrate";
    const auto t_start = std::chrono::steady_clock::now();
    const auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    RigBatch rb;
    int rc;
    if ((rc = rb.check_sizes(who, n_rig_cams, intr, dist, ext_qt0, n_tags, n_frames)) != VMM_BA_OK)
        return rc;
    if (!ext_qt)
        return bad_argument(who, "null result extrinsics");
    vmm_ba_rig_calibrate_options o;
    const bool default_mask = !opt;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_rig_calibrate_options(&o);
    const int all = (1 << n_rig_cams) - 1;
    if (default_mask || o.refine_mask == (1 << VMM_BA_RIG_MAX_CAMS) - 2)
        o.refine_mask &= all;   // the default: every camera of this rig but 0
    if (o.refine_mask < 0 || o.refine_mask > all)
        return bad_argument(who, "refine_mask has bits at or above n_rig_cams");
    if (o.refine_mask == all)
        return bad_argument(who, "refine_mask frees every camera: at least one extrinsic must be held");
    if ((rc = check_arrow_options(who, o)) != VMM_BA_OK)
        return rc;
    const size_t P = 6 * (size_t)n_rig_cams;
    const auto start_values = [&]() {   // what comes back unless the refinement moves it
        memcpy(ext_qt, ext_qt0, 7 * (size_t)n_rig_cams * sizeof(double));
        if (ext_cov)
            memset(ext_cov, 0, P * P * sizeof(double));
    };
    if (n_frames == 0) {
        if ((rc = check_rig(who, n_rig_cams, intr, dist, ext_qt0)) != VMM_BA_OK
            || (rc = check_localize_options(who, o.loc)) != VMM_BA_OK)
            return rc;
        start_values();
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        return VMM_BA_OK;
    }
    if ((rc = rb.check(who, ext_qt0, n_tags, tag_qt, tag_wh, img_start, obs_tag, obs_px, rig_qt, o.loc)) != VMM_BA_OK)
        return rc;
    start_values();
    if (rb.mb.n_obs == 0) {
        fill_no_observations(n_frames, rig_qt, rig_cov, res);
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_init_kernels, preload_localize_kernels, preload_rig_kernels }))
        != VMM_BA_OK)
        return rc;
    const size_t nf = (size_t)n_frames;
    Arena ar;
    double *d_cand = nullptr, *d_rec = nullptr, *d_elim = nullptr, *d_trial = nullptr, *d_ext_cov = nullptr;
    int32_t *d_part = nullptr, *d_n_in = nullptr;
    RigCalCtl* d_ctl = nullptr;
    if (ar.layout([&](Arena& a) {
            rb.carve(a);
            d_cand = a.take<double>(7 * nf);
            d_part = a.take<int32_t>(nf);
            d_n_in = a.take<int32_t>(nf);
            d_rec = a.take<double>((size_t)arrow_rec_doubles((int)P) * nf);
            d_elim = a.take<double>((size_t)arrow_elim_doubles((int)P) * nf);
            d_trial = a.take<double>(2 * nf);
            d_ctl = a.take<RigCalCtl>(1);
            d_ext_cov = a.take<double>(P * P);
        }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);

    RigCalArgs ca;
    ca.w.cand = d_cand;
    ca.w.part = d_part;
    ca.w.n_in = d_n_in;
    ca.w.rec = d_rec;
    ca.w.elim = d_elim;
    ca.w.trial = d_trial;
    set_arrow_options(ca.w, o);
    ca.ctl = d_ctl;
    ca.ext_cov = d_ext_cov;

    RigCalCtl ctl;
    memset(&ctl, 0, sizeof(ctl));
    memcpy(ctl.ext, ext_qt0, 7 * (size_t)n_rig_cams * sizeof(double));
    memcpy(ctl.ext_cand, ext_qt0, 7 * (size_t)n_rig_cams * sizeof(double));
    ctl.lm.refine_mask = o.refine_mask;
    ctl.lm.max_trials = o.max_trials;
    ctl.lm.first = 1;

    ca.rig = rb.run(ar, ext_qt0, o.loc, [&](const RigArgs& a) {
        ca.rig = a;
        launch_rigcal_begin(nullptr, ca);
    });
    const ArrowRun run = run_arrow(ar, ctl, d_ctl, o.reclassify_passes, [&] { launch_rigcal_classify(nullptr, ca); },
                                   [&] { launch_rigcal_trial(nullptr, ca); }, [&] { launch_rigcal_covariance(nullptr, ca); });
    const int n_used = ctl.lm.n_used;
    rb.results(ar, rig_qt, rig_cov, obs_inlier, res);
    if (ext_cov && n_used > 0)
        ar.copy(ext_cov, d_ext_cov, 8 * P * P, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    if (n_used == 0) {   // no frame was localised well enough to take part: rig_cov holds the localisation's
        if (rig_cov)
            memset(rig_cov, 0, sizeof(double) * 36 * nf);
        empty_report(rep, VMM_BA_CAL_NO_IMAGES, elapsed());
        if (rep)
            rep->passes = run.passes;
        return VMM_BA_OK;
    }
    bool finite = true;
    for (int i = 0; i < 7 * n_rig_cams; ++i)
        finite = finite && isfinite(ctl.ext[i]);
    int cams_refined = 0;   // the extrinsics that moved: a held or unobserved one keeps its bits
    if (finite) {
        for (int c = 0; c < n_rig_cams; ++c)
            if (memcmp(ctl.ext + 7 * c, ext_qt0 + 7 * c, 7 * sizeof(double)) != 0)
                cams_refined |= 1 << c;
        memcpy(ext_qt, ctl.ext, 7 * (size_t)n_rig_cams * sizeof(double));
    }
    if (rep) {
        fill_arrow_report(rep, ctl.lm, run, finite, elapsed());
        rep->n_frames_used = n_used;
        rep->cams_refined = cams_refined;
    }
    return VMM_BA_OK;
}

} // extern "C"
