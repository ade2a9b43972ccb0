// vmm_ba_locate_tags (include/vmm_ba.h): host side.  The checks on the cameras, the tags' observations and the options,
// the answer that needs no device, and the known-cameras stage (KnownCameras, host.hpp) with its own four pieces behind
// and k_quad_pose -> k_camera_rigids -> k_locate_tags (kernels_init.hip, kernels_locate.hip) between its uploads and
// its copies back.
#include <math.h>
#include <string.h>

#include <vector>

#include "host.hpp"

using namespace vmm;

namespace {

const char who[] = "vmm_ba_locate_tags";

// any_staged / any_unstaged: a tag of at most / more than locate_stage_capacity() observations
int check_tags(int32_t n_cams, int32_t n_tags, const double* tag_wh, const int64_t* tag_start, const int32_t* obs_cam,
               const double* obs_px, bool& any_staged, bool& any_unstaged)
{
    if (!tag_wh)
        return bad_argument(who, "null tag_wh");
    int64_t shortest, longest;
    const int rc = check_list(who, { "tag_start", "a tag", "obs_cam", "n_cams", true }, n_tags, tag_start, obs_cam, obs_px, n_cams,
                              shortest, longest);
    if (rc != VMM_BA_OK)
        return rc;
    any_staged = shortest <= locate_stage_capacity();
    any_unstaged = longest > locate_stage_capacity();
    for (int64_t i = 0; i < 2 * (int64_t)n_tags; ++i)
        if (!isfinite(tag_wh[i]))
            return bad_argument(who, "non-finite tag size");
    for (int64_t i = 0; i < 8 * tag_start[n_tags]; ++i)
        if (!isfinite(obs_px[i]))
            return bad_argument(who, "non-finite obs_px");
    return VMM_BA_OK;
}

} // namespace

extern "C" {

int vmm_ba_locate_tags(const double intr[4], const double dist[5], int32_t n_cams, const double* cam_qt, const double* cam_cov,
                       int32_t n_tags, const double* tag_wh, const int64_t* tag_start, const int32_t* obs_cam,
                       const double* obs_px, const vmm_ba_localize_options* opt, double* tag_qt, double* tag_cov,
                       double* tag_cov_cams, uint8_t* obs_inlier, vmm_ba_localize_result* res, int device)
{
    if (!intr || !dist)
        return bad_argument(who, "null camera model");
    if (n_cams < 0 || n_tags < 0)
        return bad_argument(who, "negative size");
    if (n_tags == 0)
        return VMM_BA_OK;
    if (!tag_start || !tag_qt)
        return bad_argument(who, "null tag_start or tag_qt");
    vmm_ba_localize_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_localize_options(&o);
    bool any_staged = false, any_unstaged = false;
    int rc;
    if ((rc = check_tags(n_cams, n_tags, tag_wh, tag_start, obs_cam, obs_px, any_staged, any_unstaged)) != VMM_BA_OK
        || (rc = check_camera_model(who, intr, dist)) != VMM_BA_OK || (rc = check_cameras(who, n_cams, cam_qt, cam_cov)) != VMM_BA_OK
        || (rc = check_localize_options(who, o)) != VMM_BA_OK)
        return rc;
    // per camera R | t, per observation four corners, per tag a pose and 6 x 6 covariances
    KnownCameras<vmm_ba_localize_result> kc { n_cams, n_tags, cam_qt, cam_cov, tag_start, obs_cam, obs_px, 12, 8, 7, 36 };
    const size_t nt = (size_t)n_tags, no = kc.n_obs();
    if (no == 0) {   // every tag reports NO_OBSERVATIONS, the identity pose and zero covariances
        fill_without_device(n_tags, tag_start, 7, 36, VMM_BA_LOC_NO_OBSERVATIONS, tag_qt, tag_cov, tag_cov_cams, obs_inlier, res);
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_init_kernels, preload_locate_kernels })) != VMM_BA_OK)
        return rc;
    std::vector<int32_t> obs_tag(no);   // k_quad_pose's row of tag_wh for every observation
    for (int32_t t = 0; t < n_tags; ++t)
        for (int64_t i = tag_start[t]; i < tag_start[t + 1]; ++i)
            obs_tag[(size_t)i] = t;
    double *d_wh = nullptr, *d_quad_qt = nullptr, *d_quad_rms = nullptr;
    int32_t* d_obs_tag = nullptr;
    Arena ar;
    if (ar.layout([&](Arena& a) {
            kc.carve(a);
            d_wh = a.take<double>(2 * nt);
            d_obs_tag = a.take<int32_t>(no);
            d_quad_qt = a.take<double>(14 * no);
            d_quad_rms = a.take<double>(2 * no);
        }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    kc.upload(ar);
    ar.copy(d_wh, tag_wh, 8 * 2 * nt, hipMemcpyHostToDevice);
    ar.copy(d_obs_tag, obs_tag.data(), 4 * no, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess) {
        LocateArgs a;
        a.K = make_intrinsics(intr, dist);
        a.n_tags = n_tags;
        a.rigids = kc.derived;
        a.cam_cov = kc.cam_cov;
        a.tag_wh = d_wh;
        a.tag_start = kc.start;
        a.obs_cam = kc.obs_cam;
        a.obs_px = kc.px;
        a.quad_qt = d_quad_qt;
        a.quad_rms = d_quad_rms;
        set_refine_options(a, o, o.min_inlier_tags);
        a.tag_qt = kc.value;
        a.tag_cov = kc.cov;
        a.tag_cov_cams = kc.cov_cams;
        a.obs_inlier = kc.inl;
        a.res = kc.res;
        launch_quad_poses(nullptr, a.K, (int64_t)no, d_wh, kc.px, d_quad_qt, d_quad_rms, d_obs_tag);
        launch_camera_rigids(nullptr, n_cams, kc.cam_qt, kc.derived);
        launch_locate_tags(nullptr, a, any_staged, any_unstaged);
        ar.err = hipGetLastError();
    }
    kc.results(ar, tag_qt, tag_cov, tag_cov_cams, obs_inlier, res);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

} // extern "C"
