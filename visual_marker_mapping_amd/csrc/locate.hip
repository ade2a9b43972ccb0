// vmm_ba_locate_tags (include/vmm_ba.h): host side.  The checks on the cameras, the tags' observations and the options,
// the answers that need no device, one Arena, the uploads, k_quad_pose -> k_camera_rigids -> k_locate_tags
// (kernels_init.hip, kernels_locate.hip) and the copies back.
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
    if (tag_start[0] != 0)
        return bad_argument(who, "tag_start[0] is not 0");
    any_staged = any_unstaged = false;
    const int cap = locate_stage_capacity();
    for (int32_t t = 0; t < n_tags; ++t) {
        const int64_t m = tag_start[t + 1] - tag_start[t];
        if (m < 0)
            return bad_argument(who, "tag_start decreases");
        if (m > (int64_t)1 << 28)
            return bad_argument(who, "a tag has too many observations");
        (m <= cap ? any_staged : any_unstaged) = true;
    }
    const int64_t n_obs = tag_start[n_tags];
    if (n_obs > 0 && (!obs_cam || !obs_px))
        return bad_argument(who, "null observations");
    for (int64_t i = 0; i < n_obs; ++i)
        if (obs_cam[i] < 0 || obs_cam[i] >= n_cams)
            return bad_argument(who, "obs_cam outside [0, n_cams)");
    for (int32_t t = 0; t < n_tags; ++t)
        for (int64_t i = tag_start[t] + 1; i < tag_start[t + 1]; ++i)
            if (obs_cam[i] <= obs_cam[i - 1])
                return bad_argument(who, "obs_cam is not strictly increasing within a tag");
    for (int64_t i = 0; i < 2 * (int64_t)n_tags; ++i)
        if (!isfinite(tag_wh[i]))
            return bad_argument(who, "non-finite tag size");
    for (int64_t i = 0; i < 8 * n_obs; ++i)
        if (!isfinite(obs_px[i]))
            return bad_argument(who, "non-finite obs_px");
    return VMM_BA_OK;
}

// n_obs == 0: every tag reports NO_OBSERVATIONS, the identity pose and zero covariances
void fill_no_tags(int32_t n_tags, double* tag_qt, double* tag_cov, double* tag_cov_cams, vmm_ba_localize_result* res)
{
    fill_no_observations(n_tags, tag_qt, tag_cov, res);
    if (tag_cov_cams)
        memset(tag_cov_cams, 0, sizeof(double) * 36 * (size_t)n_tags);
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
    const size_t nc = (size_t)n_cams, nt = (size_t)n_tags, no = (size_t)tag_start[n_tags];
    if (no == 0) {
        fill_no_tags(n_tags, tag_qt, tag_cov, tag_cov_cams, res);
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_init_kernels, preload_locate_kernels })) != VMM_BA_OK)
        return rc;
    std::vector<int32_t> obs_tag(no);   // k_quad_pose's row of tag_wh for every observation
    for (int32_t t = 0; t < n_tags; ++t)
        for (int64_t i = tag_start[t]; i < tag_start[t + 1]; ++i)
            obs_tag[(size_t)i] = t;
    double *d_qt = nullptr, *d_rigids = nullptr, *d_cam_cov = nullptr, *d_wh = nullptr, *d_px = nullptr, *d_quad_qt = nullptr,
           *d_quad_rms = nullptr, *d_tag = nullptr, *d_cov = nullptr, *d_cov_cams = nullptr;
    int64_t* d_start = nullptr;
    int32_t *d_cam = nullptr, *d_obs_tag = nullptr;
    uint8_t* d_inl = nullptr;
    vmm_ba_localize_result* d_res = nullptr;
    Arena ar;
    if (ar.layout([&](Arena& a) {
            d_qt = a.take<double>(7 * nc);
            d_rigids = a.take<double>(12 * nc);
            d_cam_cov = a.take<double>(cam_cov ? 36 * nc : 0);
            d_wh = a.take<double>(2 * nt);
            d_start = a.take<int64_t>(nt + 1);
            d_cam = a.take<int32_t>(no);
            d_obs_tag = a.take<int32_t>(no);
            d_px = a.take<double>(8 * no);
            d_quad_qt = a.take<double>(14 * no);
            d_quad_rms = a.take<double>(2 * no);
            d_tag = a.take<double>(7 * nt);
            d_cov = a.take<double>(36 * nt);
            d_cov_cams = a.take<double>(36 * nt);
            d_inl = a.take<uint8_t>(no);
            d_res = a.take<vmm_ba_localize_result>(nt);
        }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    ar.copy(d_qt, cam_qt, 8 * 7 * nc, hipMemcpyHostToDevice);
    if (cam_cov)
        ar.copy(d_cam_cov, cam_cov, 8 * 36 * nc, hipMemcpyHostToDevice);
    ar.copy(d_wh, tag_wh, 8 * 2 * nt, hipMemcpyHostToDevice);
    ar.copy(d_start, tag_start, 8 * (nt + 1), hipMemcpyHostToDevice);
    ar.copy(d_cam, obs_cam, 4 * no, hipMemcpyHostToDevice);
    ar.copy(d_obs_tag, obs_tag.data(), 4 * no, hipMemcpyHostToDevice);
    ar.copy(d_px, obs_px, 8 * 8 * no, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess) {
        LocateArgs a;
        a.K = make_intrinsics(intr, dist);
        a.n_tags = n_tags;
        a.rigids = d_rigids;
        a.cam_cov = cam_cov ? d_cam_cov : nullptr;
        a.tag_wh = d_wh;
        a.tag_start = d_start;
        a.obs_cam = d_cam;
        a.obs_px = d_px;
        a.quad_qt = d_quad_qt;
        a.quad_rms = d_quad_rms;
        a.max_trials = o.refine_iterations;
        a.robustify = o.robustify != 0;
        a.passes = o.reclassify_passes;
        a.min_inliers = o.min_inlier_tags;
        a.huber_a = o.huber_a;
        a.cap2 = o.score_cap_px * o.score_cap_px;
        a.inlier2 = o.inlier_px * o.inlier_px;
        a.tag_qt = d_tag;
        a.tag_cov = d_cov;
        a.tag_cov_cams = d_cov_cams;
        a.obs_inlier = d_inl;
        a.res = d_res;
        launch_quad_poses(nullptr, a.K, (int64_t)no, d_wh, d_px, d_quad_qt, d_quad_rms, d_obs_tag);
        launch_camera_rigids(nullptr, n_cams, d_qt, d_rigids);
        launch_locate_tags(nullptr, a, any_staged, any_unstaged);
        ar.err = hipGetLastError();
    }
    ar.copy(tag_qt, d_tag, 8 * 7 * nt, hipMemcpyDeviceToHost);
    if (tag_cov)
        ar.copy(tag_cov, d_cov, 8 * 36 * nt, hipMemcpyDeviceToHost);
    if (tag_cov_cams)
        ar.copy(tag_cov_cams, d_cov_cams, 8 * 36 * nt, hipMemcpyDeviceToHost);
    if (obs_inlier)
        ar.copy(obs_inlier, d_inl, no, hipMemcpyDeviceToHost);
    if (res)
        ar.copy(res, d_res, sizeof(vmm_ba_localize_result) * nt, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

} // extern "C"
