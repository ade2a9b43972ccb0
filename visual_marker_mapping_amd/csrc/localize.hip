// vmm_ba_localize (include/vmm_ba.h): host side.  Checks the arguments, uploads the map and the detections, launches
// k_quad_pose -> k_map_corners -> k_localize (kernels_init.hip, kernels_localize.hip) and copies the results back.
#include <math.h>
#include <string.h>

#include <string>

#include "engine.hpp"

using namespace vmm;

namespace {

int bad_argument(const char* what)
{
    set_error(std::string("vmm_ba_localize: ") + what);
    return VMM_BA_ERR_ARGUMENT;
}

} // namespace

extern "C" {

void vmm_ba_default_localize_options(vmm_ba_localize_options* o)
{
    if (!o)
        return;
    memset(o, 0, sizeof(*o));
    o->refine_iterations = 30;
    o->robustify = 1;
    o->huber_a = 1.0;
    o->score_cap_px = 100.0;
    o->inlier_px = 8.0;
    o->reclassify_passes = 2;
    o->min_inlier_tags = 1;
}

int vmm_ba_localize(const double intr[4], const double dist[5], int32_t n_tags, const double* tag_qt, const double* tag_wh,
                    int32_t n_imgs, const int64_t* img_start, const int32_t* obs_tag, const double* obs_px,
                    const vmm_ba_localize_options* opt, double* cam_qt, double* cam_cov, uint8_t* obs_inlier,
                    vmm_ba_localize_result* res, int device)
{
    if (!intr || !dist)
        return bad_argument("null camera model");
    if (n_tags < 0 || n_imgs < 0)
        return bad_argument("negative size");
    if (n_imgs == 0)
        return VMM_BA_OK;
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
    for (int64_t i = 0; i < 9; ++i)
        if (!isfinite(i < 4 ? intr[i] : dist[i - 4]))
            return bad_argument("non-finite camera model");
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
    vmm_ba_localize_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_localize_options(&o);
    if (o.refine_iterations < 0 || !(o.huber_a > 0.0) || !(o.score_cap_px > 0.0) || !(o.inlier_px > 0.0) || o.reclassify_passes < 0
        || o.min_inlier_tags < 1 || !isfinite(o.huber_a) || !isfinite(o.score_cap_px) || !isfinite(o.inlier_px))
        return bad_argument("bad options");

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
        return VMM_BA_OK;
    }

    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        set_error(std::string("vmm_ba_localize: hipSetDevice: ") + hipGetErrorString(err));
        return VMM_BA_ERR_HIP;
    }
    static bool preloaded[64] = {};
    if (device >= 0 && device < 64 && !preloaded[device]) {
        if (preload_init_kernels() + preload_localize_kernels() != 0) {
            set_error("vmm_ba_localize: hipFuncGetAttributes failed (code object not loadable on this device)");
            return VMM_BA_ERR_HIP;
        }
        preloaded[device] = true;
    }
    const size_t nt = (size_t)n_tags, ni = (size_t)n_imgs, no = (size_t)n_obs;
    Arena ar;
    const size_t total = Arena::round(8 * 7 * nt) + Arena::round(8 * 2 * nt) + Arena::round(8 * 12 * nt) + Arena::round(8 * (ni + 1))
        + Arena::round(4 * no) + Arena::round(8 * 8 * no) + Arena::round(8 * 14 * no) + Arena::round(8 * 2 * no)
        + Arena::round(8 * 7 * ni) + Arena::round(8 * 36 * ni) + Arena::round(no) + Arena::round(sizeof(vmm_ba_localize_result) * ni);
    if ((err = ar.alloc(total)) != hipSuccess) {
        set_error(std::string("vmm_ba_localize: hipMalloc: ") + hipGetErrorString(err));
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
    double* d_cov = ar.take<double>(36 * ni);
    uint8_t* d_inl = ar.take<uint8_t>(no);
    vmm_ba_localize_result* d_res = ar.take<vmm_ba_localize_result>(ni);

    LocalizeArgs a;
    a.K = make_intrinsics(intr, dist);
    a.n_imgs = n_imgs;
    a.img_start = d_start;
    a.obs_tag = d_obs_tag;
    a.obs_px = d_px;
    a.tag_qt = d_tag_qt;
    a.corners = d_corners;
    a.quad_qt = d_quad_qt;
    a.quad_rms = d_quad_rms;
    a.max_trials = o.refine_iterations;
    a.robustify = o.robustify != 0;
    a.passes = o.reclassify_passes;
    a.min_inliers = o.min_inlier_tags;
    a.huber_a = o.huber_a;
    a.cap2 = o.score_cap_px * o.score_cap_px;
    a.inlier2 = o.inlier_px * o.inlier_px;
    a.cam_qt = d_cam;
    a.cam_cov = d_cov;
    a.obs_inlier = d_inl;
    a.res = d_res;

    // everything on the null stream, in order; the blocking copies back wait for the kernels
    ar.copy(d_tag_qt, tag_qt, 8 * 7 * nt, hipMemcpyHostToDevice);
    ar.copy(d_tag_wh, tag_wh, 8 * 2 * nt, hipMemcpyHostToDevice);
    ar.copy(d_start, img_start, 8 * (ni + 1), hipMemcpyHostToDevice);
    ar.copy(d_obs_tag, obs_tag, 4 * no, hipMemcpyHostToDevice);
    ar.copy(d_px, obs_px, 8 * 8 * no, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess) {
        launch_quad_poses(nullptr, a.K, n_obs, d_tag_wh, d_px, d_quad_qt, d_quad_rms, d_obs_tag);
        launch_map_corners(nullptr, n_tags, d_tag_qt, d_tag_wh, d_corners);
        launch_localize(nullptr, a, any_staged, any_unstaged);
        ar.err = hipGetLastError();
    }
    ar.copy(cam_qt, d_cam, 8 * 7 * ni, hipMemcpyDeviceToHost);
    if (cam_cov)
        ar.copy(cam_cov, d_cov, 8 * 36 * ni, hipMemcpyDeviceToHost);
    if (obs_inlier)
        ar.copy(obs_inlier, d_inl, no, hipMemcpyDeviceToHost);
    if (res)
        ar.copy(res, d_res, sizeof(vmm_ba_localize_result) * ni, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess) {
        set_error(std::string("vmm_ba_localize: ") + hipGetErrorString(ar.err));
        return VMM_BA_ERR_HIP;
    }
    return VMM_BA_OK;
}

} // extern "C"
