// vmm_ba_localize (include/vmm_ba.h): host side, and the stage it shares with vmm_ba_calibrate (MapBatch, engine.hpp):
// the checks on the batch, the map and the localisation options, the answers that need no device, the device memory of
// the common buffers, the uploads, k_quad_pose -> k_map_corners -> k_localize (kernels_init.hip, kernels_localize.hip)
// and the copies back.  vmm_ba_localize is that stage plus its return.
#include <math.h>
#include <string.h>

#include <string>

#include "host.hpp"

namespace vmm {

int bad_argument(const char* who, const char* what)
{
    set_error(std::string(who) + ": " + what);
    return VMM_BA_ERR_ARGUMENT;
}

int hip_failure(const char* who, const char* step, hipError_t err)
{
    set_error(std::string(who) + ": " + step + hipGetErrorString(err));
    return VMM_BA_ERR_HIP;
}

int check_camera_model(const char* who, const double intr[4], const double dist[5])
{
    for (int i = 0; i < 9; ++i)
        if (!isfinite(i < 4 ? intr[i] : dist[i - 4]))
            return bad_argument(who, "non-finite camera model");
    return VMM_BA_OK;
}

int check_cameras(const char* who, int32_t n_cams, const double* cam_qt, const double* cam_cov)
{
    if (n_cams > 0 && !cam_qt)
        return bad_argument(who, "null cam_qt");
    for (int32_t i = 0; i < n_cams; ++i) {
        const double* q = cam_qt + 7 * (int64_t)i;
        for (int k = 0; k < 7; ++k)
            if (!isfinite(q[k]))
                return bad_argument(who, "non-finite camera pose");
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0))
            return bad_argument(who, "zero camera quaternion");
    }
    if (cam_cov)
        for (int64_t k = 0; k < 36 * (int64_t)n_cams; ++k)
            if (!isfinite(cam_cov[k]))
                return bad_argument(who, "non-finite cam_cov");
    return VMM_BA_OK;
}

int check_batch(const char* who, MapBatch& mb, int32_t n_tags, const double* tag_qt, const double* tag_wh, int32_t n_imgs,
                const int64_t* img_start, const int32_t* obs_tag, const double* obs_px, const double* cam_qt)
{
    if (!img_start || !cam_qt)
        return bad_argument(who, "null img_start or cam_qt");
    if (n_tags > 0 && (!tag_qt || !tag_wh))
        return bad_argument(who, "null map");
    if (img_start[0] != 0)
        return bad_argument(who, "img_start[0] is not 0");
    mb.any_staged = mb.any_unstaged = false;
    const int cap = localize_stage_capacity();
    for (int32_t i = 0; i < n_imgs; ++i) {
        const int64_t m = img_start[i + 1] - img_start[i];
        if (m < 0)
            return bad_argument(who, "img_start decreases");
        if (m > (int64_t)1 << 28)
            return bad_argument(who, "an image has too many observations");
        (m <= cap ? mb.any_staged : mb.any_unstaged) = true;
    }
    const int64_t n_obs = img_start[n_imgs];
    if (n_obs > 0 && (!obs_tag || !obs_px))
        return bad_argument(who, "null observations");
    for (int64_t i = 0; i < n_obs; ++i)
        if (obs_tag[i] < 0 || obs_tag[i] >= n_tags)
            return bad_argument(who, "obs_tag outside [0, n_tags)");
    mb.n_tags = n_tags;
    mb.n_imgs = n_imgs;
    mb.n_obs = n_obs;
    mb.h_tag_qt = tag_qt;
    mb.h_tag_wh = tag_wh;
    mb.h_start = img_start;
    mb.h_obs_tag = obs_tag;
    mb.h_px = obs_px;
    return VMM_BA_OK;
}

int check_map(const char* who, const MapBatch& mb)
{
    for (int32_t t = 0; t < mb.n_tags; ++t) {
        const double* q = mb.h_tag_qt + 7 * (int64_t)t;
        for (int k = 0; k < 7; ++k)
            if (!isfinite(q[k]))
                return bad_argument(who, "non-finite map pose");
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0))
            return bad_argument(who, "zero map quaternion");
        if (!isfinite(mb.h_tag_wh[2 * t]) || !isfinite(mb.h_tag_wh[2 * t + 1]))
            return bad_argument(who, "non-finite tag size");
    }
    return VMM_BA_OK;
}

int check_localize_options(const char* who, const vmm_ba_localize_options& o)
{
    if (o.refine_iterations < 0 || !(o.huber_a > 0.0) || !(o.score_cap_px > 0.0) || !(o.inlier_px > 0.0) || o.reclassify_passes < 0
        || o.min_inlier_tags < 1 || !isfinite(o.huber_a) || !isfinite(o.score_cap_px) || !isfinite(o.inlier_px))
        return bad_argument(who, "bad localisation options");
    return VMM_BA_OK;
}

void fill_no_observations(int32_t n_imgs, double* cam_qt, double* cam_cov, vmm_ba_localize_result* res)
{
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
}

int select_device(const char* who, int device, bool (&done)[64], std::initializer_list<int (*)()> preload)
{
    const hipError_t err = hipSetDevice(device);
    if (err != hipSuccess)
        return hip_failure(who, "hipSetDevice: ", err);
    if (device >= 0 && device < 64 && !done[device]) {
        int bad = 0;
        for (int (*f)() : preload)
            bad += f();
        if (bad != 0) {
            set_error(std::string(who) + ": hipFuncGetAttributes failed (code object not loadable on this device)");
            return VMM_BA_ERR_HIP;
        }
        done[device] = true;
    }
    return VMM_BA_OK;
}

void MapBatch::carve(Arena& ar)
{
    const size_t nt = (size_t)n_tags, ni = (size_t)n_imgs, no = (size_t)n_obs;
    tag_qt = ar.take<double>(7 * nt);
    tag_wh = ar.take<double>(2 * nt);
    corners = ar.take<double>(12 * nt);
    start = ar.take<int64_t>(ni + 1);
    obs_tag = ar.take<int32_t>(no);
    px = ar.take<double>(8 * no);
    quad_qt = ar.take<double>(14 * no);
    quad_rms = ar.take<double>(2 * no);
    cam = ar.take<double>(7 * ni);
    cov = ar.take<double>(36 * ni);
    inl = ar.take<uint8_t>(no);
    res = ar.take<vmm_ba_localize_result>(ni);
}

LocalizeArgs MapBatch::args(const double intr[4], const double dist[5], const vmm_ba_localize_options& o) const
{
    LocalizeArgs a;
    a.K = make_intrinsics(intr, dist);
    a.n_imgs = n_imgs;
    a.img_start = start;
    a.obs_tag = obs_tag;
    a.obs_px = px;
    a.tag_qt = tag_qt;
    a.corners = corners;
    a.quad_qt = quad_qt;
    a.quad_rms = quad_rms;
    a.max_trials = o.refine_iterations;
    a.robustify = o.robustify != 0;
    a.passes = o.reclassify_passes;
    a.min_inliers = o.min_inlier_tags;
    a.huber_a = o.huber_a;
    a.cap2 = o.score_cap_px * o.score_cap_px;
    a.inlier2 = o.inlier_px * o.inlier_px;
    a.cam_qt = cam;
    a.cam_cov = cov;
    a.obs_inlier = inl;
    a.res = res;
    return a;
}

void MapBatch::upload(Arena& ar) const
{
    const size_t nt = (size_t)n_tags, ni = (size_t)n_imgs, no = (size_t)n_obs;
    ar.copy(tag_qt, h_tag_qt, 8 * 7 * nt, hipMemcpyHostToDevice);
    ar.copy(tag_wh, h_tag_wh, 8 * 2 * nt, hipMemcpyHostToDevice);
    ar.copy(start, h_start, 8 * (ni + 1), hipMemcpyHostToDevice);
    ar.copy(obs_tag, h_obs_tag, 4 * no, hipMemcpyHostToDevice);
    ar.copy(px, h_px, 8 * 8 * no, hipMemcpyHostToDevice);
}

void MapBatch::results(Arena& ar, double* cam_qt, double* cam_cov, uint8_t* obs_inlier, vmm_ba_localize_result* res_out) const
{
    const size_t ni = (size_t)n_imgs, no = (size_t)n_obs;
    ar.copy(cam_qt, cam, 8 * 7 * ni, hipMemcpyDeviceToHost);
    if (cam_cov)
        ar.copy(cam_cov, cov, 8 * 36 * ni, hipMemcpyDeviceToHost);
    if (obs_inlier)
        ar.copy(obs_inlier, inl, no, hipMemcpyDeviceToHost);
    if (res_out)
        ar.copy(res_out, res, sizeof(vmm_ba_localize_result) * ni, hipMemcpyDeviceToHost);
}

} // namespace vmm

using namespace vmm;

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
    static const char who[] = "vmm_ba_localize";
    if (!intr || !dist)
        return bad_argument(who, "null camera model");
    if (n_tags < 0 || n_imgs < 0)
        return bad_argument(who, "negative size");
    if (n_imgs == 0)
        return VMM_BA_OK;
    MapBatch mb;
    vmm_ba_localize_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_localize_options(&o);
    int rc;
    if ((rc = check_batch(who, mb, n_tags, tag_qt, tag_wh, n_imgs, img_start, obs_tag, obs_px, cam_qt)) != VMM_BA_OK
        || (rc = check_camera_model(who, intr, dist)) != VMM_BA_OK || (rc = check_map(who, mb)) != VMM_BA_OK
        || (rc = check_localize_options(who, o)) != VMM_BA_OK)
        return rc;
    if (mb.n_obs == 0) {
        fill_no_observations(n_imgs, cam_qt, cam_cov, res);
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_init_kernels, preload_localize_kernels })) != VMM_BA_OK)
        return rc;
    Arena ar;
    if (ar.layout([&](Arena& a) { mb.carve(a); }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    mb.run(ar, mb.args(intr, dist, o), [] {});
    mb.results(ar, cam_qt, cam_cov, obs_inlier, res);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

} // extern "C"
