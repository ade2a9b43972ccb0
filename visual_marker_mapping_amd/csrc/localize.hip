// vmm_ba_localize (include/vmm_ba.h): host side, and the stage it shares with vmm_ba_calibrate (MapBatch, engine.hpp):
// the checks on the batch, the map and the localisation options, the answers that need no device, the device memory of
// the common buffers, the uploads, k_quad_pose -> k_map_corners -> k_localize (kernels_init.hip, kernels_localize.hip)
// and the copies back.  vmm_ba_localize is that stage plus its return.  Also the checks every stateless entry shares
// (host.hpp): the camera model, known cameras, and check_list, the one walk over an item list.
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

int check_list(const char* who, const ListWords& w, int32_t n_items, const int64_t* start, const int32_t* ids, const void* obs,
               int32_t n_ids, int64_t& shortest, int64_t& longest)
{
    const std::string s(w.start), id(w.ids), item(w.item);
    if (start[0] != 0)
        return bad_argument(who, (s + "[0] is not 0").c_str());
    shortest = INT64_MAX;
    longest = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        const int64_t m = start[i + 1] - start[i];
        if (m < 0)
            return bad_argument(who, (s + " decreases").c_str());
        if (m > (int64_t)1 << 28)
            return bad_argument(who, (item + " has too many observations").c_str());
        shortest = std::min(shortest, m);
        longest = std::max(longest, m);
    }
    const int64_t n_obs = start[n_items];
    if (n_obs > 0 && (!ids || !obs))
        return bad_argument(who, "null observations");
    for (int64_t i = 0; i < n_obs; ++i)
        if (ids[i] < 0 || ids[i] >= n_ids)
            return bad_argument(who, (id + " outside [0, " + w.count + ")").c_str());
    for (int32_t k = 0; k < n_items && w.ordered; ++k)
        for (int64_t i = start[k] + 1; i < start[k + 1]; ++i)
            if (ids[i] <= ids[i - 1])
                return bad_argument(who, (id + " is not strictly increasing within " + item).c_str());
    return VMM_BA_OK;
}

int check_batch(const char* who, MapBatch& mb, int32_t n_tags, const double* tag_qt, const double* tag_wh, int32_t n_imgs,
                const int64_t* img_start, const int32_t* obs_tag, const double* obs_px, const double* cam_qt)
{
    if (!img_start || !cam_qt)
        return bad_argument(who, "null img_start or cam_qt");
    if (n_tags > 0 && (!tag_qt || !tag_wh))
        return bad_argument(who, "null map");
    int64_t shortest, longest;
    const int rc = check_list(who, { "img_start", "an image", "obs_tag", "n_tags", false }, n_imgs, img_start, obs_tag, obs_px, n_tags,
                              shortest, longest);
    if (rc != VMM_BA_OK)
        return rc;
    mb.any_staged = shortest <= localize_stage_capacity();
    mb.any_unstaged = longest > localize_stage_capacity();
    mb.n_tags = n_tags;
    mb.n_imgs = n_imgs;
    mb.n_obs = img_start[n_imgs];
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
    set_refine_options(a, o, o.min_inlier_tags);
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
