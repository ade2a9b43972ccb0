// vmm_ba_triangulate (include/vmm_ba.h): host side.  The checks on the cameras, the tracks and the options, the answers
// that need no device, one Arena, the uploads, k_cam_frames -> k_triangulate (kernels_triangulate.hip) and the copies
// back.
#include <math.h>
#include <string.h>

#include "host.hpp"

using namespace vmm;

namespace {

const char who[] = "vmm_ba_triangulate";

int check_triangulate_options(const vmm_ba_triangulate_options& o)
{
    if (o.refine_iterations < 0 || !(o.huber_a > 0.0) || !(o.score_cap_px > 0.0) || !(o.inlier_px > 0.0) || o.reclassify_passes < 0
        || o.min_inlier_views < 1 || !isfinite(o.huber_a) || !isfinite(o.score_cap_px) || !isfinite(o.inlier_px)
        || o.max_pair_views < 2 || o.max_pair_views > 64)
        return bad_argument(who, "bad triangulation options");
    return VMM_BA_OK;
}

// any_pair: whether a point has two or more observations
int check_tracks(int32_t n_cams, int32_t n_pts, const int64_t* pt_start, const int32_t* obs_cam, const double* obs_uv, bool& any_pair)
{
    if (pt_start[0] != 0)
        return bad_argument(who, "pt_start[0] is not 0");
    for (int32_t p = 0; p < n_pts; ++p)
        if (pt_start[p + 1] < pt_start[p])
            return bad_argument(who, "pt_start decreases");
    const int64_t n_obs = pt_start[n_pts];
    if (n_obs > 0 && (!obs_cam || !obs_uv))
        return bad_argument(who, "null observations");
    for (int64_t i = 0; i < n_obs; ++i)
        if (obs_cam[i] < 0 || obs_cam[i] >= n_cams)
            return bad_argument(who, "obs_cam outside [0, n_cams)");
    any_pair = false;
    for (int32_t p = 0; p < n_pts; ++p) {
        for (int64_t i = pt_start[p] + 1; i < pt_start[p + 1]; ++i)
            if (obs_cam[i] <= obs_cam[i - 1])
                return bad_argument(who, "obs_cam is not strictly increasing within a point");
        any_pair = any_pair || pt_start[p + 1] - pt_start[p] >= 2;
    }
    for (int64_t i = 0; i < 2 * n_obs; ++i)
        if (!isfinite(obs_uv[i]))
            return bad_argument(who, "non-finite obs_uv");
    return VMM_BA_OK;
}

// no point has two observations: every point reports TOO_FEW_VIEWS, the origin, zero covariances and zero flags
void fill_too_few_views(int32_t n_pts, const int64_t* pt_start, double* xyz, double* xyz_cov, double* xyz_cov_cams,
                        uint8_t* obs_inlier, vmm_ba_triangulate_result* res)
{
    memset(xyz, 0, sizeof(double) * 3 * (size_t)n_pts);
    if (xyz_cov)
        memset(xyz_cov, 0, sizeof(double) * 9 * (size_t)n_pts);
    if (xyz_cov_cams)
        memset(xyz_cov_cams, 0, sizeof(double) * 9 * (size_t)n_pts);
    if (obs_inlier)
        memset(obs_inlier, 0, (size_t)pt_start[n_pts]);
    if (res)
        for (int32_t p = 0; p < n_pts; ++p) {
            memset(&res[p], 0, sizeof(res[p]));
            res[p].status = VMM_BA_TRI_TOO_FEW_VIEWS;
            res[p].n_obs = (int32_t)(pt_start[p + 1] - pt_start[p]);
        }
}

} // namespace

extern "C" {

void vmm_ba_default_triangulate_options(vmm_ba_triangulate_options* o)
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
    o->min_inlier_views = 2;
    o->max_pair_views = 16;
}

int vmm_ba_triangulate(const double intr[4], const double dist[5], int32_t n_cams, const double* cam_qt, const double* cam_cov,
                       int32_t n_pts, const int64_t* pt_start, const int32_t* obs_cam, const double* obs_uv,
                       const vmm_ba_triangulate_options* opt, double* xyz, double* xyz_cov, double* xyz_cov_cams,
                       uint8_t* obs_inlier, vmm_ba_triangulate_result* res, int device)
{
    if (!intr || !dist)
        return bad_argument(who, "null camera model");
    if (n_cams < 0 || n_pts < 0)
        return bad_argument(who, "negative size");
    if (n_pts == 0)
        return VMM_BA_OK;
    if (!pt_start || !xyz)
        return bad_argument(who, "null pt_start or xyz");
    vmm_ba_triangulate_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_triangulate_options(&o);
    bool any_pair = false;
    int rc;
    if ((rc = check_tracks(n_cams, n_pts, pt_start, obs_cam, obs_uv, any_pair)) != VMM_BA_OK
        || (rc = check_camera_model(who, intr, dist)) != VMM_BA_OK || (rc = check_cameras(who, n_cams, cam_qt, cam_cov)) != VMM_BA_OK
        || (rc = check_triangulate_options(o)) != VMM_BA_OK)
        return rc;
    for (int32_t p = 0; p < n_pts; ++p)
        if (pt_start[p + 1] - pt_start[p] > (int64_t)1 << 28)
            return bad_argument(who, "a point has too many observations");
    if (!any_pair) {
        fill_too_few_views(n_pts, pt_start, xyz, xyz_cov, xyz_cov_cams, obs_inlier, res);
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_triangulate_kernels })) != VMM_BA_OK)
        return rc;
    const size_t nc = (size_t)n_cams, np = (size_t)n_pts, no = (size_t)pt_start[n_pts];
    double *d_qt = nullptr, *d_frames = nullptr, *d_cam_cov = nullptr, *d_uv = nullptr, *d_xyz = nullptr, *d_cov = nullptr,
           *d_cov_cams = nullptr;
    int64_t* d_start = nullptr;
    int32_t* d_cam = nullptr;
    uint8_t* d_inl = nullptr;
    vmm_ba_triangulate_result* d_res = nullptr;
    Arena ar;
    if (ar.layout([&](Arena& a) {
            d_qt = a.take<double>(7 * nc);
            d_frames = a.take<double>(kCamFrame * nc);
            d_cam_cov = a.take<double>(cam_cov ? 36 * nc : 0);
            d_start = a.take<int64_t>(np + 1);
            d_cam = a.take<int32_t>(no);
            d_uv = a.take<double>(2 * no);
            d_xyz = a.take<double>(3 * np);
            d_cov = a.take<double>(9 * np);
            d_cov_cams = a.take<double>(9 * np);
            d_inl = a.take<uint8_t>(no);
            d_res = a.take<vmm_ba_triangulate_result>(np);
        }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    ar.copy(d_qt, cam_qt, 8 * 7 * nc, hipMemcpyHostToDevice);
    if (cam_cov)
        ar.copy(d_cam_cov, cam_cov, 8 * 36 * nc, hipMemcpyHostToDevice);
    ar.copy(d_start, pt_start, 8 * (np + 1), hipMemcpyHostToDevice);
    ar.copy(d_cam, obs_cam, 4 * no, hipMemcpyHostToDevice);
    ar.copy(d_uv, obs_uv, 8 * 2 * no, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess) {
        TriangulateArgs a;
        a.K = make_intrinsics(intr, dist);
        a.n_pts = n_pts;
        a.frames = d_frames;
        a.cam_cov = cam_cov ? d_cam_cov : nullptr;
        a.pt_start = d_start;
        a.obs_cam = d_cam;
        a.obs_uv = d_uv;
        a.max_trials = o.refine_iterations;
        a.robustify = o.robustify != 0;
        a.passes = o.reclassify_passes;
        a.min_inliers = o.min_inlier_views;
        a.max_pair = o.max_pair_views;
        a.huber_a = o.huber_a;
        a.cap2 = o.score_cap_px * o.score_cap_px;
        a.inlier2 = o.inlier_px * o.inlier_px;
        a.xyz = d_xyz;
        a.cov = d_cov;
        a.cov_cams = d_cov_cams;
        a.obs_inlier = d_inl;
        a.res = d_res;
        launch_cam_frames(nullptr, n_cams, d_qt, d_frames);
        launch_triangulate(nullptr, a);
        ar.err = hipGetLastError();
    }
    ar.copy(xyz, d_xyz, 8 * 3 * np, hipMemcpyDeviceToHost);
    if (xyz_cov)
        ar.copy(xyz_cov, d_cov, 8 * 9 * np, hipMemcpyDeviceToHost);
    if (xyz_cov_cams)
        ar.copy(xyz_cov_cams, d_cov_cams, 8 * 9 * np, hipMemcpyDeviceToHost);
    if (obs_inlier)
        ar.copy(obs_inlier, d_inl, no, hipMemcpyDeviceToHost);
    if (res)
        ar.copy(res, d_res, sizeof(vmm_ba_triangulate_result) * np, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

} // extern "C"
