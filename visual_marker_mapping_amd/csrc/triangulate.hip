// vmm_ba_triangulate (include/vmm_ba.h): host side.  The checks on the cameras, the tracks and the options, the answer
// that needs no device, and the known-cameras stage (KnownCameras, host.hpp) with k_cam_frames -> k_triangulate
// (kernels_triangulate.hip) between its uploads and its copies back.
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
    int64_t shortest, longest;
    const int rc = check_list(who, { "pt_start", "a point", "obs_cam", "n_cams", true }, n_pts, pt_start, obs_cam, obs_uv, n_cams,
                              shortest, longest);
    if (rc != VMM_BA_OK)
        return rc;
    any_pair = longest >= 2;
    for (int64_t i = 0; i < 2 * pt_start[n_pts]; ++i)
        if (!isfinite(obs_uv[i]))
            return bad_argument(who, "non-finite obs_uv");
    return VMM_BA_OK;
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
    if (!any_pair) {   // every point reports TOO_FEW_VIEWS, the origin, zero covariances and zero flags
        fill_without_device(n_pts, pt_start, 3, 9, VMM_BA_TRI_TOO_FEW_VIEWS, xyz, xyz_cov, xyz_cov_cams, obs_inlier, res);
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded, { preload_triangulate_kernels })) != VMM_BA_OK)
        return rc;
    // per camera a frame, per observation (u, v), per point xyz and 3 x 3 covariances
    KnownCameras<vmm_ba_triangulate_result> kc { n_cams, n_pts, cam_qt, cam_cov, pt_start, obs_cam, obs_uv, kCamFrame, 2, 3, 9 };
    Arena ar;
    if (ar.layout([&](Arena& a) { kc.carve(a); }) != hipSuccess)
        return hip_failure(who, "hipMalloc: ", ar.err);
    kc.upload(ar);
    if (ar.err == hipSuccess) {
        TriangulateArgs a;
        a.K = make_intrinsics(intr, dist);
        a.n_pts = n_pts;
        a.frames = kc.derived;
        a.cam_cov = kc.cam_cov;
        a.pt_start = kc.start;
        a.obs_cam = kc.obs_cam;
        a.obs_uv = kc.px;
        set_refine_options(a, o, o.min_inlier_views);
        a.max_pair = o.max_pair_views;
        a.xyz = kc.value;
        a.cov = kc.cov;
        a.cov_cams = kc.cov_cams;
        a.obs_inlier = kc.inl;
        a.res = kc.res;
        launch_cam_frames(nullptr, n_cams, kc.cam_qt, kc.derived);
        launch_triangulate(nullptr, a);
        ar.err = hipGetLastError();
    }
    kc.results(ar, xyz, xyz_cov, xyz_cov_cams, obs_inlier, res);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

} // extern "C"
