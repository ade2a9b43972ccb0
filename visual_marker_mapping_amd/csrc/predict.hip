// vmm_ba_predict_localization and vmm_ba_predict_localization_joint (include/vmm_ba.h): host side.  The checks on the
// camera model, the map, the poses, the covariances and the options, the answers that need no device, and
// k_map_corners -> k_tag_faces -> k_cam_frames -> k_predict or k_predict_joint (kernels_localize.hip,
// kernels_triangulate.hip, kernels_predict.hip, kernels_predict_joint.hip) between the uploads and the copies back.
// The two entries are one call frame, predict_call; they differ in the covariance they take and in visible_in.
#include <math.h>
#include <string.h>

#include <string>

#include "host.hpp"

using namespace vmm;

namespace {

int check_predict_options(const char* who, const vmm_ba_predict_options& o)
{
    const auto non_negative = [](double v) { return isfinite(v) && v >= 0.0; };
    if (o.image_width <= 0 || o.image_height <= 0 || !isfinite(o.sigma_px) || !(o.sigma_px > 0.0) || !non_negative(o.margin_px)
        || !non_negative(o.min_depth) || !non_negative(o.min_side_px) || !(o.max_view_angle_deg > 0.0)
        || !(o.max_view_angle_deg <= 90.0) || o.min_tags < 1)
        return bad_argument(who, "bad prediction options");
    return VMM_BA_OK;
}

// joint false: tag_cov is [36 * n_tags] or null and visible_in is null; joint true: tag_cov is [36 * n_tags^2], required
int predict_call(const char* who, bool joint, const double intr[4], const double dist[5], int32_t n_tags, const double* tag_qt,
                 const double* tag_wh, const double* tag_cov, int32_t n_poses, const double* cam_qt, const uint8_t* visible_in,
                 const vmm_ba_predict_options* opt, double* cov_px, double* cov_map, uint8_t* visible, vmm_ba_predict_result* res,
                 int device)
{
    if (!intr || !dist)
        return bad_argument(who, "null camera model");
    if (!cam_qt)
        return bad_argument(who, "null cam_qt");
    if (!opt)
        return bad_argument(who, "null options");
    if (n_tags < 0 || n_poses < 0)
        return bad_argument(who, "negative size");
    if (n_tags > 0 && (!tag_qt || !tag_wh))
        return bad_argument(who, "null map");
    if (joint && n_tags > 0 && !tag_cov)
        return bad_argument(who, "null tag_cov_joint");
    const vmm_ba_predict_options o = *opt;
    MapBatch mb;   // the map alone, for check_map
    mb.n_tags = n_tags;
    mb.h_tag_qt = tag_qt;
    mb.h_tag_wh = tag_wh;
    int rc;
    if ((rc = check_camera_model(who, intr, dist)) != VMM_BA_OK || (rc = check_map(who, mb)) != VMM_BA_OK
        || (rc = check_cameras(who, n_poses, cam_qt, nullptr)) != VMM_BA_OK || (rc = check_predict_options(who, o)) != VMM_BA_OK)
        return rc;
    const size_t nt = (size_t)n_tags, np = (size_t)n_poses;
    if (joint) {   // the blocks s >= t; the upper block triangle may hold anything
        for (size_t s = 0; s < nt; ++s)
            for (size_t k = 36 * s * nt; k < 36 * (s * nt + s + 1); ++k)
                if (!isfinite(tag_cov[k]))
                    return bad_argument(who, "non-finite tag_cov_joint");
    } else {
        for (size_t k = 0; tag_cov && k < 36 * nt; ++k)
            if (!isfinite(tag_cov[k]))
                return bad_argument(who, "non-finite tag_cov");
    }
    if (n_poses == 0)
        return VMM_BA_OK;
    if (n_tags == 0) {   // every pose reports NO_VISIBLE_TAG and zero covariances; `visible` has no entry
        if (cov_px)
            memset(cov_px, 0, sizeof(double) * 36 * np);
        if (cov_map)
            memset(cov_map, 0, sizeof(double) * 36 * np);
        for (size_t i = 0; i < np && res; ++i) {
            memset(&res[i], 0, sizeof(res[i]));
            res[i].status = VMM_BA_PRED_NO_VISIBLE_TAG;
        }
        return VMM_BA_OK;
    }
    static bool preloaded[64] = {};
    if ((rc = select_device(who, device, preloaded,
                            { preload_localize_kernels, preload_triangulate_kernels, preload_predict_kernels, preload_predict_joint_kernels }))
        != VMM_BA_OK)
        return rc;
    const size_t n_cov = joint ? 36 * nt * nt : 36 * nt;
    double *d_tag_qt = nullptr, *d_tag_wh = nullptr, *d_corners = nullptr, *d_faces = nullptr, *d_tag_cov = nullptr,
           *d_cam_qt = nullptr, *d_frames = nullptr, *d_cov_px = nullptr, *d_cov_map = nullptr;
    uint8_t *d_visible = nullptr, *d_visible_in = nullptr;
    vmm_ba_predict_result* d_res = nullptr;
    auto carve = [&](Arena& a) {
        d_tag_qt = a.take<double>(7 * nt);
        d_tag_wh = a.take<double>(2 * nt);
        d_corners = a.take<double>(12 * nt);
        d_faces = a.take<double>(kTagFace * nt);
        d_tag_cov = tag_cov ? a.take<double>(n_cov) : nullptr;
        d_cam_qt = a.take<double>(7 * np);
        d_frames = a.take<double>(kCamFrame * np);
        d_cov_px = cov_px ? a.take<double>(36 * np) : nullptr;
        d_cov_map = cov_map ? a.take<double>(36 * np) : nullptr;
        d_visible = visible || joint ? a.take<uint8_t>(np * nt) : nullptr;   // k_predict_joint's second sweep reads it
        d_visible_in = visible_in ? a.take<uint8_t>(np * nt) : nullptr;
        d_res = res ? a.take<vmm_ba_predict_result>(np) : nullptr;
    };
    Arena sizing;   // no memory: the bytes the call will ask for, for the text of a failed allocation
    carve(sizing);
    Arena ar;
    if (ar.layout(carve) != hipSuccess) {
        const std::string step = joint ? "hipMalloc (" + std::to_string(sizing.used) + " bytes, " + std::to_string(8 * n_cov)
                                             + " of them the joint covariance): "
                                       : std::string("hipMalloc: ");
        return hip_failure(who, step.c_str(), ar.err);
    }
    ar.copy(d_tag_qt, tag_qt, 8 * 7 * nt, hipMemcpyHostToDevice);
    ar.copy(d_tag_wh, tag_wh, 8 * 2 * nt, hipMemcpyHostToDevice);
    if (tag_cov)
        ar.copy(d_tag_cov, tag_cov, 8 * n_cov, hipMemcpyHostToDevice);
    ar.copy(d_cam_qt, cam_qt, 8 * 7 * np, hipMemcpyHostToDevice);
    if (visible_in)
        ar.copy(d_visible_in, visible_in, np * nt, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess) {
        PredictArgs a;
        a.K = make_intrinsics(intr, dist);
        a.n_tags = n_tags;
        a.n_poses = n_poses;
        a.corners = d_corners;
        a.faces = d_faces;
        a.tag_cov = joint ? nullptr : d_tag_cov;
        a.frames = d_frames;
        a.u_lo = o.margin_px;
        a.u_hi = (double)o.image_width - o.margin_px;
        a.v_lo = o.margin_px;
        a.v_hi = (double)o.image_height - o.margin_px;
        a.min_depth = o.min_depth;
        a.cos_max_angle = cos(o.max_view_angle_deg * (M_PI / 180.0));
        a.min_side2 = o.min_side_px * o.min_side_px;
        a.sigma2 = o.sigma_px * o.sigma_px;
        a.min_tags = o.min_tags;
        a.cov_px = d_cov_px;
        a.cov_map = d_cov_map;
        a.visible = d_visible;
        a.res = d_res;
        launch_map_corners(nullptr, n_tags, d_tag_qt, d_tag_wh, d_corners);
        launch_tag_faces(nullptr, n_tags, d_tag_qt, d_faces);
        launch_cam_frames(nullptr, n_poses, d_cam_qt, d_frames);
        if (joint) {
            PredictJointArgs ja;
            ja.p = a;
            ja.tag_cov_joint = d_tag_cov;
            ja.visible_in = d_visible_in;
            launch_predict_joint(nullptr, ja);
        } else
            launch_predict(nullptr, a);
        ar.err = hipGetLastError();
    }
    // the blocking copies back wait for the kernels
    if (cov_px)
        ar.copy(cov_px, d_cov_px, 8 * 36 * np, hipMemcpyDeviceToHost);
    if (cov_map)
        ar.copy(cov_map, d_cov_map, 8 * 36 * np, hipMemcpyDeviceToHost);
    if (visible)
        ar.copy(visible, d_visible, np * nt, hipMemcpyDeviceToHost);
    if (res)
        ar.copy(res, d_res, sizeof(vmm_ba_predict_result) * np, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);
    return VMM_BA_OK;
}

} // namespace

extern "C" {

void vmm_ba_default_predict_options(vmm_ba_predict_options* o)
{
    if (!o)
        return;
    memset(o, 0, sizeof(*o));   // image_width, image_height: no default
    o->sigma_px = 1.0;
    o->margin_px = 0.0;
    o->min_depth = 1e-3;
    o->max_view_angle_deg = 70.0;
    o->min_side_px = 10.0;
    o->min_tags = 1;
}

int vmm_ba_predict_localization(const double intr[4], const double dist[5], int32_t n_tags, const double* tag_qt,
                                const double* tag_wh, const double* tag_cov, int32_t n_poses, const double* cam_qt,
                                const vmm_ba_predict_options* opt, double* cov_px, double* cov_map, uint8_t* visible,
                                vmm_ba_predict_result* res, int device)
{
    return predict_call("vmm_ba_predict_localization", false, intr, dist, n_tags, tag_qt, tag_wh, tag_cov, n_poses, cam_qt, nullptr,
                        opt, cov_px, cov_map, visible, res, device);
}

int vmm_ba_predict_localization_joint(const double intr[4], const double dist[5], int32_t n_tags, const double* tag_qt,
                                      const double* tag_wh, const double* tag_cov_joint, int32_t n_poses, const double* cam_qt,
                                      const uint8_t* visible_in, const vmm_ba_predict_options* opt, double* cov_px, double* cov_map,
                                      uint8_t* visible, vmm_ba_predict_result* res, int device)
{
    return predict_call("vmm_ba_predict_localization_joint", true, intr, dist, n_tags, tag_qt, tag_wh, tag_cov_joint, n_poses, cam_qt,
                        visible_in, opt, cov_px, cov_map, visible, res, device);
}

} // extern "C"
