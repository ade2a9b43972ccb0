// vmm_ba_initialize (include/vmm_ba.h): initial poses of a handle from its tag detections alone, grown round by round
// from the constant poses (kernels_init.hip).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "host.hpp"

using namespace vmm;

extern "C" {

void vmm_ba_default_init_options(vmm_ba_init_options* o)
{
    if (!o)
        return;
    memset(o, 0, sizeof(*o));
    o->sweeps = 1;
    o->min_tag_observations = 2;
    o->score_cap_px = 100.0;
    o->refine_iterations = 30;
}

int vmm_ba_initialize(vmm_ba_handle h, const vmm_ba_init_options* opt, vmm_ba_init_report* r, uint8_t* cam_reached,
                      uint8_t* tag_reached)
{
    if (!h) {
        set_error("null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.world > 1 || e.points) {
        set_error("vmm_ba_initialize needs a single-GPU handle with tag-pose landmarks");
        return VMM_BA_ERR_STATE;
    }
    if (!e.any_const) {
        set_error("vmm_ba_initialize needs a fixed (origin) tag or a constant pose: the map grows from there");
        return VMM_BA_ERR_ARGUMENT;
    }
    vmm_ba_init_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_init_options(&o);
    if (o.sweeps < 0 || o.min_tag_observations < 1 || !(o.score_cap_px > 0.0) || o.refine_iterations < 0) {
        set_error("bad initialisation options");
        return VMM_BA_ERR_ARGUMENT;
    }
    HIP_TRY(hipSetDevice(e.device));
    Range range("vmm_ba_initialize");
    const auto t0 = std::chrono::steady_clock::now();
    const int n_pose = e.n_cams + e.n_tags;
    int rc;
    if (!e.init_placed) {
        const size_t n_obs = (size_t)std::max<int64_t>(e.n_obs, 1);
        if ((rc = dev_alloc(e, &e.init_quad_qt, 14 * n_obs, false))) return rc;
        if ((rc = dev_alloc(e, &e.init_quad_rms, 2 * n_obs, false))) return rc;
        if ((rc = dev_alloc(e, &e.init_todo, (size_t)n_pose))) return rc;
        if ((rc = dev_alloc(e, &e.init_counter, 1))) return rc;
        if ((rc = dev_alloc(e, &e.init_stats, 2 + 2 * (size_t)e.n_cams))) return rc;
        if (hipHostMalloc((void**)&e.init_host, sizeof(double) * 4) != hipSuccess) {
            set_error("hipHostMalloc failed");
            e.init_host = nullptr;
            return VMM_BA_ERR_HIP;
        }
        if ((rc = dev_alloc(e, &e.init_placed, (size_t)n_pose))) return rc;
    }
    if ((rc = flush_state(e))) return rc;
    launch_init_begin(e);
    launch_init_quad(e);
    InitPass pass;
    pass.min_tag_observations = o.min_tag_observations;
    pass.score_cap_px = o.score_cap_px;
    pass.refine_iterations = o.refine_iterations;
    int32_t* const placed_now = reinterpret_cast<int32_t*>(e.init_host);
    int rounds = 0;
    // every round but the last places at least one pose, so n_pose rounds are the most there can be
    for (int round = 0; round < n_pose; ++round) {
        HIP_TRY(hipMemsetAsync(e.init_counter, 0, sizeof(int32_t), e.stream));
        launch_init_pass(e, true, pass);
        launch_init_pass(e, false, pass);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(placed_now, e.init_counter, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
        HIP_TRY(hipStreamSynchronize(e.stream));
        ++rounds;
        if (*placed_now == 0)
            break;
    }
    pass.sweep = true;
    for (int s = 0; s < o.sweeps; ++s) {
        launch_init_pass(e, true, pass);
        launch_init_pass(e, false, pass);
    }
    launch_init_stats(e, e.init_stats);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> placed((size_t)n_pose);
    HIP_TRY(hipMemcpyAsync(e.init_host + 2, e.init_stats, sizeof(double) * 2, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipMemcpyAsync(placed.data(), e.init_placed, sizeof(int32_t) * n_pose, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    int n_c = 0, n_t = 0;
    for (int c = 0; c < e.n_cams; ++c) {
        n_c += placed[(size_t)c] != 0;
        if (cam_reached)
            cam_reached[c] = placed[(size_t)c] != 0;
    }
    for (int t = 0; t < e.n_tags; ++t) {
        n_t += placed[(size_t)e.n_cams + t] != 0;
        if (tag_reached)
            tag_reached[t] = placed[(size_t)e.n_cams + t] != 0;
    }
    if (r) {
        memset(r, 0, sizeof(*r));
        r->rounds = rounds;
        r->cams_reached = n_c;
        r->tags_reached = n_t;
        r->avg_reprojection_px = e.init_host[3] > 0.0 ? e.init_host[2] / e.init_host[3] : 0.0;
        r->time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return VMM_BA_OK;
}

} // extern "C"
