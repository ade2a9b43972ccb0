// What the host files of libvmm_ba.so share (vmm_ba.hip, covariance.hip, selfcal.hip, initialize.hip, standalone.hip,
// diagnostics.hip, localize.hip, rig.hip, calibrate.hip, triangulate.hip).  No device code; no kernels_*.hip includes this.
#pragma once

#include <algorithm>
#include <initializer_list>
#include <string>

#include "engine.hpp"

namespace vmm {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                         \
            return VMM_BA_ERR_HIP;                                                                 \
        }                                                                                          \
    } while (0)

template <typename T>
int dev_alloc(Engine& e, T** p, size_t count, bool zero = true)
{
    *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    HIP_TRY(hipMalloc((void**)p, bytes));
    e.allocs.push_back(*p);
    if (zero)
        HIP_TRY(hipMemsetAsync(*p, 0, bytes, e.stream));
    return VMM_BA_OK;
}

// ---- vmm_ba.hip ----
struct Range {   // a roctx range, where libroctx64.so is present
    explicit Range(const char* name);
    ~Range();
};
int make_syrk_plan(Engine& e, SyrkPlan& p, int n_row_blk, int n_col_blk, int k_pad);
int setup_lookahead(Engine& e, int n_blk_max, int ld);
int ensure_dense_schur(Engine& e);
int enqueue_iteration(Engine& e, const vmm_ba_options& o);
void drop_graphs(Engine& e);
int run_iteration(Engine& e, const vmm_ba_options& o);
void init_ctl(Engine& e, LmCtl& c, const vmm_ba_options& o, int trace_capacity);
int begin_lm_loop(Engine& e, const vmm_ba_options& o, int trace_capacity);
int flush_state(Engine& e);

// ---- covariance.hip ----
int tag_pose_handle(const Engine& e, const char* who);   // VMM_BA_ERR_STATE: "<who> needs a single-GPU handle with tag-pose landmarks"

// ---- localize.hip: `who` is the entry point's name, for the error text ----
int bad_argument(const char* who, const char* what);                 // VMM_BA_ERR_ARGUMENT, "<who>: <what>"
int hip_failure(const char* who, const char* step, hipError_t err);  // VMM_BA_ERR_HIP, "<who>: <step><error string>"
int check_camera_model(const char* who, const double intr[4], const double dist[5]);   // finite
int check_batch(const char* who, MapBatch& mb, int32_t n_tags, const double* tag_qt, const double* tag_wh, int32_t n_imgs,
                const int64_t* img_start, const int32_t* obs_tag, const double* obs_px, const double* cam_qt);
int check_map(const char* who, const MapBatch& mb);
int check_localize_options(const char* who, const vmm_ba_localize_options& o);
// n_obs == 0: every image reports NO_OBSERVATIONS, the identity pose and a zero covariance
void fill_no_observations(int32_t n_imgs, double* cam_qt, double* cam_cov, vmm_ba_localize_result* res);
// hipSetDevice, and on an entry point's first call on a device every preload_* of `preload` (`done`: the caller's flags)
int select_device(const char* who, int device, bool (&done)[64], std::initializer_list<int (*)()> preload);

} // namespace vmm
