// The entries of include/vmm_ba.h that take no handle: vmm_ba_project_points, vmm_ba_pose_plus, vmm_ba_quad_poses, and the
// two dense test entries vmm_ba_dense_spd_solve and vmm_ba_dense_syrk with the scratch engine they run on.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "host.hpp"

using namespace vmm;

extern "C" {

constexpr int kMaxProjectDevices = 64;

int vmm_ba_project_points(const double intr[4], const double dist[5], int64_t n, const double* points_cam,
                          double* uv, int device)
{
    if (!intr || !dist || n < 0 || (n > 0 && (!points_cam || !uv))) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (n == 0)
        return VMM_BA_OK;
    HIP_TRY(hipSetDevice(device));
    const Intrinsics K = make_intrinsics(intr, dist);
    // CameraModel::projectPoint is called point by point by its users: the device buffer of small calls is kept per
    // device (grown on demand, up to 1 M points = 40 MB; larger calls allocate and free), calls are serialised
    static std::mutex mu;
    static double* cache[kMaxProjectDevices] = {};
    static int64_t cache_cap[kMaxProjectDevices] = {};
    std::lock_guard<std::mutex> lock(mu);
    const bool cached = n <= (int64_t)1 << 20 && device >= 0 && device < kMaxProjectDevices;
    Arena ar;   // owns the buffer of a call that is not cached
    double* buf = nullptr;
    if (cached && cache_cap[device] >= n) {
        buf = cache[device];
    } else {
        const int64_t cap = cached ? std::max<int64_t>(n, 1024) : n;
        HIP_TRY(ar.alloc(sizeof(double) * 5 * (size_t)cap));
        buf = reinterpret_cast<double*>(ar.base);
        if (cached) {
            if (cache[device])
                (void)hipFree(cache[device]);
            cache[device] = buf;
            cache_cap[device] = cap;
            ar.base = nullptr;   // the cache owns it now
        }
    }
    double *d_p = buf, *d_uv = buf + 3 * n;
    ar.copy(d_p, points_cam, sizeof(double) * 3 * n, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess)
        launch_project(nullptr, K, n, d_p, d_uv);
    ar.copy(uv, d_uv, sizeof(double) * 2 * n, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess) {
        set_error(std::string("project_points: ") + hipGetErrorString(ar.err));
        return VMM_BA_ERR_HIP;
    }
    return VMM_BA_OK;
}

int vmm_ba_pose_plus(int64_t n, const double* qt, const double* delta, double* out, int device)
{
    if (n < 0 || (n > 0 && (!qt || !delta || !out))) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (n == 0)
        return VMM_BA_OK;
    HIP_TRY(hipSetDevice(device));
    Arena ar;   // qt | delta | out
    HIP_TRY(ar.alloc(sizeof(double) * 20 * n));
    double* const d = reinterpret_cast<double*>(ar.base);
    ar.copy(d, qt, sizeof(double) * 7 * n, hipMemcpyHostToDevice);
    ar.copy(d + 7 * n, delta, sizeof(double) * 6 * n, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess)
        launch_pose_plus(nullptr, n, d, d + 7 * n, d + 13 * n);
    ar.copy(out, d + 13 * n, sizeof(double) * 7 * n, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess) {
        set_error(std::string("pose_plus: ") + hipGetErrorString(ar.err));
        return VMM_BA_ERR_HIP;
    }
    return VMM_BA_OK;
}

int vmm_ba_quad_poses(const double intr[4], const double dist[5], int64_t n, const double* tag_wh, const double* obs_px,
                      double* qt2, double* rms2, int device)
{
    if (!intr || !dist || n < 0 || (n > 0 && (!tag_wh || !obs_px || !qt2 || !rms2))) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (n == 0)
        return VMM_BA_OK;
    HIP_TRY(hipSetDevice(device));
    const Intrinsics K = make_intrinsics(intr, dist);
    Arena ar;   // tag_wh | obs_px | qt2 | rms2
    HIP_TRY(ar.alloc(sizeof(double) * 26 * n));
    double* const d = reinterpret_cast<double*>(ar.base);
    double *d_wh = d, *d_px = d + 2 * n, *d_qt = d + 10 * n, *d_rms = d + 24 * n;
    ar.copy(d_wh, tag_wh, sizeof(double) * 2 * n, hipMemcpyHostToDevice);
    ar.copy(d_px, obs_px, sizeof(double) * 8 * n, hipMemcpyHostToDevice);
    if (ar.err == hipSuccess)
        launch_quad_poses(nullptr, K, n, d_wh, d_px, d_qt, d_rms);
    ar.copy(qt2, d_qt, sizeof(double) * 14 * n, hipMemcpyDeviceToHost);
    ar.copy(rms2, d_rms, sizeof(double) * 2 * n, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess) {
        set_error(std::string("quad_poses: ") + hipGetErrorString(ar.err));
        return VMM_BA_ERR_HIP;
    }
    return VMM_BA_OK;
}

// Minimal engine for the dense test entry points: stream + panel buffer + a control block.
static int make_scratch(Engine& e, int device, int ld)
{
    e.device = device;
    e.sw = read_switches();
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            e.n_cu = prop.multiProcessorCount;
    }
    int rc;
    if ((rc = dev_alloc(e, &e.P, (size_t)4 * kNB * ld))) return rc;
    if ((rc = setup_lookahead(e, ld / kNB, ld))) return rc;
    if ((rc = dev_alloc(e, &e.dinv, (size_t)ld + kNB))) return rc;
    if ((rc = dev_alloc(e, &e.Ldiag, (size_t)(ld / kNB + 1) * 4096))) return rc;
    if ((rc = dev_alloc(e, &e.Linv, (size_t)(ld / kNB + 1) * 4096))) return rc;
    if ((rc = dev_alloc(e, &e.flags, 264))) return rc;
    if ((rc = dev_alloc(e, &e.gran, (size_t)2 * ld))) return rc;
    {
        const int nb = ld / kNB - 1;   // ld = n_pad + 64
        const size_t nd = e.sw.no_dataflow ? 0 : (size_t)dataflow_blocks(nb, e.n_cu, e.sw);
        if (nd > 0 && (rc = dev_alloc(e, &e.df_gran, nd * (nd + 1) / 2 * 8 * 1024)))
            return rc;
        if (nd > 0 && (rc = dev_alloc(e, &e.df_compact, nd * (nd + 1) / 2 * 4096, false)))
            return rc;
        if (nd > 0 && (rc = dev_alloc(e, &e.df_done, nd * (nd + 1) / 2)))
            return rc;
    }
    if ((rc = dev_alloc(e, &e.ctl, 1))) return rc;
    return VMM_BA_OK;
}

static void free_scratch(Engine& e)
{
    if (e.stream)
        (void)hipStreamSynchronize(e.stream);
    for (void* p : e.allocs)
        (void)hipFree(p);
    if (e.stream)
        (void)hipStreamDestroy(e.stream);
    e.allocs.clear();
    e.stream = nullptr;
}

int vmm_ba_dense_spd_solve(int device, int n, const double* A, const double* b, double* x, int* info)
{
    if (n <= 0 || !A || !b || !x) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    const int n_pad = round_up(n, kNB), ld = n_pad + kNB;
    Engine e;
    int rc = make_scratch(e, device, ld);
    double *S = nullptr, *y = nullptr;
    if (!rc) rc = dev_alloc(e, &S, (size_t)ld * ld);
    if (!rc) rc = dev_alloc(e, &y, (size_t)ld);
    if (rc) {
        free_scratch(e);
        return rc;
    }
    std::vector<double> hs((size_t)ld * ld, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
            hs[(size_t)i * ld + j] = A[(size_t)i * n + j];
    for (int i = n; i < n_pad; ++i)
        hs[(size_t)i * ld + i] = 1.0;
    for (int j = 0; j < n; ++j)
        hs[(size_t)n_pad * ld + j] = b[j];
    LmCtl c;
    hipError_t err = hipSuccess;
    // second attempt only after a spin give-up of the one-launch kernels: the same system on the fallback path
    for (int attempt = 0; attempt < 2 && err == hipSuccess; ++attempt) {
        memset(&c, 0, sizeof(c));
        if (attempt == 0) {
            c.spin_limit_df = e.sw.spin_df;
            c.spin_limit_chain = e.sw.spin_chain;
            c.spin_wg = e.sw.spin_wg;
        }
        err = hipMemcpyAsync(e.ctl, &c, sizeof(LmCtl), hipMemcpyHostToDevice, e.stream);
        if (err == hipSuccess)
            err = hipMemcpyAsync(S, hs.data(), sizeof(double) * hs.size(), hipMemcpyHostToDevice, e.stream);
        if (err == hipSuccess) {
            launch_cholesky_solve(e, S, n_pad, ld, y, e.ctl, attempt > 0);
            err = hipGetLastError();
        }
        if (err == hipSuccess) err = hipMemcpyAsync(x, y, sizeof(double) * n, hipMemcpyDeviceToHost, e.stream);
        if (err == hipSuccess) err = hipMemcpyAsync(&c, e.ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, e.stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e.stream);
        if (c.done != 2)
            break;
    }
    free_scratch(e);
    if (err != hipSuccess) {
        set_error(std::string("dense_spd_solve: ") + hipGetErrorString(err));
        return VMM_BA_ERR_HIP;
    }
    if (info)
        *info = c.lin_fail;
    return VMM_BA_OK;
}

int vmm_ba_dense_syrk(int device, int k, int n, const double* Zh, double* C)
{
    if (k <= 0 || n <= 0 || !Zh || !C) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    const int n_pad = round_up(n, kST), ld = n_pad;
    const int n_blk = n_pad / kST;
    const int k_pad = round_up(k, kKT);
    Engine e;
    int rc = make_scratch(e, device, ld);
    double *Z = nullptr, *S = nullptr;
    SyrkPlan plan;
    if (!rc) rc = dev_alloc(e, &Z, (size_t)k_pad * ld);
    if (!rc) rc = dev_alloc(e, &S, (size_t)ld * ld);
    if (!rc) rc = make_syrk_plan(e, plan, n_blk, n_blk, k_pad);
    if (rc) {
        free_scratch(e);
        return rc;
    }
    std::vector<double> hz((size_t)k_pad * ld, 0.0);
    for (int r = 0; r < k; ++r)
        for (int c = 0; c < n; ++c)
            hz[(size_t)r * ld + c] = Zh[(size_t)r * n + c];
    hipError_t err = hipMemcpyAsync(Z, hz.data(), sizeof(double) * hz.size(), hipMemcpyHostToDevice, e.stream);
    std::vector<double> hs((size_t)ld * ld, 0.0);
    if (err == hipSuccess) {
        launch_syrk_plan(e.stream, nullptr, Z, ld, plan);
        launch_reduce_plan(e.stream, nullptr, plan, ld, n_pad, S);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(hs.data(), S, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, e.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e.stream);
    free_scratch(e);
    if (err != hipSuccess) {
        set_error(std::string("dense_syrk: ") + hipGetErrorString(err));
        return VMM_BA_ERR_HIP;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            C[(size_t)i * n + j] = (j <= i) ? -hs[(size_t)i * ld + j] : -hs[(size_t)j * ld + i];
    return VMM_BA_OK;
}

} // extern "C"
