// The entries that factor the undamped system J^T J of a handle at its current state and read something off the factor
// (include/vmm_ba.h): vmm_ba_tag_translation_covariance, vmm_ba_covariance_blocks, vmm_ba_intrinsics_system.  The three
// share one frame, covariance_call; each brings its device workspace and the launches behind the factorisation.
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "host.hpp"

namespace vmm {

// The dense, naturally ordered system for the length of a covariance call: a handle on the block-sparse or tree-ordered
// path switches over (the covariance kernels read Z as a dense matrix) and back when the guard goes out of scope.
struct CovDensePath {
    Engine& e;
    bool v, nz;
    CovDensePath(Engine& e_) : e(e_), v(e_.sparse_schur), nz(e_.chol_nz_on) {}
    int enter()
    {
        if (v) {
            int drc;
            if ((drc = ensure_dense_schur(e))) return drc;
            e.sparse_schur = false;
        }
        e.chol_nz_on = false;   // the dense, naturally ordered system has no block structure to follow
        return VMM_BA_OK;
    }
    ~CovDensePath()
    {
        e.sparse_schur = v;
        e.chol_nz_on = nz;
    }
};

// The preamble of the three entries: the iteration's kernels on the undamped, unscaled system (H blocks, Z,
// S = L L^T + block inverses), then `tail` (the entry's own substitution, Gram kernels and copy of the result), the
// control block back and a synchronisation.  A second attempt only after a spin give-up of the one-launch
// factorisation: the same on the fallback path.
static hipError_t cov_factor_and(Engine& e, int robustify, double huber_a, hipError_t err,
                                 const std::function<hipError_t()>& tail)
{
    vmm_ba_options o;
    vmm_ba_default_options(&o);
    o.robustify = robustify;
    o.huber_a = huber_a;
    for (int attempt = 0; attempt < 2 && err == hipSuccess; ++attempt) {
        init_ctl(e, *e.ctl_host, o, 0);
        err = hipMemcpyAsync(e.ctl, e.ctl_host, sizeof(LmCtl), hipMemcpyHostToDevice, e.stream);
        if (err != hipSuccess)
            break;
        launch_eval_passes(e, robustify, huber_a, false);
        launch_cov_prepare(e);
        launch_elim(e);
        launch_syrk_reduced(e);
        launch_cholesky_solve(e, e.S, e.n_pad, e.ldz, e.yf, e.ctl, attempt > 0);
        launch_chol_inverse(e, e.n_blk - 1);
        err = tail();
        if (err == hipSuccess)
            err = hipMemcpyAsync(e.ctl_host, e.ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, e.stream);
        if (err == hipSuccess)
            err = hipStreamSynchronize(e.stream);
        if (err != hipSuccess || e.ctl_host->done != 2)
            break;
    }
    return err;
}

int tag_pose_handle(const Engine& e, const char* who)
{
    if (e.multi || e.points) {
        set_error(std::string(who) + " needs a single-GPU handle with tag-pose landmarks");
        return VMM_BA_ERR_STATE;
    }
    return VMM_BA_OK;
}

// the handle's device, and the poses staged by vmm_ba_set_state on it
static int select_and_flush(Engine& e)
{
    HIP_TRY(hipSetDevice(e.device));
    return flush_state(e);
}

// What the three entries do once their arguments are checked and their answers without a system are given: the dense
// path for the length of the call, one allocation for the pieces that `carve` takes (released on every way out; the
// Arena's blocking copy() is not used: a handle works on its own stream), `upload` (the entry's copies to those pieces,
// if any), the factorisation with `tail` behind it, and the two ways the result can be bad.  `matrix` names the system in
// the NUMERIC text, `alloc_step` goes in front of the error string of a failed allocation.
static int covariance_call(Engine& e, const char* who, int robustify, double huber_a,
                           const std::function<void(Arena&)>& carve, const std::function<hipError_t()>& tail,
                           const char* matrix = "J^T J", const std::function<hipError_t()>& upload = nullptr,
                           const std::string& alloc_step = "")
{
    CovDensePath dense(e);
    int rc;
    if ((rc = dense.enter())) return rc;
    Arena ar;
    if (ar.layout(carve) != hipSuccess)
        return hip_failure(who, alloc_step.c_str(), ar.err);
    const hipError_t err = cov_factor_and(e, robustify, huber_a, upload ? upload() : hipSuccess, tail);
    if (err != hipSuccess)
        return hip_failure(who, "", err);
    if (e.ctl_host->lin_fail) {
        set_error(std::string(who) + ": " + matrix + " is not positive definite (rank-deficient Jacobian)");
        return VMM_BA_ERR_NUMERIC;
    }
    return VMM_BA_OK;
}

} // namespace vmm

using namespace vmm;

extern "C" {

int vmm_ba_tag_translation_covariance(vmm_ba_handle h, int robustify, double huber_a, double* cov)
{
    if (!h || !cov) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    static const char who[] = "tag_translation_covariance";
    Engine& e = *reinterpret_cast<Engine*>(h);
    int rc;
    if ((rc = tag_pose_handle(e, who))) return rc;
    if ((rc = select_and_flush(e))) return rc;
    if (e.n_obs == 0 || e.n_tags == 0) {
        memset(cov, 0, sizeof(double) * 9 * (size_t)e.n_tags);
        return VMM_BA_OK;
    }
    // L X = B with B = I (tags kept) or Z^T (tags eliminated), then per-tag Gram blocks
    const bool identity_rhs = e.elim_cams;
    const int n_rhs = identity_rhs ? e.n_pad : e.k_dim;
    const int ldb = round_up(n_rhs, 64);
    double *B = nullptr, *cov_dev = nullptr;
    auto carve = [&](Arena& a) {
        B = a.take<double>((size_t)e.n_pad * ldb);
        cov_dev = a.take<double>(9 * (size_t)e.n_tags);
    };
    return covariance_call(e, who, robustify, huber_a, carve, [&]() {
        hipError_t er = hipMemsetAsync(B, 0, sizeof(double) * (size_t)e.n_pad * ldb, e.stream);
        if (er == hipSuccess) {
            launch_cov_rhs(e, B, ldb, identity_rhs);
            launch_cov_trsm(e, B, ldb, ldb / 64, identity_rhs);
            launch_cov_gram(e, B, ldb, cov_dev);
            er = hipGetLastError();
        }
        if (er == hipSuccess)
            er = hipMemcpyAsync(cov, cov_dev, sizeof(double) * 9 * (size_t)e.n_tags, hipMemcpyDeviceToHost, e.stream);
        return er;
    });
}

int vmm_ba_covariance_blocks(vmm_ba_handle h, int robustify, double huber_a, int64_t n_pairs, const int32_t* pose_a,
                             const int32_t* pose_b, double* cov)
{
    if (!h || n_pairs < 0 || n_pairs > INT32_MAX / 4 || (n_pairs > 0 && (!pose_a || !pose_b || !cov))) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    static const char who[] = "covariance_blocks";
    Engine& e = *reinterpret_cast<Engine*>(h);
    int rc;
    if ((rc = tag_pose_handle(e, who))) return rc;
    if (n_pairs == 0)
        return VMM_BA_OK;
    const int n_pose = e.n_cams + e.n_tags;
    for (int64_t p = 0; p < n_pairs; ++p)
        if (pose_a[p] < 0 || pose_a[p] >= n_pose || pose_b[p] < 0 || pose_b[p] >= n_pose) {
            set_error("covariance_blocks: pair " + std::to_string(p) + " names a pose outside [0, n_cams + n_tags)");
            return VMM_BA_ERR_ARGUMENT;
        }
    if ((rc = select_and_flush(e))) return rc;
    if (e.n_obs == 0) {
        memset(cov, 0, sizeof(double) * 36 * (size_t)n_pairs);
        return VMM_BA_OK;
    }
    // the distinct poses of the request, eliminated family first, then the kept poses by ascending row of the reduced
    // system: slot s owns columns 6 s .. 6 s + 5 of the right-hand side, and the first non-zero block row of a 64-column
    // chunk does not decrease from chunk to chunk
    auto eliminated = [&](int p) { return e.elim_cams ? p < e.n_cams : p >= e.n_cams; };
    auto family_index = [&](int p) { return p < e.n_cams ? p : p - e.n_cams; };
    std::vector<int32_t> slot_of((size_t)n_pose, -1), poses;
    for (int64_t p = 0; p < n_pairs; ++p)
        for (int32_t q : { pose_a[p], pose_b[p] })
            if (slot_of[(size_t)q] < 0) {
                slot_of[(size_t)q] = 0;
                poses.push_back(q);
            }
    std::sort(poses.begin(), poses.end(), [&](int32_t a, int32_t b) {
        return eliminated(a) != eliminated(b) ? eliminated(a) : a < b;
    });
    const int n_slots = (int)poses.size();
    const int ldb = round_up(6 * n_slots, 64), n_chunks = ldb / 64;
    // device tables: slot_src[n_slots] | pair[n_pairs][4] = pose a, pose b, slot a, slot b
    std::vector<int32_t> meta((size_t)n_slots + 4 * (size_t)n_pairs);
    std::vector<int> first_row((size_t)n_chunks, e.n_blk), chunks_at((size_t)e.n_blk, 0);
    for (int s = 0; s < n_slots; ++s) {
        const int p = poses[(size_t)s];
        slot_of[(size_t)p] = s;
        const bool el = eliminated(p);
        meta[(size_t)s] = el ? -1 - family_index(p) : 6 * family_index(p);
        for (int c = 6 * s / 64; c <= (6 * s + 5) / 64; ++c)
            first_row[(size_t)c] = std::min(first_row[(size_t)c], el ? 0 : 6 * family_index(p) / 64);
    }
    for (int k = 0; k < e.n_blk; ++k)
        for (int c = 0; c < n_chunks && first_row[(size_t)c] <= k; ++c)
            chunks_at[(size_t)k] = c + 1;
    for (int64_t p = 0; p < n_pairs; ++p) {
        int32_t* m = meta.data() + n_slots + 4 * p;
        m[0] = pose_a[p];
        m[1] = pose_b[p];
        m[2] = slot_of[(size_t)pose_a[p]];
        m[3] = slot_of[(size_t)pose_b[p]];
    }
    const size_t b_bytes = sizeof(double) * (size_t)e.n_pad * ldb;
    double *B = nullptr, *cov_dev = nullptr;
    int32_t* meta_dev = nullptr;
    auto carve = [&](Arena& a) {
        B = a.take<double>((size_t)e.n_pad * ldb);
        cov_dev = a.take<double>(36 * (size_t)n_pairs);
        meta_dev = a.take<int32_t>(meta.size());
    };
    Arena sizing;   // no memory: the bytes the call will ask for, for the text of a failed allocation
    carve(sizing);
    auto upload = [&]() {
        return hipMemcpyAsync(meta_dev, meta.data(), sizeof(int32_t) * meta.size(), hipMemcpyHostToDevice, e.stream);
    };
    auto tail = [&]() {
        hipError_t er = hipMemsetAsync(B, 0, b_bytes, e.stream);
        if (er == hipSuccess) {
            launch_cov_rhs_slots(e, meta_dev, n_slots, B, ldb);
            launch_cov_trsm_mfma(e, B, ldb, chunks_at);
            launch_cov_pairs(e, B, ldb, meta_dev + n_slots, n_pairs, cov_dev);
            er = hipGetLastError();
        }
        if (er == hipSuccess)
            er = hipMemcpyAsync(cov, cov_dev, sizeof(double) * 36 * (size_t)n_pairs, hipMemcpyDeviceToHost, e.stream);
        return er;
    };
    return covariance_call(e, who, robustify, huber_a, carve, tail, "J^T J", upload,
                           "the right-hand side needs " + std::to_string(sizing.used) + " bytes: ");
}

int vmm_ba_intrinsics_system(vmm_ba_handle h, int robustify, double huber_a, double* cost, double* g_k, double* C,
                             double* r_k, double* S_k)
{
    if (!h) {
        set_error("intrinsics_system: null handle");
        return VMM_BA_ERR_ARGUMENT;
    }
    static const char who[] = "intrinsics_system";
    Engine& e = *reinterpret_cast<Engine*>(h);
    int rc;
    if ((rc = tag_pose_handle(e, who))) return rc;
    if ((rc = select_and_flush(e))) return rc;
    double out[kBorderOut] = {};
    if (e.n_obs > 0) {
        double* ws = nullptr;
        auto carve = [&](Arena& a) { ws = a.take<double>(border_workspace_doubles(e)); };
        auto tail = [&]() {
            const double* res = launch_border(e, robustify, huber_a, ws);
            hipError_t er = hipGetLastError();
            if (er == hipSuccess)
                er = hipMemcpyAsync(out, res, sizeof(out), hipMemcpyDeviceToHost, e.stream);
            return er;
        };
        if ((rc = covariance_call(e, who, robustify, huber_a, carve, tail, "the pose system J^T J"))) return rc;
    }
    if (cost) *cost = out[0];
    if (g_k) memcpy(g_k, out + 1, sizeof(double) * 9);
    if (C) memcpy(C, out + 10, sizeof(double) * 81);
    if (r_k) memcpy(r_k, out + 91, sizeof(double) * 9);
    if (S_k) memcpy(S_k, out + 100, sizeof(double) * 81);
    return VMM_BA_OK;
}

} // extern "C"
