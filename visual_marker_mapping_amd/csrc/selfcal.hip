// The camera model of a handle, and the bundle adjustment that refines it (include/vmm_ba.h): vmm_ba_set_intrinsics,
// vmm_ba_get_intrinsics and vmm_ba_solve_selfcal with its 9 x 9 algebra on the host.  The outer loop calls the handle's
// other entries (vmm_ba_solve, vmm_ba_intrinsics_system, the state accessors) and nothing on the device itself.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "host.hpp"

using namespace vmm;

extern "C" {

int vmm_ba_set_intrinsics(vmm_ba_handle h, const double intr[4], const double dist[5])
{
    if (!h || !intr || !dist) {
        set_error("set_intrinsics: null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(k < 4 ? intr[k] : dist[k - 4])) {
            set_error("set_intrinsics: the camera model is not finite");
            return VMM_BA_ERR_ARGUMENT;
        }
    Engine& e = *reinterpret_cast<Engine*>(h);
    int rc;
    if ((rc = tag_pose_handle(e, "set_intrinsics"))) return rc;
    HIP_TRY(hipSetDevice(e.device));
    e.K = make_intrinsics(intr, dist);
    drop_graphs(e);   // the captured kernels hold the model by value: the next solve captures again
    return VMM_BA_OK;
}

int vmm_ba_get_intrinsics(vmm_ba_handle h, double intr[4], double dist[5])
{
    if (!h || !intr || !dist) {
        set_error("get_intrinsics: null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    const Intrinsics& K = reinterpret_cast<Engine*>(h)->K;
    intr[0] = K.fx; intr[1] = K.fy; intr[2] = K.cx; intr[3] = K.cy;
    dist[0] = K.k1; dist[1] = K.k2; dist[2] = K.p1; dist[3] = K.p2; dist[4] = K.k3;
    return VMM_BA_OK;
}

void vmm_ba_default_selfcal_options(vmm_ba_selfcal_options* o)
{
    if (!o)
        return;
    o->max_outer_iterations = 30;
    o->refine_mask = 0x1FF;
    o->parameter_tolerance = 1e-10;
    o->function_tolerance = 1e-12;
}

// The 9 x 9 system of the camera model on the host, as k_calib_solve (kernels_calibrate.hip) treats its own: the fixed
// parameters get unit rows, the rest is damped by lam diag(S), scaled to a unit diagonal and factored; a pivot times its
// weight must exceed min_pivot.  M receives the factor (lower), sc the scaling.
static bool selfcal_factor(const double* S, const double* C, int mask, double lam, bool weighted, double (&M)[9][9],
                           double (&sc)[9])
{
    bool ok = true;
    double weight[9];
    for (int j = 0; j < 9; ++j) {
        const bool free_j = (mask >> j) & 1;
        const double d = free_j ? S[10 * j] + lam * S[10 * j] : 1.0;
        ok = ok && d > 0.0 && std::isfinite(d);
        sc[j] = free_j && d > 0.0 ? 1.0 / sqrt(d) : 1.0;
        weight[j] = weighted && free_j ? d / C[10 * j] : 1.0;   // S_jj / C_jj
    }
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            const bool both = ((mask >> i) & 1) && ((mask >> j) & 1);
            M[i][j] = i == j ? 1.0 : (both && j < i ? S[9 * i + j] * sc[i] * sc[j] : 0.0);
        }
    for (int j = 0; j < 9 && ok; ++j) {
        double d = M[j][j];
        for (int k = 0; k < j; ++k)
            d -= M[j][k] * M[j][k];
        ok = d * weight[j] > (weighted ? 1e-13 : 0.0) && std::isfinite(d);
        if (!ok)
            break;
        const double sq = sqrt(d);
        M[j][j] = sq;
        for (int i = j + 1; i < 9; ++i) {
            double v = M[i][j];
            for (int k = 0; k < j; ++k)
                v -= M[i][k] * M[j][k];
            M[i][j] = v / sq;
        }
    }
    return ok;
}

// x = D (L L')^-1 D b
static void selfcal_apply(const double (&M)[9][9], const double (&sc)[9], const double* b, double* x)
{
    double z[9];
    for (int i = 0; i < 9; ++i) {
        double v = b[i] * sc[i];
        for (int k = 0; k < i; ++k)
            v -= M[i][k] * z[k];
        z[i] = v / M[i][i];
    }
    for (int i = 8; i >= 0; --i) {
        double v = z[i];
        for (int k = i + 1; k < 9; ++k)
            v -= M[k][i] * z[k];
        z[i] = v / M[i][i];
    }
    for (int i = 0; i < 9; ++i)
        x[i] = z[i] * sc[i];
}

// cov = S^-1 over the free parameters (zeros elsewhere), symmetric in its bits; false (and zeros): S fails the pivot test
static bool selfcal_covariance(const double* S, const double* C, int mask, double* cov)
{
    double M[9][9], sc[9];
    memset(cov, 0, sizeof(double) * 81);
    if (!selfcal_factor(S, C, mask, 0.0, true, M, sc))
        return false;
    double col[9][9];
    bool finite = true;
    for (int j = 0; j < 9; ++j) {
        double unit[9] = {};
        unit[j] = 1.0;
        selfcal_apply(M, sc, unit, col[j]);
        for (int i = 0; i < 9; ++i)
            finite = finite && std::isfinite(col[j][i]);
    }
    if (!finite)
        return false;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j <= i; ++j)
            if (((mask >> i) & 1) && ((mask >> j) & 1))
                cov[9 * i + j] = cov[9 * j + i] = col[j][i];
    return true;
}

int vmm_ba_solve_selfcal(vmm_ba_handle h, const vmm_ba_options* inner, const vmm_ba_selfcal_options* so,
                         vmm_ba_summary* last_inner, vmm_ba_selfcal_report* rep, double intr[4], double dist[5],
                         double* intr_cov)
{
    if (!h || !rep || !intr || !dist) {
        set_error("solve_selfcal: null argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    vmm_ba_selfcal_options o;
    if (so)
        o = *so;
    else
        vmm_ba_default_selfcal_options(&o);
    if (o.max_outer_iterations < 0 || o.refine_mask < 0 || o.refine_mask > 0x1FF || !(o.parameter_tolerance >= 0.0)
        || !(o.function_tolerance >= 0.0)) {
        set_error("solve_selfcal: bad options");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    int rc;
    if ((rc = tag_pose_handle(e, "solve_selfcal"))) return rc;
    vmm_ba_options in;
    if (inner)
        in = *inner;
    else
        vmm_ba_default_options(&in);
    const auto t0 = std::chrono::steady_clock::now();
    memset(rep, 0, sizeof(*rep));
    vmm_ba_summary local;
    memset(&local, 0, sizeof(local));
    vmm_ba_summary* const s = last_inner ? last_inner : &local;
    const int mask = o.refine_mask;
    double k[9], cov[81] = {};
    vmm_ba_get_intrinsics(h, k, k + 4);
    auto solve = [&]() {
        const int r = vmm_ba_solve(h, &in, s);
        if (r == VMM_BA_OK)
            rep->inner_lm_iterations += s->num_lm_iterations;
        return r;
    };
    auto finish = [&](int status, double cost) {
        rep->status = status;
        rep->final_cost = cost;
        memcpy(intr, k, sizeof(double) * 4);
        memcpy(dist, k + 4, sizeof(double) * 5);
        if (intr_cov)
            memcpy(intr_cov, cov, sizeof(cov));
        rep->time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return VMM_BA_OK;
    };
    if ((rc = solve())) return rc;
    double cost = s->final_cost;
    rep->initial_cost = cost;
    if (mask == 0)
        return finish(VMM_BA_CAL_OK, cost);
    if (!std::isfinite(cost)) {
        rep->initial_cost = HUGE_VAL;
        return finish(VMM_BA_CAL_NO_CONVERGENCE, HUGE_VAL);
    }

    const size_t nc = (size_t)7 * e.n_cams, nt = (size_t)7 * e.n_tags;
    std::vector<double> first(nc + nt), cur(nc + nt);   // the state of the first solve; the state a trial starts from
    if ((rc = vmm_ba_get_state(h, first.data(), first.data() + nc))) return rc;
    cur = first;
    double k0[9];
    memcpy(k0, k, sizeof(k));
    const double cost0 = cost;
    auto restore = [&](const std::vector<double>& x, const double* model) {
        int r = vmm_ba_set_state(h, x.data(), x.data() + nc);
        return r ? r : vmm_ba_set_intrinsics(h, model, model + 4);
    };
    // S_k fails the pivot test: the state of the first solve, no covariance
    auto singular = [&]() {
        memset(cov, 0, sizeof(cov));
        memcpy(k, k0, sizeof(k));
        const int r = restore(first, k0);
        return r ? r : finish(VMM_BA_CAL_SINGULAR, cost0);
    };

    double gk[9], C[81], rk[9], Sk[81], dk[9], M[9][9], sc[9];
    double lam = 1e-4;
    bool have_system = false;   // C, r_k, S_k and cov belong to the current state
    int status = VMM_BA_CAL_NO_CONVERGENCE;
    for (;;) {
        if (!have_system) {
            if ((rc = vmm_ba_intrinsics_system(h, in.robustify, in.huber_a, nullptr, gk, C, rk, Sk))) return rc;
            have_system = true;
            double cmax = 0.0;
            for (int j = 0; j < 81; ++j)
                cmax = std::max(cmax, fabs(C[j]));
            if (cmax == 0.0) {   // no active observation: nothing to refine
                memset(cov, 0, sizeof(cov));
                status = VMM_BA_CAL_OK;
                break;
            }
            if (!selfcal_covariance(Sk, C, mask, cov))
                return singular();
        }
        if (lam > 1e12) {
            status = VMM_BA_CAL_OK;
            break;
        }
        if (rep->outer_iterations >= o.max_outer_iterations)
            break;
        rep->outer_iterations += 1;
        bool step_ok = selfcal_factor(Sk, C, mask, lam, false, M, sc);
        if (step_ok) {
            double b[9];
            for (int j = 0; j < 9; ++j)
                b[j] = ((mask >> j) & 1) ? -rk[j] : 0.0;
            selfcal_apply(M, sc, b, dk);
            for (int j = 0; j < 9; ++j) {
                if (!((mask >> j) & 1))
                    dk[j] = 0.0;
                step_ok = step_ok && std::isfinite(dk[j]);
            }
        }
        if (!step_ok) {
            lam *= 10.0;
            continue;
        }
        double kc[9];
        for (int j = 0; j < 9; ++j)
            kc[j] = ((mask >> j) & 1) ? k[j] + dk[j] : k[j];   // a fixed parameter keeps its bits
        if ((rc = vmm_ba_set_intrinsics(h, kc, kc + 4))) return rc;
        if ((rc = solve())) return rc;
        const double cand = s->final_cost;
        if (std::isfinite(cand) && cand < cost) {
            bool small = true;
            for (int j = 0; j < 9; ++j)
                small = small && fabs(dk[j]) / std::max(fabs(k[j]), 1.0) < o.parameter_tolerance;
            const double rel = (cost - cand) / cost;
            memcpy(k, kc, sizeof(k));
            cost = cand;
            lam *= 0.1;
            rep->accepted += 1;
            have_system = false;
            if ((rc = vmm_ba_get_state(h, cur.data(), cur.data() + nc))) return rc;
            if (small || rel < o.function_tolerance) {
                status = VMM_BA_CAL_OK;
                break;
            }
        } else {
            if ((rc = restore(cur, k))) return rc;
            if (cand - cost <= 1e-10 * cost + 1e-20) {   // equal to rounding (cost_at_floor, pose_lm.hpp): the minimum
                status = VMM_BA_CAL_OK;
                break;
            }
            lam *= 10.0;
        }
    }
    if (!have_system) {   // stopped on an accepted step: the covariance at the result
        if ((rc = vmm_ba_intrinsics_system(h, in.robustify, in.huber_a, nullptr, gk, C, rk, Sk))) return rc;
        if (!selfcal_covariance(Sk, C, mask, cov))
            return singular();
    }
    return finish(status, cost);
}

} // extern "C"
