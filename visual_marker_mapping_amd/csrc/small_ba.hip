// vmm_ba_solve_small (include/vmm_ba.h): host side.  The checks on the batch, the choice of the eliminated family, the
// sort of every problem's observations by (eliminated pose, kept pose), the one allocation that holds the batch and its
// scratch, k_small_ba (kernels_small.hip) between the uploads and the copies back, and the summaries.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <vector>

#include "host.hpp"
#include "small_ba.hpp"

using namespace vmm;

namespace {

const char who[] = "vmm_ba_solve_small";

int bad_problem(int32_t i, const std::string& what)
{
    return bad_argument(who, ("problem " + std::to_string(i) + ": " + what).c_str());
}

// what vmm_ba_create rejects in a problem, and the limit of this entry
int check_problem(int32_t i, const vmm_ba_problem& p, int32_t elimination, bool& elim_cams)
{
    if (p.n_cams <= 0 || p.n_tags <= 0 || p.n_obs < 0 || !p.cam_qt || !p.tag_qt || !p.tag_wh
        || (p.n_obs > 0 && (!p.obs_cam || !p.obs_tag || !p.obs_px)))
        return bad_problem(i, "needs >= 1 camera, >= 1 tag and non-null arrays");
    if (p.n_obs >= (int64_t)1 << 31)
        return bad_problem(i, "n_obs must fit in 31 bits");
    if ((int64_t)p.n_cams + p.n_tags >= (int64_t)1 << 31)
        return bad_problem(i, "n_cams + n_tags must fit in 31 bits");
    for (int64_t k = 0; k < p.n_obs; ++k)
        if (p.obs_cam[k] < 0 || p.obs_cam[k] >= p.n_cams || p.obs_tag[k] < 0 || p.obs_tag[k] >= p.n_tags)
            return bad_problem(i, "observation " + std::to_string(k) + " references a camera or tag index out of range");
    if (p.fixed_tag >= p.n_tags)
        return bad_problem(i, "fixed_tag out of range");
    elim_cams = elimination == VMM_BA_ELIM_AUTO ? p.n_cams >= p.n_tags : elimination == VMM_BA_ELIM_CAMERAS;
    const int32_t kept = elim_cams ? p.n_tags : p.n_cams;
    if (kept > VMM_BA_SMALL_MAX_KEPT)
        return bad_problem(i, "the kept family has " + std::to_string(kept) + " poses, more than VMM_BA_SMALL_MAX_KEPT ("
                                  + std::to_string(VMM_BA_SMALL_MAX_KEPT) + ")");
    return VMM_BA_OK;
}

} // namespace

extern "C" {

int vmm_ba_solve_small(int32_t n_problems, const vmm_ba_problem* problems, const uint8_t* cam_const, const uint8_t* tag_const,
                       const vmm_ba_options* opt, int32_t elimination, double* cam_qt, double* tag_qt,
                       vmm_ba_summary* summaries, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (n_problems < 0)
        return bad_argument(who, "negative n_problems");
    if (n_problems == 0)
        return VMM_BA_OK;
    if (!problems || !cam_qt || !tag_qt || !summaries)
        return bad_argument(who, "null problems, cam_qt, tag_qt or summaries");
    if (elimination != VMM_BA_ELIM_AUTO && elimination != VMM_BA_ELIM_TAGS && elimination != VMM_BA_ELIM_CAMERAS)
        return bad_argument(who, "bad elimination mode");
    vmm_ba_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_options(&o);
    if (o.max_num_iterations < 0 || !(o.initial_trust_region_radius > 0.0))
        return bad_argument(who, "bad solver options");

    // ---- the batch: checks, offsets ----
    const size_t np = (size_t)n_problems;
    std::vector<SmallDesc> desc(np);
    std::vector<int64_t> cam_off(np + 1, 0), tag_off(np + 1, 0);
    size_t n_pose = 0, n_obs = 0, n_estart = 0, n_fstart = 0, n_pstart = 0, n_trace = 0;
    for (int32_t i = 0; i < n_problems; ++i) {
        const vmm_ba_problem& p = problems[i];
        bool elim_cams = false;
        const int rc = check_problem(i, p, elimination, elim_cams);
        if (rc != VMM_BA_OK)
            return rc;
        SmallDesc& d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.K = make_intrinsics(p.intr, p.dist);
        d.n_cams = p.n_cams;
        d.n_tags = p.n_tags;
        d.n_obs = (int32_t)p.n_obs;
        d.elim_cams = elim_cams ? 1 : 0;
        d.n_e = elim_cams ? p.n_cams : p.n_tags;
        d.n_f = elim_cams ? p.n_tags : p.n_cams;
        d.trace_capacity = summaries[i].trace ? std::max(summaries[i].trace_capacity, 0) : 0;
        d.pose_off = (int64_t)n_pose;
        d.obs_off = (int64_t)n_obs;
        d.e_start_off = (int64_t)n_estart;
        d.f_start_off = (int64_t)n_fstart;
        d.pair_start_off = (int64_t)n_pstart;
        d.trace_off = (int64_t)n_trace;
        n_pose += (size_t)p.n_cams + (size_t)p.n_tags;
        n_obs += (size_t)p.n_obs;
        n_estart += (size_t)d.n_e + 1;
        n_fstart += (size_t)d.n_f + 1;
        n_pstart += (size_t)d.n_f * ((size_t)d.n_f + 1) / 2 + 1;
        n_trace += (size_t)d.trace_capacity;
        cam_off[(size_t)i + 1] = cam_off[(size_t)i] + p.n_cams;
        tag_off[(size_t)i + 1] = tag_off[(size_t)i] + p.n_tags;
    }

    // ---- the host images of the device arrays ----
    std::vector<double> h_x(7 * n_pose), h_wh(2 * n_pose, 0.0), h_px(8 * n_obs);
    std::vector<uint8_t> h_const(n_pose, 0);
    std::vector<int32_t> h_obs_e(n_obs), h_obs_f(n_obs), h_estart(n_estart), h_fstart(n_fstart), h_flist(n_obs), h_pstart(n_pstart), h_pairs;
    std::vector<int32_t> order;
    for (int32_t i = 0; i < n_problems; ++i) {
        const vmm_ba_problem& p = problems[i];
        SmallDesc& d = desc[(size_t)i];
        const size_t po = (size_t)d.pose_off, oo = (size_t)d.obs_off, nc = (size_t)p.n_cams, nt = (size_t)p.n_tags;
        memcpy(&h_x[7 * po], p.cam_qt, sizeof(double) * 7 * nc);
        memcpy(&h_x[7 * (po + nc)], p.tag_qt, sizeof(double) * 7 * nt);
        memcpy(&h_wh[2 * (po + nc)], p.tag_wh, sizeof(double) * 2 * nt);
        for (size_t c = 0; c < nc && cam_const; ++c)
            h_const[po + c] = cam_const[(size_t)cam_off[(size_t)i] + c] ? 1 : 0;
        for (size_t t = 0; t < nt && tag_const; ++t)
            h_const[po + nc + t] = tag_const[(size_t)tag_off[(size_t)i] + t] ? 1 : 0;
        if (p.fixed_tag >= 0)
            h_const[po + nc + (size_t)p.fixed_tag] = 1;
        // the observations by (eliminated pose, kept pose, caller's order)
        const int32_t* oe = d.elim_cams ? p.obs_cam : p.obs_tag;
        const int32_t* of = d.elim_cams ? p.obs_tag : p.obs_cam;
        order.resize((size_t)p.n_obs);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](const int32_t l, const int32_t r) {
            return oe[l] != oe[r] ? oe[l] < oe[r] : of[l] < of[r];
        });
        int32_t* es = &h_estart[(size_t)d.e_start_off];
        int32_t* fs = &h_fstart[(size_t)d.f_start_off];
        std::fill(es, es + d.n_e + 1, 0);
        std::fill(fs, fs + d.n_f + 1, 0);
        for (size_t k = 0; k < order.size(); ++k) {
            const int32_t src = order[k];
            h_obs_e[oo + k] = oe[src];
            h_obs_f[oo + k] = of[src];
            memcpy(&h_px[8 * (oo + k)], p.obs_px + 8 * (size_t)src, sizeof(double) * 8);
            es[oe[src] + 1]++;
            fs[of[src] + 1]++;
        }
        for (int32_t e = 0; e < d.n_e; ++e)
            es[e + 1] += es[e];
        for (int32_t f = 0; f < d.n_f; ++f)
            fs[f + 1] += fs[f];
        std::vector<int32_t> fill(fs, fs + d.n_f);
        for (size_t k = 0; k < order.size(); ++k)   // ascending: a kept pose's list is in the order of the eliminated poses
            h_flist[oo + (size_t)fill[(size_t)h_obs_f[oo + k]]++] = (int32_t)k;
        // the block products of the reduced system, by block of its lower block triangle: every pair (ia, ib) of observations
        // of one eliminated pose with f(ia) >= f(ib); counted, then placed, in ascending order of the eliminated pose
        const size_t nblk = (size_t)d.n_f * ((size_t)d.n_f + 1) / 2;
        int32_t* ps = &h_pstart[(size_t)d.pair_start_off];
        std::vector<int64_t> count(nblk + 1, 0);
        const int32_t* fk = h_obs_f.data() + oo;   // sorted: ascending within an eliminated pose
        for (int32_t e = 0; e < d.n_e; ++e)
            for (int32_t ib = es[e]; ib < es[e + 1]; ++ib)
                for (int32_t ia = es[e]; ia < es[e + 1]; ++ia)
                    if (fk[ia] >= fk[ib])
                        count[(size_t)fk[ia] * ((size_t)fk[ia] + 1) / 2 + (size_t)fk[ib] + 1]++;
        for (size_t u = 0; u < nblk; ++u)
            count[u + 1] += count[u];
        if (count[nblk] >= (int64_t)1 << 31)
            return bad_problem(i, "more than 2^31 block products in the reduced system");
        d.pair_off = (int64_t)(h_pairs.size() / 2);
        h_pairs.resize(h_pairs.size() + 2 * (size_t)count[nblk]);
        int32_t* pr = h_pairs.data() + 2 * (size_t)d.pair_off;
        for (size_t u = 0; u <= nblk; ++u)
            ps[u] = (int32_t)count[u];
        for (int32_t e = 0; e < d.n_e; ++e)
            for (int32_t ib = es[e]; ib < es[e + 1]; ++ib)
                for (int32_t ia = es[e]; ia < es[e + 1]; ++ia)
                    if (fk[ia] >= fk[ib]) {
                        int64_t& at = count[(size_t)fk[ia] * ((size_t)fk[ia] + 1) / 2 + (size_t)fk[ib]];
                        pr[2 * at] = ia;
                        pr[2 * at + 1] = ib;
                        ++at;
                    }
    }
    const size_t n_pair = h_pairs.size() / 2;

    // ---- the device: one allocation for the batch and its scratch ----
    static bool preloaded[64] = {};
    int rc;
    if ((rc = select_device(who, device, preloaded, { preload_small_kernels })) != VMM_BA_OK)
        return rc;
    SmallArgs a;
    memset(&a, 0, sizeof(a));
    SmallDesc* d_desc = nullptr;
    uint8_t* d_const = nullptr;
    double *d_wh = nullptr, *d_px = nullptr;
    int32_t *d_obs_e = nullptr, *d_obs_f = nullptr, *d_estart = nullptr, *d_fstart = nullptr, *d_flist = nullptr, *d_pstart = nullptr, *d_pairs = nullptr;
    auto carve = [&](Arena& ar) {
        d_desc = ar.take<SmallDesc>(np);
        a.res = ar.take<SmallResult>(np);
        a.x = ar.take<double>(7 * n_pose);
        a.cand = ar.take<double>(7 * n_pose);
        d_wh = ar.take<double>(2 * n_pose);
        d_const = ar.take<uint8_t>(n_pose);
        a.Hg = ar.take<double>(2 * kSmallPosePart * n_pose);
        a.scale = ar.take<double>(6 * n_pose);
        a.diag = ar.take<double>(6 * n_pose);
        a.D2 = ar.take<double>(6 * n_pose);
        a.delta = ar.take<double>(6 * n_pose);
        a.ysol = ar.take<double>(6 * n_pose);
        a.Le = ar.take<double>(21 * n_pose);
        a.ze = ar.take<double>(6 * n_pose);
        a.active = ar.take<int32_t>(n_pose);
        d_obs_e = ar.take<int32_t>(n_obs);
        d_obs_f = ar.take<int32_t>(n_obs);
        d_px = ar.take<double>(8 * n_obs);
        a.W = ar.take<double>(2 * 36 * n_obs);
        a.Y = ar.take<double>(36 * n_obs);
        a.opart = ar.take<double>(kSmallObsPart * n_obs);
        d_estart = ar.take<int32_t>(n_estart);
        d_fstart = ar.take<int32_t>(n_fstart);
        d_flist = ar.take<int32_t>(n_obs);
        d_pstart = ar.take<int32_t>(n_pstart);
        d_pairs = ar.take<int32_t>(2 * n_pair);
        a.trace = ar.take<vmm_ba_iteration>(n_trace);
    };
    Arena sizing;
    carve(sizing);
    const size_t bytes = sizing.used;
    Arena ar;
    if (ar.layout(carve) != hipSuccess) {
        set_error(std::string(who) + ": hipMalloc of " + std::to_string(bytes) + " bytes for the batch and its scratch: "
                  + hipGetErrorString(ar.err));
        return VMM_BA_ERR_HIP;
    }
    a.desc = d_desc;
    a.o = o;
    a.wh = d_wh;
    a.is_const = d_const;
    a.hg_stride = (int64_t)(kSmallPosePart * n_pose);
    a.w_stride = (int64_t)(36 * n_obs);
    a.obs_e = d_obs_e;
    a.obs_f = d_obs_f;
    a.px = d_px;
    a.e_start = d_estart;
    a.f_start = d_fstart;
    a.f_list = d_flist;
    a.pair_start = d_pstart;
    a.pairs = d_pairs;
    ar.copy(d_desc, desc.data(), sizeof(SmallDesc) * np, hipMemcpyHostToDevice);
    ar.copy(a.x, h_x.data(), 8 * h_x.size(), hipMemcpyHostToDevice);
    ar.copy(d_wh, h_wh.data(), 8 * h_wh.size(), hipMemcpyHostToDevice);
    ar.copy(d_const, h_const.data(), h_const.size(), hipMemcpyHostToDevice);
    ar.copy(d_estart, h_estart.data(), 4 * h_estart.size(), hipMemcpyHostToDevice);
    ar.copy(d_fstart, h_fstart.data(), 4 * h_fstart.size(), hipMemcpyHostToDevice);
    ar.copy(d_pstart, h_pstart.data(), 4 * h_pstart.size(), hipMemcpyHostToDevice);
    if (n_pair > 0)
        ar.copy(d_pairs, h_pairs.data(), 4 * h_pairs.size(), hipMemcpyHostToDevice);
    if (n_obs > 0) {
        ar.copy(d_obs_e, h_obs_e.data(), 4 * n_obs, hipMemcpyHostToDevice);
        ar.copy(d_obs_f, h_obs_f.data(), 4 * n_obs, hipMemcpyHostToDevice);
        ar.copy(d_px, h_px.data(), 8 * h_px.size(), hipMemcpyHostToDevice);
        ar.copy(d_flist, h_flist.data(), 4 * n_obs, hipMemcpyHostToDevice);
    }
    if (ar.err == hipSuccess) {
        launch_small_ba(nullptr, n_problems, a);
        ar.err = hipGetLastError();
    }
    // the blocking copies back wait for the kernel
    std::vector<SmallResult> res(np);
    std::vector<vmm_ba_iteration> h_trace(n_trace);
    ar.copy(res.data(), a.res, sizeof(SmallResult) * np, hipMemcpyDeviceToHost);
    ar.copy(h_x.data(), a.x, 8 * h_x.size(), hipMemcpyDeviceToHost);
    if (n_trace > 0)
        ar.copy(h_trace.data(), a.trace, sizeof(vmm_ba_iteration) * n_trace, hipMemcpyDeviceToHost);
    if (ar.err != hipSuccess)
        return hip_failure(who, "", ar.err);

    for (int32_t i = 0; i < n_problems; ++i) {
        const vmm_ba_problem& p = problems[i];
        const SmallDesc& d = desc[(size_t)i];
        const SmallResult& r = res[(size_t)i];
        const size_t po = (size_t)d.pose_off, nc = (size_t)p.n_cams, nt = (size_t)p.n_tags;
        memcpy(cam_qt + 7 * (size_t)cam_off[(size_t)i], &h_x[7 * po], sizeof(double) * 7 * nc);
        memcpy(tag_qt + 7 * (size_t)tag_off[(size_t)i], &h_x[7 * (po + nc)], sizeof(double) * 7 * nt);
        vmm_ba_summary& s = summaries[i];
        vmm_ba_iteration* const user_trace = s.trace;
        const int32_t user_cap = d.trace_capacity;
        memset(&s, 0, sizeof(s));
        s.trace = user_trace;
        s.trace_capacity = user_cap;
        s.termination_type = r.termination;
        s.iterations = r.records;
        s.num_successful_steps = r.num_successful;
        s.num_unsuccessful_steps = r.num_unsuccessful;
        s.num_lm_iterations = r.num_lm_iterations;
        s.num_jacobian_evals = r.num_jac_evals;
        s.num_cost_evals = r.num_cost_evals;
        s.elimination = d.elim_cams ? VMM_BA_ELIM_CAMERAS : VMM_BA_ELIM_TAGS;
        s.initial_cost = r.initial_cost;
        s.final_cost = r.final_cost;
        const int32_t rows = std::min(r.records, user_cap);
        if (rows > 0)
            memcpy(user_trace, &h_trace[(size_t)d.trace_off], sizeof(vmm_ba_iteration) * (size_t)rows);
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int32_t i = 0; i < n_problems; ++i)
        summaries[i].time_solve_s = dt;
    return VMM_BA_OK;
}

} // extern "C"
