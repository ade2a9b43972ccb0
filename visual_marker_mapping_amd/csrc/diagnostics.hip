// The diagnostics of include/vmm_ba.h: vmm_ba_time_kernels, the launch schedule of the launch-per-column factorisation
// (vmm_ba_debug_chol_schedule, vmm_ba_debug_chol_tile) and vmm_ba_debug_overlap.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "host.hpp"

namespace vmm {

// What a diagnostic creates for the length of a call: N handles of one kind, destroyed in ascending order on every way
// out -- or earlier by release(), where the order of the HIP calls matters.
template <typename T, hipError_t (*Destroy)(T), int N = 1>
struct Owned {
    T h[N] = {};
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { release(); }
    void release()
    {
        for (T& x : h) {
            if (x)
                (void)Destroy(x);
            x = nullptr;
        }
    }
};
template <int N>
using OwnedEvents = Owned<hipEvent_t, hipEventDestroy, N>;

} // namespace vmm

using namespace vmm;

extern "C" {

int vmm_ba_time_kernels(vmm_ba_handle h, const vmm_ba_options* opt, int reps, vmm_ba_kernel_times* out)
{
    if (!h || !out || reps <= 0) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.multi) {
        set_error("time_kernels is a single-GPU diagnostic");
        return VMM_BA_ERR_STATE;
    }
    vmm_ba_options o;
    if (opt)
        o = *opt;
    else
        vmm_ba_default_options(&o);
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    memset(out, 0, sizeof(*out));
    out->n_obs = e.n_obs;
    out->reduced_dim = e.n_red;
    out->elim_dim = e.k_dim;
    out->schur_sparse = e.sparse_schur ? 1 : 0;
    out->syrk_wide = (!e.sparse_schur && e.syrk.wide) ? 1 : 0;
    out->schur_flops = e.schur_flops;
    out->chol_flops = e.chol_nz_on ? e.chol_flops : 0.0;
    // keep the caller's state: timing runs real iterations.  The RAW device buffers are saved and restored: through
    // vmm_ba_get_state / vmm_ba_set_state a point-landmark handle would get its tags back as exact rectangles rebuilt
    // from re-orthogonalised poses, not the optimised free corners it held.
    std::vector<double> cam0((size_t)7 * e.n_cams), tag0((size_t)7 * e.n_tags);
    HIP_TRY(hipMemcpyAsync(cam0.data(), e.cam_qt, sizeof(double) * cam0.size(), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipMemcpyAsync(tag0.data(), e.tag_qt, sizeof(double) * tag0.size(), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    auto restore_raw = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(e.cam_qt, cam0.data(), sizeof(double) * cam0.size(), hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipMemcpyAsync(e.tag_qt, tag0.data(), sizeof(double) * tag0.size(), hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipStreamSynchronize(e.stream));
        e.dirty_cam = e.dirty_tag = false;
        return VMM_BA_OK;
    };
    if (e.trace_capacity < 1) {
        if ((rc = dev_alloc(e, &e.trace, 1, false))) return rc;
        e.trace_capacity = 1;
        drop_graphs(e);
    }
    vmm_ba_options ot = o;
    ot.max_num_iterations = 1 << 30;
    ot.function_tolerance = 0.0;
    ot.parameter_tolerance = 0.0;
    ot.gradient_tolerance = 0.0;
    if ((rc = begin_lm_loop(e, ot, 0))) return rc;
    if ((rc = enqueue_iteration(e, ot))) return rc;   // populates every buffer of an iteration
    HIP_TRY(hipStreamSynchronize(e.stream));
    // the priming step was accepted and moved x; go back so that the W recomputed by the timed
    // evaluation passes stays consistent with the H blocks of the priming evaluation
    if ((rc = restore_raw())) return rc;   // the timed pieces read the poses on the device
    OwnedEvents<2> events;
    hipEvent_t &ev0 = events.h[0], &ev1 = events.h[1];
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    // each timed piece is captured into a hipGraph once and replayed, so that the gaps between its
    // launches are the ones the production iteration graph sees
    // `inner` > 1 (idempotent pieces only): the piece is captured that many times back to back and the
    // graph time divided by it, which takes the ~9 us of graph-launch overhead out of a 5-30 us kernel
    // (rocprofv3's per-kernel durations are the reference the bench line must agree with).
    auto timed = [&](auto&& fn, auto&& prep, double* ms_out, int inner = 1) -> int {
        Owned<hipGraph_t, hipGraphDestroy> graph;
        Owned<hipGraphExec_t, hipGraphExecDestroy> exec;
        hipGraph_t& g = graph.h[0];
        hipGraphExec_t& ge = exec.h[0];
        HIP_TRY(hipStreamBeginCapture(e.stream, hipStreamCaptureModeThreadLocal));
        for (int q = 0; q < inner; ++q)
            fn();
        HIP_TRY(hipStreamEndCapture(e.stream, &g));
        HIP_TRY(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        graph.release();
        double total = 0.0;
        for (int r = 0; r < reps + 1; ++r) {   // replay 0 is untimed
            prep();
            HIP_TRY(hipEventRecord(ev0, e.stream));
            HIP_TRY(hipGraphLaunch(ge, e.stream));
            HIP_TRY(hipEventRecord(ev1, e.stream));
            HIP_TRY(hipEventSynchronize(ev1));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
            if (r > 0) total += ms;
        }
        exec.release();
        *ms_out = total / reps / inner;
        return VMM_BA_OK;
    };
    auto nop = [] {};
    // the guards read ctl->done / lin_fail only; both are 0 after the priming iteration unless it failed
    HIP_TRY(hipMemcpy(e.ctl_host, e.ctl, sizeof(LmCtl), hipMemcpyDeviceToHost));
    e.ctl_host->done = 0;
    e.ctl_host->lin_fail = 0;
    HIP_TRY(hipMemcpy(e.ctl, e.ctl_host, sizeof(LmCtl), hipMemcpyHostToDevice));
    if ((rc = timed([&] { launch_eval_passes(e, o.robustify, o.huber_a, false); }, nop, &out->eval_elim_ms, 8))) return rc;
    out->eval_keep_ms = 0.0;
    if ((rc = timed([&] { launch_cost_kernel(e, e.cam_qt, e.tag_qt, false, o.robustify, o.huber_a); }, nop, &out->cost_ms, 8))) return rc;
    if ((rc = timed([&] { launch_elim(e); }, nop, &out->form_z_ms, 8))) return rc;
    if ((rc = timed([&] { launch_syrk_only(e); }, nop, &out->syrk_ms, 4))) return rc;
    if ((rc = timed([&] { launch_cholesky_solve(e, e.S, e.n_pad, e.ldz, e.yf, e.ctl); },
                    [&] {
                        launch_syrk_reduced(e);
                        launch_pack_lower(e, false);   // world > 1: this rank's share alone (no all-reduce here)
                        launch_pack_lower(e, true);
                    },
                    &out->cholesky_ms)))
        return rc;
    if ((rc = timed([&] { launch_backsub(e); }, nop, &out->backsub_ms, 8))) return rc;
    if (e.sw.debug) {
        HIP_TRY(hipMemcpy(e.ctl_host, e.ctl, sizeof(LmCtl), hipMemcpyDeviceToHost));
        fprintf(stderr, "[vmm_ba debug] after kernel timing: done=%d lin_fail=%d termination=%d iteration=%d\n",
                e.ctl_host->done, e.ctl_host->lin_fail, e.ctl_host->termination, e.ctl_host->iteration);
    }
    // whole iterations from the caller's state
    if ((rc = restore_raw())) return rc;
    if ((rc = begin_lm_loop(e, ot, 0))) return rc;
    HIP_TRY(hipEventRecord(ev0, e.stream));
    int passes = 0;
    for (int r = 0; r < reps; ++r) {
        if ((rc = run_iteration(e, ot))) return rc;
        passes += e.last_passes;
    }
    HIP_TRY(hipEventRecord(ev1, e.stream));
    HIP_TRY(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    out->lm_iteration_ms = ms / passes;
    events.release();
    return restore_raw();
}

int vmm_ba_debug_chol_schedule(int n_blk, int n_df, int n_cu, int32_t* launches, int cap, int* n_launches, int* n_df_used)
{
    if (n_blk < 1 || n_cu < 1 || cap < 0 || (cap > 0 && !launches) || !n_launches || (n_df > 0 && n_df > n_blk - 2)) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    if (n_df < 0) {
        n_df = dataflow_blocks(n_blk, n_cu, read_switches());
        if (n_df == n_blk)
            n_df = 0;   // the one-launch kernel takes the whole system: what is returned is the fallback schedule
    }
    const std::vector<CholLaunch> sched = chol_step_schedule(n_blk, n_df);
    for (size_t i = 0; i < sched.size() && (int)i < cap; ++i) {
        const CholLaunch& L = sched[i];
        const int32_t row[8] = { L.k, L.lazy[0], L.lazy[1], L.upd[0], L.upd[1], L.c0, L.t0, L.t1 };
        memcpy(launches + 8 * i, row, sizeof(row));
    }
    *n_launches = (int)sched.size();
    if (n_df_used)
        *n_df_used = n_df;
    return VMM_BA_OK;
}

int vmm_ba_debug_chol_tile(int n_blk, const int32_t* launch, int t, int* bi, int* bj)
{
    if (!launch || !bi || !bj || t < 0 || t >= launch[7]) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    const CholLaunch L = { launch[0], { launch[1], launch[2] }, { launch[3], launch[4] }, launch[5], launch[6], launch[7] };
    chol_schedule_tile(n_blk, L, t, bi, bj);
    return VMM_BA_OK;
}

// Diagnostic behind DESIGN.md's question "can the reduced-system assembly hide behind the factorisation?": times, with
// HIP events, (0) rank-k update + partial-tile sum alone, (1) factorisation + triangular solves alone, (2) both back to
// back on one stream (today's order), (3) both at once on two streams -- the factorisation on a valid S, the rank-k
// update of the same Z writing its sum into a scratch matrix, so that only the sharing of the chip is measured, not a
// dependency; (4) the factorisation's own duration inside (3).  Dense elimination, one GPU.  ms[5] averages over reps.
int vmm_ba_debug_overlap(vmm_ba_handle h, int reps, double* ms)
{
    if (!h || !ms || reps <= 0) {
        set_error("bad argument");
        return VMM_BA_ERR_ARGUMENT;
    }
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.multi || e.sparse_schur || !e.Z) {
        set_error("debug_overlap needs a single-GPU handle on the dense elimination path");
        return VMM_BA_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(e.device));
    int rc;
    if ((rc = flush_state(e))) return rc;
    vmm_ba_options o;
    vmm_ba_default_options(&o);
    o.max_num_iterations = 1 << 30;
    o.function_tolerance = o.parameter_tolerance = o.gradient_tolerance = 0.0;
    if (e.trace_capacity < 1) {
        if ((rc = dev_alloc(e, &e.trace, 1, false))) return rc;
        e.trace_capacity = 1;
        drop_graphs(e);
    }
    if ((rc = begin_lm_loop(e, o, 0))) return rc;
    if ((rc = enqueue_iteration(e, o))) return rc;   // populates Z, the small blocks and the control block
    HIP_TRY(hipStreamSynchronize(e.stream));
    Arena scratch;   // S2
    Owned<hipStream_t, hipStreamDestroy> second;
    OwnedEvents<5> events;
    hipStream_t& sb = second.h[0];
    hipEvent_t(&ev)[5] = events.h;
    hipError_t err = scratch.alloc(sizeof(double) * (size_t)e.ldz * e.ldz);
    double* const S2 = reinterpret_cast<double*>(scratch.base);
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&sb, hipStreamNonBlocking);
    for (int i = 0; i < 5 && err == hipSuccess; ++i)
        err = hipEventCreate(&ev[i]);
    auto reset_flags = [&]() -> hipError_t {
        hipError_t r = hipMemcpy(e.ctl_host, e.ctl, sizeof(LmCtl), hipMemcpyDeviceToHost);
        if (r != hipSuccess) return r;
        e.ctl_host->done = 0;
        e.ctl_host->lin_fail = 0;
        e.ctl_host->sync_timeout = 0;
        return hipMemcpy(e.ctl, e.ctl_host, sizeof(LmCtl), hipMemcpyHostToDevice);
    };
    double acc[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int r = 0; r < reps + 1 && err == hipSuccess; ++r) {   // repetition 0 is untimed
        float t[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        // (0) rank-k update + sum (leaves a valid S), (1) factorisation + solves
        if ((err = reset_flags()) != hipSuccess) break;
        (void)hipEventRecord(ev[0], e.stream);
        launch_syrk_reduced(e);
        (void)hipEventRecord(ev[1], e.stream);
        launch_cholesky_solve(e, e.S, e.n_pad, e.ldz, e.yf, e.ctl);
        (void)hipEventRecord(ev[2], e.stream);
        if ((err = hipEventSynchronize(ev[2])) != hipSuccess) break;
        (void)hipEventElapsedTime(&t[0], ev[0], ev[1]);
        (void)hipEventElapsedTime(&t[1], ev[1], ev[2]);
        (void)hipEventElapsedTime(&t[2], ev[0], ev[2]);
        // (3) both at once: S rebuilt first (untimed), then the factorisation beside a second rank-k update into S2
        if ((err = reset_flags()) != hipSuccess) break;
        launch_syrk_reduced(e);
        if ((err = hipStreamSynchronize(e.stream)) != hipSuccess) break;
        // the factorisation is enqueued first: its workgroups (84 KB of LDS, one per CU) take their CUs, the rank-k
        // update's (72 KB) fill what is left beside them
        (void)hipEventRecord(ev[0], e.stream);
        (void)hipStreamWaitEvent(sb, ev[0], 0);
        launch_cholesky_solve(e, e.S, e.n_pad, e.ldz, e.yf, e.ctl);
        (void)hipEventRecord(ev[3], e.stream);
        launch_syrk_plan(sb, e.ctl, e.Z, e.ldz, e.syrk);
        launch_reduce_plan(sb, e.ctl, e.syrk, e.ldz, e.n_pad + 1, S2);
        (void)hipEventRecord(ev[1], sb);
        (void)hipStreamWaitEvent(e.stream, ev[1], 0);
        (void)hipEventRecord(ev[2], e.stream);
        if ((err = hipEventSynchronize(ev[2])) != hipSuccess) break;
        (void)hipEventElapsedTime(&t[3], ev[0], ev[2]);
        (void)hipEventElapsedTime(&t[4], ev[0], ev[3]);
        (void)hipEventElapsedTime(&t[5], ev[0], ev[1]);
        // (6) the same with the rank-k update enqueued FIRST (its 495 workgroups take their slots, the factorisation's
        // workgroups follow as slots fall free)
        if ((err = reset_flags()) != hipSuccess) break;
        launch_syrk_reduced(e);
        if ((err = hipStreamSynchronize(e.stream)) != hipSuccess) break;
        (void)hipEventRecord(ev[0], e.stream);
        (void)hipStreamWaitEvent(sb, ev[0], 0);
        launch_syrk_plan(sb, e.ctl, e.Z, e.ldz, e.syrk);
        launch_reduce_plan(sb, e.ctl, e.syrk, e.ldz, e.n_pad + 1, S2);
        (void)hipEventRecord(ev[1], sb);
        (void)hipEventRecord(ev[4], e.stream);
        launch_cholesky_solve(e, e.S, e.n_pad, e.ldz, e.yf, e.ctl);
        (void)hipEventRecord(ev[3], e.stream);
        (void)hipStreamWaitEvent(e.stream, ev[1], 0);
        (void)hipEventRecord(ev[2], e.stream);
        if ((err = hipEventSynchronize(ev[2])) != hipSuccess) break;
        (void)hipEventElapsedTime(&t[6], ev[0], ev[2]);
        (void)hipEventElapsedTime(&t[7], ev[4], ev[3]);
        if (r > 0)
            for (int i = 0; i < 8; ++i)
                acc[i] += t[i];
    }
    if (err == hipSuccess)
        err = hipGetLastError();
    events.release();
    second.release();
    if (err != hipSuccess) {
        set_error(std::string("debug_overlap: ") + hipGetErrorString(err));
        return VMM_BA_ERR_HIP;
    }
    for (int i = 0; i < 8; ++i)
        ms[i] = acc[i] / reps;
    return VMM_BA_OK;
}

} // extern "C"
