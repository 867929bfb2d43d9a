// csrc/solve_plan.h -- launch form and scratch layout of the fused solver, stated once (host only).
// os_solve_impl (api_solve.hip) follows the plan; sosgpu_debug_solve_plan reports it.  Nothing here calls HIP, reads the environment
// or touches a context: the plan is a function of the problem shape and of the overrides api_solve.hip has read.  The kernel variant
// in it is solve_variant's (solve_variant.h), which the launchers follow.
#pragma once
#include "solve_variant.h"
#include <algorithm>

// output slots (sosgpu_os_solve_levels): lane-private state per work region, [nz][SOS_LV_N][threads] doubles, placed behind
// the streamed kernel's regions at a 64-byte boundary
inline size_t lv_stride(int nz, int threads) { return (size_t)nz * SOS_LV_N * threads; }
inline size_t lv_off(size_t doubles) { return (doubles + 7) & ~(size_t)7; }

// scratch budget in doubles: 64 GiB of the 288 GB (a launch covers ~40 000 bins at 608 levels)
inline size_t solve_scratch_cap(const SolveOverrides &ov)
{
    const size_t gib = ov.scratch_gib > 0 ? (size_t)ov.scratch_gib : 64;
    return (gib << 30) / sizeof(double);
}

// Few bins (a band of one wavelength): the order-parallel form -- up to 48 Fourier orders of every bin at a time, each in a
// work region of its own, so that the band fills ~1024 workgroup slots (sos_stream.hip).  A single bin takes 11 ms as one
// workgroup, ~1.5 ms this way.  Used up to 128 bins per call; an explicitly chosen other form wins.
inline int solve_spec_max_bins(const SolveOverrides &ov)
{
    int spec_max = 128;
    if (ov.spec_off) spec_max = 0;
    if (ov.has_spec_maxbins) spec_max = ov.spec_maxbins;
    if (ov.persist != 0) spec_max = 0;
    if (ov.orders_per_launch > 0) spec_max = 0;
    return spec_max;
}

// Whether the plan needs the largest valid NT of the batch (solve_plan's nt_max): the order-parallel form is a candidate.  The
// few NT then come to the host -- one small copy behind the work already queued on the stream, which this latency-bound form
// has to wait for anyway.
inline bool solve_plan_needs_nt(const SolveShape &sh, const SolveOverrides &ov)
{
    SolvePlan v;
    if (solve_variant(sh, ov, &v) != 0 || !v.big) return false;
    return !sh.table && sh.nb <= solve_spec_max_bins(ov) && sh.smax >= 1;
}

// The plan of one solve.  nt_max: the largest valid NT of the batch, read only when solve_plan_needs_nt().  Returns 0 or the
// code of solve_variant.  Scratch layout (doubles from the start of the context's scratch, each block from the end of the
// one before it):
//   work regions [regions][per_bin] | I3 hand-over block of the order-parallel form | task queues and per-bin order flags of
//   the persistent form (ints) | lane-private state of the output slots [regions][slot_stride], from a 64-byte boundary
inline int solve_plan(const SolveShape &sh, const SolveOverrides &ov, int nt_max, SolvePlan *out)
{
    SolvePlan p = SolvePlan();
    // variant: field in LDS, or (too many levels) field in a per-bin HBM scratch, launched in sub-batches so that the scratch
    // stays below its budget
    const int rc = solve_variant(sh, ov, &p);
    if (rc) return rc;
    const int s1n = sh.smax + 1;
    p.q_tail = ov.q_tail;
    p.lpb = sos_round_up(sh.lp, 32);
    if (!p.big) {
        // LDS-resident kernel: no scratch but the output slots' state, one region per bin
        p.form = SOSGPU_FORM_LDS;
        p.per_launch = sh.nb;
        p.regions = (size_t)sh.nb;
        p.slot_stride = lv_stride(sh.nz, p.threads);
        p.need = p.slot_stride * p.regions;
        *out = p;
        return 0;
    }
    p.slot_stride = lv_stride(sh.nz, p.threads);
    p.per_bin = stream_scratch_doubles(p.nw, p.kht, p.lpb);
    const size_t cap = solve_scratch_cap(ov);
    // (output slots: a bin's work region also carries the slots' lane-private state)
    p.per_launch = (int)std::min<size_t>((size_t)sh.nb, std::max<size_t>(1, cap / (p.per_bin + p.slot_stride)));
    p.needs_nt = solve_plan_needs_nt(sh, ov);
    if (p.needs_nt) {
        // first round: 48 orders (a series typically ends after 25-50 of its up to 81), 24 above 40 bins; later rounds run
        // half as many.  Measured (profiles/r02_sos_proc_latency.txt): the number of rounds is what costs, not the tasks
        // beyond the chip's 512 workgroup slots.
        p.spec_k = std::min(s1n, sh.nb <= 40 ? 48 : 24);
        // The work regions are laid out for the batch's own level count, not for the padded row length `lp` of the caller
        // (608 for profiles made by sosgpu_profile).  per_launch keeps the value of the unshrunk region.
        const int lpb_full = p.lpb;
        const size_t per_bin_full = p.per_bin;
        p.lpb = std::min(p.lpb, sos_round_up(std::max(1, nt_max) + 1, 32));
        p.per_bin = stream_scratch_doubles(p.nw, p.kht, p.lpb);
        // at most 4 GiB of work regions (128 bins x 24 orders at 600 levels need 4.6): beyond, fewer orders per round
        const size_t soft = ((size_t)4 << 30) / sizeof(double);
        const size_t fit = soft / ((size_t)sh.nb * p.per_bin);
        if (fit < (size_t)p.spec_k) p.spec_k = std::max(std::min(p.spec_k, 8), (int)fit);
        if (ov.has_spec_k) p.spec_k = std::min(s1n, std::max(1, ov.spec_k));   // (tests)
        if ((size_t)sh.nb * p.spec_k * p.per_bin > cap) p.spec_k = 0;
        if (!p.spec_k) { p.lpb = lpb_full; p.per_bin = per_bin_full; }
    }
    if (p.spec_k) p.form = SOSGPU_FORM_SPEC;
    else {
        // The streamed kernel can run `opl` Fourier orders of every bin per launch (order-synchronous launches: every
        // workgroup then streams the same source operator).  Measured on the realistic mix (profiles/r02_stream_experiments.txt):
        // 1 order per launch 21.1k bins/s, all orders in one launch 21.9k -- the operator stream is not what binds, so one
        // launch is the default for large batches; SOSGPU_STREAM_ORDERS_PER_LAUNCH = n selects n orders per launch (tests cover both).
        p.opl = ov.orders_per_launch > 0 ? ov.orders_per_launch : s1n;
        // SOSGPU_STREAM_PERSIST=1: ONE persistent launch whose workgroups take (Fourier order, bin) tasks from per-XCD queues,
        // so that the workgroups of an XCD share the source operators of one or two orders in L2 (sos_stream.hip, PERSIST).
        // Measured on the realistic mix (profiles/r02_stream_experiments.txt): fabric reads 505 -> 317 GB per launch (the
        // operator misses are gone), 22.2 k against 22.6 k bins/s -- the kernel is not bound by that traffic, so one
        // workgroup per bin stays the default.  Launches with a context table always use the default form, and so do output
        // slots (the plain launch).
        const bool persist = ov.persist != 0 && !sh.table && p.opl == s1n && sh.nz == 0;
        p.form = persist ? SOSGPU_FORM_PERSIST : SOSGPU_FORM_STREAM;
    }
    p.regions = p.spec_k ? (size_t)sh.nb * p.spec_k : (size_t)p.per_launch;
    p.off_i3 = p.per_bin * p.regions;
    p.i3_doubles = p.spec_k ? (size_t)sh.nb * s1n * p.threads : 0;
    p.off_queue = p.off_i3 + p.i3_doubles;
    p.queue_doubles = (256 + (size_t)p.per_launch) / 2 + 1;     // 256 queue ints + a flag per bin, budgeted in every form
    p.need = p.off_queue + p.queue_doubles;
    if (sh.nz > 0) {
        p.off_slots = lv_off(p.need);
        p.need = p.off_slots + p.slot_stride * p.regions;
    }
    *out = p;
    return 0;
}
