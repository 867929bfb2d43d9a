// csrc/api_solve.hip -- the solver dispatch: os_solve_impl follows the plan of solve_plan.h and queues the launches of
// sos_os.hip / sos_stream.hip; on it stand the four solve entry points, the output levels, the diffuse transmissions and the
// spherical albedo (one order-0 solve per spectrum), the solve's timing and flop count, and the solver's diagnostics.
#include "api_internal.h"
#include "solve_plan.h"
#include <algorithm>
#include <climits>
#include <cstdlib>

using namespace sosgpu_internal;

// the solver's environment switches, read once per solve (not cached: a process may change them between solves)
static SolveOverrides read_solve_overrides()
{
    SolveOverrides ov;
    if (const char *e = getenv("SOSGPU_SCRATCH_GIB")) ov.scratch_gib = atol(e);
    if (const char *e = getenv("SOSGPU_STREAM_SPEC")) ov.spec_off = atoi(e) == 0;
    if (const char *e = getenv("SOSGPU_STREAM_SPEC_MAXBINS")) { ov.has_spec_maxbins = true; ov.spec_maxbins = atoi(e); }
    if (const char *e = getenv("SOSGPU_STREAM_SPEC_K")) { ov.has_spec_k = true; ov.spec_k = atoi(e); }
    if (const char *e = getenv("SOSGPU_STREAM_PERSIST")) ov.persist = atoi(e);
    if (const char *e = getenv("SOSGPU_STREAM_ORDERS_PER_LAUNCH")) ov.orders_per_launch = atoi(e);
    if (const char *e = getenv("SOSGPU_STREAM_QTAIL")) ov.q_tail = atoi(e);
    return ov;
}

// The context's scratch holds at least `need` doubles afterwards (grow-only; taken from / handed back to the scratch pool, api_mem.hip).
// (The scratch is reused from solve to solve and from context to context without being cleared: the streamed kernel
//  initialises what it reads; the pad levels and pad columns it stages along with a chunk feed columns / rows of the
//  contraction that are never stored.)
static int ensure_scratch(sosgpu_ctx *cx, size_t need)
{
    if (need <= cx->scratch_doubles) return SOSGPU_OK;
    if (cx->scratch) {
        HIPCHK(sync_ctx_streams(cx));   // an earlier solve of this context may still be using it, on any of its streams
        pool_give(cx->device, cx->scratch, cx->scratch_doubles);
    }
    cx->scratch = nullptr;
    cx->scratch_doubles = 0;
    size_t got = 0;
    cx->scratch = pool_take(cx->device, need, &got);
    if (!cx->scratch) { g_last_hip = (int)hipGetLastError(); return SOSGPU_E_HIP; }
    cx->scratch_doubles = got;
    return SOSGPU_OK;
}

// sosgpu_os_solve (table == null) and sosgpu_os_solve_multi (per-bin contexts from a device table)
// nz > 0: sosgpu_os_solve_levels / sosgpu_os_solve_multi_levels (d_jout / d_zz / d_rec hold nz slots; a split batch reads
// slot k of its bins at k nb + b0 -- bn.zbs is the whole batch's bin count)
// Kernel variant, launch form, bins per launch and every scratch offset come from solve_plan (solve_plan.h); every launch takes `pl`.
static int os_solve_impl(sosgpu_ctx *cx, const SosDev *table, const int32_t *d_ctx_of_bin, const int32_t *d_order, int nb, int lp, const int32_t *d_nt,
                         const int32_t *d_iborm, const double *d_prof, const int32_t *d_jout, const double *d_zz,
                         double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux, void *stream, int nz = 0,
                         const SosDev *as = nullptr, long scratch_gib = 0)
{
    if (!cx || nb < 0 || lp < 2 || !d_nt || !d_iborm || !d_prof || !d_rec || !d_norders || !d_iglast || !d_flux)
        return SOSGPU_E_ARG;
    if ((d_jout == nullptr) != (d_zz == nullptr)) return SOSGPU_E_ARG;
    // `as`: what the entries of `table` have in common where that is not cx's own description (sosgpu_trans_spectrum: order 0
    // only, no surface); it selects the variant and the record layout, cx still lends its scratch, events and stream list
    const SosDev &dv = as ? *as : cx->d;
    if (dv.imat_surf && !dv.mp_gnd) return SOSGPU_E_ARG;
    if (nb == 0) return SOSGPU_OK;
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t st = (hipStream_t)stream;
    const SolveShape sh = {dv.n, dv.smax, nb, lp, nz, table != nullptr};
    SolveOverrides ov = read_solve_overrides();
    if (ov.scratch_gib <= 0) ov.scratch_gib = scratch_gib;      // (0: the plan's default budget)
    int ntm = 1;
    if (solve_plan_needs_nt(sh, ov)) {
        std::vector<int32_t> h_nt((size_t)nb);
        HIPCHK(hipMemcpyAsync(h_nt.data(), d_nt, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int b = 0; b < nb; b++) if (h_nt[b] < lp) ntm = std::max(ntm, (int)h_nt[b]);    // (malformed bins are flagged by the kernel)
    }
    SolvePlan pl;
    int rc = solve_plan(sh, ov, ntm, &pl);
    if (rc) return rc;
    if ((rc = ensure_scratch(cx, pl.need))) return rc;
    if (!cx->ev0) { HIPCHK(hipEventCreate(&cx->ev0)); }
    if (!cx->ev1) { HIPCHK(hipEventCreate(&cx->ev1)); }
    HIPCHK(hipEventRecord(cx->ev0, st));
    const int S1 = dv.smax + 1, W = dv.w;
    const int nt_max = lp - 1;          // lp - 1 bounds every NT of the batch (the host pads the level axis to lp)
    for (int b0 = 0; b0 < nb; b0 += pl.per_launch) {
        SosBins bn;
        bn.nb = std::min(pl.per_launch, nb - b0); bn.lp = lp;
        bn.nt = d_nt + b0; bn.iborm = d_iborm + b0; bn.jout = d_jout ? d_jout + b0 : nullptr;
        bn.prof = d_prof + (size_t)b0 * 3 * lp; bn.zz = d_zz ? d_zz + b0 : nullptr;
        bn.rec = d_rec + (size_t)b0 * S1 * 3 * W; bn.flux = d_flux + (size_t)2 * b0;
        bn.norders = d_norders + b0; bn.iglast = d_iglast + (size_t)b0 * S1;
        bn.scratch = pl.big ? cx->scratch : nullptr; bn.scr_stride = pl.per_bin; bn.lpb = pl.lpb;
        bn.phase = cx->phase ? cx->phase + (size_t)b0 * 8 : nullptr;
        bn.ctxs = table; bn.ctx_of_bin = table ? d_ctx_of_bin + b0 : nullptr;
        bn.order = (table && pl.per_launch >= nb) ? d_order : nullptr;      // (a split batch keeps its given order)
        bn.queue = bn.qflag = nullptr; bn.q_tail = pl.q_tail;
        bn.spec_k = 0; bn.spec_i3 = nullptr;
        bn.s_begin = 0; bn.s_end = S1;
        bn.nz = nz; bn.zbs = nb; bn.zrs = (size_t)nb * S1 * 3 * W;
        bn.zst = nz > 0 ? cx->scratch + pl.off_slots : nullptr; bn.zst_stride = nz > 0 ? pl.slot_stride : 0;
        if (pl.form == SOSGPU_FORM_SPEC) {
            // order-parallel form: set-up launch, then rounds of (K order tasks per bin, replay of their stop tests)
            bn.spec_i3 = cx->scratch + pl.off_i3;
            cx->dbg_spec_i3 = pl.off_i3;
            const int nt_max_r = pl.lpb - 1;           // level capacity of the regions (>= every valid NT of the batch)
            bn.spec_k = -pl.spec_k; bn.s_begin = 0; bn.s_end = 0;
            rc = launch_sos_stream(dv, bn, pl, nt_max_r, st, &g_last_hip);
            bn.spec_k = pl.spec_k;
            // (a series typically ends after 25-50 of its up to 81 orders: 32 + 16 + ... wastes less than all at once, and a
            //  launch whose bins have all stopped costs a few microseconds)
            for (int s0 = 0, kr = pl.spec_k; s0 < S1 && rc == 0; s0 += kr, kr = std::max(1, pl.spec_k / 2)) {
                bn.s_begin = s0; bn.s_end = std::min(S1, s0 + kr);
                rc = launch_sos_stream(dv, bn, pl, nt_max_r, st, &g_last_hip);
                if (rc == 0) rc = launch_sos_stream_replay(dv, bn, pl, bn.s_begin, bn.s_end, st, &g_last_hip);
            }
        } else if (pl.big) {
            if (pl.form == SOSGPU_FORM_PERSIST) {
                bn.queue = reinterpret_cast<int *>(cx->scratch + pl.off_queue);
                bn.qflag = bn.queue + 256;
                HIPCHK(hipMemsetAsync(bn.queue, 0, (256 + (size_t)bn.nb) * sizeof(int), st));
            }
            for (int s0 = 0; s0 < S1 && rc == 0; s0 += pl.opl) {
                bn.s_begin = s0; bn.s_end = std::min(S1, s0 + pl.opl);
                rc = table ? launch_sos_stream_multi(dv, bn, pl, nt_max, st, &g_last_hip)
                           : launch_sos_stream(dv, bn, pl, nt_max, st, &g_last_hip);
            }
        } else rc = table ? launch_sos_os_multi(dv, bn, pl, st, &g_last_hip)
                          : launch_sos_os(dv, bn, pl, st, &g_last_hip);
        if (rc == -2) return SOSGPU_E_HIP;
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(cx->ev1, st));
    cx->timed = true;
    note_stream(cx, st);
    return SOSGPU_OK;
}

extern "C" int sosgpu_os_solve(sosgpu_ctx *cx, int nb, int lp, const int32_t *d_nt, const int32_t *d_iborm,
                               const double *d_prof, const int32_t *d_jout, const double *d_zz,
                               double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux, void *stream)
{
    return os_solve_impl(cx, nullptr, nullptr, nullptr, nb, lp, d_nt, d_iborm, d_prof, d_jout, d_zz, d_rec, d_norders, d_iglast,
                         d_flux, stream);
}

extern "C" int sosgpu_os_solve_levels(sosgpu_ctx *cx, int nb, int lp, const int32_t *d_nt, const int32_t *d_iborm,
                                      const double *d_prof, int nz, const int32_t *d_jout, const double *d_zz,
                                      double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux, void *stream)
{
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS || !d_jout || !d_zz) return SOSGPU_E_ARG;
    return os_solve_impl(cx, nullptr, nullptr, nullptr, nb, lp, d_nt, d_iborm, d_prof, d_jout, d_zz, d_rec, d_norders, d_iglast,
                         d_flux, stream, nz);
}

extern "C" int sosgpu_output_levels(sosgpu_ctx *cx, int nb, int lp, const double *d_prof, const double *d_zprof, const int32_t *d_nt,
                                    int nz, const double *zout, int32_t *d_jout, double *d_zz, double *d_tauout, void *stream)
{
    if (!cx || nb < 0 || lp < 2 || !d_prof || !d_zprof || !d_nt || !zout || !d_jout || !d_zz || !d_tauout) return SOSGPU_E_ARG;
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS) return SOSGPU_E_ARG;
    if (nb == 0) return SOSGPU_OK;
    HIPCHK(hipSetDevice(cx->device));
    OutputLevelArgs a;
    a.nb = nb; a.lp = lp; a.nz = nz;
    for (int k = 0; k < SOSGPU_MAX_OUTPUT_LEVELS; k++) a.zout[k] = k < nz ? zout[k] : -1.0;
    a.prof = d_prof; a.zprof = d_zprof; a.nt = d_nt; a.jout = d_jout; a.zz = d_zz; a.tauout = d_tauout;
    launch_output_levels(a, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    note_stream(cx, (hipStream_t)stream);
    return SOSGPU_OK;
}

extern "C" int sosgpu_output_depths(int device, int nb, int lp, const double *d_h, size_t h_stride, const double *d_zprof,
                                    const int32_t *d_nt, int nz, const double *zout, double *d_tau, void *stream)
{
    if (nb < 0 || lp < 2 || !d_h || h_stride < (size_t)lp || !d_zprof || !d_nt || !zout || !d_tau) return SOSGPU_E_ARG;
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS) return SOSGPU_E_ARG;
    if (nb == 0) return SOSGPU_OK;
    if (const int rc = use_device(device)) return rc;
    OutputDepthArgs a;
    a.nb = nb; a.lp = lp; a.nz = nz; a.h_stride = h_stride;
    for (int k = 0; k < SOSGPU_MAX_OUTPUT_LEVELS; k++) a.zout[k] = k < nz ? zout[k] : -1.0;
    a.h = d_h; a.zprof = d_zprof; a.nt = d_nt; a.tau = d_tau;
    launch_output_depths(a, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_os_solve_multi(sosgpu_ctx *cx, const void *d_table, const int32_t *d_ctx_of_bin, const int32_t *d_order,
                                     int nb, int lp,
                                     const int32_t *d_nt, const int32_t *d_iborm, const double *d_prof, const int32_t *d_jout,
                                     const double *d_zz, double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux,
                                     void *stream)
{
    if (!d_table || !d_ctx_of_bin) return SOSGPU_E_ARG;
    return os_solve_impl(cx, static_cast<const SosDev *>(d_table), d_ctx_of_bin, d_order, nb, lp, d_nt, d_iborm, d_prof, d_jout,
                         d_zz, d_rec, d_norders, d_iglast, d_flux, stream);
}

extern "C" int sosgpu_os_solve_multi_levels(sosgpu_ctx *cx, const void *d_table, const int32_t *d_ctx_of_bin, const int32_t *d_order,
                                            int nb, int lp, const int32_t *d_nt, const int32_t *d_iborm, const double *d_prof,
                                            int nz, const int32_t *d_jout, const double *d_zz, double *d_rec, int32_t *d_norders,
                                            int32_t *d_iglast, double *d_flux, void *stream)
{
    if (!d_table || !d_ctx_of_bin) return SOSGPU_E_ARG;
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS || !d_jout || !d_zz) return SOSGPU_E_ARG;
    return os_solve_impl(cx, static_cast<const SosDev *>(d_table), d_ctx_of_bin, d_order, nb, lp, d_nt, d_iborm, d_prof, d_jout,
                         d_zz, d_rec, d_norders, d_iglast, d_flux, stream, nz);
}

// Diffuse transmissions of -SOS.Trans for the bins of many wavelengths (SOS.F:600-635): every (context, direction) pair becomes
// a child entry of a context table in the work area, every (bin, direction) pair an item of ONE order-0 multi-wavelength solve
// (trans.hip).  The spherical albedo (sosgpu_albedo_spectrum, albedo.hip) is the same stage with items of its own and the other
// flux kept.  Work area, from its first 256-byte boundary, every block at a multiple of 256 bytes:
//   parents [nctx] SosDev | children [nctx N] SosDev | sv [nctx N][4][kp] | ctx_of_item, nt, iborm, norders, iglast [nb N] int32
//   | flux [nb N][2] | rec [nb N][3][W] | prof [nb N][3][lp]
namespace {
struct TransLayout { size_t parents, children, sv, ctx_of_item, nt, iborm, norders, iglast, flux, rec, prof, total; };

bool trans_layout(int n, int kp, int nctx, int nb, int lp, TransLayout *out)
{
    if (n < 1 || nctx < 1 || nb < 0 || lp < 2) return false;
    const size_t nchild = (size_t)nctx * n, nitems = (size_t)nb * n;
    // children and items are counted in int by the kernels and the solver; the item kernel has one thread per profile element
    if (nchild > (size_t)INT_MAX || nitems > (size_t)INT_MAX || nitems * 3 * lp / 256 >= (size_t)INT_MAX) return false;
    WorkLayout w;
    TransLayout L;
    L.parents = w.take((size_t)nctx * sizeof(SosDev), 256);
    L.children = w.take(nchild * sizeof(SosDev), 256);
    L.sv = w.take(nchild * 4 * kp * sizeof(double), 256);
    L.ctx_of_item = w.take(nitems * sizeof(int32_t), 256);
    L.nt = w.take(nitems * sizeof(int32_t), 256);
    L.iborm = w.take(nitems * sizeof(int32_t), 256);
    L.norders = w.take(nitems * sizeof(int32_t), 256);
    L.iglast = w.take(nitems * sizeof(int32_t), 256);
    L.flux = w.take(nitems * 2 * sizeof(double), 256);
    L.rec = w.take(nitems * 3 * (2 * (size_t)n + 1) * sizeof(double), 256);
    L.prof = w.take(nitems * 3 * lp * sizeof(double), 256);
    L.total = w.total + 256;                                // (the caller's area need only be 8-byte aligned)
    *out = L;
    return true;
}

// the contexts of a call: all there, built, on one device, one N
bool trans_ctxs_ok(sosgpu_ctx *const *ctxs, int nctx)
{
    if (!ctxs || nctx < 1) return false;
    for (int i = 0; i < nctx; i++)
        if (!ctxs[i] || !ctxs[i]->built || ctxs[i]->device != ctxs[0]->device || ctxs[i]->d.n != ctxs[0]->d.n) return false;
    return true;
}
}   // namespace

extern "C" size_t sosgpu_trans_spectrum_work_bytes(sosgpu_ctx *const *ctxs, int nctx, int nb, int lp)
{
    TransLayout L;
    if (!trans_ctxs_ok(ctxs, nctx) || !trans_layout(ctxs[0]->d.n, ctxs[0]->d.kp, nctx, nb, lp, &L)) return 0;
    return L.total;
}

// What sosgpu_trans_spectrum and sosgpu_albedo_spectrum share: the refusals, the parents' copy, the child table, the items and
// the order-0 solve.  d_out: the output neither call can do without (refused when NULL).  albedo: 0 the items of
// k_trans_items; 1, 2 those of k_albedo_items, 2 with the mirrored profile.  *q describes the items for the kernels behind
// the solve (unset where the call refuses or nb = 0 queues nothing).
static int trans_stage(sosgpu_ctx *const *ctxs, int nctx, const int32_t *d_ctx_of_bin, int nb, int lp, const int32_t *d_nt,
                       const double *d_prof, const void *d_out, void *d_work, size_t work_bytes, void *stream, int albedo,
                       AlbedoItems *q)
{
    if (!d_nt || !d_prof || !d_out || !d_work || nb < 0 || lp < 2) return SOSGPU_E_ARG;
    if (!trans_ctxs_ok(ctxs, nctx) || (!d_ctx_of_bin && nctx > 1)) return SOSGPU_E_ARG;
    const SosDev &p0 = ctxs[0]->d;
    TransLayout L;
    if (!trans_layout(p0.n, p0.kp, nctx, nb, lp, &L) || !work_area_ok(d_work, work_bytes, L.total)) return SOSGPU_E_ARG;
    SolvePlan variant;                       // (refused here as the solve would refuse it; no switch changes that)
    if (const int rc = solve_variant({p0.n, 0, nb, lp, 0, true}, SolveOverrides(), &variant)) return rc;
    if (nb == 0) return SOSGPU_OK;
    const int device = ctxs[0]->device;
    HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    char *base = reinterpret_cast<char *>(((unsigned long long)d_work + 255) & ~255ull);
    SosDev *d_parents = reinterpret_cast<SosDev *>(base + L.parents), *d_children = reinterpret_cast<SosDev *>(base + L.children);
    int os_nb_max = 0;
    {
        Staged s(device, (size_t)nctx * sizeof(SosDev));
        if (s.rc) return s.rc;
        SosDev *tab = static_cast<SosDev *>(s.host());
        for (int i = 0; i < nctx; i++) { tab[i] = ctxs[i]->d; os_nb_max = std::max(os_nb_max, ctxs[i]->d.os_nb); }
        HIPCHK(s.send(d_parents, st));
    }
    const int nchild = nctx * p0.n, nitems = nb * p0.n;
    launch_trans_table(d_parents, nchild, p0.n, d_children, reinterpret_cast<double *>(base + L.sv), os_nb_max, st);
    TransItems &it = q->t;
    it.nb = nb; it.n = p0.n; it.lp = lp; it.nctx = nctx;
    it.ctx_of_bin = d_ctx_of_bin; it.nt = d_nt; it.prof = d_prof;
    it.ctx_of_item = reinterpret_cast<int32_t *>(base + L.ctx_of_item);
    it.nt_item = reinterpret_cast<int32_t *>(base + L.nt);
    it.iborm_item = reinterpret_cast<int32_t *>(base + L.iborm);
    it.prof_item = reinterpret_cast<double *>(base + L.prof);
    it.flux = reinterpret_cast<double *>(base + L.flux);
    q->parents = d_parents; q->from_below = albedo == 2;
    if (albedo) launch_albedo_items(*q, st);
    else launch_trans_items(it, st);
    HIPCHK(hipGetLastError());
    // what the children have in common: order 0 only, a black ground without matrices (variant and record layout of the solve)
    SosDev as = p0;
    as.smax = 0; as.imat_surf = 0; as.ifresnel = 0; as.ro = 0.; as.mp_gnd = nullptr; as.rdir = nullptr;
    // 4 GiB of streamed-field scratch at a time: a few thousand items, several times what the chip hosts at once
    const int rc = os_solve_impl(ctxs[0], d_children, it.ctx_of_item, nullptr, nitems, lp, it.nt_item, it.iborm_item, it.prof_item,
                                 nullptr, nullptr, reinterpret_cast<double *>(base + L.rec),
                                 reinterpret_cast<int32_t *>(base + L.norders), reinterpret_cast<int32_t *>(base + L.iglast),
                                 it.flux, stream, 0, &as, 4);
    for (int i = 0; i < nctx; i++) note_stream(ctxs[i], st);       // (the kernels queued so far read their tables)
    return rc;
}

extern "C" int sosgpu_trans_spectrum(sosgpu_ctx *const *ctxs, int nctx, const int32_t *d_ctx_of_bin, int nb, int lp,
                                     const int32_t *d_nt, const double *d_prof, double *d_tdifmug, void *d_work,
                                     size_t work_bytes, void *stream)
{
    AlbedoItems q;
    const int rc = trans_stage(ctxs, nctx, d_ctx_of_bin, nb, lp, d_nt, d_prof, d_tdifmug, d_work, work_bytes, stream, 0, &q);
    if (rc || nb == 0) return rc;
    launch_trans_gather((size_t)q.t.nb * q.t.n, q.t.flux, d_tdifmug, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

// Spherical albedo of the atmosphere per bin (albedo.hip): the stage of sosgpu_trans_spectrum -- its work area, child table and
// solve -- with the items of k_albedo_items, and the up-going flux of every item summed over the directions.
extern "C" size_t sosgpu_albedo_spectrum_work_bytes(sosgpu_ctx *const *ctxs, int nctx, int nb, int lp)
{
    return sosgpu_trans_spectrum_work_bytes(ctxs, nctx, nb, lp);
}

extern "C" int sosgpu_albedo_spectrum(sosgpu_ctx *const *ctxs, int nctx, const int32_t *d_ctx_of_bin, int nb, int lp,
                                      const int32_t *d_nt, const double *d_prof, int from_below, double *d_plane, double *d_salb,
                                      void *d_work, size_t work_bytes, void *stream)
{
    AlbedoItems q;
    const int rc = trans_stage(ctxs, nctx, d_ctx_of_bin, nb, lp, d_nt, d_prof, d_salb, d_work, work_bytes, stream,
                               from_below ? 2 : 1, &q);
    if (rc || nb == 0) return rc;
    launch_albedo_sum(q, d_plane, d_salb, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_albedo_band(int nseg, const int32_t *d_seg, const double *d_aik, const double *d_salb, double *d_out,
                                  int device, void *stream)
{
    if (nseg < 0 || !d_seg || !d_aik || !d_salb || !d_out) return SOSGPU_E_ARG;
    if (nseg == 0) return SOSGPU_OK;
    if (const int rc = use_device(device)) return rc;
    launch_albedo_band(nseg, d_seg, d_aik, d_salb, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_last_solve_ms(sosgpu_ctx *cx, float *ms)
{
    if (!cx || !ms || !cx->timed) return SOSGPU_E_ARG;
    HIPCHK(hipEventSynchronize(cx->ev1));
    HIPCHK(hipEventElapsedTime(ms, cx->ev0, cx->ev1));
    return SOSGPU_OK;
}

extern "C" int sosgpu_os_flops(sosgpu_ctx *cx, int nb, const int32_t *d_nt, const int32_t *d_norders,
                               const int32_t *d_iglast, double *flops_out)
{
    if (!cx || !flops_out || nb < 0) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    const int S1 = cx->d.smax + 1;
    std::vector<int32_t> nt(nb), no(nb), ig((size_t)nb * S1);
    hipStream_t us = util_stream(cx->device);
    if (!us) return SOSGPU_E_HIP;
    HIPCHK(sync_ctx_streams(cx));              // the solve whose counts are read
    HIPCHK(hipMemcpyAsync(nt.data(), d_nt, nb * sizeof(int32_t), hipMemcpyDeviceToHost, us));
    HIPCHK(hipMemcpyAsync(no.data(), d_norders, nb * sizeof(int32_t), hipMemcpyDeviceToHost, us));
    HIPCHK(hipMemcpyAsync(ig.data(), d_iglast, (size_t)nb * S1 * sizeof(int32_t), hipMemcpyDeviceToHost, us));
    HIPCHK(hipStreamSynchronize(us));
    const double r6 = 6.0 * cx->d.n, r3 = 3.0 * cx->d.n, k3 = 3.0 * cx->d.nwgt;
    double tot = 0., exe = 0.;
    for (int b = 0; b < nb; b++) {
        const double L = nt[b] + 1.0;
        for (int s = 0; s < no[b]; s++) {
            const int steps = ig[(size_t)b * S1 + s] - 1;    // scattering orders >= 2 actually computed
            if (steps <= 0) continue;
            double w = 2. * r6 * r6 * L + 12. * r6 * nt[b];  // SURVEY 8d W_step
            double e = 2. * 2. * r3 * k3 * L + 10. * r6 * nt[b];
            if (s <= 2) { w += 2. * 3. * r6 * L * 3.; e += 2. * 4. * (r3 + k3) * L; }
            tot += steps * w;
            exe += steps * e;
        }
    }
    flops_out[0] = tot;
    flops_out[1] = exe;
    return SOSGPU_OK;
}

// Diagnostic: the plan a solve of this shape would follow, under the environment switches as they stand (solve_plan.h).
extern "C" int sosgpu_debug_solve_plan(int n, int smax, int nb, int lp, int nz, int table, int nt_max, sosgpu_solve_plan *plan)
{
    if (!plan || smax < 0 || nb < 1 || lp < 2 || nz < 0 || nz > SOSGPU_MAX_OUTPUT_LEVELS) return SOSGPU_E_ARG;
    const SolveShape sh = {n, smax, nb, lp, nz, table != 0};
    return solve_plan(sh, read_solve_overrides(), nt_max, plan);
}

// Diagnostic: the k-pair count of the order-0 contraction -- the rule itself (no context, no device), and a context's count
// with the switch back to the full contraction that the A/B of the two needs (include/sosgpu.h).
extern "C" int sosgpu_debug_order0_kpairs(int nwgt, int imat_surf)
{
    if (nwgt < 1 || nwgt > 85) return SOSGPU_E_ARG;
    return sos_order0_kpairs(nwgt, (3 * nwgt + 7) / 8, imat_surf != 0);
}

extern "C" int sosgpu_debug_ctx_order0_kpairs(sosgpu_ctx *cx, int mode)
{
    if (!cx) return SOSGPU_E_ARG;
    SosDev &d = cx->d;
    if (mode == 0) d.ks2h0 = sos_order0_kpairs(d.nwgt, d.ks2h, d.imat_surf != 0);
    else if (mode > 0) d.ks2h0 = d.ks2h;
    return d.ks2h0;
}

// Diagnostic: the streamed solver's scratch of this context (device pointer, size in doubles) and, after an order-parallel
// solve, where its I3 hand-over block starts (doubles from the start; 0 when the last solve did not use that form).
extern "C" int sosgpu_debug_scratch(sosgpu_ctx *cx, double **d_scratch, size_t *doubles, size_t *spec_i3_offset)
{
    if (!cx || !d_scratch || !doubles || !spec_i3_offset) return SOSGPU_E_ARG;
    *d_scratch = cx->scratch;
    *doubles = cx->scratch_doubles;
    *spec_i3_offset = cx->dbg_spec_i3;
    return SOSGPU_OK;
}
