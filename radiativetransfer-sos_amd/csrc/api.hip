// csrc/api.hip -- extern "C" surface of libsosgpu.so (see include/sosgpu.h for the contract and the
// reference routine each entry point replaces).  This unit: the error state, the device and utility-stream rules, and the
// life of a context.  The other entry points live in the api_*.hip units, one concern each; api_internal.h is what they share.
#include "api_internal.h"
#include "solve_variant.h"
#include <cmath>
#include <algorithm>
#include <cstring>

using namespace sosgpu_internal;

namespace sosgpu_internal {
__thread int g_last_hip = 0;
}   // namespace sosgpu_internal

extern "C" const char *sosgpu_version(void) { return "sosgpu 0.1 (gfx950)"; }
extern "C" int sosgpu_last_hip_error(void) { return g_last_hip; }

extern "C" const char *sosgpu_strerror(int code)
{
    switch (code) {
    case SOSGPU_OK: return "ok";
    case SOSGPU_E_ARG: return "bad argument";
    case SOSGPU_E_HIP: return "HIP runtime error";
    case SOSGPU_E_UNSUPPORTED: return "problem size outside the compiled kernel variants";
    case SOSGPU_E_NODEVICE: return "no gfx950 device visible";
    case SOSGPU_E_RCCL: return "RCCL unavailable or an RCCL call failed";
    default: return "unknown error";
    }
}

extern "C" int sosgpu_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_last_hip = (int)e; return SOSGPU_E_NODEVICE; }
    return n;
}

namespace sosgpu_internal {
// Entry points that name their device: SOSGPU_E_NODEVICE without a usable GPU, SOSGPU_E_ARG for an index out of range,
// otherwise `device` becomes the calling thread's current device.  (Runs after the host validation of the arguments.)
int use_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SOSGPU_E_NODEVICE;
    if (device < 0 || device >= ndev) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(device));
    return SOSGPU_OK;
}

// Ordering rule of the library (include/sosgpu.h, "Streams"): no entry point synchronises the DEVICE and none uses the
// null stream.  Host-synchronous entry points (sosgpu_create, sosgpu_ctx_table, sosgpu_os_flops, ...) move their data on a
// utility stream of the calling thread (non-blocking, created on first use, one per device) and wait for THAT stream only, so
// a call never waits for -- or is overtaken by -- work other host threads have queued on their own streams.
hipStream_t util_stream(int device)
{
    static thread_local hipStream_t st[16] = {nullptr};
    if (device < 0 || device >= 16) return nullptr;
    if (!st[device]) {
        // highest priority: the runtime maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES), in order per queue, and a
        // host framework may have created dozens of streams (torch: 32 per priority) -- at normal priority this stream then shares
        // a queue with caller streams, and its 20 us copies wait behind their kernels (0.4 ms per sosgpu_create inside
        // sos_spectrum, whose side streams run 1-2 ms profile kernels).  High-priority streams have hardware queues of their own.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        if (hipStreamCreateWithPriority(&st[device], hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();
            if (hipStreamCreateWithFlags(&st[device], hipStreamNonBlocking) != hipSuccess) st[device] = nullptr;
        }
    }
    return st[device];
}
}   // namespace sosgpu_internal

// Wait for the (short) work just queued on a utility stream.  hipStreamSynchronize blocks the thread on an interrupt once its
// spin window is over -- with kernels of other streams in flight that costs 0.3-0.4 ms of wake-up latency for a 20 us copy
// (measured inside sos_spectrum: sosgpu_create 0.41 ms against 0.03 ms on an idle device) -- so poll the stream first.
static hipError_t wait_short(hipStream_t us)
{
    for (int i = 0; i < 4000; i++) {
        const hipError_t q = hipStreamQuery(us);
        if (q == hipSuccess) return hipSuccess;
        if (q != hipErrorNotReady) return q;
    }
    return hipStreamSynchronize(us);
}

namespace sosgpu_internal {
void note_stream(sosgpu_ctx *cx, hipStream_t st)
{
    cx->last_stream = st;
    if (std::find(cx->used_streams.begin(), cx->used_streams.end(), st) == cx->used_streams.end()) cx->used_streams.push_back(st);
}

// waits for everything this context has queued (its solves may be in flight on several streams of the caller)
hipError_t sync_ctx_streams(sosgpu_ctx *cx)
{
    hipError_t e = hipSuccess;
    for (hipStream_t st : cx->used_streams) { const hipError_t r = hipStreamSynchronize(st); if (e == hipSuccess) e = r; }
    return e;
}
}   // namespace sosgpu_internal

extern "C" int sosgpu_create(sosgpu_ctx **out, int device, const sosgpu_wave *wv, const double *mu, const double *ga,
                             const double *alpha, const double *beta, const double *gamma, const double *zeta,
                             int iborm_max)
{
    if (!out || !wv || !mu || !ga || !alpha || !beta || !gamma || !zeta) return SOSGPU_E_ARG;
    const int N = wv->n, B = wv->os_nb;
    if (N < 1 || N > 85 || B < 2 || B > 400 || iborm_max < 0 || iborm_max > B) return SOSGPU_E_ARG;
    if (wv->n0 < 1 || wv->n0 > N) return SOSGPU_E_ARG;          // the solar direction must be one of mu[]
    if (wv->igmax < 1) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;

    sosgpu_ctx *cx = new sosgpu_ctx();
    cx->device = device;
    cx->bytes = 0;
    cx->timed = false;
    cx->built = false;
    cx->last_stream = nullptr;
    cx->ind_surf = wv->ind_surf;
    cx->scratch = nullptr;
    cx->scratch_doubles = 0;
    cx->dbg_spec_i3 = 0;
    cx->phase = nullptr;
    cx->agg_partial = nullptr;
    cx->prof_ng = nullptr;
    cx->prof_ng_stream = nullptr;
    cx->gnd_op = nullptr;
    cx->gnd_dir = nullptr;
    SosDev &d = cx->d;
    memset(&d, 0, sizeof(d));
    d.n = N; d.w = 2 * N + 1; d.r6 = 6 * N;
    d.kp = sos_round_up(6 * N, 8);
    d.kh = sos_round_up(3 * N, 8);
    // half-system row order: directions with a non-zero quadrature weight first (component-major), the zero-weight
    // ones (the solar direction, user angles: SOS_ANGLES gives them weight 0) last.  Their operator COLUMNS vanish, so
    // the contraction only runs over K = 3 Nw (N = 41: 15 k-pairs instead of 16); their rows are still computed.
    int nwgt = 0;
    for (int j = 0; j < N; j++) nwgt += ga[j] != 0.0;
    if (nwgt < 1) { delete cx; return SOSGPU_E_ARG; }
    d.ks2h = (3 * nwgt + 7) / 8;
    {   // projection rows ride in the last quad of the last row tile when that quad is padding
        const int cand = ((3 * N - 1) / 16) * 16 + 12;
        d.prow = cand >= 3 * N ? cand : -1;
    }
    std::vector<int32_t> rowmap(d.kh, -1);
    {
        int pos = 0;
        for (int pass = 0; pass < 2; pass++)
            for (int c = 0; c < 3; c++)
                for (int j = 0; j < N; j++)
                    if ((ga[j] != 0.0) == (pass == 0)) rowmap[pos++] = c * N + j;
    }
    d.rtph = (d.kh + 15) / 16;
    d.os_nb = B; d.smax = iborm_max;
    d.n0 = wv->n0; d.imat_surf = wv->imat_surf == 1; d.ifresnel = wv->ifresnel == 1 ? 1 : 0;
    d.igmax = wv->igmax; d.ipolar = wv->ipolar ? 1 : 0;
    d.ks2h0 = sos_order0_kpairs(nwgt, d.ks2h, d.imat_surf != 0);      // order 0: the I and Q columns only (solve_variant.h)
    d.mus = mu[wv->n0 - 1];
    d.ro = wv->ro;
    // molecular phase-matrix coefficients, SOS_OS.F:678-684
    double aaa = wv->ron / (2 - wv->ron);
    aaa = (1 - aaa) / (1 + 2 * aaa);
    d.beta2 = 0.5 * aaa; d.gamma2 = -aaa * sqrt(1.5); d.alpha2 = 3. * aaa;
    std::vector<double> coef((size_t)4 * (B + 1));
    for (int l = 0; l <= B; l++) {
        coef[l] = alpha[l]; coef[(B + 1) + l] = beta[l]; coef[2 * (B + 1) + l] = gamma[l]; coef[3 * (B + 1) + l] = zeta[l];
    }
    if (!d.ipolar) {    // SOS_OS.F:689-699
        d.gamma2 = 0.; d.alpha2 = 0.;
        for (int l = 0; l <= B; l++) { coef[l] = 0.; coef[2 * (B + 1) + l] = 0.; coef[3 * (B + 1) + l] = 0.; }
    }
    // thresholds: REAL*4 literals widened (SOS.h:389,394,400), D literal (SOS.h:395)
    d.thr_cv = (double)0.00001f; d.thr_sum = (double)0.00001f; d.thr_sf = (double)0.00001f; d.thr_val = 1.0e-50;
    // flat-sea Fresnel matrix, SOS_MAT_FRESNEL_PLAN_REFL (SOS_OS.F:1753-1780)
    std::vector<double> fres((size_t)3 * N, 0.);
    if (d.ifresnel) {
        for (int j = 0; j <= N; j++) {
            const double m = (j == 0) ? d.mus : mu[j - 1];
            const double ind2 = wv->ind_surf * wv->ind_surf, mu2 = m * m;
            const double x = sqrt(ind2 - 1.0 + mu2);
            const double rl = (ind2 * m - x) / (ind2 * m + x);
            const double rr = (m - x) / (m + x);
            const double f11 = (rl * rl + rr * rr) / 2.;
            const double f12 = d.ipolar ? (rl * rl - rr * rr) / 2. : 0.;
            const double f33 = d.ipolar ? rl * rr : 0.;
            if (j == 0) { d.f11sun = f11; d.f12sun = f12; }
            else { fres[j - 1] = f11; fres[N + j - 1] = f12; fres[2 * N + j - 1] = f33; }
        }
    }
    int rc;
    hipStream_t us = util_stream(device);
    if (!us) { delete cx; return SOSGPU_E_HIP; }
    // The context's small tables share ONE allocation, filled by ONE copy from a pinned block of the calling thread and one
    // memset: [mu | ga | coef | fres | rowmap] copied, [mp_vt | mp_uf] cleared (a spectrum creates one context per
    // wavelength: five pageable uploads, two fills and ten pool requests were 0.2 ms of each).  Offsets in doubles, each
    // a multiple of 32 (256-byte alignment of the operator fragments).
    auto up32 = [](size_t v) { return (v + 31) & ~(size_t)31; };
    const size_t o_mu = 0, o_ga = up32(o_mu + N), o_coef = up32(o_ga + N), o_fres = up32(o_coef + coef.size()),
                 o_map = up32(o_fres + fres.size()), o_vt = up32(o_map + (rowmap.size() + 1) / 2),
                 n_vt = (size_t)3 * d.ks2h * 128, n_uf = (size_t)3 * d.rtph * 64, o_uf = up32(o_vt + n_vt), n_small = o_uf + n_uf;
    // ... followed, in the same allocation, by the tables the kernels of sosgpu_noyaux / sosgpu_set_surface_matrices fill
    // (one pool request -- in a cold process one hipMalloc -- per context instead of six)
    const size_t per = (size_t)2 * d.rtph * d.ks2h * 128, S1c = (size_t)d.smax + 1;
    const size_t o_prt = up32(n_small), o_aer = up32(o_prt + S1c * 3 * (B + 1) * d.w), o_sv = up32(o_aer + S1c * per),
                 o_gop = up32(o_sv + S1c * 4 * d.kp), n_gop = d.imat_surf ? S1c * (per / 2) : 0, o_gdir = up32(o_gop + n_gop),
                 n_gdir = d.imat_surf ? S1c * 3 * N : 0, n_all = o_gdir + n_gdir;
    double *small = nullptr;
    if ((rc = dev_alloc(cx, &small, n_all))) { sosgpu_destroy(cx); return rc; }
    static thread_local double *stage = nullptr;           // (kept for the life of the thread: 64 KB at the largest N and OS_NB)
    static thread_local size_t stage_n = 0;
    if (stage_n < o_vt) {
        if (stage) (void)hipHostFree(stage);
        stage = nullptr; stage_n = 0;
        if (hipHostMalloc((void **)&stage, up32(o_vt + 4096) * sizeof(double), hipHostMallocDefault) != hipSuccess) {
            g_last_hip = (int)hipGetLastError(); sosgpu_destroy(cx); return SOSGPU_E_HIP; }
        stage_n = up32(o_vt + 4096);
    }
    memset(stage, 0, o_vt * sizeof(double));
    memcpy(stage + o_mu, mu, (size_t)N * sizeof(double));
    memcpy(stage + o_ga, ga, (size_t)N * sizeof(double));
    memcpy(stage + o_coef, coef.data(), coef.size() * sizeof(double));
    memcpy(stage + o_fres, fres.data(), fres.size() * sizeof(double));
    memcpy(stage + o_map, rowmap.data(), rowmap.size() * sizeof(int32_t));
    d.mu = small + o_mu; d.ga = small + o_ga; d.coef = small + o_coef; d.fres = small + o_fres;
    d.rowmap = reinterpret_cast<int32_t *>(small + o_map);
    d.nwgt = nwgt;
    d.mp_vt = small + o_vt; d.mp_uf = small + o_uf;
    d.prt = small + o_prt; d.mp_aer = small + o_aer; d.sv = small + o_sv;
    if (d.imat_surf) { cx->gnd_op = small + o_gop; cx->gnd_dir = small + o_gdir; }
    // The upload and the fill run on the calling thread's utility stream and are waited for here (the pinned block is reused by
    // the thread's next call): when the call returns every table is in place, whatever stream sosgpu_noyaux and the solves are
    // queued on afterwards.  (Round 2 filled on the null stream: a non-blocking caller stream does not wait for it, and a fill
    // could land on top of the molecular operator sosgpu_noyaux had already packed.)
    if (hipMemcpyAsync(small, stage, o_vt * sizeof(double), hipMemcpyHostToDevice, us) != hipSuccess ||
        hipMemsetAsync(small + o_vt, 0, (n_small - o_vt) * sizeof(double), us) != hipSuccess ||
        wait_short(us) != hipSuccess) {
        g_last_hip = (int)hipGetLastError();
        sosgpu_destroy(cx);
        return SOSGPU_E_HIP;
    }
    cx->ev0 = cx->ev1 = nullptr;                           // (created by the first solve)
    *out = cx;
    return SOSGPU_OK;
}

extern "C" int sosgpu_destroy(sosgpu_ctx *cx)
{
    if (!cx) return SOSGPU_OK;
    // teardown: nothing useful can be done with a failing free, errors are deliberately dropped
    (void)hipSetDevice(cx->device);
    (void)sync_ctx_streams(cx);        // solves / table builds of this context may still be running, on any of its streams
    for (size_t i = 0; i < cx->allocs.size(); i++) mem_give(cx->device, cx->allocs[i], cx->alloc_cls[i]);
    if (cx->scratch) pool_give(cx->device, cx->scratch, cx->scratch_doubles);
    if (cx->ev0) (void)hipEventDestroy(cx->ev0);
    if (cx->ev1) (void)hipEventDestroy(cx->ev1);
    delete cx;
    return SOSGPU_OK;
}

extern "C" size_t sosgpu_ctx_bytes(const sosgpu_ctx *cx) { return cx ? cx->bytes : 0; }

// Diagnostic: the context's per-wavelength tables and layout numbers, copied to the host (read-only; include/sosgpu.h).
extern "C" int sosgpu_debug_tables(sosgpu_ctx *cx, sosgpu_tables_info *info, double *prt, double *mp_aer, double *mp_vt,
                                   double *mp_uf, double *sv, double *mp_gnd, double *rdir, int32_t *rowmap)
{
    if (!cx || !info) return SOSGPU_E_ARG;
    const SosDev &d = cx->d;
    if ((mp_gnd || rdir) && (!d.mp_gnd || !d.rdir)) return SOSGPU_E_ARG;
    info->n = d.n; info->w = d.w; info->kp = d.kp; info->kh = d.kh; info->ks2h = d.ks2h; info->rtph = d.rtph;
    info->nwgt = d.nwgt; info->prow = d.prow; info->os_nb = d.os_nb; info->smax = d.smax; info->n0 = d.n0;
    info->ipolar = d.ipolar;
    info->beta2 = d.beta2; info->gamma2 = d.gamma2; info->alpha2 = d.alpha2; info->f11sun = d.f11sun;
    info->f12sun = d.f12sun; info->mus = d.mus; info->ro = d.ro;
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t us = util_stream(cx->device);
    if (!us) return SOSGPU_E_HIP;
    HIPCHK(sync_ctx_streams(cx));            // the table builds may still be running on the streams they were queued on
    const size_t S1 = (size_t)d.smax + 1, per = (size_t)d.rtph * d.ks2h * 128;
    const struct { void *dst; const void *src; size_t bytes; } cp[] = {
        {prt, d.prt, S1 * 3 * (d.os_nb + 1) * d.w * sizeof(double)},
        {mp_aer, d.mp_aer, S1 * 2 * per * sizeof(double)},
        {mp_vt, d.mp_vt, (size_t)3 * d.ks2h * 128 * sizeof(double)},
        {mp_uf, d.mp_uf, (size_t)3 * d.rtph * 64 * sizeof(double)},
        {sv, d.sv, S1 * 4 * d.kp * sizeof(double)},
        {mp_gnd, d.mp_gnd, S1 * per * sizeof(double)},
        {rdir, d.rdir, S1 * 3 * d.n * sizeof(double)},
        {rowmap, d.rowmap, (size_t)d.kh * sizeof(int32_t)},
    };
    for (const auto &c : cp)
        if (c.dst) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, us));
    HIPCHK(hipStreamSynchronize(us));
    return SOSGPU_OK;
}

// Diagnostic: per-bin phase cycle counters [nb][8] (filled only by builds with -DSOS_PROFILE_PHASES).
extern "C" int sosgpu_debug_phase_buffer(sosgpu_ctx *cx, unsigned long long *d_phase)
{
    if (!cx) return SOSGPU_E_ARG;
    cx->phase = d_phase;
    return SOSGPU_OK;
}
