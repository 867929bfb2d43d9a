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

// The host half of a new context, shared by sosgpu_create and sosgpu_create_spectrum (the same statements, so the same bits):
// the argument rules (ctx_args_ok, and ctx_plan's "no direction has a weight"), the layout numbers and scalars of SosDev with
// the offsets of the context's one allocation (ctx_plan), the image of its small tables (ctx_image), the host-side state of a
// context that has its block (ctx_new, ctx_place).  None of them makes a device call.
namespace {
struct CtxArgs {                // the arguments of one sosgpu_create
    const sosgpu_wave *wv;
    const double *mu, *ga, *alpha, *beta, *gamma, *zeta;
    int iborm_max;
};

// Offsets in doubles, each a multiple of 32 (256-byte alignment of the operator fragments).  The context's small tables share
// ONE allocation: [mu | ga | coef | fres | rowmap] copied, [mp_vt | mp_uf] cleared (a spectrum creates one context per
// wavelength: five pageable uploads, two fills and ten pool requests were 0.2 ms of each) ...
struct CtxPlan {
    SosDev d;                   // everything but the pointers
    size_t o_mu, o_ga, o_coef, o_fres, o_map, o_vt, o_uf, n_small;
    // ... followed, in the same allocation, by the tables the kernels of sosgpu_noyaux / sosgpu_set_surface_matrices fill
    // (one pool request -- in a cold process one hipMalloc -- per context instead of six)
    size_t o_prt, o_aer, o_sv, o_gop, o_gdir, n_all;
};

bool ctx_args_ok(const CtxArgs &a)
{
    const sosgpu_wave *wv = a.wv;
    if (!wv || !a.mu || !a.ga || !a.alpha || !a.beta || !a.gamma || !a.zeta) return false;
    const int N = wv->n, B = wv->os_nb;
    if (N < 1 || N > 85 || B < 2 || B > 400 || a.iborm_max < 0 || a.iborm_max > B) return false;
    if (wv->n0 < 1 || wv->n0 > N) return false;          // the solar direction must be one of mu[]
    if (wv->igmax < 1) return false;
    return true;
}

// flat-sea Fresnel matrix at direction cosine m, SOS_MAT_FRESNEL_PLAN_REFL (SOS_OS.F:1753-1780)
void ctx_fresnel(double ind_surf, int ipolar, double m, double *f11, double *f12, double *f33)
{
    const double ind2 = ind_surf * ind_surf, mu2 = m * m;
    const double x = sqrt(ind2 - 1.0 + mu2);
    const double rl = (ind2 * m - x) / (ind2 * m + x);
    const double rr = (m - x) / (m + x);
    *f11 = (rl * rl + rr * rr) / 2.;
    *f12 = ipolar ? (rl * rl - rr * rr) / 2. : 0.;
    *f33 = ipolar ? rl * rr : 0.;
}

// SOSGPU_E_ARG for arguments ctx_args_ok refuses and when no direction has a weight
int ctx_plan(CtxPlan &p, const CtxArgs &a)
{
    if (!ctx_args_ok(a)) return SOSGPU_E_ARG;
    const sosgpu_wave *wv = a.wv;
    const double *mu = a.mu, *ga = a.ga;
    const int N = wv->n, B = wv->os_nb;
    SosDev &d = p.d;
    memset(&d, 0, sizeof(d));
    d.n = N; d.w = 2 * N + 1; d.r6 = 6 * N;
    d.kp = sos_round_up(6 * N, 8);
    d.kh = sos_round_up(3 * N, 8);
    // half-system row order: directions with a non-zero quadrature weight first (component-major), the zero-weight
    // ones (the solar direction, user angles: SOS_ANGLES gives them weight 0) last.  Their operator COLUMNS vanish, so
    // the contraction only runs over K = 3 Nw (N = 41: 15 k-pairs instead of 16); their rows are still computed.
    int nwgt = 0;
    for (int j = 0; j < N; j++) nwgt += ga[j] != 0.0;
    if (nwgt < 1) return SOSGPU_E_ARG;
    d.nwgt = nwgt;
    d.ks2h = (3 * nwgt + 7) / 8;
    {   // projection rows ride in the last quad of the last row tile when that quad is padding
        const int cand = ((3 * N - 1) / 16) * 16 + 12;
        d.prow = cand >= 3 * N ? cand : -1;
    }
    d.rtph = (d.kh + 15) / 16;
    d.os_nb = B; d.smax = a.iborm_max;
    d.n0 = wv->n0; d.imat_surf = wv->imat_surf == 1; d.ifresnel = wv->ifresnel == 1 ? 1 : 0;
    d.igmax = wv->igmax; d.ipolar = wv->ipolar ? 1 : 0;
    d.ks2h0 = sos_order0_kpairs(nwgt, d.ks2h, d.imat_surf != 0);      // order 0: the I and Q columns only (solve_variant.h)
    d.mus = mu[wv->n0 - 1];
    d.ro = wv->ro;
    // molecular phase-matrix coefficients, SOS_OS.F:678-684
    double aaa = wv->ron / (2 - wv->ron);
    aaa = (1 - aaa) / (1 + 2 * aaa);
    d.beta2 = 0.5 * aaa; d.gamma2 = -aaa * sqrt(1.5); d.alpha2 = 3. * aaa;
    if (!d.ipolar) { d.gamma2 = 0.; d.alpha2 = 0.; }    // SOS_OS.F:689-699
    // thresholds: REAL*4 literals widened (SOS.h:389,394,400), D literal (SOS.h:395)
    d.thr_cv = (double)0.00001f; d.thr_sum = (double)0.00001f; d.thr_sf = (double)0.00001f; d.thr_val = 1.0e-50;
    if (d.ifresnel) {
        double f33;
        ctx_fresnel(wv->ind_surf, d.ipolar, d.mus, &d.f11sun, &d.f12sun, &f33);
    }
    auto up32 = [](size_t v) { return (v + 31) & ~(size_t)31; };
    const size_t n_coef = (size_t)4 * (B + 1), n_fres = (size_t)3 * N, n_map = (size_t)d.kh;
    p.o_mu = 0; p.o_ga = up32(p.o_mu + N); p.o_coef = up32(p.o_ga + N); p.o_fres = up32(p.o_coef + n_coef);
    p.o_map = up32(p.o_fres + n_fres); p.o_vt = up32(p.o_map + (n_map + 1) / 2);
    const size_t n_vt = (size_t)3 * d.ks2h * 128, n_uf = (size_t)3 * d.rtph * 64;
    p.o_uf = up32(p.o_vt + n_vt); p.n_small = p.o_uf + n_uf;
    const size_t per = (size_t)2 * d.rtph * d.ks2h * 128, S1c = (size_t)d.smax + 1;
    p.o_prt = up32(p.n_small); p.o_aer = up32(p.o_prt + S1c * 3 * (B + 1) * d.w); p.o_sv = up32(p.o_aer + S1c * per);
    p.o_gop = up32(p.o_sv + S1c * 4 * d.kp);
    const size_t n_gop = d.imat_surf ? S1c * (per / 2) : 0, n_gdir = d.imat_surf ? S1c * 3 * N : 0;
    p.o_gdir = up32(p.o_gop + n_gop); p.n_all = p.o_gdir + n_gdir;
    return SOSGPU_OK;
}

// the small-table image [mu | ga | coef | fres | rowmap] of p.o_vt doubles, padding zero
void ctx_image(const CtxPlan &p, const CtxArgs &a, double *img)
{
    const SosDev &d = p.d;
    const int N = d.n, B = d.os_nb;
    memset(img, 0, p.o_vt * sizeof(double));
    memcpy(img + p.o_mu, a.mu, (size_t)N * sizeof(double));
    memcpy(img + p.o_ga, a.ga, (size_t)N * sizeof(double));
    double *coef = img + p.o_coef;                       // IPOLAR = 0 (SOS_OS.F:689-699): beta alone, the other rows stay 0
    memcpy(coef + (B + 1), a.beta, (size_t)(B + 1) * sizeof(double));
    if (d.ipolar) {
        memcpy(coef, a.alpha, (size_t)(B + 1) * sizeof(double));
        memcpy(coef + 2 * (B + 1), a.gamma, (size_t)(B + 1) * sizeof(double));
        memcpy(coef + 3 * (B + 1), a.zeta, (size_t)(B + 1) * sizeof(double));
    }
    if (d.ifresnel) {
        double *fres = img + p.o_fres;
        for (int j = 0; j < N; j++) ctx_fresnel(a.wv->ind_surf, d.ipolar, a.mu[j], fres + j, fres + N + j, fres + 2 * N + j);
    }
    int32_t *rowmap = reinterpret_cast<int32_t *>(img + p.o_map);
    for (int q = 0; q < d.kh; q++) rowmap[q] = -1;
    int pos = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int c = 0; c < 3; c++)
            for (int j = 0; j < N; j++)
                if ((a.ga[j] != 0.0) == (pass == 0)) rowmap[pos++] = c * N + j;
}

// a context in the host-side state sosgpu_create leaves, before it has its block
sosgpu_ctx *ctx_new(int device, const CtxPlan &p, const sosgpu_wave *wv)
{
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
    cx->ev0 = cx->ev1 = nullptr;                           // (created by the first solve)
    cx->d = p.d;
    return cx;
}

// the context's pointers into its block `small` of p.n_all doubles
void ctx_place(sosgpu_ctx *cx, const CtxPlan &p, double *small)
{
    SosDev &d = cx->d;
    d.mu = small + p.o_mu; d.ga = small + p.o_ga; d.coef = small + p.o_coef; d.fres = small + p.o_fres;
    d.rowmap = reinterpret_cast<int32_t *>(small + p.o_map);
    d.mp_vt = small + p.o_vt; d.mp_uf = small + p.o_uf;
    d.prt = small + p.o_prt; d.mp_aer = small + p.o_aer; d.sv = small + p.o_sv;
    if (d.imat_surf) { cx->gnd_op = small + p.o_gop; cx->gnd_dir = small + p.o_gdir; }
}
}   // namespace

extern "C" int sosgpu_create(sosgpu_ctx **out, int device, const sosgpu_wave *wv, const double *mu, const double *ga,
                             const double *alpha, const double *beta, const double *gamma, const double *zeta,
                             int iborm_max)
{
    const CtxArgs a = {wv, mu, ga, alpha, beta, gamma, zeta, iborm_max};
    if (!out || !ctx_args_ok(a)) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    CtxPlan p;
    if (const int rc = ctx_plan(p, a)) return rc;
    int rc;
    hipStream_t us = util_stream(device);
    if (!us) return SOSGPU_E_HIP;
    sosgpu_ctx *cx = ctx_new(device, p, wv);
    double *small = nullptr;
    if ((rc = dev_alloc(cx, &small, p.n_all))) { sosgpu_destroy(cx); return rc; }
    // filled by ONE copy from a pinned block of the calling thread and one memset
    auto up32 = [](size_t v) { return (v + 31) & ~(size_t)31; };
    static thread_local double *stage = nullptr;           // (kept for the life of the thread: 64 KB at the largest N and OS_NB)
    static thread_local size_t stage_n = 0;
    if (stage_n < p.o_vt) {
        if (stage) (void)hipHostFree(stage);
        stage = nullptr; stage_n = 0;
        if (hipHostMalloc((void **)&stage, up32(p.o_vt + 4096) * sizeof(double), hipHostMallocDefault) != hipSuccess) {
            g_last_hip = (int)hipGetLastError(); sosgpu_destroy(cx); return SOSGPU_E_HIP; }
        stage_n = up32(p.o_vt + 4096);
    }
    ctx_image(p, a, stage);
    ctx_place(cx, p, small);
    // The upload and the fill run on the calling thread's utility stream and are waited for here (the pinned block is reused by
    // the thread's next call): when the call returns every table is in place, whatever stream sosgpu_noyaux and the solves are
    // queued on afterwards.  (Round 2 filled on the null stream: a non-blocking caller stream does not wait for it, and a fill
    // could land on top of the molecular operator sosgpu_noyaux had already packed.)
    if (hipMemcpyAsync(small, stage, p.o_vt * sizeof(double), hipMemcpyHostToDevice, us) != hipSuccess ||
        hipMemsetAsync(small + p.o_vt, 0, (p.n_small - p.o_vt) * sizeof(double), us) != hipSuccess ||
        wait_short(us) != hipSuccess) {
        g_last_hip = (int)hipGetLastError();
        sosgpu_destroy(cx);
        return SOSGPU_E_HIP;
    }
    *out = cx;
    return SOSGPU_OK;
}

// sosgpu_create for the nctx contexts of a part of a spectrum: d_work = [job table | images], each image 256-byte aligned IN
// DEVICE MEMORY (k_ctx_fill moves 16 bytes per lane, and an area need only be 8-byte aligned: the layout keeps 248 bytes spare and
// starts at the first 256-byte address of the area), filled by one copy from a recycled pinned block (Staged); one k_ctx_fill
// launch then does for every context what the copy and the memset of sosgpu_create do.  Nothing is waited for.
namespace {
struct CreateLayout {
    size_t jobs, table_bytes, total;         // table_bytes: what the one copy moves; total: with the spare bytes
    std::vector<size_t> image;               // byte offset of every image from the aligned start
    size_t max_doubles;                      // largest n_small of the contexts (the grid of k_ctx_fill)
};
constexpr size_t kImageAlign = 256;

// the plans and the layout of a list of specs; SOSGPU_E_ARG when the call would refuse the list (nctx = 0: an empty layout)
int create_layout(const sosgpu_ctx_spec *specs, int nctx, std::vector<CtxPlan> &plans, CreateLayout &L)
{
    if (nctx < 0 || nctx > 65535 || (!specs && nctx > 0)) return SOSGPU_E_ARG;
    plans.resize((size_t)nctx);
    L.image.resize((size_t)nctx);
    L.max_doubles = 0;
    WorkLayout w;
    L.jobs = w.take((size_t)nctx * sizeof(CtxFillJob), kImageAlign);
    for (int i = 0; i < nctx; i++) {
        const sosgpu_ctx_spec &s = specs[i];
        const CtxArgs a = {&s.wv, s.mu, s.ga, s.alpha, s.beta, s.gamma, s.zeta, s.iborm_max};
        if (const int rc = ctx_plan(plans[i], a)) return rc;
        L.image[i] = w.take(plans[i].o_vt * sizeof(double), kImageAlign);
        L.max_doubles = std::max(L.max_doubles, plans[i].n_small);
    }
    L.table_bytes = w.total;
    w.take(kImageAlign - 8, 8);
    L.total = nctx > 0 ? w.total : 0;
    return SOSGPU_OK;
}
}   // namespace

extern "C" size_t sosgpu_create_spectrum_work_bytes(const sosgpu_ctx_spec *specs, int nctx)
{
    std::vector<CtxPlan> plans;
    CreateLayout L;
    return create_layout(specs, nctx, plans, L) == SOSGPU_OK ? L.total : 0;
}

extern "C" int sosgpu_create_spectrum(sosgpu_ctx **out, int device, const sosgpu_ctx_spec *specs, int nctx, void *d_work,
                                      size_t work_bytes, void *stream)
{
    if (!out) return SOSGPU_E_ARG;
    for (int i = 0; i < nctx; i++) out[i] = nullptr;
    std::vector<CtxPlan> plans;
    CreateLayout L;
    if (const int rc = create_layout(specs, nctx, plans, L)) return rc;
    if (nctx == 0) return SOSGPU_OK;
    if (!work_area_ok(d_work, work_bytes, L.total)) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    Staged s(device, L.table_bytes);
    if (s.rc) return s.rc;
    char *stage = static_cast<char *>(s.host());
    char *d_base = static_cast<char *>(d_work) + ((kImageAlign - ((uintptr_t)d_work & (kImageAlign - 1))) & (kImageAlign - 1));
    CtxFillJob *jobs = reinterpret_cast<CtxFillJob *>(stage + L.jobs);
    std::vector<sosgpu_ctx *> made;
    auto undo = [&made](int rc) { for (sosgpu_ctx *cx : made) sosgpu_destroy(cx); return rc; };
    for (int i = 0; i < nctx; i++) {
        const sosgpu_ctx_spec &sp = specs[i];
        const CtxArgs a = {&sp.wv, sp.mu, sp.ga, sp.alpha, sp.beta, sp.gamma, sp.zeta, sp.iborm_max};
        const CtxPlan &p = plans[i];
        sosgpu_ctx *cx = ctx_new(device, p, &sp.wv);
        made.push_back(cx);
        double *small = nullptr;
        if (const int rc = dev_alloc(cx, &small, p.n_all)) return undo(rc);
        ctx_image(p, a, reinterpret_cast<double *>(stage + L.image[i]));
        ctx_place(cx, p, small);
        jobs[i].dst = small;
        jobs[i].src_off = (uint32_t)(L.image[i] / sizeof(double));
        jobs[i].n_copy = (uint32_t)p.o_vt;
        jobs[i].n_clear = (uint32_t)(p.n_small - p.o_vt);
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = s.send(d_base, st);
    if (e == hipSuccess) {
        launch_ctx_fill(reinterpret_cast<const CtxFillJob *>(d_base + L.jobs), reinterpret_cast<const double *>(d_base), nctx,
                        L.max_doubles, st);
        e = hipGetLastError();
        for (sosgpu_ctx *cx : made) note_stream(cx, st);          // (a destroy -- undo's too -- waits for the fill)
    }
    if (e != hipSuccess) { g_last_hip = (int)e; return undo(SOSGPU_E_HIP); }
    for (int i = 0; i < nctx; i++) out[i] = made[i];
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
