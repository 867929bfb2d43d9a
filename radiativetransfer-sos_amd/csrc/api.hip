// csrc/api.hip -- extern "C" surface of libsosgpu.so (see include/sosgpu.h for the contract and the
// reference routine each entry point replaces).
#include "../../include/sosgpu.h"
#include "kernels.h"
#include "sos_common.h"
#include "solve_plan.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <climits>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <vector>

static thread_local int g_last_hip = 0;
#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t e_ = (x);                       \
        if (e_ != hipSuccess) {                    \
            g_last_hip = (int)e_;                  \
            return SOSGPU_E_HIP;                   \
        }                                          \
    } while (0)

struct sosgpu_ctx {
    int device;
    SosDev d;
    std::vector<void *> allocs;
    std::vector<size_t> alloc_cls;   // size class of each entry of allocs (mem_give)
    size_t bytes;
    hipEvent_t ev0, ev1;
    bool timed;
    bool built;             // sosgpu_noyaux / sosgpu_noyaux_spectrum has been queued: the operator tables are (being) filled
    hipStream_t last_stream;
    std::vector<hipStream_t> used_streams;   // every stream a solve / table build of this context was queued on
    int nt_max_hint;
    double ind_surf;
    unsigned long long *phase;   // diagnostic phase-cycle buffer (sosgpu_debug_phase_buffer), else null
    double *agg_partial;    // chunk partials of the large-batch aggregate
    double *scratch;        // field-in-HBM variant: grow-only per-bin scratch
    double *prof_ng;        // [4][608] no-gas profile of the wavelength (sosgpu_profile)
    hipStream_t prof_ng_stream;   // stream of the last sosgpu_profile (the block is rewritten in stream order)
    double *gnd_op, *gnd_dir;   // packed ground-reflection operators / solar-beam columns of the surface matrices (context-owned)
    size_t scratch_doubles;
    size_t dbg_spec_i3;     // offset of the order-parallel form's I3 block in the scratch of the last solve (diagnostic)
};

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

// Entry points that name their device: SOSGPU_E_NODEVICE without a usable GPU, SOSGPU_E_ARG for an index out of range,
// otherwise `device` becomes the calling thread's current device.  (Runs after the host validation of the arguments.)
static int use_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SOSGPU_E_NODEVICE;
    if (device < 0 || device >= ndev) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(device));
    return SOSGPU_OK;
}

// Device memory of the per-wavelength tables and of the entry points' temporaries comes from a process-wide pool of released
// blocks (size classes: 256 B steps up to 4 KiB, then eighths of the leading power of two; at most 16 GiB of the 288 / 8192 blocks kept:
// a chunk of sos_spectrum holds 256 contexts of six blocks each, and what the pool drops is a hipFree + hipMalloc per block).
// One sos_proc call = one context: without the pool every call pays ~10 hipMalloc + hipFree, and hipFree waits for the
// whole device -- i.e. for the kernels of every other host thread.  A block is only returned after the work that used it has been
// waited for (sosgpu_destroy: the context's streams; temporaries: their stream).  sosgpu_trim() empties the pool.
namespace {
struct PoolBlock { void *p; size_t n; int dev; };
std::mutex g_mem_mutex;
std::vector<PoolBlock> g_mem_free;
size_t g_mem_bytes = 0;

size_t mem_class(size_t n)
{
    if (n <= 4096) return (std::max<size_t>(n, 1) + 255) & ~(size_t)255;
    size_t p2 = 1;
    while ((p2 << 1) <= n) p2 <<= 1;
    const size_t step = p2 >> 3;
    return (n + step - 1) / step * step;
}

void mem_trim()
{
    std::vector<PoolBlock> all;
    {
        std::lock_guard<std::mutex> lk(g_mem_mutex);
        all.swap(g_mem_free);
        g_mem_bytes = 0;
    }
    for (const PoolBlock &b : all) { (void)hipSetDevice(b.dev); (void)hipFree(b.p); }
}

// *cls receives the size class (pass it back to mem_give); nullptr on failure
void *mem_take(int dev, size_t bytes, size_t *cls)
{
    const size_t c = mem_class(bytes);
    *cls = c;
    {
        std::lock_guard<std::mutex> lk(g_mem_mutex);
        for (size_t i = g_mem_free.size(); i-- > 0;)
            if (g_mem_free[i].dev == dev && g_mem_free[i].n == c) {
                void *p = g_mem_free[i].p;
                g_mem_free.erase(g_mem_free.begin() + i);
                g_mem_bytes -= c;
                return p;
            }
    }
    void *p = nullptr;
    if (hipMalloc(&p, c) != hipSuccess) {
        (void)hipGetLastError();
        sosgpu_trim();                             // the pools themselves may be what fills the device: release and retry once
        (void)hipSetDevice(dev);
        if (hipMalloc(&p, c) != hipSuccess) return nullptr;
    }
    return p;
}

void mem_give(int dev, void *p, size_t cls)
{
    if (!p) return;
    std::vector<PoolBlock> drop;
    {
        std::lock_guard<std::mutex> lk(g_mem_mutex);
        g_mem_free.push_back({p, cls, dev});
        g_mem_bytes += cls;
        while (g_mem_free.size() > 8192 || g_mem_bytes > ((size_t)16 << 30)) {     // oldest first
            g_mem_bytes -= g_mem_free.front().n;
            drop.push_back(g_mem_free.front());
            g_mem_free.erase(g_mem_free.begin());
        }
    }
    for (const PoolBlock &b : drop) (void)hipFree(b.p);
}

// temporary of one entry point: taken from the pool, returned by the destructor (the entry point has waited for its stream)
struct TmpBuf {
    int dev; void *p; size_t cls;
    TmpBuf(int device, size_t bytes) : dev(device), p(mem_take(device, bytes, &cls)) {}
    ~TmpBuf() { mem_give(dev, p, cls); }
    TmpBuf(const TmpBuf &) = delete;
    TmpBuf &operator=(const TmpBuf &) = delete;
};
}   // namespace

template <typename T>
static int dev_alloc(sosgpu_ctx *cx, T **p, size_t count)
{
    size_t cls = 0;
    void *q = mem_take(cx->device, count * sizeof(T), &cls);
    if (!q) { g_last_hip = (int)hipGetLastError(); return SOSGPU_E_HIP; }
    cx->allocs.push_back(q);
    cx->alloc_cls.push_back(cls);
    cx->bytes += count * sizeof(T);
    *p = static_cast<T *>(q);
    return 0;
}

// Ordering rule of the library (include/sosgpu.h, "Streams"): no entry point synchronises the DEVICE and none uses the
// null stream.  Host-synchronous entry points (sosgpu_create, sosgpu_ctx_table, sosgpu_os_flops, ...) move their data on a
// utility stream of the calling thread (non-blocking, created on first use, one per device) and wait for THAT stream only, so
// a call never waits for -- or is overtaken by -- work other host threads have queued on their own streams.
static hipStream_t util_stream(int device)
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

static void note_stream(sosgpu_ctx *cx, hipStream_t st)
{
    cx->last_stream = st;
    if (std::find(cx->used_streams.begin(), cx->used_streams.end(), st) == cx->used_streams.end()) cx->used_streams.push_back(st);
}

// waits for everything this context has queued (its solves may be in flight on several streams of the caller)
static hipError_t sync_ctx_streams(sosgpu_ctx *cx)
{
    hipError_t e = hipSuccess;
    for (hipStream_t st : cx->used_streams) { const hipError_t r = hipStreamSynchronize(st); if (e == hipSuccess) e = r; }
    return e;
}

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

// The streamed solver's scratch outlives its context: one sos_proc call = one context (one wavelength), and a fresh hipMalloc
// of the 60-1000 MB the order-parallel form wants costs ~9 ms per call (scripts/latency_bench.py: 1.1 ms solve, 9.2 ms first
// call) -- more than the solve.  Released buffers wait here (per device, at most 8 of them and 8 GiB in total) for the next
// context.  A buffer is only returned after the stream of its last solve has been synchronised.
namespace {
struct ScratchBuf { double *p; size_t n; int dev; };
std::mutex g_pool_mutex;
std::vector<ScratchBuf> g_pool;

double *pool_take(int dev, size_t need, size_t *got)
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        int best = -1;
        for (int i = 0; i < (int)g_pool.size(); i++)
            if (g_pool[i].dev == dev && g_pool[i].n >= need && (best < 0 || g_pool[i].n < g_pool[best].n)) best = i;
        if (best >= 0) {
            ScratchBuf b = g_pool[best];
            g_pool.erase(g_pool.begin() + best);
            *got = b.n;
            return b.p;
        }
    }
    double *p = nullptr;
    if (getenv("SOSGPU_DEBUG_POOL")) fprintf(stderr, "[sosgpu pool] hipMalloc %.1f MB\n", need * 8e-6);
    if (hipMalloc((void **)&p, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        sosgpu_trim();                             // up to 8 GiB of kept scratch + 16 GiB of kept tables: release, retry once
        (void)hipSetDevice(dev);
        if (hipMalloc((void **)&p, need * sizeof(double)) != hipSuccess) return nullptr;
    }
    *got = need;
    return p;
}

void pool_give(int dev, double *p, size_t n)
{
    if (!p) return;
    std::vector<double *> drop;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        g_pool.push_back({p, n, dev});
        size_t total = 0;
        for (const ScratchBuf &b : g_pool) total += b.n * sizeof(double);
        while (g_pool.size() > 8 || total > ((size_t)8 << 30)) {     // oldest first
            total -= g_pool.front().n * sizeof(double);
            drop.push_back(g_pool.front().p);
            g_pool.erase(g_pool.begin());
        }
    }
    if (!drop.empty() && getenv("SOSGPU_DEBUG_POOL")) fprintf(stderr, "[sosgpu pool] hipFree of %zu buffer(s)\n", drop.size());
    for (double *q : drop) (void)hipFree(q);
}
}   // namespace

// The per-wavelength or per-job table of every table-form entry point travels to the caller's work area from a pinned block
// the library recycles (per device): a block is free again when the event recorded behind its copy has passed.  Nothing is
// waited for and no context owns a block; sosgpu_trim frees those that have passed.
namespace {
struct StageBlock { void *p; size_t bytes; hipEvent_t ev; int device; };
std::mutex g_stage_mutex;
std::vector<StageBlock> g_stage;     // the blocks in no call's hands

bool stage_passed(const StageBlock &b)      // (a never-recorded event queries as complete)
{
    if (hipEventQuery(b.ev) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// One table on its way: takes the first block of the device that is large enough and has passed out of g_stage, else makes
// one (16 KiB at least); the caller fills host() in place and send()s it.  A block that is never sent goes back as it came.
class Staged {
    StageBlock b = {};
    const size_t n;
    int take(int device)
    {
        {
            std::lock_guard<std::mutex> lk(g_stage_mutex);
            for (auto it = g_stage.begin(); it != g_stage.end(); ++it)
                if (it->device == device && it->bytes >= n && stage_passed(*it)) { b = *it; g_stage.erase(it); return SOSGPU_OK; }
        }
        b.bytes = std::max(n, (size_t)16384); b.device = device;
        HIPCHK(hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
        const hipError_t e = hipHostMalloc(&b.p, b.bytes, hipHostMallocDefault);
        if (e != hipSuccess) { b.p = nullptr; (void)hipEventDestroy(b.ev); HIPCHK(e); }
        return SOSGPU_OK;
    }
    void give()
    {
        if (!b.p) return;
        std::lock_guard<std::mutex> lk(g_stage_mutex);
        g_stage.push_back(b);
        b.p = nullptr;
    }
public:
    const int rc;                    // SOSGPU_OK, or why there is no block (g_last_hip set)
    Staged(int device, size_t bytes) : n(bytes), rc(take(device)) {}
    ~Staged() { give(); }
    Staged(const Staged &) = delete;
    void *host() const { return b.p; }
    // queues the copy of the table to d_dst on st and records the event that frees the block behind it; the copy's status
    hipError_t send(void *d_dst, hipStream_t st)
    {
        const hipError_t e = hipMemcpyAsync(d_dst, b.p, n, hipMemcpyHostToDevice, st);
        (void)hipEventRecord(b.ev, st);
        give();
        return e;
    }
};

// Work areas (include/sosgpu.h, "Work areas").  A layout is written once, as a function that take()s its sections in order: the
// _work_bytes query returns its total, the call places its pointers at the offsets take() gave.
struct WorkLayout {
    size_t total = 0;
    // a section of `bytes` at the running total, which then moves to the next multiple of `align` behind it
    size_t take(size_t bytes, size_t align)
    {
        const size_t at = total;
        total = (total + bytes + align - 1) & ~(align - 1);
        return at;
    }
};

// what every table-form call asks of its area: there, 8-byte aligned, `need` bytes at least
bool work_area_ok(const void *d_work, size_t work_bytes, size_t need)
{
    return d_work && ((uintptr_t)d_work & 7) == 0 && work_bytes >= need;
}

// closing of a host-synchronous entry point: `st` is waited for whatever `e` says; the first error of the two
hipError_t finish_sync(hipError_t e, hipStream_t st)
{
    const hipError_t s = hipStreamSynchronize(st);
    return e == hipSuccess ? s : e;
}
}   // namespace

extern "C" int sosgpu_trim(void)
{
    std::vector<ScratchBuf> all;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        all.swap(g_pool);
    }
    for (const ScratchBuf &b : all) { (void)hipSetDevice(b.dev); (void)hipFree(b.p); }
    mem_trim();
    std::lock_guard<std::mutex> lk(g_stage_mutex);
    for (size_t i = g_stage.size(); i-- > 0;) {
        const StageBlock b = g_stage[i];
        if (stage_passed(b)) { (void)hipHostFree(b.p); (void)hipEventDestroy(b.ev); g_stage.erase(g_stage.begin() + i); }
    }
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

// Ground-reflection operator of a BRDF/BPDF surface in the packed A-fragment layout of the source operators (one system,
// rows = up-going half-system positions (c, k), columns = down-going positions (b, j), sos_common.h):
//   G[(c,k)][(b,j)] = (2/mu_k) w_j R_cb(j, k)   (SOS_OS.F:1194-1220; R_cb(I = j, J = k) = r[s][c*3+b][k*N + j])
//                     + 2 rho w_j mu_j for c = b = 0 and s = 0 (Lambertian part, SOS_OS.F:1177-1190)
// with the polarisation cut of SOS_OS.F:928-941 (IPOLAR = 0: only R_11 is kept), plus the solar-beam column
// rdir[s][c][k] = R_c1(N0, k) of the direct term (SOS_OS.F:984-990).
// (the body of element q of order s, shared by k_pack_ground and the table form k_pack_ground_table: the same bits)
template <class CX>
__device__ inline void pack_ground_body(const CX &cx, const int s, const size_t q, const float *__restrict__ r,
                                        double *__restrict__ gop, double *__restrict__ rdir)
{
    // no fused multiply-add: the Lambertian term is added to the rounded BRDF term, as the formula above reads (with
    // contraction the sum was one ulp off its plain evaluation in about one entry of eight)
#pragma clang fp contract(off)
    const int N = cx.n;
    const size_t per = (size_t)cx.rtph * cx.ks2h * 128;
    const float *rs = r + (size_t)s * 9 * N * N;
    if (q < per) {
        const int e2 = q & 1, lane = (q >> 1) & 63;
        const int m = (int)((q >> 7) % cx.ks2h), rt = (int)((q >> 7) / cx.ks2h);
        // A-operand order of v_mfma_f64_4x4x4f64 (sos_dev.h ground_mfma): block = row quad, lane>>4 = k
        const int row = rt * 16 + ((lane >> 2) & 3) * 4 + (lane & 3), col = 8 * m + 4 * e2 + (lane >> 4);
        double v = 0.;
        if (row < 3 * N && col < 3 * N) {
            const int ro = cx.rowmap[row], co = cx.rowmap[col];
            const int c = ro / N, k = ro % N, b = co / N, j = co % N;
            double x = rs[(size_t)(c * 3 + b) * N * N + (size_t)k * N + j];
            if (!cx.ipolar && (c || b)) x = 0.;
            v = (2. / cx.mu[k]) * cx.ga[j] * x;
            if (c == 0 && b == 0 && s == 0 && cx.ro != 0.) v = v + 2. * cx.ro * cx.ga[j] * cx.mu[j];
        }
        gop[(size_t)s * per + q] = v;
    }
    if (q < (size_t)3 * N) {
        const int c = (int)(q / N), k = (int)(q % N);
        double x = rs[(size_t)(c * 3) * N * N + (size_t)k * N + (cx.n0 - 1)];
        if (!cx.ipolar && c) x = 0.;
        rdir[(size_t)s * 3 * N + q] = x;
    }
}

__global__ void k_pack_ground(SosDev cx, const float *__restrict__ r, double *__restrict__ gop, double *__restrict__ rdir)
{
    pack_ground_body(cx, blockIdx.y, (size_t)blockIdx.x * blockDim.x + threadIdx.x, r, gop, rdir);
}

// Table form (sosgpu_noyaux_spectrum): context = blockIdx.z of a device table, its matrices rsurf[blockIdx.z] (null: the
// context has none, the workgroup leaves), its outputs the entry's own mp_gnd / rdir.  The grid takes the largest context with
// matrices; a workgroup tests the order against its own context, the body tests the element (q < per, q < 3N).
__global__ void k_pack_ground_table(const SosDev *tab, const float *const *rsurf)
{
    const SosDevK &cx = *(const SosDevK *)(unsigned long long)(tab + blockIdx.z);
    const float *r = rsurf[blockIdx.z];
    if (!r || (int)blockIdx.y > cx.smax) return;
    pack_ground_body(cx, blockIdx.y, (size_t)blockIdx.x * blockDim.x + threadIdx.x, r, const_cast<double *>(cx.mp_gnd),
                     const_cast<double *>(cx.rdir));
}

static int set_surface_matrices_impl(sosgpu_ctx *cx, const float *d_rsurf, hipStream_t st)
{
    if (!cx) return SOSGPU_E_ARG;
    if (cx->d.imat_surf && !d_rsurf) return SOSGPU_E_ARG;
    if (!d_rsurf) { cx->d.mp_gnd = nullptr; cx->d.rdir = nullptr; return SOSGPU_OK; }
    HIPCHK(hipSetDevice(cx->device));
    const size_t per = (size_t)cx->d.rtph * cx->d.ks2h * 128, S1 = (size_t)cx->d.smax + 1;
    if (!cx->gnd_op) {
        int rc = dev_alloc(cx, &cx->gnd_op, S1 * per);
        if (!rc) rc = dev_alloc(cx, &cx->gnd_dir, S1 * 3 * cx->d.n);
        if (rc) return rc;
    }
    dim3 grid((unsigned)((std::max(per, (size_t)3 * cx->d.n) + 255) / 256), (unsigned)S1);
    k_pack_ground<<<grid, 256, 0, st>>>(cx->d, d_rsurf, cx->gnd_op, cx->gnd_dir);
    HIPCHK(hipGetLastError());
    note_stream(cx, st);
    cx->d.mp_gnd = cx->gnd_op;
    cx->d.rdir = cx->gnd_dir;
    return SOSGPU_OK;
}

// stream-ordered form: the packing kernel is queued on `stream` (where d_rsurf was produced, or after it was complete) and
// nothing is waited for; d_rsurf must stay allocated until that work has run
extern "C" int sosgpu_set_surface_matrices_async(sosgpu_ctx *cx, const float *d_rsurf, void *stream)
{
    return set_surface_matrices_impl(cx, d_rsurf, (hipStream_t)stream);
}

// host-synchronous form (round 1's contract: the caller may release d_rsurf on return).  d_rsurf must be complete when the call
// is made -- the packing runs on the calling thread's utility stream, which is all the call waits for.
extern "C" int sosgpu_set_surface_matrices(sosgpu_ctx *cx, const float *d_rsurf)
{
    if (!cx) return SOSGPU_E_ARG;
    hipStream_t us = util_stream(cx->device);
    if (!us) return SOSGPU_E_HIP;
    const int rc = set_surface_matrices_impl(cx, d_rsurf, us);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(us));
    return SOSGPU_OK;
}

extern "C" int sosgpu_noyaux(sosgpu_ctx *cx, void *stream)
{
    if (!cx) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    launch_noyaux(cx->d, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    note_stream(cx, (hipStream_t)stream);
    cx->built = true;
    return SOSGPU_OK;
}

// sosgpu_set_surface_matrices_async + sosgpu_noyaux of nctx contexts in at most five launches (the table forms of their
// kernels, noyaux.hip / k_pack_ground_table).  d_work = [SosDev entries | matrix pointers], filled by one copy from a recycled
// pinned block (Staged).  Everything is checked before a context is touched.
namespace {
struct NoyauxLayout { size_t tab, rsurf, total; };
NoyauxLayout noyaux_layout(int nctx)
{
    static_assert(sizeof(SosDev) % 8 == 0, "the pointer list follows the entries");
    WorkLayout w;
    NoyauxLayout L;
    L.tab = w.take((size_t)nctx * sizeof(SosDev), 8);
    L.rsurf = w.take((size_t)nctx * sizeof(const float *), 8);
    L.total = w.total;
    return L;
}
}   // namespace

extern "C" size_t sosgpu_noyaux_spectrum_work_bytes(int nctx)
{
    return nctx > 0 && nctx <= 65535 ? noyaux_layout(nctx).total : 0;
}

extern "C" int sosgpu_noyaux_spectrum(sosgpu_ctx *const *ctxs, int nctx, const float *const *d_rsurf, void *d_work,
                                      size_t work_bytes, void *stream)
{
    if (!ctxs || !d_work || nctx < 0 || nctx > 65535) return SOSGPU_E_ARG;
    if (nctx == 0) return SOSGPU_OK;
    const NoyauxLayout L = noyaux_layout(nctx);
    if (!work_area_ok(d_work, work_bytes, L.total)) return SOSGPU_E_ARG;
    NoyauxTableGrid g = {0, 0, 0};
    size_t gnd_elems = 0;                       // ground launch: largest max(per, 3N) and smax over the contexts with matrices
    int gnd_smax = -1;
    for (int i = 0; i < nctx; i++) {
        const sosgpu_ctx *cx = ctxs[i];
        if (!cx || cx->device != ctxs[0]->device) return SOSGPU_E_ARG;
        const float *r = d_rsurf ? d_rsurf[i] : nullptr;
        if ((cx->d.imat_surf != 0) != (r != nullptr)) return SOSGPU_E_ARG;
        if (r && (!cx->gnd_op || !cx->gnd_dir)) return SOSGPU_E_ARG;
        const size_t per = (size_t)cx->d.rtph * cx->d.ks2h * 128;
        g.smax = std::max(g.smax, cx->d.smax); g.kp = std::max(g.kp, cx->d.kp); g.per = std::max(g.per, per);
        if (r) { gnd_elems = std::max(gnd_elems, std::max(per, (size_t)3 * cx->d.n)); gnd_smax = std::max(gnd_smax, cx->d.smax); }
    }
    HIPCHK(hipSetDevice(ctxs[0]->device));
    Staged s(ctxs[0]->device, L.total);
    if (s.rc) return s.rc;
    char *stage = static_cast<char *>(s.host());
    SosDev *tab = reinterpret_cast<SosDev *>(stage + L.tab);
    const float **rs = reinterpret_cast<const float **>(stage + L.rsurf);
    for (int i = 0; i < nctx; i++) {
        sosgpu_ctx *cx = ctxs[i];
        rs[i] = d_rsurf ? d_rsurf[i] : nullptr;
        cx->d.mp_gnd = rs[i] ? cx->gnd_op : nullptr;
        cx->d.rdir = rs[i] ? cx->gnd_dir : nullptr;
        tab[i] = cx->d;
    }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(s.send(d_work, st));
    char *dp = static_cast<char *>(d_work);
    const SosDev *d_tab = reinterpret_cast<const SosDev *>(dp + L.tab);
    if (gnd_smax >= 0) {
        dim3 grid((unsigned)((gnd_elems + 255) / 256), (unsigned)gnd_smax + 1, (unsigned)nctx);
        k_pack_ground_table<<<grid, 256, 0, st>>>(d_tab, reinterpret_cast<const float *const *>(dp + L.rsurf));
    }
    launch_noyaux_table(d_tab, nctx, g, st);
    HIPCHK(hipGetLastError());
    for (int i = 0; i < nctx; i++) { note_stream(ctxs[i], st); ctxs[i]->built = true; }
    return SOSGPU_OK;
}

extern "C" int sosgpu_noyaux_fetch(sosgpu_ctx *cx, int is, double *out)
{
    if (!cx || !out || is < 0 || is > cx->d.smax) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    const size_t cnt = (size_t)6 * cx->d.w * cx->d.w + 3 * cx->d.w;
    hipStream_t us = util_stream(cx->device);
    if (!us) return SOSGPU_E_HIP;
    TmpBuf tmp(cx->device, cnt * sizeof(double));
    if (!tmp.p) return SOSGPU_E_HIP;
    HIPCHK(sync_ctx_streams(cx));            // sosgpu_noyaux may still be running on the stream it was queued on
    launch_noyaux_fetch(cx->d, is, (double *)tmp.p, us);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, tmp.p, cnt * sizeof(double), hipMemcpyDeviceToHost, us));
    HIPCHK(hipStreamSynchronize(us));
    return SOSGPU_OK;
}

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

// The context's scratch holds at least `need` doubles afterwards (grow-only; taken from / handed back to the pool above).
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

extern "C" size_t sosgpu_ctx_table_entry_bytes(void) { return sizeof(SosDev); }

extern "C" int sosgpu_ctx_table(sosgpu_ctx *const *ctxs, int nctx, void *d_table, void *stream)
{
    if (!ctxs || nctx < 1 || !d_table || !ctxs[0]) return SOSGPU_E_ARG;
    const SosDev &a = ctxs[0]->d;
    for (int i = 0; i < nctx; i++) {
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device) return SOSGPU_E_ARG;
        const SosDev &d = ctxs[i]->d;
        // what selects the kernel variant and the record layout must agree over the table
        if (d.n != a.n || d.kh != a.kh || d.ks2h != a.ks2h || d.rtph != a.rtph || d.smax != a.smax ||
            (d.imat_surf != 0) != (a.imat_surf != 0))
            return SOSGPU_E_ARG;
        if (d.imat_surf && !d.mp_gnd) return SOSGPU_E_ARG;
    }
    // copied on the caller's stream (d_table may be a buffer the caller's allocator has just recycled, still read by work queued there)
    HIPCHK(hipSetDevice(ctxs[0]->device));
    Staged s(ctxs[0]->device, (size_t)nctx * sizeof(SosDev));
    if (s.rc) return s.rc;
    SosDev *tab = static_cast<SosDev *>(s.host());
    for (int i = 0; i < nctx; i++) tab[i] = ctxs[i]->d;
    HIPCHK(s.send(d_table, (hipStream_t)stream));
    note_stream(ctxs[0], (hipStream_t)stream);
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

__global__ void k_aggregate_empty(int nel, int sw, double *out_rec, double *out_scal)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nel) out_rec[e] = 0.;
    if (e < sw) out_scal[e] = (e == 8) ? -2147483647. : 0.;
}

extern "C" int sosgpu_aggregate(sosgpu_ctx *cx, int nb, int nseg, const int32_t *d_seg, const double *d_aik,
                                const double *d_rec, const int32_t *d_norders, const double *d_flux, const double *d_scal,
                                const double *d_tdifmug, double *d_out_rec, double *d_out_scal, void *stream)
{
    if (!cx || nb < 0 || nseg < 1 || !d_out_rec || !d_out_scal) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t st = (hipStream_t)stream;
    const int nel = (cx->d.smax + 1) * 3 * cx->d.w;
    if (nb == 0) {          // empty shard of a band: neutral element of the cross-rank reduce
        if (nseg != 1) return SOSGPU_E_ARG;
        const int sw = SOSGPU_SCAL_BASE + cx->d.n;
        k_aggregate_empty<<<(std::max(nel, sw) + 255) / 256, 256, 0, st>>>(nel, sw, d_out_rec, d_out_scal);
        HIPCHK(hipGetLastError());
        return SOSGPU_OK;
    }
    if (nseg > nb || !d_seg || !d_aik || !d_rec || !d_norders || !d_flux || !d_scal) return SOSGPU_E_ARG;
    const int max_chunks = 4096;
    const int nb_single = (nseg == 1) ? nb : 0;      // one band: big batches use the chunked reduction
    if (nb_single > 128 && !cx->agg_partial) {
        if (int rc = dev_alloc(cx, &cx->agg_partial, (size_t)nel * max_chunks)) return rc;
    }
    launch_aggregate(cx->d, nseg, d_seg, d_aik, d_rec, d_norders, d_flux, d_scal, d_tdifmug, d_out_rec, d_out_scal, st,
                     nb_single, cx->agg_partial, max_chunks);
    HIPCHK(hipGetLastError());
    note_stream(cx, st);
    return SOSGPU_OK;
}

extern "C" int sosgpu_level_transmission(int device, int nb, int nseg, const int32_t *d_seg, const double *d_aik,
                                         const int32_t *d_norders, int nz, const double *d_tau, double *d_out_scal,
                                         size_t slot_stride, int block_width, void *stream)
{
    if (nb < 0 || nseg < 1 || nseg > 65535 || !d_seg || !d_aik || !d_norders || !d_tau || !d_out_scal) return SOSGPU_E_ARG;
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS || block_width < SOSGPU_SCAL_BASE) return SOSGPU_E_ARG;
    if (nz > 1 && slot_stride < (size_t)nseg * (size_t)block_width) return SOSGPU_E_ARG;      // slots would overlap
    if (nb == 0) return SOSGPU_OK;          // empty shard of a band: sosgpu_aggregate's 0 is the neutral element
    if (nseg > nb) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    launch_level_transmission(nb, nseg, d_seg, d_aik, d_norders, nz, d_tau, d_out_scal, slot_stride, block_width,
                              (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// Cross-GPU reduce of the band partials over RCCL (xGMI).  librccl is resolved lazily with dlopen: a process that
// already holds an RCCL (torch's) gets that one, single-GPU users never load it.
// ---------------------------------------------------------------------------------------------
struct Uid { char internal[SOSGPU_UNIQUE_ID_BYTES]; };   // ncclUniqueId (nccl.h: 128 opaque bytes, passed by value)
namespace {
struct Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, Uid, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
};
}  // namespace
static Rccl g_rccl;
static int rccl_load_once()
{
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return SOSGPU_E_RCCL;
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(h, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(h, "ncclGroupEnd");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce || !g_rccl.GroupStart ||
        !g_rccl.GroupEnd)
        return SOSGPU_E_RCCL;
    g_rccl.h = h;
    return 0;
}
static int rccl_load()
{
    static std::once_flag once;            // host threads may reach the first RCCL call together
    static int rc = SOSGPU_E_RCCL;
    std::call_once(once, [] { rc = rccl_load_once(); });
    return rc;
}

extern "C" int sosgpu_comm_unique_id(char id[SOSGPU_UNIQUE_ID_BYTES])
{
    if (!id) return SOSGPU_E_ARG;
    if (int rc = rccl_load()) return rc;
    Uid u;
    memset(&u, 0, sizeof u);
    if (g_rccl.GetUniqueId(&u) != 0) return SOSGPU_E_RCCL;
    memcpy(id, u.internal, SOSGPU_UNIQUE_ID_BYTES);
    return SOSGPU_OK;
}

extern "C" int sosgpu_comm_init_rank(void **comm, int nranks, const char id[SOSGPU_UNIQUE_ID_BYTES], int rank)
{
    if (!comm || !id || nranks < 1 || rank < 0 || rank >= nranks) return SOSGPU_E_ARG;
    if (int rc = rccl_load()) return rc;
    Uid u;
    memcpy(u.internal, id, SOSGPU_UNIQUE_ID_BYTES);
    return g_rccl.CommInitRank(comm, nranks, u, rank) == 0 ? SOSGPU_OK : SOSGPU_E_RCCL;
}

extern "C" int sosgpu_comm_destroy(void *comm)
{
    if (!comm) return SOSGPU_OK;
    if (int rc = rccl_load()) return rc;
    return g_rccl.CommDestroy(comm) == 0 ? SOSGPU_OK : SOSGPU_E_RCCL;
}

extern "C" int sosgpu_pack(sosgpu_ctx *cx, int nseg, const double *d_out_rec, const double *d_out_scal, double *d_buf, void *stream)
{
    if (!cx || nseg < 1 || !d_out_rec || !d_out_scal || !d_buf) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    const size_t nel = (size_t)(cx->d.smax + 1) * 3 * cx->d.w, sw = SOSGPU_SCAL_BASE + cx->d.n, row = nel + sw;
    HIPCHK(hipMemcpy2DAsync(d_buf, row * 8, d_out_rec, nel * 8, nel * 8, nseg, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(hipMemcpy2DAsync(d_buf + nel, row * 8, d_out_scal, sw * 8, sw * 8, nseg, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SOSGPU_OK;
}

extern "C" int sosgpu_unpack(sosgpu_ctx *cx, int nseg, const double *d_buf, double *d_out_rec, double *d_out_scal, void *stream)
{
    if (!cx || nseg < 1 || !d_out_rec || !d_out_scal || !d_buf) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    const size_t nel = (size_t)(cx->d.smax + 1) * 3 * cx->d.w, sw = SOSGPU_SCAL_BASE + cx->d.n, row = nel + sw;
    HIPCHK(hipMemcpy2DAsync(d_out_rec, nel * 8, d_buf, row * 8, nel * 8, nseg, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(hipMemcpy2DAsync(d_out_scal, sw * 8, d_buf + nel, row * 8, sw * 8, nseg, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SOSGPU_OK;
}

// the two MAX-combined scalars of every segment are saved before the SUM all-reduce and restored from their own MAX
// all-reduce afterwards
__global__ void k_reduce_save(int nseg, size_t row, size_t off, double *buf, double *mx, int restore)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * nseg) return;
    double *p = buf + (size_t)(i / 2) * row + off + 7 + (i & 1);
    if (restore) *p = mx[i]; else mx[i] = *p;
}

extern "C" int sosgpu_reduce(sosgpu_ctx *cx, void *comm, int nseg, double *d_buf, void *stream)
{
    if (!cx || nseg < 1 || !d_buf) return SOSGPU_E_ARG;
    if (!comm) return SOSGPU_OK;                  // single rank
    if (int rc = rccl_load()) return rc;
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nel = (size_t)(cx->d.smax + 1) * 3 * cx->d.w, row = nel + SOSGPU_SCAL_BASE + cx->d.n;
    TmpBuf mxb(cx->device, (size_t)2 * nseg * sizeof(double));
    if (!mxb.p) return SOSGPU_E_HIP;
    double *mx = (double *)mxb.p;
    k_reduce_save<<<(2 * nseg + 63) / 64, 64, 0, st>>>(nseg, row, nel, d_buf, mx, 0);
    const int ncclDouble = 8, ncclSum = 0, ncclMax = 2;    // nccl.h enumerators (ncclFloat64 = 8)
    int bad = g_rccl.AllReduce(d_buf, d_buf, row * nseg, ncclDouble, ncclSum, comm, st);
    bad |= g_rccl.AllReduce(mx, mx, (size_t)2 * nseg, ncclDouble, ncclMax, comm, st);
    k_reduce_save<<<(2 * nseg + 63) / 64, 64, 0, st>>>(nseg, row, nel, d_buf, mx, 1);
    hipError_t e = hipStreamSynchronize(st);
    if (bad) return SOSGPU_E_RCCL;
    HIPCHK(e);
    return SOSGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// Cox-Munk glitter: host part = SOS_MAT_FRESNEL (SOS_SURFACE.F:1235-1603), O(N*OS_NS) flops and a
// 4(E15.8) text round trip (:1552 write, :1822 read) that has to be reproduced digit for digit.
// ---------------------------------------------------------------------------------------------
static double through_e15_8(double x)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.7E", x);   // 8 significant digits, round to nearest = Fortran E15.8
    return strtod(buf, nullptr);
}

static double sigma2_of_wind(double wind) { return (double)0.003f + (double)0.00512f * wind; }   // SOS_GLITTER.F:300

extern "C" int sosgpu_mat_fresnel_host(int n, const double *mu, const double *chr, double ind, int os_ns, double *out)
{
    if (n < 1 || os_ns < 2 || !mu || !chr || !out) return SOSGPU_E_ARG;
    const int K = os_ns + 1;
    double *alpha = out, *beta = out + K, *gamma = out + 2 * K, *zeta = out + 3 * K;
    std::vector<double> delta(K, 0.), pl(os_ns + 3, 0.), pol(os_ns + 2, 0.), r11(2 * n), r12(2 * n), r33(2 * n), xm(2 * n), xw(2 * n);
    for (int k = 0; k < 4 * K; k++) out[k] = 0.;
    // directions in the reference loop order J = -N..-1, 1..N (SOS_SURFACE.F:1346)
    for (int q = 0; q < 2 * n; q++) {
        const int j = q < n ? -(n - q) : q - n + 1;
        xm[q] = j > 0 ? mu[j - 1] : -mu[-j - 1];
        xw[q] = j > 0 ? chr[j - 1] : chr[-j - 1];
        double c = sqrt(.5 * (1 + xm[q]));
        const double a = sqrt(ind * ind - 1.0 + c * c);
        const double b = ind * ind * c;
        const double rl = -(b - a) / (b + a);
        const double rr = (c - a) / (c + a);
        r11[q] = .5 * (rl * rl + rr * rr);
        r12[q] = .5 * (rl * rl - rr * rr);
        r33[q] = rl * rr;
    }
    double *PL = pl.data() + 1;   // PL(-1:OS_NS+1)
    for (int q = 0; q < 2 * n; q++) {            // :1387-1400
        const double x = r11[q] * xw[q], xrmu = xm[q];
        PL[-1] = 0.; PL[0] = 1.;
        for (int k = 0; k <= os_ns; k++) {
            PL[k + 1] = ((2 * k + 1.) * xrmu * PL[k] - k * PL[k - 1]) / (k + 1.);
            beta[k] = beta[k] + x * PL[k];
        }
    }
    for (int k = 0; k <= os_ns; k++) beta[k] = (2 * k + 1) * beta[k] * .5;
    for (int q = 0; q < 2 * n; q++) {            // :1433-1456
        const double xxx = xw[q] * r12[q], xx = xw[q] * r33[q], xrmu = xm[q];
        pol[0] = 0.; pol[1] = 0.;
        PL[-1] = 0.; PL[0] = 1.;
        pol[2] = 3. * (1. - xrmu * xrmu) / 2. / sqrt(6.0);
        for (int k = 2; k <= os_ns; k++) {
            const double d = (2. * k + 1.) / sqrt(1.0 * (k + 3.) * (k - 1.));
            const double e = sqrt(1.0 * (k + 2.) * (k - 2.)) / (2. * k + 1.);
            pol[k + 1] = d * (xrmu * pol[k] - e * pol[k - 1]);
            gamma[k] = gamma[k] + xxx * pol[k];
        }
        for (int k = 0; k <= os_ns; k++) {
            PL[k + 1] = ((2. * k + 1.) * xrmu * PL[k] - k * PL[k - 1]) / (k + 1.);
            delta[k] = delta[k] + xx * PL[k];
        }
    }
    for (int k = 0; k <= os_ns; k++) {
        delta[k] = delta[k] * (2. * k + 1.) * .5;
        gamma[k] = gamma[k] * (2. * k + 1.) * .5;
    }
    for (int i = 2; i <= os_ns; i++) {           // :1521-1546 ; CO1, CO2 are REAL*4 expressions
        const float co1f = 4 * (2 * i + 1.f) / (float)i / (i - 1.f) / (i + 1.f) / (i + 2.f);
        const float co2f = i * (i - 1.f) / ((i + 1.f) * (i + 2.f));
        const double co1 = co1f;
        double co2 = co2f;
        const double co3 = co2 * delta[i];
        co2 = co2 * beta[i];
        const int nn = (int)(i * .5f), mm = (int)((i - 1) * .5f);
        double som1 = 0., som2 = 0., som3 = 0., som4 = 0.;
        for (int j = 1; j <= nn; j++) {
            const double x2 = (double)((i - 1.f) * (i - 1.f) - 3.f * (2 * j - 1.f) * (i - j));
            som1 = som1 + x2 * beta[i - 2 * j];
            som2 = som2 + x2 * delta[i - 2 * j];
        }
        for (int j = 0; j <= mm; j++) {
            const double x2 = (double)((i - 1.f) * (i - 1.f) - 3.f * j * (2 * i - 2 * j - 1.f));
            som3 = som3 + x2 * beta[i - 2 * j - 1];
            som4 = som4 + x2 * delta[i - 2 * j - 1];
        }
        zeta[i] = co3 - co1 * (som2 - som3);
        alpha[i] = co2 - co1 * (som1 - som4);
    }
    for (int k = 0; k < 4 * K; k++) out[k] = through_e15_8(out[k]);
    return SOSGPU_OK;
}

extern "C" int sosgpu_glitter(int device, int n, const double *mu, const double *chr, double wind, double ind,
                              int os_nb, int os_ns, int os_nm, float *d_rsurf, int32_t *d_il, double *d_e, void *stream)
{
    if (n < 1 || n > 85 || !mu || !chr || !d_rsurf || !d_il || !d_e) return SOSGPU_E_ARG;
    if (os_nb < 0 || os_ns < 2 || os_nm < os_nb + os_ns || os_nm > 2000) return SOSGPU_E_ARG;
    if (mat_reflexion_lds_bytes(os_ns, os_nm) > kLdsMaxBytes) return SOSGPU_E_ARG;    // k_mat_reflexion could not be launched
    if (const int rc = use_device(device)) return rc;
    std::vector<double> fcoef((size_t)4 * (os_ns + 1));
    int rc = sosgpu_mat_fresnel_host(n, mu, chr, ind, os_ns, fcoef.data());
    if (rc) return rc;
    const size_t cnt = (size_t)n + fcoef.size();
    TmpBuf tb(device, cnt * sizeof(double));
    if (!tb.p) return SOSGPU_E_HIP;
    double *d_buf = (double *)tb.p;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(d_buf, mu, n * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_buf + n, fcoef.data(), fcoef.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        launch_glitter(n, d_buf, sigma2_of_wind(wind), os_nb, os_ns, os_nm, d_buf + n, d_il, d_e, d_rsurf, st);
        e = hipGetLastError();
    }
    HIPCHK(finish_sync(e, st));
    return SOSGPU_OK;
}

static LandTerms land_terms(const sosgpu_land *land)
{
    LandTerms t;
    memset(&t, 0, sizeof t);
    if (land && land->isurf >= 3) {
        t.iroujean = 1;
        t.irondeaux = land->isurf == 4; t.ibreon = land->isurf == 5; t.imaignan = land->isurf == 7;
        t.k0 = land->k0; t.k1 = land->k1; t.k2 = land->k2; t.coef_c = land->coef_c;
    }
    return t;
}

extern "C" int sosgpu_trphi(sosgpu_ctx *cx, int nf, const double *d_rec, double tau, double tauout, int nphi,
                            const double *d_phi, int igli, double wind, const sosgpu_land *land, double *d_out, void *stream)
{
    if (!cx || nf < 1 || nf > cx->d.smax + 1 || !d_rec || nphi < 1 || !d_phi || !d_out) return SOSGPU_E_ARG;
    if (land && (land->isurf < 3 || land->isurf > 7)) return SOSGPU_E_ARG;
    if (land && land->isurf == 6) return SOSGPU_E_UNSUPPORTED;       // Nadal: refused by the reference's SOS_PROC as well
    HIPCHK(hipSetDevice(cx->device));
    launch_trphi(cx->d, nf, d_rec, tau, tauout, nphi, d_phi, igli, sigma2_of_wind(wind), cx->ind_surf, land_terms(land), d_out,
                 (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    note_stream(cx, (hipStream_t)stream);       // the kernel reads the context's mu: sosgpu_destroy waits for this stream
    return SOSGPU_OK;
}

extern "C" size_t sosgpu_trphi_spectrum_work_bytes(int njobs)
{
    static_assert(sizeof(TrphiJobDev) % 8 == 0, "entries of pointers and doubles");
    return njobs > 0 && njobs <= 65535 ? (size_t)njobs * sizeof(TrphiJobDev) : 0;
}

// sosgpu_trphi of njobs (context, record, azimuth range) jobs in ONE launch (k_trphi_table).  d_work = the job entries, filled
// by one copy from a recycled pinned block (Staged).  Everything is checked before anything is queued.
extern "C" int sosgpu_trphi_spectrum(const sosgpu_trphi_job *jobs, int njobs, const double *d_phi, int nphi_total,
                                     double *d_out, void *d_work, size_t work_bytes, void *stream)
{
    if (!jobs || !d_phi || !d_out || njobs < 0 || njobs > 65535) return SOSGPU_E_ARG;
    const size_t need = sosgpu_trphi_spectrum_work_bytes(njobs);
    if (!work_area_ok(d_work, work_bytes, need)) return SOSGPU_E_ARG;
    if (njobs == 0) return SOSGPU_OK;
    long long nblocks = 0;
    int w_max = 0;
    bool nadal = false;
    for (int i = 0; i < njobs; i++) {
        const sosgpu_trphi_job &j = jobs[i];
        if (!j.cx || !j.d_rec || j.cx->device != jobs[0].cx->device) return SOSGPU_E_ARG;
        if (j.nf < 1 || j.nf > j.cx->d.smax + 1) return SOSGPU_E_ARG;
        if (j.nphi < 1 || j.phi_off < 0 || (long long)j.phi_off + j.nphi > (long long)nphi_total) return SOSGPU_E_ARG;
        if (j.land && (j.land->isurf < 3 || j.land->isurf > 7)) return SOSGPU_E_ARG;
        nadal = nadal || (j.land && j.land->isurf == 6);
        nblocks += j.nphi;
        w_max = std::max(w_max, j.cx->d.w);
    }
    if (nblocks > 0x7fffffffLL) return SOSGPU_E_ARG;                 // (one grid dimension, first_block an int32)
    if (nadal) return SOSGPU_E_UNSUPPORTED;                          // Nadal: refused by the reference's SOS_PROC as well
    HIPCHK(hipSetDevice(jobs[0].cx->device));
    Staged s(jobs[0].cx->device, need);
    if (s.rc) return s.rc;
    TrphiJobDev *tab = static_cast<TrphiJobDev *>(s.host());
    int first = 0;
    double *out = d_out;
    for (int i = 0; i < njobs; i++) {
        const sosgpu_trphi_job &j = jobs[i];
        const SosDev &d = j.cx->d;
        TrphiJobDev &e = tab[i];
        e.n = d.n; e.w = d.w; e.n0 = d.n0; e.ipolar = d.ipolar; e.ifresnel = d.ifresnel;
        e.nf = j.nf; e.igli = j.igli; e.first_block = first;
        e.mu = d.mu; e.rec = j.d_rec; e.phis = d_phi + j.phi_off; e.out = out;
        e.ind_surf = j.cx->ind_surf; e.sigma2 = sigma2_of_wind(j.wind); e.tau = j.tau; e.tauout = j.tauout;
        e.land = land_terms(j.land);
        first += j.nphi;
        out += (size_t)j.nphi * 7 * d.w;
    }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(s.send(d_work, st));
    launch_trphi_table(static_cast<const TrphiJobDev *>(d_work), njobs, (int)nblocks, w_max, st);
    HIPCHK(hipGetLastError());
    for (int i = 0; i < njobs; i++) note_stream(jobs[i].cx, st);
    return SOSGPU_OK;
}

extern "C" int sosgpu_level_flux(sosgpu_ctx *cx, const double *d_rec, double *d_out, void *stream)
{
    if (!cx || !d_rec || !d_out) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    launch_level_flux(cx->d, d_rec, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    note_stream(cx, (hipStream_t)stream);       // the kernel reads the context's mu and ga: sosgpu_destroy waits for this stream
    return SOSGPU_OK;
}

extern "C" size_t sosgpu_level_flux_spectrum_work_bytes(int njobs)
{
    static_assert(sizeof(FluxJobDev) % 8 == 0, "entries of pointers");
    return njobs > 0 && njobs <= 0x3fffffff ? (size_t)njobs * sizeof(FluxJobDev) : 0;    // (2 njobs threads, an int32)
}

// sosgpu_level_flux of njobs (context, record) jobs in ONE launch (k_level_flux_table).  d_work = the job entries, filled by one
// copy from a recycled pinned block (Staged).  Everything is checked before anything is queued.
extern "C" int sosgpu_level_flux_spectrum(const sosgpu_flux_job *jobs, int njobs, double *d_out, void *d_work, size_t work_bytes,
                                          void *stream)
{
    if (!jobs || !d_out || njobs < 0 || njobs > 0x3fffffff) return SOSGPU_E_ARG;
    const size_t need = sosgpu_level_flux_spectrum_work_bytes(njobs);
    if (!work_area_ok(d_work, work_bytes, need)) return SOSGPU_E_ARG;
    if (njobs == 0) return SOSGPU_OK;
    for (int i = 0; i < njobs; i++)
        if (!jobs[i].cx || !jobs[i].d_rec) return SOSGPU_E_ARG;
    for (int i = 1; i < njobs; i++)
        if (jobs[i].cx->device != jobs[0].cx->device) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(jobs[0].cx->device));
    Staged s(jobs[0].cx->device, need);
    if (s.rc) return s.rc;
    FluxJobDev *tab = static_cast<FluxJobDev *>(s.host());
    for (int i = 0; i < njobs; i++) {
        const SosDev &d = jobs[i].cx->d;
        FluxJobDev &e = tab[i];
        e.n = d.n; e.n0 = d.n0; e.mu = d.mu; e.ga = d.ga; e.rec = jobs[i].d_rec; e.out = d_out + 2 * (size_t)i;
    }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(s.send(d_work, st));
    launch_level_flux_table(static_cast<const FluxJobDev *>(d_work), njobs, st);
    HIPCHK(hipGetLastError());
    for (int i = 0; i < njobs; i++) note_stream(jobs[i].cx, st);
    return SOSGPU_OK;
}

// Actinic flux and absorbed power at the output slots of a levels solve (k_level_absorption): one launch, no allocation.
// Everything is checked before anything is queued.
extern "C" int sosgpu_level_absorption(sosgpu_ctx *cx, const void *d_table, const int32_t *d_ctx_of_bin, int nb, int lp,
                                       const int32_t *d_nt, const double *d_prof, const double *d_zprof, int nz,
                                       const int32_t *d_jout, const double *d_zz, const double *d_tauout, const double *d_rec,
                                       const int32_t *d_norders, int nseg, const int32_t *d_seg, const double *d_aik,
                                       double *d_out, void *stream)
{
    if (!cx || !d_nt || !d_prof || !d_zprof || !d_jout || !d_zz || !d_tauout || !d_rec || !d_norders || !d_seg || !d_aik || !d_out)
        return SOSGPU_E_ARG;
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS || lp < 2 || nb < 0 || nseg < 0) return SOSGPU_E_ARG;
    if (d_table && !d_ctx_of_bin) return SOSGPU_E_ARG;
    if (nb == 0 || nseg == 0) return SOSGPU_OK;
    HIPCHK(hipSetDevice(cx->device));
    launch_level_absorption(cx->d, static_cast<const SosDev *>(d_table), d_ctx_of_bin, nb, lp, d_nt, d_prof, d_zprof, nz, d_jout,
                            d_zz, d_tauout, d_rec, d_norders, nseg, d_seg, d_aik, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    note_stream(cx, (hipStream_t)stream);       // the kernel reads the context's mu and ga: sosgpu_destroy waits for this stream
    return SOSGPU_OK;
}

// Every irradiance quantity at the output slots of a levels solve (k_level_irradiance): one launch, no allocation, no work
// area.  Everything is checked before anything is queued.
extern "C" int sosgpu_level_irradiance(sosgpu_ctx *cx, const void *d_table, const int32_t *d_ctx_of_bin, int nb, int lp,
                                       const int32_t *d_nt, const double *d_prof, const double *d_zprof, int nz,
                                       const int32_t *d_jout, const double *d_zz, const double *d_tauout, const double *d_rec,
                                       const int32_t *d_norders, const double *d_flux, const double *d_scal,
                                       const double *d_tauvrai, int nseg, const int32_t *d_seg, const double *d_aik,
                                       double *d_out, void *stream)
{
    if (!cx || !d_nt || !d_prof || !d_zprof || !d_jout || !d_zz || !d_tauout || !d_rec || !d_norders || !d_seg || !d_aik || !d_out)
        return SOSGPU_E_ARG;
    if (!d_flux || !d_scal) return SOSGPU_E_ARG;
    if (nz < 1 || nz > SOSGPU_MAX_OUTPUT_LEVELS || lp < 2 || nb < 0 || nseg < 0) return SOSGPU_E_ARG;
    if (d_table && !d_ctx_of_bin) return SOSGPU_E_ARG;
    if (nb == 0 || nseg == 0) return SOSGPU_OK;
    HIPCHK(hipSetDevice(cx->device));
    launch_level_irradiance(cx->d, static_cast<const SosDev *>(d_table), d_ctx_of_bin, nb, lp, d_nt, d_prof, d_zprof, nz, d_jout,
                            d_zz, d_tauout, d_rec, d_norders, d_flux, d_scal, d_tauvrai, nseg, d_seg, d_aik, d_out,
                            (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    note_stream(cx, (hipStream_t)stream);       // the kernel reads the context's mu and ga: sosgpu_destroy waits for this stream
    return SOSGPU_OK;
}

static bool channel_shape_ok(int nchan, int nslots, int nphi, int w)
{
    if (nchan < 1 || nchan > 65535 || nslots < 1 || nslots > 65535 || nphi < 1 || w < 1) return false;   // (grid y and z)
    return (long long)nphi * 7 * w <= 0x7fffffffLL;                                                    // (element index an int32)
}

// the term table in the work area: wgt[nterms] | first[nchan + 1] | job[nterms], rounded up to 8 bytes
namespace {
struct ChannelLayout { size_t wgt, first, job, total; };
ChannelLayout channel_layout(int nchan, int nterms)
{
    WorkLayout w;
    ChannelLayout L;
    L.wgt = w.take((size_t)nterms * sizeof(double), 8);
    L.first = w.take(((size_t)nchan + 1) * sizeof(int32_t), 4);
    L.job = w.take((size_t)nterms * sizeof(int32_t), 8);
    L.total = w.total;
    return L;
}
}   // namespace

extern "C" size_t sosgpu_channel_accumulate_work_bytes(int nchan, int nterms)
{
    return nchan < 1 || nterms < 0 ? 0 : channel_layout(nchan, nterms).total;
}

// The terms of nchan channels onto the accumulator in ONE launch (k_channel_accumulate).  d_work = the term table, filled by one
// copy from a recycled pinned block (Staged).  Everything is checked before anything is queued.
extern "C" int sosgpu_channel_accumulate(int device, const double *d_blocks, int njobs, int nslots, int nphi, int w, int nchan,
                                         const int32_t *first, const int32_t *job, const double *wgt, double *d_acc,
                                         void *d_work, size_t work_bytes, void *stream)
{
    if (!d_blocks || !first || !job || !wgt || !d_acc || !d_work || njobs < 1) return SOSGPU_E_ARG;
    if (!channel_shape_ok(nchan, nslots, nphi, w)) return SOSGPU_E_ARG;
    if (first[0] != 0) return SOSGPU_E_ARG;
    for (int c = 0; c < nchan; c++)
        if (first[c + 1] < first[c]) return SOSGPU_E_ARG;
    const int nterms = first[nchan];
    for (int m = 0; m < nterms; m++)
        if (job[m] < 0 || job[m] >= njobs || !std::isfinite(wgt[m])) return SOSGPU_E_ARG;
    const ChannelLayout L = channel_layout(nchan, nterms);
    if (!work_area_ok(d_work, work_bytes, L.total)) return SOSGPU_E_ARG;
    if (nterms == 0) return SOSGPU_OK;
    if (const int rc = use_device(device)) return rc;
    Staged s(device, L.total);
    if (s.rc) return s.rc;
    char *hp = static_cast<char *>(s.host());
    const size_t job_end = L.job + (size_t)nterms * sizeof(int32_t);
    memcpy(hp + L.wgt, wgt, (size_t)nterms * sizeof(double));
    memcpy(hp + L.first, first, ((size_t)nchan + 1) * sizeof(int32_t));
    memcpy(hp + L.job, job, (size_t)nterms * sizeof(int32_t));
    memset(hp + job_end, 0, L.total - job_end);                        // (the padding to 8 bytes)
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(s.send(d_work, st));
    const char *dp = static_cast<const char *>(d_work);
    launch_channel_accumulate(d_blocks, nslots, nphi, w, nchan, reinterpret_cast<const int32_t *>(dp + L.first),
                              reinterpret_cast<const int32_t *>(dp + L.job), reinterpret_cast<const double *>(dp + L.wgt), d_acc, st);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_channel_finish(int device, const double *d_acc, const double *d_angdiff_block, int nchan, int nslots,
                                     int nphi, int w, double *d_out, void *stream)
{
    if (!d_acc || !d_angdiff_block || !d_out || !channel_shape_ok(nchan, nslots, nphi, w) || w < 3 || !(w & 1)) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    launch_channel_finish(d_acc, d_angdiff_block, nchan, nslots, nphi, w, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_land_surface(int device, const sosgpu_land *land, int n, const double *mu, const double *chr, double ind,
                                   int os_nb, int os_ns, int os_nm, float *d_rsurf, int32_t *ier_out, void *stream)
{
    if (!land || land->isurf < 3 || land->isurf > 7 || n < 1 || n > 85 || !mu || !chr || !d_rsurf) return SOSGPU_E_ARG;
    if (land->isurf == 6) return SOSGPU_E_UNSUPPORTED;               // Nadal: refused by the reference's SOS_PROC as well
    if (os_nb < 0 || os_ns < 2 || os_nm < os_nb + os_ns || os_nm > 2000) return SOSGPU_E_ARG;
    if (mat_reflexion_lds_bytes(os_ns, os_nm) > kLdsMaxBytes) return SOSGPU_E_ARG;    // k_mat_reflexion could not be launched
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> fcoef((size_t)4 * (os_ns + 1), 0.);
    if (land->isurf > 3) {
        int rc = sosgpu_mat_fresnel_host(n, mu, chr, ind, os_ns, fcoef.data());
        if (rc) return rc;
    }
    const size_t npairs = (size_t)n * (n + 1) / 2, nn = (size_t)n * n, cnt = (size_t)(os_nb + 1) * 9 * nn;
    // one allocation: mu | fcoef | e_nn [N^2][os_nb+1] | e [npairs][os_nm+1] | il_nn, il, err (int32) | tmp matrices (float)
    const size_t nd = (size_t)n + fcoef.size() + nn * (os_nb + 1) + npairs * (os_nm + 1);
    const size_t ni = nn + npairs + 2;
    TmpBuf tb(device, nd * 8 + ni * 4 + cnt * 4 + 64);
    if (!tb.p) return SOSGPU_E_HIP;
    char *buf = (char *)tb.p;
    double *d_mu = (double *)buf, *d_fc = d_mu + n, *d_enn = d_fc + fcoef.size(), *d_e = d_enn + nn * (os_nb + 1);
    int32_t *d_ilnn = (int32_t *)(d_e + npairs * (os_nm + 1)), *d_il = d_ilnn + nn, *d_err = d_il + npairs;
    float *d_tmp = (float *)(d_err + 2);
    int32_t err[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(d_mu, mu, n * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_fc, fcoef.data(), fcoef.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 2 * sizeof(int32_t), st);
    if (e == hipSuccess) {
        launch_land(land->isurf, n, d_mu, land->k0, land->k1, land->k2, land->coef_c, os_nb, os_ns,
                    os_nm, d_fc, d_enn, d_ilnn, d_e, d_il, d_tmp, d_rsurf, d_err, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(err, d_err, sizeof err, hipMemcpyDeviceToHost, st);
    HIPCHK(finish_sync(e, st));
    if (ier_out) *ier_out = err[0] ? -1 : 0;
    return SOSGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// sosgpu_surface_batch: the two entry points above for many jobs on one angle set.  The host finds the distinct parameter sets
// (exact equality of the doubles, compared as bit patterns), lays the work area out and fills the tables; the device side is
// the table forms of the same kernels (glitter.hip, land.hip) and one compose kernel.
// Work area, every section 8-byte aligned; [tables] travel in the one staged copy:
//   [ mu[n] | fcoef[nind][4][os_ns+1] | sigma2[nwind] | C[nmaignan] | SurfReflSet[nrefl] | SurfTriple[ntrip] | SurfJobDev[njobs]
//     | model[nconst] | flag[ntrip] (zero) ]
//   il[nan][npairs] | e[nan][npairs][os_nm+1] | il_nn[ntrip][n^2] | e_nn[ntrip][n^2][os_nb+1] | refl[nrefl][os_nb+1][9][n][n]
// nan = nwind + nmaignan + nconst analyses, in that order.
// ---------------------------------------------------------------------------------------------
namespace {
struct SurfacePlan {
    std::vector<double> winds, cs, inds;             // distinct values, in order of first appearance
    std::vector<int32_t> models;                     // constant analyses present: 0 Rondeaux-Herman, 1 Breon
    std::vector<SurfReflSet> refl;
    std::vector<SurfTriple> trip;
    std::vector<int32_t> job_refl, job_trip;         // per job, -1: none
    size_t o_fc, o_par0, o_par1, o_refl, o_trip, o_jobs, o_models, o_flags, table_bytes;
    size_t o_il, o_e, o_ilnn, o_enn, o_rb, total;
    int nan() const { return (int)(winds.size() + cs.size() + models.size()); }
};

uint64_t dbl_bits(double v) { uint64_t b; memcpy(&b, &v, sizeof b); return b; }

// the refusals that need no device, and the plan; SOSGPU_OK, SOSGPU_E_ARG or SOSGPU_E_UNSUPPORTED
int surface_plan(int n, int os_nb, int os_ns, int os_nm, const sosgpu_surface_job *jobs, int njobs, SurfacePlan *pl)
{
    if (n < 1 || n > 85 || !jobs || njobs < 0 || njobs > 65535) return SOSGPU_E_ARG;
    if (os_nb < 0 || os_ns < 2 || os_nm < os_nb + os_ns || os_nm > 2000) return SOSGPU_E_ARG;
    if (mat_reflexion_lds_bytes(os_ns, os_nm) > kLdsMaxBytes) return SOSGPU_E_ARG;    // k_mat_reflexion could not be launched
    bool nadal = false;
    for (int j = 0; j < njobs; j++) {
        const int s = jobs[j].isurf;
        if (s != 1 && (s < 3 || s > 7)) return SOSGPU_E_ARG;
        nadal = nadal || s == 6;
    }
    if (nadal) return SOSGPU_E_UNSUPPORTED;          // Nadal: refused by the reference's SOS_PROC as well
    std::map<uint64_t, int> wind_of, c_of, ind_of;
    std::map<std::pair<int, int>, int> refl_of;      // (analysis key, ind) -> block; analysis key: see below
    std::map<std::vector<uint64_t>, int> trip_of;
    auto distinct = [](std::map<uint64_t, int> &m, std::vector<double> &v, double x) {
        auto it = m.find(dbl_bits(x));
        if (it != m.end()) return it->second;
        v.push_back(x);
        return m[dbl_bits(x)] = (int)v.size() - 1;
    };
    int const_of[2] = {-1, -1};
    // first pass: the analyses, so that their final indices (winds, then Maignan, then constant) are known
    struct Need { int kind, idx, ind; };             // kind 0 Cox-Munk, 1 Maignan, 2 constant, -1 none
    std::vector<Need> need(njobs);
    for (int j = 0; j < njobs; j++) {
        const sosgpu_surface_job &jb = jobs[j];
        Need &q = need[j];
        q.kind = -1; q.idx = q.ind = 0;
        if (jb.isurf == 1) { q.kind = 0; q.idx = distinct(wind_of, pl->winds, jb.wind); }
        else if (jb.isurf == 7) { q.kind = 1; q.idx = distinct(c_of, pl->cs, jb.coef_c); }
        else if (jb.isurf == 4 || jb.isurf == 5) {
            const int m = jb.isurf == 4 ? 0 : 1;
            if (const_of[m] < 0) { const_of[m] = (int)pl->models.size(); pl->models.push_back(m); }
            q.kind = 2; q.idx = const_of[m];
        }
        if (q.kind >= 0) q.ind = distinct(ind_of, pl->inds, jb.ind);
    }
    const int nwind = (int)pl->winds.size(), ncm = (int)pl->cs.size();
    pl->job_refl.assign(njobs, -1);
    pl->job_trip.assign(njobs, -1);
    for (int j = 0; j < njobs; j++) {
        const sosgpu_surface_job &jb = jobs[j];
        const Need &q = need[j];
        if (q.kind >= 0) {
            const int an = q.kind == 0 ? q.idx : q.kind == 1 ? nwind + q.idx : nwind + ncm + q.idx;
            auto it = refl_of.find({an, q.ind});
            if (it == refl_of.end()) {
                SurfReflSet r;
                r.coef = q.kind == 0 ? 1. / sigma2_of_wind(pl->winds[q.idx]) : 1.0;
                r.analysis = an; r.ind = q.ind;
                pl->refl.push_back(r);
                it = refl_of.emplace(std::make_pair(an, q.ind), (int)pl->refl.size() - 1).first;
            }
            pl->job_refl[j] = it->second;
        }
        if (jb.isurf >= 3) {
            const std::vector<uint64_t> key = {dbl_bits(jb.k0), dbl_bits(jb.k1), dbl_bits(jb.k2)};
            auto it = trip_of.find(key);
            if (it == trip_of.end()) {
                pl->trip.push_back({jb.k0, jb.k1, jb.k2});
                it = trip_of.emplace(key, (int)pl->trip.size() - 1).first;
            }
            pl->job_trip[j] = it->second;
        }
    }
    const size_t npairs = (size_t)n * (n + 1) / 2, nn = (size_t)n * n, cnt = (size_t)(os_nb + 1) * 9 * nn;
    const size_t nan = (size_t)pl->nan(), ntrip = pl->trip.size(), nrefl = pl->refl.size();
    WorkLayout w;
    w.take((size_t)n * 8, 8);                                  // mu, at the start of the area
    pl->o_fc = w.take(pl->inds.size() * 4 * (os_ns + 1) * 8, 8);
    pl->o_par0 = w.take((size_t)nwind * 8, 8);
    pl->o_par1 = w.take((size_t)ncm * 8, 8);
    pl->o_refl = w.take(nrefl * sizeof(SurfReflSet), 8);
    pl->o_trip = w.take(ntrip * sizeof(SurfTriple), 8);
    pl->o_jobs = w.take((size_t)njobs * sizeof(SurfJobDev), 8);
    pl->o_models = w.take(pl->models.size() * 4, 8);
    pl->o_flags = w.take(ntrip * 4, 8);
    pl->table_bytes = w.total;                                 // (what travels in the staged copy)
    pl->o_il = w.take(nan * npairs * 4, 8);
    pl->o_e = w.take(nan * npairs * (os_nm + 1) * 8, 8);
    pl->o_ilnn = w.take(ntrip * nn * 4, 8);
    pl->o_enn = w.take(ntrip * nn * (os_nb + 1) * 8, 8);
    pl->o_rb = w.take(nrefl * cnt * 4, 8);
    pl->total = w.total;
    return SOSGPU_OK;
}
}   // namespace
static_assert(sizeof(SurfReflSet) % 8 == 0 && sizeof(SurfTriple) % 8 == 0 && sizeof(SurfJobDev) % 8 == 0, "8-byte sections");

extern "C" size_t sosgpu_surface_batch_work_bytes(int n, int os_nb, int os_ns, int os_nm, const sosgpu_surface_job *jobs, int njobs)
{
    SurfacePlan pl;
    if (surface_plan(n, os_nb, os_ns, os_nm, jobs, njobs, &pl) != SOSGPU_OK) return 0;
    return pl.total;
}

extern "C" int sosgpu_surface_batch(int device, int n, const double *mu, const double *chr, int os_nb, int os_ns, int os_nm,
                                    const sosgpu_surface_job *jobs, int njobs, int32_t *d_status, void *d_work,
                                    size_t work_bytes, void *stream)
{
    if (!mu || !chr || !d_status || !d_work) return SOSGPU_E_ARG;
    SurfacePlan pl;
    if (const int rc = surface_plan(n, os_nb, os_ns, os_nm, jobs, njobs, &pl)) return rc;
    for (int j = 0; j < njobs; j++)
        if (!jobs[j].d_rsurf) return SOSGPU_E_ARG;
    if (!work_area_ok(d_work, work_bytes, pl.total)) return SOSGPU_E_ARG;
    if (njobs == 0) return SOSGPU_OK;
    if (const int rc = use_device(device)) return rc;
    Staged s(device, pl.table_bytes);
    if (s.rc) return s.rc;
    char *hp = static_cast<char *>(s.host());
    char *dp = static_cast<char *>(d_work);
    const int nwind = (int)pl.winds.size(), ncm = (int)pl.cs.size(), nconst = (int)pl.models.size();
    const int nrefl = (int)pl.refl.size(), ntrip = (int)pl.trip.size();
    memset(hp + pl.o_models, 0, pl.table_bytes - pl.o_models);         // the flags, and the padding of both int sections
    memcpy(hp, mu, (size_t)n * sizeof(double));
    double *fc = reinterpret_cast<double *>(hp + pl.o_fc);
    for (size_t i = 0; i < pl.inds.size(); i++)
        if (const int rc = sosgpu_mat_fresnel_host(n, mu, chr, pl.inds[i], os_ns, fc + i * 4 * (os_ns + 1))) return rc;
    double *par0 = reinterpret_cast<double *>(hp + pl.o_par0);
    for (int i = 0; i < nwind; i++) par0[i] = sigma2_of_wind(pl.winds[i]);
    if (ncm) memcpy(hp + pl.o_par1, pl.cs.data(), (size_t)ncm * sizeof(double));
    if (nrefl) memcpy(hp + pl.o_refl, pl.refl.data(), (size_t)nrefl * sizeof(SurfReflSet));
    if (ntrip) memcpy(hp + pl.o_trip, pl.trip.data(), (size_t)ntrip * sizeof(SurfTriple));
    SurfJobDev *jt = reinterpret_cast<SurfJobDev *>(hp + pl.o_jobs);
    for (int j = 0; j < njobs; j++) {
        jt[j].out = jobs[j].d_rsurf; jt[j].isurf = jobs[j].isurf; jt[j].refl = pl.job_refl[j]; jt[j].trip = pl.job_trip[j];
        jt[j].pad = 0;
    }
    if (nconst) memcpy(hp + pl.o_models, pl.models.data(), (size_t)nconst * sizeof(int32_t));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(s.send(d_work, st));
    const double *d_mu = reinterpret_cast<const double *>(dp);
    const size_t npairs = (size_t)n * (n + 1) / 2;
    int32_t *d_il = reinterpret_cast<int32_t *>(dp + pl.o_il);
    double *d_e = reinterpret_cast<double *>(dp + pl.o_e);
    int32_t *d_flags = reinterpret_cast<int32_t *>(dp + pl.o_flags);
    double *d_enn = reinterpret_cast<double *>(dp + pl.o_enn);
    float *d_rb = reinterpret_cast<float *>(dp + pl.o_rb);
    if (nwind) launch_gsf_table(0, n, d_mu, reinterpret_cast<const double *>(dp + pl.o_par0), nwind, os_nm, d_il, d_e, st);
    if (ncm)
        launch_gsf_table(1, n, d_mu, reinterpret_cast<const double *>(dp + pl.o_par1), ncm, os_nm, d_il + (size_t)nwind * npairs,
                         d_e + (size_t)nwind * npairs * (os_nm + 1), st);
    if (nconst)
        launch_gsf_const_table(n, nconst, reinterpret_cast<const int32_t *>(dp + pl.o_models), d_mu, os_nm,
                               d_il + (size_t)(nwind + ncm) * npairs, d_e + (size_t)(nwind + ncm) * npairs * (os_nm + 1), st);
    if (nrefl)
        launch_mat_reflexion_table(n, d_mu, reinterpret_cast<const SurfReflSet *>(dp + pl.o_refl), nrefl, os_nb, os_ns, os_nm,
                                   reinterpret_cast<const double *>(dp + pl.o_fc), d_il, d_e, d_rb, st);
    if (ntrip)
        launch_fsf_table(n, d_mu, os_nb, reinterpret_cast<const SurfTriple *>(dp + pl.o_trip), ntrip,
                         reinterpret_cast<int32_t *>(dp + pl.o_ilnn), d_enn, d_flags, st);
    launch_surface_compose(n, os_nb, reinterpret_cast<const SurfJobDev *>(dp + pl.o_jobs), njobs, d_rb, d_enn, d_flags, d_status,
                           st);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// SOS_PROFILE on the device (profile.hip): the no-gas profile (SOS_PROFIL.F:349-489), the same for every bin of a wavelength, by
// one wavefront, the per-bin gas step by one wavefront per bin.
// ---------------------------------------------------------------------------------------------
namespace {
const int kOsNt = 600, kOsNtMin = 100;
const double kTcouche = (double)0.005f, kTFirst = (double)0.0002f;

// Level count and the two optical-depth steps of the no-gas profile (SOS_PROFIL.F:349-366): returns NT or -1 (more than
// CTE_OS_NT levels, or no scatterer at all).  The levels themselves are placed on the device (k_profile_nogas).
int profile_nogas_grid(double tr, double ta, double *t_first, double *t_layer)
{
    int nt;
    const double ttot = tr + ta;
    if ((ttot / kOsNtMin) <= kTFirst) { nt = kOsNtMin; *t_layer = ttot / nt; *t_first = *t_layer; }
    else if ((ttot / kOsNtMin) < kTcouche) { nt = kOsNtMin + 1; *t_first = kTFirst; *t_layer = (ttot - *t_first) / kOsNtMin; }
    else { *t_first = kTFirst; nt = (int)((ttot - *t_first) / kTcouche); *t_layer = (ttot - *t_first) / nt; nt = nt + 1; }
    if (nt > kOsNt || !(ttot > 0.)) return -1;
    return nt;
}
}  // namespace

extern "C" int sosgpu_profile_true(sosgpu_ctx *cx, int nb, double tr, double hr, double ta, double ha, int absprofil,
                                   int nblev, const double *d_altabs, const double *d_tabs,
                                   double a_tronc, double piz, double piztr, double zout, int lp,
                                   double *d_prof, int32_t *d_nt, int32_t *d_iborm, double *d_zprof,
                                   int32_t *d_jout, double *d_zz, double *d_scal, const double *d_nogas, double *d_hvrai,
                                   void *stream)
{
    if (!cx || nb < 1 || lp < 2 || !d_prof || !d_nt || !d_iborm || !d_zprof || !d_scal) return SOSGPU_E_ARG;
    if ((d_jout == nullptr) != (d_zz == nullptr)) return SOSGPU_E_ARG;
    if (d_tabs && (!d_altabs || nblev < 2)) return SOSGPU_E_ARG;
    if (d_tabs && nblev > SOS_PROF_NBLEV_MAX) return SOSGPU_E_UNSUPPORTED;
    if (!(hr > 0.) || !(ha > 0.) || tr < 0. || ta < 0.) return SOSGPU_E_ARG;
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t st = (hipStream_t)stream;
    const int NG = SOSGPU_NOGAS_LEVELS;
    double t_first = 0., t_layer = 0.;
    const int nt_ng = profile_nogas_grid(tr, ta, &t_first, &t_layer);
    if (nt_ng < 0) return SOSGPU_E_UNSUPPORTED;        // more than CTE_OS_NT levels (IER = -1 in the reference)
    if (lp <= nt_ng) return SOSGPU_E_ARG;
    // the no-gas profile is made on `stream` in front of the bins' kernel (unless the caller queued it earlier, sosgpu_profile_nogas):
    // nothing is waited for, so profiles, solve and aggregate of a wavelength queue up behind one another without a host stall
    const double *ngp = d_nogas;
    if (!ngp) {
        if (!cx->prof_ng) { if (int rc = dev_alloc(cx, &cx->prof_ng, (size_t)4 * NG)) return rc; }
        else if (cx->prof_ng_stream != st) HIPCHK(sync_ctx_streams(cx));    // an earlier call on another stream may still be reading it
        cx->prof_ng_stream = st;
        launch_profile_nogas(tr, hr, ta, ha, nt_ng, t_first, t_layer, cx->prof_ng, NG, st);
        HIPCHK(hipGetLastError());
        ngp = cx->prof_ng;
    }
    ProfileArgs a;
    a.nb = nb; a.lp = lp; a.nblev = nblev; a.absprofil = d_tabs ? absprofil : 7; a.smax = cx->d.smax; a.nt_ng = nt_ng;
    a.tr = tr; a.hr = hr; a.ta = ta; a.ha = ha; a.a_tronc = a_tronc; a.piz = piz; a.piztr = piztr; a.zout = zout;
    a.altabs = d_altabs; a.tabs = d_tabs;
    a.z_ng = ngp; a.h_ng = ngp + NG; a.pca_ng = ngp + 2 * NG; a.pcm_ng = ngp + 3 * NG;
    a.prof = d_prof; a.zprof = d_zprof; a.zz = d_zz; a.scal = d_scal; a.nt = d_nt; a.iborm = d_iborm; a.jout = d_jout;
    a.hvrai = d_hvrai;
    launch_profile(a, st);
    HIPCHK(hipGetLastError());
    note_stream(cx, st);
    return SOSGPU_OK;
}

extern "C" int sosgpu_profile(sosgpu_ctx *cx, int nb, double tr, double hr, double ta, double ha, int absprofil,
                              int nblev, const double *d_altabs, const double *d_tabs,
                              double a_tronc, double piz, double piztr, double zout, int lp,
                              double *d_prof, int32_t *d_nt, int32_t *d_iborm, double *d_zprof,
                              int32_t *d_jout, double *d_zz, double *d_scal, const double *d_nogas, void *stream)
{
    return sosgpu_profile_true(cx, nb, tr, hr, ta, ha, absprofil, nblev, d_altabs, d_tabs, a_tronc, piz, piztr, zout, lp, d_prof,
                               d_nt, d_iborm, d_zprof, d_jout, d_zz, d_scal, d_nogas, nullptr, stream);
}

extern "C" int sosgpu_profile_nogas(int device, double tr, double hr, double ta, double ha, double *d_nogas, void *stream)
{
    if (!d_nogas || !(hr > 0.) || !(ha > 0.) || tr < 0. || ta < 0.) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    double t_first = 0., t_layer = 0.;
    const int nt_ng = profile_nogas_grid(tr, ta, &t_first, &t_layer);
    if (nt_ng < 0) return SOSGPU_E_UNSUPPORTED;
    launch_profile_nogas(tr, hr, ta, ha, nt_ng, t_first, t_layer, d_nogas, SOSGPU_NOGAS_LEVELS, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_absprofile(int device, int nb, int nlev, int nterm, const int32_t *d_ik, const double *d_xk,
                                 const double *d_ro, double *d_tabs, void *stream)
{
    if (nb < 1 || nlev < 2 || nlev > SOS_PROF_NBLEV_MAX || nterm < 1 || !d_ik || !d_xk || !d_ro || !d_tabs) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    launch_absprofile(nb, nlev, nterm, d_ik, d_xk, d_ro, d_tabs, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// The profile stage of many wavelengths as three launches (profile.hip, the *_table kernels).
// ---------------------------------------------------------------------------------------------
// work area: the no-gas blocks [nwl][4][SOSGPU_NOGAS_LEVELS] | the per-wavelength table
namespace {
struct ProfileLayout { size_t nogas, tab, total; };
ProfileLayout profile_layout(int nwl)
{
    static_assert(sizeof(ProfileWl) % 8 == 0, "entries of doubles and int64");
    WorkLayout w;
    ProfileLayout L;
    L.nogas = w.take((size_t)nwl * 4 * SOSGPU_NOGAS_LEVELS * sizeof(double), 8);
    L.tab = w.take((size_t)nwl * sizeof(ProfileWl), 8);
    L.total = w.total;
    return L;
}
}   // namespace

extern "C" size_t sosgpu_profile_spectrum_work_bytes(int nwl) { return nwl < 1 ? 0 : profile_layout(nwl).total; }

extern "C" int sosgpu_profile_nogas_levels(double tr, double ta)
{
    double t_first = 0., t_layer = 0.;
    if (tr < 0. || ta < 0.) return -1;
    return profile_nogas_grid(tr, ta, &t_first, &t_layer);
}

extern "C" int sosgpu_profile_spectrum_true(int device, int nwl, const sosgpu_profile_wl *wl, int nb, const int32_t *d_wl_of_bin,
                                            const int32_t *d_ik, const double *d_gas, size_t gas_doubles, int nblev, int lp,
                                            void *d_work, size_t work_bytes, double *d_tabs, double *d_prof, int32_t *d_nt,
                                            int32_t *d_iborm, double *d_zprof, int32_t *d_jout, double *d_zz, double *d_scal,
                                            int *bad_wl, double *d_hvrai, void *stream)
{
    if (bad_wl) *bad_wl = -1;
    if (nwl < 1 || !wl || nb < 1 || lp < 2 || !d_wl_of_bin) return SOSGPU_E_ARG;
    const ProfileLayout L = profile_layout(nwl);
    if (!work_area_ok(d_work, work_bytes, L.total)) return SOSGPU_E_ARG;
    if (!d_prof || !d_nt || !d_iborm || !d_zprof || !d_scal) return SOSGPU_E_ARG;
    if ((d_jout == nullptr) != (d_zz == nullptr)) return SOSGPU_E_ARG;
    // --- the rules of sosgpu_profile / sosgpu_absprofile, per wavelength, before anything is queued
    std::vector<ProfileWl> tab((size_t)nwl);
    long long bins = 0;
    bool any_gas = false;
    for (int w = 0; w < nwl; w++) {
        const sosgpu_profile_wl &s = wl[w];
        ProfileWl &t = tab[w];
        if (bad_wl) *bad_wl = w;
        if (s.nbins < 1 || s.nterm < 0 || s.smax < 0) return SOSGPU_E_ARG;
        if (!(s.hr > 0.) || !(s.ha > 0.) || s.tr < 0. || s.ta < 0.) return SOSGPU_E_ARG;
        if (s.zout != -1.0 && !d_jout) return SOSGPU_E_ARG;
        if (s.nterm > 0) {
            any_gas = true;
            if (!d_gas || !d_ik || !d_tabs || nblev < 2) return SOSGPU_E_ARG;
            if (nblev > SOS_PROF_NBLEV_MAX) return SOSGPU_E_UNSUPPORTED;
            const long long nl1 = nblev - 1, gd = (long long)gas_doubles;
            if (s.xk_off < 0 || s.ro_off < 0 || s.alt_off < 0 || s.xk_off + 8ll * s.nterm * nl1 > gd || s.ro_off + 8 * nl1 > gd ||
                s.alt_off + nblev > gd)
                return SOSGPU_E_ARG;
        } else if (s.nbins != 1) return SOSGPU_E_ARG;
        t.tr = s.tr; t.hr = s.hr; t.ta = s.ta; t.ha = s.ha; t.a_tronc = s.a_tronc; t.piz = s.piz; t.piztr = s.piztr; t.zout = s.zout;
        t.t_first = 0.; t.t_layer = 0.;
        t.nt_ng = profile_nogas_grid(s.tr, s.ta, &t.t_first, &t.t_layer);
        if (t.nt_ng < 0) return SOSGPU_E_UNSUPPORTED;          // more than CTE_OS_NT levels (IER = -1 in the reference)
        if (lp <= t.nt_ng) return SOSGPU_E_ARG;
        t.xk_off = s.xk_off; t.ro_off = s.ro_off; t.alt_off = s.alt_off;
        t.nterm = s.nterm; t.absprofil = s.absprofil; t.smax = s.smax;
        bins += s.nbins;
    }
    if (bad_wl) *bad_wl = -1;
    if (bins != nb) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // --- the table: pinned block -> the work area on the caller's stream, nothing waited for
    Staged s(device, (size_t)nwl * sizeof(ProfileWl));
    if (s.rc) return s.rc;
    memcpy(s.host(), tab.data(), (size_t)nwl * sizeof(ProfileWl));
    char *dp = static_cast<char *>(d_work);
    HIPCHK(s.send(dp + L.tab, st));
    const ProfileWl *d_tab = reinterpret_cast<const ProfileWl *>(dp + L.tab);
    double *d_nogas = reinterpret_cast<double *>(dp + L.nogas);
    const int NG = SOSGPU_NOGAS_LEVELS;
    launch_profile_nogas_table(d_tab, nwl, d_nogas, NG, st);
    HIPCHK(hipGetLastError());
    if (any_gas) {
        launch_absprofile_table(d_tab, nwl, d_wl_of_bin, nb, nblev, d_ik, d_gas, d_tabs, st);
        HIPCHK(hipGetLastError());
    }
    ProfileTableArgs q;
    q.nb = nb; q.nwl = nwl; q.lp = lp; q.nblev = any_gas ? nblev : 0; q.ngl = NG;
    q.tab = d_tab; q.wl_of_bin = d_wl_of_bin; q.gas = d_gas; q.tabs = any_gas ? d_tabs : nullptr; q.nogas = d_nogas;
    q.prof = d_prof; q.zprof = d_zprof; q.zz = d_zz; q.scal = d_scal; q.nt = d_nt; q.iborm = d_iborm; q.jout = d_jout;
    q.hvrai = d_hvrai;
    launch_profile_table(q, st);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_profile_spectrum(int device, int nwl, const sosgpu_profile_wl *wl, int nb, const int32_t *d_wl_of_bin,
                                       const int32_t *d_ik, const double *d_gas, size_t gas_doubles, int nblev, int lp,
                                       void *d_work, size_t work_bytes, double *d_tabs, double *d_prof, int32_t *d_nt,
                                       int32_t *d_iborm, double *d_zprof, int32_t *d_jout, double *d_zz, double *d_scal,
                                       int *bad_wl, void *stream)
{
    return sosgpu_profile_spectrum_true(device, nwl, wl, nb, d_wl_of_bin, d_ik, d_gas, gas_doubles, nblev, lp, d_work, work_bytes,
                                        d_tabs, d_prof, d_nt, d_iborm, d_zprof, d_jout, d_zz, d_scal, bad_wl, nullptr, stream);
}

// COEFF_ABS_CKD of many wavelengths in one launch (ckd.hip): the per-wavelength table and the slot pointers go through one
// recycled pinned block into the caller's work area, the status words are cleared, the kernel is queued -- all on `stream`.
// work area: the per-wavelength table | the slot pointers
namespace {
struct CkdLayout { size_t tab, slots, total; };
CkdLayout ckd_layout(int nwl, int nslots)
{
    static_assert(sizeof(CkdWl) % 8 == 0, "the slot pointers follow the entries");
    WorkLayout w;
    CkdLayout L;
    L.tab = w.take((size_t)nwl * sizeof(CkdWl), 8);
    L.slots = w.take((size_t)nslots * sizeof(double *), 8);
    L.total = w.total;
    return L;
}
}   // namespace

extern "C" size_t sosgpu_ckd_layer_tables_work_bytes(int nwl, int nslots)
{
    return nwl < 1 || nslots < 1 ? 0 : ckd_layout(nwl, nslots).total;
}

extern "C" int sosgpu_ckd_layer_tables(int device, int nwl, const sosgpu_ckd_wl *wl, int nslots, const double *const *ki,
                                       const double *d_axes, size_t axes_doubles, int nlay, void *d_work, size_t work_bytes,
                                       double *d_out, size_t out_doubles, int32_t *d_status, int *bad_wl, void *stream)
{
    if (bad_wl) *bad_wl = -1;
    if (nwl < 1 || !wl || nslots < 1 || !ki || !d_axes || !d_out || !d_status) return SOSGPU_E_ARG;
    const CkdLayout L = ckd_layout(nwl, nslots);
    if (!work_area_ok(d_work, work_bytes, L.total)) return SOSGPU_E_ARG;
    if (nlay < 1 || nlay > SOS_CKD_NLAY_MAX) return SOSGPU_E_UNSUPPORTED;
    // --- limits and argument rules per wavelength, before anything is queued
    std::vector<CkdWl> tab((size_t)nwl);
    long long slots = 0;
    int max_slots = 0;
    const long long ad = (long long)axes_doubles, od = (long long)out_doubles;
    for (int w = 0; w < nwl; w++) {
        const sosgpu_ckd_wl &s = wl[w];
        CkdWl &t = tab[w];
        if (bad_wl) *bad_wl = w;
        if (s.nterm < 1 || s.nterm > 65535) return SOSGPU_E_ARG;
        if (s.nt < 2 || s.nt > SOS_CKD_NT_MAX || s.np < 2 || s.np > SOS_CKD_NP_MAX || s.nc < 2 || s.nc > SOS_CKD_NC_MAX)
            return SOSGPU_E_UNSUPPORTED;
        const struct { long long off, len; } in[] = {{s.pres_off, s.np}, {s.temp_off, s.nt}, {s.conc_off, s.nc},
                                                     {s.prs_off, nlay}, {s.tmp_off, nlay}, {s.cl_off, nlay}};
        for (const auto &a : in)
            if (a.off < 0 || a.off > ad || a.len > ad - a.off) return SOSGPU_E_ARG;
        const long long xn = 8ll * s.nterm * nlay;
        if (s.xk_off < 0 || s.xk_off > od || xn > od - s.xk_off) return SOSGPU_E_ARG;
        t.pres_off = s.pres_off; t.temp_off = s.temp_off; t.conc_off = s.conc_off;
        t.prs_off = s.prs_off; t.tmp_off = s.tmp_off; t.cl_off = s.cl_off;
        t.xk_off = s.xk_off; t.slot0 = slots;
        t.nterm = s.nterm; t.nt = s.nt; t.np = s.np; t.nc = s.nc;
        slots += 8ll * s.nterm;
        max_slots = std::max(max_slots, 8 * s.nterm);
    }
    if (bad_wl) *bad_wl = -1;
    if (slots != nslots) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Staged s(device, L.total);
    if (s.rc) return s.rc;
    char *hp = (char *)s.host();
    memcpy(hp + L.tab, tab.data(), (size_t)nwl * sizeof(CkdWl));
    memcpy(hp + L.slots, ki, (size_t)nslots * sizeof(double *));
    HIPCHK(s.send(d_work, st));
    HIPCHK(hipMemsetAsync(d_status, 0, (size_t)nwl * sizeof(int32_t), st));
    const char *dp = (const char *)d_work;
    launch_coeff_abs_ckd_table((const CkdWl *)(dp + L.tab), nwl, max_slots, (const double *const *)(dp + L.slots), d_axes, nlay,
                               d_out, d_status, st);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_mie(int device, int nbmu, const double *xmu, double rn, double in, int nalpha, const double *alphas,
                          float *d_rec, double *d_g, void *stream)
{
    if (nbmu < 1 || nbmu > 100 || !xmu || nalpha < 1 || !alphas || !d_rec || !d_g) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int W = 2 * nbmu + 1;
    // ascending size parameters (SOS_MIE's grid): those whose 11 arrays of 2 alpha + 24 terms fit LDS form a prefix
    const double lds_alpha = 850.;
    double amax = 0., alds = 0.;
    int n_lds = 0;
    for (int i = 0; i < nalpha; i++) {
        if (!(alphas[i] > 0.) || (i && alphas[i] < alphas[i - 1])) return SOSGPU_E_ARG;
        amax = alphas[i];
        if (alphas[i] <= lds_alpha) { n_lds = i + 1; alds = alphas[i]; }
    }
    if (2 * amax + 24 > 10000) return SOSGPU_E_UNSUPPORTED;                      // CTE_MIE_DIM, SOS.h:117
    const size_t nscr = n_lds < nalpha ? mie_scratch_doubles(amax, nalpha - n_lds) : 0;
    TmpBuf tb(device, (size_t)(W + nalpha + nscr) * sizeof(double) + 64);
    if (!tb.p) return SOSGPU_E_HIP;
    char *buf = (char *)tb.p;
    double *d_xmu = (double *)buf, *d_al = d_xmu + W, *d_scr = d_al + nalpha;
    int32_t *d_err = (int32_t *)(d_scr + nscr);
    int32_t err = 0;
    hipError_t e = hipMemcpyAsync(d_xmu, xmu, W * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_al, alphas, nalpha * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, sizeof(int32_t), st);
    int rc = 0;
    if (e == hipSuccess) {
        rc = launch_mie(nalpha, nbmu, d_xmu, rn, in, d_al, n_lds, alds, amax, nscr ? d_scr : nullptr, d_rec, d_g, d_err, st);
        if (rc == 0) e = hipGetLastError();
    }
    if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, st);
    e = finish_sync(e, st);
    if (rc == -3) return SOSGPU_E_UNSUPPORTED;
    if (rc == -2) { g_last_hip = (int)hipGetLastError(); return SOSGPU_E_HIP; }
    HIPCHK(e);
    return err ? SOSGPU_E_UNSUPPORTED : SOSGPU_OK;
}

// The records of many refractive indices, queued (mie.hip k_mie_batch).  mie_batch_plan checks every job with sosgpu_mie's
// rules and lays the work area out: xmu | packed lists | job table | first[classes + 1][count + 1] | scratch.
namespace {
static_assert(sizeof(MieBatchJob) == 64, "the job table keeps the item offsets behind it 8-byte aligned");
struct MieBatchPlan {
    std::vector<MieBatchJob> tab;
    std::vector<int> first;                       // [MIE_BATCH_CLASSES + 1][count + 1]
    std::vector<std::pair<const double *, int>> lists;       // the distinct lists, in upload order
    int nitems[MIE_BATCH_CLASSES + 1];
    double scr_alpha;
    size_t al_doubles, scr_doubles;
    size_t o_al, o_tab, o_first, head_bytes, o_scr, total;
};

int mie_batch_plan(int nbmu, int count, const sosgpu_mie_job *jobs, MieBatchPlan &p)
{
    if (nbmu < 1 || nbmu > 100 || count < 0 || (count && !jobs)) return SOSGPU_E_ARG;
    const int NC = MIE_BATCH_CLASSES + 1, W = 2 * nbmu + 1;
    p.tab.assign((size_t)count, MieBatchJob());
    p.first.assign((size_t)NC * (count + 1), 0);
    p.lists.clear();
    p.scr_alpha = 0.;
    p.al_doubles = 0;
    long long n[MIE_BATCH_CLASSES + 1] = {};
    std::map<std::pair<const double *, int>, long long> seen;
    int rc = SOSGPU_OK;
    for (int k = 0; k < count; k++) {
        const sosgpu_mie_job &j = jobs[k];
        MieBatchJob &t = p.tab[k];
        if (!j.alphas || j.nalpha < 1 || !j.d_rec || !j.d_g) return SOSGPU_E_ARG;
        for (int c = 0; c <= NC; c++) t.bound[c] = j.nalpha;
        t.bound[0] = 0;
        for (int i = 0, c = 0; i < j.nalpha; i++) {
            const double a = j.alphas[i];
            if (!(a > 0.) || (i && a < j.alphas[i - 1])) return SOSGPU_E_ARG;
            for (const int ca = mie_batch_class(a); c < ca; c++) t.bound[c + 1] = i;
        }
        const double amax = j.alphas[j.nalpha - 1];
        if (2 * amax + 24 > 10000) rc = SOSGPU_E_UNSUPPORTED;                    // CTE_MIE_DIM (a malformed later job still wins)
        if (t.bound[NC] > t.bound[NC - 1]) p.scr_alpha = std::max(p.scr_alpha, amax);
        for (int c = 0; c < NC; c++) {
            p.first[(size_t)c * (count + 1) + k] = (int)n[c];
            n[c] += t.bound[c + 1] - t.bound[c];
            if (n[c] > INT_MAX) rc = SOSGPU_E_UNSUPPORTED;
        }
        const auto key = std::make_pair(j.alphas, (int)j.nalpha);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (long long)p.al_doubles).first;
            p.lists.push_back(key);
            p.al_doubles += (size_t)j.nalpha;
        }
        t.al_off = it->second;
        t.rn = j.rn; t.in = j.in; t.rec = j.d_rec; t.g = j.d_g;
    }
    if (rc) return rc;
    for (int c = 0; c < NC; c++) {
        p.first[(size_t)c * (count + 1) + count] = (int)n[c];
        p.nitems[c] = (int)n[c];
    }
    p.scr_doubles = p.nitems[NC - 1] ? (size_t)mie_batch_slots(p.nitems[NC - 1]) * 11 * (size_t)(int)(2 * p.scr_alpha + 24) : 0;
    WorkLayout w;
    w.take((size_t)W * sizeof(double), 8);                     // xmu, at the start of the area
    p.o_al = w.take(p.al_doubles * sizeof(double), 8);
    p.o_tab = w.take((size_t)count * sizeof(MieBatchJob), 8);
    p.o_first = w.take((size_t)NC * (count + 1) * sizeof(int), 8);
    p.head_bytes = w.total;                                    // (what travels in the staged copy)
    p.o_scr = w.take(p.scr_doubles * sizeof(double), 8);
    p.total = w.total;
    return SOSGPU_OK;
}
}  // namespace

extern "C" size_t sosgpu_mie_batch_work_bytes(int nbmu, int count, const sosgpu_mie_job *jobs)
{
    MieBatchPlan p;
    if (mie_batch_plan(nbmu, count, jobs, p) != SOSGPU_OK || !count) return 0;
    return p.total;
}

extern "C" int sosgpu_mie_batch(int device, int nbmu, const double *xmu, int count, const sosgpu_mie_job *jobs, void *d_work,
                                size_t work_bytes, int32_t *d_status, void *stream)
{
    MieBatchPlan p;
    if (int rc = mie_batch_plan(nbmu, count, jobs, p)) return rc;
    if (!count) return SOSGPU_OK;
    if (!xmu || !d_status || !work_area_ok(d_work, work_bytes, 0)) return SOSGPU_E_ARG;
    if (work_bytes < p.total) return SOSGPU_E_UNSUPPORTED;             // (this entry point's code for a short area)
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // --- angle set, lists, job table and item offsets: one pinned block -> d_work on the caller's stream, nothing waited for
    Staged s(device, p.head_bytes);
    if (s.rc) return s.rc;
    char *hp = (char *)s.host();
    memcpy(hp, xmu, p.o_al);
    size_t o = p.o_al;
    for (const auto &l : p.lists) { memcpy(hp + o, l.first, (size_t)l.second * sizeof(double)); o += (size_t)l.second * sizeof(double); }
    memcpy(hp + p.o_tab, p.tab.data(), (size_t)count * sizeof(MieBatchJob));
    memcpy(hp + p.o_first, p.first.data(), p.first.size() * sizeof(int));
    HIPCHK(s.send(d_work, st));
    HIPCHK(hipMemsetAsync(d_status, 0, (size_t)count * sizeof(int32_t), st));
    char *dw = (char *)d_work;
    const int rc = launch_mie_batch(nbmu, (const double *)dw, count, (const MieBatchJob *)(dw + p.o_tab), (const int *)(dw + p.o_first),
                                    p.nitems, (const double *)(dw + p.o_al), p.scr_alpha,
                                    p.scr_doubles ? (double *)(dw + p.o_scr) : nullptr, d_status, st);
    if (rc == -3) return SOSGPU_E_UNSUPPORTED;
    if (rc == -2) { g_last_hip = (int)hipGetLastError(); return SOSGPU_E_HIP; }
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

extern "C" int sosgpu_granu(int device, int nbmu, int nalpha, const float *d_rec, int igranu, double v1, double v2, double v3,
                            double wa, double alphaf, double *out, void *stream)
{
    if (nbmu < 1 || nbmu > 100 || nalpha < 1 || !d_rec || igranu < 1 || igranu > 2 || !out || !(wa > 0.)) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nout = (size_t)3 + 3 * (2 * nbmu + 1), nwork = (size_t)3 * nalpha + 1;
    TmpBuf tb(device, (nout + nwork) * sizeof(double));
    if (!tb.p) return SOSGPU_E_HIP;
    double *d_out = (double *)tb.p, *d_work = d_out + nout;
    launch_granu(nalpha, nbmu, d_rec, igranu, v1, v2, v3, wa, alphaf, d_work, d_out, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, nout * sizeof(double), hipMemcpyDeviceToHost, st);
    HIPCHK(finish_sync(e, st));
    return SOSGPU_OK;
}

extern "C" int sosgpu_granu_batch(int device, int nbmu, int count, const sosgpu_granu_job *jobs, double *d_out, double *d_work,
                                  size_t work_stride, void *stream)
{
    if (nbmu < 1 || nbmu > 100 || count < 0 || (count && (!jobs || !d_out || !d_work))) return SOSGPU_E_ARG;
    for (int k = 0; k < count; k++) {
        const sosgpu_granu_job &j = jobs[k];
        if (j.nalpha < 1 || !j.d_rec || j.igranu < 1 || j.igranu > 2 || !(j.wa > 0.) || work_stride < (size_t)3 * j.nalpha + 1)
            return SOSGPU_E_ARG;
    }
    if (!count) return SOSGPU_OK;
    if (const int rc = use_device(device)) return rc;
    launch_granu_batch(count, nbmu, jobs, d_work, work_stride, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

// Diagnostic: the streamed solver's scratch of this context (device pointer, size in doubles) and, after an order-parallel
// solve, where its I3 hand-over block starts (doubles from the start; 0 when the last solve did not use that form).
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

extern "C" int sosgpu_debug_scratch(sosgpu_ctx *cx, double **d_scratch, size_t *doubles, size_t *spec_i3_offset)
{
    if (!cx || !d_scratch || !doubles || !spec_i3_offset) return SOSGPU_E_ARG;
    *d_scratch = cx->scratch;
    *doubles = cx->scratch_doubles;
    *spec_i3_offset = cx->dbg_spec_i3;
    return SOSGPU_OK;
}

// Diagnostic: the pinned staging blocks the library holds for `device`, and how many of them a table could take now.
extern "C" int sosgpu_debug_stage_blocks(int device, int *total, int *idle)
{
    if (!total || !idle) return SOSGPU_E_ARG;
    std::lock_guard<std::mutex> lk(g_stage_mutex);
    *total = *idle = 0;
    for (const StageBlock &b : g_stage)
        if (b.device == device) { *total += 1; *idle += stage_passed(b); }
    return SOSGPU_OK;
}

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

// Diagnostic: the decimal round trip k_profile applies to its levels (profile.hip rt_e15_8 / rt_f10_5), element by element.
extern "C" int sosgpu_debug_roundtrip(int device, int fmt, size_t n, const double *d_in, double *d_out, void *stream)
{
    if ((fmt != 0 && fmt != 1) || n < 1 || n > ((size_t)1 << 31) || !d_in || !d_out) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    launch_debug_roundtrip(fmt, n, d_in, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}
