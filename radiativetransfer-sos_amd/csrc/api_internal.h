// csrc/api_internal.h -- what the units of the C ABI layer (api.hip, api_*.hip) share, and nothing else: the error slot, the
// context, the device and stream rules, the faces of the three memory recyclers and the work-area contract.  Every cross-unit
// dependency of the layer is a declaration of this header ("The C ABI layer: one unit per concern").
#pragma once
#include "../../include/sosgpu.h"
#include "kernels.h"
#include "sos_common.h"
#include <cstring>
#include <vector>

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

namespace sosgpu_internal {
// The one error slot of the library: defined in api.hip, written by HIPCHK in every unit, handed as &g_last_hip to the
// launch_sos_* functions, read by sosgpu_last_hip_error.  (__thread, not thread_local: a thread_local declared extern is
// reached through a wrapper call that tests for dynamic initialisation; this is the plain thread-local access a file-local
// one had.)
extern __thread int g_last_hip;
#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t e_ = (x);                       \
        if (e_ != hipSuccess) {                    \
            g_last_hip = (int)e_;                  \
            return SOSGPU_E_HIP;                   \
        }                                          \
    } while (0)

// --- device and stream rules (api.hip)
int use_device(int device);
hipStream_t util_stream(int device);
void note_stream(sosgpu_ctx *cx, hipStream_t st);
hipError_t sync_ctx_streams(sosgpu_ctx *cx);

// --- the size-class table pool (api_mem.hip)
// *cls receives the size class (pass it back to mem_give); nullptr on failure
void *mem_take(int dev, size_t bytes, size_t *cls);
void mem_give(int dev, void *p, size_t cls);

// temporary of one entry point: taken from the pool, returned by the destructor (the entry point has waited for its stream)
struct TmpBuf {
    int dev; void *p; size_t cls;
    TmpBuf(int device, size_t bytes) : dev(device), p(mem_take(device, bytes, &cls)) {}
    ~TmpBuf() { mem_give(dev, p, cls); }
    TmpBuf(const TmpBuf &) = delete;
    TmpBuf &operator=(const TmpBuf &) = delete;
};

template <typename T>
int dev_alloc(sosgpu_ctx *cx, T **p, size_t count)
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

// --- the best-fit scratch pool (api_mem.hip)
double *pool_take(int dev, size_t need, size_t *got);
void pool_give(int dev, double *p, size_t n);

// --- the pinned staging blocks (api_mem.hip)
struct StageBlock { void *p; size_t bytes; hipEvent_t ev; int device; };

// One table on its way: takes the first block of the device that is large enough and has passed out of g_stage, else makes
// one (16 KiB at least); the caller fills host() in place and send()s it.  A block that is never sent goes back as it came.
class Staged {
    StageBlock b = {};
    const size_t n;
    int take(int device);
    void give();
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
inline bool work_area_ok(const void *d_work, size_t work_bytes, size_t need)
{
    return d_work && ((uintptr_t)d_work & 7) == 0 && work_bytes >= need;
}

// closing of a host-synchronous entry point: `st` is waited for whatever `e` says; the first error of the two
inline hipError_t finish_sync(hipError_t e, hipStream_t st)
{
    const hipError_t s = hipStreamSynchronize(st);
    return e == hipSuccess ? s : e;
}

// --- what the surface units (api_surface.hip) and the azimuth stage (api_outputs.hip) both evaluate
inline double sigma2_of_wind(double wind) { return (double)0.003f + (double)0.00512f * wind; }   // SOS_GLITTER.F:300

inline LandTerms land_terms(const sosgpu_land *land)
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
}   // namespace sosgpu_internal
