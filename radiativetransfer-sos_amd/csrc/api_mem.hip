// csrc/api_mem.hip -- the three memory recyclers of the C ABI layer, each with its state and mutex: the size-class table pool
// (mem_take / mem_give), the best-fit scratch pool (pool_take / pool_give) and the pinned staging blocks (Staged).  The state is
// file-local; other units reach it through the functions api_internal.h declares.  sosgpu_trim and sosgpu_debug_stage_blocks
// live here because they read that state.
#include "api_internal.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>

using namespace sosgpu_internal;

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
}   // namespace

namespace sosgpu_internal {
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
}   // namespace sosgpu_internal

// The streamed solver's scratch outlives its context: one sos_proc call = one context (one wavelength), and a fresh hipMalloc
// of the 60-1000 MB the order-parallel form wants costs ~9 ms per call (scripts/latency_bench.py: 1.1 ms solve, 9.2 ms first
// call) -- more than the solve.  Released buffers wait here (per device, at most 8 of them and 8 GiB in total) for the next
// context.  A buffer is only returned after the stream of its last solve has been synchronised.
namespace {
struct ScratchBuf { double *p; size_t n; int dev; };
std::mutex g_pool_mutex;
std::vector<ScratchBuf> g_pool;
}   // namespace

namespace sosgpu_internal {
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
}   // namespace sosgpu_internal

// The per-wavelength or per-job table of every table-form entry point travels to the caller's work area from a pinned block
// the library recycles (per device): a block is free again when the event recorded behind its copy has passed.  Nothing is
// waited for and no context owns a block; sosgpu_trim frees those that have passed.
namespace {
std::mutex g_stage_mutex;
std::vector<StageBlock> g_stage;     // the blocks in no call's hands

bool stage_passed(const StageBlock &b)      // (a never-recorded event queries as complete)
{
    if (hipEventQuery(b.ev) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
}   // namespace

namespace sosgpu_internal {
int Staged::take(int device)
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

void Staged::give()
{
    if (!b.p) return;
    std::lock_guard<std::mutex> lk(g_stage_mutex);
    g_stage.push_back(b);
    b.p = nullptr;
}
}   // namespace sosgpu_internal

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
