// csrc/api_reduce.hip -- from bins to bands and from ranks to one result: the aggregate of a band's bins (aggregate.hip, and
// the neutral element of an empty shard, k_aggregate_empty), the level transmissions, and the cross-GPU reduce over RCCL with
// its lazily loaded function table (g_rccl, file-local) and the k_reduce_save kernel.
#include "api_internal.h"
#include <algorithm>
#include <cstring>
#include <dlfcn.h>
#include <mutex>

using namespace sosgpu_internal;

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
