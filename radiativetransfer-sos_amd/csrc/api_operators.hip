// csrc/api_operators.hip -- the operator tables of a context: the ground-reflection operator of the surface matrices
// (k_pack_ground, k_pack_ground_table and their shared body, launched here), the source operators (sosgpu_noyaux and its
// spectrum form, kernels in noyaux.hip), and the device table of contexts the multi-wavelength solves read.
#include "api_internal.h"
#include <algorithm>

using namespace sosgpu_internal;

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
