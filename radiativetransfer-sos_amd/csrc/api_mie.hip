// csrc/api_mie.hip -- the aerosol models: the Mie records of one refractive index or of many (mie.hip), and the size integrals
// over them (sosgpu_granu and its batch form).
#include "api_internal.h"
#include <algorithm>
#include <climits>
#include <map>

using namespace sosgpu_internal;

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
