// csrc/api_surface.hip -- the surface matrices: the host half of the Cox-Munk Fresnel matrix with its decimal round trip,
// the sea (sosgpu_glitter) and land (sosgpu_land_surface) entry points, and their batch form for many jobs on one angle set
// (kernels in glitter.hip and land.hip).
#include "api_internal.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>

using namespace sosgpu_internal;

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
