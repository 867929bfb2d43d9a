// csrc/api_outputs.hip -- what is read off a solve's records: the azimuth recomposition (trphi.hip), the fluxes, the actinic
// flux and absorbed power, the irradiance quantities at the output slots (flux.hip, absorb.hip, irradiance.hip), and the
// sensor channels (channels.hip) -- each with its spectrum form where there is one.
#include "api_internal.h"
#include <algorithm>
#include <cmath>

using namespace sosgpu_internal;

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
