// csrc/api_atmosphere.hip -- the atmosphere in front of a solve: the profile stage per wavelength and per spectrum
// (profile.hip), the gas absorption profile, and the CKD layer tables of a spectrum (ckd.hip).
#include "api_internal.h"
#include <algorithm>

using namespace sosgpu_internal;

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

// The device entry of one layer profile: the caller's parameters and the grid of sosgpu_profile_layer_grid; its status.
int layer_entry(double tr, double hr, double ta, double zmin, double zmax, double a_tronc, double piz, double piztr, double zout,
                int smax, LayerWl *t)
{
    int32_t c[4];
    const int nt = sosgpu_profile_layer_grid(tr, hr, ta, zmin, zmax, c);
    if (nt < 0) return nt;
    t->tr = tr; t->hr = hr; t->ta = ta; t->zmin = zmin; t->zmax = zmax;
    t->a_tronc = a_tronc; t->piz = piz; t->piztr = piztr; t->zout = zout;
    t->smax = smax; t->nt = c[0]; t->c1 = c[1]; t->c2 = c[2]; t->c3 = c[3]; t->pad = 0;
    return SOSGPU_OK;
}
}  // namespace

// Level counts of the aerosol-layer profile (SOS_PROFIL.F:800-870): closed forms of the five parameters, host arithmetic with the
// C library's exp, so that they are the integers of the Python restatement (geometry.layer_grid).
#pragma clang fp contract(off)
extern "C" int sosgpu_profile_layer_grid(double tr, double hr, double ta, double zmin, double zmax, int32_t counts[4])
{
    if (!counts || !(hr > 0.) || !(tr > 0.) || !(ta >= 0.)) return SOSGPU_E_ARG;
    if (!(zmin >= 0.0) || !(zmax > zmin)) return SOSGPU_E_ARG;             // 0 <= Zmin < Zmax
    const double ttot = tr + ta;
    const double q = ttot / kTcouche;
    const int nt = q >= (double)kOsNt ? kOsNt : (int)q;
    const double dzt = (double)0.010f;                                     // CTE_DZTRANSI
    const double vr_c1 = tr * exp(-(zmax + dzt) / hr);
    double vr_c3 = 0.;
    int nb_tr = 1;
    if (zmin != 0.0) { vr_c3 = tr * (1.0 - exp(-(zmin - dzt) / hr)); nb_tr = 2; }
    const int c1 = std::max(3, (int)((nt - nb_tr) * vr_c1 / (tr + ta)));   // CTE_PROFIL_MIN_NBC = 3
    const int c3 = zmin == 0.0 ? 0 : std::max(3, (int)((nt - nb_tr) * vr_c3 / (tr + ta)));
    const int c2 = (nt - nb_tr) - c1 - c3;
    if (c2 <= 0 || (ta / c2) < (double)0.00001f) return SOSGPU_E_UNSUPPORTED;   // not enough sublayers (ERROR 1020)
    counts[0] = nt; counts[1] = c1; counts[2] = c2; counts[3] = c3;
    return nt;
}

extern "C" int sosgpu_profile_layer(sosgpu_ctx *cx, double tr, double hr, double ta, double zmin, double zmax, double a_tronc,
                                    double piz, double piztr, double zout, int lp, double *d_prof, int32_t *d_nt,
                                    int32_t *d_iborm, double *d_zprof, int32_t *d_jout, double *d_zz, double *d_scal,
                                    double *d_hvrai, void *stream)
{
    if (!cx || lp < 2 || !d_prof || !d_nt || !d_iborm || !d_zprof || !d_scal) return SOSGPU_E_ARG;
    if ((d_jout == nullptr) != (d_zz == nullptr) || (zout != -1.0 && !d_jout)) return SOSGPU_E_ARG;
    LayerArgs q;
    if (const int rc = layer_entry(tr, hr, ta, zmin, zmax, a_tronc, piz, piztr, zout, 0, &q.one)) return rc;
    q.one.smax = cx->d.smax;
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t st = (hipStream_t)stream;
    q.nb = 1; q.lp = lp; q.tab = nullptr;
    q.prof = d_prof; q.zprof = d_zprof; q.zz = d_zz; q.scal = d_scal; q.nt = d_nt; q.iborm = d_iborm; q.jout = d_jout;
    q.hvrai = d_hvrai;
    launch_profile_layer(q, st);
    HIPCHK(hipGetLastError());
    note_stream(cx, st);
    return SOSGPU_OK;
}

// work area: the per-wavelength table
extern "C" size_t sosgpu_profile_layer_spectrum_work_bytes(int nwl)
{
    static_assert(sizeof(LayerWl) % 8 == 0, "entries of doubles and int32 pairs");
    return nwl < 1 ? 0 : (size_t)nwl * sizeof(LayerWl);
}

extern "C" int sosgpu_profile_layer_spectrum(int device, int nwl, const sosgpu_layer_wl *wl, int lp, void *d_work, size_t work_bytes,
                                             double *d_prof, int32_t *d_nt, int32_t *d_iborm, double *d_zprof, int32_t *d_jout,
                                             double *d_zz, double *d_scal, double *d_hvrai, int *bad_wl, void *stream)
{
    if (bad_wl) *bad_wl = -1;
    if (nwl < 1 || !wl || lp < 2) return SOSGPU_E_ARG;
    const size_t need = sosgpu_profile_layer_spectrum_work_bytes(nwl);
    if (!work_area_ok(d_work, work_bytes, need)) return SOSGPU_E_ARG;
    if (!d_prof || !d_nt || !d_iborm || !d_zprof || !d_scal) return SOSGPU_E_ARG;
    if ((d_jout == nullptr) != (d_zz == nullptr)) return SOSGPU_E_ARG;
    // --- the rules of sosgpu_profile_layer, per wavelength, before anything is queued
    std::vector<LayerWl> tab((size_t)nwl);
    for (int w = 0; w < nwl; w++) {
        const sosgpu_layer_wl &s = wl[w];
        if (bad_wl) *bad_wl = w;
        if (s.smax < 0 || (s.zout != -1.0 && !d_jout)) return SOSGPU_E_ARG;
        if (const int rc = layer_entry(s.tr, s.hr, s.ta, s.zmin, s.zmax, s.a_tronc, s.piz, s.piztr, s.zout, s.smax, &tab[w])) return rc;
    }
    if (bad_wl) *bad_wl = -1;
    if (const int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Staged s(device, need);
    if (s.rc) return s.rc;
    memcpy(s.host(), tab.data(), need);
    HIPCHK(s.send(d_work, st));
    LayerArgs q;
    memset(&q.one, 0, sizeof q.one);
    q.nb = nwl; q.lp = lp; q.tab = static_cast<const LayerWl *>(d_work);
    q.prof = d_prof; q.zprof = d_zprof; q.zz = d_zz; q.scal = d_scal; q.nt = d_nt; q.iborm = d_iborm; q.jout = d_jout;
    q.hvrai = d_hvrai;
    launch_profile_layer(q, st);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}

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

// Diagnostic: the decimal round trip k_profile applies to its levels (profile.hip rt_e15_8 / rt_f10_5), element by element.
extern "C" int sosgpu_debug_roundtrip(int device, int fmt, size_t n, const double *d_in, double *d_out, void *stream)
{
    if ((fmt != 0 && fmt != 1) || n < 1 || n > ((size_t)1 << 31) || !d_in || !d_out) return SOSGPU_E_ARG;
    if (const int rc = use_device(device)) return rc;
    launch_debug_roundtrip(fmt, n, d_in, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SOSGPU_OK;
}
