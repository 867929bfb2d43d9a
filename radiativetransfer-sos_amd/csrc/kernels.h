// csrc/kernels.h -- host-side launchers of the gfx950 kernels (internal to libsosgpu.so).
#pragma once
#include "../../include/sosgpu.h"
#include "sos_common.h"
#include <atomic>

void launch_noyaux(const SosDev &cx, hipStream_t st);
void launch_noyaux_fetch(const SosDev &cx, int s, double *d_out, hipStream_t st);
// Table forms (sosgpu_noyaux_spectrum): the same four kernels for the nctx entries of a device table, context = blockIdx.z.
// The grids take the largest context of the call; every workgroup tests its own context's bounds.
struct NoyauxTableGrid {
    int smax, kp;                // largest iborm_max and order-1 stride
    size_t per;                  // largest rtph * ks2h * 128 (elements of one system per order)
};
void launch_noyaux_table(const SosDev *d_tab, int nctx, const NoyauxTableGrid &g, hipStream_t st);

// The small tables of many new contexts (ctx_fill.hip k_ctx_fill, sosgpu_create_spectrum): job i copies n_copy doubles from
// d_images + src_off to dst and clears the n_clear doubles behind them.  dst, d_images + src_off: 16-byte aligned; the three
// counts: multiples of 32 doubles.  One launch of (tiles of the largest n_copy + n_clear = max_doubles, nctx) workgroups.
struct CtxFillJob {
    double *dst;
    uint32_t src_off, n_copy, n_clear;
};
void launch_ctx_fill(const CtxFillJob *d_jobs, const double *d_images, int nctx, size_t max_doubles, hipStream_t st);

// Fused successive-orders solver, LDS-resident variants (sos_os.hip).  `pl`: the solve's plan -- the launcher runs the
// instantiation its variant fields name (solve_variant.h) and derives nothing itself.  Returns 0, SOSGPU_E_UNSUPPORTED when the
// context does not fit that variant, or -2 with the HIP error code in *hip_err.
int launch_sos_os(const SosDev &cx, const SosBins &bn, const sosgpu_solve_plan &pl, hipStream_t st, int *hip_err);
// Streamed-field solver (sos_stream.hip) for level grids beyond the LDS-resident variants: same contract.  nt_max bounds every NT
// of the launch; bn.scratch holds bn.scr_stride >= stream_scratch_doubles(pl.nw, pl.kht, bn.lpb) doubles per bin, bn.lpb a
// multiple of 32.
int launch_sos_stream(const SosDev &cx, const SosBins &bn, const sosgpu_solve_plan &pl, int nt_max, hipStream_t st, int *hip_err);
// order-parallel form (bn.spec_k): the Fourier stop tests of orders [s0, s1) of every bin, after the order tasks of a round
int launch_sos_stream_replay(const SosDev &cx, const SosBins &bn, const sosgpu_solve_plan &pl, int s0, int s1, hipStream_t st,
                             int *hip_err);
// the same two solvers with a per-bin context (bn.ctxs, bn.ctx_of_bin; sos_os_multi.hip, sos_stream_multi.hip): `cx` is any
// context of the table -- its N and surface-matrix flag are what the caller guarantees equal over the table
int launch_sos_os_multi(const SosDev &cx, const SosBins &bn, const sosgpu_solve_plan &pl, hipStream_t st, int *hip_err);
int launch_sos_stream_multi(const SosDev &cx, const SosBins &bn, const sosgpu_solve_plan &pl, int nt_max, hipStream_t st,
                            int *hip_err);
// What the four launchers share.  The (output mode ZM, SURF) instantiation of a launcher template F<A, B, C, ZM, SURF>: ZM = 2
// with output slots, 1 with one output altitude, else 0.
#define SOS_LAUNCH_ZM_SURF(F, A, B, C, nz, zo, surf, ...)                                                        \
    ((nz) > 0 ? ((surf) ? F<A, B, C, 2, true>(__VA_ARGS__) : F<A, B, C, 2, false>(__VA_ARGS__))                   \
     : (surf) ? ((zo) ? F<A, B, C, 1, true>(__VA_ARGS__) : F<A, B, C, 0, true>(__VA_ARGS__))                      \
              : ((zo) ? F<A, B, C, 1, false>(__VA_ARGS__) : F<A, B, C, 0, false>(__VA_ARGS__)))
// The dynamic-LDS limit of a kernel is set once per device and size (the call costs tens of microseconds: with few bins per
// wavelength the host launch path is what bounds a hyperspectral loop, scripts/spectrum_bench.py).  configured[16]: the sizes
// set so far, one array per kernel (atomics: host threads of run_sos.sos_proc_many launch concurrently; a lost update only
// repeats the call).  *dev: the current device.
inline hipError_t sos_set_dynamic_lds(const void *kern, size_t lds, std::atomic<size_t> *configured, int *dev)
{
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e == hipSuccess && (d < 0 || d >= 16 || configured[d].load(std::memory_order_acquire) < lds)) {
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess && d >= 0 && d < 16) configured[d].store(lds, std::memory_order_release);
    }
    if (dev) *dev = d;
    return e;
}

// The stage around the solver for the diffuse transmissions of -SOS.Trans (trans.hip, sosgpu_trans_spectrum).
// launch_trans_table: the nchild = nctx * n child entries (incidence J = 1..n of every parent, n common to the parents) and
// their order-1 vectors d_sv[nchild][4][kp]; two launches.  os_nb_max: the largest OS_NB of the parents (LDS of the second).
inline size_t trans_sv_lds_bytes(int os_nb) { return (size_t)8 * (os_nb + 1) * sizeof(double); }
void launch_trans_table(const SosDev *d_parents, int nchild, int n, SosDev *d_children, double *d_sv, int os_nb_max, hipStream_t st);
// the arrays the multi solver takes for the nb * n items (bin b, incidence J) -> item b * n + J - 1; one launch
struct TransItems {
    int nb, n, lp, nctx;
    const int32_t *ctx_of_bin, *nt;              // [nb]; ctx_of_bin null: context 0
    const double *prof;                          // [nb][3][lp]
    int32_t *ctx_of_item, *nt_item, *iborm_item; // [nb n]
    double *prof_item, *flux;                    // [nb n][3][lp], [nb n][2] (cleared)
};
void launch_trans_items(const TransItems &a, hipStream_t st);
// tdifmug[i] = EMOINS of item i; one launch
void launch_trans_gather(size_t nitems, const double *d_flux, double *d_tdifmug, hipStream_t st);

// The same stage for the spherical albedo (albedo.hip, sosgpu_albedo_spectrum): the items of launch_trans_items with, from_below
// != 0, the profile rows mirrored about each bin's nt, and with the items of weight-0 directions made malformed (parents: the
// device table [t.nctx] the children were made from, read for ga and mu); one launch
struct AlbedoItems {
    TransItems t;
    const SosDev *parents;
    int from_below;
};
void launch_albedo_items(const AlbedoItems &q, hipStream_t st);
// plane[b][j] = EPLUS of item (b, j + 1), 0 in weight-0 columns (d_plane may be null); salb[b] = sum_j ((2 ga_j) mu_j) plane[b][j]
// in ascending j; one launch of nb workgroups
void launch_albedo_sum(const AlbedoItems &q, double *d_plane, double *d_salb, hipStream_t st);
// out[g] = sum aik * salb over the bins of segment g (k_aggregate_scal's striding and tree); one launch of nseg workgroups
void launch_albedo_band(int nseg, const int32_t *d_seg, const double *d_aik, const double *d_salb, double *d_out, hipStream_t st);

void launch_aggregate(const SosDev &cx, int nseg, const int32_t *d_seg, const double *d_aik,
                      const double *d_rec, const int32_t *d_norders, const double *d_flux, const double *d_scal,
                      const double *d_tdifmug, double *d_out_rec, double *d_out_scal, hipStream_t st, int nb_single,
                      double *d_partial, int max_chunks);
// element [9] of the scalar blocks of nz slots: sum aik * exp(-tau[k][b]) over the bins of every segment (k_level_transmission)
void launch_level_transmission(int nb, int nseg, const int32_t *d_seg, const double *d_aik, const int32_t *d_norders, int nz,
                               const double *d_tau, double *d_out_scal, size_t slot_stride, int block_width, hipStream_t st);

void launch_glitter(int n, const double *d_mu, double sig, int os_nb, int os_ns, int os_nm, const double *d_fcoef,
                    int32_t *d_il, double *d_e, float *d_rsurf, hipStream_t st);
// pieces of the surface-matrix chains (glitter.hip / land.hip): azimuth quadrature of SOS_GSF (model 0: Cox-Munk, par = sigma^2)
// or SOS_GSF_MAIGNAN (model 1, par = C exp(-NDVI)); SOS_MAT_REFLEXION + SOS_MISE_FORMAT with COEF = 1/sigma^2 or 1
void launch_gsf(int model, int n, const double *d_mu, double par, int os_nm, int32_t *d_il, double *d_e, hipStream_t st);
void launch_mat_reflexion(int n, const double *d_mu, double coef, int os_nb, int os_ns, int os_nm, const double *d_fcoef,
                          const int32_t *d_il, const double *d_e, float *d_rsurf, hipStream_t st);
// dynamic LDS k_mat_reflexion asks for (the series g[os_nm+1] and twelve Fresnel kernels per Fourier index), and the most a
// workgroup can have on gfx950 (160 KiB; the kernel has no static LDS): a larger shape cannot be launched
inline size_t mat_reflexion_lds_bytes(int os_ns, int os_nm)
{
    return ((size_t)(os_nm + 1) + 12 * (size_t)(os_ns + 1)) * sizeof(double);
}
constexpr size_t kLdsMaxBytes = 160 * 1024;
// land surfaces (-SURF.Type 3, 4, 5, 7): Roujean BRDF, + Rondeaux-Herman / Breon / Maignan BPDF
void launch_land(int isurf, int n, const double *d_mu, double k0, double k1, double k2, double coef_c, int os_nb, int os_ns, int os_nm, const double *d_fcoef, double *d_e_nn, int32_t *d_il_nn,
                 double *d_e, int32_t *d_il, float *d_tmp, float *d_rsurf, int32_t *d_err, hipStream_t st);
// Table forms of the surface-matrix kernels (sosgpu_surface_batch): the distinct parameter sets of many jobs, one launch per
// kernel.  The tables sit in the caller's work area; every kernel takes its entry by scalar loads.
struct SurfReflSet {          // one SOS_MAT_REFLEXION result: COEF, the azimuth analysis it reads, its Fresnel coefficients
    double coef;
    int32_t analysis, ind;
};
struct SurfTriple { double k0, k1, k2; };
struct SurfJobDev {
    float *out;               // the job's block [os_nb+1][9][N][N]
    int32_t isurf, refl, trip, pad;   // refl / trip: index of its reflexion block / Roujean triple, -1: none
};
// analyses of nsets parameters d_par[nsets] (model as launch_gsf): il[nsets][npairs], e[nsets][npairs][os_nm+1]
void launch_gsf_table(int model, int n, const double *d_mu, const double *d_par, int nsets, int os_nm, int32_t *d_il, double *d_e,
                      hipStream_t st);
// constant analyses (d_models[s] = 0 Rondeaux-Herman, 1 Breon): the same layout
void launch_gsf_const_table(int n, int nsets, const int32_t *d_models, const double *d_mu, int os_nm, int32_t *d_il, double *d_e,
                            hipStream_t st);
// d_refl[nsets][os_nb+1][9][N][N]; d_il / d_e: analysis 0 of the call, d_fcoef[nind][4][os_ns+1]
void launch_mat_reflexion_table(int n, const double *d_mu, const SurfReflSet *d_sets, int nsets, int os_nb, int os_ns, int os_nm,
                                const double *d_fcoef, const int32_t *d_il, const double *d_e, float *d_refl, hipStream_t st);
// Roujean analyses of ntrip triples: il_nn[ntrip][N^2], e_nn[ntrip][N^2][os_nb+1], flags[ntrip] (cleared by the caller)
void launch_fsf_table(int n, const double *d_mu, int os_nb, const SurfTriple *d_trip, int ntrip, int32_t *d_il_nn, double *d_e_nn,
                      int32_t *d_flags, hipStream_t st);
void launch_surface_compose(int n, int os_nb, const SurfJobDev *d_jobs, int njobs, const float *d_refl, const double *d_e_nn,
                            const int32_t *d_flags, int32_t *d_status, hipStream_t st);
struct LandTerms {            // direct surface terms of the land models in SOS_TRPHI (SOS_PREPA_OS.F:479-497 flags)
    int iroujean, irondeaux, ibreon, imaignan;
    double k0, k1, k2, coef_c;
};
void launch_trphi(const SosDev &cx, int nf, const double *d_rec, double tau, double tauout, int nphi,
                  const double *d_phi, int igli, double sigma2, double ind_surf, const LandTerms &land, double *d_out,
                  hipStream_t st);
// Table form (sosgpu_trphi_spectrum): launch_trphi's arguments per job, in a device array.  One launch of nblocks = sum of the
// jobs' azimuth counts; first_block is their running sum (ascending, 0 for the first job), w_max the largest W of the jobs.
struct TrphiJobDev {
    int n, w, n0, ipolar, ifresnel;      // of the job's context, with mu
    int nf, igli;
    int first_block;
    const double *mu, *rec, *phis;       // phis: the job's own azimuths
    double *out;                         // [nphi][7][W] of the job
    double ind_surf, sigma2, tau, tauout;
    LandTerms land;
};
void launch_trphi_table(const TrphiJobDev *d_jobs, int njobs, int nblocks, int w_max, hipStream_t st);

// Diffuse fluxes of an aggregated record at its output altitude (flux.hip): d_out[0] = E-, d_out[1] = E+ from the order-0
// intensity row d_rec[0][0][W] and the context's mu, ga, n0
void launch_level_flux(const SosDev &cx, const double *d_rec, double *d_out, hipStream_t st);
// Table form (sosgpu_level_flux_spectrum): launch_level_flux's arguments per job, in a device array; one launch of
// ceil(2 njobs / 64) workgroups, thread = (job, hemisphere)
struct FluxJobDev {
    int n, n0;                           // of the job's context, with mu and ga
    const double *mu, *ga, *rec;
    double *out;                         // [2] of the job
};
void launch_level_flux_table(const FluxJobDev *d_jobs, int njobs, hipStream_t st);

// Actinic flux and absorbed power of nz output slots (absorb.hip k_level_absorption): d_out[nz][nseg][4] = sum aik * {a_dir, a_dn,
// a_up, q} over the bins of every segment, formed per bin from the slot's order-0 row of d_rec[nz][nb][smax+1][3][W], the
// profile rows and level altitudes; d_table null: every bin with cx, else bin b with entry d_ctx_of_bin[b] (cx: the layout)
void launch_level_absorption(const SosDev &cx, const SosDev *d_table, const int32_t *d_ctx_of_bin, int nb, int lp,
                             const int32_t *d_nt, const double *d_prof, const double *d_zprof, int nz, const int32_t *d_jout,
                             const double *d_zz, const double *d_tauout, const double *d_rec, const int32_t *d_norders, int nseg,
                             const int32_t *d_seg, const double *d_aik, double *d_out, hipStream_t st);
// Every irradiance quantity of nz output slots (irradiance.hip k_level_irradiance): d_out[nz][nseg][SOSGPU_IRRADIANCE_COLS], the
// four sums above, sum aik {E-, E+} formed per bin from the same order-0 row (d_flux[nb][2] in a standard-output slot) and
// the band scalars of d_scal[nb][4], d_tauout and d_tauvrai[nz][nb] (may be null); one launch, the other arguments as above
void launch_level_irradiance(const SosDev &cx, const SosDev *d_table, const int32_t *d_ctx_of_bin, int nb, int lp,
                             const int32_t *d_nt, const double *d_prof, const double *d_zprof, int nz, const int32_t *d_jout,
                             const double *d_zz, const double *d_tauout, const double *d_rec, const int32_t *d_norders,
                             const double *d_flux, const double *d_scal, const double *d_tauvrai, int nseg, const int32_t *d_seg,
                             const double *d_aik, double *d_out, hipStream_t st);

// Sensor channels of a spectrum (channels.hip).  launch_channel_accumulate: acc[nchan][nslots][nphi][3][W] += the terms
// first[c] .. first[c + 1] - 1 of every channel c, term m = wgt[m] x rows 0..2 of block (job[m], slot) of d_blocks
// [njobs][nslots][nphi][7][W]; one launch of (ceil(nphi 3 W / 256), nslots, nchan) workgroups, first / job / wgt on the device.
void launch_channel_accumulate(const double *d_blocks, int nslots, int nphi, int w, int nchan, const int32_t *d_first,
                               const int32_t *d_job, const double *d_wgt, double *d_acc, hipStream_t st);
// out[nchan][nslots][nphi][7][W] of the sums: thresholds, ANGDIFF from d_angdiff_block[nphi][7][W], SOS_POLAR
void launch_channel_finish(const double *d_acc, const double *d_angdiff_block, int nchan, int nslots, int nphi, int w,
                           double *d_out, hipStream_t st);

#define SOS_PROF_NBLEV_MAX 64     // levels of the absorption profile held in LDS (CTE_ABS_NBLEV = 50 in the reference)
// Per-bin profile discretisation (profile.hip).  *_ng: the no-gas profile of the wavelength (host-computed, device copy).
struct ProfileArgs {
    int nb, lp, nblev, absprofil, smax, nt_ng;
    double tr, hr, ta, ha, a_tronc, piz, piztr, zout;
    const double *altabs, *tabs;                 // [nblev], [nb][nblev] or null
    const double *z_ng, *h_ng, *pca_ng, *pcm_ng;  // [nt_ng+1]
    double *prof, *zprof, *zz, *scal;
    int32_t *nt, *iborm, *jout;
    double *hvrai;                               // [nb][lp] or null: H before the truncation rescale (the untruncated depth)
};
void launch_profile(const ProfileArgs &a, hipStream_t st);
// Table forms of the three profile kernels (sosgpu_profile_spectrum): the bins of MANY wavelengths in one launch per kernel.
// One entry per wavelength, uploaded by the entry point; offsets count doubles from the start of the packed gas buffer.
struct ProfileWl {
    double tr, hr, ta, ha, a_tronc, piz, piztr, zout;
    double t_first, t_layer;                     // steps of the no-gas grid (profile_nogas_grid)
    long long xk_off, ro_off, alt_off;           // xk[8][nterm][nblev-1], ro[8][nblev-1], altabs[nblev] of the wavelength
    int nterm;                                   // 0: no gas (one bin, ABSPROFIL = 7)
    int absprofil, smax, nt_ng;                  // nt_ng < 1: refused by the host, its bins come back with nt = -1
};
struct ProfileTableArgs {
    int nb, nwl, lp, nblev, ngl;                 // ngl: levels per array of a no-gas block (SOSGPU_NOGAS_LEVELS)
    const ProfileWl *tab;
    const int32_t *wl_of_bin;                    // [nb]
    const double *gas, *tabs, *nogas;            // packed gas buffer, tabs[nb][nblev] (or null), nogas[nwl][4][ngl]
    double *prof, *zprof, *zz, *scal;
    int32_t *nt, *iborm, *jout;
    double *hvrai;                               // [nb][lp] or null, as ProfileArgs
};
void launch_profile_nogas_table(const ProfileWl *d_tab, int nwl, double *d_ng, int ngl, hipStream_t st);
void launch_absprofile_table(const ProfileWl *d_tab, int nwl, const int32_t *d_wl_of_bin, int nb, int nlev, const int32_t *d_ik,
                             const double *d_gas, double *d_tabs, hipStream_t st);
void launch_profile_table(const ProfileTableArgs &q, hipStream_t st);
// Aerosol-layer profile (IPROFIL = 2, profile.hip k_profile_layer): one wavefront per bin, a bin being one wavelength.  The
// level counts are the host's (sosgpu_profile_layer_grid): nt = nb_tr + c1 + c2 + c3 with nb_tr = 1 (zmin = 0, c3 = 0) or 2.
struct LayerWl {
    double tr, hr, ta, zmin, zmax, a_tronc, piz, piztr, zout;
    int smax, nt, c1, c2, c3, pad;
};
struct LayerArgs {
    int nb, lp;
    const LayerWl *tab;                          // [nb] (table form), or null: the one bin is `one`
    LayerWl one;
    double *prof, *zprof, *zz, *scal;            // outputs as ProfileArgs; jout / zz written for bins with zout != -1 only
    int32_t *nt, *iborm, *jout;
    double *hvrai;
};
void launch_profile_layer(const LayerArgs &q, hipStream_t st);
// output levels of nz altitudes (profile.hip k_output_levels): jout / zz / tauout[nz][nb] from zprof[nb][lp], prof[nb][3][lp], nt[nb]
struct OutputLevelArgs {
    int nb, lp, nz;
    double zout[SOSGPU_MAX_OUTPUT_LEVELS];
    const double *prof, *zprof;
    const int32_t *nt;
    int32_t *jout;
    double *zz, *tauout;
};
void launch_output_levels(const OutputLevelArgs &a, hipStream_t st);
// the depth of nz altitudes alone, on a depth row of any stride (k_output_depths): tau[nz][nb] from h[b * h_stride + level]
struct OutputDepthArgs {
    int nb, lp, nz;
    size_t h_stride;
    double zout[SOSGPU_MAX_OUTPUT_LEVELS];
    const double *h, *zprof;
    const int32_t *nt;
    double *tau;
};
void launch_output_depths(const OutputDepthArgs &a, hipStream_t st);
// diagnostic: out[i] = the E15.8 (fmt 0) or F10.5 (fmt 1) round trip of in[i] as k_profile applies it
void launch_debug_roundtrip(int fmt, size_t n, const double *d_in, double *d_out, hipStream_t st);
// the no-gas profile of the wavelength into d_ng = z | h | pca | pcm, `ng` doubles each (nt + 1 <= ng used)
void launch_profile_nogas(double tr, double hr, double ta, double ha, int nt, double t_first, double t_layer, double *d_ng, int ng,
                          hipStream_t st);

// SOS_ABSPROFILE for nb bins: ik[nb][8] 1-based term per gas, xk[8][nterm][nlev-1], ro[8][nlev-1] -> tabs[nb][nlev]
void launch_absprofile(int nb, int nlev, int nterm, const int32_t *d_ik, const double *d_xk, const double *d_ro, double *d_tabs,
                       hipStream_t st);

// COEFF_ABS_CKD of many wavelengths (ckd.hip k_coeff_abs_ckd_table, sosgpu_ckd_layer_tables): one wavefront per slot =
// (wavelength, gas, term), lane = layer.  One entry per wavelength, uploaded by the entry point; offsets count doubles in
// the packed axes buffer / the output block; slot0: the wavelength's first slot in the pointer table (8 * nterm slots each).
#define SOS_CKD_NT_MAX 16         // temperature nodes (9 in the reference's tables)
#define SOS_CKD_NP_MAX 64         // pressure nodes (31)
#define SOS_CKD_NC_MAX 16         // H2O concentration nodes (12)
#define SOS_CKD_NLAY_MAX 63       // layers = lanes (49)
struct CkdWl {
    long long pres_off, temp_off, conc_off;      // tab_pres[np], tab_temp[nt], tab_conc[nc]
    long long prs_off, tmp_off, cl_off;          // layer means prs / tmp / conc [nlay], unclamped, layer 0 = top layer
    long long xk_off;                            // xk[8][nterm][nlay] of the wavelength in the output block
    long long slot0;
    int nterm, nt, np, nc;
};
void launch_coeff_abs_ckd_table(const CkdWl *d_tab, int nwl, int max_slots, const double *const *d_ki, const double *d_axes, int nlay,
                                double *d_out, int32_t *d_status, hipStream_t st);

// Mie records of a size-parameter grid (mie.hip): rec[nalpha][4 + 3 (2 nbmu + 1)] floats, g[nalpha]; returns 0, -2 (HIP) or -3
// (alpha_max beyond the LDS-resident coefficient arrays)
size_t mie_scratch_doubles(double alpha_max, int count);
// SOS_GRANU on the device records: d_work[3 na + 1], d_out[3 + 3 (2 nbmu + 1)] (mie.hip)
void launch_granu(int na, int nbmu, const float *d_rec, int igranu, double v1, double v2, double v3, double wa, double alphaf,
                  double *d_work, double *d_out, hipStream_t st);
// ... for `count` jobs, one workgroup each: d_work[count][work_stride], d_out[count][3 + 3 (2 nbmu + 1)]
void launch_granu_batch(int count, int nbmu, const sosgpu_granu_job *jobs, double *d_work, size_t work_stride, double *d_out,
                        hipStream_t st);
int launch_mie(int nalpha, int nbmu, const double *d_xmu, double rn, double in, const double *d_alphas, int n_lds, double alpha_lds,
               double alpha_max, double *d_scratch, float *d_rec, double *d_g, int32_t *d_err, hipStream_t st);
// ... of many refractive indices as one pool of (job, size parameter) items (mie.hip: the classes and the item mapping).
// bound[c] .. bound[c + 1]: the size parameters of the job in class c (its list ascends; class MIE_BATCH_CLASSES = scratch form)
#define MIE_BATCH_CLASSES 4
struct MieBatchJob {
    double rn, in;
    float *rec;
    double *g;
    long long al_off;                            // its list in the packed size parameters, in doubles
    int bound[MIE_BATCH_CLASSES + 2];
};
int mie_batch_class(double alpha);
int mie_batch_slots(long long scratch_items);    // resident workgroups (= scratch slots) of the scratch-form launch
int launch_mie_batch(int nbmu, const double *d_xmu, int count, const MieBatchJob *d_jobs, const int *d_first, const int *nitems,
                     const double *d_alphas, double alpha_scr_max, double *d_scratch, int32_t *d_status, hipStream_t st);
