/* oracle/sos_oracle.h -- CPU restatement (plain C, fp64) of the reference hot path.
 *
 * TEST INFRASTRUCTURE ONLY: this library is the parity checker.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it; the product path
 * (radiativetransfer-sos_amd/, libsosgpu.so) never links, imports or calls it.
 *
 * Pinning: every function here is checked against the real reference Fortran compiled from
 * /root/reference (oracle/_ref/libsos_ref.so, see oracle/Makefile) by tests/test_oracle_vs_ref.py in the
 * authoring container, and against the committed golden vectors under tests/golden/ (generated
 * from that same Fortran by tests/golden/make_golden.py) everywhere else.
 *
 * Conventions shared by all entry points
 *   N  = NBMU: number of positive directions (Gauss + sun [+ user]); mu[0..N-1] = RMU(1..N) > 0.
 *   Direction index jj in -N..N is stored at offset jj+N in arrays of width W = 2N+1; jj = 0 is the
 *   solar beam slot (RMU(0) = -mus) and is meaningless in outputs (set to 0 here; the reference
 *   leaves it uninitialised, SOS_OS.F:337-358).
 *   Fourier records: rec[s][c][jj+N], c = 0:I 1:Q 2:U (the reference file order is Q,U,I,
 *   SOS_OS.F:1572-1574).
 *   Level index i = 0 (TOA) .. NT (ground).
 */
#ifndef SOS_ORACLE_H
#define SOS_ORACLE_H
#ifdef __cplusplus
extern "C" {
#endif

/* SOS_NOYAUX, SOS_OS.F:1857-2158.  rmu0 = RMU(0) (= -mus).  Outputs: six (W x W) kernels stored
 * X[(j+N)*W + (k+N)] = X(J,K) and three W-vectors XPL/XRL/XTL. */
void sos_oracle_noyaux(int is, int n, double rmu0, const double *mu, int os_nb,
                       const double *alpha, const double *beta, const double *gamma, const double *zeta,
                       double *xpl, double *xrl, double *xtl,
                       double *bp, double *gr, double *gt, double *arr, double *art, double *att);

/* Extended form (sos_oracle_noyaux is this with start = psl_all = rsl_all = tsl_all = NULL, bit for bit).
 *  start   : NULL, or [3][n+1]: the start values PSL/RSL/TSL(IS, j), j = 0..n, of IS >= 2 taken from the caller instead of the
 *            three expressions with XX**(IS/2) and XX**YY (SOS_OS.F:2040-2049); ignored for IS < 2
 *  psl_all, rsl_all, tsl_all : NULL, or [os_nb+1][W]: PSL/RSL/TSL(l, j) for every l = 0..os_nb (entries the reference never
 *            assigns are 0)
 *  bp == NULL: the six kernel sums are skipped (they cost O(W^2 OS_NB)). */
void sos_oracle_noyaux_ext(int is, int n, double rmu0, const double *mu, int os_nb,
                           const double *alpha, const double *beta, const double *gamma, const double *zeta,
                           const double *start, double *psl_all, double *rsl_all, double *tsl_all,
                           double *xpl, double *xrl, double *xtl,
                           double *bp, double *gr, double *gt, double *arr, double *art, double *att);

/* Single pieces of SOS_OS for the table tests.  kern6 = BP,GR,GT,ARR,ART,ATT [6][W][W], xprt3 = XPL,XRL,XTL [3][W] as
 * sos_oracle_noyaux returns them; vectors [3][W] are I,Q,U over jj = -N..N (slot jj = 0 unused).
 *  ray_coefs     BETA2, GAMMA2, ALPHA2 of SOS_OS.F:678-699 (polarisation cut applied)
 *  ray_kernels   the molecular second terms of SOS_OS.F:2859-2876 as six kernels (BETA0 = 1 at IS = 0; zero for IS > 2)
 *  order1_coefs  SOS_FSOURCE_ORDRE1 at one level with ATTDIR = 1: aer = (SA2, SB2, -SC2), ray = (SA1, SB1, -SC1)
 *  fresnel1_coefs  SOS_FSOURCE_DIFF_FRESNEL1 without COEFK and the profile: aerosol and molecular part per field direction
 *  ordreig_level SOS_FSOURCE_ORDREIG at one level applied to fld_in [3][W]: aer with (PCAER, PCRAY) = (1, 0), ray with (0, 1) */
void sos_oracle_ray_coefs(double ron, int ipolar, double *b2g2a2);
void sos_oracle_ray_kernels(int is, int n, const double *xprt3, double beta2, double gamma2, double alpha2, double *kern6);
void sos_oracle_order1_coefs(int is, int n, const double *kern6, const double *xprt3,
                             double beta2, double gamma2, double *aer, double *ray);
void sos_oracle_fresnel1_coefs(int is, int n, double f11sun, double f12sun, const double *kern6, const double *xprt3,
                               double beta2, double gamma2, double alpha2, double *aer, double *ray);
/* SOS_FSOURCE_DIFF_FRESNEL1 itself at H = 0, MUS = 1 with one (PCAER, PCRAY): out [3][W] = a quarter of the coefficients above */
void sos_oracle_fresnel1_routine(int is, int n, double f11sun, double f12sun, const double *kern6, const double *xprt3,
                                 double beta2, double gamma2, double alpha2, double pcaer, double pcray, double *out);
void sos_oracle_ordreig_level(int is, int n, const double *ga, const double *kern6, const double *xprt3,
                              double beta2, double gamma2, double alpha2, const double *fld_in,
                              double *aer, double *ray);

/* SOS_OS, SOS_OS.F:303-1674 (with SOS_FSOURCE_ORDRE1/ORDREIG, SOS_INTEGR_EPOPT, the Fresnel flat-sea
 * pieces, the four stop tests and SOS_AJOUT_QUEUE).
 *  rsurf : REAL*4 surface matrices in FICSURF record order [iborm+1][9][N][N] with
 *          rsurf[s][ab][(J-1)*N + (I-1)] = R_ab(I,J)  (SOS_OS.F:916-925); NULL unless imat_surf==1.
 *  rec   : out, [iborm+1][3][W]; orders not run are left zero.
 *  n_orders : out, number of Fourier orders actually run (F).
 *  ig_last  : out, [iborm+1] last scattering order computed for each Fourier order.
 * returns IER (0 ok, -1 error as the reference). */
int sos_oracle_os(int n, const double *mu, const double *ga, int os_nb, int nt,
                  int n0, double tetas, double ro, int imat_surf, int ifresnel, double ind_surf,
                  const double *h, const double *xdel, const double *ydel, const double *zprof, double ron,
                  const double *alpha, const double *beta, const double *gamma, const double *zeta,
                  double zout, int igmax, int iborm, int ipolar, const float *rsurf,
                  double *rec, int *n_orders, int *ig_last, double *emoins, double *eplus);

/* The same solve with nz output altitudes zouts[nz] (-1 allowed per slot) in place of zout: rec is [nz][iborm+1][3][W]; order
 * counts, ig_last and fluxes are those of the one solve.  sos_oracle_os is the nz = 1 call of this function. */
int sos_oracle_os_levels(int n, const double *mu, const double *ga, int os_nb, int nt,
                         int n0, double tetas, double ro, int imat_surf, int ifresnel, double ind_surf,
                         const double *h, const double *xdel, const double *ydel, const double *zprof, double ron,
                         const double *alpha, const double *beta, const double *gamma, const double *zeta,
                         int nz, const double *zouts, int igmax, int iborm, int ipolar, const float *rsurf,
                         double *rec, int *n_orders, int *ig_last, double *emoins, double *eplus);

/* Tie audit: minimum over every stop decision (SOS_PARAM_CONV, SOS_ARRET_DIFFUS_1/2, SOS_ARRET_FOURIER) of the last
 * sos_oracle_os / sos_oracle_os_levels call of the calling thread of |tested value / threshold - 1|. */
double sos_oracle_stop_margin(void);

/* SOS.F:523-550: delta-truncation rescale of a profile (in place) and IBORM choice.
 * Returns IBORM (os_nb, or 2 when no aerosol).  h/xdel/ydel: [nt+1]. */
int sos_oracle_profile_rescale(int nt, double a_tronc, double piz, double piztr, int os_nb,
                               double *h, double *xdel, double *ydel);

/* SOS_AGGREGATE.F:372-488 for a whole list of bins at once (serial accumulation in bin order).
 *  rec_bins [nb][fmax][3][W] (orders >= nf[b] are ignored = zero-padded, SOS_AGGREGATE.F:357-413)
 *  scal_bins[nb][7]: TDIFMUS, EMOINS, EPLUS, TTOT_TRONC, TTOT_VRAI, TAUOUT, (unused)
 *  out_rec [fmax][3][W], out_scal[7] (same order; the three taus are -ln sum aik*exp(-tau)),
 *  returns max nf. */
int sos_oracle_aggregate(int nb, int fmax, int w, const int *nf, const double *aik,
                         const double *rec_bins, const double *scal_bins,
                         double *out_rec, double *out_scal);

/* ---- Cox-Munk glitter (sos_glitter_oracle.c) ---- */
/* SIG = .003 + .00512*WIND with the REAL*4 literals of SOS_GLITTER.F:300 */
double sos_oracle_sigma2(double wind);
/* SOS_GSF for one pair (SOS_GLITTER.F:523-683): e[0..os_nm], returns IL */
int sos_oracle_gsf_pair(double mu1, double mu2, double sig, int os_nm, double *e);
/* the quadrature of SOS_GSF over any facet function g(ctx, phi): shared by SOS_GSF and SOS_GSF_MAIGNAN */
typedef double (*sos_oracle_facet_fn)(const void *ctx, double phi);
int sos_oracle_gsf_quad(sos_oracle_facet_fn g, const void *ctx, int os_nm, double *e);
/* Tie audit of that quadrature since the last reset (sos_oracle_glitter and sos_oracle_land reset it): min
 * |tested / threshold - 1| of m3[0] the per-level 1e-4 test, m3[1] the 1e-3 closure that sets IL, m3[2] the 1 % bisection test */
void sos_oracle_quad_margin_reset(void);
void sos_oracle_quad_margin(double *m3);
/* SOS_MAT_REFLEXION + SOS_MISE_FORMAT (SOS_SURFACE.F:1708-1973, 2307-2443) from the series il[npairs], e[npairs][os_nm+1]
 * and the Fresnel expansion coefs[4][os_ns+1]; out REAL*4 [os_nb+1][9][N][N] */
void sos_oracle_mat_reflexion(int n, const double *mu, double coef, int os_nb, int os_ns, int os_nm, const double *coefs,
                              const int *il, const double *e, float *out);
/* SOS_MAT_FRESNEL incl. the 4(E15.8) round trip (SOS_SURFACE.F:1235-1603) */
void sos_oracle_mat_fresnel(int n, const double *mu, const double *chr, double ind, int os_ns,
                            double *alpha, double *beta, double *gamma, double *zeta);
/* SOS_GLITTER end to end (SOS_GLITTER.F:229-371): out REAL*4 [os_nb+1][9][N][N] in GLITTER-file order;
 * optional il_out[npairs], e_out[npairs][os_nm+1], coef_out[4][os_ns+1] */
int sos_oracle_glitter(int n, const double *mu, const double *chr, double wind, double ind,
                       int os_nb, int os_ns, int os_nm, float *out, int *il_out, double *e_out, double *coef_out);

/* ---- azimuth recomposition (sos_trphi_oracle.c) ---- */
void sos_oracle_polar(double xi, double xq, double xu, double *xan, double *tpol, double *lpol);
void sos_oracle_trphi(int n, const double *mu, int nf, const double *rec, double tau, double tauout, double phi,
                      int igli, int n0, double wind, double ind_surf, int ifresnel, int ipolar,
                      double *xit, double *xqt, double *xut, double *angdiff);

/* as sos_oracle_trphi, plus the direct term of a land surface (isurf 0 none, 3, 4, 5, 7); optional cosdif[W] (the cosine
 * behind ANGDIFF) and pre[3][W] (XIT, XQT, XUT before the zeroing thresholds) */
void sos_oracle_trphi_land(int n, const double *mu, int nf, const double *rec, double tau, double tauout, double phi,
                           int igli, int n0, double wind, double ind_surf, int ifresnel, int ipolar,
                           int isurf, double k0, double k1, double k2, double coef_c,
                           double *xit, double *xqt, double *xut, double *angdiff, double *cosdif, double *pre);

/* ---- land surfaces (sos_land_oracle.c) ---- */
double sos_oracle_calc_f_roujean(double k0, double k1, double k2, double c1, double s1, double c2, double s2, double phi);
double sos_oracle_calcg_maignan(double c1, double c2, double s12, double phi, double coef_c);
/* SOS_FSF_ROUJEAN for one ordered pair: e[0..os_nb], returns IL, sets *neg when the BRDF is negative somewhere; cs: optional
 * table cos(is * (i * pi / 1024)) [os_nb+1][1025] */
int sos_oracle_fsf_roujean_pair(double k0, double k1, double k2, double mu1, double mu2, int os_nb, const double *cs, double *e,
                                int *neg);
/* SOS_GSF_MAIGNAN for one pair: e[0..os_nm], returns IL */
int sos_oracle_gsf_maignan_pair(double mu1, double mu2, double coef_c, int os_nm, double *e);
/* SOS_ROUJEAN / SOS_SURFACE_BPDF / SOS_BPDF_AJOUT_BRDF end to end for isurf 3, 4, 5, 7: out REAL*4 [os_nb+1][9][N][N];
 * optional il_nn[N*N], e_nn[N*N][os_nb+1]; returns 0 or -1 (negative Roujean BRDF, the reference's IER) */
int sos_oracle_land(int isurf, int n, const double *mu, const double *chr, double k0, double k1, double k2, double coef_c,
                    double ind, int os_nb, int os_ns, int os_nm, float *out, int *il_nn, double *e_nn);
/* stop margins of the last sos_oracle_land call: Roujean B1 <= 1e-3, B1 < previous B1, then the three of the quadrature */
void sos_oracle_land_margin(double *m5);

/* ---- Mie theory and the size-distribution integral (sos_mie_oracle.c) ---- */
/* SOS_MIE + SOS_FPHASE_MIE for the size parameters alphas[nalpha] (any order), xmu[2 nbmu + 1] = RMU(-nbmu:nbmu):
 * rec REAL*4 [nalpha][4 + 3 (2 nbmu + 1)] = {alpha, Qext, Qsca, 0, Imie, Qmie, Umie}, g[nalpha];
 * optional info[nalpha][4] = {n2 finally used, overflow break of the CNA recurrence taken (0/1), number of SNA rescales, n1}.
 * Returns 0, -1 (argument), -2 (memory). */
int sos_oracle_mie(int nbmu, const double *xmu, double rn, double in, int nalpha, const double *alphas, float *rec, double *g,
                   int *info);
/* the same, plus optional unrounded[nalpha][3 + 3 (2 nbmu + 1)] = Qext, Qsca, g, Imie, Qmie, Umie as doubles, before the
 * record's REAL*4 rounding (what an independent high-precision series can be compared with) */
int sos_oracle_mie_f64(int nbmu, const double *xmu, double rn, double in, int nalpha, const double *alphas, float *rec, double *g,
                       int *info, double *unrounded);
/* SOS_GRANU on the records rec[na][4 + 3 (2 nbmu + 1)], sums in record order: out[3 + 3 (2 nbmu + 1)] = KMAT1 / SOMME_NR,
 * KMAT2 / SOMME_NR, SOMME_NR, then P11 | P12 | P33 (normalised by KMAT2); *nuse = number of records used.
 * igranu 1: log-normal (v1 modal radius, v2 ln-std); 2: Junge (v1 = r0, v2 slope, v3 = rmax).  Returns 0 or -1. */
int sos_oracle_granu(int nbmu, int na, const float *rec, int igranu, double v1, double v2, double v3, double wa, double alphaf,
                     double *out, int *nuse);

#ifdef __cplusplus
}
#endif
#endif
