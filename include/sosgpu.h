/* include/sosgpu.h -- C ABI of libsosgpu.so, the MI355X (gfx950) drop-in for the SOS-ABS hot path.
 *
 * Plain C: pointers + sizes, int status (0 ok, negative = error, see sosgpu_strerror).  No torch
 * types, no Fortran hidden lengths, no files.  All `d_` pointers are DEVICE (HBM) addresses owned by
 * the caller (the Python host allocates them with torch); `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Calls are asynchronous on `stream` unless stated.
 *
 * Streams (the ordering rule).  No entry point synchronises the device, and none touches the null stream on its own:
 *   - entry points taking `stream` queue ALL their device work on it and -- unless documented "synchronous" -- return
 *     without waiting; their d_ inputs must have been produced on `stream` (or be complete) and must stay allocated
 *     until the queued work has run;
 *   - host-synchronous entry points without a stream argument (sosgpu_create, sosgpu_set_surface_matrices,
 *     sosgpu_noyaux_fetch, sosgpu_os_flops) move their data on a private non-blocking stream of the calling host thread
 *     (created at the highest stream priority: the runtime maps streams onto a few hardware queues, in order per queue,
 *     and at normal priority these short copies would wait behind the kernels of whatever caller stream shares the queue)
 *     and wait for that stream only; the last two first wait for the streams THIS context's work was queued on.  They
 *     write only memory the library owns (never a caller's buffer, which the caller's other queued work may still be
 *     using), and what they wrote is complete on return, so work queued afterwards on any stream sees it;
 *   - a context may be used from one host thread at a time; different contexts may be driven from different host
 *     threads on different streams concurrently (run_sos.sos_proc_many), and no call waits for another thread's work;
 *   - sosgpu_destroy waits for the streams the context's own work was queued on, nothing else.
 * Device memory of contexts and of temporaries is recycled through a process-wide pool (hipFree would synchronise the
 * device); sosgpu_trim() returns it.
 * The table of every table-form entry point (sosgpu_ctx_table, the *_spectrum, *_tables and *_batch calls) travels to the caller's
 * work area from a pinned block the library recycles: nothing is waited for and no context owns it, so any context of such a
 * call may be destroyed as soon as the call has returned (sosgpu_destroy waits for the context's streams, as ever).
 *
 * Work areas (the contract of every `void *d_work, size_t work_bytes` pair).  A table-form entry point sosgpu_<name> keeps its
 * table and its intermediates in a DEVICE area the caller provides, of work_bytes >= sosgpu_<name>_work_bytes(...) bytes:
 *   - the area is 8-byte aligned and the caller's until `stream` has passed the call (an allocator that recycles memory in
 *     stream order may drop it when the call returns); the table arrives there in ONE copy on `stream`;
 *   - nothing beyond the first sosgpu_<name>_work_bytes(...) bytes is read or written;
 *   - a NULL or misaligned d_work and a work_bytes below the query are refused with SOSGPU_E_ARG before anything is queued, a
 *     staging block is taken or a context is changed (sosgpu_mie_batch alone answers SOSGPU_E_UNSUPPORTED for a short area);
 *   - the query is host arithmetic (no device call) and returns 0 for arguments the call would refuse.
 *
 * Each entry point replaces one routine of the reference per-wavelength pipeline that
 * binding/run_sos.py reaches through sos.sos_proc (binding/run_sos.py:640, SOS_PROC.F:415):
 *
 *   sosgpu_profile     <- SOS_PROFILE + SOS_DISC  src/SOS_PROFIL.F:224,1210 (+ the PROFIL read-back and rescale of
 *                                                 SOS, src/SOS.F:511-550; all bins of a wavelength at once)
 *   sosgpu_profile_spectrum   the same and SOS_ABSPROFILE for the bins of many wavelengths: three launches in all
 *   sosgpu_ckd_layer_tables <- COEFF_ABS_CKD      src/SOS_SUB_TRS.F:171 (every gas, term and layer of many wavelengths)
 *   sosgpu_noyaux      <- SOS_NOYAUX              src/SOS_OS.F:1857   (phase-matrix Fourier kernels,
 *                                                                     hoisted out of the bin loop)
 *   sosgpu_create_spectrum    the contexts (SOS_PREPA_OS) of a part of a spectrum: one asynchronous call, one launch
 *   sosgpu_os_solve    <- SOS_OS (+ leaves)       src/SOS_OS.F:303    (one call = a batch of CKD bins,
 *                                                                     i.e. the loop SOS_PROC.F:3459-3594)
 *   sosgpu_aggregate   <- SOS_AGGREGATE           src/SOS_AGGREGATE.F:172
 *   sosgpu_glitter     <- SOS_GLITTER (+SOS_GSF, SOS_MAT_FRESNEL, SOS_MAT_REFLEXION, SOS_MISE_FORMAT)
 *                                                 src/SOS_GLITTER.F:229, src/SOS_SURFACE.F:1235,1708,2307
 *   sosgpu_surface_batch      sea and land surface matrices of a part of a spectrum: one asynchronous call
 *   sosgpu_trphi       <- SOS_TRPHI               src/SOS_TRPHI.F:749
 *   sosgpu_trphi_spectrum     the same for the wavelengths and output altitudes of a part of a spectrum: one launch
 *   sosgpu_level_flux  <- EMOINS / EPLUS of SOS_OS  src/SOS_OS.F:1447-1456, at the output altitude of an aggregated record
 *   sosgpu_level_flux_spectrum   the same for the wavelengths and output altitudes of a part of a spectrum: one launch
 *   sosgpu_level_absorption   actinic flux and absorbed power per km of a band at the output slots of a levels solve
 *
 * Index conventions (identical to oracle/sos_oracle.h): N = NBMU positive directions, mu[0..N-1] =
 * RMU(1..N) descending; direction jj in -N..N lives at offset jj+N of width W = 2N+1 (slot jj=0 is
 * unused and written as 0); Fourier records rec[s][c][W], c = 0:I 1:Q 2:U; level 0 = TOA.
 */
#ifndef SOSGPU_H
#define SOSGPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SOSGPU_OK            0
#define SOSGPU_E_ARG        -1   /* bad argument / inconsistent sizes (reference IER=-1) */
#define SOSGPU_E_HIP        -2   /* HIP runtime error (sosgpu_last_hip_error) */
#define SOSGPU_E_UNSUPPORTED -3  /* size outside the compiled kernel variants */
#define SOSGPU_E_NODEVICE   -4   /* no gfx950 device visible */
#define SOSGPU_E_RCCL       -5   /* librccl missing or an RCCL call failed */

/* Per-wavelength description (everything SOS_OS receives that does not depend on the CKD bin). */
typedef struct sosgpu_wave {
    int32_t n;          /* NBMU: Gauss + sun (+ user) positive directions, <= 80 (SOS.h:471) */
    int32_t os_nb;      /* max Legendre order of the phase-matrix expansion, <= 200 (SOS.h:480) */
    int32_t n0;         /* 1-based index of the solar direction in mu[] (N0 of SOS_OS); mus = mu[n0-1] */
    int32_t imat_surf;  /* 1: BRDF/BPDF matrices given in d_rsurf (SOS_OS.F:912-925) */
    int32_t ifresnel;   /* 1: flat-sea Fresnel reflection (SOS_OS.F:817,1010,1225) */
    int32_t ipolar;     /* 0: no polarisation (SOS_OS.F:689-699, 928-941), 1: normal */
    int32_t igmax;      /* max scattering order (CTE_DEFAULT_IGMAX = 100) */
    int32_t reserved;
    double  ro;         /* Lambertian albedo */
    double  ind_surf;   /* refractive index (Fresnel) */
    double  ron;        /* molecular depolarisation factor (CTE_MDF) */
} sosgpu_wave;

/* Opaque per-wavelength context living on one device. */
typedef struct sosgpu_ctx sosgpu_ctx;

const char *sosgpu_strerror(int code);
int  sosgpu_last_hip_error(void);
/* Number of visible gfx950 devices, or negative error. */
int  sosgpu_device_count(void);
const char *sosgpu_version(void);

/* Create / destroy a context on `device`.  Host arrays are copied: mu[n], ga[n] (Gauss weights, 0 for
 * the sun/user angles), alpha/beta/gamma/zeta[os_nb+1].  iborm_max = highest Fourier order any bin of
 * this wavelength may need (OS_NB, or 2 for a purely molecular atmosphere, SOS.F:549-550). */
int  sosgpu_create(sosgpu_ctx **out, int device, const sosgpu_wave *wv, const double *mu, const double *ga,
                   const double *alpha, const double *beta, const double *gamma, const double *zeta,
                   int iborm_max);
int  sosgpu_destroy(sosgpu_ctx *cx);
/* sosgpu_create for the nctx contexts of a part of a spectrum in ONE asynchronous call: the small tables of all of them travel
 * to the work area in one staged copy, and one launch (k_ctx_fill) moves each into its context's block and clears what
 * sosgpu_create clears.  The contexts are, field for field and bit for bit, those nctx sosgpu_create calls make; each has its
 * own block of the pool, and sosgpu_destroy, sosgpu_ctx_bytes and every later call treat them alike.
 *  out[nctx]       receives the contexts
 *  specs[nctx]     HOST array; the contexts may differ in every size and flag
 *  d_work, work_bytes   see "Work areas": the job table and the images of the small tables,
 *                  sosgpu_create_spectrum_work_bytes(specs, nctx) bytes
 * Asynchronous on `stream`: nothing is waited for (see "Streams").  On return every context is in the host-side state
 * sosgpu_create leaves and `stream` is noted for sosgpu_destroy, so a context may be destroyed at once (the destroy waits for
 * the fill); its device tables are in place once `stream` has passed the call.  Work queued later on the same stream sees
 * them; work that reads them on OTHER streams (sosgpu_noyaux, a solve, sosgpu_ctx_table's readers) must be ordered after the
 * call by the caller (event / synchronise).
 * Every spec is checked before any device call, allocation or staging block, by the rules of sosgpu_create (sizes, n0, igmax,
 * iborm_max, NULL arrays, no direction with a weight).  SOSGPU_E_ARG for: NULL out, NULL specs with nctx > 0, nctx < 0 or
 * nctx > 65535, a bad spec, the work area's rules.  On any refusal or failure every out[i] is NULL and no context survives
 * (a HIP failure after some contexts were made destroys them).  nctx = 0 returns SOSGPU_OK with nothing queued.  The query is
 * host arithmetic and returns 0 for a list the call would refuse. */
typedef struct sosgpu_ctx_spec {      /* the arguments of one sosgpu_create */
    sosgpu_wave wv;
    const double *mu, *ga, *alpha, *beta, *gamma, *zeta;   /* HOST arrays, as sosgpu_create takes them */
    int32_t iborm_max, reserved;
} sosgpu_ctx_spec;
size_t sosgpu_create_spectrum_work_bytes(const sosgpu_ctx_spec *specs, int nctx);
int    sosgpu_create_spectrum(sosgpu_ctx **out, int device, const sosgpu_ctx_spec *specs, int nctx,
                              void *d_work, size_t work_bytes, void *stream);

/* Surface reflection matrices for imat_surf=1: REAL*4, reference FICSURF record order
 * d_rsurf[s][ab][(J-1)*N+(I-1)] = R_ab(I,J), s = 0..iborm_max (SOS_OS.F:916-925).  Device pointer; the call
 * packs them into the context as FP64 ground-reflection operators in matrix-core fragment order (weights, 2/mu and the
 * Lambertian part folded in).  Host-synchronous: d_rsurf must be complete when the call is made and may be released when it
 * returns (see "Streams" above; no device-wide synchronisation).  Call it after sosgpu_create and before sosgpu_os_solve. */
int  sosgpu_set_surface_matrices(sosgpu_ctx *cx, const float *d_rsurf);
/* Stream-ordered form of the same: the packing is queued on `stream` and nothing is waited for (d_rsurf complete or being
 * produced on `stream`; keep it allocated until the stream has passed this point).  Solves queued later on the same stream
 * see the operators; solves on OTHER streams must be ordered after it by the caller (event / synchronise). */
int  sosgpu_set_surface_matrices_async(sosgpu_ctx *cx, const float *d_rsurf, void *stream);

/* Replaces SOS_NOYAUX (SOS_OS.F:1857-2158) for every Fourier order 0..iborm_max at once; must be called
 * once per context before sosgpu_os_solve.  Fills the context's packed source operators. */
int  sosgpu_noyaux(sosgpu_ctx *cx, void *stream);
/* The two calls above for the contexts of a part of a spectrum at once: sosgpu_set_surface_matrices_async followed by
 * sosgpu_noyaux of every context, in at most FIVE launches whatever nctx is (table forms of the same kernels: a workgroup takes
 * its context from a device table, and the doubles written are, bit for bit, those of the two calls).
 *  ctxs[nctx]      HOST array of contexts of one device; they may differ in N, OS_NB, iborm_max, IPOLAR, Fresnel and surface
 *  d_rsurf[nctx]   HOST array of DEVICE pointers, each laid out as sosgpu_set_surface_matrices takes it; NULL for a context with
 *                  imat_surf = 0.  The whole argument may be NULL when no context has matrices (the fifth launch, the ground
 *                  operators, is made only when some entry is non-NULL).  Keep the matrices allocated until `stream` has passed
 *                  the call.
 *  d_work, work_bytes   see "Work areas": the table of the contexts and the list of matrix pointers,
 *                  sosgpu_noyaux_spectrum_work_bytes(nctx) bytes
 * Asynchronous: nothing is waited for and no device memory is allocated.  On return every context is in the host-side state the
 * two calls leave (its ground operators registered, `stream` noted for sosgpu_destroy); once `stream` has passed the call its
 * tables are filled.  Call sosgpu_ctx_table AFTER this call, not before: the table copies the ground-operator pointers this
 * call registers.
 * Checked before anything is queued or any context is changed, SOSGPU_E_ARG for: NULL ctxs or d_work, a NULL entry of ctxs,
 * nctx < 0 or nctx > 65535, contexts on different devices, imat_surf = 1 with a NULL matrix pointer, a matrix pointer for a
 * context with imat_surf = 0, the work area's rules.  nctx = 0 returns SOSGPU_OK with nothing queued. */
size_t sosgpu_noyaux_spectrum_work_bytes(int nctx);
int  sosgpu_noyaux_spectrum(sosgpu_ctx *const *ctxs, int nctx, const float *const *d_rsurf, void *d_work, size_t work_bytes,
                            void *stream);
/* Debug/parity accessor: copies the six kernels of order `is` to host as the reference lays them
 * out, X[(j+N)*W + (k+N)] = X(J,K), in the order BP,GR,GT,ARR,ART,ATT, then XPL,XRL,XTL (W each).
 * Synchronous.  out must hold 6*W*W + 3*W doubles. */
int  sosgpu_noyaux_fetch(sosgpu_ctx *cx, int is, double *out);

/* Replaces the per-bin SOS_OS calls of the CKD loop (SOS_PROC.F:3459-3594 -> SOS.F:554 -> SOS_OS.F:303).
 *  nb          number of bins in this batch
 *  lp          padded level count (row stride of d_prof), >= max(nt)+1
 *  d_nt[nb]    NT of each bin (int32)
 *  d_iborm[nb] IBORM of each bin (int32; SOS.F:549-550), <= iborm_max
 *  d_prof[nb][3][lp]   H, XDEL, YDEL after the truncation rescale of SOS.F:523-543
 *  d_jout[nb]  output level pair for ZOUT != -1: levels jout-1 and jout bracket ZOUT (SOS_OS.F:1514-1520);
 *              0 = standard output (ZOUT = -1: TOA up, ground down).  May be NULL (= all 0).
 *  d_zz[nb]    interpolation weight ZZ (SOS_OS.F:1520); ignored when jout = 0.  May be NULL.
 * outputs
 *  d_rec[nb][iborm_max+1][3][W]  Fourier records; only orders 0..d_norders[b]-1 hold records on return (the reference's FICOS
 *                                file of a bin holds one record per order run, SOS_OS.F:1571-1575): a buffer zero-filled by the
 *                                caller is zero beyond them (the order-parallel launch form computes a few orders past the
 *                                stop and clears their rows again)
 *  d_norders[nb]                 number of Fourier orders run (int32); -1 = malformed bin (NT < 1, NT >= lp, IBORM out of
 *                                range: the reference's IER = -1), nothing else is written for it
 *  d_iglast[nb][iborm_max+1]     last scattering order computed per Fourier order (int32)
 *  d_flux[nb][2]                 EMOINS, EPLUS (SOS_OS.F:1447-1456)
 */
int  sosgpu_os_solve(sosgpu_ctx *cx, int nb, int lp, const int32_t *d_nt, const int32_t *d_iborm,
                     const double *d_prof, const int32_t *d_jout, const double *d_zz,
                     double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux, void *stream);

/* Several output altitudes from ONE solve.  The output altitude (-SOS.OutputAlt, ZOUT) does not enter the solve: it only
 * chooses the two levels whose field is captured and interpolated (SOS_OS.F:1511-1534); the stop tests, the orders run and
 * the fluxes come from TOA and ground.  Each bin here carries nz output slots (jout, zz), and the record set of slot k is,
 * bit for bit, the d_rec of sosgpu_os_solve with d_jout / d_zz = that slot's (jout 0: the standard output).
 *  nz                    1 .. SOSGPU_MAX_OUTPUT_LEVELS (SOSGPU_E_ARG otherwise)
 *  d_jout[nz][nb], d_zz[nz][nb]   output levels of every slot and bin (sosgpu_output_levels), both required
 *  d_rec[nz][nb][iborm_max+1][3][W]  one ordinary record array per slot: sosgpu_aggregate / sosgpu_reduce / sosgpu_trphi take
 *                        slot k at d_rec + k nb (iborm_max+1) 3 W as they take the d_rec of sosgpu_os_solve
 *  d_norders, d_iglast, d_flux   as sosgpu_os_solve (common to the slots); a bin with a jout outside 0 .. NT is malformed
 *                        (norders = -1)
 * Every other argument and rule as sosgpu_os_solve.  The cost over a single-altitude solve is the capture of the slots'
 * levels: two field reads and a few lane-private state accesses per slot, row and scattering order. */
#define SOSGPU_MAX_OUTPUT_LEVELS 16
int  sosgpu_os_solve_levels(sosgpu_ctx *cx, int nb, int lp, const int32_t *d_nt, const int32_t *d_iborm,
                            const double *d_prof, int nz, const int32_t *d_jout, const double *d_zz,
                            double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux, void *stream);
/* Output levels of nz altitudes for bins profiled by sosgpu_profile: from its d_prof (H), d_zprof and d_nt, the level,
 * weight and optical depth sosgpu_profile computes for zout (SOS.F:570-582, SOS_OS.F:1514-1520), with the same arithmetic:
 *  zout[nz]          altitudes (km, host array), -1 = standard output (jout 0, zz 0, TAUOUT = H(0))
 *  d_jout[nz][nb], d_zz[nz][nb], d_tauout[nz][nb]   device outputs; a flagged bin (NT < 1) gets 0, 0, 0
 * One small kernel on `stream`. */
int  sosgpu_output_levels(sosgpu_ctx *cx, int nb, int lp, const double *d_prof, const double *d_zprof, const int32_t *d_nt,
                          int nz, const double *zout, int32_t *d_jout, double *d_zz, double *d_tauout, void *stream);
/* The optical depth alone, on any cumulative-depth row of the bins: the statements of sosgpu_output_levels for the level, the
 * weight and (1 - zz) H(j-1) + zz H(j) (same roundings, same -1 rule H(0), a flagged bin gets 0), with
 *  d_h, h_stride     the row of bin b starts at d_h + b * h_stride (doubles): lp for the d_hvrai of sosgpu_profile_true,
 *                    3 lp for the H row of d_prof -- where d_tau is sosgpu_output_levels' d_tauout bit for bit
 *  d_tau[nz][nb]     device output
 * No context is needed.  nb = 0 queues nothing.  One small kernel on `stream`. */
int  sosgpu_output_depths(int device, int nb, int lp, const double *d_h, size_t h_stride, const double *d_zprof,
                          const int32_t *d_nt, int nz, const double *zout, double *d_tau, void *stream);

/* The scratch of the streamed solver (level grids beyond 64 levels) is kept by the library when a context is destroyed and
 * handed to the next context that needs one (at most 8 buffers and 8 GiB per process): a context per wavelength would
 * otherwise pay a 60-1000 MB hipMalloc per call.  sosgpu_trim() returns that memory to the device, and frees the pinned
 * staging blocks whose copies have passed. */
int  sosgpu_trim(void);

/* Many wavelengths in ONE launch (hyperspectral runs, BASELINE config 5: each wavelength has only 5-100 CKD bins, a fraction
 * of the 512 workgroups the chip hosts).  The reference runs SOS_PROC once per wavelength (binding/run_sos.py:640); here the
 * bin loops SOS_PROC.F:3459-3594 of nctx wavelengths are concatenated and every bin carries the index of its wavelength.
 *   sosgpu_ctx_table   copies the device-side description of nctx contexts (sosgpu_ctx_table_entry_bytes() each) into the
 *                      caller's device buffer d_table, ordered on `stream` (nothing is waited for: the copy comes from a pinned
 *                      block the library recycles).  All contexts must live on one device and agree in
 *                      N, iborm_max and IMAT_SURF (E_ARG otherwise).  The table refers to the contexts' operator tables: it
 *                      stays valid until one of them is destroyed or has sosgpu_set_surface_matrices called again -- a
 *                      destroyed context's memory is recycled at once, so wait for the launches that use the table first.
 *   sosgpu_os_solve_multi   sosgpu_os_solve with d_ctx_of_bin[nb] (int32, 0..nctx-1): bin b is solved with the operators of
 *                      table entry d_ctx_of_bin[b].  `cx` is any context of the table (it provides the variant selection, the
 *                      streamed variant's scratch and the timing events).  d_order[nb] (int32, a permutation of 0..nb-1) or
 *                      NULL: workgroup i solves bin d_order[i] -- workgroups start in index order, so listing the costliest
 *                      bins first shortens the tail of the launch while the bins stay grouped by wavelength in memory.
 *                      All other arguments as sosgpu_os_solve; feed sosgpu_aggregate with one segment per wavelength. */
size_t sosgpu_ctx_table_entry_bytes(void);
int  sosgpu_ctx_table(sosgpu_ctx *const *ctxs, int nctx, void *d_table, void *stream);
int  sosgpu_os_solve_multi(sosgpu_ctx *cx, const void *d_table, const int32_t *d_ctx_of_bin, const int32_t *d_order, int nb, int lp,
                           const int32_t *d_nt, const int32_t *d_iborm, const double *d_prof, const int32_t *d_jout,
                           const double *d_zz, double *d_rec, int32_t *d_norders, int32_t *d_iglast, double *d_flux,
                           void *stream);
/*   sosgpu_os_solve_multi_levels   the two joined: one launch over the bins of many wavelengths (table rules of
 *                      sosgpu_os_solve_multi), each bin with nz output slots (argument rules of sosgpu_os_solve_levels:
 *                      1 <= nz <= SOSGPU_MAX_OUTPUT_LEVELS, d_jout and d_zz required).  Layout as sosgpu_os_solve_levels:
 *                      d_jout[nz][nb], d_zz[nz][nb], d_rec[nz][nb][iborm_max+1][3][W]; slot k of bin b equals, bit for bit,
 *                      the record of sosgpu_os_solve with that bin's context and the slot's (jout, zz).  Feed sosgpu_aggregate
 *                      slot by slot (d_rec + k nb (iborm_max+1) 3 W), one segment per wavelength, with that slot's TAUOUT. */
int  sosgpu_os_solve_multi_levels(sosgpu_ctx *cx, const void *d_table, const int32_t *d_ctx_of_bin, const int32_t *d_order,
                                  int nb, int lp, const int32_t *d_nt, const int32_t *d_iborm, const double *d_prof, int nz,
                                  const int32_t *d_jout, const double *d_zz, double *d_rec, int32_t *d_norders,
                                  int32_t *d_iglast, double *d_flux, void *stream);

/* Diffuse transmissions of the -SOS.Trans option (SOS.F:600-635) for the bins of MANY wavelengths in one solve.  The reference
 * runs SOS_OS once per direction J with N0 = J, Fourier order 0 only, RHO = 0 and no surface, and keeps EMOINS: TDIFMUG(J).  Here
 * every (context, direction) pair becomes a child entry of a device context table -- the context's own order-0 operators, which
 * never touch the solar slot, with n0 = J, mus = mu[J-1], a black ground and order-1 vectors of its own, formed on the device by
 * the statements of sosgpu_noyaux -- and every (bin, direction) pair an item of one order-0 multi-wavelength solve:
 *   d_tdifmug[b][J-1] = the d_flux[.][0] of sosgpu_os_solve for a context created with n0 = J, iborm_max = 0, ro = 0,
 *                       imat_surf = ifresnel = 0 and d_iborm = 0, bit for bit; 0 for a malformed bin (NT < 1, NT >= lp).
 *  ctxs[nctx]        HOST array of contexts of one device whose operators have been queued (sosgpu_noyaux or
 *                    sosgpu_noyaux_spectrum, on `stream` or complete); they must agree in N and may differ in OS_NB,
 *                    iborm_max, IPOLAR, surface and Fresnel flags, none of which a child inherits
 *  d_ctx_of_bin[nb]  index into ctxs of every bin (int32), or NULL with nctx = 1; a bin whose index is out of range is
 *                    treated as malformed
 *  d_nt[nb], d_prof[nb][3][lp]   as sosgpu_os_solve takes them
 *  d_work, work_bytes   see "Work areas": the context table, followed by the child table, the children's vectors and the items'
 *                    arrays (the profile rows are replicated per direction: 24 N lp bytes per bin)
 * Asynchronous: nothing is waited for and no device memory is allocated -- except for level grids beyond the LDS-resident
 * solver (lp > 64), whose streamed-field scratch comes from where sosgpu_os_solve_multi takes it (ctxs[0], at most 4 GiB at a
 * time).  Launches: two for the child table, one for the items, the solve, one gather -- whatever N, nctx and nb are; the new
 * kernels index children and items by blockIdx.x, so nctx N and nb N are bounded by 2^31 - 1 only (SOSGPU_E_ARG beyond), and
 * the solve is split only where 4 GiB of scratch do not hold all items.  `stream` is noted for sosgpu_destroy on every context.
 * Checked before anything is queued or a staging block is taken, SOSGPU_E_ARG for: NULL ctxs, d_nt, d_prof, d_tdifmug or
 * d_work, a NULL context or one whose operators were never queued, contexts on different devices or with different N,
 * nctx < 1, nb < 0, lp < 2, d_ctx_of_bin = NULL with nctx > 1, the work area's rules; SOSGPU_E_UNSUPPORTED when (N, lp) has no
 * solver variant.  nb = 0 returns SOSGPU_OK with nothing queued. */
size_t sosgpu_trans_spectrum_work_bytes(sosgpu_ctx *const *ctxs, int nctx, int nb, int lp);
int    sosgpu_trans_spectrum(sosgpu_ctx *const *ctxs, int nctx, const int32_t *d_ctx_of_bin, int nb, int lp,
                             const int32_t *d_nt, const double *d_prof,
                             double *d_tdifmug /*[nb][N]*/, void *d_work, size_t work_bytes, void *stream);

/* Spherical albedo of the atmosphere for the bins of many wavelengths, in ONE order-0 solve.  Per bin
 *   d_salb[b] = 2 sum_j ga_j mu_j A_j,     d_plane[b][j-1] = A_j (the plane albedo for incidence mu_j),
 * with A_j the up-going flux (the d_flux[.][1] of sosgpu_os_solve) of the order-0 solve over a black ground with incidence
 * J = j that sosgpu_trans_spectrum queues -- the same child table, items, work area and solve.  The sum runs in ascending j,
 * s = s + ((2 ga_j) mu_j) A_j.  Directions of quadrature weight 0 (the inserted solar angle, the user angles) are not
 * solved: their column of d_plane is 0 and they add nothing.
 *  from_below != 0   the atmosphere is lit from the GROUND: every item's profile is mirrored in the vertical about the bin's own
 *                    NT (h'[k] = h[NT] - h[NT-k], xdel'[k] = xdel[NT-k], ydel'[k] = ydel[NT-k], zeros past NT).  This is the S
 *                    of rho_toa = rho_path + T_down T_up rho_s / (1 - S rho_s): with it the ground flux of sosgpu_os_solve
 *                    over a Lambert ground of albedo a obeys E_down(a) (1 - a S) = E_down(0) to the stop test of the
 *                    scattering orders.  0: seen from space over a black ground (the planetary quantity).
 *  d_plane           [nb][N], or NULL when only d_salb is wanted
 * S belongs to the truncated, equivalent atmosphere of d_prof, as TDIFMUG does.  A malformed bin (NT < 1, NT >= lp, context
 * index out of range) gets d_salb = 0 and a zero row of d_plane.
 * Everything else -- ctxs, d_ctx_of_bin, d_nt, d_prof, d_work and its size (sosgpu_albedo_spectrum_work_bytes equals
 * sosgpu_trans_spectrum_work_bytes), asynchrony, the refusals (d_salb in the place of d_tdifmug) checked before anything is
 * queued or a staging block is taken, nb = 0, the noted stream -- is as sosgpu_trans_spectrum states it.  Launches: two for
 * the child table, one for the items, the solve, one for the sums. */
size_t sosgpu_albedo_spectrum_work_bytes(sosgpu_ctx *const *ctxs, int nctx, int nb, int lp);
int    sosgpu_albedo_spectrum(sosgpu_ctx *const *ctxs, int nctx, const int32_t *d_ctx_of_bin, int nb, int lp,
                              const int32_t *d_nt, const double *d_prof, int from_below,
                              double *d_plane /*[nb][N], may be NULL*/, double *d_salb /*[nb]*/,
                              void *d_work, size_t work_bytes, void *stream);
/* Band value of the spherical albedo: d_out[g] = sum_b d_aik[b] d_salb[b] over the bins d_seg[g] .. d_seg[g+1]-1 of segment g
 * (sosgpu_aggregate's per-thread striding and fixed tree; a segment of one bin gives aik * salb exactly).  With sum aik = 1 it
 * is the aik-weighted mean; the coupling formula is exact per bin only.  One launch; nseg = 0 queues nothing; SOSGPU_E_ARG for
 * nseg < 0 or a NULL pointer.  No context is needed. */
int    sosgpu_albedo_band(int nseg, const int32_t *d_seg /*[nseg+1]*/, const double *d_aik, const double *d_salb,
                          double *d_out /*[nseg]*/, int device, void *stream);

/* Replaces SOS_AGGREGATE (SOS_AGGREGATE.F:372-488) for nseg independent wavelengths/bands at once:
 * segment g covers bins seg[g]..seg[g+1]-1 of d_rec; seg[0] = 0, seg[nseg] = nb.  One big band (nseg = 1,
 * nb > 128) is reduced in chunks of 64 bins (deterministic; the strict serial bin order of the reference is kept for
 * small bands and multi-band calls).  nb = 0 (a rank whose shard of the band is empty) is allowed with nseg = 1: the
 * outputs are the neutral element of the cross-rank reduce.
 *  d_scal[nb][4]     per-bin scalars: TDIFMUS, TTOT_TRONC, TTOT_VRAI, TAUOUT
 *  d_tdifmug[nb][N]  per-bin diffuse transmissions TDIFMUG(1..N) of the -SOS.Trans option (SOS.F:611-635), or NULL
 *  d_out_rec[nseg][iborm_max+1][3][W] = sum_b aik[b] * rec[b]   (orders a bin did not run count as zero records,
 *                    SOS_AGGREGATE.F:357-413; bins with norders < 0 are skipped)
 *  d_out_scal[nseg][SOSGPU_SCAL_BASE + N]:
 *      [0..2] sum aik*{TDIFMUS, EMOINS, EPLUS}     [3..5] sum aik*exp(-{TTOT_TRONC, TTOT_VRAI, TAUOUT})
 *      [6]    sum aik        [7] max norders       [8] -(min norders): > 0 when a bin of the segment failed
 *      [9]    0 (sosgpu_level_transmission, queued behind this call, puts sum aik*exp(-tau_vrai(z)) of an output slot here)
 *      [10..10+N) sum aik*TDIFMUG(j)     (SOS_AGGREGATE.F:452-459)
 *   Across GPUs elements 7 and 8 combine with MAX, all others (and d_out_rec) with SUM; the -ln of the three
 *   transmissions (SOS_AGGREGATE.F:467-488) is applied afterwards (sosgpu_reduce does all of this).
 */
#define SOSGPU_SCAL_BASE 10
int  sosgpu_aggregate(sosgpu_ctx *cx, int nb, int nseg, const int32_t *d_seg, const double *d_aik,
                      const double *d_rec, const int32_t *d_norders, const double *d_flux, const double *d_scal,
                      const double *d_tdifmug, double *d_out_rec, double *d_out_scal, void *stream);
/* Band transmission of a per-slot optical depth (the untruncated depth down to an output altitude, sosgpu_output_depths on
 * d_hvrai): for slot k = 0..nz-1 and segment g, sum_b aik[b] exp(-d_tau[k][b]) over the bins of the segment, written into
 * element [9] of the scalar block at d_out_scal + k * slot_stride + g * block_width (doubles; block_width =
 * SOSGPU_SCAL_BASE + N of the blocks sosgpu_aggregate wrote, slot_stride >= nseg * block_width when nz > 1).  Bins with
 * norders < 0 are skipped, and the sum has sosgpu_aggregate's shape (per-thread striding, fixed tree): a slot whose depth is
 * TTOT_VRAI gets the bits of element [4].  Queue it on the stream of the slots' sosgpu_aggregate calls, behind them (they
 * write 0 there); the element then sums across GPUs like its neighbours.  One launch for all slots and segments; nb = 0
 * queues nothing.  No context is needed. */
int  sosgpu_level_transmission(int device, int nb, int nseg, const int32_t *d_seg, const double *d_aik, const int32_t *d_norders,
                               int nz, const double *d_tau, double *d_out_scal, size_t slot_stride, int block_width,
                               void *stream);

/* Cross-GPU step of SOS_AGGREGATE for callers without torch.distributed (C / Fortran hosts): one RCCL
 * all-reduce (ncclDouble, ncclSum) over xGMI of the packed buffer d_buf[nseg][(iborm_max+1)*3*W + SOSGPU_SCAL_BASE + N]
 * (records followed by the scalar block, the layout sosgpu_pack writes) plus one 2-element MAX all-reduce per segment
 * for elements 7 and 8.  `comm` is an ncclComm_t (as void*) the caller created -- sosgpu_comm_* wrap ncclGetUniqueId /
 * ncclCommInitRank / ncclCommDestroy so that a host needs no RCCL headers.  librccl is resolved at the first call
 * (dlopen), so single-GPU users carry no RCCL dependency.  nranks = 1 is a no-op. */
#define SOSGPU_UNIQUE_ID_BYTES 128
int  sosgpu_comm_unique_id(char id[SOSGPU_UNIQUE_ID_BYTES]);
int  sosgpu_comm_init_rank(void **comm, int nranks, const char id[SOSGPU_UNIQUE_ID_BYTES], int rank);
int  sosgpu_comm_destroy(void *comm);
/* d_out_rec / d_out_scal of sosgpu_aggregate -> d_buf (device-to-device copies on `stream`) and back. */
int  sosgpu_pack(sosgpu_ctx *cx, int nseg, const double *d_out_rec, const double *d_out_scal, double *d_buf, void *stream);
int  sosgpu_unpack(sosgpu_ctx *cx, int nseg, const double *d_buf, double *d_out_rec, double *d_out_scal, void *stream);
int  sosgpu_reduce(sosgpu_ctx *cx, void *comm, int nseg, double *d_buf, void *stream);

/* Replaces SOS_GLITTER (SOS_GLITTER.F:229-371: SOS_GSF + SOS_MAT_FRESNEL + SOS_MAT_REFLEXION +
 * SOS_MISE_FORMAT, no temporary files).  Host inputs mu[n], chr[n] (Gauss weights), wind (m/s), ind (water
 * refractive index), orders OS_NB, OS_NS, OS_NM (>= OS_NB+OS_NS).  Device outputs:
 *  d_rsurf[os_nb+1][9][N][N]  REAL*4 matrices in GLITTER-file record order (feed to
 *                             sosgpu_set_surface_matrices with imat_surf = 1)
 *  d_il[N(N+1)/2]             series length IL of each angle pair (I1 = 1..N, I2 = 1..I1), SOS_GLITTER.F:676
 *  d_e[N(N+1)/2][os_nm+1]     Fourier coefficients E(0:IL) of the facet function, zero beyond IL
 * Synchronous with respect to the host arrays; kernels run on `stream`.
 * SOSGPU_E_ARG, before any device work, unless 2 <= OS_NS, OS_NB + OS_NS <= OS_NM <= 2000 and the reflection kernel's
 * work area fits the 160 KiB of LDS of a workgroup: 8 (OS_NM + 1 + 12 (OS_NS + 1)) <= 163840 bytes. */
int  sosgpu_glitter(int device, int n, const double *mu, const double *chr, double wind, double ind,
                    int os_nb, int os_ns, int os_nm, float *d_rsurf, int32_t *d_il, double *d_e, void *stream);
/* Host helper used by sosgpu_glitter, exposed for parity tests: SOS_MAT_FRESNEL (SOS_SURFACE.F:1235-1603)
 * including the 4(E15.8) text round trip; out[4][os_ns+1] = alpha, beta, gamma, zeta. */
int  sosgpu_mat_fresnel_host(int n, const double *mu, const double *chr, double ind, int os_ns, double *out);

/* Replaces SOS_TRPHI (SOS_TRPHI.F:749-1243) + SOS_POLAR (:1843) for nphi azimuths at once.
 *  nf           number of Fourier orders in d_rec (records beyond are ignored)
 *  d_rec[nf][3][W]  aggregated Fourier records (sosgpu_aggregate output, after the cross-GPU reduce)
 *  tau, tauout  total (truncated) optical depth and optical depth of the output level (TTOT_TRONC, TAUOUT)
 *  d_phi[nphi]  azimuths in radians
 *  igli         1: add the directly reflected Cox-Munk glint (needs wind); the flat-sea sun glint is added
 *               when the context has ifresnel = 1
 *  d_out[nphi][7][W]: XIT, XQT, XUT, ANGDIFF (deg), polarisation angle, rate (%), polarised radiance;
 *               slot jj = 0 is zero.
 *  land         NULL, or the land-surface model of -SURF.Type 3..7 whose directly reflected term is added
 *               (SOS_TRPHI.F:1047-1200): Roujean BRDF for every type, plus the BPDF of type 4..7. */
typedef struct sosgpu_land {
    int32_t isurf;            /* 3 Roujean, 4 + Rondeaux-Herman, 5 + Breon, 7 + Maignan (SOS_PREPA_OS.F:479-497); 6 (Nadal) is
                               * refused with SOSGPU_E_UNSUPPORTED, as the reference's SOS_PROC refuses it */
    int32_t reserved;
    double  k0, k1, k2;       /* Roujean coefficients */
    double  alpha, beta;      /* Nadal (kept for layout compatibility, unused) */
    double  coef_c;           /* Maignan C exp(-NDVI) */
} sosgpu_land;
int  sosgpu_trphi(sosgpu_ctx *cx, int nf, const double *d_rec, double tau, double tauout, int nphi,
                  const double *d_phi, int igli, double wind, const sosgpu_land *land, double *d_out, void *stream);

/* sosgpu_trphi for many (context, record, azimuth list) jobs -- the wavelengths and output altitudes of a part of a spectrum -- in
 * ONE launch: one workgroup per (job, azimuth) pair, each finding its job in a device array of job entries.  Block j of d_out holds,
 * bit for bit, what sosgpu_trphi writes for job j's arguments.
 *  jobs[njobs]     HOST array; jobs may share a context, a record pointer and an azimuth range
 *  d_phi[nphi_total]  DEVICE azimuths (radians) of the whole call; job j reads d_phi[phi_off .. phi_off + nphi)
 *  d_out           DEVICE, the blocks [nphi_j][7][W_j] of the jobs back to back, in job order
 *  d_work, work_bytes   see "Work areas": the job entries, sosgpu_trphi_spectrum_work_bytes(njobs) bytes
 * Asynchronous: one launch, nothing is waited for and no device memory is allocated; `stream` is noted for sosgpu_destroy on
 * every context of the call.  Records, azimuths and contexts must stay alive until `stream` has passed the call.
 * Checked before anything is queued, SOSGPU_E_ARG for: NULL jobs, d_phi, d_out or d_work, njobs < 0 or njobs > 65535, a NULL cx
 * or d_rec, nf < 1 or nf > iborm_max + 1 of the job's context, nphi < 1, phi_off < 0 or phi_off + nphi > nphi_total, contexts
 * on different devices, a land->isurf outside 3..7, the work area's rules; SOSGPU_E_UNSUPPORTED for isurf = 6, as sosgpu_trphi.
 * njobs = 0 returns SOSGPU_OK with nothing queued. */
typedef struct sosgpu_trphi_job {
    sosgpu_ctx *cx;            /* context of the wavelength (HOST handle) */
    const double *d_rec;       /* [>= nf][3][W] aggregated records (DEVICE) */
    int32_t nf, igli;
    int32_t phi_off, nphi;     /* this job's azimuths: d_phi[phi_off .. phi_off + nphi) */
    double tau, tauout, wind;
    const sosgpu_land *land;   /* HOST pointer or NULL, as sosgpu_trphi takes it */
} sosgpu_trphi_job;
size_t sosgpu_trphi_spectrum_work_bytes(int njobs);
int  sosgpu_trphi_spectrum(const sosgpu_trphi_job *jobs, int njobs, const double *d_phi, int nphi_total,
                           double *d_out, void *d_work, size_t work_bytes, void *stream);

/* Diffuse fluxes of an aggregated record at its output altitude: d_out[0] = E-(z), d_out[1] = E+(z), the Gauss quadrature the
 * reference applies to the order-0 intensity at the ground and at the top of the atmosphere (EMOINS / EPLUS, SOS_OS.F:1447-1456):
 *   e = sum_{j=1..N} mu_j ga_j I(-+j)   (- : E-, + : E+; j ascending, products formed as (mu ga) I),   E = -e * 2 / TAB,
 * TAB = -mu[n0-1].  d_rec: DEVICE, the aggregated records of one output slot (sosgpu_aggregate); only its order-0 intensity row
 * d_rec[0][0][W] is read.  For the standard output (altitude -1) E- is the ground value and E+ the top-of-atmosphere value.
 * Asynchronous on `stream` (one launch), noted for sosgpu_destroy.  SOSGPU_E_ARG for a NULL cx, d_rec or d_out. */
int  sosgpu_level_flux(sosgpu_ctx *cx, const double *d_rec, double *d_out /*[2]*/, void *stream);

/* sosgpu_level_flux for many (context, record) jobs -- the wavelengths and output altitudes of a part of a spectrum -- in ONE
 * launch: one thread per (job, hemisphere).  d_out[j][0..1] holds, bit for bit, what sosgpu_level_flux writes for job j.
 *  jobs[njobs]     HOST array; jobs may share a context and a record pointer
 *  d_out[njobs][2] DEVICE
 *  d_work, work_bytes   see "Work areas": the job entries, sosgpu_level_flux_spectrum_work_bytes(njobs) bytes
 * Asynchronous: one launch, nothing is waited for and no device memory is allocated; `stream` is noted for sosgpu_destroy on
 * every context of the call (the kernel reads their mu and ga).  Records and contexts must stay alive until `stream` has passed
 * the call.  Checked before anything is queued, SOSGPU_E_ARG for: NULL jobs, d_out or d_work, njobs < 0 (or > 2^30 - 1), a NULL
 * cx or d_rec, contexts on different devices, the work area's rules.  njobs = 0 returns SOSGPU_OK with nothing queued. */
typedef struct sosgpu_flux_job { sosgpu_ctx *cx; const double *d_rec; } sosgpu_flux_job;
size_t sosgpu_level_flux_spectrum_work_bytes(int njobs);
int  sosgpu_level_flux_spectrum(const sosgpu_flux_job *jobs, int njobs, double *d_out /*[njobs][2]*/,
                                void *d_work, size_t work_bytes, void *stream);

/* Actinic flux and absorbed power of a band at the output slots of a levels solve (sosgpu_os_solve_levels,
 * sosgpu_os_solve_multi_levels): the angular moment of the captured order-0 field that carries no factor mu, and the radiative
 * power absorbed per kilometre -- the shortwave heating rate up to the factor mu_s E0 / (rho c_p).  All values are in the unit
 * of sosgpu_level_flux, i.e. relative to the irradiance mu_s E0 at the top of the atmosphere on a horizontal plane.  Per slot k
 * and bin b, with N, n0, mu, ga of the bin's context, row = d_rec[k][b][0][0][0..W) (direction jj at offset jj + N),
 * (j, zz) = (d_jout[k][b], d_zz[k][b]) and H / XDEL / YDEL = d_prof[b][0..2][.], every step one rounding, no FMA:
 *   s_dn = sum_{jj=1..N} ga_jj row[N - jj]  (s_up: row[N + jj]; jj ascending),   a_dn = -s_dn * 2 / TAB,  a_up = -s_up * 2 / TAB,
 *   TAB = -mu[n0-1]  (sosgpu_level_flux's statements without the factor mu),   a_dir = exp(-d_tauout[k][b] / mu_s) / mu_s,
 *   om    = (1 - zz) (XDEL[j-1] + YDEL[j-1]) + zz (XDEL[j] + YDEL[j]),
 *   slope = (H[j] - H[j-1]) / (zprof[j-1] - zprof[j]),   0 when zprof[j-1] <= zprof[j] (levels that coincide after F10.5),
 *   q     = slope * (1 - om) * (a_dn + a_up + a_dir)          [per km].
 * The single-scattering albedo is a LEVEL quantity here: the solver's discretisation obeys, for layer j,
 *   F_net(j-1) - F_net(j) = dtau_j / 2 ((1 - om_{j-1}) A_{j-1} + (1 - om_j) A_j)
 * with om_j = XDEL[j] + YDEL[j]; q follows the reference's linear interpolation between the two levels that bracket z, and its
 * integral over a layer is q(z_mid) dz.  The truncation rescale leaves (1 - om) dtau unchanged: q belongs to the true atmosphere.
 *   d_out[k][g][0..3] = sum_b d_aik[b] * {a_dir, a_dn, a_up, q}   over the bins d_seg[g] .. d_seg[g+1]-1 with d_norders[b] >= 0,
 * with sosgpu_level_transmission's shape (256 threads stride over the bins, serial within a thread, fixed tree): a segment of
 * one bin gives aik * term exactly.  a_dir of a band is the exact band mean sum aik exp(-tau_b / mu_s) / mu_s, not the value at
 * the band-mean depth.  A standard-output slot (jout = 0) mixes the ground and the top of the atmosphere: its bins add nothing
 * and its block is zeros.  A bin with jout outside 0 .. NT is skipped like a failed bin.
 *  cx                the context of the bins; with d_table any context of the table (it provides N and iborm_max)
 *  d_table, d_ctx_of_bin[nb]   NULL: every bin with cx; else the buffer of sosgpu_ctx_table and the entry of every bin, as
 *                    sosgpu_os_solve_multi takes them (contexts of different mu but equal N)
 *  d_nt[nb], d_prof[nb][3][lp]   as the solve took them;  d_zprof[nb][lp]   level altitudes (km, descending; sosgpu_profile)
 *  d_jout, d_zz, d_tauout [nz][nb]   of sosgpu_output_levels;  d_rec[nz][nb][iborm_max+1][3][W], d_norders[nb]   of the solve
 *  d_seg[nseg+1], d_aik[nb]   as sosgpu_aggregate takes them
 * Asynchronous: one launch on `stream` (queue it behind the solve), no allocation, no work area; `stream` is noted for
 * sosgpu_destroy on cx.  nb = 0 or nseg = 0 queues nothing.  Checked before anything is queued, SOSGPU_E_ARG for: a NULL cx,
 * d_nt, d_prof, d_zprof, d_jout, d_zz, d_tauout, d_rec, d_norders, d_seg, d_aik or d_out, nz outside
 * 1 .. SOSGPU_MAX_OUTPUT_LEVELS, lp < 2, nb < 0, nseg < 0, d_table without d_ctx_of_bin. */
int  sosgpu_level_absorption(sosgpu_ctx *cx, const void *d_table /*NULL: cx alone*/, const int32_t *d_ctx_of_bin /*NULL with d_table NULL*/,
                             int nb, int lp, const int32_t *d_nt, const double *d_prof, const double *d_zprof /*[nb][lp]*/, int nz,
                             const int32_t *d_jout, const double *d_zz, const double *d_tauout /*[nz][nb] each*/,
                             const double *d_rec /*[nz][nb][iborm_max+1][3][W]*/, const int32_t *d_norders, int nseg,
                             const int32_t *d_seg, const double *d_aik, double *d_out /*[nz][nseg][4]*/, void *stream);

/* Every irradiance quantity of a solved group at its output slots, in ONE launch: what the flux, split and absorption rows of a
 * levels pass are made of, formed from the order-0 row of every bin and summed with aik -- without sosgpu_aggregate,
 * sosgpu_level_flux_spectrum, sosgpu_level_transmission and sosgpu_level_absorption, whose statements it executes.  Only the
 * order-0 intensity row d_rec[k][b][0][0][0..W) of every slot is read: iborm_max of the context may be 0 (a context that holds
 * the order-0 operators alone, solved with d_iborm = 0), the record layout is the context's own [iborm_max+1][3][W].
 *   d_out[k][g][c], c < SOSGPU_IRRADIANCE_COLS, over the bins d_seg[g] .. d_seg[g+1]-1 (bounds clamped to 0 .. nb) of slot k:
 *     [0..3]  sum aik {a_dir, a_dn, a_up, q}: the bits of sosgpu_level_absorption's block
 *     [4, 5]  sum aik {E-_b, E+_b}, E-+_b = sosgpu_level_flux's statement on the bin's OWN order-0 row (products (mu ga) I, j
 *             ascending, E = -e * 2 / TAB), each then one multiply by aik and one add.  The chain through sosgpu_aggregate takes
 *             the moment of the summed record instead: for a segment of one bin with aik = 1 the two are equal bit for bit,
 *             for several bins at most nbins + 2 N roundings of non-negative terms differ (below 1e-13 relative for 300 bins,
 *             N = 85).  A standard-output slot (jout = 0) is no exception: its record row is the ground going down and the top
 *             going up, and [4, 5] are what sosgpu_level_flux gives for that slot (the flux rows of the levels passes); its
 *             [0..3] are 0
 *     [12,13] sum aik {EMOINS, EPLUS} of d_flux, the solve's own pair: the bits of elements 1 and 2 of sosgpu_aggregate's
 *             scalar block, in every slot.  They agree with [4, 5] of a standard-output slot to rounding without surface
 *             matrices and to some 1e-9 with them, as the reference's EPLUS and its own record do
 *     [6..8]  sum aik exp(-{TTOT_TRONC, TTOT_VRAI, TAUOUT(slot k)}) from d_scal[b][1], d_scal[b][2] and d_tauout[k][b]: the
 *             bits of elements 3, 4, 5 of sosgpu_aggregate's scalar block for that slot (whose d_scal[b][3] is d_tauout[k][b];
 *             column 3 of the d_scal given here is not read)
 *     [9]     sum aik        [10] -(min norders): > 0 when a bin of the segment failed; combines with MAX across segments or
 *             ranks (elements 6 and 8 of that block)
 *     [11]    sum aik exp(-d_tauvrai[k][b]): the bits of element 9 after sosgpu_level_transmission; 0 when d_tauvrai is NULL
 *   with sosgpu_level_absorption's shape (256 threads stride over the bins, serial within a thread, fixed tree).  A bin with
 *   d_norders[b] < 0 adds nothing and is reported through [10].  A bin with jout outside 0 .. NT or NT outside 1 .. lp-1 adds
 *   nothing to [0..5], as in sosgpu_level_absorption (the solvers give such a bin norders = -1); the band scalars take it as
 *   sosgpu_aggregate does.
 *  d_flux[nb][2]     EMOINS, EPLUS of the solve;  d_scal[nb][4]   per-bin scalars as sosgpu_aggregate takes them
 *  d_tauvrai[nz][nb] NULL, or sosgpu_output_depths on the d_hvrai of the profile stage
 * Every other argument as sosgpu_level_absorption takes it.  Asynchronous: one launch on `stream` (queue it behind the solve),
 * no allocation, no work area; `stream` is noted for sosgpu_destroy on cx.  nb = 0 or nseg = 0 queues nothing.  Checked before
 * anything is queued, SOSGPU_E_ARG for: what sosgpu_level_absorption refuses, a NULL d_flux or d_scal. */
#define SOSGPU_IRRADIANCE_COLS 14
int  sosgpu_level_irradiance(sosgpu_ctx *cx, const void *d_table /*NULL: cx alone*/, const int32_t *d_ctx_of_bin /*NULL with d_table NULL*/,
                             int nb, int lp, const int32_t *d_nt, const double *d_prof, const double *d_zprof /*[nb][lp]*/, int nz,
                             const int32_t *d_jout, const double *d_zz, const double *d_tauout /*[nz][nb] each*/,
                             const double *d_rec /*[nz][nb][iborm_max+1][3][W]*/, const int32_t *d_norders,
                             const double *d_flux /*[nb][2]*/, const double *d_scal /*[nb][4]*/,
                             const double *d_tauvrai /*[nz][nb], may be NULL*/, int nseg, const int32_t *d_seg,
                             const double *d_aik, double *d_out /*[nz][nseg][SOSGPU_IRRADIANCE_COLS]*/, void *stream);

/* Sensor channels of a spectrum: response-weighted sums of recomposition blocks over the wavelengths, on the device.
 * A call adds the terms of nchan channels onto an accumulator that lives for the whole spectrum:
 *   d_acc[c][k][iphi][q][t] += sum_m wgt[m] * block(job[m], k)[iphi][q][t],   q = 0, 1, 2 (XIT, XQT, XUT),
 * over the terms m = first[c] .. first[c+1]-1 of channel c in term order, every step formed as a = a + w * x (one multiply,
 * one add, no FMA): a host loop in term order reproduces the sum bit for bit, and successive calls on one accumulator give
 * the bits of one call with the concatenated term lists.  Rows 3..6 of a block are never read.  A channel without a term
 * in the call leaves its part of d_acc untouched.
 *  d_blocks        DEVICE, [njobs][nslots][nphi][7][W]: the blocks of the call back to back, job j, slot k at
 *                  d_blocks + (j * nslots + k) * nphi * 7 * W -- what sosgpu_trphi_spectrum writes for the jobs of a part of
 *                  a spectrum with nslots output altitudes each, all of one azimuth list and direction count
 *  first[nchan+1]  HOST, non-decreasing from first[0] = 0; first[nchan] = the number of terms of the call
 *  job[], wgt[]    HOST, first[nchan] entries each: block index 0..njobs-1 and finite weight of every term
 *  d_acc           DEVICE, [nchan][nslots][nphi][3][W]; the caller zeroes it before the first call of a spectrum
 *  d_work, work_bytes   see "Work areas": the term table, sosgpu_channel_accumulate_work_bytes(nchan, first[nchan]) bytes
 * Asynchronous: one launch, nothing is waited for, no device memory is allocated and no context is needed.
 * Checked before anything is queued, SOSGPU_E_ARG for: njobs, nslots, nphi, w or nchan < 1 (or nslots, nchan > 65535,
 * nphi * 7 * w > 2^31 - 1), a NULL pointer, first[0] != 0 or a decreasing first, a job outside 0..njobs-1, a weight that is
 * not finite, the work area's rules.  A call without a term returns SOSGPU_OK with nothing queued. */
size_t sosgpu_channel_accumulate_work_bytes(int nchan, int nterms);
int  sosgpu_channel_accumulate(int device, const double *d_blocks, int njobs, int nslots, int nphi, int w, int nchan,
                               const int32_t *first, const int32_t *job, const double *wgt, double *d_acc, void *d_work,
                               size_t work_bytes, void *stream);
/* The channel radiances from the sums: d_out[nchan][nslots][nphi][7][W] in the row order of sosgpu_trphi.  Rows 0..2: d_acc
 * behind the reference's output thresholds (XIT <= 1e-99 -> 0; |XQT|, |XUT| < 1e-15 -> 0, SOS_TRPHI.F:1212-1218); row 3
 * (ANGDIFF): copied from d_angdiff_block[nphi][7][W], any block of the spectrum (the scattering angle depends on the
 * directions and the azimuth only); rows 4..6: SOS_POLAR of rows 0..2, the statements sosgpu_trphi executes; direction 0
 * (t = N, W = 2N + 1) is zero in every row.  Asynchronous: one launch on `stream`, no device memory allocated, no context
 * needed.  SOSGPU_E_ARG, before anything is queued, for a NULL pointer, nchan, nslots, nphi < 1, an even w or w < 3, and the
 * size limits of sosgpu_channel_accumulate. */
int  sosgpu_channel_finish(int device, const double *d_acc, const double *d_angdiff_block, int nchan, int nslots, int nphi,
                           int w, double *d_out, void *stream);

/* Replaces SOS_ROUJEAN (src/SOS_ROUJEAN.F:212), SOS_SURFACE_BPDF (src/SOS_SURFACE_BPDF.F:219) and SOS_BPDF_AJOUT_BRDF
 * (src/SOS_SURFACE.F:2503) for -SURF.Type 3..7, no temporary files: Fourier reflection matrices of the land surface,
 *  d_rsurf[os_nb+1][9][N][N]  REAL*4, reference surface-file record order (feed to sosgpu_set_surface_matrices).
 * Host inputs mu[n], chr[n]; ind = surface refractive index (BPDF types).  *ier_out (host) = 0, or -1 when the Roujean BRDF
 * goes negative for some geometry (the reference's IER = -1, SOS_ROUJEAN.F:548).  Synchronous.  The bounds on OS_NB, OS_NS,
 * OS_NM are those of sosgpu_glitter. */
int  sosgpu_land_surface(int device, const sosgpu_land *land, int n, const double *mu, const double *chr, double ind,
                         int os_nb, int os_ns, int os_nm, float *d_rsurf, int32_t *ier_out, void *stream);

/* sosgpu_glitter / sosgpu_land_surface for many jobs on one angle set -- the wavelengths of a part of a spectrum, whose water
 * index or Roujean coefficients change with the wavelength -- in ONE asynchronous call.  Block j holds, bit for bit, the
 * d_rsurf sosgpu_glitter (isurf 1) or sosgpu_land_surface (isurf 3, 4, 5, 7) writes for job j's parameters.
 * What the jobs have in common is computed once; the distinct parameter sets are found by exact equality of the doubles:
 *   one Cox-Munk azimuth analysis per distinct wind, one Maignan analysis per distinct coef_c, one constant analysis each for
 *   Rondeaux-Herman and Breon; one SOS_MAT_REFLEXION result per distinct (analysis, ind), COEF = 1/sigma^2 for the sea and 1
 *   for land; one sosgpu_mat_fresnel_host per distinct ind (on the host, inside the call); one Roujean analysis per distinct
 *   (k0, k1, k2); one kernel that writes every job's block and status.
 *  mu[n], chr[n]   HOST, as sosgpu_glitter
 *  jobs[njobs]     HOST array; jobs may repeat one another (their blocks are then equal) but not share a d_rsurf
 *  d_status[njobs] DEVICE, written on `stream` for every job: 0, or -1 when the Roujean function goes negative for the job's
 *                  coefficients (the reference's IER = -1, SOS_ROUJEAN.F:548).  A flagged job disturbs no other job; the
 *                  content of its block is unspecified.
 *  d_work, work_bytes   see "Work areas": the tables and the Fresnel coefficients; the intermediates (E, IL of every analysis,
 *                  the reflexion blocks) live behind them
 * Asynchronous: one copy and at most six launches whatever njobs is, nothing is waited for, no device memory is allocated.
 * Checked on the host before anything is queued: SOSGPU_E_ARG for n outside 1..85, the order bounds and the LDS limit of
 * sosgpu_glitter, NULL mu, chr, jobs, d_status, d_work or a NULL d_rsurf, njobs < 0 or njobs > 65535, an isurf outside
 * {1, 3, 4, 5, 6, 7}, the work area's rules; SOSGPU_E_UNSUPPORTED for isurf = 6, as sosgpu_land_surface.
 * njobs = 0 returns SOSGPU_OK with nothing queued.  sosgpu_surface_batch_work_bytes does not look at d_rsurf, so that the area
 * can be sized before the blocks exist. */
typedef struct sosgpu_surface_job {
    int32_t isurf;          /* 1 Cox-Munk sea; 3, 4, 5, 7 land (6: SOSGPU_E_UNSUPPORTED, as sosgpu_land_surface) */
    int32_t reserved;
    double  wind, ind;      /* sea: wind speed, water index; land 4, 5, 7: ind of the BPDF; land 3: ind ignored */
    double  k0, k1, k2, coef_c;
    float  *d_rsurf;        /* DEVICE output block [os_nb+1][9][N][N], reference surface-file record order */
} sosgpu_surface_job;
size_t sosgpu_surface_batch_work_bytes(int n, int os_nb, int os_ns, int os_nm, const sosgpu_surface_job *jobs, int njobs);
int    sosgpu_surface_batch(int device, int n, const double *mu, const double *chr, int os_nb, int os_ns, int os_nm,
                            const sosgpu_surface_job *jobs, int njobs, int32_t *d_status /*[njobs]*/,
                            void *d_work, size_t work_bytes, void *stream);

/* Scratch requirements (bytes) of the context on its device, for memory planning. */
size_t sosgpu_ctx_bytes(const sosgpu_ctx *cx);

/* Floating-point work of the last solve, computed on the host from d_nt/d_norders/d_iglast after a synchronise
 * (used by bench.py for the roofline).  flops_out[0] = SURVEY 8d count of the reference algorithm: every computed
 * scattering order >= 2 costs 2*(6N)^2*(NT+1) [+ 2*3*6N*(NT+1)*3 for the molecular operator, s <= 2] + 12*6N*NT.
 * flops_out[1] = the same steps in the form this library executes: two 3N x 3N half systems
 * 2*2*(3N)^2*(NT+1), the molecular operator in rank-4 form 2*2*4*3N*(NT+1) for s <= 2, and 10 flops per row and
 * layer of formal solution (6N*NT*10); padding to MFMA tiles is not counted. */
int  sosgpu_os_flops(sosgpu_ctx *cx, int nb, const int32_t *d_nt, const int32_t *d_norders,
                     const int32_t *d_iglast, double *flops_out);

/* Time (ms) of the last sosgpu_os_solve kernel, measured with HIP events on its own stream.
 * Synchronises that stream. */
int  sosgpu_last_solve_ms(sosgpu_ctx *cx, float *ms);

/* Per-bin atmospheric profiles on the device: SOS_PROFILE for IPROFIL = 1 (src/SOS_PROFIL.F:224-1170) with SOS_DISC
 * (:1210-1332), the PROFIL-file round trip (formats F10.5 / E15.8, SOS_PROFIL.F:1084,1150 -> SOS.F:515,692), the truncation
 * rescale and IBORM of SOS (src/SOS.F:521-550), TAUOUT / TTOT (SOS.F:567-589) and the output level of SOS_OS.F:1514-1520,
 * for nb CKD bins at once.  Replaces the per-bin calls `CALL SOS_PROFILE` (SOS_PROC.F:3518) + the read in `SOS`.
 *   tr, hr, ta, ha      Rayleigh / aerosol optical thickness and scale heights of the wavelength
 *   d_tabs[nb][nblev]   cumulative gas absorption optical depth of every bin on the altitude grid d_altabs[nblev]
 *                       (descending, ground last; CTE_ABS_NBLEV = 50 in the reference); NULL = no gas (ABSPROFIL = 7)
 *   a_tronc, piz, piztr truncation coefficient and single-scattering albedos of SOS.F:523-541;  zout: -1 = TOA/ground
 * Outputs (device): d_prof[nb][3][lp] (H, XDEL, YDEL as sosgpu_os_solve takes them), d_nt[nb] (-1: the profile needs
 * more than CTE_OS_NT = 600 levels or lp is too small -- the reference's IER = -1), d_iborm[nb], d_zprof[nb][lp],
 * d_jout[nb] / d_zz[nb] (NULL when zout = -1), d_scal[nb][4] = {0, TTOT_TRONC, TTOT_VRAI, TAUOUT} (the layout
 * sosgpu_aggregate takes).  The no-gas profile of the wavelength (SOS_PROFIL.F:349-489) is made by one wavefront queued on
 * `stream` in front of the bins' kernel, or taken from d_nogas (sosgpu_profile_nogas below); nothing is waited for (a second call on the same context from ANOTHER stream first
 * waits for the context's earlier work).  IPROFIL = 2 (aerosol layer between two altitudes) is made by
 * sosgpu_profile_layer / sosgpu_profile_layer_spectrum below.  (The reference's branch reads Hmol(0) before it assigns it;
 * they start its recurrence from Hmol(0) = 0, the value on a fresh stack.) */
int  sosgpu_profile(sosgpu_ctx *cx, int nb, double tr, double hr, double ta, double ha, int absprofil,
                    int nblev, const double *d_altabs, const double *d_tabs,
                    double a_tronc, double piz, double piztr, double zout, int lp,
                    double *d_prof, int32_t *d_nt, int32_t *d_iborm, double *d_zprof,
                    int32_t *d_jout, double *d_zz, double *d_scal, const double *d_nogas, void *stream);
/* sosgpu_profile with one more output: d_hvrai[nb][lp] (device, NULL = sosgpu_profile), the cumulative optical depth H of
 * every level as the PROFIL file gives it, BEFORE the truncation rescale of SOS.F:521-543 -- the untruncated depth, of which
 * d_scal keeps the last entry only (d_hvrai[b][nt] = TTOT_VRAI); zeros above nt, and the row of a flagged bin (nt = -1) is
 * left as passed.  Every other output has the bits of sosgpu_profile. */
int  sosgpu_profile_true(sosgpu_ctx *cx, int nb, double tr, double hr, double ta, double ha, int absprofil,
                         int nblev, const double *d_altabs, const double *d_tabs,
                         double a_tronc, double piz, double piztr, double zout, int lp,
                         double *d_prof, int32_t *d_nt, int32_t *d_iborm, double *d_zprof,
                         int32_t *d_jout, double *d_zz, double *d_scal, const double *d_nogas, double *d_hvrai, void *stream);

/* Head start for sosgpu_profile (optional).  The level placement of a wavelength's no-gas profile is a serial chain of about a
 * millisecond on one wavefront and needs (tr, hr, ta, ha) only: a driver can queue it here as soon as it knows them -- before it
 * has the gas tables, the surface or even the context of the wavelength -- and hand the block to sosgpu_profile as d_nogas
 * (NULL there: sosgpu_profile queues the same kernel itself, in front of the bins' kernel).
 *   d_nogas[4][SOSGPU_NOGAS_LEVELS] (DEVICE, caller-owned): altitude, optical depth, aerosol and molecular share of each level;
 *   must be complete, or queued on the same stream, when sosgpu_profile runs, and stay allocated until that work has run.
 * Asynchronous on `stream`.  SOSGPU_E_UNSUPPORTED: more than CTE_OS_NT levels (the reference's IER = -1). */
#define SOSGPU_NOGAS_LEVELS 608
int  sosgpu_profile_nogas(int device, double tr, double hr, double ta, double ha, double *d_nogas, void *stream);

/* Replaces the per-bin calls `CALL SOS_ABSPROFILE` of the CKD loop (SOS_PROC.F:3494; src/SOS_ABSPROFILE.F:184, core :325-371)
 * for nb bins at once.  The coefficient of a gas depends on the gas, the exponential term and the layer only, so it is
 * tabulated once per wavelength (COEFF_ABS_CKD, src/SOS_SUB_TRS.F:171: on the device by sosgpu_ckd_layer_tables below, or on
 * the host as absorption.layer_tables does) and a bin is one term index per gas:
 *   d_ik[nb][8]              1-based term index IK1..IK8 of each bin (gas order H2O, CO2, O3, N2O, CO, CH4, O2, NO2)
 *   d_xk[8][nterm][nlev-1]   k_i of (gas, term, layer), layer 0 = top layer;  d_ro[8][nlev-1] molecules/cm2 of the layer
 *   d_tabs[nb][nlev]         TAUABS: cumulative absorption optical depth per level, level 0 = TOA (feeds sosgpu_profile)
 * nlev = CTE_ABS_NBLEV = 50 in the reference. */
int  sosgpu_absprofile(int device, int nb, int nlev, int nterm, const int32_t *d_ik, const double *d_xk, const double *d_ro,
                       double *d_tabs, void *stream);

/* The profile stage of MANY wavelengths (a part of a spectrum) as three launches: the no-gas profiles (one wavefront per
 * wavelength), SOS_ABSPROFILE and SOS_PROFILE (one wavefront per bin of every wavelength, each reading the index of its
 * wavelength and that wavelength's parameters from a device table) -- as the solver takes its contexts from a table
 * (sosgpu_os_solve_multi).  Per bin the kernels run the device code of sosgpu_profile_nogas / sosgpu_absprofile /
 * sosgpu_profile: the outputs are theirs, bit for bit.  No context is needed.
 *   wl[nwl] (HOST)       one entry per wavelength, in bin order: its nbins bins are consecutive, sum of nbins = nb
 *       tr, hr, ta, ha, a_tronc, piz, piztr, zout, absprofil   as sosgpu_profile
 *       smax             highest Fourier order of the wavelength's context (iborm_max of sosgpu_create): caps IBORM
 *       nterm            exponential terms of its gas tables; 0 = no gas (ABSPROFIL = 7): then nbins must be 1
 *       xk_off, ro_off, alt_off   where its xk[8][nterm][nblev-1], ro[8][nblev-1] and altitude grid altabs[nblev] start
 *                        in d_gas, counted in doubles (ignored with nterm = 0)
 *   d_wl_of_bin[nb]      index into wl of every bin (int32);  d_ik[nb][8] as sosgpu_absprofile (rows of no-gas bins unused)
 *   d_gas[gas_doubles]   the wavelengths' tables, packed; nblev (2..64) is common to the launch; both unused when no
 *                        wavelength has gas (NULL, 0, nblev 0, d_ik and d_tabs NULL)
 *   d_work, work_bytes   see "Work areas": the no-gas blocks [nwl][4][SOSGPU_NOGAS_LEVELS] (doubles) of the wavelengths first,
 *                        the per-wavelength table behind them; sosgpu_profile_spectrum_work_bytes(nwl) bytes
 * Outputs (device) for the concatenated bins: d_tabs[nb][nblev] (TAUABS, as sosgpu_absprofile; rows of no-gas bins are not
 * written), d_prof[nb][3][lp], d_nt[nb], d_iborm[nb], d_zprof[nb][lp], d_scal[nb][4] as sosgpu_profile; d_jout[nb] /
 * d_zz[nb] are written for the bins of wavelengths with zout != -1 only (both may be NULL when no wavelength has one).
 * A bin whose profile does not fit comes back with nt = -1.  A wavelength that cannot be profiled at all is reported with
 * its index in *bad_wl (NULL allowed; -1 = none) and nothing is queued: SOSGPU_E_UNSUPPORTED when its no-gas grid needs
 * more than CTE_OS_NT levels (sosgpu_profile_nogas_levels(tr, ta) < 0 tells beforehand), SOSGPU_E_ARG for the argument rules
 * of sosgpu_profile / sosgpu_absprofile.  Asynchronous on `stream`; nothing is waited for, and the work areas and inputs
 * must stay allocated until the three kernels have run. */
typedef struct sosgpu_profile_wl {
    double tr, hr, ta, ha;
    double a_tronc, piz, piztr, zout;
    int64_t xk_off, ro_off, alt_off;
    int32_t nterm, nbins, absprofil, smax;
} sosgpu_profile_wl;
/* level count NT of the no-gas grid of (tr, ta) (SOS_PROFIL.F:349-366), or -1: more than CTE_OS_NT levels / no scatterer */
int  sosgpu_profile_nogas_levels(double tr, double ta);
size_t sosgpu_profile_spectrum_work_bytes(int nwl);
int  sosgpu_profile_spectrum(int device, int nwl, const sosgpu_profile_wl *wl, int nb, const int32_t *d_wl_of_bin,
                             const int32_t *d_ik, const double *d_gas, size_t gas_doubles, int nblev, int lp,
                             void *d_work, size_t work_bytes, double *d_tabs, double *d_prof, int32_t *d_nt, int32_t *d_iborm,
                             double *d_zprof, int32_t *d_jout, double *d_zz, double *d_scal, int *bad_wl, void *stream);
/* ... with d_hvrai[nb][lp] for the concatenated bins, as sosgpu_profile_true (NULL = sosgpu_profile_spectrum) */
int  sosgpu_profile_spectrum_true(int device, int nwl, const sosgpu_profile_wl *wl, int nb, const int32_t *d_wl_of_bin,
                                  const int32_t *d_ik, const double *d_gas, size_t gas_doubles, int nblev, int lp,
                                  void *d_work, size_t work_bytes, double *d_tabs, double *d_prof, int32_t *d_nt,
                                  int32_t *d_iborm, double *d_zprof, int32_t *d_jout, double *d_zz, double *d_scal,
                                  int *bad_wl, double *d_hvrai, void *stream);

/* SOS_PROFILE for IPROFIL = 2 (src/SOS_PROFIL.F:800-946): a homogeneous layer of aerosols and molecules between zmin and zmax
 * (km) inside a molecular atmosphere, without gas absorption (the reference refuses the combination).  The recurrence
 * Hmol(I) = Hmol(I-1) + VR_SC of the reference reads Hmol(0) before it is assigned; it starts from Hmol(0) = 0 here, the value
 * on a fresh stack, and Hmol(0) = TR exp(-120 / HR) is assigned afterwards, as there.
 *
 * sosgpu_profile_layer_grid: the level counts, host arithmetic (no device): counts = {NT, sublayers above the layer, inside
 * it, below it (0 for zmin = 0)}.  Returns NT (<= CTE_OS_NT), SOSGPU_E_ARG unless 0 <= zmin < zmax (and tr, hr > 0, ta >= 0),
 * SOSGPU_E_UNSUPPORTED when the layer gets no sublayer or less than 1e-5 of aerosol per sublayer (the reference's ERROR 1020).
 *
 * sosgpu_profile_layer: one bin, by one wavefront; tr, hr, ta, a_tronc, piz, piztr, zout, lp and the outputs as
 * sosgpu_profile_true with nb = 1 (d_hvrai NULL allowed; d_jout / d_zz are written when zout != -1 only and may be NULL
 * otherwise).  What follows the level placement -- round trip, rescale, IBORM, output level, d_scal -- is the device code of
 * sosgpu_profile.  The refusals of the grid are returned before anything is queued; a profile that does not fit lp
 * (lp <= NT) comes back with nt = -1.  Asynchronous on `stream`; nothing is waited for.
 *
 * sosgpu_profile_layer_spectrum: nwl such bins, one per entry of wl (HOST), in ONE launch of the same device code: bin w has
 * the bits sosgpu_profile_layer gives for wl[w] on a context with iborm_max = smax.  No context is needed.
 *   d_work, work_bytes   see "Work areas": the per-wavelength table, sosgpu_profile_layer_spectrum_work_bytes(nwl) bytes
 *   outputs              for the nwl bins, as sosgpu_profile_spectrum_true; d_jout / d_zz are written for wavelengths with
 *                        zout != -1 only (both may be NULL when no wavelength has one)
 * A wavelength the grid refuses, or with smax < 0, is reported in *bad_wl (NULL allowed; -1 = none) with the grid's code and
 * nothing is queued.  Asynchronous on `stream`; the work area stays allocated until the kernel has run. */
typedef struct sosgpu_layer_wl {
    double tr, hr, ta, zmin, zmax;
    double a_tronc, piz, piztr, zout;
    int32_t smax, reserved;
} sosgpu_layer_wl;
int  sosgpu_profile_layer_grid(double tr, double hr, double ta, double zmin, double zmax, int32_t counts[4]);
int  sosgpu_profile_layer(sosgpu_ctx *cx, double tr, double hr, double ta, double zmin, double zmax, double a_tronc,
                          double piz, double piztr, double zout, int lp, double *d_prof, int32_t *d_nt, int32_t *d_iborm,
                          double *d_zprof, int32_t *d_jout, double *d_zz, double *d_scal, double *d_hvrai, void *stream);
size_t sosgpu_profile_layer_spectrum_work_bytes(int nwl);
int  sosgpu_profile_layer_spectrum(int device, int nwl, const sosgpu_layer_wl *wl, int lp, void *d_work, size_t work_bytes,
                                   double *d_prof, int32_t *d_nt, int32_t *d_iborm, double *d_zprof, int32_t *d_jout,
                                   double *d_zz, double *d_scal, double *d_hvrai, int *bad_wl, void *stream);

/* Replaces the calls `CALL COEFF_ABS_CKD` of SOS_ABSPROFILE's gas and layer loops (src/SOS_ABSPROFILE.F:325-353; the routine:
 * src/SOS_SUB_TRS.F:171-393) for MANY wavelengths in one launch: k_i of every (gas, exponential term) table of every
 * wavelength interpolated to the layers -- along the H2O concentration (gas 0 only), the pressure, then by SOS_SPLINE /
 * SOS_SPLINT along the temperature, with the linear fallback for a negative spline value -- statement for statement, so the
 * doubles are the host routine's.  One wavefront per slot = (wavelength, gas, term); the coefficient tables stay on the device.
 *   wl[nwl] (HOST)       one entry per wavelength:
 *       nterm            terms per gas of its output block (1 .. 65535); the wavelength has 8 * nterm slots, slot = gas * nterm + term
 *       nt, np, nc       lengths of its temperature, pressure and H2O-concentration axes: 2..16, 2..64, 2..16
 *       pres_off, temp_off, conc_off   where tab_pres[np], tab_temp[nt], tab_conc[nc] (ascending) start in d_axes, in doubles
 *       prs_off, tmp_off, cl_off       where the layer means prs[nlay] (hPa), tmp[nlay] (K), conc[nlay] (H2O, ppmv * 1e-6) start
 *                        in d_axes: the UNCLAMPED means of SOS_ABSPROFILE.F:330-337, layer 0 = top layer
 *       xk_off           where its xk[8][nterm][nlay] starts in d_out, in doubles
 *   ki[nslots] (HOST)    one DEVICE pointer per slot, wavelength after wavelength (nslots = sum of 8 * nterm): the table
 *                        [np][nt] of the (gas, term), for gas 0 [nc][np][nt]; NULL = no absorption (a term >= NEXP of the gas,
 *                        a table that is all zero): the slot's layers are written +0.0
 *   d_axes[axes_doubles] the axes and layer states, packed;  nlay 1..63 is common to the launch (49 in the reference)
 *   d_work, work_bytes   see "Work areas": the per-wavelength table and the slot pointers,
 *                        sosgpu_ckd_layer_tables_work_bytes(nwl, nslots) bytes
 *   d_out[out_doubles]   every xk block is written in full (nothing needs clearing); it may be the d_gas buffer of
 *                        sosgpu_profile_spectrum, the xk_off being that call's, when this call is queued first on the same stream
 *   d_status[nwl]        int32, cleared by this call on `stream`, then 0 = ok, 1 = SOS_SPLINT met two equal temperature nodes
 *                        ('ERROR for SPLINT interpolation'), 2 = COEFF_ABS_CKD ERROR_923 (k_i < 0 after the linear fallback);
 *                        the failing entries of xk are +0.0
 * Returns SOSGPU_E_ARG for the argument rules (NULL pointers, nterm < 1, nslots, an offset outside d_axes / d_out) and
 * SOSGPU_E_UNSUPPORTED for an axis length or nlay outside the limits above, with the wavelength's index in *bad_wl (NULL
 * allowed; -1 = none); nothing is queued then.  No context; asynchronous on `stream`, nothing is waited for; the inputs, the
 * tables and the work area must stay allocated until the kernel has run. */
typedef struct sosgpu_ckd_wl {
    int64_t pres_off, temp_off, conc_off;
    int64_t prs_off, tmp_off, cl_off;
    int64_t xk_off;
    int32_t nterm, nt, np, nc;
} sosgpu_ckd_wl;
size_t sosgpu_ckd_layer_tables_work_bytes(int nwl, int nslots);
int  sosgpu_ckd_layer_tables(int device, int nwl, const sosgpu_ckd_wl *wl, int nslots, const double *const *ki,
                             const double *d_axes, size_t axes_doubles, int nlay, void *d_work, size_t work_bytes,
                             double *d_out, size_t out_doubles, int32_t *d_status, int *bad_wl, void *stream);

/* Replaces SOS_MIE + SOS_FPHASE_MIE (src/SOS_MIE.F:205, :801) for a whole grid of size parameters, no MIE cache file:
 *   xmu[2 nbmu + 1]  cosines RMU(-nbmu:nbmu) of the Mie angle set (host); rn, in: refractive index (in <= 0)
 *   alphas[nalpha]   size parameters, ascending (host; the reference's grid: steps 1e-4 ... 1 growing with alpha,
 *                    SOS_MIE.F:437-443)
 *   d_rec[nalpha][4 + 3 (2 nbmu + 1)]  REAL*4 records {alpha, Qext, Qsca, 0, Imie(-nbmu:nbmu), Qmie(..), Umie(..)}
 *   d_g[nalpha]      asymmetry factor (double, as the file keeps it)
 * The Mie coefficient arrays (2 alpha + 24 terms) live in LDS up to alpha = 850 and in a temporary HBM scratch beyond;
 * SOSGPU_E_UNSUPPORTED past the reference's own dimension (CTE_MIE_DIM = 10000 terms, SOS.h:96).  Synchronous. */
int  sosgpu_mie(int device, int nbmu, const double *xmu, double rn, double in, int nalpha, const double *alphas,
                float *d_rec, double *d_g, void *stream);

/* sosgpu_mie for `count` (refractive index, size-parameter list, records) jobs at once, ASYNCHRONOUS on `stream`: the
 * table-driven aerosol models (WMO, Shettle & Fenn) change the index of every component with the wavelength, so a spectrum
 * needs three or four fresh record sets per wavelength; this queues those of a chunk without a host wait, ahead of the
 * sosgpu_granu_batch call that reads them on the same stream.  All jobs share the angle set xmu[2 nbmu + 1] (HOST).
 *   jobs[count] (HOST; the structures and the lists are read before the call returns)
 *       rn, in           refractive index (in <= 0), as sosgpu_mie
 *       alphas[nalpha]   HOST, positive and ascending; jobs that pass the same pointer and length share one uploaded copy
 *       d_rec, d_g       DEVICE outputs of the job, [nalpha][4 + 3 (2 nbmu + 1)] REAL*4 and [nalpha] doubles as sosgpu_mie writes
 *                        them: the same bits (both entry points run the same device code per size parameter)
 *   d_work, work_bytes   see "Work areas": the angle set, the lists and the job table; behind them the coefficient scratch of
 *                        the sizes past alpha = 850, one for the whole batch: min(such items, 2048) slots of 11 (2 A + 24)
 *                        doubles, A the largest alpha of the batch
 *   d_status[count]      int32, cleared by this call on `stream`, then 0 = ok, bit 0 = a size parameter of the job did not fit
 *                        the coefficient arrays (what sosgpu_mie reports as SOSGPU_E_UNSUPPORTED after its own wait)
 * The work unit is one (job, size parameter), not one job: the items of all jobs are split by the size of their coefficient
 * arrays over at most 5 launches (4 LDS classes, 1 scratch form; csrc/mie.hip), whatever `count` is.
 * Every job is checked on the host first, with sosgpu_mie's rules: SOSGPU_E_ARG for a malformed job (NULL pointer, nalpha < 1,
 * a list that is not positive and ascending), SOSGPU_E_UNSUPPORTED for 2 alpha + 24 > 10000 (CTE_MIE_DIM) or a work_bytes
 * below the size above.  One bad job refuses the whole call: nothing is queued, no output and no status is touched.
 * count = 0: SOSGPU_OK, nothing queued.  No allocation and no wait inside. */
typedef struct sosgpu_mie_job {
    double rn, in;
    const double *alphas;               /* HOST */
    int32_t nalpha, reserved;
    float  *d_rec;                      /* DEVICE */
    double *d_g;                        /* DEVICE */
} sosgpu_mie_job;
/* bytes of d_work for these jobs; 0 when a job is malformed or unsupported (sosgpu_mie_batch tells which) */
size_t sosgpu_mie_batch_work_bytes(int nbmu, int count, const sosgpu_mie_job *jobs);
int  sosgpu_mie_batch(int device, int nbmu, const double *xmu, int count, const sosgpu_mie_job *jobs, void *d_work,
                      size_t work_bytes, int32_t *d_status, void *stream);

/* Replaces SOS_GRANU (src/SOS_AEROSOLS.F:4392-4820): the integral of Mie records over a size distribution, on the device -- the
 * records (2 MB per refractive index at 40 Mie angles) never travel to the host.  The reference reads its MIE file record by
 * record and accumulates in file order; the kernel adds in record order too (the sums of the Fortran loop term for term).
 *   d_rec[nalpha][4 + 3 (2 nbmu + 1)]  records as sosgpu_mie wrote them (the reference re-uses a MIE file for every
 *          wavelength with the same refractive index, angle set and size-parameter range: keep d_rec the same way)
 *   igranu 1: log-normal distribution, v1 = modal radius (microns), v2 = ln-standard deviation (v3 unused);
 *          2: Junge's law, v1 = r0, v2 = slope, v3 = rmax;   wa = wavelength (microns);  alphaf = upper limit of the grid
 *   out[3 + 3 (2 nbmu + 1)] (HOST): extinction and scattering cross sections per particle KMAT1, KMAT2, the number integral
 *          SOMME_NR, then P11, P12, P33 at the 2 nbmu + 1 angles (normalised as SOS_GRANU leaves them).  Synchronous. */
int  sosgpu_granu(int device, int nbmu, int nalpha, const float *d_rec, int igranu, double v1, double v2, double v3,
                  double wa, double alphaf, double *out, void *stream);

/* The same integral for `count` (records, distribution, wavelength) jobs at once, ASYNCHRONOUS on `stream` (the wavelengths of
 * a spectrum: run_sos.sos_spectrum queues the integrals of a batch of wavelengths ahead of their host preparation and fetches
 * all results with one copy).  One workgroup per job, SOSGPU_GRANU_JOBS_PER_LAUNCH jobs per launch; a job's sums are those of
 * sosgpu_granu bit for bit (the same code per workgroup).
 *   jobs[count] (HOST; read before the call returns)   one sosgpu_granu argument set each, all with the same nbmu
 *   d_out[count][3 + 3 (2 nbmu + 1)] (DEVICE)          the `out` block of sosgpu_granu per job
 *   d_work[count][work_stride] (DEVICE)                work_stride >= 3 max(nalpha) + 1 doubles; free after `stream` passed the call
 * Errors: SOSGPU_E_ARG for a malformed job (nothing is launched), SOSGPU_E_HIP. */
#define SOSGPU_GRANU_JOBS_PER_LAUNCH 32
typedef struct sosgpu_granu_job {
    const float *d_rec;                 /* records of sosgpu_mie (device) */
    int32_t nalpha, igranu;
    double v1, v2, v3, wa, alphaf;
} sosgpu_granu_job;
int  sosgpu_granu_batch(int device, int nbmu, int count, const sosgpu_granu_job *jobs, double *d_out, double *d_work,
                        size_t work_stride, void *stream);

/* Diagnostic hook: hand the context a device buffer [nb][8] of uint64 that builds compiled with
 * -DSOS_PROFILE_PHASES fill with per-phase cycle sums of the solver kernel (0 order-1 fill, 1 formal solution,
 * 2 contraction, 3 write-back, 4 stop tests, 5 ground boundary, 6 Fourier bookkeeping).  NULL disables.
 * The shipped build never writes it. */
int  sosgpu_debug_phase_buffer(sosgpu_ctx *cx, unsigned long long *d_phase);
/* Diagnostic accessor: device pointer and size (doubles) of the streamed solver's scratch of this context, and the offset of the
 * order-parallel form's I3 hand-over block [nb][iborm_max+1][threads] inside it after such a solve (0 otherwise). */
int  sosgpu_debug_scratch(sosgpu_ctx *cx, double **d_scratch, size_t *doubles, size_t *spec_i3_offset);
/* Diagnostic: how many pinned staging blocks the library holds for `device` (*total), and how many of them the next
 * table-form call could take now (*idle: in no call's hands, the event behind its last copy passed). */
int  sosgpu_debug_stage_blocks(int device, int *total, int *idle);
/* Diagnostic: the launch plan sosgpu_os_solve (table = 0) / sosgpu_os_solve_multi (table != 0) and their _levels forms (nz > 0
 * output slots) would follow for `nb` bins of `lp` padded levels in a context of `n` directions and iborm_max = `smax` -- the
 * kernel variant, the launch form, the bins per launch and the layout of the context's scratch.  Needs no context and no
 * device; the environment switches are read exactly as a solve reads them.  `nt_max` is the largest valid NT of the batch,
 * which a solve fetches from the device when (and only when) `needs_nt` comes back set; otherwise it is ignored.
 * Offsets and sizes are in doubles from the start of the scratch; the blocks follow each other in the order
 *   work regions [regions][per_bin] | I3 block [i3_doubles] | queue and flag ints [queue_doubles] | slot state
 *   [regions][slot_stride] (from a multiple of 8 doubles)
 * and `need` is the end of the last one (0: the solve uses no scratch).
 * Errors: SOSGPU_E_ARG, SOSGPU_E_UNSUPPORTED as the solve itself. */
enum { SOSGPU_FORM_LDS = 0,        /* field resident in LDS, one workgroup per bin */
       SOSGPU_FORM_STREAM = 1,     /* field streamed from the scratch, one workgroup per bin, `opl` Fourier orders per launch */
       SOSGPU_FORM_PERSIST = 2,    /* streamed, one persistent launch taking (order, bin) tasks from queues */
       SOSGPU_FORM_SPEC = 3 };     /* streamed, order-parallel: rounds of `spec_k` orders of every bin */
typedef struct sosgpu_solve_plan {
    int32_t nw, rtw, ct, big;      /* kernel variant: waves, row tiles per wave, column tiles, streamed (1) or LDS-resident (0) */
    int32_t split, kht;            /* ... the shared-tile form of the LDS-resident contraction (five or six row tiles on four waves:
                                    * N = 22 ... 32 at up to 32 levels), never with `big`; row tiles of the streamed field layout
                                    * (4, 5, 6, 8 or 16; SOSGPU_STREAM_PERSIST != 0 widens 5 and 6 to 8), 0 when LDS-resident */
    int32_t form, opl, spec_k;     /* SOSGPU_FORM_*; orders per launch (STREAM, PERSIST); orders per round (SPEC), else 0 */
    int32_t needs_nt;              /* the order-parallel form is a candidate: the solve reads the batch's NT back */
    int32_t per_launch, lpb;       /* bins per sub-launch; level capacity of a work region (multiple of 32) */
    int32_t threads, q_tail;       /* workgroup size; SosBins::q_tail of the persistent form (-1: the launcher's default) */
    size_t  lds_bytes;             /* dynamic LDS the variant is launched with */
    size_t  per_bin, regions;      /* doubles per work region, number of work regions */
    size_t  off_i3, i3_doubles, off_queue, queue_doubles, off_slots, slot_stride, need;
} sosgpu_solve_plan;
int  sosgpu_debug_solve_plan(int n, int smax, int nb, int lp, int nz, int table, int nt_max, sosgpu_solve_plan *plan);
/* Diagnostic: k-pairs (8 columns each) the LDS-resident solver contracts at Fourier order 0 in a context of `nwgt` directions
 * with a non-zero quadrature weight: ceil(2 nwgt / 8), the I and Q columns -- U is exactly zero at order 0 -- or, with BRDF/BPDF
 * matrices (imat_surf != 0), all ceil(3 nwgt / 8).  Needs no context and no device.  Returns the count, or SOSGPU_E_ARG (< 0).
 * sosgpu_debug_ctx_order0_kpairs: the count of a context; mode > 0 first sets it to the full ceil(3 nwgt / 8) for the context's
 * later solves (A/B of the two contractions), mode = 0 first sets it back to the rule, mode < 0 only reads. */
int  sosgpu_debug_order0_kpairs(int nwgt, int imat_surf);
int  sosgpu_debug_ctx_order0_kpairs(sosgpu_ctx *cx, int mode);
/* Diagnostic accessor: the per-wavelength tables of a context (built by sosgpu_create, sosgpu_noyaux and
 * sosgpu_set_surface_matrices; csrc/sos_common.h documents every layout) and the numbers that describe them, copied to the
 * HOST.  Read-only: nothing in the context changes.  Like sosgpu_noyaux_fetch it waits for the streams the context's work was
 * queued on, then copies on the calling thread's utility stream.  `info` is required; every array pointer may be NULL (not
 * copied), so a first call with info alone gives the sizes (doubles unless noted):
 *   prt    [smax+1][3][os_nb+1][w]            mp_aer [smax+1][2][rtph*ks2h*128]
 *   mp_vt  [3][ks2h*128]                      mp_uf  [3][rtph*64]
 *   sv     [smax+1][4][kp]                    rowmap [kh] (int32)
 *   mp_gnd [smax+1][rtph*ks2h*128], rdir [smax+1][3][n]: only after sosgpu_set_surface_matrices (SOSGPU_E_ARG otherwise) */
typedef struct sosgpu_tables_info {
    int32_t n, w, kp, kh, ks2h, rtph, nwgt, prow, os_nb, smax, n0, ipolar;
    double  beta2, gamma2, alpha2, f11sun, f12sun, mus, ro;
} sosgpu_tables_info;
int  sosgpu_debug_tables(sosgpu_ctx *cx, sosgpu_tables_info *info, double *prt, double *mp_aer, double *mp_vt, double *mp_uf,
                         double *sv, double *mp_gnd, double *rdir, int32_t *rowmap);
/* Diagnostic: d_out[i] = d_in[i] as sosgpu_profile reads it back from the PROFIL file -- written with E15.8 (fmt 0: H, XDEL,
 * YDEL) or F10.5 (fmt 1: the altitudes) and read again -- by the device code sosgpu_profile applies to its levels, one thread per
 * element (1 <= n <= 2^31, d_in / d_out on the device, may be the same array).  Asynchronous on `stream`. */
int  sosgpu_debug_roundtrip(int device, int fmt, size_t n, const double *d_in, double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
