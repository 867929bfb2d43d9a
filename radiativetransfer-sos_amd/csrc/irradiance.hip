// csrc/irradiance.hip -- every irradiance quantity of a solved group at its output slots, in ONE launch (gfx950).
//
// The flux, split and absorption rows of a levels pass are angular moments of the Fourier order-0 field at the altitude, plus
// band scalars.  The chain that serves them next to the radiances -- sosgpu_aggregate once per slot, sosgpu_level_flux_spectrum,
// sosgpu_level_transmission, sosgpu_level_absorption -- sums records of iborm_max + 1 orders only to read one row of the sum.
// Here the moments are formed PER BIN from the order-0 row the solver captured (so the context may hold order 0 alone,
// iborm_max = 0) and summed with aik, next to the band scalars the rows need.  Workgroup (g, k): the bins of segment g at
// output slot k, with k_level_absorption's skeleton -- 256 threads stride over the bins (serial within a thread), then the
// fixed tree of tree256.h over the SOSGPU_IRRADIANCE_COLS columns.  The terms are those of level_terms.h, the statements of
// k_level_flux, k_level_absorption, k_aggregate_scal and k_level_transmission: columns that sum the same terms have the bits
// of those kernels.  Latency-bound and tiny: 4 N + 16 loads and 4 N multiply-adds per bin and slot, 28 KiB of LDS.
#include "sos_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "tree256.h"
#include "level_terms.h"

#define IRC SOSGPU_IRRADIANCE_COLS
static_assert(IRC == 14, "the column list of include/sosgpu.h");

// Columns of out[k][g][.] (include/sosgpu.h): 0..3 sum aik {a_dir, a_dn, a_up, q}; 4, 5 sum aik {E-, E+}; 6..8 sum aik
// exp(-{TTOT_TRONC, TTOT_VRAI, TAUOUT(slot)}); 9 sum aik; 10 -(min norders), combined with MAX; 11 sum aik exp(-tauvrai(slot));
// 12, 13 sum aik {EMOINS, EPLUS} of the solve.  A failed bin (norders < 0) is flagged through column 10 and adds nothing;
// the band scalars 6..9 and 11..13 take every other bin, as k_aggregate_scal and k_level_transmission do; the moments 0..5
// skip a malformed bin (jout outside 0..NT, NT outside 1..lp-1) as k_level_absorption does.  A standard-output bin (jout = 0)
// adds nothing to columns 0..3; its E-, E+ are the moments of its record row like any other slot's, which is what
// sosgpu_level_flux gives for that slot (the solve's own pair, columns 12 and 13, agrees with them to rounding without surface
// matrices and to some 1e-9 with them, as the reference's EPLUS and its own record do).
__global__ __launch_bounds__(256) void k_level_irradiance(const SosDev cx, const SosDev *__restrict__ table,
                                                          const int32_t *__restrict__ ctx_of_bin, const int nb, const int lp,
                                                          const int32_t *__restrict__ nt, const double *__restrict__ prof,
                                                          const double *__restrict__ zprof, const int32_t *__restrict__ jout,
                                                          const double *__restrict__ zz, const double *__restrict__ tauout,
                                                          const double *__restrict__ rec, const int32_t *__restrict__ norders,
                                                          const double *__restrict__ flux, const double *__restrict__ scal,
                                                          const double *__restrict__ tauvrai, const int32_t *__restrict__ seg,
                                                          const double *__restrict__ aik, double *__restrict__ out)
{
    __shared__ double sm[256][IRC];
    const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    const int b0 = max(seg[g], 0), b1 = min(seg[g + 1], nb);        // (a segment table past the bins reads nothing)
    const size_t per_bin = (size_t)(cx.smax + 1) * 3 * cx.w;
    const size_t slot = (size_t)k * nb;
    double a[IRC];
    for (int i = 0; i < IRC; i++) a[i] = 0.;
    a[10] = -2147483647.;
    for (int b = b0 + t; b < b1; b += 256) {
        const double w = aik[b];
        const int no = norders[b];
        a[10] = fmax(a[10], -(double)no);
        if (no < 0) continue;                       // failed bin: flagged through a[10], no contribution
        a[6] = a[6] + transmission_term(w, scal[4 * (size_t)b + 1]);
        a[7] = a[7] + transmission_term(w, scal[4 * (size_t)b + 2]);
        a[8] = a[8] + transmission_term(w, tauout[slot + b]);
        a[9] = a[9] + w;
        if (tauvrai) a[11] = a[11] + transmission_term(w, tauvrai[slot + b]);
        a[12] = a[12] + w * flux[2 * (size_t)b + 0];
        a[13] = a[13] + w * flux[2 * (size_t)b + 1];
        const int j = jout[slot + b], ntb = nt[b];
        if (ntb < 1 || ntb >= lp || j < 0 || j > ntb) continue;
        // (a standard-output bin, j = 0: its record row is the ground going down and the top going up)
        const SosDev &d = table ? table[ctx_of_bin[b]] : cx;
        const double *row = rec + (slot + b) * per_bin;
        a[4] = a[4] + w * flux_body(cx.n, d.n0, d.mu, d.ga, row, 0);
        a[5] = a[5] + w * flux_body(cx.n, d.n0, d.mu, d.ga, row, 1);
        double term[4];
        if (absorption_terms(cx.n, d.n0, d.mu, d.ga, row, lp, ntb, prof + (size_t)b * 3 * lp, zprof + (size_t)b * lp, j,
                             zz[slot + b], tauout[slot + b], term))
            for (int i = 0; i < 4; i++) a[i] = a[i] + w * term[i];
    }
    for (int i = 0; i < IRC; i++) sm[t][i] = a[i];
    __syncthreads();
    tree256<IRC, 1u << 10>(sm, t);
    if (t < IRC) out[((size_t)k * gridDim.x + g) * IRC + t] = sm[0][t];
}

void launch_level_irradiance(const SosDev &cx, const SosDev *d_table, const int32_t *d_ctx_of_bin, int nb, int lp,
                             const int32_t *d_nt, const double *d_prof, const double *d_zprof, int nz, const int32_t *d_jout,
                             const double *d_zz, const double *d_tauout, const double *d_rec, const int32_t *d_norders,
                             const double *d_flux, const double *d_scal, const double *d_tauvrai, int nseg, const int32_t *d_seg,
                             const double *d_aik, double *d_out, hipStream_t st)
{
    k_level_irradiance<<<dim3(nseg, nz), 256, 0, st>>>(cx, d_table, d_ctx_of_bin, nb, lp, d_nt, d_prof, d_zprof, d_jout, d_zz,
                                                       d_tauout, d_rec, d_norders, d_flux, d_scal, d_tauvrai, d_seg, d_aik,
                                                       d_out);
}
