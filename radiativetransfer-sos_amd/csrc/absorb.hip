// csrc/absorb.hip -- actinic flux and absorbed power of a band at every output altitude (gfx950).
//
// The output slots of the solvers capture the order-0 field of every bin at every output altitude.  flux.hip forms its
// hemispheric fluxes (weight mu ga) from the aggregated record; the other angular moment, the actinic flux (weight ga: 4 pi x
// the mean intensity, in the unit of the flux columns), and the power absorbed per kilometre,
//     q_b(z) = (dtau_b / dz) (1 - omega_b(z)) A_b(z),
// are formed here PER BIN, ahead of the band sum: q is a product of three bin quantities and cannot be formed from the
// aggregated record.  Workgroup (g, k): the bins of segment g at output slot k, with k_level_transmission's skeleton --
// 256 threads stride over the bins (serial within a thread), then the fixed tree of tree256.h over four columns.
// Latency-bound and tiny: 2 N + 8 loads and 2 N multiply-adds per bin and slot.
#include "sos_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "tree256.h"
#include "level_terms.h"      // absorption_terms: the four terms of a bin at one slot, shared with k_level_irradiance

// cx: the context of every bin (table null), or what the entries of `table` share (N, iborm_max: the record layout); bin b then
// takes mu, ga and n0 from entry ctx_of_bin[b].  out[k][g][0..3] = sum aik * {a_dir, a_dn, a_up, q} over the bins of segment g
// with norders >= 0.
__global__ __launch_bounds__(256) void k_level_absorption(const SosDev cx, const SosDev *__restrict__ table,
                                                          const int32_t *__restrict__ ctx_of_bin, const int nb, const int lp,
                                                          const int32_t *__restrict__ nt, const double *__restrict__ prof,
                                                          const double *__restrict__ zprof, const int32_t *__restrict__ jout,
                                                          const double *__restrict__ zz, const double *__restrict__ tauout,
                                                          const double *__restrict__ rec, const int32_t *__restrict__ norders,
                                                          const int32_t *__restrict__ seg, const double *__restrict__ aik,
                                                          double *__restrict__ out)
{
    __shared__ double sm[256][4];
    const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    const int b0 = max(seg[g], 0), b1 = min(seg[g + 1], nb);        // (a segment table past the bins reads nothing)
    const size_t per_bin = (size_t)(cx.smax + 1) * 3 * cx.w;
    const size_t slot = (size_t)k * nb;
    double a[4] = {0., 0., 0., 0.};
    for (int b = b0 + t; b < b1; b += 256) {
        if (norders[b] < 0) continue;               // failed bin: no contribution, as in k_aggregate_scal
        const SosDev &d = table ? table[ctx_of_bin[b]] : cx;
        double term[4];
        if (!absorption_terms(cx.n, d.n0, d.mu, d.ga, rec + (slot + b) * per_bin, lp, nt[b], prof + (size_t)b * 3 * lp,
                              zprof + (size_t)b * lp, jout[slot + b], zz[slot + b], tauout[slot + b], term))
            continue;
        const double w = aik[b];
        for (int i = 0; i < 4; i++) a[i] = a[i] + w * term[i];
    }
    for (int i = 0; i < 4; i++) sm[t][i] = a[i];
    __syncthreads();
    tree256<4, 0u>(sm, t);
    if (t < 4) out[((size_t)k * gridDim.x + g) * 4 + t] = sm[0][t];
}

void launch_level_absorption(const SosDev &cx, const SosDev *d_table, const int32_t *d_ctx_of_bin, int nb, int lp,
                             const int32_t *d_nt, const double *d_prof, const double *d_zprof, int nz, const int32_t *d_jout,
                             const double *d_zz, const double *d_tauout, const double *d_rec, const int32_t *d_norders, int nseg,
                             const int32_t *d_seg, const double *d_aik, double *d_out, hipStream_t st)
{
    k_level_absorption<<<dim3(nseg, nz), 256, 0, st>>>(cx, d_table, d_ctx_of_bin, nb, lp, d_nt, d_prof, d_zprof, d_jout, d_zz,
                                                       d_tauout, d_rec, d_norders, d_seg, d_aik, d_out);
}
