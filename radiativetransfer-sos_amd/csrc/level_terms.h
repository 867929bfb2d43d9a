// csrc/level_terms.h -- the per-bin terms of the irradiance quantities at an output slot, each stated ONCE: the kernels of
// flux.hip (k_level_flux, k_level_flux_table), absorb.hip (k_level_absorption), aggregate.hip (k_aggregate_scal,
// k_level_transmission) and irradiance.hip (k_level_irradiance) call them, so that equal inputs give equal bits whichever
// kernel forms them.  Include it inside the file's `fp contract(off)` region.
#pragma once

// up = 0: down-going hemisphere, E- from I(-j); up = 1: up-going, E+ from I(+j).  row: the order-0 intensity row, direction jj
// at offset jj + N.  tab = -mu[n0 - 1], the reference's TAB (the solar cosine as the solvers use it, SosDev::mus).
__device__ __forceinline__ double flux_body(const int n, const int n0, const double *__restrict__ mu, const double *__restrict__ ga,
                                            const double *__restrict__ row, const int up)
{
    double e = 0.;
    for (int j = 1; j <= n; j++) e = e + mu[j - 1] * ga[j - 1] * row[up ? n + j : n - j];
    const double tab = -mu[n0 - 1];
    return -e * 2 / tab;
}

// The four terms of bin b at one slot: t[0] = a_dir, t[1] = a_dn, t[2] = a_up, t[3] = q; false: the bin adds nothing (a
// standard-output slot, jout = 0, mixes the ground and the top of the atmosphere; a jout outside 0..NT or an NT outside
// 1..lp-1 is a malformed bin).  row: the order-0 intensity row of the bin's record, direction jj at offset jj + N as in
// flux_body, whose statements a_dn / a_up repeat without the factor mu.  The single-scattering albedo is a LEVEL quantity of
// the solver's discretisation (XDEL + YDEL at level j), interpolated between the two levels that bracket z as the field is;
// the slope is that of the layer between them, 0 where the two altitudes coincide.
__device__ __forceinline__ bool absorption_terms(const int n, const int n0, const double *__restrict__ mu,
                                                 const double *__restrict__ ga, const double *__restrict__ row, const int lp,
                                                 const int nt, const double *__restrict__ prof, const double *__restrict__ zprof,
                                                 const int j, const double zz, const double tauout, double t[4])
{
    if (nt < 1 || nt >= lp || j < 1 || j > nt) return false;
    double s_dn = 0., s_up = 0.;
    for (int jj = 1; jj <= n; jj++) s_dn = s_dn + ga[jj - 1] * row[n - jj];
    for (int jj = 1; jj <= n; jj++) s_up = s_up + ga[jj - 1] * row[n + jj];
    const double tab = -mu[n0 - 1];
    const double a_dn = -s_dn * 2 / tab, a_up = -s_up * 2 / tab;
    const double mus = mu[n0 - 1];
    const double a_dir = exp(-tauout / mus) / mus;
    const double *h = prof, *xdel = prof + lp, *ydel = prof + 2 * (size_t)lp;
    const double om = (1 - zz) * (xdel[j - 1] + ydel[j - 1]) + zz * (xdel[j] + ydel[j]);
    const double slope = zprof[j - 1] <= zprof[j] ? 0. : (h[j] - h[j - 1]) / (zprof[j - 1] - zprof[j]);
    t[0] = a_dir; t[1] = a_dn; t[2] = a_up;
    t[3] = slope * (1 - om) * (a_dn + a_up + a_dir);
    return true;
}

// The term of a bin in a band transmission: k_aggregate_scal, k_level_transmission and k_level_irradiance share it, so that
// equal depths give equal bits.
__device__ __forceinline__ double transmission_term(double w, double tau) { return w * exp(-tau); }
