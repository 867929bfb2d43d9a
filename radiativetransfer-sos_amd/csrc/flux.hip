// csrc/flux.hip -- diffuse fluxes E-(z), E+(z) of an aggregated record at its output altitude (gfx950).
//
// The reference forms EMOINS / EPLUS inside SOS_OS from the order-0 intensity at the ground and at the top of the atmosphere
// (src/SOS_OS.F:1447-1456).  The output slots of the solvers capture the same order-0 record at
// every output altitude and sosgpu_aggregate sums it over the bins, so the flux at an altitude is this quadrature of the
// aggregated row rec[0][0][W]: one thread per (job, hemisphere), the sum sequential in the reference's order (j ascending,
// products formed as (mu ga) I).  k_level_flux_table: the same for the jobs of a device table (the wavelengths and altitudes
// of a part of a spectrum) in one launch.  Latency-bound and tiny: 3 N loads and N multiply-adds per thread.
#include "sos_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "level_terms.h"      // flux_body: the quadrature of one hemisphere, shared with k_level_irradiance

// out[0] = E-, out[1] = E+ of one record: threads 0 and 1 of one workgroup
__global__ void k_level_flux(SosDev cx, const double *__restrict__ rec, double *__restrict__ out)
{
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= 2) return;
    out[t] = flux_body(cx.n, cx.n0, cx.mu, cx.ga, rec, t);
}

// Table form (sosgpu_level_flux_spectrum): thread i of the flat grid is hemisphere i & 1 of job i >> 1, 32 jobs per workgroup;
// threads past 2 njobs leave.  The entries are read through the constant address space; the job differs from lane to lane, so
// every lane loads its own entry's fields (the loads of a lane pair coincide).
__global__ void k_level_flux_table(const FluxJobDev *jobs, int njobs)
{
    typedef const __attribute__((address_space(4))) FluxJobDev JobK;
    JobK *tab = (JobK *)(unsigned long long)jobs;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2LL * njobs) return;
    JobK &jb = tab[i >> 1];
    const int up = (int)(i & 1);
    jb.out[up] = flux_body(jb.n, jb.n0, jb.mu, jb.ga, jb.rec, up);
}

void launch_level_flux(const SosDev &cx, const double *d_rec, double *d_out, hipStream_t st)
{
    k_level_flux<<<1, 64, 0, st>>>(cx, d_rec, d_out);
}

void launch_level_flux_table(const FluxJobDev *d_jobs, int njobs, hipStream_t st)
{
    k_level_flux_table<<<(2 * njobs + 63) / 64, 64, 0, st>>>(d_jobs, njobs);
}
