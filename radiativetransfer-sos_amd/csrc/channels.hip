// csrc/channels.hip -- sensor channels: response-weighted sums of the recomposition blocks of a spectrum (gfx950).
//
// A channel is a list of terms (job, weight): the radiance of an instrument band is the sum over its wavelengths of
// weight x monochromatic radiance.  k_channel_accumulate adds the terms of one call (the jobs of a chunk of a spectrum, whose
// blocks [nphi][7][W] lie back to back as sosgpu_trphi_spectrum wrote them) onto an accumulator that lives for the whole
// spectrum; k_channel_finish applies SOS_TRPHI's output thresholds and SOS_POLAR (sos_polar.h) to the sums.  Every step of the
// sum is a = a + w * x, one multiply and one add in term order: a host loop reproduces it bit for bit, however the spectrum
// was cut into calls.  HBM-streaming and tiny: 3 of the 7 rows of every block are read once per channel that names it.
#include "sos_common.h"
#include "kernels.h"

#pragma clang fp contract(off)
#include "sos_polar.h"

// acc[c][k][iphi][q][t] += sum_m wgt[m] * block(job[m], k)[iphi][q][t], q = 0..2 (XIT, XQT, XUT; rows 3..6 are never read),
// m = first[c] .. first[c + 1] - 1.  One thread per element, t fastest: the grid's x runs flat over [iphi][q][t], y = k, z = c.
// The term list is the same for every thread of a workgroup and is read through the constant address space, so first / job /
// wgt arrive by scalar loads and the loop is wave-uniform.  A channel without a term leaves its elements alone.
__global__ void k_channel_accumulate(const double *__restrict__ blocks, int nslots, int nphi, int w, const int32_t *first,
                                     const int32_t *job, const double *wgt, double *__restrict__ acc)
{
    typedef const __attribute__((address_space(4))) int32_t IntK;
    typedef const __attribute__((address_space(4))) double DblK;
    IntK *firstk = (IntK *)(unsigned long long)first;
    IntK *jobk = (IntK *)(unsigned long long)job;
    DblK *wgtk = (DblK *)(unsigned long long)wgt;
    const int k = blockIdx.y, c = blockIdx.z;
    const int m0 = firstk[c], m1 = firstk[c + 1];
    if (m0 >= m1) return;
    const int row = 3 * w;                         // elements of one azimuth in the accumulator
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nphi * row) return;
    const int iphi = e / row, r = e - iphi * row;  // r = q * W + t: the first three rows of a block's azimuth are contiguous
    const size_t blk = (size_t)nphi * 7 * w;
    const double *src = blocks + (size_t)k * blk + (size_t)iphi * 7 * w + r;
    const size_t step = (size_t)nslots * blk;      // from job j to job j + 1
    double *dst = acc + ((size_t)c * nslots + k) * nphi * row + e;
    double a = *dst;
    for (int m = m0; m < m1; m++) a = a + wgtk[m] * src[(size_t)jobk[m] * step];
    *dst = a;
}

// out[c][k][iphi][7][W] from acc[c][k][iphi][3][W]: rows 0..2 the sums behind SOS_TRPHI's thresholds, row 3 (ANGDIFF: a matter
// of the angles and the azimuth alone) from a block of the spectrum, rows 4..6 SOS_POLAR of rows 0..2; direction 0 (t = N)
// is zero in every row, as the recomposition writes it.  One thread per (c, k, iphi, t): x flat over [iphi][t], y = k, z = c.
__global__ void k_channel_finish(const double *__restrict__ acc, const double *__restrict__ angdiff_block, int nslots, int nphi,
                                 int w, double *__restrict__ out)
{
    const int k = blockIdx.y, c = blockIdx.z;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nphi * w) return;
    const int iphi = e / w, t = e - iphi * w;
    const size_t ck = (size_t)c * nslots + k;
    double *o = out + (ck * nphi + iphi) * 7 * w;
    if (t == (w - 1) / 2) { for (int q = 0; q < 7; q++) o[q * w + t] = 0.; return; }
    const double *a = acc + (ck * nphi + iphi) * 3 * w;
    double xit = a[0 * w + t], xqt = a[1 * w + t], xut = a[2 * w + t];
    sos_trphi_thresholds(xit, xqt, xut);
    double xan, tpol, lpol;
    sos_polar(xit, xqt, xut, xan, tpol, lpol);
    o[0 * w + t] = xit; o[1 * w + t] = xqt; o[2 * w + t] = xut; o[3 * w + t] = angdiff_block[((size_t)iphi * 7 + 3) * w + t];
    o[4 * w + t] = xan; o[5 * w + t] = tpol; o[6 * w + t] = lpol;
}

void launch_channel_accumulate(const double *d_blocks, int nslots, int nphi, int w, int nchan, const int32_t *d_first,
                               const int32_t *d_job, const double *d_wgt, double *d_acc, hipStream_t st)
{
    const dim3 grid((unsigned)((nphi * 3 * w + 255) / 256), (unsigned)nslots, (unsigned)nchan);
    k_channel_accumulate<<<grid, 256, 0, st>>>(d_blocks, nslots, nphi, w, d_first, d_job, d_wgt, d_acc);
}

void launch_channel_finish(const double *d_acc, const double *d_angdiff_block, int nchan, int nslots, int nphi, int w,
                           double *d_out, hipStream_t st)
{
    const dim3 grid((unsigned)((nphi * w + 255) / 256), (unsigned)nslots, (unsigned)nchan);
    k_channel_finish<<<grid, 256, 0, st>>>(d_acc, d_angdiff_block, nslots, nphi, w, d_out);
}
