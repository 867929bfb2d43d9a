// csrc/albedo.hip -- the stage around the solver for the spherical albedo of the atmosphere (gfx950).
//
// Per bin, S = 2 sum_j ga_j mu_j A_j, where A_j is the up-going flux EPLUS at the lit boundary of an order-0 solve over a
// black ground with incidence mu_j.  sosgpu_trans_spectrum (trans.hip) queues exactly those solves and keeps the other flux;
// sosgpu_albedo_spectrum (api_solve.hip) shares its child table (k_trans_table, k_trans_sv) and differs in the items:
//   k_albedo_items  k_trans_items, and with from_below the profile rows of every item MIRRORED in the vertical about the
//                   item's own nt -- the atmosphere lit from the ground, which is the S of the coupling formula
//                   rho_toa = rho_path + T_down T_up rho_s / (1 - S rho_s); items of weight-0 directions (the inserted solar
//                   angle, the user angles) are made malformed, so the solver skips them
//   (the solve: os_solve_impl, untouched)
//   k_albedo_sum    plane[b][j] = A_j and salb[b], summed in ascending j
//   k_albedo_band   sum_b aik[b] salb[b] per segment (sosgpu_albedo_band)
#include "sos_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "tree256.h"

// what the two item-side kernels decide alike for bin b: its context, its nt, and whether it is well formed
struct AlbedoBin { int c, nt; bool ok; };
__device__ __forceinline__ AlbedoBin albedo_bin(const TransItems &a, const size_t b)
{
    AlbedoBin r;
    r.c = a.ctx_of_bin ? a.ctx_of_bin[b] : 0;
    r.nt = a.nt[b];
    r.ok = r.c >= 0 && r.c < a.nctx && r.nt >= 1 && r.nt < a.lp;
    return r;
}

// Element e of the items' profile rows, as k_trans_items.  Mirror of a well-formed bin (rows h, xdel, ydel of lp levels,
// levels 0..nt used): h'[k] = h[nt] - h[nt-k], xdel'[k] = xdel[nt-k], ydel'[k] = ydel[nt-k] for k <= nt, zeros past nt as
// the upload pads them.  Every index read lies in 0..nt < lp of the bin's own row.
__global__ void k_albedo_items(const AlbedoItems q)
{
    const TransItems &a = q.t;
    const size_t row = (size_t)3 * a.lp;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)a.nb * a.n * row) return;
    const size_t item = e / row, off = e % row;
    const size_t b = item / a.n;
    const AlbedoBin bin = albedo_bin(a, b);
    const double *src = a.prof + b * row;
    double v = src[off];
    if (q.from_below && bin.ok) {
        const int r = (int)(off / a.lp), k = (int)(off % a.lp);
        const double *s = src + (size_t)r * a.lp;
        if (k > bin.nt) v = 0.;
        else if (r == 0) v = s[bin.nt] - s[bin.nt - k];
        else v = s[bin.nt - k];
    }
    a.prof_item[e] = v;
    if (off == 0) {
        const int j0 = (int)(item % a.n);
        const bool lit = bin.ok && q.parents[bin.c].ga[j0] != 0.;       // (a context's weights go with its solar angle)
        a.ctx_of_item[item] = (bin.ok ? bin.c : 0) * a.n + j0;
        a.nt_item[item] = lit ? bin.nt : -1;
        a.iborm_item[item] = 0;
        a.flux[2 * item] = 0.; a.flux[2 * item + 1] = 0.;
    }
}

// One workgroup per bin: the plane albedos side by side, the Gauss sum by one lane in ascending j.  A weight-0 direction
// adds nothing (its item was skipped: the term would be (0 mu_j) 0), a malformed bin gives zeros throughout.
__global__ void k_albedo_sum(const AlbedoItems q, double *__restrict__ plane, double *__restrict__ salb)
{
    const TransItems &a = q.t;
    const size_t b = blockIdx.x;
    const int n = a.n;
    const AlbedoBin bin = albedo_bin(a, b);
    const double *ga = bin.ok ? q.parents[bin.c].ga : nullptr, *mu = bin.ok ? q.parents[bin.c].mu : nullptr;
    const double *f = a.flux + 2 * b * n;
    if (plane)
        for (int j = threadIdx.x; j < n; j += blockDim.x) plane[b * n + j] = (bin.ok && ga[j] != 0.) ? f[2 * j + 1] : 0.;
    if (threadIdx.x == 0) {
        double s = 0.;
        if (bin.ok)
            for (int j = 0; j < n; j++)
                if (ga[j] != 0.) s = s + ((2. * ga[j]) * mu[j]) * f[2 * j + 1];
        salb[b] = s;
    }
}

// Workgroup g: sum aik(b) salb(b) over the bins of segment g, with k_aggregate_scal's striding and tree.
__global__ __launch_bounds__(256) void k_albedo_band(const int32_t *__restrict__ seg, const double *__restrict__ aik,
                                                     const double *__restrict__ salb, double *__restrict__ out)
{
    __shared__ double sm[256][1];
    const int g = blockIdx.x, t = threadIdx.x;
    const int b0 = seg[g], b1 = seg[g + 1];
    double acc = 0.;
    for (int b = b0 + t; b < b1; b += 256) acc = acc + aik[b] * salb[b];
    sm[t][0] = acc;
    __syncthreads();
    tree256<1, 0u>(sm, t);
    if (t == 0) out[g] = sm[0][0];
}

void launch_albedo_items(const AlbedoItems &q, hipStream_t st)
{
    const size_t ne = (size_t)q.t.nb * q.t.n * 3 * q.t.lp;
    k_albedo_items<<<(unsigned)((ne + 255) / 256), 256, 0, st>>>(q);
}

void launch_albedo_sum(const AlbedoItems &q, double *d_plane, double *d_salb, hipStream_t st)
{
    k_albedo_sum<<<(unsigned)q.t.nb, 64, 0, st>>>(q, d_plane, d_salb);
}

void launch_albedo_band(int nseg, const int32_t *d_seg, const double *d_aik, const double *d_salb, double *d_out, hipStream_t st)
{
    k_albedo_band<<<(unsigned)nseg, 256, 0, st>>>(d_seg, d_aik, d_salb, d_out);
}
