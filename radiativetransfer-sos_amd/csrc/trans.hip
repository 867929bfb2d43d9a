// csrc/trans.hip -- the stage around the solver for the diffuse transmissions of the -SOS.Trans option (gfx950).
//
// The reference (SOS.F:600-635) runs SOS_OS once per direction J with N0 = J, Fourier order 0 only, over a black ground, and
// keeps EMOINS: TDIFMUG(J).  Such a run differs from the wavelength's own in very little.  The packed source operators never
// touch the solar slot, so those of order 0 are the wavelength's; what changes is the solar cosine and with it the order-1
// source vectors, which need the solar column of P, R, T (c = -mu_J) next to the table columns +-1..N of order 0.
//
// sosgpu_trans_spectrum (api_solve.hip) therefore makes every (context, direction) pair a CHILD entry of a device context table
// and every (bin, direction) pair an ITEM of one multi-wavelength solve:
//   k_trans_table   child entries: the parent's with n0 = J, mus = mu[J-1], smax = 0, ro = 0, no surface, its own sv
//   k_trans_sv      sv[4][kp] of every child, by the statements of noyaux.hip (noyaux_dev.h): the same bits as the tables of
//                   a context created for that incidence
//   k_trans_items   ctx_of_item, nt, iborm = 0 and the profile rows of the items, and their cleared flux
//   (the solve: launch_sos_os_multi / launch_sos_stream_multi, untouched)
//   k_trans_gather  tdifmug[b][J-1] = EMOINS of item (b, J)
#include "sos_common.h"
#include "kernels.h"
#include "noyaux_dev.h"

#pragma clang fp contract(off)

// thread t = child i * N + (J - 1)
__global__ void k_trans_table(const SosDev *__restrict__ parents, const int nchild, const int n, SosDev *__restrict__ children,
                              double *__restrict__ sv)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchild) return;
    SosDev c = parents[t / n];
    const int j = t % n + 1;
    c.smax = 0;
    c.n0 = j;
    c.mus = c.mu[j - 1];
    c.ro = 0.;
    c.imat_surf = 0; c.ifresnel = 0;
    c.f11sun = 0.; c.f12sun = 0.;
    c.fres = nullptr; c.mp_gnd = nullptr; c.rdir = nullptr;      // read under the two flags only
    c.sv = sv + (size_t)t * 4 * c.kp;
    // prt, mp_aer, mp_vt, mp_uf: the parent's, whose order 0 comes first in each
    children[t] = c;
}

// One workgroup per child.  LDS: the recurrence coefficients of order 0 (they do not depend on the direction, so the
// workgroup forms them side by side), then the solar column of P, R, T, which one lane walks upwards in l as k_gsf does.
__global__ void k_trans_sv(const SosDev *__restrict__ children)
{
    extern __shared__ double lds[];
    const SosDevK &cx = *(const SosDevK *)(unsigned long long)(children + blockIdx.x);
    const int B = cx.os_nb, N = cx.n, kp = cx.kp;
    GsfCoef *kc = reinterpret_cast<GsfCoef *>(lds);             // [B+1], entries 2 .. B-1 used
    double *sp = lds + (size_t)5 * (B + 1), *sr = sp + (B + 1), *st = sr + (B + 1);
    for (int l = threadIdx.x; l <= B; l += blockDim.x) {
        if (l >= 2 && l <= B - 1) kc[l] = gsf_coef(0, l);
        sp[l] = 0.; sr[l] = 0.; st[l] = 0.;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double c = -cx.mus;
        double p2, r2;
        gsf_start0(c, p2, r2);
        sp[0] = 1.; sp[1] = c; sp[2] = p2; sr[2] = r2;
        double pl = p2, plm = c, rl = r2, rlm = 0., tl = 0., tlm = 0.;
        for (int l = 2; l <= B - 1; l++) {
            double pn, rn, tn;
            gsf_step(kc[l], c, pl, plm, rl, rlm, tl, tlm, pn, rn, tn);
            sp[l + 1] = pn; sr[l + 1] = rn; st[l + 1] = tn;
            plm = pl; pl = pn; rlm = rl; rl = rn; tlm = tl; tl = tn;
        }
    }
    __syncthreads();
    PrtSun q;
    q.tab = prt_table(cx, 0);
    q.sp = sp; q.sr = sr; q.st = st;
    for (int r = threadIdx.x; r < kp; r += blockDim.x) {
        double v[4] = {0., 0., 0., 0.};
        if (r < cx.r6) sv_rows(q, cx.coef, 0, B, N, r, cx.f11sun, cx.f12sun, cx.beta2, cx.gamma2, cx.alpha2, v);
        cx.sv[0 * kp + r] = v[0]; cx.sv[1 * kp + r] = v[1]; cx.sv[2 * kp + r] = v[2]; cx.sv[3 * kp + r] = v[3];
    }
}

// Element e of the items' profile rows: item = b * N + (J - 1) takes the three rows of bin b; the thread of a row's first
// element also writes the item's scalars.  A bin whose context index is out of range becomes a malformed item (nt = -1).
__global__ void k_trans_items(const TransItems a)
{
    const size_t row = (size_t)3 * a.lp;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)a.nb * a.n * row) return;
    const size_t item = e / row, off = e % row;
    const size_t b = item / a.n;
    a.prof_item[e] = a.prof[b * row + off];
    if (off == 0) {
        const int j0 = (int)(item % a.n);
        const int c = a.ctx_of_bin ? a.ctx_of_bin[b] : 0;
        const bool ok = c >= 0 && c < a.nctx;
        a.ctx_of_item[item] = (ok ? c : 0) * a.n + j0;
        a.nt_item[item] = ok ? a.nt[b] : -1;
        a.iborm_item[item] = 0;
        a.flux[2 * item] = 0.; a.flux[2 * item + 1] = 0.;
    }
}

__global__ void k_trans_gather(const size_t nitems, const double *__restrict__ flux, double *__restrict__ tdifmug)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nitems) tdifmug[i] = flux[2 * i];
}

void launch_trans_table(const SosDev *d_parents, int nchild, int n, SosDev *d_children, double *d_sv, int os_nb_max, hipStream_t st)
{
    k_trans_table<<<(nchild + 63) / 64, 64, 0, st>>>(d_parents, nchild, n, d_children, d_sv);
    k_trans_sv<<<nchild, 256, trans_sv_lds_bytes(os_nb_max), st>>>(d_children);
}

void launch_trans_items(const TransItems &a, hipStream_t st)
{
    const size_t ne = (size_t)a.nb * a.n * 3 * a.lp;
    k_trans_items<<<(unsigned)((ne + 255) / 256), 256, 0, st>>>(a);
}

void launch_trans_gather(size_t nitems, const double *d_flux, double *d_tdifmug, hipStream_t st)
{
    k_trans_gather<<<(unsigned)((nitems + 255) / 256), 256, 0, st>>>(nitems, d_flux, d_tdifmug);
}
