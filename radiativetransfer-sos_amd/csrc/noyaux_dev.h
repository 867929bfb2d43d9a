// csrc/noyaux_dev.h -- the statements of SOS_NOYAUX that more than one kernel executes (gfx950, device only).
//
// noyaux.hip builds the tables of a context from them; trans.hip forms the order-1 vectors of the -SOS.Trans incidences
// from them, where the solar column of P, R, T is not in any context's table.  Both callers execute the same statements in
// the same order with contraction disabled, so a value formed here has the same bits wherever it is formed.
#pragma once
#include "sos_common.h"

#pragma clang fp contract(off)

// Upward recurrence of the generalised spherical functions in l (SOS_OS.F:2067-2100): the coefficients of the step
// l -> l + 1 of Fourier order s.  They do not depend on the direction.
struct GsfCoef { double a, b, d, e, f; };

__device__ inline GsfCoef gsf_coef(const int s, const int l)
{
    GsfCoef k;
    k.a = (2 * l + 1.) / sqrt((l + s + 1.0) * (l - s + 1.));
    k.b = sqrt((double)((l + s) * (l - s))) / (2. * l + 1.);
    k.d = (l + 1.) * (2 * l + 1.) / sqrt((l + 3.0) * (l - 1.) * (l + s + 1.) * (l - s + 1.));
    k.e = sqrt((l + 2.0) * (l - 2.) * (l + s) * (l - s)) / (l * (2. * l + 1.));
    // F = 2.*IS/(L*(L+1.)) is evaluated in REAL*4 by the reference (SOS_OS.F:2079)
    k.f = (double)((2.f * (float)s) / ((float)l * ((float)l + 1.f)));
    return k;
}

// one step: the values at l + 1 for the cosine c from those at l and l - 1
__device__ inline void gsf_step(const GsfCoef &k, const double c, const double pl, const double plm, const double rl,
                                const double rlm, const double tl, const double tlm, double &pn, double &rn, double &tn)
{
    pn = k.a * (c * pl - k.b * plm);
    rn = k.d * (c * rl - k.f * tl - k.e * rlm);
    tn = k.d * (c * tl - k.f * rl - k.e * tlm);
}

// starting values of order 0 at l = 2 (SOS_OS.F:1970-1991); P_0 = 1, P_1 = c
__device__ inline void gsf_start0(const double c, double &p2, double &r2)
{
    const double x26 = 2. * sqrt(6.0);
    p2 = (3. * c * c - 1.) * 0.5;
    r2 = 3. * (1. - c * c) / x26;
}

// P, R, T of one Fourier order as the kernels of SOS_NOYAUX read them: value at degree l and direction a in -N..N (0 = the
// solar slot).  PrtTable: the block of a context's prt table.
struct PrtTable {
    const double *P, *R, *T;          // [os_nb+1][W], each pointing at direction 0
    int W;
    __device__ double p(const int l, const int a) const { return P[(size_t)l * W + a]; }
    __device__ double r(const int l, const int a) const { return R[(size_t)l * W + a]; }
    __device__ double t(const int l, const int a) const { return T[(size_t)l * W + a]; }
};

template <class CX>
__device__ inline PrtTable prt_table(const CX &cx, const int s)
{
    const int N = cx.n, W = cx.w, B = cx.os_nb;
    PrtTable q;
    q.P = cx.prt + ((size_t)(s * 3 + 0) * (B + 1)) * W + N;
    q.R = cx.prt + ((size_t)(s * 3 + 1) * (B + 1)) * W + N;
    q.T = cx.prt + ((size_t)(s * 3 + 2) * (B + 1)) * W + N;
    q.W = W;
    return q;
}

// PrtSun: the directions +-1..N from a table, the solar slot from three columns of its own [os_nb+1] (another incidence than
// the one the table was built for: the columns +-j do not depend on the sun)
struct PrtSun {
    PrtTable tab;
    const double *sp, *sr, *st;
    __device__ double p(const int l, const int a) const { return a ? tab.p(l, a) : sp[l]; }
    __device__ double r(const int l, const int a) const { return a ? tab.r(l, a) : sr[l]; }
    __device__ double t(const int l, const int a) const { return a ? tab.t(l, a) : st[l]; }
};

// One element of one of the six kernels of SOS_NOYAUX (SOS_OS.F:2134-2143) for order s:
//   X: 0 BP, 1 GR, 2 GT, 3 ARR, 4 ART, 5 ATT;  a, b in -N..N (0 = solar slot)
// with the aerosol coefficient arrays coef = alpha, beta, gamma, zeta [4][B+1], l = s..B ascending.
template <class PRT>
__device__ inline double ktab_sum(const PRT &q, const double *coef, const int s, const int B, const int X, const int a, const int b)
{
    const double *AL = coef, *BE = coef + (B + 1), *GA = coef + 2 * (B + 1), *ZE = coef + 3 * (B + 1);
    double sum = 0.;
    for (int l = s; l <= B; l++) {
        switch (X) {
        case 0: sum = sum + BE[l] * q.p(l, a) * q.p(l, b); break;
        case 1: sum = sum + GA[l] * q.p(l, a) * q.r(l, b); break;
        case 2: sum = sum + GA[l] * q.p(l, a) * q.t(l, b); break;
        case 3: { double r1 = q.t(l, a) * q.t(l, b), r2 = q.r(l, a) * q.r(l, b); sum = sum + ZE[l] * r1 + AL[l] * r2; } break;
        case 4: sum = sum + AL[l] * q.r(l, b) * q.t(l, a) + ZE[l] * q.r(l, a) * q.t(l, b); break;
        default: { double r1 = q.t(l, a) * q.t(l, b), r2 = q.r(l, a) * q.r(l, b); sum = sum + AL[l] * r1 + ZE[l] * r2; } break;
        }
    }
    return sum;
}

// The four order-1 source values of state row r < 6N (the rows of sv, noyaux.hip k_sv) for order s:
//   v[0]  aerosol part of SOS_FSOURCE_ORDRE1:  I: BP(0,J), Q: GR(0,J), U: -GT(0,J)   (SOS_OS.F:2557-2559)
//   v[1]  molecular part (s <= 2)
//   v[2]  aerosol part of SOS_FSOURCE_DIFF_FRESNEL1 for the field of direction J = +-k, which uses the mirrored direction
//         D = -J (SOS_OS.F:3280-3289): I: F11sun BP(0,D) + F12sun GR(D,0), Q: F11sun GR(0,D) + F12sun ARR(0,D),
//         U: F11sun GT(0,D) + F12sun ART(D,0)
//   v[3]  molecular part of the same (s <= 2)
// f11, f12: the Fresnel matrix at the solar incidence; b2, g2, a2: the molecular coefficients of the context.
template <class PRT>
__device__ inline void sv_rows(const PRT &q, const double *coef, const int s, const int B, const int N, const int r,
                               const double f11, const double f12, const double b2, const double g2, const double a2, double v[4])
{
    double v0 = 0., v1 = 0., v2 = 0., v3 = 0.;
    const int c = r / (2 * N), d = r % (2 * N);
    const int J = d < N ? d + 1 : -(d - N + 1);
    const int D = -J;
    // molecular parts: single l = 2 terms, multiplied in the order the reference writes each of them (SOS_OS.F:2533-2545,
    // 3237-3252 -- GR(D,0) is written differently for the two signs of D), so that they are its values to the last bit
    const bool ray = s <= 2;
    const double b0 = (s == 0) ? 1. : 0.;
    const double spl = q.p(2, 0), srl = q.r(2, 0);
    if (c == 0) {
        v0 = ktab_sum(q, coef, s, B, 0, 0, J);
        v2 = f11 * ktab_sum(q, coef, s, B, 0, 0, D) + f12 * ktab_sum(q, coef, s, B, 1, D, 0);
        if (ray) {
            v1 = b0 + b2 * q.p(2, J) * spl;
            v3 = f11 * (b0 + b2 * q.p(2, D) * spl) + f12 * (D < 0 ? g2 * srl * q.p(2, D) : srl * q.p(2, D) * g2);
        }
    } else if (c == 1) {
        v0 = ktab_sum(q, coef, s, B, 1, 0, J);
        v2 = f11 * ktab_sum(q, coef, s, B, 1, 0, D) + f12 * ktab_sum(q, coef, s, B, 3, 0, D);
        if (ray) {
            v1 = g2 * q.r(2, J) * spl;
            v3 = f11 * (q.r(2, D) * spl * g2) + f12 * (a2 * srl * q.r(2, D));
        }
    } else {
        v0 = -ktab_sum(q, coef, s, B, 2, 0, J);
        v2 = f11 * ktab_sum(q, coef, s, B, 2, 0, D) + f12 * ktab_sum(q, coef, s, B, 4, D, 0);
        if (ray) {
            v1 = -(g2 * q.t(2, J) * spl);
            v3 = f11 * (g2 * spl * q.t(2, D)) + f12 * (a2 * q.t(2, D) * srl);
        }
    }
    v[0] = v0; v[1] = v1; v[2] = v2; v[3] = v3;
}
