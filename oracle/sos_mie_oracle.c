/* oracle/sos_mie_oracle.c -- TEST INFRASTRUCTURE ONLY: serial fp64 restatement of the aerosol device chain.
 *
 *   sos_oracle_mie    SOS_MIE + SOS_FPHASE_MIE (src/SOS_MIE.F:205-715, :801-945): the MIE-file records of a list of size
 *                     parameters, one after the other, plain heap arrays (no LDS / scratch distinction), REAL*4 rounding where the
 *                     file record rounds.
 *   sos_oracle_granu  SOS_GRANU (src/SOS_AEROSOLS.F:4392-4820) on given records: sums in record order.
 *
 * Built with -ffp-contract=off: every product and sum below is rounded on its own, in the statement order of the Fortran. */
#include "sos_oracle.h"
#include <math.h>
#include <stdlib.h>

/* arrays with Fortran lower bound -1: element i at [i + 1] */
#define A(x, i) x[(i) + 1]

/* one size parameter; arr: 11 arrays of nmax doubles.  info4: n2 used, break taken (0/1), number of SNA rescales, n1 used;
 * unrounded (optional) [3 + 3 W]: Qext, Qsca, g, Imie, Qmie, Umie before the REAL*4 rounding of the record */
static void mie_one(int nbmu, const double *xmu, double rn, double in, double alpha, int nmax, double *arr, float *r, double *gout,
                    int *info4, double *unrounded)
{
    double *cna = arr, *sna = cna + nmax, *rgna = sna + nmax, *igna = rgna + nmax;
    double *rdna = igna + nmax, *rdnb = rdna + nmax, *idnb = rdnb + nmax;
    double *ra = idnb + nmax, *ia = ra + nmax, *rb = ia + nmax, *ib = rb + nmax;
    const int W = 2 * nbmu + 1;
    int n1 = (int)(alpha + alpha + 20), n2 = (int)(alpha + alpha + 5);
    int broke = 0, nresc = 0;
    double c2 = -sin(alpha), c1 = cos(alpha), rg = 0., ig = -1.;             /* CNA(-1), CNA(0), RGNA(0), IGNA(0) */
    A(cna, -1) = c2; A(cna, 0) = c1;
    A(rgna, -1) = 0.; A(rgna, 0) = rg; A(igna, -1) = 0.; A(igna, 0) = ig;
    for (int i = 1; i <= n2; i++) {                                          /* SOS_MIE.F:455-470 */
        const double x = rg, z = i / alpha, y = ig;
        const double w = ((z - x) * (z - x) + (y * y));
        rg = (z - x) / w - z;
        ig = y / w;
        const double c0 = (2 * i - 1.) * c1 / alpha - c2;
        A(rgna, i) = rg; A(igna, i) = ig; A(cna, i) = c0;
        c2 = c1; c1 = c0;
        if (!(c0 < 1.e304)) { n2 = i; n1 = i + 15; broke = 1; break; }
    }
    const double rbeta = rn * alpha, ibeta = in * alpha;
    const double xx1 = rbeta * rbeta + ibeta * ibeta;
    const double xx2 = rbeta / xx1, xx3 = ibeta / xx1;
    double nb_r = 0., nb_i = 0., na_r = 0., s_up = 0., s_at = 1.;
    A(rdna, n1) = 0.; A(rdnb, n1) = 0.; A(idnb, n1) = 0.; A(sna, n1) = 0.; A(sna, n1 - 1) = 1.;
    for (int i = n1 - 1; i >= 0; i--) {                                      /* :482-503 */
        double z = nb_r + (i + 1.) * xx2, w = nb_i - (i + 1.) * xx3;
        const double x4 = z * z + w * w;
        nb_r = (i + 1.) * xx2 - z / x4;
        nb_i = -(i + 1.) * xx3 + w / x4;
        z = (i + 1.) / alpha;
        na_r = z - 1. / (na_r + z);
        double s_lo = (2. * i + 1.) * s_at / alpha - s_up;
        A(rdnb, i) = nb_r; A(idnb, i) = nb_i; A(rdna, i) = na_r; A(sna, i - 1) = s_lo;
        s_up = s_at;
        if (s_lo > 1.e304) {
            const int test = i - 1;
            const double xx = s_lo;
            for (int j = test; j <= n2; j++) A(sna, j) = A(sna, j) / xx;
            s_lo = A(sna, test);
            s_up = A(sna, test + 1);
            nresc++;
        }
        s_at = s_lo;
    }
    double q = A(sna, 0) / sin(alpha);
    for (int i = 0; i <= n2; i++) A(sna, i) = A(sna, i) / q;
    double un = 1;
    for (int i = 1; i <= n2; i++) {                                          /* :509-555 */
        const double x1 = A(sna, i), x2 = A(cna, i), x3 = A(rdnb, i), x4 = A(idnb, i), x5 = A(rdna, i);
        const double x6 = A(rgna, i), x7 = A(igna, i);
        double y1 = x3 - rn * x5, y2 = x4 - in * x5, y3 = x3 - rn * x6 + in * x7, y4 = x4 - rn * x7 - in * x6;
        const double y5 = rn * x3 - in * x4 - x5, y6 = in * x3 + rn * x4, y7 = rn * x3 - in * x4 - x6,
                     y8 = in * x3 + rn * x4 - x7;
        const double z4 = y2 * y3 - y1 * y4, z3 = y1 * y3 + y2 * y4, z5 = x1 * x1 + x2 * x2, z6 = y3 * y3 + y4 * y4;
        const double z7 = y5 * y7 + y6 * y8, z8 = y6 * y7 - y5 * y8, z9 = y7 * y7 + y8 * y8;
        q = (i + i + 1.) / i / (i + 1.) * un;
        if (x2 > 1.e300) { y1 = 0.; y2 = 0.; y3 = 0.; y4 = 0.; }
        else {
            y1 = x1 * (x1 * z3 + x2 * z4) / z5 / z6;
            y2 = x1 * (x1 * z4 - x2 * z3) / z5 / z6;
            y3 = x1 * (x1 * z7 + x2 * z8) / z5 / z9;
            y4 = x1 * (x1 * z8 - x2 * z7) / z5 / z9;
        }
        ra[i] = y2 * q; ib[i] = y3 * q;
        q = -q;
        rb[i] = y4 * q; ia[i] = y1 * q;
        un = -un;
    }
    ra[0] = 0.; ia[0] = 0.; rb[0] = 0.; ib[0] = 0.;
    ra[n2 + 1] = 0.; ia[n2 + 1] = 0.; rb[n2 + 1] = 0.; ib[n2 + 1] = 0.;
    double qext = 0., qsca = 0., g = 0.;
    int j = -1;
    double x = ra[1], y = ia[1], z = rb[1], tt0 = ib[1];
    for (int n = 1; n <= n2; n++) {                                          /* :572-588 */
        const int m = n + 1;
        const double xx = ra[m], yy = ia[m], zz = rb[m], tt = ib[m];
        const double a2 = (n + 1.);
        qext = qext + n * a2 * j * (y - tt0);
        qsca = qsca + n * n * a2 * a2 / (n + a2) * (x * x + y * y + z * z + tt0 * tt0);
        j = -j;
        g = g - a2 * n / (a2 + n) * (n * (a2 + 1.) * (a2 + 1.) / (2. * n + 3.) * (y * yy + x * xx + tt0 * tt + z * zz) + y * tt0 + x * z);
        x = xx; y = yy; z = zz; tt0 = tt;
    }
    const double w6 = 2. / alpha / alpha;
    qext = w6 * qext; qsca = w6 * qsca;
    g = 4. * g / qsca / alpha / alpha;
    r[0] = (float)alpha; r[1] = (float)qext; r[2] = (float)qsca; r[3] = 0.f;
    *gout = g;
    if (unrounded) { unrounded[0] = qext; unrounded[1] = qsca; unrounded[2] = g; }
    const double coef = 2. / qsca / (alpha * alpha);
    for (int jj = 0; jj < W; jj++) {                                         /* SOS_FPHASE_MIE :873-900 */
        const double xm = -xmu[jj];
        double pim = 0., piv = 1., tau = xm, res1 = 0., res2 = 0., ims1 = 0., ims2 = 0.;
        for (int n = 1; n <= n2; n++) {
            const double ai = ia[n], bi = ib[n], ar = ra[n], br = rb[n];
            res1 = res1 - ai * piv - bi * tau;
            res2 = res2 + ai * tau + bi * piv;
            ims1 = ims1 + ar * piv + br * tau;
            ims2 = ims2 - ar * tau - br * piv;
            const double pip = ((2. * n + 1.) * xm * piv - (n + 1.) * pim) / n;
            pim = piv; piv = pip;
            tau = (n + 1.) * xm * piv - (n + 2.) * pim;
        }
        const double y1 = res1 * res1 + ims1 * ims1, y2 = res2 * res2 + ims2 * ims2;
        const double y3 = 2. * res2 * res1, y4 = 2. * ims2 * ims1;
        r[4 + jj] = (float)(coef * (y1 + y2));
        r[4 + W + jj] = (float)(coef * (y2 - y1));
        r[4 + 2 * W + jj] = (float)(coef * (y3 + y4));
        if (unrounded) {
            unrounded[3 + jj] = coef * (y1 + y2);
            unrounded[3 + W + jj] = coef * (y2 - y1);
            unrounded[3 + 2 * W + jj] = coef * (y3 + y4);
        }
    }
    info4[0] = n2; info4[1] = broke; info4[2] = nresc; info4[3] = n1;
}

int sos_oracle_mie_f64(int nbmu, const double *xmu, double rn, double in, int nalpha, const double *alphas, float *rec, double *g,
                       int *info, double *unrounded)
{
    const int W = 2 * nbmu + 1;
    if (nbmu < 1 || nalpha < 1) return -1;
    double amax = 0.;
    for (int a = 0; a < nalpha; a++) {
        if (!(alphas[a] > 0.) || !(alphas[a] < 1.e8)) return -1;
        if (alphas[a] > amax) amax = alphas[a];
    }
    const int nmax = (int)(2 * amax + 24) + 4;
    double *arr = (double *)malloc((size_t)11 * nmax * sizeof(double));
    if (!arr) return -2;
    for (int a = 0; a < nalpha; a++) {
        int i4[4];
        mie_one(nbmu, xmu, rn, in, alphas[a], nmax, arr, rec + (size_t)a * (4 + 3 * W), g + a, i4,
                unrounded ? unrounded + (size_t)a * (3 + 3 * W) : 0);
        if (info) for (int k = 0; k < 4; k++) info[4 * a + k] = i4[k];
    }
    free(arr);
    return 0;
}

int sos_oracle_mie(int nbmu, const double *xmu, double rn, double in, int nalpha, const double *alphas, float *rec, double *g,
                   int *info)
{
    return sos_oracle_mie_f64(nbmu, xmu, rn, in, nalpha, alphas, rec, g, info, 0);
}

/* the REAL*4 step ladder of SOS_GRANU (:4523-4527), the literals of SOS_MIE's */
static float granu_step(float a)
{
    float pas = 0.0001f;
    if (a > 0.10f) pas = 0.001f;
    if (a > 1.00f) pas = 0.01f;
    if (a > 10.f) pas = 0.05f;
    if (a > 30.f) pas = 0.10f;
    if (a > 100.f) pas = 1.00f;
    return pas;
}

int sos_oracle_granu(int nbmu, int na, const float *rec, int igranu, double v1, double v2, double v3, double wa, double alphaf,
                     double *out, int *nuse_out)
{
    const int W = 2 * nbmu + 1, RS = 4 + 3 * W;
    const double pi = 3.141592653589793;
    if (nbmu < 1 || na < 1 || igranu < 1 || igranu > 2) return -1;
    double kmat1 = 0., kmat2 = 0., somme = 0.;
    for (int o = 0; o < 3 * W; o++) out[3 + o] = 0.;
    float pas_prev = 0.0001f;              /* PAS still holds the previous record's step when the stop is tested (:4520) */
    int i = 0;
    for (; i < na; i++) {
        const float *r_ = rec + (size_t)i * RS;
        const float af = r_[0];
        const double a64 = (double)af;
        if (a64 >= (alphaf - (double)pas_prev)) break;                       /* IF (ALPHA.GE.(ALPHAF-PAS)) GOTO 40 */
        const float pas = granu_step(af);
        pas_prev = pas;
        const double r = a64 * wa / 2. / pi;
        double nr;
        if (igranu == 1) {
            const double b = log(r / v1) / v2;
            nr = exp(-b * b / 2.) / (r * v2 * sqrt(2 * pi));
        } else {
            if (r > v3) break;                                               /* IF (R.GT.RMAX) GOTO 40 */
            nr = (r <= v1) ? pow(v1, -v2) : pow(r, -v2);
        }
        const double pr = wa * (double)pas / 2. / pi;
        const double x1 = nr * pr * pi * (r * r);
        kmat1 = kmat1 + x1 * (double)r_[1];
        const double x1s = (double)r_[2] * x1;
        kmat2 = kmat2 + x1s;
        somme = somme + nr * pr;
        for (int o = 0; o < 3 * W; o++) out[3 + o] = out[3 + o] + (double)r_[4 + o] * x1s;
    }
    out[0] = kmat1 / somme;
    out[1] = kmat2 / somme;
    out[2] = somme;
    for (int o = 0; o < 3 * W; o++) out[3 + o] = out[3 + o] / kmat2;
    *nuse_out = i;
    return 0;
}
