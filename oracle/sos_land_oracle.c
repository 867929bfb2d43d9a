/* oracle/sos_land_oracle.c -- CPU restatement of the land-surface reflection matrices and model functions.
 *
 * TEST INFRASTRUCTURE ONLY (see sos_oracle.h).
 *
 * Follows, for -SURF.Type 3 (Roujean), 4 (+ Rondeaux-Herman), 5 (+ Breon) and 7 (+ Maignan):
 *   SOS_ROUJEAN        src/SOS_ROUJEAN.F:212 = SOS_FSF_ROUJEAN (:417) + SOS_CALC_F_ROUJEAN (:891) + SOS_MISE_FORMAT_RJ (:1102)
 *   SOS_SURFACE_BPDF   src/SOS_SURFACE_BPDF.F:219: SOS_GSF_RONDEAUX_BREON (:463), SOS_GSF_MAIGNAN (:1305) with
 *                      SOS_CALCG_MAIGNAN (:1606), then SOS_MAT_FRESNEL / SOS_MAT_REFLEXION(1.0, ...) / SOS_MISE_FORMAT
 *                      (sos_glitter_oracle.c, shared with the sea surface)
 *   SOS_BPDF_AJOUT_BRDF src/SOS_SURFACE.F:2503: BPDF + BRDF, REAL*4 element by element
 * Nadal (-SURF.Type 6) is refused by the reference's own SOS_PROC and is not restated.
 *
 * Plain fp64, every sum serial in index order.  The reference sources are not part of this repository: the restatement is
 * pinned to the surface files and radiances the compiled reference wrote (tests/golden/sos_proc_land_*.npz,
 * sos_proc_cfg5_roujean_maignan.npz) by tests/test_land.py.
 */
#include "sos_oracle.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define PH_NU 1024   /* SOS.h:319 */

/* SOS_CALC_F_ROUJEAN (SOS_ROUJEAN.F:891-1000); phi in the Roujean convention */
double sos_oracle_calc_f_roujean(double k0, double k1, double k2, double c1, double s1, double c2, double s2, double phi)
{
    const double pi = 4. * atan(1.0);
    double xphi = phi, xc1 = c1, xs1 = s1, xc2 = c2, xs2 = s2;
    double cosphi, tants, tantv, f1, coszeta, zeta, f2;
    if (xphi < 0.) xphi = -xphi;
    if (xphi > pi) xphi = 2. * pi - xphi;
    if (acos(c1) * 180. / pi > 60) { xc1 = cos(60 * pi / 180.); xs1 = sin(60 * pi / 180.); } /* CTE_TETAS_LIM_ROUJEAN */
    if (acos(c2) * 180. / pi > 60) { xc2 = cos(60 * pi / 180.); xs2 = sin(60 * pi / 180.); } /* CTE_TETAV_LIM_ROUJEAN */
    cosphi = cos(xphi); tants = xs1 / xc1; tantv = xs2 / xc2;
    f1 = 0.5 * ((pi - xphi) * cosphi + sin(xphi)) * tants * tantv;
    f1 = f1 - tants - tantv;
    f1 = f1 - sqrt(tants * tants + tantv * tantv - 2. * tantv * tants * cosphi);
    f1 = f1 / pi;
    coszeta = xc1 * xc2 + xs1 * xs2 * cosphi;
    if (fabs(fabs(coszeta) - 1.) <= 1.e-10) coszeta = (coszeta >= (1. - 1.e-10) && coszeta <= (1. + 1.e-10)) ? 1. : -1.;
    zeta = acos(coszeta);
    f2 = 4. * ((pi / 2. - zeta) * coszeta + sin(zeta)) / (3. * pi * (xc1 + xc2));
    f2 = f2 - (1. / 3.);
    return (k0 + k1 * f1 + k2 * f2) * c2 * c1;
}

/* SOS_CALCG_MAIGNAN (SOS_SURFACE_BPDF.F:1606-1641) */
double sos_oracle_calcg_maignan(double c1, double c2, double s12, double phi, double coef_c)
{
    double cos2i = c1 * c2 - s12 * cos(phi);
    double tan2i = (1 - cos2i) / (1 + cos2i);
    if (tan2i < 0.) tan2i = 0.;
    return coef_c * exp(-sqrt(tan2i)) / (1. / c1 + 1. / c2);
}

/* Tie audit of SOS_FSF_ROUJEAN's two stop rules: [0] B1 against CTE_SEUIL_SF_ROUJEAN, [1] B1 against the previous B1. */
static double fsf_margin[2] = {1e300, 1e300};
static void audit(int k, double tested, double threshold)
{
    double m = fabs(tested / threshold - 1.);
    if (m < fsf_margin[k]) fsf_margin[k] = m;
}

/* SOS_FSF_ROUJEAN (SOS_ROUJEAN.F:417-700) for one ordered pair: 1025 samples of the BRDF over [0, pi], the rectangle sum
 * E(IS) (:589-596), the largest relative error B1 of the recombined series (:601-623) and its two stop rules.
 * e[0..os_nb] (orders not computed stay zero; the order that made B1 grow is kept, as the reference stores it, :640-643).
 * Returns IL; *neg is set when a sample is negative (IER = -1, :548).
 * cs (optional): cos(is * (i * q)) for is = 0..os_nb, i = 0..1024 as [os_nb+1][1025] -- the cosines do not depend on the
 * pair, so a caller that runs many pairs tabulates them once; NULL computes them in place (the same values). */
int sos_oracle_fsf_roujean_pair(double k0, double k1, double k2, double mu1, double mu2, int os_nb, const double *cs, double *e,
                                int *neg)
{
    const double pi = acos(-1.0);
    static double u[PH_NU + 1], t1[PH_NU + 1];
    const double c1 = mu1, s1 = sqrt(1 - c1 * c1), c2 = mu2, s2 = sqrt(1 - c2 * c2);
    const double q = pi / PH_NU;
    double b1_prec = 1.e300;
    int i, is, il = os_nb;
    for (i = 0; i <= PH_NU; i++) {
        double phi = q * i;
        u[i] = sos_oracle_calc_f_roujean(k0, k1, k2, c1, s1, c2, s2, pi - phi);
        if (u[i] < 0.) *neg = 1;
        t1[i] = 0.;
    }
    for (is = 0; is <= os_nb; is++) e[is] = 0.;
    for (is = 0; is <= os_nb; is++) {
        double y = 0., es, b1 = 0.;
        for (i = 0; i <= PH_NU; i++) y = y + u[i] * (cs ? cs[(size_t)is * (PH_NU + 1) + i] : cos(is * (i * q)));
        es = y * q / pi;
        e[is] = es;
        for (i = 0; i <= PH_NU; i++) {
            double d;
            t1[i] = (is == 0) ? es : t1[i] + 2. * es * (cs ? cs[(size_t)is * (PH_NU + 1) + i] : cos(is * (i * q)));
            d = fabs((t1[i] - u[i]) / u[i]);
            if (d > b1) b1 = d;
        }
        audit(0, b1, (double)0.001f);
        if (!(b1 > (double)0.001f)) { il = is; break; }   /* CTE_SEUIL_SF_ROUJEAN (REAL*4 literal, SOS.h:339) */
        if (is > 0) audit(1, b1, b1_prec);
        if (!(b1 < b1_prec)) { il = is - 1; break; }
        b1_prec = b1;
    }
    return il;
}

struct maignan { double c1, c2, s12, coef_c; };
static double maignan_g(const void *p, double phi)
{
    const struct maignan *m = p;
    return sos_oracle_calcg_maignan(m->c1, m->c2, m->s12, phi, m->coef_c);
}

/* SOS_GSF_MAIGNAN for one pair: the quadrature of SOS_GSF around SOS_CALCG_MAIGNAN.  e[0..os_nm]; returns IL. */
int sos_oracle_gsf_maignan_pair(double mu1, double mu2, double coef_c, int os_nm, double *e)
{
    struct maignan m;
    m.c1 = mu1; m.c2 = mu2; m.coef_c = coef_c;
    m.s12 = sqrt(1 - mu1 * mu1) * sqrt(1 - mu2 * mu2);
    return sos_oracle_gsf_quad(maignan_g, &m, os_nm, e);
}

/* Land-surface matrices end to end.  out: REAL*4 [os_nb+1][9][N][N] in surface-file record order.
 * il_nn (optional) [N*N], e_nn (optional) [N*N][os_nb+1]: the Roujean series of the ordered pairs (I1-1)*N + (I2-1).
 * Returns 0, or -1 when the Roujean function is negative for some geometry (the matrices are still computed). */
int sos_oracle_land(int isurf, int n, const double *mu, const double *chr, double k0, double k1, double k2, double coef_c,
                    double ind, int os_nb, int os_ns, int os_nm, float *out, int *il_nn, double *e_nn)
{
    const size_t cnt = (size_t)(os_nb + 1) * 9 * n * n;
    const int npairs = n * (n + 1) / 2;
    double *es = calloc(os_nb + 1, sizeof(double));
    float *brdf = calloc(cnt, sizeof(float));
    int i, j, s, neg = 0;
    size_t k;
    double *cs = malloc(sizeof(double) * (size_t)(os_nb + 1) * (PH_NU + 1));
    fsf_margin[0] = fsf_margin[1] = 1e300;
    sos_oracle_quad_margin_reset();
    for (s = 0; s <= os_nb; s++)
        for (i = 0; i <= PH_NU; i++) cs[(size_t)s * (PH_NU + 1) + i] = cos(s * (i * (acos(-1.0) / PH_NU)));
    /* SOS_FSF_ROUJEAN + SOS_MISE_FORMAT_RJ (:1102-1224): P11(I,J) = REAL(E_(I,J)(IS)), every other element zero */
    for (i = 0; i < n; i++)
        for (j = 0; j < n; j++) {
            int il = sos_oracle_fsf_roujean_pair(k0, k1, k2, mu[i], mu[j], os_nb, cs, es, &neg);
            if (il_nn) il_nn[i * n + j] = il;
            if (e_nn) memcpy(e_nn + ((size_t)i * n + j) * (os_nb + 1), es, sizeof(double) * (os_nb + 1));
            for (s = 0; s <= os_nb; s++) brdf[(((size_t)s * 9 + 0) * n + j) * n + i] = (float)es[s];
        }
    if (isurf == 3) memcpy(out, brdf, cnt * sizeof(float));
    else {
        double *coefs = calloc((size_t)4 * (os_ns + 1), sizeof(double));
        int *il = calloc(npairs, sizeof(int));
        double *e = calloc((size_t)npairs * (os_nm + 1), sizeof(double));
        double *g = calloc(os_nm + 1, sizeof(double));
        int pair = 0;
        sos_oracle_mat_fresnel(n, mu, chr, ind, os_ns, coefs, coefs + (os_ns + 1), coefs + 2 * (os_ns + 1), coefs + 3 * (os_ns + 1));
        for (i = 0; i < n; i++)
            for (j = 0; j <= i; j++, pair++) {
                double *ep = e + (size_t)pair * (os_nm + 1);
                if (isurf == 4) ep[0] = 1. / (1. / mu[i] + 1. / mu[j]);   /* Rondeaux-Herman, SOS_SURFACE_BPDF.F:560-575 */
                else if (isurf == 5) ep[0] = 1.;                          /* Breon */
                else {
                    il[pair] = sos_oracle_gsf_maignan_pair(mu[i], mu[j], coef_c, os_nm, g);
                    memcpy(ep, g, sizeof(double) * (il[pair] + 1));
                }
            }
        sos_oracle_mat_reflexion(n, mu, 1.0, os_nb, os_ns, os_nm, coefs, il, e, out);
        for (k = 0; k < cnt; k++) out[k] = out[k] + brdf[k];              /* SOS_BPDF_AJOUT_BRDF, REAL*4 */
        free(coefs); free(il); free(e); free(g);
    }
    free(es); free(brdf); free(cs);
    return neg ? -1 : 0;
}

/* Stop margins of the last sos_oracle_land call: m5[0..1] SOS_FSF_ROUJEAN (B1 <= 1e-3; B1 against the previous B1),
 * m5[2..4] the Maignan quadrature (per-level 1e-4, 1e-3 closure, 1 % bisection; 1e300 where the test never ran). */
void sos_oracle_land_margin(double *m5)
{
    m5[0] = fsf_margin[0]; m5[1] = fsf_margin[1];
    sos_oracle_quad_margin(m5 + 2);
}
