/* oracle/sos_profile_oracle.c -- TEST INFRASTRUCTURE ONLY (never linked or imported by the product path).
 *
 * Plain-C restatement of the reference's atmospheric profile discretisation for IPROFIL = 1 (exponential aerosol
 * profile), with or without gas absorption:
 *   SOS_PROFILE   src/SOS_PROFIL.F:224-1170   (no-gas step :349-489, selection :492-508, gas step :509-795,
 *                                               PROFIL file written with format 20 `2X,I5,F10.5,3(E15.8)` :1084,1150)
 *   SOS_DISC      src/SOS_PROFIL.F:1210-1332  (bisection on altitude)
 * Statement order follows the Fortran; REAL*4 literals of inc/SOS.h (CTE_TCOUCHE 0.005, first-layer thickness 0.0002,
 * CTE_DELTA_Z 0.05, CTE_THRESHOLD_DZ 0.001, the .000001 of SOS_DISC) are widened from float exactly as Fortran does.
 * The returned arrays are the values SOS reads back from the PROFIL file (SOS.F:511-516): ZPROF through F10.5, H,
 * PCAER (= XDEL), PCMOL (= YDEL) through E15.8.
 * Pinned against the real reference (oracle/_ref, sos_profile_) by tests/golden/profile_*.npz.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define OS_NT 600          /* CTE_OS_NT            SOS.h:202 */
#define OS_NT_MIN 100      /* CTE_OS_NT_MIN        SOS.h:229 */
#define ABS_NBLEV 50       /* CTE_ABS_NBLEV        SOS.h:250 */
#define TOA_ALT 120.0      /* CTE_TOA_ALT          SOS.h:197 */
#define THRESHOLD_TAUABS 1.5   /* SOS.h:301 (exact in REAL*4) */
static const double TCOUCHE = (double)0.005f;        /* SOS.h:208 */
static const double T_FIRST = (double)0.0002f;       /* CTE_TOA_FIRST_LAYER_OPT_THICKNESS  SOS.h:213 */
static const double DELTA_Z = (double)0.05f;         /* SOS.h:218 */
static const double THRESHOLD_DZ = (double)0.001f;   /* SOS.h:224 */

/* ---- exp mode (sos_profile_oracle_exp_mode): 0 = exp() itself (the default, and the only mode the pins use); 1 / 2 = every
 * exp result moved by +1 / -1 ulp; 3 = by +1 or -1 ulp, chosen by a hash of the argument's bits and a key.  The moved modes
 * exist to find, from the reference alone, which printed digits and which level counts hang on the last bit of exp. */
static int g_exp_mode = 0;
static uint64_t g_exp_key = 0;
static double exp_moved(double x)
{
    const double r = exp(x);
    int up;
    if (!(r > 0.0) || isinf(r)) return r;
    if (g_exp_mode == 1) up = 1;
    else if (g_exp_mode == 2) up = 0;
    else {
        uint64_t u;
        memcpy(&u, &x, sizeof u);
        u = (u ^ g_exp_key) * 0x9E3779B97F4A7C15ull;      /* splitmix64 finaliser */
        u = (u ^ (u >> 30)) * 0xBF58476D1CE4E5B9ull;
        u = (u ^ (u >> 27)) * 0x94D049BB133111EBull;
        up = (int)((u ^ (u >> 31)) & 1u);
    }
    return nextafter(r, up ? INFINITY : 0.0);
}
#define EXP(x) (g_exp_mode == 0 ? exp(x) : exp_moved(x))

void sos_profile_oracle_exp_mode(int mode, unsigned long long key) { g_exp_mode = mode; g_exp_key = key; }

/* what the info form reports besides the profile (all optional: a NULL info costs nothing) */
typedef struct {
    int *bin;            /* [SOS_PROFILE_INFO_BIN] see sos_profile_oracle_info */
    double *binf;        /* [SOS_PROFILE_INFO_BINF] */
    int *lev;            /* [4][OS_NT + 2]: bisection steps, stopped on ZMOY == 0, forced no-gas level, near-DZ skip */
    int *lev_ng;         /* [2][OS_NT + 2]: bisection steps and ZMOY == 0 stop of the no-gas profile's levels */
    double *raw;         /* [4][OS_NT + 2]: Z, H, PCAER, PCMOL before the decimal round trip */
} prof_info;
static int g_disc_steps, g_disc_zero;

/* index (1-based) of the absorption-profile segment holding z: the reference scans upwards without a bound (its grid ends at
 * the ground and z >= 0); the bound only matters for a grid that does not reach z, where the last segment is used */
static int seg_of(double z, const double *altabs, int nblev)
{
    int j = 2;
    while (j < nblev && z < altabs[j - 1]) j++;
    return j;
}

/* gas optical depth at altitude z by the linear interpolation of SOS_DISC (SOS_PROFIL.F:1283-1296) */
static double disc(double dt, double ta, double ha, double tr, double hr, const double *tabs, const double *altabs, int nblev,
                   double tim1, double zmax_init, double tg_zlim, double zlim)
{
    const double ti = tim1 + dt;
    double zmax = zmax_init, zmin = zlim, zmoy;
    g_disc_steps = 0; g_disc_zero = 0;
    for (;;) {
        double tg;
        zmoy = (zmax + zmin) / 2.;
        g_disc_steps++;
        if (tg_zlim > 0.0) {
            const int j = seg_of(zmoy, altabs, nblev);   /* 1-based */
            double zz;
            if (zmoy > altabs[0]) zz = 0;
            else zz = (zmoy - altabs[j - 2]) / (altabs[j - 1] - altabs[j - 2]);
            tg = (1 - zz) * tabs[j - 2] + zz * tabs[j - 1];
        } else tg = 0.0;
        const double tzmoy = ta * EXP(-zmoy / ha) + tr * EXP(-zmoy / hr) + tg;
        const double xd = fabs(ti - tzmoy);
        if (xd < (double).000001f) break;
        if (zmoy == 0.0) { g_disc_zero = 1; break; }
        if ((ti - tzmoy) < 0.0) zmin = zmoy; else zmax = zmoy;
    }
    return zmoy;
}

static double rt_e15_8(double v) { char b[64]; snprintf(b, sizeof b, "%.7E", v); return strtod(b, NULL); }
static double rt_f10_5(double v) { char b[64]; snprintf(b, sizeof b, "%.5f", v); return strtod(b, NULL); }

/* the decimal round trip of n values on its own (fmt 0: E15.8, 1: F10.5), for the device's register form of it */
void sos_profile_oracle_roundtrip(int fmt, long n, const double *in, double *out)
{
    long i;
    for (i = 0; i < n; i++) out[i] = fmt ? rt_f10_5(in[i]) : rt_e15_8(in[i]);
}

#define SOS_PROFILE_INFO_BIN 12
#define SOS_PROFILE_INFO_BINF 9
#define INFO_BIN(k, v) do { if (info && info->bin) info->bin[k] = (v); } while (0)
#define INFO_BINF(k, v) do { if (info && info->binf) info->binf[k] = (v); } while (0)
#define INFO_LEV(r, i, v) do { if (info && info->lev) info->lev[(r) * (OS_NT + 2) + (i)] = (v); } while (0)

/* returns 0, or -1 (IER) when the profile needs more than CTE_OS_NT levels / bad constants.
 * tabs == NULL or absprofil == 7 or tabs[nblev - 1] == 0: no gas.  Arrays hold OS_NT+1 doubles. */
static int profile_core(double tr, double hr, double ta, double ha, int absprofil, int nblev, const double *altabs,
                        const double *tabs, int *nt_out, double *zprof, double *h, double *pcaer, double *pcmol,
                        const prof_info *info)
{
    static double hmol_ng[OS_NT + 2], haer_ng[OS_NT + 2], h_ng[OS_NT + 2], z_ng[OS_NT + 2], pcm_ng[OS_NT + 2], pca_ng[OS_NT + 2];
    static double hmol[OS_NT + 2], haer[OS_NT + 2], habs[OS_NT + 2];
    int nt_ng, nt, i, steps;
    double t_first_ng, t_layer_ng, ttot, z, vr, va, vg, dtau;

    /* (levels past NT of the no-gas profile read as the ground: the gas step looks one past it when a level lands within
     *  THRESHOLD_DZ of the ground -- the Fortran reads whatever its array holds there, and never uses it) */
    memset(z_ng, 0, sizeof z_ng);
    if (info && info->bin) memset(info->bin, 0, SOS_PROFILE_INFO_BIN * sizeof(int));
    if (info && info->binf) memset(info->binf, 0, SOS_PROFILE_INFO_BINF * sizeof(double));
    if (info && info->lev) memset(info->lev, 0, 4 * (OS_NT + 2) * sizeof(int));
    if (info && info->lev_ng) memset(info->lev_ng, 0, 2 * (OS_NT + 2) * sizeof(int));
    if (info && info->raw) memset(info->raw, 0, 4 * (OS_NT + 2) * sizeof(double));

    /* ---- step 1: profile without gas (SOS_PROFIL.F:349-489) */
    ttot = tr + ta;
    if ((ttot / OS_NT_MIN) <= T_FIRST) {
        nt_ng = OS_NT_MIN; t_layer_ng = ttot / nt_ng; t_first_ng = t_layer_ng;
        INFO_BIN(8, 0);
    } else if ((ttot / OS_NT_MIN) < TCOUCHE) {
        nt_ng = OS_NT_MIN + 1; t_first_ng = T_FIRST; t_layer_ng = (ttot - t_first_ng) / OS_NT_MIN;
        INFO_BIN(8, 1);
    } else {
        t_first_ng = T_FIRST;
        nt_ng = (int)((ttot - t_first_ng) / TCOUCHE);
        t_layer_ng = (ttot - t_first_ng) / nt_ng;
        nt_ng = nt_ng + 1;
        INFO_BIN(8, 2);
    }
    INFO_BIN(7, nt_ng);
    INFO_BINF(6, ttot); INFO_BINF(7, t_first_ng); INFO_BINF(8, t_layer_ng);
    if (nt_ng > OS_NT) { INFO_BIN(10, 1); return -1; }
    if (ta == 0.0) {
        hmol_ng[0] = 0.; hmol_ng[1] = t_first_ng;
        for (i = 2; i <= nt_ng; i++) hmol_ng[i] = (i - 1) * t_layer_ng + t_first_ng;
        for (i = 0; i <= nt_ng; i++) { pcm_ng[i] = 1.; pca_ng[i] = 0.; haer_ng[i] = 0.; h_ng[i] = hmol_ng[i]; }
        z_ng[0] = TOA_ALT;
        for (i = 1; i <= nt_ng; i++) z_ng[i] = hr * log(tr / hmol_ng[i]);
    } else {
        z_ng[0] = TOA_ALT; hmol_ng[0] = 0.; haer_ng[0] = 0.; h_ng[0] = 0.;
        dtau = 0.; z = TOA_ALT;
        steps = 0;
        while (dtau < t_first_ng) { z = z - DELTA_Z; dtau = tr * EXP(-z / hr) + ta * EXP(-z / ha); steps++; }
        INFO_BIN(9, steps);
        z_ng[1] = z;
        vr = tr * EXP(-z / hr); va = ta * EXP(-z / ha);
        hmol_ng[1] = vr; haer_ng[1] = va; h_ng[1] = dtau;
        pcm_ng[1] = vr / dtau; pca_ng[1] = va / dtau;
        pcm_ng[0] = pcm_ng[1]; pca_ng[0] = pca_ng[1];
        for (i = 2; i <= nt_ng - 1; i++) {
            z = disc(t_layer_ng, ta, ha, tr, hr, tabs, altabs, nblev, h_ng[i - 1], z_ng[1], 0., 0.);
            if (info && info->lev_ng) { info->lev_ng[i] = g_disc_steps; info->lev_ng[OS_NT + 2 + i] = g_disc_zero; }
            z_ng[i] = z;
            vr = tr * EXP(-z / hr); va = ta * EXP(-z / ha);
            hmol_ng[i] = vr; haer_ng[i] = va; h_ng[i] = vr + va;
            vr = vr - hmol_ng[i - 1]; va = va - haer_ng[i - 1];
            pcm_ng[i] = vr / (vr + va); pca_ng[i] = va / (vr + va);
        }
        z_ng[nt_ng] = 0.; hmol_ng[nt_ng] = tr; haer_ng[nt_ng] = ta; h_ng[nt_ng] = tr + ta;
        vr = tr - hmol_ng[nt_ng - 1]; va = ta - haer_ng[nt_ng - 1];
        pcm_ng[nt_ng] = vr / (vr + va); pca_ng[nt_ng] = va / (vr + va);
    }

    if (absprofil == 7 || tabs == NULL || tabs[nblev - 1] == 0.0) {     /* SOS_PROFIL.F:492-508 */
        nt = nt_ng;
        INFO_BIN(0, -1);
        for (i = 0; i <= nt; i++) {
            zprof[i] = z_ng[i]; h[i] = hmol_ng[i] + haer_ng[i]; pcaer[i] = pca_ng[i]; pcmol[i] = pcm_ng[i];
        }
    } else {
        /* ---- step 2: profile with gas absorption (SOS_PROFIL.F:509-795) */
        double t_first, t_layer, zlim, tg_zlim, ttot_zlim, zing;
        int ing, j;
        const int strong = tabs[nblev - 1] > THRESHOLD_TAUABS;
        if (TCOUCHE > THRESHOLD_TAUABS) return -1;
        ttot = tr + ta + tabs[nblev - 1];
        if (strong) {
            i = 1;
            while (tabs[i - 1] < THRESHOLD_TAUABS) i++;
            const double alin = (tabs[i - 1] - tabs[i - 2]) / (altabs[i - 1] - altabs[i - 2]);
            const double blin = tabs[i - 1] - alin * altabs[i - 1];
            tg_zlim = THRESHOLD_TAUABS;
            zlim = (tg_zlim - blin) / alin;
            t_first = T_FIRST;
            ttot_zlim = ta * EXP(-zlim / ha) + tr * EXP(-zlim / hr) + tg_zlim;
            t_layer = (ttot_zlim - t_first) / (OS_NT - nt_ng - 2);
            INFO_BIN(0, 3); INFO_BIN(2, !(t_layer > TCOUCHE)); INFO_BINF(5, t_layer);
            t_layer = t_layer > TCOUCHE ? t_layer : TCOUCHE;
        } else {
            zlim = 0.; tg_zlim = tabs[nblev - 1];
            if ((ttot / OS_NT_MIN) <= T_FIRST) { nt = OS_NT_MIN; t_layer = ttot / nt; t_first = t_layer; INFO_BIN(0, 0); }
            else if ((ttot / OS_NT_MIN) < TCOUCHE) { nt = OS_NT_MIN + 1; t_first = T_FIRST; t_layer = (ttot - t_first) / OS_NT_MIN; INFO_BIN(0, 1); }
            else { t_first = T_FIRST; nt = (int)((ttot - t_first) / TCOUCHE); t_layer = (ttot - t_first) / nt; nt = nt + 1; INFO_BIN(0, 2); }
        }
        INFO_BIN(1, strong);
        INFO_BINF(0, zlim); INFO_BINF(1, t_first); INFO_BINF(2, t_layer); INFO_BINF(3, ttot); INFO_BINF(4, tabs[nblev - 1]);
        nt = 1; z = TOA_ALT; zing = z_ng[1];
        hmol[0] = 0.; haer[0] = 0.; habs[0] = 0.; h[0] = 0.;
        ing = 1;
        ttot_zlim = ta * EXP(-zlim / ha) + tr * EXP(-zlim / hr) + tg_zlim;
        while ((ttot_zlim - h[nt - 1]) > t_layer) {
            i = nt;
            if (i > OS_NT - 1) { INFO_BIN(10, 2); INFO_BIN(11, i); return -1; }   /* the Fortran would overrun its arrays here */
            if (i == 1) {
                dtau = 0.;
                steps = 0;
                while (dtau < t_first) {
                    z = z - DELTA_Z;
                    steps++;
                    j = seg_of(z, altabs, nblev);
                    if (z <= altabs[0]) {
                        const double zz = (z - altabs[j - 2]) / (altabs[j - 1] - altabs[j - 2]);
                        vg = (1 - zz) * tabs[j - 2] + zz * tabs[j - 1];
                    } else vg = 0.;
                    vr = tr * EXP(-z / hr); va = ta * EXP(-z / ha);
                    dtau = vr + va + vg;
                }
                zprof[1] = z; h[1] = dtau; ing = 1;
                INFO_BIN(3, steps);
            } else {
                z = disc(t_layer, ta, ha, tr, hr, tabs, altabs, nblev, h[i - 1], zprof[1], tg_zlim, zlim);
                INFO_LEV(0, i, g_disc_steps); INFO_LEV(1, i, g_disc_zero);
            }
            if (z <= zing) { z = zing; ing = ing + 1; zing = z_ng[ing]; INFO_LEV(2, i, 1); }
            else if ((z - zing) <= THRESHOLD_DZ) { ing = ing + 1; zing = z_ng[ing]; INFO_LEV(3, i, 1); }
            zprof[i] = z;
            j = seg_of(z, altabs, nblev);
            if (z > altabs[0]) vg = tabs[j - 2];
            else {
                const double zz = (z - altabs[j - 2]) / (altabs[j - 1] - altabs[j - 2]);
                vg = (1 - zz) * tabs[j - 2] + zz * tabs[j - 1];
            }
            vr = tr * EXP(-z / hr); va = ta * EXP(-z / ha);
            hmol[i] = vr; haer[i] = va; habs[i] = vg;
            h[i] = va + vr + vg;
            va = va - haer[i - 1]; vr = vr - hmol[i - 1]; vg = vg - habs[i - 1];
            pcaer[i] = va / (va + vr + vg); pcmol[i] = vr / (va + vr + vg);
            nt = nt + 1;
        }
        INFO_BIN(11, nt); INFO_BIN(6, ing);
        if ((zprof[nt - 1] - zlim) <= THRESHOLD_DZ) { nt = nt - 1; INFO_BIN(4, 1); INFO_BIN(5, nt - 1 == 0); }
        zprof[nt] = zlim;
        vr = tr * EXP(-zlim / hr); va = ta * EXP(-zlim / ha); vg = tg_zlim;
        hmol[nt] = vr; haer[nt] = va; habs[nt] = vg; h[nt] = vr + va + tg_zlim;
        va = va - haer[nt - 1]; vr = vr - hmol[nt - 1]; vg = vg - habs[nt - 1];
        pcaer[nt] = va / (va + vr + vg); pcmol[nt] = vr / (va + vr + vg);
        zprof[0] = TOA_ALT; pcaer[0] = pcaer[1]; pcmol[0] = pcmol[1];
        hmol[0] = 0.; haer[0] = 0.; habs[0] = 0.; h[0] = 0.;
        if (strong) {
            nt = nt + 1;
            if (nt > OS_NT) { INFO_BIN(10, 3); return -1; }
            hmol[nt] = tr; haer[nt] = ta; habs[nt] = tabs[nblev - 1];
            h[nt] = hmol[nt] + haer[nt] + habs[nt];
            vr = hmol[nt] - hmol[nt - 1]; va = haer[nt] - haer[nt - 1]; vg = habs[nt] - habs[nt - 1];
            pcaer[nt] = va / (va + vr + vg); pcmol[nt] = vr / (va + vr + vg);
            zprof[nt] = 0.;
        }
    }
    if (info && info->raw)
        for (i = 0; i <= nt; i++) {
            info->raw[i] = zprof[i]; info->raw[OS_NT + 2 + i] = h[i];
            info->raw[2 * (OS_NT + 2) + i] = pcaer[i]; info->raw[3 * (OS_NT + 2) + i] = pcmol[i];
        }
    /* PROFIL file round trip (write SOS_PROFIL.F:1084 format 20, read SOS.F:515 format 70) */
    for (i = 0; i <= nt; i++) {
        zprof[i] = rt_f10_5(zprof[i]); h[i] = rt_e15_8(h[i]); pcaer[i] = rt_e15_8(pcaer[i]); pcmol[i] = rt_e15_8(pcmol[i]);
    }
    *nt_out = nt;
    return 0;
}

int sos_profile_oracle(double tr, double hr, double ta, double ha, int absprofil, const double *altabs,
                       const double *tabs, int *nt_out, double *zprof, double *h, double *pcaer, double *pcmol)
{
    return profile_core(tr, hr, ta, ha, absprofil, ABS_NBLEV, altabs, tabs, nt_out, zprof, h, pcaer, pcmol, NULL);
}

/* The info form: the same statements for an absorption grid of nblev levels (2 <= nblev), plus what the run did.
 *   bin[12]  0 regime of the gas step (-1 no gas step, 0 / 1 / 2 the three T_FIRST / T_LAYER regimes, 3 strong absorption),
 *            1 strong, 2 the FMAX(T_LAYER, TCOUCHE) clamp was hit, 3 steps of the first-level scan, 4 last level dropped,
 *            5 ... with NT - 1 == 0, 6 final ING, 7 NT of the no-gas profile, 8 its regime, 9 steps of its first-level scan,
 *            10 where IER = -1 came from (0 none, 1 no-gas grid, 2 level loop, 3 strong-absorption ground level),
 *            11 level count when the loop ended (before the drop; the refused index for 10 = 2)
 *   binf[9]  0 ZLIM, 1 T_FIRST, 2 T_LAYER, 3 TTOT, 4 TGTOT, 5 T_LAYER before the clamp (strong), 6 TTOT, 7 T_FIRST and
 *            8 T_LAYER of the no-gas profile
 *   lev[4][OS_NT + 2]     per level of the gas step: bisection steps, stop on ZMOY == 0, forced no-gas level, near-DZ skip
 *   lev_ng[2][OS_NT + 2]  per level of the no-gas profile: bisection steps, stop on ZMOY == 0
 *   raw[4][OS_NT + 2]     Z, H, PCAER, PCMOL before the decimal round trip */
int sos_profile_oracle_info(double tr, double hr, double ta, double ha, int absprofil, int nblev, const double *altabs,
                            const double *tabs, int *nt_out, double *zprof, double *h, double *pcaer, double *pcmol,
                            int *bin, double *binf, int *lev, int *lev_ng, double *raw)
{
    prof_info info;
    info.bin = bin; info.binf = binf; info.lev = lev; info.lev_ng = lev_ng; info.raw = raw;
    if (tabs && nblev < 2) return -2;
    return profile_core(tr, hr, ta, ha, absprofil, tabs ? nblev : ABS_NBLEV, altabs, tabs, nt_out, zprof, h, pcaer, pcmol, &info);
}

/* SOS_ABSPROFILE (src/SOS_ABSPROFILE.F:325-371) for one bin: the optical depth of a layer is the sum over the eight gases, in
 * order, of XK RO; the transmission is the running product from the top; TAUABS(level) = -ln(TRS), or CTE_TAUABS_MAX = 999
 * (SOS.h:297) once the product has underflowed.  xk[8][nterm][nlev - 1], ro[8][nlev - 1], ik[8] 1-based (an index outside
 * 1..nterm takes the nearest term, as the device entry documents), tau[nlev]. */
void sos_absprofile_oracle(int nlev, int nterm, const int *ik, const double *xk, const double *ro, double *tau)
{
    const int nl1 = nlev - 1;
    double trs = 1.0;
    int j, k;
    tau[0] = 0.;
    for (j = 0; j < nl1; j++) {
        double t1c = 0.;
        for (k = 0; k < 8; k++) {
            int t = ik[k];
            t = t < 1 ? 1 : (t > nterm ? nterm : t);
            t1c = t1c + xk[((size_t)k * nterm + (t - 1)) * nl1 + j] * ro[(size_t)k * nl1 + j];
        }
        trs = trs * exp(-t1c);
        tau[j + 1] = trs > 0. ? -log(trs) : 999.;
    }
}
