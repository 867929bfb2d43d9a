// csrc/profile.hip -- per-bin atmospheric profile discretisation on the device (gfx950).
//
// Replaces, for every CKD bin of a wavelength at once, the step immediately before the solver:
//   SOS_PROFILE (IPROFIL = 1)  src/SOS_PROFIL.F:224-1170   gas step :509-795 (level placement by optical-depth steps,
//                                                            forced levels of the no-gas profile, limit layer for
//                                                            strong absorption), PROFIL file formats :1084,1150
//   SOS_DISC                   src/SOS_PROFIL.F:1210-1332  bisection on altitude
//   SOS (wrapper)              src/SOS.F:511-550           read-back of the PROFIL file, truncation rescale, IBORM
//                              src/SOS.F:567-589           TAUOUT / TTOT_TRONC; output level of SOS_OS.F:1514-1520
// The reference writes one PROFIL text file per bin and reads it back; here the profile goes straight into the
// device layout of sosgpu_os_solve and the text round trip (F10.5 / E15.8) is applied in registers, exactly.
//
// Work split: the no-gas profile (SOS_PROFIL.F:349-489) depends only on (TR,HR,TA,HA) -- identical for all bins of a
// wavelength -- and is computed once, by one wavefront (k_profile_nogas, queued in front of k_profile); the gas step depends
// on the bin's absorption profile and runs one wavefront per bin (the level loop is a serial recurrence: each level starts
// from the optical depth the previous bisection actually reached).  Latency/transcendental-bound: ~NT * 25 bisection steps * 2 exp per bin, no
// HBM traffic to speak of (50 doubles in, 4 * (NT+1) doubles out per bin).
#include <algorithm>
#include "sos_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "pow10_dd.h"
__device__ const double P10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                   1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// round(x * p) to the nearest integer (ties to even) where p is an exact power of ten: the product is formed exactly as
// hi + lo (one FMA), so the decision never sees the rounding error of the multiplication
__device__ __forceinline__ double round_scaled(double x, double p)
{
    const double hi = x * p;
    const double lo = __builtin_fma(x, p, -hi);
    double r = rint(hi);
    const double d = (hi - r) + lo;                  // exact: |hi - r| <= 0.5, lo tiny
    if (d > 0.5 || (d == 0.5 && fmod(r, 2.0) != 0.0)) r += 1.0;
    else if (d < -0.5 || (d == -0.5 && fmod(r, 2.0) != 0.0)) r -= 1.0;
    return r;
}

// av 10^m as hi + lo for |m| <= 308, to a relative 2^-104: the power of ten as a pair of doubles (pow10_dd.h), the product
// (m >= 0) or the quotient and its remainder (m < 0) by one FMA each
__device__ __forceinline__ void scaled_dd(double av, int m, double &hi, double &lo)
{
    if (m >= 0) {
        const double ph = P10DD[m][0], pl = P10DD[m][1];
        hi = av * ph;
        lo = __builtin_fma(av, ph, -hi) + av * pl;
    } else {
        const double ph = P10DD[-m][0], pl = P10DD[-m][1];
        hi = av / ph;
        lo = (__builtin_fma(-hi, ph, av) - hi * pl) / ph;
    }
}

// rt_e15_8 where 10^m is not one double (m > 22: |v| < 1e-15; m < -22: |v| >= 1e30).  From 1e-300 to 1e300 both steps are
// done on the pair: the eight digits are round(av 10^m) decided on hi + lo, the value read back is r 10^-m as hi + lo rounded
// once.  Neither step can meet an exact tie it would misjudge: av 10^m is never a half-integer here (5^23 > 2^53), and
// r 10^-m is exact as a pair wherever it can be a midpoint of doubles (10^k exact up to k = 44, no midpoint beyond).
// Outside that range (denormals, the last decades before overflow) one double stands for the power: the value read back may
// be the neighbour of the C library's.
__device__ double rt_e15_8_wide(double av, double v, int m)
{
    if ((m > 22 && m <= 307) || (m < -22 && m >= -301)) {
        double hi, lo;
        scaled_dd(av, m, hi, lo);                       // the log10 estimate may be one off: no exact comparison fixed it
        if (hi > 1e8 || (hi == 1e8 && lo >= 0.)) scaled_dd(av, --m, hi, lo);
        else if (hi < 1e7 || (hi == 1e7 && lo < 0.)) scaled_dd(av, ++m, hi, lo);
        double r = rint(hi);
        const double d = (hi - r) + lo;
        if (d > 0.5 || (d == 0.5 && fmod(r, 2.0) != 0.0)) r += 1.0;
        else if (d < -0.5 || (d == -0.5 && fmod(r, 2.0) != 0.0)) r -= 1.0;
        scaled_dd(r, -m, hi, lo);
        return copysign(hi + lo, v);
    }
    if (m < 0) {
        const double q = pow(10.0, (double)(-m - 22));
        const double r = rint(av / P10[22] / q);
        return copysign(r * q * P10[22], v);
    }
    const int ka = (m - 22) / 2, kb = (m - 22) - ka;    // 10^m would overflow: scale in three steps
    const double pa = pow(10.0, (double)ka), pb = pow(10.0, (double)kb);
    const double r = rint(av * P10[22] * pa * pb);
    return copysign(r / pb / pa / P10[22], v);
}

// value read back from a Fortran E15.8 field: 8 significant decimal digits, correctly rounded both ways
// (decimal -> binary is r / 10^m with r < 2^27 and 10^m exact: one correctly rounded division; where 10^m is not one double,
// rt_e15_8_wide)
__device__ double rt_e15_8(double v)
{
    if (v == 0.0 || !isfinite(v)) return v;
    const double av = fabs(v);
    int e = (int)floor(log10(av));
    // fix the estimate with exact comparisons where the powers are exact
    if (e >= 0 && e < 22) { if (av >= P10[e + 1]) e++; else if (av < P10[e]) e--; }
    else if (e < 0 && e >= -22) { if (av * P10[-e] < 1.0) e--; else if (e < -1 && av * P10[-e - 1] >= 1.0) e++; }
    const int m = 7 - e;                             // scale so that the integer has 8 digits
    double r;
    if (m >= 0 && m <= 22) {
        r = round_scaled(av, P10[m]);
        if (r >= 1e8) return copysign(r / P10[m], v);            // carried into the next decade: same value
        if (r < 1e7) {                                          // estimate one too high (only at exact powers of ten)
            r = round_scaled(av, P10[m] * 10.0);
            return copysign(r / (P10[m] * 10.0), v);
        }
        return copysign(r / P10[m], v);
    }
    if (m < 0) {                                     // |v| >= 1e8: divide
        const int k = -m;
        if (k <= 22) {
            // the quotient is rounded before rint sees it, which misplaces values on or next to a tie: decide on the
            // remainder av - r 10^k instead, which one FMA forms exactly (r < 2^27, 10^k exact, |remainder| <= 10^k)
            r = rint(av / P10[k]);
            const double rem = __builtin_fma(-r, P10[k], av), half = 0.5 * P10[k];
            if (rem > half || (rem == half && fmod(r, 2.0) != 0.0)) r += 1.0;
            else if (rem < -half || (rem == -half && fmod(r, 2.0) != 0.0)) r -= 1.0;
            return copysign(r * P10[k], v);
        }
        return rt_e15_8_wide(av, v, m);               // |v| >= 1e30
    }
    return rt_e15_8_wide(av, v, m);                   // |v| < 1e-15
}

__device__ __forceinline__ double rt_f10_5(double v) { return copysign(round_scaled(fabs(v), 1e5) / 1e5, v); }

struct GasProf {
    const double *alt, *tab;     // altitude grid (descending) and cumulative gas optical depth of the bin, in LDS
    int n;
    // index J of the absorption-profile segment holding altitude z: first J >= 2 with z >= ALTABS(J), i.e.
    // ALTABS(J-1) > z >= ALTABS(J) (SOS_PROFIL.F:694-697).  The reference scans J upwards; the grid is monotonic, so a
    // bisection returns the same J in 6 steps instead of up to 50 dependent loads.
    __device__ __forceinline__ int seg(double z) const
    {
        int lo = 2, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (z < alt[mid - 1]) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
};

// SOS_DISC (SOS_PROFIL.F:1260-1325)
__device__ double disc(double dt, double ta, double ha, double tr, double hr, const GasProf &g, double tim1,
                       double zmax_init, double tg_zlim, double zlim)
{
    const double ti = tim1 + dt;
    double zmax = zmax_init, zmin = zlim, zmoy;
    for (int guard = 0; guard < 4096; guard++) {
        double tg;
        zmoy = (zmax + zmin) / 2.;
        if (tg_zlim > 0.0) {
            const int j = g.seg(zmoy);
            double zz;
            if (zmoy > g.alt[0]) zz = 0;
            else zz = (zmoy - g.alt[j - 2]) / (g.alt[j - 1] - g.alt[j - 2]);
            tg = (1 - zz) * g.tab[j - 2] + zz * g.tab[j - 1];
        } else tg = 0.0;
        const double tzmoy = ta * exp(-zmoy / ha) + tr * exp(-zmoy / hr) + tg;
        const double xd = fabs(ti - tzmoy);
        if (xd < (double).000001f) break;
        if (zmoy == 0.0) break;
        if ((ti - tzmoy) < 0.0) zmin = zmoy; else zmax = zmoy;
    }
    return zmoy;
}

// SOS_DISC by the 64 lanes of a wavefront: the same bisection, six of its steps per evaluation.  The bisection visits a path
// in the binary tree of brackets below [zmin, zmax]; lane n = 1..63 takes heap node n of the six-level subtree under the
// current bracket, walks to it with the reference's own midpoint statement (so its ZMOY is bit for bit the one the serial loop
// would form on that path), and evaluates the optical depth there -- the 2 exponentials and the gas-profile lookup that make a
// serial step ~1000 cycles.  The comparison and stop results of all nodes are two wave masks; the path through them is resolved
// with scalar bit tests.  25-30 serial evaluations per level become 5 rounds.
__device__ __forceinline__ double lane_read(double v, int lane)
{
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], lane);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], lane);
    return u.d;
}

__device__ double disc_wave(double dt, double ta, double ha, double tr, double hr, const GasProf &g, double tim1,
                            double zmax_init, double tg_zlim, double zlim)
{
    const double ti = tim1 + dt;
    const int lane = threadIdx.x & 63;
    const int node = lane ? lane : 1;                        // lane 0 shadows the root (its results are not used)
    const int depth = 31 - __builtin_clz(node);              // 0..5
    double zmax = zmax_init, zmin = zlim, zres = 0.;
    for (int round = 0; round < 683; round++) {              // 683 x 6 >= the 4096 evaluations of the serial guard
        double lo = zmin, hi = zmax, zmoy = (hi + lo) / 2.;
        for (int k = depth - 1; k >= 0; --k) {               // the path to this lane's node: bit set = "ZMIN = ZMOY" was taken
            if ((node >> k) & 1) lo = zmoy; else hi = zmoy;
            zmoy = (hi + lo) / 2.;
        }
        double tg;
        if (tg_zlim > 0.0) {
            const int j = g.seg(zmoy);
            double zz;
            if (zmoy > g.alt[0]) zz = 0;
            else zz = (zmoy - g.alt[j - 2]) / (g.alt[j - 1] - g.alt[j - 2]);
            tg = (1 - zz) * g.tab[j - 2] + zz * g.tab[j - 1];
        } else tg = 0.0;
        const double tzmoy = ta * exp(-zmoy / ha) + tr * exp(-zmoy / hr) + tg;
        const double xd = fabs(ti - tzmoy);
        const bool stop = xd < (double).000001f || zmoy == 0.0;
        const bool up = (ti - tzmoy) < 0.0;                  // ZMIN = ZMOY
        const unsigned long long sm = __ballot(stop), um = __ballot(up);
        int n = 1;
        bool found = false;
        for (int d = 0; d < 6; d++) {
            if ((sm >> n) & 1ull) { found = true; break; }
            if (d == 5) break;
            n = 2 * n + (int)((um >> n) & 1ull);
        }
        n = __builtin_amdgcn_readfirstlane(n);
        zres = lane_read(zmoy, n);
        if (found) return zres;
        // six steps taken without a stop: the bracket below node n (a node of the last level)
        const double lo_n = lane_read(lo, n), hi_n = lane_read(hi, n);
        if ((um >> n) & 1ull) { zmin = zres; zmax = hi_n; } else { zmin = lo_n; zmax = zres; }
    }
    return zres;
}

// The first level below the top of the atmosphere (SOS_PROFIL.F:424-433 without gas, :601-624 with): Z = Z - DELTA_Z from Z0
// until the optical depth above Z reaches T_FIRST -- ~1700 steps of two exponentials each down to 35 km, the reference's serial
// scan, and half of the time this file's kernels took.  By the 64 lanes of a wavefront: a block of 64 consecutive steps at a
// time, lane l forming ITS altitude by the same l + 1 subtractions the serial loop makes (so it is bit for bit the loop's
// value) and evaluating the optical depth there; the first lane whose depth is not below T_FIRST is where the loop stops.
template <bool GAS>
__device__ double scan_first_wave(double tr, double hr, double ta, double ha, const GasProf &g, double t_first, double z0,
                                  double delta_z)
{
    const int lane = threadIdx.x & 63;
    double zbase = z0;
    for (int blk = 0; blk < 65536; blk++) {                  // (the serial loop has no guard either: TAU(Z) reaches T_FIRST or Z = -inf)
        double z = zbase;
        for (int j = 0; j <= lane; j++) z = z - delta_z;     // lane l: step blk * 64 + l + 1 of the serial loop
        double dtau;
        if (GAS) {
            double vg;
            const int j = g.seg(z);
            if (z <= g.alt[0]) {
                const double zz = (z - g.alt[j - 2]) / (g.alt[j - 1] - g.alt[j - 2]);
                vg = (1 - zz) * g.tab[j - 2] + zz * g.tab[j - 1];
            } else vg = 0.;
            const double vr = tr * exp(-z / hr), va = ta * exp(-z / ha);
            dtau = vr + va + vg;
        } else dtau = tr * exp(-z / hr) + ta * exp(-z / ha);
        const unsigned long long stop = __ballot(!(dtau < t_first));
        if (stop) return lane_read(z, __builtin_ctzll(stop));
        zbase = lane_read(z, 63);
    }
    return zbase;
}

}  // namespace

// The no-gas profile of the wavelength (SOS_PROFIL.F:349-489): level altitudes by equal optical-depth steps of molecules +
// aerosols, the shares of the two in every layer.  One wavefront, all lanes in lockstep on the same values (stores of one
// instruction go to one address), SOS_DISC by the 64 lanes (disc_wave).  Rounds 1-2 ran this loop on the host inside
// sosgpu_profile -- NT x 25 bisection steps x 2 exp, 0.3-0.4 ms of every wavelength of a spectrum plus a waited-for upload;
// the level count and the two steps are closed forms of (TR, TA) and stay there (api_atmosphere.hip, profile_nogas_grid).
//   z, h, pca, pcm [nt + 1]: altitude, cumulative optical depth, aerosol and molecular share of the layer ending at the level
// (the body is shared by k_profile_nogas and the table form k_profile_nogas_table: one statement sequence, one result)
__device__ __forceinline__ void profile_nogas_body(double tr, double hr, double ta, double ha, int nt, double t_first,
                                                   double t_layer, double *__restrict__ z, double *__restrict__ h,
                                                   double *__restrict__ pca, double *__restrict__ pcm)
{
    const double TOA = 120.0, DELTA_Z = (double)0.05f;
    if (ta == 0.0) {                                             // molecules only: closed form (SOS_PROFIL.F:367-392)
        for (int i = threadIdx.x; i <= nt; i += 64) {
            const double hm = i == 0 ? 0. : (i == 1 ? t_first : (i - 1) * t_layer + t_first);
            pcm[i] = 1.; pca[i] = 0.;
            z[i] = i == 0 ? TOA : hr * log(tr / hm);
            h[i] = hm + 0.;
        }
        return;
    }
    GasProf g;
    g.n = 0; g.alt = nullptr; g.tab = nullptr;                   // (never read: TG_ZLIM = 0 below)
    double zz = scan_first_wave<false>(tr, hr, ta, ha, g, t_first, TOA, DELTA_Z);
    const double dtau = tr * exp(-zz / hr) + ta * exp(-zz / ha);
    double vr = tr * exp(-zz / hr), va = ta * exp(-zz / ha);
    double hmol_p = vr, haer_p = va;
    const double z1 = zz;
    z[0] = TOA; h[0] = 0.;
    z[1] = zz; h[1] = vr + va;
    pcm[1] = vr / dtau; pca[1] = va / dtau;
    pcm[0] = pcm[1]; pca[0] = pca[1];
    double hprev = dtau;
    for (int i = 2; i <= nt - 1; i++) {
        zz = disc_wave(t_layer, ta, ha, tr, hr, g, hprev, z1, 0.0, 0.0);
        z[i] = zz;
        vr = tr * exp(-zz / hr); va = ta * exp(-zz / ha);
        const double hm = vr, hae = va;
        hprev = vr + va;
        h[i] = hprev;
        vr = vr - hmol_p; va = va - haer_p;
        pcm[i] = vr / (vr + va); pca[i] = va / (vr + va);
        hmol_p = hm; haer_p = hae;
    }
    z[nt] = 0.; h[nt] = tr + ta;
    vr = tr - hmol_p; va = ta - haer_p;
    pcm[nt] = vr / (vr + va); pca[nt] = va / (vr + va);
}

__global__ __launch_bounds__(64) void k_profile_nogas(double tr, double hr, double ta, double ha, int nt, double t_first,
                                                      double t_layer, double *__restrict__ z, double *__restrict__ h,
                                                      double *__restrict__ pca, double *__restrict__ pcm)
{
    profile_nogas_body(tr, hr, ta, ha, nt, t_first, t_layer, z, h, pca, pcm);
}

// Table form: one wavefront per WAVELENGTH of a part of a spectrum, its (TR, HR, TA, HA) and grid from the device table, its
// block at ng + w * 4 * ngl.  A wavelength the host refused (nt_ng < 1) writes nothing.
__global__ __launch_bounds__(64) void k_profile_nogas_table(const ProfileWl *__restrict__ tab, int nwl, double *__restrict__ ng, int ngl)
{
    const int w = blockIdx.x;
    if (w >= nwl) return;
    const ProfileWl &t = tab[w];
    if (t.nt_ng < 1 || t.nt_ng >= ngl) return;
    double *z = ng + (size_t)w * 4 * ngl;
    profile_nogas_body(t.tr, t.hr, t.ta, t.ha, t.nt_ng, t.t_first, t.t_layer, z, z + ngl, z + 2 * ngl, z + 3 * ngl);
}

void launch_profile_nogas_table(const ProfileWl *d_tab, int nwl, double *d_ng, int ngl, hipStream_t st)
{
    k_profile_nogas_table<<<nwl, 64, 0, st>>>(d_tab, nwl, d_ng, ngl);
}

void launch_profile_nogas(double tr, double hr, double ta, double ha, int nt, double t_first, double t_layer, double *d_ng, int ng,
                          hipStream_t st)
{
    k_profile_nogas<<<1, 64, 0, st>>>(tr, hr, ta, ha, nt, t_first, t_layer, d_ng, d_ng + ng, d_ng + 2 * ng, d_ng + 3 * ng);
}

// One thread per bin, `bpw` bins per wavefront.  The work of a bin is a long serial chain (latency-bound) and very ragged
// (NT 100...600, bisection depth varies), so a wavefront is deliberately left mostly EMPTY: with few bins per wave the
// batch spreads over all 1024 SIMDs and a wave only waits for the slowest of its few bins.
// prof[b][3][lp] <- H, XDEL, YDEL (after the rescale), zprof[b][lp], nt, iborm, jout, zz, hvrai[b][lp] <- H before the rescale (if asked for),
// scal[b][4] = {0, TTOT_TRONC, TTOT_VRAI, TAUOUT}; nt[b] = -1 flags a profile that does not fit (IER of the reference).
// WAVE = true (the form launched): ONE WAVEFRONT per bin.  All 64 lanes run the bin's level loop in lockstep on the same
// values (stores of one instruction go to one address) and share the work where the time is: SOS_DISC (disc_wave).  A single
// bin takes 6.5-9.7 ms with one lane (most of the latency of a 25-bin sos_proc call) and 2.3-2.9 ms this way; 4096 bins 24.8 -> 3.8-5.3 ms.
// (the body of bin b, shared by k_profile and the table form k_profile_table: s_alt / s_tab are the caller's LDS blocks)
template <bool WAVE>
__device__ __forceinline__ void profile_bin_body(const ProfileArgs &a, const int b, double *s_alt, double *s_tab_slot)
{
    const double TCOUCHE = (double)0.005f, T_FIRST = (double)0.0002f, DELTA_Z = (double)0.05f, DZ = (double)0.001f;
    const double TAUABS_MAX = 1.5, TOA = 120.0;
    const int OS_NT = 600, OS_NT_MIN = 100;
    const double tr = a.tr, hr = a.hr, ta = a.ta, ha = a.ha;
    double *H = a.prof + (size_t)b * 3 * a.lp, *XD = H + a.lp, *YD = XD + a.lp;
    double *Z = a.zprof + (size_t)b * a.lp;
    double *HV = a.hvrai ? a.hvrai + (size_t)b * a.lp : nullptr;     // untruncated depth row of the bin (or none)
    // the bin's absorption profile is read thousands of times: keep it (and the altitude grid) in LDS
    GasProf g;
    g.n = a.nblev; g.alt = s_alt; g.tab = nullptr;
    if (a.tabs) {
        for (int i = 0; i < a.nblev; i++) { s_tab_slot[i] = a.tabs[(size_t)b * a.nblev + i]; s_alt[i] = a.altabs[i]; }
        g.tab = s_tab_slot;
    }
    const double tgtot = g.tab ? g.tab[a.nblev - 1] : 0.0;
    int nt;
    bool bad = a.nt_ng < 1 || a.nt_ng > OS_NT || a.nt_ng >= a.lp;

    if (bad) {
        nt = 0;
    } else if (a.absprofil == 7 || tgtot == 0.0) {                    // SOS_PROFIL.F:492-508
        nt = a.nt_ng;
        for (int i = 0; i <= nt; i++) { Z[i] = a.z_ng[i]; H[i] = a.h_ng[i]; XD[i] = a.pca_ng[i]; YD[i] = a.pcm_ng[i]; }
    } else {
        // ---- profile with gas absorption (SOS_PROFIL.F:509-795); Hmol/Haer/Habs of the previous level in registers
        const bool strong = tgtot > TAUABS_MAX;
        double t_first, t_layer, zlim, tg_zlim, ttot_zlim;
        const double ttot = tr + ta + tgtot;
        if (strong) {
            int i = 1;
            while (g.tab[i - 1] < TAUABS_MAX) i++;
            const double alin = (g.tab[i - 1] - g.tab[i - 2]) / (g.alt[i - 1] - g.alt[i - 2]);
            const double blin = g.tab[i - 1] - alin * g.alt[i - 1];
            tg_zlim = TAUABS_MAX;
            zlim = (tg_zlim - blin) / alin;
            t_first = T_FIRST;
            ttot_zlim = ta * exp(-zlim / ha) + tr * exp(-zlim / hr) + tg_zlim;
            t_layer = (ttot_zlim - t_first) / (OS_NT - a.nt_ng - 2);
            t_layer = fmax(t_layer, TCOUCHE);
        } else {
            zlim = 0.; tg_zlim = tgtot;
            if ((ttot / OS_NT_MIN) <= T_FIRST) { t_layer = ttot / OS_NT_MIN; t_first = t_layer; }
            else if ((ttot / OS_NT_MIN) < TCOUCHE) { t_first = T_FIRST; t_layer = (ttot - t_first) / OS_NT_MIN; }
            else { t_first = T_FIRST; const int n0 = (int)((ttot - t_first) / TCOUCHE); t_layer = (ttot - t_first) / n0; }
        }
        nt = 1;
        double z = TOA, zing = a.z_ng[1];
        double hmol_p = 0., haer_p = 0., habs_p = 0., h_p = 0.;   // level nt-1
        int ing = 1;
        ttot_zlim = ta * exp(-zlim / ha) + tr * exp(-zlim / hr) + tg_zlim;
        H[0] = 0.;
        while ((ttot_zlim - h_p) > t_layer) {
            const int i = nt;
            if (i > OS_NT - 1 || i >= a.lp - 1) { bad = true; break; }
            double vr, va, vg;
            if (i == 1 && WAVE) {
                z = scan_first_wave<true>(tr, hr, ta, ha, g, t_first, z, DELTA_Z);
                ing = 1;
            } else if (i == 1) {
                double dtau = 0.;
                while (dtau < t_first) {
                    z = z - DELTA_Z;
                    const int j = g.seg(z);
                    if (z <= g.alt[0]) {
                        const double zz = (z - g.alt[j - 2]) / (g.alt[j - 1] - g.alt[j - 2]);
                        vg = (1 - zz) * g.tab[j - 2] + zz * g.tab[j - 1];
                    } else vg = 0.;
                    vr = tr * exp(-z / hr); va = ta * exp(-z / ha);
                    dtau = vr + va + vg;
                }
                ing = 1;
            } else {
                z = WAVE ? disc_wave(t_layer, ta, ha, tr, hr, g, h_p, Z[1], tg_zlim, zlim)
                         : disc(t_layer, ta, ha, tr, hr, g, h_p, Z[1], tg_zlim, zlim);
            }
            if (z <= zing) { z = zing; ing = ing + 1; zing = a.z_ng[min(ing, a.nt_ng)]; }
            else if ((z - zing) <= DZ) { ing = ing + 1; zing = a.z_ng[min(ing, a.nt_ng)]; }
            Z[i] = z;
            const int j = g.seg(z);
            if (z > g.alt[0]) vg = g.tab[j - 2];
            else {
                const double zz = (z - g.alt[j - 2]) / (g.alt[j - 1] - g.alt[j - 2]);
                vg = (1 - zz) * g.tab[j - 2] + zz * g.tab[j - 1];
            }
            vr = tr * exp(-z / hr); va = ta * exp(-z / ha);
            const double hm = vr, hae = va, hab = vg;
            h_p = va + vr + vg;
            H[i] = h_p;
            va = va - haer_p; vr = vr - hmol_p; vg = vg - habs_p;
            XD[i] = va / (va + vr + vg); YD[i] = vr / (va + vr + vg);
            hmol_p = hm; haer_p = hae; habs_p = hab;
            nt = nt + 1;
        }
        if (!bad) {
            // limit level (ground, or the altitude where the gas optical depth reaches the threshold)
            double hmol_q = hmol_p, haer_q = haer_p, habs_q = habs_p;      // level nt-1 ...
            if ((Z[nt - 1] - zlim) <= DZ) {
                // the last computed level is dropped: level nt-1 is the one before it -- recompute its parts from Z
                nt = nt - 1;
                const double zq = Z[nt - 1];
                if (nt - 1 == 0) { hmol_q = 0.; haer_q = 0.; habs_q = 0.; }
                else {
                    hmol_q = tr * exp(-zq / hr); haer_q = ta * exp(-zq / ha);
                    const int j = g.seg(zq);
                    if (zq > g.alt[0]) habs_q = g.tab[j - 2];
                    else {
                        const double zz = (zq - g.alt[j - 2]) / (g.alt[j - 1] - g.alt[j - 2]);
                        habs_q = (1 - zz) * g.tab[j - 2] + zz * g.tab[j - 1];
                    }
                }
            }
            Z[nt] = zlim;
            double vr = tr * exp(-zlim / hr), va = ta * exp(-zlim / ha), vg = tg_zlim;
            const double hm = vr, hae = va, hab = vg;
            H[nt] = vr + va + tg_zlim;
            va = va - haer_q; vr = vr - hmol_q; vg = vg - habs_q;
            XD[nt] = va / (va + vr + vg); YD[nt] = vr / (va + vr + vg);
            Z[0] = TOA; XD[0] = XD[1]; YD[0] = YD[1]; H[0] = 0.;
            if (strong) {
                nt = nt + 1;
                if (nt > OS_NT || nt >= a.lp) bad = true;
                else {
                    H[nt] = (tr + ta) + tgtot;
                    vr = tr - hm; va = ta - hae; vg = tgtot - hab;
                    XD[nt] = va / (va + vr + vg); YD[nt] = vr / (va + vr + vg);
                    Z[nt] = 0.;
                }
            }
        }
    }
    if (bad) {
        a.nt[b] = -1; a.iborm[b] = 0;
        if (a.jout) { a.jout[b] = 0; a.zz[b] = 0.; }
        for (int k = 0; k < 4; k++) a.scal[4 * b + k] = 0.;
        return;
    }
    // PROFIL file round trip (SOS_PROFIL.F:1084 format 20 -> SOS.F:515 format 70)
    // (WAVE: the independent per-level passes are dealt to the lanes, level i to lane i mod 64; the barrier of the one-wave
    //  block makes the stores of the other lanes visible to the serial passes that follow)
    const int i0 = WAVE ? (int)(threadIdx.x & 63) : 0, di = WAVE ? 64 : 1;
    if (WAVE) __syncthreads();
    for (int i = i0; i <= nt; i += di) { Z[i] = rt_f10_5(Z[i]); H[i] = rt_e15_8(H[i]); XD[i] = rt_e15_8(XD[i]); YD[i] = rt_e15_8(YD[i]); }
    // H as the reference reads it back, before the rescale below overwrites it: the untruncated cumulative depth (HV[nt] = TTOT_VRAI)
    if (HV) for (int i = i0; i <= nt; i += di) HV[i] = H[i];
    if (WAVE) __syncthreads();
    const double ttot_vrai = H[nt];
    // truncation rescale (SOS.F:521-543) and IBORM (:549-550)
    bool lta = true;
    if (a.a_tronc != 0.) {
        double htr_p = H[0], h_prev = H[0];
        for (int i = 1; i <= nt; i++) {
            const double dh = H[i] - h_prev;
            h_prev = H[i];
            const double va = XD[i] * dh;
            const double vatr = va * (1 - a.piz * 0.5 * a.a_tronc);
            const double vr = YD[i] * dh;
            const double vg = (1 - XD[i] - YD[i]) * dh;
            const double htr = (vatr + vr + vg) + htr_p;
            XD[i] = vatr / (vatr + vr + vg);
            YD[i] = vr / (vatr + vr + vg);
            H[i] = htr;
            htr_p = htr;
        }
    }
    if (WAVE) __syncthreads();
    for (int i = i0; i <= nt; i += di) { XD[i] = XD[i] * a.piztr; if (XD[i] != 0.) lta = false; }
    if (WAVE) lta = !__any(!lta);
    for (int i = nt + 1 + i0; i < a.lp; i += di) { H[i] = 0.; XD[i] = 0.; YD[i] = 0.; Z[i] = 0.; }
    if (HV) for (int i = nt + 1 + i0; i < a.lp; i += di) HV[i] = 0.;
    if (WAVE) __syncthreads();
    a.nt[b] = nt;
    a.iborm[b] = lta ? min(2, a.smax) : a.smax;
    double tauout = H[0];
    if (a.jout) {
        int j = 0;
        double zz = 0.;
        if (a.zout != -1.0) {                                              // SOS.F:570-582, SOS_OS.F:1514-1520
            j = 1;
            while (j < nt && a.zout < Z[j]) j++;
            zz = (a.zout - Z[j - 1]) / (Z[j] - Z[j - 1]);
            tauout = (1 - zz) * H[j - 1] + zz * H[j];
        }
        a.jout[b] = j; a.zz[b] = zz;
    }
    a.scal[4 * b + 0] = 0.;
    a.scal[4 * b + 1] = H[nt];           // TTOT_TRONC
    a.scal[4 * b + 2] = ttot_vrai;       // TTOT_VRAI
    a.scal[4 * b + 3] = tauout;
}

template <bool WAVE>
__global__ __launch_bounds__(64) void k_profile(ProfileArgs a, int bpw)
{
    if (!WAVE && (int)threadIdx.x >= bpw) return; // no barrier below: every thread only touches its own LDS slice
    const int b = WAVE ? (int)blockIdx.x : blockIdx.x * bpw + threadIdx.x;
    const int slot = WAVE ? 0 : (int)threadIdx.x;
    if (b >= a.nb) return;
    __shared__ double s_alt[SOS_PROF_NBLEV_MAX];
    __shared__ double s_tab[WAVE ? 1 : 64][SOS_PROF_NBLEV_MAX + 1];     // +1: odd stride, lanes on different banks
    profile_bin_body<WAVE>(a, b, s_alt, s_tab[slot]);
}

// Table form: one wavefront per bin of ALL wavelengths of a part of a spectrum.  The wavefront reads the index of its
// wavelength and forms, from that wavelength's table entry, the ProfileArgs the per-wavelength launch gets as its kernel
// argument -- with the output arrays of the whole part, so that bin b of the part is bin b of the body.  A wavelength without
// gas (nterm 0) is a one-bin wavelength with tabs = null; jout / zz are written for wavelengths with zout != -1 only.
__global__ __launch_bounds__(64) void k_profile_table(ProfileTableArgs q)
{
    const int b = blockIdx.x;
    if (b >= q.nb) return;
    const int w = q.wl_of_bin[b];
    if (w < 0 || w >= q.nwl) return;
    const ProfileWl &t = q.tab[w];
    const bool gas = t.nterm > 0;
    const double *ngp = q.nogas + (size_t)w * 4 * q.ngl;
    ProfileArgs a;
    a.nb = q.nb; a.lp = q.lp; a.nblev = gas ? q.nblev : 0; a.absprofil = gas ? t.absprofil : 7; a.smax = t.smax; a.nt_ng = t.nt_ng;
    a.tr = t.tr; a.hr = t.hr; a.ta = t.ta; a.ha = t.ha; a.a_tronc = t.a_tronc; a.piz = t.piz; a.piztr = t.piztr; a.zout = t.zout;
    a.altabs = gas ? q.gas + t.alt_off : nullptr; a.tabs = gas ? q.tabs : nullptr;
    a.z_ng = ngp; a.h_ng = ngp + q.ngl; a.pca_ng = ngp + 2 * q.ngl; a.pcm_ng = ngp + 3 * q.ngl;
    a.prof = q.prof; a.zprof = q.zprof; a.scal = q.scal; a.nt = q.nt; a.iborm = q.iborm; a.hvrai = q.hvrai;
    const bool lev = t.zout != -1.0 && q.jout;
    a.jout = lev ? q.jout : nullptr; a.zz = lev ? q.zz : nullptr;
    __shared__ double s_alt[SOS_PROF_NBLEV_MAX];
    __shared__ double s_tab[SOS_PROF_NBLEV_MAX + 1];
    profile_bin_body<true>(a, b, s_alt, s_tab);
}

void launch_profile_table(const ProfileTableArgs &q, hipStream_t st)
{
    k_profile_table<<<q.nb, 64, 0, st>>>(q);
}

void launch_profile(const ProfileArgs &a, hipStream_t st)
{
    // one wavefront per bin; SOSGPU_PROFILE_LANES=1: the one-lane-per-bin form (about 2048 wavefronts whatever the batch size)
    const char *e = getenv("SOSGPU_PROFILE_LANES");
    if (e && atoi(e)) {
        const int bpw = std::min(64, std::max(1, (a.nb + 2047) / 2048));
        k_profile<false><<<(a.nb + bpw - 1) / bpw, 64, 0, st>>>(a, bpw);
    } else k_profile<true><<<a.nb, 64, 0, st>>>(a, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// SOS_PROFILE for IPROFIL = 2 (SOS_PROFIL.F:800-946): a homogeneous layer of aerosols and molecules between ZMIN and ZMAX
// inside a molecular atmosphere, no gas.  Three zones of sublayers -- c1 of equal molecular depth above ZMAX + 10 m, c2 of equal
// height inside the layer, c3 of equal molecular depth below ZMIN - 10 m (none for a layer on the ground) -- whose counts are
// closed forms the host evaluates (sosgpu_profile_layer_grid).  The reference's recurrence Hmol(I) = Hmol(I-1) + VR_SC starts
// from an Hmol(0) it assigns afterwards; as on a fresh stack, it starts from 0 here.
// One wavefront.  The serial chains keep the reference's order, all lanes in lockstep on the same values (stores of one
// instruction go to one address): the repeated sums of zones 1 and 3, Z = Z - DELTA_Z through the layer, Haer(I) = Haer(I-1) + ...
// What depends on one level alone -- the exponential of a level of the layer, the aerosol increment, the closing pass with its
// logarithm and shares -- is dealt to the lanes, level i to lane i mod 64.
//   z, h, pca, pcm [nt + 1]: the block profile_bin_body takes in place of the no-gas profile;  hm, ha [nt + 1]: Hmol, Haer
// (all six rows in LDS; z and h carry the layer's altitudes and increments until the closing pass overwrites them)
// ---------------------------------------------------------------------------------------------------------------------
#define SOS_LAYER_ROW 601         // CTE_OS_NT + 1 levels
__device__ __forceinline__ void profile_layer_body(double tr, double hr, double ta, double zmin, double zmax, int nt, int c1, int c2,
                                                   int c3, double *z, double *h, double *pca, double *pcm, double *hm, double *ha)
{
    const double TOA = 120.0, DZT = (double)0.010f;                  // CTE_DZTRANSI
    const int lane = threadIdx.x & 63;
    const int i1 = c1 + 1, i2 = c1 + c2 + 1, i3 = c1 + c2 + 2;       // top and bottom level of the layer, level at ZMIN - 10 m
    const double vr_c1 = tr * exp(-(zmax + DZT) / hr);
    const double vr_c2 = tr * (exp(-zmin / hr) - exp(-(zmax + DZT) / hr));
    hm[0] = 0.; ha[0] = 0.;
    double vr_sc = vr_c1 / c1, acc = 0.;
    for (int i = 1; i <= c1; i++) { acc = acc + vr_sc; hm[i] = acc; }
    hm[i1] = tr * exp(-zmax / hr);
    const double delta_z = (zmax - zmin) / c2;
    double zc = zmax;
    for (int i = i1 + 1; i <= i2; i++) { zc = zc - delta_z; z[i] = zc; }
    if (zmin != 0.0) {
        const double vr_c3 = tr * (1.0 - exp(-(zmin - DZT) / hr));
        acc = tr * exp(-(zmin - DZT) / hr);
        hm[i3] = acc;
        vr_sc = vr_c3 / c3;
        for (int i = i3 + 1; i <= nt; i++) { acc = vr_sc + acc; hm[i] = acc; }
    }
    __syncthreads();
    for (int i = i1 + 1 + lane; i <= i2; i += 64) hm[i] = tr * exp(-z[i] / hr);
    __syncthreads();
    for (int i = i1 + lane; i <= i2; i += 64) h[i] = ta * (hm[i] - hm[i - 1]) / vr_c2;
    __syncthreads();
    for (int i = 1; i <= c1; i++) ha[i] = 0.;
    acc = 0.;
    for (int i = i1; i <= i2; i++) { acc = acc + h[i]; ha[i] = acc; }
    for (int i = i3; i <= nt; i++) ha[i] = acc;
    __syncthreads();
    for (int i = lane; i <= nt; i += 64) {
        if (i == 0) {
            z[0] = TOA; h[0] = tr * exp(-TOA / hr) + ha[0];          // Hmol(0), assigned after the chains: H(0) != 0
            pca[0] = 0.; pcm[0] = 1.;
            continue;
        }
        h[i] = hm[i] + ha[i];
        z[i] = hr * log(tr / hm[i]);
        if (ha[i] == ha[i - 1]) { pca[i] = 0.; pcm[i] = 1.; }
        else { const double ym = 1 / (1 + (ta / vr_c2)); pcm[i] = ym; pca[i] = 1 - ym; }
    }
    __syncthreads();
}

// The bin of one layer profile, shared by the single form (the entry as a kernel argument) and the table form (the entry of
// bin b): the block above, then the no-gas branch of profile_bin_body on it -- round trip, hvrai, rescale, IBORM, output level,
// scal -- with the layer's NT in place of nt_ng.  An entry whose counts do not add up to its NT, or whose NT does not fit the
// rows, makes no block and comes back flagged (nt = -1), as a no-gas profile that does not fit lp.
__global__ __launch_bounds__(64) void k_profile_layer(LayerArgs q)
{
    const int b = blockIdx.x;
    if (b >= q.nb) return;
    const LayerWl &t = q.tab ? q.tab[b] : q.one;
    __shared__ double rows[6][SOS_LAYER_ROW];
    const int nb_tr = t.zmin == 0.0 ? 1 : 2;
    const bool grid_ok = t.c1 >= 1 && t.c2 >= 1 && (nb_tr == 1 ? t.c3 == 0 : t.c3 >= 1) && t.nt == nb_tr + t.c1 + t.c2 + t.c3 &&
                         t.nt < SOS_LAYER_ROW;
    const bool fits = grid_ok && t.nt < q.lp;
    if (fits) profile_layer_body(t.tr, t.hr, t.ta, t.zmin, t.zmax, t.nt, t.c1, t.c2, t.c3, rows[0], rows[1], rows[2], rows[3], rows[4], rows[5]);
    ProfileArgs a;
    a.nb = q.nb; a.lp = q.lp; a.nblev = 0; a.absprofil = 7; a.smax = t.smax; a.nt_ng = grid_ok ? t.nt : -1;
    a.tr = t.tr; a.hr = t.hr; a.ta = t.ta; a.ha = 1.; a.a_tronc = t.a_tronc; a.piz = t.piz; a.piztr = t.piztr; a.zout = t.zout;
    a.altabs = nullptr; a.tabs = nullptr;
    a.z_ng = rows[0]; a.h_ng = rows[1]; a.pca_ng = rows[2]; a.pcm_ng = rows[3];
    a.prof = q.prof; a.zprof = q.zprof; a.scal = q.scal; a.nt = q.nt; a.iborm = q.iborm; a.hvrai = q.hvrai;
    const bool lev = t.zout != -1.0 && q.jout;
    a.jout = lev ? q.jout : nullptr; a.zz = lev ? q.zz : nullptr;
    profile_bin_body<true>(a, b, nullptr, nullptr);
}

void launch_profile_layer(const LayerArgs &q, hipStream_t st)
{
    k_profile_layer<<<q.nb, 64, 0, st>>>(q);
}

// ---------------------------------------------------------------------------------------------------------------------
// SOS_ABSPROFILE (src/SOS_ABSPROFILE.F:325-371) for every CKD bin of a wavelength: the absorption coefficient XK of a gas
// depends on the gas, on the exponential term chosen for it and on the layer only, so the host tabulates
// xk[gas][term][layer] (COEFF_ABS_CKD, SOS_SUB_TRS.F:171) once and a bin is one term index per gas.  Per bin, exactly the
// reference's loop: layer optical depth = sum over the eight gases (in order) of XK RO, transmission accumulated from the
// top, TAUABS(level) = -ln(TRS) or CTE_TAUABS_MAX when the transmission underflows.
// ---------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
// One WAVEFRONT per bin (round 3; one thread per bin before: 49 dependent exp / log pairs, 80 us for a band -- a sixth of the
// device-side chain of a wavelength in sos_spectrum).  Lane j forms the optical depth of layer j (the eight gases added in the
// reference's order) and its transmission; the running product TRS is then formed in layer order -- the same left-to-right
// product as the loop's -- each lane keeping the value of its own layer, and takes its logarithm.  Bands with more layers than
// lanes walk the layers in blocks of 64 with the product carried over.  (Today that second block never runs: the entry points
// refuse nlev > SOS_PROF_NBLEV_MAX = 64, i.e. more than 63 layers, because k_profile keeps the levels in LDS.  The loop is kept
// so that raising that limit stays a change of one constant; no test can reach its carry until then.)
// (the body of bin b, shared by k_absprofile and the table form k_absprofile_table)
__device__ __forceinline__ void absprofile_bin_body(const int b, const int lane, int nlev, int nterm, const int32_t *__restrict__ ik,
                                                    const double *__restrict__ xk, const double *__restrict__ ro,
                                                    double *__restrict__ tabs)
{
    const int nl1 = nlev - 1;
    int term[8];
    for (int k = 0; k < 8; k++) term[k] = min(max(ik[8 * b + k], 1), nterm) - 1;
    if (lane == 0) tabs[(size_t)b * nlev] = 0.;
    double trs = 1.0;                                            // TRS after the layers of the blocks before (wave-uniform)
    for (int j0 = 0; j0 < nl1; j0 += 64) {
        const int j = j0 + lane;
        double e = 1.0;
        if (j < nl1) {
            double t1c = 0.;
            for (int k = 0; k < 8; k++) t1c = t1c + xk[((size_t)k * nterm + term[k]) * nl1 + j] * ro[(size_t)k * nl1 + j];
            e = exp(-t1c);
        }
        double mine = 0.;
        const int cnt = min(64, nl1 - j0);
        for (int q = 0; q < cnt; q++) {                          // TRS = TRS * EXP(-T1C), layer by layer
            trs = trs * lane_read(e, q);
            if (q == lane) mine = trs;
        }
        if (j < nl1) tabs[(size_t)b * nlev + j + 1] = (mine > 0.) ? -log(mine) : 999.;           // CTE_TAUABS_MAX (SOS.h:297)
    }
}

__global__ __launch_bounds__(64) void k_absprofile(int nb, int nlev, int nterm, const int32_t *__restrict__ ik,
                                                   const double *__restrict__ xk, const double *__restrict__ ro,
                                                   double *__restrict__ tabs)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= nb) return;
    absprofile_bin_body(b, lane, nlev, nterm, ik, xk, ro, tabs);
}

// Table form: one wavefront per bin of all wavelengths of a part; NTERM and the places of the wavelength's xk / ro tables in
// the packed buffer `gas` come from its table entry.  Bins of a wavelength without gas (nterm 0) leave their row alone.
__global__ __launch_bounds__(64) void k_absprofile_table(const ProfileWl *__restrict__ tab, int nwl, const int32_t *__restrict__ wl_of_bin,
                                                         int nb, int nlev, const int32_t *__restrict__ ik,
                                                         const double *__restrict__ gas, double *__restrict__ tabs)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= nb) return;
    const int w = wl_of_bin[b];
    if (w < 0 || w >= nwl) return;
    const ProfileWl &t = tab[w];
    if (t.nterm < 1) return;
    absprofile_bin_body(b, lane, nlev, t.nterm, ik, gas + t.xk_off, gas + t.ro_off, tabs);
}

void launch_absprofile_table(const ProfileWl *d_tab, int nwl, const int32_t *d_wl_of_bin, int nb, int nlev, const int32_t *d_ik,
                             const double *d_gas, double *d_tabs, hipStream_t st)
{
    k_absprofile_table<<<nb, 64, 0, st>>>(d_tab, nwl, d_wl_of_bin, nb, nlev, d_ik, d_gas, d_tabs);
}

void launch_absprofile(int nb, int nlev, int nterm, const int32_t *d_ik, const double *d_xk, const double *d_ro, double *d_tabs,
                       hipStream_t st)
{
    k_absprofile<<<nb, 64, 0, st>>>(nb, nlev, nterm, d_ik, d_xk, d_ro, d_tabs);
}

// ---------------------------------------------------------------------------------------------------------------------
// Output levels of several altitudes (sosgpu_output_levels): the statements of k_profile's ZOUT branch (SOS.F:570-582,
// SOS_OS.F:1514-1520) on the profile k_profile left -- Z in zprof, H (after the rescale) in prof -- one thread per
// (slot, bin).  zout = -1: the standard output (level 0, TAUOUT = H(0)); a flagged bin (NT < 1): 0, 0 and TAUOUT = 0, as
// k_profile leaves it.  (fp contract is off for this file: the same roundings as k_profile.)
// ---------------------------------------------------------------------------------------------------------------------
// (the statements of one (altitude, bin), shared by k_output_levels and k_output_depths: H is any cumulative-depth row on Z)
__device__ __forceinline__ double output_level(const double *Z, const double *H, int nt, int lp, double zout, int &j, double &zz)
{
    double tauout = 0.;
    j = 0; zz = 0.;
    if (nt >= 1 && nt < lp) {
        tauout = H[0];
        if (zout != -1.0) {
            j = 1;
            while (j < nt && zout < Z[j]) j++;
            zz = (zout - Z[j - 1]) / (Z[j] - Z[j - 1]);
            tauout = (1 - zz) * H[j - 1] + zz * H[j];
        }
    }
    return tauout;
}

__global__ __launch_bounds__(256) void k_output_levels(OutputLevelArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nz * a.nb) return;
    const int k = i / a.nb, b = i - k * a.nb;
    int j;
    double zz;
    const double tauout = output_level(a.zprof + (size_t)b * a.lp, a.prof + (size_t)b * 3 * a.lp, a.nt[b], a.lp, a.zout[k], j, zz);
    a.jout[i] = j; a.zz[i] = zz; a.tauout[i] = tauout;
}

// The depth alone, on a depth row of any stride (sosgpu_output_depths): h_stride = lp for the untruncated rows k_profile
// exports (hvrai), 3 lp for the H row of prof -- where it returns k_output_levels' tauout bit for bit.
__global__ __launch_bounds__(256) void k_output_depths(OutputDepthArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nz * a.nb) return;
    const int k = i / a.nb, b = i - k * a.nb;
    int j;
    double zz;
    a.tau[i] = output_level(a.zprof + (size_t)b * a.lp, a.h + (size_t)b * a.h_stride, a.nt[b], a.lp, a.zout[k], j, zz);
}

// Diagnostic (sosgpu_debug_roundtrip): the register form of the PROFIL file's decimal round trip over an array, one thread per
// element -- fmt 0: rt_e15_8, 1: rt_f10_5 -- so that a test can hold it against the C library's print-and-read, value by value.
__global__ __launch_bounds__(256) void k_debug_roundtrip(int fmt, size_t n, const double *__restrict__ in, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fmt ? rt_f10_5(in[i]) : rt_e15_8(in[i]);
}

void launch_debug_roundtrip(int fmt, size_t n, const double *d_in, double *d_out, hipStream_t st)
{
    k_debug_roundtrip<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(fmt, n, d_in, d_out);
}

void launch_output_levels(const OutputLevelArgs &a, hipStream_t st)
{
    const int n = a.nz * a.nb;
    k_output_levels<<<(n + 255) / 256, 256, 0, st>>>(a);
}

void launch_output_depths(const OutputDepthArgs &a, hipStream_t st)
{
    const int n = a.nz * a.nb;
    k_output_depths<<<(n + 255) / 256, 256, 0, st>>>(a);
}
