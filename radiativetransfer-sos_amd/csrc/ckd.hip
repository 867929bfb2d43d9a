// csrc/ckd.hip -- COEFF_ABS_CKD (src/SOS_SUB_TRS.F:171-393) for the wavelengths of a part of a spectrum in one launch:
// the absorption coefficient k_i of every (wavelength, gas, exponential term) table interpolated to the layers of the
// atmosphere, with the parsed coefficient tables resident in device memory (sosgpu_ckd_layer_tables).
#include <hip/hip_runtime.h>
#include "kernels.h"

// Every statement below is the reference's, in its order, in IEEE double arithmetic: no contraction into fused multiply-adds.
#pragma clang fp contract(off)

namespace {
// SOS_INTERPOL (SOS_AEROSOLS.F:3862)
__device__ __forceinline__ double ckd_interpol(double y1, double y2, double x1, double x2, double x)
{
    return ((y2 - y1) / (x2 - x1)) * (x - x2) + y2;
}

// `I = 1; DO WHILE (TAB(I) <= V .AND. I < N) I = I + 1; I = I - 1` on 0-based indices.  The clamps in front of every call
// give tab[0] <= v, so the result is 0 .. n-2; a NaN abscissa would give -1: held at 0, the tables are never read out of bounds.
__device__ __forceinline__ int ckd_bracket(const double *tab, int n, double v)
{
    int i = 0;
    while (tab[i] <= v && i < n - 1) ++i;
    --i;
    return i < 0 ? 0 : i;
}
}  // namespace

// One wavefront per slot = (wavelength, gas, term): blockIdx.y walks the wavelengths, blockIdx.x = gas * nterm + term.  Lane j
// is layer j (layer 0 = top layer), nlay <= 63.  The slot's parameters -- axis lengths, the places of the axes and of the layer
// state in `axes`, the table pointer -- are wave-uniform and come from the device table, as k_profile_table takes its ProfileWl.
// The three per-lane arrays of runtime length (XKI, U, Y2 of SOS_SPLINE) are columns of LDS: [node][lane], a lane's column is
// its own, consecutive lanes on consecutive banks.  The only barrier stands behind the cooperative load of the axes, before
// any lane leaves.
__global__ __launch_bounds__(64) void k_coeff_abs_ckd_table(const CkdWl *__restrict__ tab, int nwl, const double *const *__restrict__ ki_of_slot,
                                                            const double *__restrict__ axes, int nlay, double *__restrict__ out,
                                                            int32_t *__restrict__ status)
{
    __shared__ double s_t[SOS_CKD_NT_MAX], s_p[SOS_CKD_NP_MAX], s_c[SOS_CKD_NC_MAX];
    __shared__ double s_xki[SOS_CKD_NT_MAX][64], s_u[SOS_CKD_NT_MAX][64], s_d2[SOS_CKD_NT_MAX][64];
    const int lane = threadIdx.x;
    for (int w = blockIdx.y; w < nwl; w += gridDim.y) {
        const CkdWl &e = tab[w];
        const int slot = blockIdx.x;
        if (slot >= 8 * e.nterm) continue;                       // (wave-uniform)
        const int gas = slot / e.nterm;
        const int nt = e.nt, np = e.np, nc = e.nc;
        const double *__restrict__ ki = ki_of_slot[e.slot0 + slot];
        double *__restrict__ xk = out + e.xk_off + (size_t)slot * nlay;
        if (!ki) {                                               // term >= NEXP of the gas, or a table that is all zero
            if (lane < nlay) xk[lane] = 0.0;
            continue;
        }
        __syncthreads();                                         // (the axes of the wavelength before are no longer read)
        if (lane < nt) s_t[lane] = axes[e.temp_off + lane];
        if (lane < np) s_p[lane] = axes[e.pres_off + lane];
        if (lane < nc) s_c[lane] = axes[e.conc_off + lane];
        __syncthreads();
        if (lane >= nlay) continue;                              // (no barrier below in this iteration)
        double prs = axes[e.prs_off + lane], tmp = axes[e.tmp_off + lane], conc = axes[e.cl_off + lane];
        tmp = (s_t[0] > tmp) ? s_t[0] : tmp;                     // TMP = MIN(MAX(TMP, T(1)), T(NT))
        tmp = (s_t[nt - 1] < tmp) ? s_t[nt - 1] : tmp;
        if (prs <= s_p[0]) { xk[lane] = 0.0; continue; }         // above the table: no absorption
        prs = (s_p[np - 1] < prs) ? s_p[np - 1] : prs;
        const int ip = ckd_bracket(s_p, np, prs);
        const double p0 = s_p[ip], p1 = s_p[ip + 1];
        if (gas == 0) {                                          // H2O: along the concentration first, then along the pressure
            conc = (s_c[0] > conc) ? s_c[0] : conc;
            conc = (s_c[nc - 1] < conc) ? s_c[nc - 1] : conc;
            const int ic = ckd_bracket(s_c, nc, conc);
            const double c0 = s_c[ic], c1 = s_c[ic + 1];
            const double *k0 = ki + ((size_t)ic * np + ip) * nt, *k1 = k0 + (size_t)np * nt;
            for (int t = 0; t < nt; t++) {
                const double a0 = ckd_interpol(k0[t], k1[t], c0, c1, conc);
                const double a1 = ckd_interpol(k0[nt + t], k1[nt + t], c0, c1, conc);
                s_xki[t][lane] = ckd_interpol(a0, a1, p0, p1, prs);
            }
        } else {
            const double *k0 = ki + (size_t)ip * nt;
            for (int t = 0; t < nt; t++) s_xki[t][lane] = ckd_interpol(k0[t], k0[nt + t], p0, p1, prs);
        }
        // SOS_INTERPO_SPLINT: end slopes, SOS_SPLINE (SOS_AEROSOLS.F:4976-5010), SOS_SPLINT (:5060-5079)
        const double big = (double).99E30f;                      // the REAL*4 literal, widened as the compiler widens it
        const double dy1 = (s_xki[1][lane] - s_xki[0][lane]) / (s_t[1] - s_t[0]);
        const double dyn = (s_xki[nt - 1][lane] - s_xki[nt - 2][lane]) / (s_t[nt - 1] - s_t[nt - 2]);
        if (dy1 > big) { s_d2[0][lane] = 0.; s_u[0][lane] = 0.; }
        else {
            s_d2[0][lane] = -0.5;
            s_u[0][lane] = (3. / (s_t[1] - s_t[0])) * ((s_xki[1][lane] - s_xki[0][lane]) / (s_t[1] - s_t[0]) - dy1);
        }
        for (int k = 1; k < nt - 1; k++) {
            const double sig = (s_t[k] - s_t[k - 1]) / (s_t[k + 1] - s_t[k - 1]);
            const double p = sig * s_d2[k - 1][lane] + 2.;
            s_d2[k][lane] = (sig - 1.) / p;
            s_u[k][lane] = (6. * ((s_xki[k + 1][lane] - s_xki[k][lane]) / (s_t[k + 1] - s_t[k])
                                  - (s_xki[k][lane] - s_xki[k - 1][lane]) / (s_t[k] - s_t[k - 1])) / (s_t[k + 1] - s_t[k - 1])
                            - sig * s_u[k - 1][lane]) / p;
        }
        double qn, un;
        if (dyn > big) { qn = 0.; un = 0.; }
        else {
            qn = 0.5;
            un = (3. / (s_t[nt - 1] - s_t[nt - 2])) * (dyn - (s_xki[nt - 1][lane] - s_xki[nt - 2][lane]) / (s_t[nt - 1] - s_t[nt - 2]));
        }
        s_d2[nt - 1][lane] = (un - qn * s_u[nt - 2][lane]) / (qn * s_d2[nt - 2][lane] + 1.);
        for (int k = nt - 2; k >= 0; k--) s_d2[k][lane] = s_d2[k][lane] * s_d2[k + 1][lane] + s_u[k][lane];
        int klo = 0, khi = nt - 1;
        while (khi - klo > 1) {
            const int k = (khi + klo + 2) / 2 - 1;               // (KHI+KLO)/2 on 1-based indices
            if (s_t[k] > tmp) khi = k; else klo = k;
        }
        const double h = s_t[khi] - s_t[klo];
        if (h == 0.) {                                           // 'ERROR for SPLINT interpolation'
            atomicMax(&status[w], 1);
            xk[lane] = 0.0;
            continue;
        }
        const double a = (s_t[khi] - tmp) / h;
        const double b = (tmp - s_t[klo]) / h;
        double v = a * s_xki[klo][lane] + b * s_xki[khi][lane]
                   + ((a * a * a - a) * s_d2[klo][lane] + (b * b * b - b) * s_d2[khi][lane]) * (h * h) / 6.;
        if (v < 0.) {                                            // the spline undershoots: linear in temperature
            const int it = ckd_bracket(s_t, nt, tmp);
            v = ckd_interpol(s_xki[it][lane], s_xki[it + 1][lane], s_t[it], s_t[it + 1], tmp);
            if (v < 0.) {                                        // COEFF_ABS_CKD ERROR_923
                atomicMax(&status[w], 2);
                v = 0.0;
            }
        }
        xk[lane] = v;
    }
}

void launch_coeff_abs_ckd_table(const CkdWl *d_tab, int nwl, int max_slots, const double *const *d_ki, const double *d_axes, int nlay,
                                double *d_out, int32_t *d_status, hipStream_t st)
{
    const dim3 grid((unsigned)max_slots, (unsigned)(nwl < 65535 ? nwl : 65535));
    k_coeff_abs_ckd_table<<<grid, 64, 0, st>>>(d_tab, nwl, d_ki, d_axes, nlay, d_out, d_status);
}
