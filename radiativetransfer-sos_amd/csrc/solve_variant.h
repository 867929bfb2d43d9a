// csrc/solve_variant.h -- which instantiation of the fused solver runs for a problem, and the sizes that go with it, stated
// once.  The capacity formulas are shared with the kernels (sos_dev.h includes this file); solve_variant() is host only, calls
// no HIP and reads no environment: it is a function of the problem shape and of the switches api_solve.hip has read.  solve_plan
// (solve_plan.h) builds on it, sosgpu_debug_solve_plan reports it, and the launchers of sos_os.hip / sos_stream.hip dispatch
// on what it says -- they refuse a context it does not fit, they do not choose.
#pragma once
#include "../../include/sosgpu.h"
#include "sos_common.h"

// ---- LDS-resident kernel (sos_os.hip) -----------------------------------------------------------------------------------
// Capacity constants of a variant of NW waves with RTWH row tiles each:
//   KHM = rows per direction half (3N <= KHM), FS = level stride of the field, NS = row stride of the attenuation table
__host__ __device__ constexpr int sos_khm(int nw, int rtwh) { return 16 * nw * rtwh; }
__host__ __device__ constexpr int sos_fs(int nw, int rtwh) { return 2 * sos_khm(nw, rtwh) + 2; }
__host__ __device__ constexpr int sos_ns(int nw, int rtwh) { return (sos_khm(nw, rtwh) / 3 + 1) & ~1; }

// dynamic LDS of k_sos_os<nw, rtw, ct>: the arrays its body carves out of smem, in their order
inline size_t lds_bytes_for(int nw, int rtw, int ct)
{
    const int cols = 16 * ct, fs = sos_fs(nw, rtw), ns = sos_ns(nw, rtw);
    return ((size_t)cols * fs + 3 * ns + 2 + 2 * ns + 16 + 2 * ns + (size_t)cols * ns + 7 * cols) * sizeof(double);
}

// k-pairs of the source contraction at Fourier order 0 (SosDev::ks2h0, set by sosgpu_create; sosgpu_debug_order0_kpairs reports
// the rule).  At s = 0 the function T^0_l is zero for every l (noyaux.hip gsf_body: it starts from zeros and its recurrence has
// F = 2 s / (l (l + 1)) = 0), so the kernels GT and ART that couple U to I and Q, the U rows of the order-1 vectors and the U
// terms of the molecular factors are exact zeros (noyaux_dev.h ktab_sum, sv_rows; noyaux.hip ray_vt_element, pack_ray_body).  The
// Lambert ground reflects into I only and the flat Fresnel matrix takes U into U (F33), so U(s = 0) stays exactly zero through
// every scattering order and the K positions of the U columns, 2 Nw ... 3 Nw - 1 in rowmap's component-major order, contribute
// products with an exact zero factor: the contraction stops after the k-pairs that hold the I and Q columns.  The accumulators
// start from +0 and a sum never gives -0 from there, so the dropped terms would not even have changed a sign bit.  A BRDF/BPDF
// surface (imat_surf) reflects through REAL*4 matrices in which nothing guarantees the zeros: the full count.
inline int sos_order0_kpairs(int nwgt, int ks2h, bool imat_surf)
{
    const int iq = (2 * nwgt + 7) / 8;
    return (imat_surf || iq > ks2h) ? ks2h : iq;
}

// ---- streamed kernel (sos_stream.hip) -----------------------------------------------------------------------------------
constexpr int COLS = 32;      // levels per chunk (two 16-column MFMA tiles)
constexpr int VPAD = 8;       // level vectors are stored with a +1 offset (entry e = level e-1) and a few spare entries

// Row capacity of the field layout.  Round 2 sized it by the wave shape alone, KHM = 16 NW RTWH rows per half: 64, 128, 256.  A half
// system of 66 ... 96 rows (N = 22 ... 32 -- the reference's default of 24 Gauss angles is N = 25) then moved 128-row chunks through
// LDS and HBM: N = 22 ran 32 % slower than N = 21 for 5 % more work (profiles/r03_n_sweep.txt).  The layout is now sized in row
// tiles, KHT = 5 or 6 for those direction counts (KHM = 80 / 96, FS = 162 / 194: 41 / 50 KB chunks instead of 66 KB), the wave
// shape staying <4,2> (wave 0, or waves 0 and 1, carry a second tile).  KHM = 16 KHT, FS = 2 KHM + 2 (still = 2 mod 4 doubles:
// conflict-free ds_read_b128 of the B operands), NS = directions capacity.
__host__ __device__ constexpr int skhm(int kht) { return 16 * kht; }
__host__ __device__ constexpr int sfs(int kht) { return 2 * skhm(kht) + 2; }
__host__ __device__ constexpr int sns(int kht) { return (skhm(kht) / 3 + 1) & ~1; }

// scratch of one bin, in doubles (lpb = level capacity, a multiple of COLS)
__host__ __device__ inline size_t stream_scratch_doubles(int nw, int kht, int lpb)
{
    const size_t fs = sfs(kht), ns = sns(kht), khm = skhm(kht), nch = lpb / COLS;
    const size_t d = (size_t)lpb * fs + (size_t)(lpb + 1) * ns + 7 * (size_t)(lpb + VPAD) + nch * (2 * khm + 2 * ns) +
                     2 * 64 * (size_t)nw + 8;                  // + state carried from one launch to the next (i4, i5 per thread)
    return (d + 15) & ~(size_t)15;
}

// dynamic LDS of k_sos_stream<.., KHT>
inline size_t stream_lds_bytes(int kht)
{
    const int fs = sfs(kht), ns = sns(kht);
    return ((size_t)COLS * fs + 3 * ns + 2 + 2 * ns + 16 + 2 * ns + (size_t)COLS * ns + 7 * (COLS + VPAD)) * sizeof(double);
}

// ---- the choice ---------------------------------------------------------------------------------------------------------
// the solver's environment switches, as read once per solve
struct SolveOverrides {
    long scratch_gib = 0;                          // SOSGPU_SCRATCH_GIB; <= 0: the default budget
    bool spec_off = false;                         // SOSGPU_STREAM_SPEC=0
    bool has_spec_maxbins = false; int spec_maxbins = 0;     // SOSGPU_STREAM_SPEC_MAXBINS
    bool has_spec_k = false; int spec_k = 0;       // SOSGPU_STREAM_SPEC_K
    int persist = 0;                               // SOSGPU_STREAM_PERSIST; non-zero: the persistent form, on the 8-tile layout
    int orders_per_launch = 0;                     // SOSGPU_STREAM_ORDERS_PER_LAUNCH; <= 0: all orders in one launch
    int q_tail = -1;                               // SOSGPU_STREAM_QTAIL; < 0: the launcher's default
};

struct SolveShape {
    int n, smax, nb, lp, nz;
    bool table;                                    // per-bin contexts from a device table (the _multi kernels)
};

typedef sosgpu_solve_plan SolvePlan;

// Fills the variant fields of *p (nw, rtw, ct, big, split, kht, threads, lds_bytes) or returns SOSGPU_E_UNSUPPORTED.
// lp - 1 bounds every NT of the batch (the host pads the level axis to lp), so the field has up to lp levels:
//   lp <= 32 : field in LDS, two column tiles, 4 waves (two workgroups per CU) -- the flagship; five or six row tiles on four
//              waves (N = 22 ... 32) run its shared-tile form SPLIT, the partials in the pad rows of the field (sos_dev.h
//              gemm_source_split)
//   lp <= 64 : field in LDS, four column tiles; for 21 < N <= 42 EIGHT waves with one row tile each, so that the
//              accumulators stay at 64 VGPRs and the CU still hosts two waves per SIMD although the 64-level field
//              leaves room for one workgroup only (68.6k vs 61.3k bins/s for <4,2,4> at N = 41, NT = 60)
//   lp >  64 : field streamed from a per-bin HBM scratch in chunks of two column tiles (sos_stream.hip), two workgroups per CU
//              (the 8-wave four-tile form was slower there: 21.8k vs 26.5k bins/s at NT = 100); the layout has KHT row tiles:
//              the wave shape's NW RTWH, but 5 or 6 for N = 22 ... 32 (above) -- unless the persistent form is asked for, which
//              exists for the full width only: the switch widens them to 8 whatever form the solve then takes
//   N > 42   : eight waves, two row tiles each, two column tiles (LDS holds 32 levels of the 6N x 8 B rows)
// kh and rtph are the context's, as sosgpu_create derives them from N.
inline int solve_variant(const SolveShape &sh, const SolveOverrides &ov, SolvePlan *p)
{
    if (sh.n < 1 || sh.n > 85 || sh.lp < 2 || sh.lp > 1024) return SOSGPU_E_UNSUPPORTED;
    const int kh = sos_round_up(3 * sh.n, 8), rtph = (kh + 15) / 16;
    p->split = p->kht = 0;
    if (kh > 128) { p->nw = 8; p->rtw = 2; p->ct = 2; p->big = sh.lp > 32; }
    else if (sh.lp <= 32 || sh.lp > 64) { p->nw = 4; p->rtw = kh <= 64 ? 1 : 2; p->ct = 2; p->big = sh.lp > 64; }
    else { p->nw = kh <= 64 ? 4 : 8; p->rtw = 1; p->ct = 4; p->big = 0; }
    if (p->big) {
        p->kht = p->nw * p->rtw;
        if (kh > 64 && kh <= 128) {
            p->kht = kh <= 80 ? 5 : kh <= 96 ? 6 : 8;
            if (ov.persist != 0) p->kht = 8;
        }
        p->lds_bytes = stream_lds_bytes(p->kht);
    } else {
        p->split = p->nw == 4 && p->rtw == 2 && p->ct == 2 && rtph > 4 && rtph <= 6 && 16 * rtph + 16 * (rtph - 4) <= sos_khm(4, 2);
        p->lds_bytes = lds_bytes_for(p->nw, p->rtw, p->ct);
    }
    p->threads = 64 * p->nw;
    return p->lds_bytes > 160 * 1024 ? SOSGPU_E_UNSUPPORTED : 0;
}
