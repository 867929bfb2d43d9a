"""The aerosol device chain of csrc/mie.hip -- k_mie<false> (coefficient arrays in LDS), k_mie<true> (arrays in an HBM scratch,
grid-strided over 2048 slots) and k_granu_batch (SOS_GRANU, the size-distribution integral) -- against the serial fp64 oracle
(oracle/sos_mie_oracle.c), at the shapes where their loops, forms and branches change.

The oracle is pinned on the CPU three ways: it reproduces every record of tests/golden/mie_chain.npz, it agrees with an
independent 50-digit Mie series (mpmath) for refractive indices that have no golden, and its SOS_GRANU gives the sums of
tests/aerosol_loops.granu_host.  The GPU tests drive sosgpu_mie / sosgpu_granu / sosgpu_granu_batch directly through capi with
hand-made size-parameter lists; one parametrised cell per edge, ids that name it.  CPU tests assert from the oracle's `info` and
from plain arithmetic that the tables cover every edge, so a later edit cannot quietly drop one.
A kernel trace of this module is kept in profiles/mie_granu_kernel_stats.csv."""
import ctypes as C
import functools
import importlib
import math
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
A = importlib.import_module("radiativetransfer-sos_amd.aerosols")       # host helpers only (alpha_grid, mie_angles)

E_ARG, E_UNSUPPORTED = -1, -3
LDS_ALPHA = 850.0                        # sosgpu_mie: size parameters up to here run in the LDS form
ABOVE = float(np.nextafter(LDS_ALPHA, np.inf))
SLOTS = 2048                             # workgroups (scratch slots) of the scratch form
MIE_THREADS, GRANU_THREADS, GRANU_UNROLL = 128, 256, 24
ALPHA_LAST = 4988.0                      # the largest alpha with 2 alpha + 24 <= 10000 (CTE_MIE_DIM)
ALPHA_OVER = float(np.nextafter(ALPHA_LAST, np.inf))
MPMATH_BAR = 1e-11                       # ten times the worst case measured on the CPU, 9.7e-13

GOLDEN_INDICES = [(1.45, -0.003), (1.33, 0.0), (1.53, -0.008)]
NEW_INDICES = [(1.75, -0.44), (1.95, -0.79), (1.05, -1e-6)]
INDICES = GOLDEN_INDICES + NEW_INDICES + [(1.5, 0.0)]                   # (1.33, 0) and (1.5, 0): `in` = 0 exactly


def before(x):
    return float(np.nextafter(x, 0.0))


@functools.lru_cache(maxsize=None)
def xmu_of(nbmu):
    return A.mie_angles(nbmu)[0]


# ---------------------------------------------------------------------------------------------------------------------
# k_mie cells: id -> (nbmu, (rn, in), size parameters)
# ---------------------------------------------------------------------------------------------------------------------
LDS_LIST = [0.5, 3.7, 25.0, 140.3, 612.5]
SCR_LIST = [851.5, 1203.25, 2750.0]
MIXED = [1e-4, 0.01, 0.7, 5.0, 33.3, 250.0, 849.0, LDS_ALPHA, ABOVE, 1500.0]
OVERFLOW_LDS = np.arange(740.0, 790.0, 0.125)       # both onsets inside: first rescale 745.5, first break 768.5 (test below)
OVERFLOW_SCR = np.arange(851.0, 900.25, 0.5)
N2_STEPS = [v for k in (10.0, 10.5, 100.0, 425.5, 700.0) for v in (before(k), k)]    # int(2 alpha + 5) steps between each pair


def stride_alphas(n):
    """n distinct size parameters just above the LDS limit (cheap, and a record written to the wrong place shows)."""
    return 850.25 + np.arange(n) * 2.0 ** -12


def _mie_cells():
    cells = {}
    for k, nbmu in enumerate((1, 31, 63, 64, 100)):                    # W = 3, 63, 127, 129, 201 against 128 threads
        cells["angles-nbmu%d-lds" % nbmu] = (nbmu, INDICES[k % 7], LDS_LIST)
        cells["angles-nbmu%d-scratch" % nbmu] = (nbmu, INDICES[(k + 3) % 7], SCR_LIST)
    for rn, in_ in INDICES:
        cells["index-%g%+gi" % (rn, in_)] = (12, (rn, in_), MIXED)
    cells["split-all-lds"] = (10, INDICES[0], [0.2, 77.7, 849.5, LDS_ALPHA])
    cells["split-none-lds"] = (10, INDICES[3], [ABOVE, 850.5, 1000.0])
    cells["split-straddle"] = (10, INDICES[2], [12.0, 849.5, LDS_ALPHA, ABOVE, 850.5, 2000.0])
    cells["split-one-lds"] = (10, INDICES[4], [LDS_ALPHA])
    cells["split-one-scratch"] = (10, INDICES[5], [ABOVE])
    cells["split-repeated"] = (10, INDICES[0], [3.0, 3.0, 3.0, 849.0, 849.0, 851.0, 851.0, 851.0])
    cells["stride-2048"] = (1, INDICES[0], stride_alphas(SLOTS))
    cells["stride-2049"] = (1, INDICES[3], stride_alphas(SLOTS + 1))
    cells["stride-4100-with-lds-prefix"] = (31, INDICES[1], np.concatenate([[1.0, 849.75], stride_alphas(4100)]))
    cells["overflow-onsets-lds"] = (12, INDICES[0], OVERFLOW_LDS)
    cells["overflow-onsets-lds-soot"] = (64, INDICES[3], OVERFLOW_LDS[120:300])
    cells["overflow-scratch-851-900"] = (12, INDICES[4], OVERFLOW_SCR)
    cells["n2-steps"] = (12, INDICES[2], N2_STEPS)
    cells["limit-alpha-1e-4"] = (100, INDICES[0], [1e-4])
    cells["limit-alpha-4988"] = (12, INDICES[0], [ALPHA_LAST])
    return {k: (v[0], v[1], np.asarray(v[2], dtype=np.float64)) for k, v in cells.items()}


MIE = _mie_cells()
REJECTED = {                                                              # id -> (size parameters, expected return code)
    "over-the-reference-dimension": ([1.0, ALPHA_OVER], E_UNSUPPORTED),
    "descending": ([2.0, 1.0], E_ARG),
    "descending-late": ([1.0, 2.0, 900.0, 899.0], E_ARG),
    "zero": ([0.0, 1.0], E_ARG),
    "negative": ([-1.0], E_ARG),
    "nan": ([1.0, float("nan")], E_ARG),
}


def n_lds_of(alphas):
    return int(np.sum(np.asarray(alphas) <= LDS_ALPHA))


@functools.lru_cache(maxsize=None)
def mie_oracle(cid):
    from oracle import oracle_ctypes as O
    nbmu, (rn, in_), alphas = MIE[cid]
    return O.mie(xmu_of(nbmu), rn, in_, alphas)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)


def ulp32(x):
    """Spacing of REAL*4 at |x|."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def near_zero(ref):
    """Q and U elements below 1e-6 of I at their angle, decided from the oracle's doubles alone: mask [na][2 W] over qmie | umie."""
    w = (ref["f64"].shape[1] - 3) // 3
    i = ref["f64"][:, 3:3 + w]
    return np.abs(ref["f64"][:, 3 + w:]) < 1e-6 * np.abs(np.concatenate([i, i], axis=1))


def record_report(got_rec, got_g, ref):
    """Field by field at the bar of test_mie_kernel_records_vs_the_references_mie_file: REAL*4 fields within 1 ulp and at most
    0.1 % of a field's entries different, g to 1e-13.  Returns (list of failures, report lines).  A cell that fails in Q or U only
    at elements next to a zero crossing (near_zero) has those held to 1 REAL*4 ulp of I at that angle instead."""
    w = (got_rec.shape[1] - 4) // 3
    fields = dict(alpha=slice(0, 1), qext=slice(1, 2), qsca=slice(2, 3), pad=slice(3, 4), imie=slice(4, 4 + w),
                  qmie=slice(4 + w, 4 + 2 * w), umie=slice(4 + 2 * w, 4 + 3 * w))
    nz = near_zero(ref)
    esc = dict(qmie=nz[:, :w], umie=nz[:, w:])
    fails, lines = [], []
    for k, sl in fields.items():
        a, b = got_rec[:, sl], ref["rec"][:, sl]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            fails.append("%s: not finite" % k)
            continue
        d = np.abs(bits(a) - bits(b))
        lines.append("%s: max %d ulp, %d of %d differ" % (k, d.max(), int((d != 0).sum()), d.size))
        if d.max() <= 1 and np.mean(d != 0) <= 1e-3:
            continue
        if k in esc:                                                  # the capped escape (test_zero_crossing_share_is_capped)
            m = esc[k]
            strict = d[~m]
            loose = np.abs(a.astype(np.float64) - b.astype(np.float64))[m] <= ulp32(ref["rec"][:, fields["imie"]])[m]
            lines.append("%s: %d elements next to a zero crossing held to 1 ulp of I" % (k, int(m.sum())))
            if (strict.size == 0 or (strict.max() <= 1 and np.mean(strict != 0) <= 1e-3)) and loose.all():
                continue
        fails.append("%s: max %d ulp, share different %.3g, first records %s" % (k, d.max(), np.mean(d != 0),
                                                                                np.unique(np.argwhere(d != 0)[:, 0])[:8]))
    rel = np.abs(got_g - ref["g"]) / np.abs(ref["g"])
    lines.append("g: rel %.2e" % rel.max())
    if not rel.max() <= 1e-13:
        fails.append("g: rel %.3g at record %d" % (rel.max(), int(np.argmax(rel))))
    return fails, lines


# ---------------------------------------------------------------------------------------------------------------------
# The oracle pinned on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _golden_ranges():
    g = np.load(os.path.join(GOLD, "mie_chain.npz"))
    for name in ("small", "mid", "large", "lds_edge", "dustlike"):
        rn, in_, a0, a1 = g["range_" + name]
        ref = {k: g["range_%s_%s" % (name, k)] for k in ("alpha", "qext", "qsca", "g", "imie", "qmie", "umie")}
        yield name, g["range_xmu"], rn, in_, A.alpha_grid(a0, a1), ref
    ref = {k[4:]: g[k] for k in g.files if k.startswith("mie_") and k != "mie_file_name"}
    yield ("chain", A.mie_angles(int(ref["nbmu"]))[0], float(ref["rn"]), float(ref["in_"]),
           A.alpha_grid(A.MIE_ALPHAMIN, float(ref["alphaf"])), ref)


def test_oracle_reproduces_the_references_mie_records(oracle):
    """sos_oracle_mie against all of mie_chain.npz (five ranges and the 3900-record chain) at the bar of
    test_mie_kernel_records_vs_the_references_mie_file.  Measured: every REAL*4 entry and every g identical (0 of 394 158
    entries different, g rel 0)."""
    ntot = ndiff = 0
    for name, xmu, rn, in_, alphas, ref in _golden_ranges():
        got = oracle.mie(xmu, rn, in_, alphas)
        for k in ("alpha", "qext", "qsca", "imie", "qmie", "umie"):
            d = np.abs(bits(got[k]) - bits(ref[k]))
            ntot, ndiff = ntot + d.size, ndiff + int((d != 0).sum())
            assert d.max() <= 1 and np.mean(d != 0) <= 1e-3, (name, k, d.max(), np.mean(d != 0))
        grel = np.abs(got["g"] - ref["g"]) / np.abs(ref["g"])
        print("oracle vs MIE file, %s: g rel %.2e" % (name, grel.max()))
        assert np.allclose(got["g"], ref["g"], rtol=1e-13, atol=0), name
    print("oracle vs MIE file: %d of %d REAL*4 entries different" % (ndiff, ntot))
    assert ntot == 394158


MP_ALPHAS = [1e-4, 1e-2, 0.3, 1.0, 5.0, 12.0, 20.0, 37.5, 60.0]
MP_INDICES = NEW_INDICES + [(1.33, 0.0)]
MP_ANGLES = [3, 100, 150, 197]           # of the W = 201 set: backward, 90 degrees, and two beyond index 128


def mp_mie(mp, x, rn, in_, mus):
    """Mie series in 50 digits from the textbook formulas (Bohren & Huffman 4.53, 4.61, 4.62, 4.74): Riccati-Bessel functions
    from besselj / bessely of half-integer order, their derivatives from psi_n' = psi_(n-1) - n psi_n / z.  Shares no code and no
    recurrence direction with SOS_MIE.  Returns Qext, Qsca, g and (I, Q, U) per cosine, normalised as the MIE record."""
    x, m, half = mp.mpf(x), mp.mpc(rn, -in_), mp.mpf(1) / 2
    mx = m * x
    nmax = int(float(x) + 8 * float(x) ** (1 / 3) + 25)
    psi = lambda n, z: z * mp.sqrt(mp.pi / (2 * z)) * mp.besselj(n + half, z)
    chi = lambda n, z: -z * mp.sqrt(mp.pi / (2 * z)) * mp.bessely(n + half, z)
    px, cx, pm = ([f(n, z) for n in range(nmax + 1)] for f, z in ((psi, x), (chi, x), (psi, mx)))
    a, b = [0] * (nmax + 2), [0] * (nmax + 2)
    for n in range(1, nmax + 1):
        dpx, dcx, dpm = px[n - 1] - n * px[n] / x, cx[n - 1] - n * cx[n] / x, pm[n - 1] - n * pm[n] / mx
        xi, dxi = px[n] - 1j * cx[n], dpx - 1j * dcx
        a[n] = (m * pm[n] * dpx - px[n] * dpm) / (m * pm[n] * dxi - xi * dpm)
        b[n] = (pm[n] * dpx - m * px[n] * dpm) / (pm[n] * dxi - m * xi * dpm)
    ns = range(1, nmax + 1)
    qe = sum((2 * n + 1) * mp.re(a[n] + b[n]) for n in ns) * 2 / x ** 2
    qs = sum((2 * n + 1) * (abs(a[n]) ** 2 + abs(b[n]) ** 2) for n in ns) * 2 / x ** 2
    g = sum(mp.mpf(n) * (n + 2) / (n + 1) * mp.re(a[n] * mp.conj(a[n + 1]) + b[n] * mp.conj(b[n + 1]))
            + mp.mpf(2 * n + 1) / (n * (n + 1)) * mp.re(a[n] * mp.conj(b[n])) for n in ns) * 4 / (x ** 2 * qs)
    iqu = []
    for mu in mus:
        mu, pi0, pi1, s1, s2 = mp.mpf(mu), mp.mpf(0), mp.mpf(1), 0, 0
        for n in ns:
            tau, f = n * mu * pi1 - (n + 1) * pi0, mp.mpf(2 * n + 1) / (n * (n + 1))
            s1, s2 = s1 + f * (a[n] * pi1 + b[n] * tau), s2 + f * (a[n] * tau + b[n] * pi1)
            pi0, pi1 = pi1, ((2 * n + 1) * mu * pi1 - (n + 1) * pi0) / n
        c = 2 / (qs * x ** 2)
        iqu.append((c * (abs(s1) ** 2 + abs(s2) ** 2), c * (abs(s2) ** 2 - abs(s1) ** 2), c * 2 * mp.re(s1 * mp.conj(s2))))
    return qe, qs, g, iqu


def test_oracle_vs_an_independent_mie_series(oracle):
    """The oracle's unrounded Qext, Qsca, g, I, Q, U against mp_mie for four refractive indices without a golden, alpha from 1e-4
    to 60, at four angles of the W = 201 set (two beyond index 128).  Qext, Qsca and I relative to themselves; Q and U, which cross
    zero, relative to I at their angle; g, a mean cosine bounded by 1 that goes to zero like alpha^2 in the Rayleigh limit, by its
    absolute difference everywhere and relative to itself from alpha = 0.3 up.  Measured worst case 9.7e-13 (U at the backward angle, alpha = 5,
    m = 1.75-0.44i; g differs by 2.4e-15 at most); the bar is ten times that, below the project's parity bar of 1e-9.
    A finding about the algorithm, not covered by a bar: relative to itself g is off by 1.5e-6 at alpha = 1e-4 (m = 1.05-1e-6i,
    g = 1.6e-9) and by 6.5e-11 at alpha = 0.01 -- SOS_MIE sums g from products of coefficients that are O(1) after the division
    by Qsca alpha^2, so its rounding error is absolute.  No caller of the records reads g."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    xmu = xmu_of(100)
    worst, where = 0.0, None
    for rn, in_ in MP_INDICES:
        f64 = oracle.mie(xmu, rn, in_, MP_ALPHAS)["f64"]
        for k, al in enumerate(MP_ALPHAS):
            qe, qs, g, iqu = mp_mie(mp, al, rn, in_, [xmu[j] for j in MP_ANGLES])
            errs = dict(qext=abs(f64[k, 0] - qe) / qe, qsca=abs(f64[k, 1] - qs) / qs, g_abs=abs(f64[k, 2] - g))
            g_rel = float(abs((f64[k, 2] - g) / g))
            if al >= 0.3:
                errs["g"] = g_rel
            for j, (i_, q_, u_) in zip(MP_ANGLES, iqu):
                errs["I%d" % j] = abs(f64[k, 3 + j] - i_) / i_
                errs["Q%d" % j] = abs(f64[k, 3 + 201 + j] - q_) / i_
                errs["U%d" % j] = abs(f64[k, 3 + 402 + j] - u_) / i_
            name, e = max(errs.items(), key=lambda kv: kv[1])
            print("oracle vs series, m = %g%+gi, alpha = %g: worst %.2e (%s), g relative %.2e" % (rn, in_, al, float(e), name, g_rel))
            if e > worst:
                worst, where = float(e), (rn, in_, al, name)
    print("oracle vs series: worst %.2e at %s, bar %.1e" % (worst, where, MPMATH_BAR))
    assert worst <= MPMATH_BAR, (worst, where)


def test_oracle_granu_vs_the_host_restatement(oracle):
    """sos_oracle_granu against aerosol_loops.granu_host (which reproduces the reference's Aerosols.txt) on the golden chain's
    3900 records, log-normal and Junge laws (stopped by alphaf and by rmax), to 1e-14; the record count from plain arithmetic."""
    import aerosol_loops
    g = np.load(os.path.join(GOLD, "mie_chain.npz"))
    rec = {k[4:]: g[k] for k in g.files if k.startswith("mie_") and k != "mie_file_name"}
    full = np.concatenate([rec["alpha"][:, None], rec["qext"][:, None], rec["qsca"][:, None], np.zeros((3900, 1), np.float32),
                           rec["imie"], rec["qmie"], rec["umie"]], axis=1)
    for igranu, v1, v2, v3, wa, af in ((1, 0.12, 0.45, -999.0, 0.865, 100.0), (1, 0.8, 0.6, -999.0, 0.55, 40.0),
                                       (2, 0.05, 4.2, 12.0, 0.865, 100.0), (2, 0.1, 3.5, 50.0, 1.6, 25.0)):
        rec["alphaf"] = af
        ref = aerosol_loops.granu_host(rec, igranu, v1, v2, v3, wa)
        out, n = oracle.granu(full, igranu, v1, v2, v3, wa, af)
        want = np.concatenate([ref[:3], *ref[3:]])
        err = np.abs(out - want) / np.maximum(np.abs(want), 1e-300)
        print("oracle granu law %d: nuse %d, worst rel %.2e" % (igranu, n, err.max()))
        a64, r = rec["alpha"].astype(np.float64), rec["alpha"].astype(np.float64) * wa / 2. / math.pi
        pp = np.array([step_of(np.float32(0))] + [step_of(a) for a in rec["alpha"][:-1]])
        assert n == int(np.argmax((a64 >= af - pp) | ((r > v3) & (igranu == 2)))) and 0 < n < 3900
        assert np.allclose(out, want, rtol=1e-14, atol=1e-16 * np.abs(want).max()), (igranu, err.max())


# ---------------------------------------------------------------------------------------------------------------------
# The k_mie table covers its edges (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_mie_table_covers_angles_forms_and_indices():
    ws = {(2 * MIE[c][0] + 1, c.rsplit("-", 1)[1]) for c in MIE if c.startswith("angles-")}
    assert ws == {(w, f) for w in (3, 63, 127, 129, 201) for f in ("lds", "scratch")}
    for c in MIE:
        nbmu, _, al = MIE[c]
        assert np.all(np.diff(al) >= 0) and al[0] > 0 and 2 * al[-1] + 24 <= 10000 and 1 <= nbmu <= 100, c
        if c.startswith("angles-") and c.endswith("-lds"):
            assert n_lds_of(al) == len(al), c
        if c.startswith("angles-") and c.endswith("-scratch"):
            assert n_lds_of(al) == 0, c
    # angle loop of 128 threads: under one pass, one pass less one, one pass plus one, and into the second pass up to 201
    assert [w for w, f in sorted(ws) if f == "lds"] == [3, 63, MIE_THREADS - 1, MIE_THREADS + 1, 201]
    assert {MIE[c][1] for c in MIE if c.startswith("index-")} == set(INDICES) and len(set(INDICES)) == 7
    assert sum(1 for _, in_ in INDICES if in_ == 0.0) == 2
    for c in MIE:
        if c.startswith("index-"):                                    # each index in both forms
            assert 0 < n_lds_of(MIE[c][2]) < len(MIE[c][2])
    # form split
    s = {c[6:]: MIE[c][2] for c in MIE if c.startswith("split-")}
    assert n_lds_of(s["all-lds"]) == len(s["all-lds"]) and s["all-lds"][-1] == LDS_ALPHA
    assert n_lds_of(s["none-lds"]) == 0 and s["none-lds"][0] == ABOVE
    k = n_lds_of(s["straddle"])
    assert s["straddle"][k - 1] == LDS_ALPHA and s["straddle"][k] == ABOVE and ABOVE > LDS_ALPHA and 0 < k < len(s["straddle"]) - 1
    assert list(s["one-lds"]) == [LDS_ALPHA] and list(s["one-scratch"]) == [ABOVE]
    r = s["repeated"]
    assert len(set(r)) == 3 and len(r) == 8 and 0 < n_lds_of(r) < len(r)
    # grid stride over the 2048 slots: one full grid, one record into the second trip, and a third trip
    n_scr = {c: len(MIE[c][2]) - n_lds_of(MIE[c][2]) for c in MIE if c.startswith("stride-")}
    assert sorted(n_scr.values()) == [SLOTS, SLOTS + 1, 4100] and 4100 > 2 * SLOTS
    for c in n_scr:
        al = MIE[c][2]
        assert len(set(al)) == len(al) and al[-1] < 852.0
    assert n_lds_of(MIE["stride-4100-with-lds-prefix"][2]) == 2
    # limits
    assert list(MIE["limit-alpha-1e-4"][2]) == [1e-4]
    assert 2 * ALPHA_LAST + 24 <= 10000 < 2 * ALPHA_OVER + 24 and list(MIE["limit-alpha-4988"][2]) == [ALPHA_LAST]
    codes = {k: v[1] for k, v in REJECTED.items()}
    assert codes["over-the-reference-dimension"] == E_UNSUPPORTED and sum(1 for v in codes.values() if v == E_ARG) >= 4


def test_overflow_cells_sit_on_both_onsets(oracle):
    """From the oracle's info: where the CNA break is first taken and where SNA is first rescaled, and that the overflow cells
    hold size parameters on either side of each, with the break index n2, n2 - 1, ... below int(2 alpha + 5) in turn.  Neither
    onset depends on the refractive index, and neither is monotonic: between 745.5 and 746.375, and between 768.5 and 769.0, a
    branch is taken at one size parameter and not at the next."""
    ref = mie_oracle("overflow-onsets-lds")
    al, info = MIE["overflow-onsets-lds"][2], ref["info"]
    n2_0 = (al + al + 5).astype(int)
    n1_0 = (al + al + 20).astype(int)
    broke, resc = info[:, 1] == 1, info[:, 2]
    first_break, first_resc = al[broke][0], al[resc > 0][0]
    print("first break at %.3f (index %d = n2), first rescale at %.3f" % (first_break, info[broke][0, 0], first_resc))
    assert first_break == 768.5 and first_resc == 745.5
    assert al[~broke][-1] == 769.375 and al[resc == 0][-1] == 746.375 and set(resc) == {0, 1}
    assert np.all(info[~broke, 0] == n2_0[~broke]) and np.all(info[~broke, 3] == n1_0[~broke])
    assert np.all(info[broke, 3] == info[broke, 0] + 15)
    # on integers the break is first taken at 769, at i = 1543 = n2 exactly: the last term
    k769 = int(np.flatnonzero(al == 769.0)[0])
    assert broke[k769] and not broke[int(np.flatnonzero(al == 768.0)[0])] and info[k769, 0] == 1543 == n2_0[k769]
    drop = n2_0[broke] - info[broke, 0]
    assert set(drop) >= set(range(0, 8)) and np.all(np.diff(drop) >= -1)          # the break index sweeps down from n2
    assert (info[broke, 3] != n1_0[broke]).any() and (info[broke, 3] == n1_0[broke]).any()
    # both sides of each onset are in the cell: 20 size parameters at least
    for on in (broke, resc > 0):
        assert on.sum() >= 20 and (~on).sum() >= 20
    soot = mie_oracle("overflow-onsets-lds-soot")["info"]
    lo, hi = 120, 300
    assert np.array_equal(soot[:, :4], info[lo:hi, :4]) and set(soot[:, 1]) == {0, 1}       # the onsets do not move with the index
    scr = mie_oracle("overflow-scratch-851-900")["info"]
    als = MIE["overflow-scratch-851-900"][2]
    assert als[0] == 851.0 and als[-1] == 900.0 and np.all(scr[:, 1] == 1) and np.all(scr[:, 2] >= 1)
    assert len(set((als + als + 5).astype(int) - scr[:, 0])) >= 10
    # int(2 alpha + 5) steps between the members of each pair
    st = mie_oracle("n2-steps")["info"][:, 0]
    assert np.all(st[1::2] - st[0::2] == 1)
    # the rest of the table, for the record: the LDS-form angle cells stay below both onsets, the scratch form is beyond both
    for c in MIE:
        if c.startswith("angles-"):
            i = mie_oracle(c)["info"]
            assert np.all(i[:, 1] == (0 if c.endswith("-lds") else 1)), c


def test_zero_crossing_share_is_capped():
    """The escape of record_report applies to at most 1 % of a cell's I, Q, U elements, in every cell of the table (decided
    from the oracle alone)."""
    worst = 0.0
    for c in MIE:
        m = near_zero(mie_oracle(c))
        share = m.sum() / (1.5 * m.size)
        worst = max(worst, share)
        assert share <= 0.01, (c, share)
    print("largest share of elements next to a zero crossing: %.4f" % worst)


# ---------------------------------------------------------------------------------------------------------------------
# k_mie on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def run_mie(pkg, nbmu, rn, in_, alphas, fill=0.0):
    """sosgpu_mie through capi.  Returns (rc, rec [na][4 + 3 W] float32, g [na]) on the host; outputs pre-filled with `fill`."""
    import torch
    xmu = np.ascontiguousarray(xmu_of(nbmu), dtype=np.float64)
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    dev = torch.device("cuda", 0)
    rec = torch.full((len(al), 4 + 3 * len(xmu)), fill, dtype=torch.float32, device=dev)
    g = torch.full((len(al),), fill, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = pkg.capi.lib().sosgpu_mie(0, nbmu, xmu.ctypes.data_as(C.c_void_p), float(rn), float(in_), len(al),
                                   al.ctypes.data_as(C.c_void_p), C.c_void_p(rec.data_ptr()), C.c_void_p(g.data_ptr()), st)
    torch.cuda.synchronize()
    return rc, rec, g


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(MIE))
def test_mie_records(gpu_pkg, oracle, cid):
    """sosgpu_mie against sos_oracle_mie, every record of the cell, field by field (record_report)."""
    nbmu, (rn, in_), alphas = MIE[cid]
    ref = mie_oracle(cid)
    rc, rec, g = run_mie(gpu_pkg, nbmu, rn, in_, alphas, fill=float("nan"))
    assert rc == 0, rc
    rec, g = rec.cpu().numpy(), g.cpu().numpy()
    fails, lines = record_report(rec, g, ref)
    print("mie %s: n_lds %d of %d; %s" % (cid, n_lds_of(alphas), len(alphas), "; ".join(lines)))
    assert not fails, fails
    if cid == "split-repeated":                                       # equal size parameters: identical records
        for lo, hi in ((0, 3), (3, 5), (5, 8)):
            assert np.all(rec[lo:hi] == rec[lo]) and np.all(g[lo:hi] == g[lo])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(REJECTED))
def test_mie_rejects_on_the_host(gpu_pkg, cid):
    """Lists sosgpu_mie must refuse before any launch: the outputs keep their fill."""
    alphas, code = REJECTED[cid]
    rc, rec, g = run_mie(gpu_pkg, 3, 1.45, -0.003, alphas, fill=-7.25)
    assert rc == code, (rc, code)
    assert bool((rec == -7.25).all()) and bool((g == -7.25).all())


# ---------------------------------------------------------------------------------------------------------------------
# k_granu_batch cells.  The records come from sosgpu_mie on a hand-made list that crosses every boundary of the step ladder.
# ---------------------------------------------------------------------------------------------------------------------
LADDER = [(0.1, 0.0001, 0.001), (1.0, 0.001, 0.01), (10.0, 0.01, 0.05), (30.0, 0.05, 0.1), (100.0, 0.1, 1.0)]
_SEGMENTS = [(0.094, 0.106), (0.94, 1.06), (9.4, 10.6), (29.4, 30.6), (97.0, 112.0)]


@functools.lru_cache(maxsize=None)
def granu_alphas():
    """257 ascending size parameters: stretches of the reference's grid around each ladder boundary."""
    al = np.concatenate([A.alpha_grid(a0, a1) for a0, a1 in _SEGMENTS])
    assert len(al) >= 257 and np.all(np.diff(al) > 0)
    return al[:257]


def step_of(a32):
    pas = np.float32(0.0001)
    for lim, st in ((0.10, 0.001), (1.00, 0.01), (10., 0.05), (30., 0.10), (100., 1.00)):
        if a32 > np.float32(lim):
            pas = np.float32(st)
    return float(pas)


def granu_steps():
    """(alpha REAL*4 as the record holds it, own step, the step the stop rule sees = the previous record's) per record."""
    a32 = granu_alphas().astype(np.float32)
    pas = np.array([step_of(a) for a in a32])
    return a32.astype(np.float64), pas, np.concatenate([[step_of(np.float32(0))], pas[:-1]])


def alphaf_for(nuse, na=257):
    """An upper limit whose stop rule ALPHA >= ALPHAF - PAS first holds at record `nuse` (none when nuse == na)."""
    a, _, pp = granu_steps()
    if nuse >= na:
        return 1.0e4
    return a[nuse] + pp[nuse] - 0.25 * (a[nuse] - a[nuse - 1] if nuse else a[0])


def rmax_for(nuse, wa):
    """A Junge rmax between the radii of records nuse - 1 and nuse."""
    a, _, _ = granu_steps()
    return 0.5 * (a[nuse - 1] + a[nuse]) * wa / 2.0 / math.pi


def first_after(boundary):
    return int(np.argmax(granu_steps()[0] > float(np.float32(boundary))))


LND = (1, 0.12, 0.45, -999.0)
NO_RMAX = 1.0e6


def _granu_cells():
    """id -> (nbmu, na, igranu, v1, v2, v3, wa, alphaf)"""
    cells = {}
    for k, nbmu in enumerate((1, 41, 42, 84, 85, 100)):                 # 6 nbmu + 6 outputs against 256 threads
        law = LND if k % 2 else (2, 0.05, 4.2, NO_RMAX)
        cells["outputs-nbmu%d" % nbmu] = (nbmu, 60, *law, 0.865, alphaf_for(50))
    for na in (1, 255, 256, 257):                                       # records against 256 threads, no stop and one short
        cells["na%d-nostop-lnd" % na] = (2, na, *LND, 0.55, alphaf_for(na, na))
        if na > 1:
            cells["na%d-stop-at-last-lnd" % na] = (2, na, *LND, 0.55, alphaf_for(na - 1))
            cells["na%d-stop-at-last-rmax" % na] = (2, na, 2, 0.05, 4.2, rmax_for(na - 1, 0.55), 0.55, 1.0e4)
    for nuse in (1, 23, 24, 25, 47, 48, 49):                            # the 24-wide unrolled record loop and its remainder
        cells["nuse%d-alphaf-lnd" % nuse] = (2, 257, *LND, 0.865, alphaf_for(nuse))
        cells["nuse%d-alphaf-junge" % nuse] = (2, 257, 2, 0.05, 4.2, NO_RMAX, 0.865, alphaf_for(nuse))
        cells["nuse%d-rmax-junge" % nuse] = (2, 257, 2, 0.002, 3.5, rmax_for(nuse, 0.865), 0.865, 1.0e4)
    a, pas, pp = granu_steps()
    for b, _, _ in LADDER:
        k = first_after(b)
        # the deciding record is the first after the boundary: it stops with the previous record's step ...
        cells["ladder%g-stops-at-first-after" % b] = (2, 257, *LND, 0.865, alphaf_for(k))
        # ... and with ALPHAF half way between alpha + previous step and alpha + own step it must NOT stop there (its own, ten
        # times larger step would stop it) but at the next record
        cells["ladder%g-passes-first-after" % b] = (2, 257, 2, 0.05, 4.2, NO_RMAX, 0.865, a[k] + 0.5 * (pp[k] + pas[k]))
    wa = 0.865
    cells["junge-rmax-before-alphaf"] = (2, 257, 2, 0.05, 4.2, rmax_for(40, wa), wa, alphaf_for(130))
    cells["junge-rmax-after-alphaf"] = (2, 257, 2, 0.05, 4.2, rmax_for(130, wa), wa, alphaf_for(40))
    r = a * wa / 2.0 / math.pi
    cells["junge-all-below-r0"] = (2, 257, 2, 2.0 * r[-1], 4.2, NO_RMAX, wa, 1.0e4)
    cells["junge-some-below-r0"] = (2, 257, 2, 0.5 * (r[99] + r[100]), 4.2, NO_RMAX, wa, 1.0e4)
    cells["junge-none-below-r0"] = (2, 257, 2, 0.5 * r[0], 4.2, NO_RMAX, wa, 1.0e4)
    return cells


GRANU = _granu_cells()
GRANU_INDEX = (1.45, -0.003)


def expected_nuse(cell):
    """The record count from plain arithmetic on the REAL*4 size parameters (no kernel, no oracle)."""
    nbmu, na, igranu, v1, v2, v3, wa, alphaf = cell
    a, _, pp = granu_steps()
    for i in range(na):
        if a[i] >= alphaf - pp[i] or (igranu == 2 and a[i] * wa / 2. / math.pi > v3):
            return i
    return na


def test_granu_table_covers_its_edges():
    a, pas, pp = granu_steps()
    assert len(a) == 257 and np.all(np.diff(a) > 0)
    out = sorted(6 * c[0] + 6 for k, c in GRANU.items() if k.startswith("outputs-"))
    assert out == [12, 252, 258, 510, 516, 606]
    assert out[1] < GRANU_THREADS < out[2] and out[3] < 2 * GRANU_THREADS < out[4] and out[5] > 2 * GRANU_THREADS
    nuse = {k: expected_nuse(c) for k, c in GRANU.items()}
    assert all(n >= 1 for n in nuse.values())
    nas = {c[1] for c in GRANU.values()}
    assert nas >= {1, GRANU_THREADS - 1, GRANU_THREADS, GRANU_THREADS + 1}
    for na in (1, 255, 256, 257):
        assert nuse["na%d-nostop-lnd" % na] == na
        if na > 1:
            assert nuse["na%d-stop-at-last-lnd" % na] == na - 1 == nuse["na%d-stop-at-last-rmax" % na]
            assert GRANU["na%d-stop-at-last-rmax" % na][7] == 1.0e4                  # reached through rmax alone
    for n in (1, 23, 24, 25, 47, 48, 49):
        for how in ("alphaf-lnd", "alphaf-junge", "rmax-junge"):
            assert nuse["nuse%d-%s" % (n, how)] == n, (n, how)
    assert {n % GRANU_UNROLL for n in (23, 24, 25, 47, 48, 49)} == {GRANU_UNROLL - 1, 0, 1}
    # stop rule at the ladder: the first record after each boundary has a step unlike the one the rule must use
    for b, lo, hi in LADDER:
        k = first_after(b)
        assert a[k - 1] <= float(np.float32(b)) < a[k] and pp[k] == float(np.float32(lo)) and pas[k] == float(np.float32(hi))
        assert nuse["ladder%g-stops-at-first-after" % b] == k
        c = GRANU["ladder%g-passes-first-after" % b]
        assert nuse["ladder%g-passes-first-after" % b] == k + 1
        assert a[k] >= c[7] - pas[k] and not a[k] >= c[7] - pp[k]             # the record's own step would stop one record early
    assert nuse["junge-rmax-before-alphaf"] == 40 and nuse["junge-rmax-after-alphaf"] == 40
    c1, c2 = GRANU["junge-rmax-before-alphaf"], GRANU["junge-rmax-after-alphaf"]
    assert expected_nuse(c1[:5] + (NO_RMAX,) + c1[6:]) == 130 and expected_nuse(c2[:7] + (1.0e4,)) == 130
    r = a * 0.865 / 2. / math.pi
    below = {k: int(np.sum(r <= GRANU["junge-%s-below-r0" % k][3])) for k in ("all", "some", "none")}
    assert below == dict(all=257, some=100, none=0)
    # batch
    assert [c for c, _ in BATCHES] == [1, 32, 33, 65] and 32 == 32 * 1 and 33 > 32 and 65 > 2 * 32
    for count, stride in BATCHES:
        jobs = batch_jobs(count)
        assert stride > 3 * max(j[0] for j in jobs) + 1
        if count > 1:
            assert len({j[0] for j in jobs}) > 1 and {j[1] for j in jobs} == {1, 2}


# batch: (count, work_stride); SOSGPU_GRANU_JOBS_PER_LAUNCH = 32
BATCHES = [(1, 3 * 257 + 1 + 5), (32, 3 * 257 + 1 + 37), (33, 3 * 257 + 1 + 37), (65, 1000)]


def batch_jobs(count):
    """(na, igranu, v1, v2, v3, wa, alphaf) per job: record-set prefixes of different length, both laws."""
    jobs = []
    for k in range(count):
        na = (257, 100, 24, 1, 255, 49)[k % 6]
        wa = 0.4 + 0.03 * k
        if k % 2:
            jobs.append((na, 2, 0.03 + 0.001 * k, 3.5 + 0.01 * k, NO_RMAX if k % 4 == 1 else rmax_for(max(na - 2, 1), wa), wa, 1.0e4))
        else:
            jobs.append((na, 1, 0.05 + 0.005 * k, 0.3 + 0.004 * k, -999.0, wa, alphaf_for(na - (k % 3), na)))
    return jobs


_RECORDS = {}


def granu_records(pkg, nbmu):
    """Device records of granu_alphas() at the nbmu-angle set, checked against the oracle once."""
    if nbmu not in _RECORDS:
        from oracle import oracle_ctypes as O
        rc, rec, g = run_mie(pkg, nbmu, *GRANU_INDEX, granu_alphas())
        assert rc == 0
        ref = O.mie(xmu_of(nbmu), *GRANU_INDEX, granu_alphas())
        fails, _ = record_report(rec.cpu().numpy(), g.cpu().numpy(), ref)
        assert not fails, fails
        _RECORDS[nbmu] = (rec, rec.cpu().numpy())
    return _RECORDS[nbmu]


def run_granu_batch(pkg, nbmu, rec, jobs, stride, fill=-7.25):
    """sosgpu_granu_batch: returns out [count][3 + 3 W] and the work rows [count][stride] (pre-filled with `fill`)."""
    import torch
    dev = torch.device("cuda", 0)
    count, w = len(jobs), 2 * nbmu + 1
    arr = (pkg.capi.GranuJob * count)()
    for k, (na, igranu, v1, v2, v3, wa, alphaf) in enumerate(jobs):
        arr[k] = pkg.capi.GranuJob(rec.data_ptr(), na, igranu, v1, v2, v3, wa, alphaf)
    out = torch.full((count, 3 + 3 * w), fill, dtype=torch.float64, device=dev)
    work = torch.full((count, stride), fill, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    pkg.capi.check(pkg.capi.lib().sosgpu_granu_batch(0, nbmu, count, arr, C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()),
                                                     stride, st), "sosgpu_granu_batch")
    torch.cuda.synchronize()
    return out.cpu().numpy(), work.cpu().numpy()


def run_granu(pkg, nbmu, rec, job):
    na, igranu, v1, v2, v3, wa, alphaf = job
    out = np.full(3 + 3 * (2 * nbmu + 1), -7.25)
    pkg.capi.check(pkg.capi.lib().sosgpu_granu(0, nbmu, na, C.c_void_p(rec.data_ptr()), igranu, v1, v2, v3, wa, alphaf,
                                               out.ctypes.data_as(C.c_void_p), None), "sosgpu_granu")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(GRANU))
def test_size_integral(gpu_pkg, oracle, cid):
    """sosgpu_granu against sos_oracle_granu on the device's own records at the bar of
    test_device_size_integral_vs_host_restatement (1e-13), the record count equal (read from the work row of a one-job batch,
    whose sums must be those of the single call bit for bit)."""
    nbmu, na, igranu, v1, v2, v3, wa, alphaf = GRANU[cid]
    rec, rec_host = granu_records(gpu_pkg, nbmu)
    job = (na, igranu, v1, v2, v3, wa, alphaf)
    want, nuse = oracle.granu(rec_host[:na], igranu, v1, v2, v3, wa, alphaf)
    assert nuse == expected_nuse(GRANU[cid]) and np.isfinite(want).all()
    got = run_granu(gpu_pkg, nbmu, rec, job)
    stride = 3 * na + 1 + 3
    out, work = run_granu_batch(gpu_pkg, nbmu, rec, [job], stride)
    w = 2 * nbmu + 1
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print("granu %s: nuse %d of %d, scalars rel %.2e, worst array err / max %.2e" % (
        cid, nuse, na, err[:3].max(), max(np.abs(got[3 + c * w:3 + (c + 1) * w] - want[3 + c * w:3 + (c + 1) * w]).max()
                                          / np.abs(want[3 + c * w:3 + (c + 1) * w]).max() for c in range(3))))
    assert int(work[0, 3 * na]) == nuse == work[0, 3 * na]
    assert np.all(work[0, 3 * na + 1:] == -7.25)
    assert np.array_equal(out[0], got)
    assert np.isfinite(got).all()
    for a, b in zip(got[:3], want[:3]):
        assert abs(a - b) <= 1e-13 * abs(b), (a, b)
    for c in range(3):
        a, b = got[3 + c * w:3 + (c + 1) * w], want[3 + c * w:3 + (c + 1) * w]
        assert np.allclose(a, b, rtol=1e-13, atol=1e-15 * np.abs(b).max()), (c, np.abs(a - b).max())


@pytest.mark.gpu
@pytest.mark.parametrize("count,stride", BATCHES, ids=["count%d" % c for c, _ in BATCHES])
def test_size_integral_batch(gpu_pkg, oracle, count, stride):
    """sosgpu_granu_batch with jobs of different record count and law and a work stride larger than needed: each job bit-equal
    to the single call and at the oracle's record count, the doubles of its work row beyond 3 nalpha + 1 left untouched."""
    nbmu = 42
    rec, rec_host = granu_records(gpu_pkg, nbmu)
    jobs = batch_jobs(count)
    out, work = run_granu_batch(gpu_pkg, nbmu, rec, jobs, stride)
    for k, job in enumerate(jobs):
        na = job[0]
        single = run_granu(gpu_pkg, nbmu, rec, job)
        _, nuse = oracle.granu(rec_host[:na], *job[1:])
        assert nuse >= 1 and np.isfinite(single).all()
        assert np.array_equal(out[k], single), k
        assert work[k, 3 * na] == nuse, (k, work[k, 3 * na], nuse)
        assert np.all(work[k, 3 * na + 1:] == -7.25), k
        assert np.isfinite(work[k, :3 * na]).all() and not np.any(work[k, :3 * na] == -7.25), k
