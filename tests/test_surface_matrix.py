"""The kernels on either side of the solve -- surface matrices (glitter.hip, land.hip), azimuth recomposition (trphi.hip) and
CKD aggregation (aggregate.hip) -- against the C oracle, at the shapes where their loops, wavefronts and chunks change.

One table of cells per kernel family, ids that name the cell.  The CPU tests check with the oracle alone that the tables
cover every axis value and corner, that no cell sits on a data-dependent stop (a tie two correct implementations could
resolve differently), and that the share of azimuth elements left out next to a zeroing threshold stays below 0.5 %.
A kernel trace of this module is kept in profiles/surface_matrix_kernel_stats.csv."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases

S = cases.S
EPS = 2.0 ** -52
MARGIN = 1e-9            # two correct implementations differ by ~1e-13 in the quantities the stops test


def angles(n, sun, users=0):
    """N directions: Gauss nodes + the sun (weight 0) + `users` user directions of weight 0 (SOS_ANGLES inserts them so)."""
    mu, w, n0 = S.gauss_angles(n - 1 - users, sun)
    for deg in (12.5, 57.3)[:users]:
        m = float(np.cos(np.deg2rad(deg)))
        pos = int(np.sum(mu > m))
        mu, w = np.insert(mu, pos, m), np.insert(w, pos, 0.0)
        n0 += pos < n0
    assert len(mu) == n and np.all(np.diff(mu) < 0) and abs(mu[n0 - 1] - np.cos(np.deg2rad(sun))) < 1e-12
    return mu, w, int(n0)


# ---------------------------------------------------------------------------------------------------------------------
# Cox-Munk glitter: (N, zero-weight user directions, sun, wind, ind, os_nb, os_ns, os_nm)
# ---------------------------------------------------------------------------------------------------------------------
# k_mat_reflexion asks for (os_nm + 1 + 12 (os_ns + 1)) * 8 bytes of dynamic LDS and has no static LDS; a workgroup of gfx950 has
# 160 KiB, so os_nm + 12 os_ns + 13 <= 20480.  With os_nb = 2 and os_nm = os_nb + os_ns that is os_ns <= 1574.
LDS_MAX = 160 * 1024
LDS_EDGE = (2, 1574, 1576)


def lds_bytes(os_ns, os_nm):
    return (os_nm + 1 + 12 * (os_ns + 1)) * 8


GLITTER = [
    (3, 0, 5.0, 0.0, 1.33, 2, 2, 4),                 # corner: smallest N, smallest orders
    (85, 0, 40.0, 0.0, 1.33, 200, 130, 330),         # corner: largest N, wind 0 (series open to os_nm), both strides looping
    (13, 0, 40.0, 0.5, 1.5, 24, 24, 48),
    (26, 2, 85.0, 2.0, 1.33, 80, 80, 160),
    (42, 0, 40.0, 7.0, 1.5, 127, 24, 151),           # os_nb + 1 = 128 = blockDim: one full trip
    (42, 0, 5.0, 15.0, 1.33, 128, 24, 152),          # one element into the second trip
    (13, 0, 85.0, 30.0, 1.5, 129, 130, 259),         # both strides into the second trip
    (85, 0, 85.0, 30.0, 1.5, 24, 24, 48),
    (85, 0, 5.0, 7.0, 1.33, 2, 2, 4),
    (3, 0, 40.0, 30.0, 1.5, 200, 130, 330),
    (13, 0, 40.0, 7.0, 1.33, 24, 24, 100),           # os_nm larger than os_nb + os_ns
    (3, 0, 40.0, 2.0, 1.33) + LDS_EDGE,              # the largest work area that fits the LDS of a workgroup
]


def gid(c):
    return "N%d%s-sun%g-w%g-ind%g-nb%d-ns%d-nm%d" % (c[0], "u%d" % c[1] if c[1] else "", c[2], c[3], c[4], c[5], c[6], c[7])


@functools.lru_cache(maxsize=None)
def glitter_oracle(cell):
    from oracle import oracle_ctypes as O
    n, users, sun, wind, ind, os_nb, os_ns, os_nm = cell
    mu, w, _ = angles(n, sun, users)
    ref = O.glitter(mu, w, wind, ind, os_nb, os_ns, os_nm)
    ref["margin"] = O.glitter_margin()
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# Land: (isurf, N, sun, (k0, k1, k2), coef_c, ind, os_nb, os_ns); os_nm = os_nb + os_ns
# ---------------------------------------------------------------------------------------------------------------------
TRIPLES = [(0.3, 0.0, 0.0), (0.3, 0.05, 0.0), (0.3, 0.0, 0.4), (0.25, 0.04, 0.3)]   # the goldens' is (0.2, 0.03, 0.25)
NEGATIVE_TRIPLE = (0.05, 0.1, 0.0)              # k0 + k1 f1 < 0 towards grazing incidence: the reference's IER = -1
LAND_ORDERS = [(2, 2), (24, 24), (80, 80), (140, 24)]


def _land_cells():
    cells, k = [], 0
    for isurf in (3, 4, 5, 7):
        for n in (3, 13, 25, 42, 85):
            os_nb, os_ns = LAND_ORDERS[(k + (n == 85)) % 4]       # N = 85 takes os_nb 140, 2, 24, 80 over the four models
            cells.append((isurf, n, (40.0, 75.0)[k % 2], TRIPLES[(k // 2) % 4], (1.0, 4.0, 8.0)[k % 3], (1.33, 1.5)[(k // 3) % 2],
                          os_nb, os_ns))
            k += 1
    return cells


LAND = _land_cells()
LAND_NEGATIVE = (7, 3, 40.0, NEGATIVE_TRIPLE, 4.0, 1.5, 24, 24)


def lid(c):
    return "surf%d-N%d-sun%g-k%g_%g_%g-C%g-ind%g-nb%d-ns%d" % (c[0], c[1], c[2], *c[3], c[4], c[5], c[6], c[7])


@functools.lru_cache(maxsize=None)
def land_oracle(cell):
    from oracle import oracle_ctypes as O
    isurf, n, sun, (k0, k1, k2), coef_c, ind, os_nb, os_ns = cell
    mu, w, _ = angles(n, sun)
    ref = O.land(isurf, mu, w, k0, k1, k2, coef_c, ind, os_nb, os_ns, os_nb + os_ns)
    ref["margin"] = O.land_margin()
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# Azimuth recomposition: (N, nf, nphi, tauout as thirds of tau, igli, ifresnel, ipolar, isurf, record scale)
# ---------------------------------------------------------------------------------------------------------------------
TR_OS_NB = 24                                     # smax + 1 = 25 orders
TR_TAU = 0.4
TR_WIND = 5.0
TR_LAND = dict(k0=0.25, k1=0.04, k2=0.3, coef_c=4.0)
TR_FLAGS = ([(g, f, p, 0) for g in (0, 1) for f in (0, 1) for p in (0, 1)]          # every combination of the three flags
            + [(0, 0, p, isurf) for isurf in (3, 4, 5, 7) for p in (1, 0)])         # each land model, polarised and not


def _trphi_cells():
    ns, nfs, touts = (3, 13, 31, 32, 42, 85), (TR_OS_NB + 1, 1, 2), (1, 0, 3)
    cells = []
    for k, (igli, ifres, ipol, isurf) in enumerate(TR_FLAGS):
        cells.append((ns[k % 6], nfs[k % 3], (361, 1)[(k // 3) % 2], touts[(k // 2) % 3], igli, ifres, ipol, isurf, 1.0))
    cells += [(85, TR_OS_NB + 1, 361, 1, 1, 0, 1, 0, 1.0),      # three wavefronts, every order, the glint
              (32, TR_OS_NB + 1, 361, 3, 0, 0, 1, 7, 1.0),      # W = 65: one lane into the second wavefront
              (31, TR_OS_NB + 1, 361, 0, 0, 1, 1, 0, 1.0),      # W = 63: one wavefront
              (85, TR_OS_NB + 1, 361, 1, 0, 0, 1, 0, 1e-14),    # Q, U around 1e-15, some I at and below 1e-99: zeroing, -999
              (13, 2, 1, 1, 0, 0, 1, 0, 1e-14)]
    return cells


TRPHI = _trphi_cells()


def tid(c):
    return "N%d-nf%d-nphi%d-tout%d_3-gli%d-fres%d-pol%d-surf%d-x%g" % c


def trphi_azimuths(nphi):
    """361: every degree of the reference's full view, with a negative azimuth and values on each side of sin(phi) = 0 put
    in place of some; 0, pi and 2 pi stay.  1: one negative azimuth."""
    if nphi == 1:
        return np.array([-0.7])
    phis = np.radians(np.arange(361.0))
    phis[1], phis[359] = 1e-12, 2 * np.pi - 1e-12
    phis[179], phis[181] = np.pi - 1e-12, np.pi + 1e-12
    phis[7], phis[8] = -0.5, -1e-12
    assert phis[0] == 0.0 and phis[180] == np.pi and phis[360] == 2 * np.pi
    return phis


def trphi_records(n, scale, seed):
    """Fourier records [smax+1][3][W] of realistic sign and decay: I > 0 at order 0 and falling off geometrically, Q and U a
    few per cent of I with either sign.  In the scaled cells one direction in four is 1e4 times brighter (its Q, U stay above
    the 1e-15 threshold), and a few directions have I = 0, I ~ 1e-101 and I ~ 1e-95 (around the 1e-99 threshold)."""
    rng = np.random.default_rng(seed)
    w = 2 * n + 1
    s = np.arange(TR_OS_NB + 1)[:, None, None]
    rec = rng.uniform(0.5, 1.5, (TR_OS_NB + 1, 3, w)) * 0.6 ** s * np.array([0.2, 0.02, 0.015])[None, :, None]
    rec[1:] *= rng.choice([-1.0, 1.0], (TR_OS_NB, 3, w)) * 0.5
    rec[:, 1:] *= rng.choice([-1.0, 1.0], (1, 2, w))
    rec[0, 2] = 0.0                                             # U has no order-0 term
    if scale != 1.0:
        rec *= scale
        rec[:, :, ::4] *= 1e4
        for j, f in ((1, 0.0), (2, 1e-87), (w - 2, 1e-81), (w - 3, 0.0)):
            rec[:, 0, j] *= f
        rec[:, 1:, 1] = 0.0                                     # I = Q = U = 0: both -999 values
    return rec


@functools.lru_cache(maxsize=None)
def trphi_oracle(cell):
    from oracle import oracle_ctypes as O
    n, nf, nphi, tout, igli, ifres, ipol, isurf, scale = cell
    mu, w, n0 = angles(n, 35.0)
    rec = trphi_records(n, scale, 1000 + n)
    phis = trphi_azimuths(nphi)
    land = TR_LAND if isurf else dict(k0=0.0, k1=0.0, k2=0.0, coef_c=0.0)
    out, cosd, pre = [], [], []
    for phi in phis:
        o = O.trphi_land(mu, rec[:nf], TR_TAU, TR_TAU * tout / 3.0, float(phi), igli=igli, n0=n0, wind=TR_WIND, ind_surf=1.34,
                         ifresnel=ifres, ipolar=ipol, isurf=isurf, **land)
        out.append(np.array(o["out"])); cosd.append(o["cosdif"]); pre.append(o["pre"])
    out, pre = np.array(out), np.array(pre)                     # [nphi][4][W], [nphi][3][W]
    # next to a zeroing threshold (within a factor 2) the two sides may fall on either side of it: left out of the comparison
    near = np.zeros(pre.shape, dtype=bool)
    near[:, 0] = (pre[:, 0] > 0.5e-99) & (pre[:, 0] < 2e-99)
    near[:, 1:] = (np.abs(pre[:, 1:]) > 0.5e-15) & (np.abs(pre[:, 1:]) < 2e-15)
    near[:, :, n] = False                                       # slot jj = 0 carries nothing
    return dict(out=out, cosdif=np.array(cosd), near=near, rec=rec, phis=phis, mu=mu, w=w, n0=n0)


# ---------------------------------------------------------------------------------------------------------------------
# Aggregate: (nb, cut): cut "one" = one segment, "cut" = segments that include length 1, "each" = nseg = nb
# ---------------------------------------------------------------------------------------------------------------------
AGG_NB = (1, 64, 128, 129, 192, 193, 257, 1000)
AGG = [(nb, cut, td) for nb in AGG_NB for cut, td in (("one", nb % 2 == 0), ("cut", nb % 2 == 1))] + [(64, "each", True), (257, "each", False)]
AGG_N, AGG_OS_NB = 13, 8                         # nel = 9 * 3 * 27 = 729: three blocks of 256, the last one partial


def aid(c):
    return "nb%d-%s-%s" % (c[0], c[1], "tdifmug" if c[2] else "notdifmug")


def agg_segments(nb, cut):
    if cut == "one":
        return [0, nb]
    if cut == "each" or nb < 4:
        return list(range(nb + 1))
    inner = sorted({1, 2, nb // 3, nb // 3 + 1, (2 * nb) // 3, nb - 1})     # lengths 1 at the head, middle and tail
    return [0] + [x for x in inner if 0 < x < nb] + [nb]


def agg_inputs(nb, seed):
    rng = np.random.default_rng(seed)
    w = 2 * AGG_N + 1
    smax = AGG_OS_NB
    norders = (np.arange(nb) * 7 % (smax + 1) + 1).astype(np.int32)         # ragged 1 .. smax + 1
    if nb >= 3:
        norders[[nb // 3, nb - 2]] = -1                                     # two failed bins
    rec = rng.uniform(-1.0, 1.0, (nb, smax + 1, 3, w))
    flux = rng.uniform(0.1, 1.0, (nb, 2))
    scal = rng.uniform(0.05, 2.0, (nb, 4))
    td = rng.uniform(0.0, 1.0, (nb, AGG_N))
    for b in range(nb):                                                     # what a kernel must not read
        rec[b, max(int(norders[b]), 0):] = np.nan
        if norders[b] < 0:
            flux[b], scal[b], td[b] = np.nan, np.nan, np.nan
    aik = rng.integers(1, 64, nb) / 4096.0                                  # dyadic: sum aik is exact in any order
    return dict(rec=rec, norders=norders, flux=flux, scal=scal, td=td, aik=aik)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: coverage, ties, threshold share, the host-side LDS bound
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_cover_every_axis_value_and_corner():
    g = GLITTER
    assert {c[0] for c in g} == {3, 13, 26, 42, 85} and all((c[1] == 2) == (c[0] == 26) for c in g)
    assert {c[2] for c in g} == {5.0, 40.0, 85.0} and {c[3] for c in g} == {0.0, 0.5, 2.0, 7.0, 15.0, 30.0}
    assert {c[4] for c in g} == {1.33, 1.5}
    assert {(c[5], c[6]) for c in g if c[7] == c[5] + c[6]} >= {(2, 2), (24, 24), (80, 80), (127, 24), (128, 24), (129, 130), (200, 130)}
    assert any(c[7] > c[5] + c[6] for c in g)
    assert any(c[0] == 85 and c[3] == 0.0 and c[5:] == (200, 130, 330) for c in g) and any(c[0] == 3 and c[5:] == (2, 2, 4) for c in g)
    assert any(c[0] == 85 and c[5:7] == (2, 2) for c in g) and any(c[0] == 3 and c[5:7] == (200, 130) for c in g)
    mu, w, _ = angles(26, 85.0, 2)
    assert np.sum(w == 0) == 3                                              # the sun and two user directions
    # the LDS edge: the cell fits, one more Fourier index of the Fresnel kernels does not
    assert g[-1][5:] == LDS_EDGE and lds_bytes(1574, 1576) <= LDS_MAX < lds_bytes(1575, 1577)
    assert all(lds_bytes(c[6], c[7]) <= LDS_MAX for c in g) and all(lds_bytes(c[7], c[6] + c[7]) <= LDS_MAX for c in LAND)

    ln = LAND
    assert {(c[0], c[1]) for c in ln} == {(s, n) for s in (3, 4, 5, 7) for n in (3, 13, 25, 42, 85)} and len(ln) == 20
    assert {c[3] for c in ln} == set(TRIPLES) and {c[4] for c in ln} == {1.0, 4.0, 8.0} and {c[5] for c in ln} == {1.33, 1.5}
    assert any(c[3][1] == 0 and c[3][2] == 0 for c in ln) and any(c[3][1] > 0 and c[3][2] == 0 for c in ln)
    assert any(c[3][1] == 0 and c[3][2] > 0 for c in ln) and any(c[3][1] > 0 and c[3][2] > 0 and c[3] != (0.2, 0.03, 0.25) for c in ln)
    assert {c[2] < 60 for c in ln} == {True, False} and {c[6] for c in ln} == {2, 24, 80, 140}
    assert {c[6] for c in ln if c[1] == 85} == {2, 24, 80, 140}
    for isurf in (3, 4, 5, 7):                                              # each model meets each axis value that matters to it
        sub = [c for c in ln if c[0] == isurf]
        assert {c[2] for c in sub} == {40.0, 75.0} and len({c[3] for c in sub}) >= 3

    t = TRPHI
    assert {c[0] for c in t} == {3, 13, 31, 32, 42, 85} and {c[1] for c in t} == {1, 2, TR_OS_NB + 1}
    assert {c[2] for c in t} == {1, 361} and {c[3] for c in t} == {0, 1, 3}
    assert {c[4:7] for c in t if c[7] == 0} == {(g_, f, p) for g_ in (0, 1) for f in (0, 1) for p in (0, 1)}
    assert {c[7] for c in t} == {0, 3, 4, 5, 7} and any(c[8] == 1e-14 for c in t)
    assert all(2 * c[0] + 1 > 64 for c in t if c[0] >= 32) and 2 * 31 + 1 < 64 and 2 * 85 + 1 > 128
    phis = trphi_azimuths(361)
    assert {0.0, np.pi, 2 * np.pi} <= set(phis) and phis.min() < 0
    assert any(np.sin(p) > 0 and abs(p - np.pi) < 1e-9 for p in phis) and any(np.sin(p) < 0 and abs(p - np.pi) < 1e-9 for p in phis)

    assert {c[0] for c in AGG if c[1] == "one"} == set(AGG_NB) and {c[0] for c in AGG if c[1] == "cut"} == set(AGG_NB)
    assert any(c[1] == "each" for c in AGG) and {c[2] for c in AGG} == {True, False}
    for nb in AGG_NB:
        seg = agg_segments(nb, "cut")
        assert seg[0] == 0 and seg[-1] == nb and np.all(np.diff(seg) > 0) and 1 in np.diff(seg)
        inp = agg_inputs(nb, nb)
        if nb >= 64:
            assert np.sum(inp["norders"] < 0) == 2 and set(inp["norders"][inp["norders"] > 0]) == set(range(1, AGG_OS_NB + 2))


@pytest.mark.parametrize("cell", GLITTER, ids=gid)
def test_glitter_cell_is_off_every_stop_tie(oracle, cell):
    """The oracle's smallest |tested / threshold - 1| over the per-level 1e-4 test, the 1e-3 closure that sets IL and the 1 %
    bisection test of the cell; a cell below the margin is replaced by nudging its wind, never dropped."""
    ref = glitter_oracle(cell)
    assert np.isfinite(ref["rsurf"]).all() and np.isfinite(ref["e"]).all()
    assert ref["margin"].min() > MARGIN, ref["margin"]


@pytest.mark.parametrize("cell", LAND + [LAND_NEGATIVE], ids=lid)
def test_land_cell_is_off_every_stop_tie(oracle, cell):
    """Same for SOS_FSF_ROUJEAN's two B1 tests and the Maignan quadrature; the triples keep the BRDF positive at every pair
    (the kernel divides by the samples), but for the one cell that is there for IER = -1."""
    ref = land_oracle(cell)
    assert ref["ier"] == (-1 if cell is LAND_NEGATIVE else 0)
    assert np.isfinite(ref["rsurf"]).all()
    assert ref["margin"].min() > MARGIN, ref["margin"]


@pytest.mark.parametrize("cell", TRPHI, ids=tid)
def test_trphi_threshold_share(oracle, cell):
    """Elements whose pre-threshold |Q|, |U| lies within a factor 2 of 1e-15, or XIT within a factor 2 of 1e-99, are left out of
    the GPU comparison: at most 0.5 % of a cell.  The scaled cells must reach both sides of the thresholds and -999."""
    ref = trphi_oracle(cell)
    n = cell[0]
    assert np.isfinite(ref["out"]).all()
    assert ref["near"].mean() <= 0.005, ref["near"].mean()
    if cell[8] != 1.0:
        out = np.delete(ref["out"], n, axis=2)
        assert (out[:, 0] == 0).any() and (out[:, 0] > 0).any()
        for q in (1, 2):
            assert (out[:, q] == 0).any() and (np.abs(out[:, q]) >= 1e-15).any()
        from oracle import oracle_ctypes as O
        assert O.polar(0.0, 0.0, 0.0)[:2] == (-999.0, -999.0)


def test_surface_entries_refuse_a_work_area_beyond_the_lds(pkg):
    """sosgpu_glitter / sosgpu_land_surface return SOSGPU_E_ARG on the host, before any device work, for a shape whose
    k_mat_reflexion work area does not fit a workgroup's LDS (no kernel runs: the refusal precedes even the device lookup)."""
    L = pkg.capi.lib()
    mu, w, _ = angles(3, 40.0)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    buf = np.zeros(16)
    land = pkg.surface.land_model(7, 0.3, 0.0, 0.0, coef_c=4.0)
    ier = C.c_int32(0)
    for os_nb, os_ns, os_nm in [(2, 1575, 1577), (2, 1998, 2000), (200, 1540, 2000)]:
        assert lds_bytes(os_ns, os_nm) > LDS_MAX
        assert L.sosgpu_glitter(0, 3, dp(mu), dp(w), 2.0, 1.33, os_nb, os_ns, os_nm, dp(buf), dp(buf), dp(buf), None) == -1
        assert L.sosgpu_land_surface(0, C.byref(land), 3, dp(mu), dp(w), 1.5, os_nb, os_ns, os_nm, dp(buf), C.byref(ier), None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cell", GLITTER, ids=gid)
def test_glitter_matrix(gpu_pkg, oracle, cell):
    """surface.glitter_matrices against oracle.glitter: IL identical, E at 1e-12 max, REAL*4 matrices with fewer than 1e-3
    differing elements and at most 2e-7 scale apart, everything finite."""
    n, users, sun, wind, ind, os_nb, os_ns, os_nm = cell
    mu, w, _ = angles(n, sun, users)
    ref = glitter_oracle(cell)
    out = gpu_pkg.surface.glitter_matrices(mu, w, wind, ind, os_nb, os_ns, os_nm)
    il, e, rs = out["il"].cpu().numpy(), out["e"].cpu().numpy(), out["rsurf"].cpu().numpy()
    assert np.isfinite(e).all() and np.isfinite(rs).all() and np.isfinite(ref["e"]).all() and np.isfinite(ref["rsurf"]).all()
    diff = rs != ref["rsurf"]
    scale = np.abs(ref["rsurf"]).max()
    err = np.abs(rs.astype(np.float64) - ref["rsurf"]).max()
    print("glitter %s: IL %d..%d, E err %.2e, flips %.2e, err/scale %.2e" % (gid(cell), ref["il"].min(), ref["il"].max(),
          np.abs(e - ref["e"]).max() / np.abs(ref["e"]).max(), diff.mean(), err / scale))
    assert np.array_equal(il, ref["il"]), np.flatnonzero(il != ref["il"])[:8]
    assert np.abs(e - ref["e"]).max() <= 1e-12 * np.abs(ref["e"]).max()
    assert diff.mean() < 1e-3, (diff.mean(), np.unique(np.argwhere(diff)[:, 0])[:16])
    assert err <= 2e-7 * scale, err / scale


@pytest.mark.gpu
@pytest.mark.parametrize("cell", LAND, ids=lid)
def test_land_matrix(gpu_pkg, oracle, cell):
    """surface.land_matrices against oracle.land at the bars of test_land_matrices_vs_reference_file: flips < 2e-2, 4e-7 scale,
    zero pattern; no IER."""
    import torch
    isurf, n, sun, (k0, k1, k2), coef_c, ind, os_nb, os_ns = cell
    mu, w, _ = angles(n, sun)
    ref = land_oracle(cell)["rsurf"]
    got = gpu_pkg.surface.land_matrices(gpu_pkg.surface.land_model(isurf, k0, k1, k2, coef_c=coef_c), mu, w, ind, os_nb, os_ns,
                                        os_nb + os_ns)              # raises ValueError on IER = -1: no cell here may
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
    scale = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("land %s: flips %.2e, err/scale %.2e" % (lid(cell), np.mean(got != ref), err.max() / scale))
    assert err.max() <= 4e-7 * scale, err.max() / scale
    assert np.mean(got != ref) < 2e-2
    assert np.array_equal(got == 0, ref == 0) or np.mean((got == 0) != (ref == 0)) < 1e-3


@pytest.mark.gpu
def test_land_negative_brdf_raises(gpu_pkg, oracle):
    """The reference's IER = -1 (SOS_ROUJEAN.F:548): where the oracle meets a negative sample the GPU entry raises."""
    isurf, n, sun, (k0, k1, k2), coef_c, ind, os_nb, os_ns = LAND_NEGATIVE
    assert land_oracle(LAND_NEGATIVE)["ier"] == -1
    mu, w, _ = angles(n, sun)
    with pytest.raises(ValueError, match="IER = -1"):
        gpu_pkg.surface.land_matrices(gpu_pkg.surface.land_model(isurf, k0, k1, k2, coef_c=coef_c), mu, w, ind, os_nb, os_ns,
                                      os_nb + os_ns)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", TRPHI, ids=tid)
def test_trphi_matrix(gpu_pkg, oracle, cell):
    """SosContext.trphi against oracle.trphi_land.  I, Q, U at 1e-9 |ref| + 1e-12 max(1, max |ref|) -- in the scaled cells the
    absolute term is scaled with the records, or it would pass anything -- but for the elements next to a zeroing threshold;
    ANGDIFF by the conditioned bound of acos; outputs 4..6 against oracle.polar of the GPU's own I, Q, U."""
    import torch
    n, nf, nphi, tout, igli, ifres, ipol, isurf, scale = cell
    ref = trphi_oracle(cell)
    mu, w, n0, phis = ref["mu"], ref["w"], ref["n0"], ref["phis"]
    al, be, ga, ze = S.hg_phase(TR_OS_NB, 0.6)
    cx = gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, ifresnel=ifres, ipolar=ipol, ind_surf=1.34)
    land = gpu_pkg.surface.land_model(isurf, TR_LAND["k0"], TR_LAND["k1"], TR_LAND["k2"], coef_c=TR_LAND["coef_c"]) if isurf else None
    rec = torch.from_numpy(ref["rec"][:nf].copy())
    out = cx.trphi(rec, nf, TR_TAU, TR_TAU * tout / 3.0, phis, igli=igli, wind=TR_WIND, land=land).cpu().numpy()
    cx.close()
    assert out.shape == (len(phis), 7, 2 * n + 1) and np.isfinite(out).all()
    assert np.all(out[:, :, n] == 0)                                        # slot jj = 0
    dirs = np.arange(2 * n + 1) != n
    worst = 0.0
    for q in range(3):
        r, g_ = ref["out"][:, q][:, dirs], out[:, q][:, dirs]
        keep = ~ref["near"][:, q][:, dirs]
        tol = 1e-9 * np.abs(r) + 1e-12 * scale * max(1.0, np.abs(r).max() / scale)
        bad = (np.abs(g_ - r) > tol) & keep
        worst = max(worst, (np.abs(g_ - r) / tol)[keep].max())
        assert not bad.any(), (q, np.argwhere(bad)[:8], np.abs(g_ - r)[bad][:8])
        assert np.array_equal((g_ == 0)[keep], (r == 0)[keep]), q           # zeroed on the same elements
    c = ref["cosdif"][:, dirs]
    bound = (180 / np.pi) * 4 * EPS / np.maximum(np.sqrt(np.maximum(1 - c * c, 0.0)), np.sqrt(4 * EPS)) + 1e-9 * np.abs(ref["out"][:, 3][:, dirs])
    dang = np.abs(out[:, 3][:, dirs] - ref["out"][:, 3][:, dirs])
    print("trphi %s: worst I,Q,U err/tol %.2e, ANGDIFF err/bound %.2e, left out %.2e" % (tid(cell), worst, (dang / bound).max(),
          ref["near"].mean()))
    assert np.all(dang <= bound), (dang / bound).max()
    from oracle import oracle_ctypes as O
    rows = range(len(phis)) if len(phis) == 1 or scale != 1.0 else (0, 1, 7, 8, 90, 179, 180, 181, 270, 359, 360)
    seen = set()
    for k in rows:
        for jj in np.flatnonzero(dirs):
            xan, tpol, lpol = O.polar(out[k, 0, jj], out[k, 1, jj], out[k, 2, jj])
            seen.update(v for v in (xan, tpol) if v == -999.0)
            assert abs(out[k, 4, jj] - xan) <= 1e-9 * max(1.0, abs(xan)), (k, jj)
            assert abs(out[k, 5, jj] - tpol) <= 1e-9 * max(1.0, abs(tpol)), (k, jj)
            assert abs(out[k, 6, jj] - lpol) <= 1e-12 * scale + 1e-9 * abs(lpol), (k, jj)
    if scale != 1.0:
        assert -999.0 in seen                                               # the undefined values are reached


@pytest.mark.gpu
@pytest.mark.parametrize("cell", AGG, ids=aid)
def test_aggregate_matrix(gpu_pkg, oracle, cell):
    """SosContext.aggregate on a hand-filled batch: orders a bin did not run and every record of a failed bin hold NaN.
    Segmented path and nb <= 128: records bit-identical to oracle.aggregate.  Chunked path (one segment, nb > 128): within
    nchunk eps sum |aik rec| (chunks of 64; only the association of the outer sum differs).  sum aik, the two MAX slots and
    TDIFMUG exact; the tree-summed scalars within 256 eps sum |terms|."""
    import torch
    nb, cut, with_td = cell
    inp = agg_inputs(nb, nb)
    seg = agg_segments(nb, cut)
    mu, w, n0 = angles(AGG_N, 35.0)
    al, be, ga, ze = S.hg_phase(AGG_OS_NB, 0.6)
    cx = gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze)
    d = cx.device
    out = dict(rec=torch.from_numpy(inp["rec"]).to(d), norders=torch.from_numpy(inp["norders"]).to(d),
               flux=torch.from_numpy(inp["flux"]).to(d))
    o_rec, o_scal = cx.aggregate(out, inp["aik"], seg=None if cut == "one" else np.array(seg, dtype=np.int32), scal=inp["scal"],
                                 tdifmug=inp["td"] if with_td else None)
    o_rec, o_scal = o_rec.cpu().numpy(), o_scal.cpu().numpy()
    cx.close()
    assert o_rec.shape == (len(seg) - 1, AGG_OS_NB + 1, 3, 2 * AGG_N + 1) and o_scal.shape == (len(seg) - 1, 10 + AGG_N)
    assert np.isfinite(o_rec).all() and np.isfinite(o_scal).all()
    chunked = cut == "one" and nb > 128
    worst = 0.0
    for g_ in range(len(seg) - 1):
        b = np.arange(seg[g_], seg[g_ + 1])
        ok = b[inp["norders"][b] >= 0]
        exp = np.zeros((AGG_OS_NB + 1, 3, 2 * AGG_N + 1))
        if len(ok):
            r, _ = oracle.aggregate(inp["rec"][ok], inp["norders"][ok], inp["aik"][ok], np.zeros((len(ok), 7)))
            exp[:len(r)] = r
        if not chunked:
            assert np.array_equal(o_rec[g_], exp), (g_, np.abs(o_rec[g_] - exp).max())
        else:
            mass = np.nansum(np.abs(inp["aik"][ok, None, None, None] * inp["rec"][ok]), axis=0)
            bound = ((nb + 63) // 64) * EPS * mass
            worst = max(worst, (np.abs(o_rec[g_] - exp)[mass > 0] / bound[mass > 0]).max())
            assert np.all(np.abs(o_rec[g_] - exp) <= bound), (np.abs(o_rec[g_] - exp) / np.maximum(bound, 1e-300)).max()
        a, no = inp["aik"], inp["norders"]
        sc = o_scal[g_]
        assert sc[6] == a[ok].sum() and sc[7] == max(no[b].max(), 0) and sc[8] == -no[b].min() and sc[9] == 0
        terms = [a[ok] * inp["scal"][ok, 0], a[ok] * inp["flux"][ok, 0], a[ok] * inp["flux"][ok, 1], a[ok] * np.exp(-inp["scal"][ok, 1]),
                 a[ok] * np.exp(-inp["scal"][ok, 2]), a[ok] * np.exp(-inp["scal"][ok, 3])]
        for i, t in enumerate(terms):
            assert abs(sc[i] - t.sum()) <= 256 * EPS * np.abs(t).sum(), (g_, i)
        td = np.zeros(AGG_N)
        if with_td:
            for bb in ok:                                                   # bins in serial order, un-fused
                td = td + a[bb] * inp["td"][bb]
        assert np.array_equal(sc[10:], td), g_
    if chunked:
        print("aggregate %s: worst err / (nchunk eps sum|aik rec|) %.3f" % (aid(cell), worst))
