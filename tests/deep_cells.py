"""The cells of test_deep_bins: one batch per layout of the single-context solver whose seven bins climb from a transparent
atmosphere (total optical depth 0.4) to depth 400, the oracle's solves of them, and the bar that holds each half of a record
to the oracle on that half's own scale.  Importable without a device.

A record is [order][3][2N+1].  Direction jj in -N..N lives at column jj + N (include/sosgpu.h): columns 0 ... N-1 are the
`down` half -- the radiance leaving the column downwards, at the ground in the standard output (ZOUT = -1: "TOA up, ground
down") -- column N is the stored zero, columns N+1 ... 2N the `up` half, at the top in the standard output.  Under a bin of
depth 30 the down half is 1e-14 of the up half, under depth 400 it is 1e-138 of it, and cases.compare_records, whose absolute
floor is 1e-12 of max |I| over the whole record, accepts any finite number there.  compare_halves takes the floor of each half
from that half alone.

A cell is a batch in the form of test_variant_matrix.make_batch (so _upload / _context / _fetch take it), plus `k_abs`, the gas
depth of every bin, `zlev` and `alts`."""
import numpy as np

import cases
import incidence_cells as ic
import test_variant_matrix as vm

S = cases.S
OS_NB, G = 16, 0.7
THETA_S = 35.0
RESCALE = (0.3, 0.95, 0.93)                    # a_tronc, piz, piztr
TAU_A = 0.3
K_ABS = (0.0, 3.0, 10.0, 30.0, 100.0, 200.0, 400.0)
DEPTHS = (0.4, 3.4, 10.4, 30.4, 100.4, 200.4, 400.4)      # total depth of each bin after the rescale, to 0.05
K_BLIND = 30.0                                  # from this gas depth on the whole-record bar no longer sees the down half
K_ZLEV = 200.0                                  # the bin whose middle level is the altitude `zlev` of the cell
Z_MID = 7.0                                     # km: between two levels of every bin; the depth above it is ~35 at k = 200
TAU_MUS_MAX = 700.0                             # beyond it the reference's own formulation returns NaN
IPOLAR0 = "os<8,2,2>"                           # the cell without polarisation
HALVES = ("down", "up")
AIK = np.array([0.05, 0.25, 0.1, 0.2, 0.15, 0.05, 0.2])   # the band of the seven bins: unequal weights that sum to 1
TWIN_CELLS = ("os_4_1_4", "stream_4_2_6")       # one LDS-resident, one streamed cell for the two-context table
CONDITIONING_CELLS = ("os_4_1_2", "stream_4_1_4", "stream_8_2_16")     # (N, lp) = (21, 32), (21, 80), (43, 48)
CONDITIONING_K = (30.0, 200.0, 400.0)


def half(rec, n, which):
    """The `down` (columns 0 ... N-1) or `up` (columns N+1 ... 2N) half of records [...][2N+1], as a view."""
    assert rec.shape[-1] == 2 * n + 1 and which in HALVES
    return rec[..., :n] if which == "down" else rec[..., n + 1:]


def half_tolerance(ref, n, which, rtol=1e-9):
    """The project's rule on one half: rtol |ref| + rtol 1e-3 max |I_ref|, the maximum over that half, over all orders."""
    r = half(ref, n, which)
    return rtol * np.abs(r) + rtol * 1e-3 * np.abs(half(ref[:, 0], n, which)).max()


def half_excess(got, ref, rtol=1e-9):
    """{half: max |got - ref| / tolerance of that half}: at most 1 where compare_halves passes, inf where an entry is not finite
    or the two runs differ in their number of Fourier orders."""
    n = (ref.shape[-1] - 1) // 2
    if got.shape != ref.shape:
        return dict.fromkeys(HALVES, float("inf"))
    out = {}
    for which in HALVES:
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(half(got, n, which) - half(ref, n, which)) / half_tolerance(ref, n, which, rtol)
        out[which] = float("inf") if not np.isfinite(q).all() else float(q.max())
    return out


def compare_halves(got, ref, rtol=1e-9, what=""):
    """cases.compare_records on each half of the record on its own scale: |got - ref| <= rtol |ref| + rtol 1e-3 max |I_ref|
    with the maximum over that half, over all orders.  NaN on either side is a mismatch; the middle column is the stored zero.
    Returns half_excess."""
    assert got.shape == ref.shape and ref.ndim == 3 and ref.shape[1] == 3, (what, got.shape, ref.shape)
    n = (ref.shape[-1] - 1) // 2
    assert not got[..., n].any() and not ref[..., n].any(), "%s: the middle column is not zero" % what
    for which in HALVES:
        compare_half(got, ref, which, rtol, what)
    return half_excess(got, ref, rtol)


def compare_half(got, ref, which, rtol=1e-9, what=""):
    """The rule of compare_halves on the half `which` of the records alone."""
    assert got.shape == ref.shape and ref.ndim == 3 and ref.shape[1] == 3, (what, got.shape, ref.shape)
    n = (ref.shape[-1] - 1) // 2
    err = np.abs(half(got, n, which) - half(ref, n, which))
    tol = half_tolerance(ref, n, which, rtol)
    bad = ~(err <= tol)                        # (NaN on either side is a mismatch)
    assert not bad.any(), "%s: %d entries of the %s half exceed its tolerance; worst err/tol %.3g (max |I| of the half %.3g)" % (
        what, bad.sum(), which, (err / tol).max(), np.abs(half(ref[:, 0], n, which)).max())


def assert_bin_vs_oracle(got, k, rec, ref, records, what):
    """test_variant_matrix._assert_bin_vs_oracle with the per-half bar: row k of the fetched outputs `got`, its records `rec`,
    against the oracle's solve `ref` and its `records`.  Order counts exact, fluxes at 1e-9 |ref| + 1e-300."""
    f = len(records)
    assert np.isfinite(records).all() and np.isfinite(rec).all(), what
    assert ref["ier"] == 0 and int(got["norders"][k]) == f, (what, int(got["norders"][k]), f)
    assert np.array_equal(got["iglast"][k, :f], ref["ig_counts"]), (what, got["iglast"][k, :f], ref["ig_counts"])
    e = compare_halves(rec[:f], records, 1e-9, what)
    assert not rec[f:].any(), "%s: records past the orders run" % what
    assert abs(got["flux"][k, 0] - ref["emoins"]) <= 1e-9 * abs(ref["emoins"]) + 1e-300, (what, got["flux"][k, 0], ref["emoins"])
    assert abs(got["flux"][k, 1] - ref["eplus"]) <= 1e-9 * abs(ref["eplus"]) + 1e-300, (what, got["flux"][k, 1], ref["eplus"])
    return e


def small_half(records, n):
    """The half of the records with the smaller max |I|."""
    return min(HALVES, key=lambda which: np.abs(half(records[:, 0], n, which)).max())


def spoiled(records, n, factor):
    """A copy of the records with its small half multiplied by `factor`."""
    out = records.copy()
    half(out, n, small_half(records, n))[...] *= factor
    return out


# ---- the cells ------------------------------------------------------------------------------------------------------------

def profile(nt, k):
    """(h, xdel, ydel, zprof) of the bin of gas depth k on nt layers, as SOS_OS receives them."""
    h, x, y, z = S.profile(nt, tau_a=TAU_A, k_abs=k)
    h, x, y, iborm = S.rescale_profile(h, x, y, *RESCALE, OS_NB)
    assert iborm == OS_NB
    return h, x, y, z


def ground(i, n):
    """Boundary condition of cell i: Lambert / flat-sea Fresnel / surface matrices, by index."""
    kw = dict([dict(ro=0.1), dict(ro=0.05, ifresnel=1, ind_surf=1.34), dict(ro=0.02, imat_surf=1)][i % 3])
    if kw.get("imat_surf"):
        kw["rsurf"] = cases._surf_matrices(n, OS_NB, 71 + i)
    return kw


def _cell(i, route, n, lp):
    mu, w, n0 = S.gauss_angles(n - 1, THETA_S)
    kw = dict(ground(i, n), ipolar=0 if route == IPOLAR0 else 1)
    bins = [profile(lp - 1, k) for k in K_ABS]
    for h, _, _, _ in bins:
        assert h[-1] / mu[n0 - 1] < TAU_MUS_MAX
    nb = len(bins)
    zlev = float(bins[K_ABS.index(K_ZLEV)][3][(lp - 1) // 2])
    return dict(i=i, name=ic._name(route), route=route, layout=route.split(":")[0], n=n, lp=lp, mu=mu, w=w, n0=n0, os_nb=OS_NB,
                nt=np.full(nb, lp - 1, dtype=np.int32), iborm=np.full(nb, OS_NB, dtype=np.int32), bins=bins, kw=kw, zout=-1.0,
                k_abs=K_ABS, zlev=zlev, alts=[-1.0, Z_MID, zlev, 0.0], zo=Z_MID if i % 2 == 0 else zlev)


CELLS = [_cell(i, *row) for i, row in enumerate(ic.LAYOUT_TABLE)]
NAMES = [c["name"] for c in CELLS]
STREAMED = [c["name"] for c in CELLS if c["layout"].startswith("stream")]


def by_name(name):
    return CELLS[NAMES.index(name)]


def at(c, zout):
    """The cell with the output altitude `zout` (what _upload reads)."""
    return dict(c, zout=zout)


# ---- the oracle's side ------------------------------------------------------------------------------------------------------

def solve(oracle, c, k, zout=-1.0, zouts=None, mu=None, g=G):
    """oracle.sos_os of bin k of the cell at `zout` (sos_os_levels with `zouts`), with the tie margin of this very call; `mu`
    replaces the cell's cosines (the conditioning test), `g` the asymmetry of the phase function (the second context)."""
    h, x, y, z = c["bins"][k]
    args = (c["mu"] if mu is None else mu, c["w"], c["os_nb"], h, x, y) + tuple(S.hg_phase(c["os_nb"], g))
    kw = dict(c["kw"], n0=c["n0"], zprof=z, iborm=int(c["iborm"][k]))
    if zouts is not None:
        return oracle.sos_os_levels(*args, zouts, **kw)
    r = oracle.sos_os(*args, zout=zout, **kw)
    r["margin"] = oracle.stop_margin()                      # (the audit of the last call of this thread)
    return r


_REFS = {}


def queue(oracle, c, what="plain"):
    """The solves of the cell's seven bins, queued once per session on the pool of test_variant_matrix.  what: "plain" (ZOUT =
    -1), "zo" (the cell's own interior altitude c["zo"]), "mid" / "lev" (7 km / zlev), "levels" (the four altitudes in one
    solve), "g2" (plain, the phase function of the second context of the table twin)."""
    key = (c["name"], what)
    if key not in _REFS:
        how = dict(plain={}, zo=dict(zout=c["zo"]), mid=dict(zout=Z_MID), lev=dict(zout=c["zlev"]), levels=dict(zouts=c["alts"]),
                   g2=dict(g=0.8))[what]
        if what in ("mid", "lev") and c["zo"] == how["zout"]:
            _REFS[key] = queue(oracle, c, "zo")
        elif what == "zo" and (c["name"], "mid" if c["zo"] == Z_MID else "lev") in _REFS:
            _REFS[key] = _REFS[(c["name"], "mid" if c["zo"] == Z_MID else "lev")]
        else:
            _REFS[key] = [vm._POOL.submit(solve, oracle, c, k, **how) for k in range(len(c["bins"]))]
    return _REFS[key]


def reference(oracle, c, what="plain"):
    return [f.result() for f in queue(oracle, c, what)]
