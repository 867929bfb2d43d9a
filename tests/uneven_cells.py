"""The cells of test_uneven_grids: level grids whose layers differ in optical depth by up to nine decades, one batch per layout
of the single-context solver, and the oracle's solves of them.  Importable without a device.

synth.profile places the levels of a bin by bisection on that bin's own optical depth, so every layer of every other synthetic
test has the same dtau, and an index slip between the per-layer tables of the kernels (attenuation row, 1/dtau entry, level
vectors) changes nothing there.  The grids here are the ones the product makes: levels placed on the no-gas profile with the
gas added per bin (B, C), and a user's altitudes (D, E, F).

A cell is a batch in the form of test_variant_matrix.make_batch (so _upload / _context / _fetch take it), plus `kinds`, the
grid kind of every bin, and `slabs`, the (j0, j1) of the slab bins."""
import numpy as np

import cases
import incidence_cells as ic
import test_albedo_many as A
import test_variant_matrix as vm

S = cases.S
OS_NB, G = 16, 0.7
TAU_R, TAU_A, HR, HA, HG, ZTOA = 0.0948, 0.3, 8.0, 2.0, 4.0, 120.0
THETA_S = 35.0
RESCALE = (0.3, 0.95, 0.93)                    # a_tronc, piz, piztr
# Gas depth of each kind (why the slab holds 4: profiles/uneven_grid_parity.txt, section 1)
K_EQUAL, K_NOGAS_GRID, K_SLAB, K_THIN, K_THICK = 0.3, 2.0, 4.0, 0.3, 30.0
KINDS = ("equal", "nogas_grid", "slab", "user_thin", "user_thick", "mirror_thick", "two_layers")
TWO_LAYERS = dict(h=(3e-8, 4e-8, 12.0), xdel=0.4, ydel=0.4, zprof=(120.0, 50.0, 0.0))
ZOUT_SLAB, ZOUT_THIN = 2.0, 70.0              # ZOUT_SLAB where it lies inside the cell's slab, else the middle of slab layer j0
SECOND_SLAB = {"stream<4,1,4>": (62, 66)}      # the streamed cell with a second slab bin, across the second chunk edge
IPOLAR0 = "os<8,1,4>"                           # the cell without polarisation


def edge(lp):
    """The level the slab of a layout straddles: the column-tile edge of the two-tile LDS layouts (lp = 32), the first
    32-level chunk edge of the streamed kernel / the second tile edge of the four-tile LDS layouts otherwise."""
    return 16 if lp == 32 else 32


def slab_of(lp):
    return (edge(lp) - 2, edge(lp) + 2)


def slab_edge(slab):
    """The level a slab (j0, j1) straddles: 16 or 32 for slab_of(lp), the second chunk edge 64 for (62, 66)."""
    return (slab[0] + slab[1]) // 2


def zout_in_slab(z, slab):
    """An output altitude inside the slab (j0, j1) on the levels z: ZOUT_SLAB where that is one, else the middle of layer j0,
    whose upper neighbour is the thin layer j0 - 1."""
    j0, j1 = slab
    return ZOUT_SLAB if z[j1] < ZOUT_SLAB < z[j0] else float(np.round(0.5 * (z[j0] + z[j0 + 1]), 5))


def _tr(z):
    return TAU_R * np.exp(-z / HR)


def _ta(z):
    return TAU_A * np.exp(-z / HA)


def _columns(z, tg, dtg_toa):
    """h, xdel, ydel on the levels z for the cumulative gas depth tg(z), as synth.profile forms them (dtg_toa = -d tg / dz at the
    top), rounded to the 8 digits of the profile file and rescaled."""
    h = _tr(z) + _ta(z) + tg(z)
    dt = np.diff(h)
    x, y = np.zeros_like(h), np.zeros_like(h)
    x[1:] = np.diff(_ta(z)) / dt
    y[1:] = np.diff(_tr(z)) / dt
    d0 = TAU_R / HR * np.exp(-ZTOA / HR) + TAU_A / HA * np.exp(-ZTOA / HA) + dtg_toa
    x[0] = (TAU_A / HA * np.exp(-ZTOA / HA)) / d0
    y[0] = (TAU_R / HR * np.exp(-ZTOA / HR)) / d0
    return _rescaled(S._round_sig(h, 8), S._round_sig(x, 8), S._round_sig(y, 8))


def _rescaled(h, x, y, os_nb=OS_NB):
    h, x, y, iborm = S.rescale_profile(h, x, y, *RESCALE, os_nb)
    assert iborm == os_nb
    return h, x, y


def _exp_gas(k):
    return (lambda z: k * np.exp(-z / HG)), k / HG * np.exp(-ZTOA / HG)


def profile(kind, nt, slab=None):
    """(h, xdel, ydel, zprof) of one bin of `kind` on nt layers, as SOS_OS receives them."""
    if kind == "equal":
        h, x, y, z = S.profile(nt, tau_r=TAU_R, tau_a=TAU_A, k_abs=K_EQUAL, hr=HR, ha=HA, hg=HG, ztoa=ZTOA)
        return _rescaled(h, x, y) + (z,)
    if kind == "two_layers":
        assert nt == 2
        t = TWO_LAYERS
        return _rescaled(np.array(t["h"]), np.full(3, t["xdel"]), np.full(3, t["ydel"])) + (np.array(t["zprof"]),)
    if kind in ("nogas_grid", "slab"):
        z = S.profile(nt, tau_r=TAU_R, tau_a=TAU_A, k_abs=0.0, hr=HR, ha=HA, hg=HG, ztoa=ZTOA)[3]
    else:
        z = np.round(np.linspace(ZTOA, 0.0, nt + 1), 5)
    if kind == "nogas_grid":
        return _columns(z, *_exp_gas(K_NOGAS_GRID)) + (z,)
    if kind == "slab":
        j0, j1 = slab
        return _columns(z, lambda v: K_SLAB * np.clip((z[j0] - v) / (z[j0] - z[j1]), 0.0, 1.0), 0.0) + (z,)
    if kind == "user_thin":
        return _columns(z, *_exp_gas(K_THIN)) + (z,)
    h, x, y = _columns(z, *_exp_gas(K_THICK))
    if kind == "user_thick":
        return h, x, y, z
    assert kind == "mirror_thick", kind
    h, x, y = (a[0] for a in A.mirror(h, x, y))
    return h, x, y, np.round(ZTOA - z[::-1], 5)


def _settings(i, n, lp):
    """Boundary conditions of cell i, spread over the table by index: Lambert / flat-sea Fresnel / surface matrices, one cell
    without polarisation, every second cell with an output altitude, alternately in the slab's range and in the thin layers."""
    kw = dict(ipolar=0 if ic.LAYOUT_TABLE[i][0] == IPOLAR0 else 1)
    kw.update([dict(ro=0.1), dict(ro=0.05, ifresnel=1, ind_surf=1.34), dict(ro=0.02, imat_surf=1)][i % 3])
    if kw.get("imat_surf"):
        kw["rsurf"] = cases._surf_matrices(n, OS_NB, 51 + i)
    if i % 2 == 0:
        return kw, -1.0
    if (i // 2) % 2:
        return kw, ZOUT_THIN
    return kw, zout_in_slab(S.profile(lp - 1, tau_r=TAU_R, tau_a=TAU_A, k_abs=0.0, hr=HR, ha=HA, hg=HG, ztoa=ZTOA)[3], slab_of(lp))


def _cell(i, route, n, lp):
    mu, w, n0 = S.gauss_angles(n - 1, THETA_S)
    kw, zout = _settings(i, n, lp)
    kinds, slabs, bins = [], [], []
    second = SECOND_SLAB.get(route)
    for kind in KINDS:
        for slab in ((slab_of(lp), second) if kind == "slab" and second else (slab_of(lp),) if kind == "slab" else (None,)):
            kinds.append(kind)
            slabs.append(slab)
            bins.append(profile(kind, 2 if kind == "two_layers" else lp - 1, slab))
    nb = len(bins)
    return dict(i=i, name=ic._name(route), route=route, layout=route.split(":")[0], n=n, lp=lp, mu=mu, w=w, n0=n0, os_nb=OS_NB,
                nt=np.array([len(b[0]) - 1 for b in bins], dtype=np.int32), iborm=np.full(nb, OS_NB, dtype=np.int32), bins=bins,
                kw=kw, zout=zout, kinds=kinds, slabs=slabs)


CELLS = [_cell(i, *row) for i, row in enumerate(ic.LAYOUT_TABLE)]
NAMES = [c["name"] for c in CELLS]
STREAMED = [c["name"] for c in CELLS if c["layout"].startswith("stream")]
# one LDS-resident, one streamed (the one with two slab bins); both put out at 70 km, next to the straddled edge of the user grids
SEPARATION_CELLS = ("os_4_2_2", "stream_4_1_4")
WRONG_KINDS = ("slab", "user_thin", "user_thick", "mirror_thick")
CAPTURE_CELLS = ("os_4_2_2_SPLIT_rt5", "stream_4_2_5")


def by_name(name):
    return CELLS[NAMES.index(name)]


def dtau(c, k):
    return np.diff(c["bins"][k][0])


# ---- the oracle's side ------------------------------------------------------------------------------------------------------

def excess(a, b, rtol=1e-9):
    """max |a - b| / tolerance with the tolerance of cases.compare_records: rtol |b| + rtol 1e-3 max |I|.  At most 1 where
    compare_records passes; inf when the two runs differ in their number of Fourier orders."""
    if a.shape != b.shape:
        return float("inf")
    scale = np.abs(b[:, 0]).max()
    return float((np.abs(a - b) / (rtol * np.abs(b) + rtol * 1e-3 * scale)).max())


def solve(oracle, c, k, h=None, mu=None, zouts=None):
    """oracle.sos_os of bin k of the cell (sos_os_levels with `zouts`), with the tie margin of this very call; `h` and `mu`
    replace the bin's optical depths and the cell's cosines (the wrong inputs of the separation test, the perturbation)."""
    hh, x, y, z = c["bins"][k]
    args = (c["mu"] if mu is None else mu, c["w"], c["os_nb"], hh if h is None else h, x, y) + tuple(S.hg_phase(c["os_nb"], G))
    kw = dict(c["kw"], n0=c["n0"], zprof=z, iborm=int(c["iborm"][k]))
    if zouts is not None:
        return oracle.sos_os_levels(*args, zouts, **kw)
    r = oracle.sos_os(*args, zout=c["zout"], **kw)
    r["margin"] = oracle.stop_margin()                      # (the audit of the last call of this thread)
    return r


_REFS = {}


def queue(oracle, c):
    """The cell's bins, queued once per session on the pool of test_variant_matrix."""
    if c["name"] not in _REFS:
        _REFS[c["name"]] = [vm._POOL.submit(solve, oracle, c, k) for k in range(len(c["bins"]))]
    return _REFS[c["name"]]


def reference(oracle, c):
    return [f.result() for f in queue(oracle, c)]


def equal_grid(h):
    """The optical depths a kernel reading an equal grid would see."""
    return np.linspace(h[0], h[-1], len(h))


def swapped_at(h, j):
    """h with the depths of layers j - 1 and j (on either side of level j) exchanged."""
    out = np.array(h)
    out[j] = h[j - 1] + (h[j + 1] - h[j])
    return out


def separation(oracle, c):
    """[(bin, which wrong input, factor)]: by how many times compare_records' tolerance at 1e-9 the oracle's own solve of a wrong
    input misses its solve of the right one, for the slab, user and mirrored bins of the cell.  The wrong inputs: an equal grid
    of the same total depth, and the two layers at the straddled edge exchanged -- the edge the bin's own slab straddles in a
    slab bin, the layout's edge(lp) in the others."""
    queue(oracle, c)
    futs = []
    for k, kind in enumerate(c["kinds"]):
        if kind in WRONG_KINDS:
            h = c["bins"][k][0]
            futs.append((k, "equal grid", vm._POOL.submit(solve, oracle, c, k, h=equal_grid(h))))
            e = slab_edge(c["slabs"][k]) if kind == "slab" else edge(c["lp"])
            futs.append((k, "edge swapped", vm._POOL.submit(solve, oracle, c, k, h=swapped_at(h, e))))
    out = []
    for k, how, fut in futs:
        ref, got = reference(oracle, c)[k], fut.result()
        assert got["ier"] == 0, (c["name"], k, how)
        f = min(len(ref["records"]), len(got["records"]))
        out.append((k, how, excess(got["records"][:f], ref["records"][:f])))
    return out
