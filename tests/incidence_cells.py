"""The cells of test_incidence_sweep: literal inputs, and the oracle's order-0 solves of every (bin, incidence) pair of them.

A cell is one call of solver.diffuse_transmissions_many / spherical_albedo_many: a list of parent contexts, and groups of bins
(one upload_bins call each) that solver.concat_profiles joins.  `ctx_of_group` names the parent of a group, so a cell with more
groups than contexts has an interleaved, unsorted ctx_of_bin."""
import numpy as np

import cases
import test_albedo_many as A
import test_trans_many as T
import test_variant_matrix as vm

S = cases.S
OS_NB, G = 16, 0.7

# The multi-context solver's routes, one cell each: (route, N, padded level count lp).  The route is the plan's layout
# (test_variant_matrix.route's naming); the shared-tile form SPLIT is ONE kernel that loops over the context's five or six row
# tiles, and counts as two routes here, ":5" and ":6".
LAYOUT_TABLE = [
    ("os<4,1,2>", 21, 32),
    ("os<4,2,2,SPLIT>:5", 22, 32),
    ("os<4,2,2,SPLIT>:6", 27, 32),
    ("os<4,2,2>", 33, 32),
    ("os<8,2,2>", 43, 32),
    ("os<4,1,4>", 21, 64),
    ("os<8,1,4>", 22, 48),
    ("stream<4,1,4>", 21, 80),
    ("stream<4,2,5>", 22, 80),
    ("stream<4,2,6>", 27, 80),
    ("stream<4,2,8>", 33, 80),
    ("stream<8,2,16>", 43, 48),
]
# what a parent carries and a child must not: a Lambert albedo, a Fresnel interface (f11sun, f12sun, fres), surface matrices
GROUNDS = (dict(ro=0.1), dict(ro=0.1, ifresnel=1, ind_surf=1.34), dict(ro=0.05, matrices=True))
K_ABS = (0.3, 2.0)                             # gas absorption of the NT = 1 and the NT = lp - 1 bin of a layout cell


def _name(route):
    return route.replace("<", "_").replace(">", "").replace(",", "_").replace(":", "_rt")


def _ctx(mu, w, n0, os_nb=OS_NB, g=G, ipolar=1, **ground):
    return dict(mu=np.asarray(mu), w=np.asarray(w), n0=int(n0), os_nb=os_nb, g=g, ipolar=ipolar, ground=dict(ground),
                phase=S.hg_phase(os_nb, g))


def _rescaled(h, x, y, os_nb=OS_NB):
    """test_trans_many._profiles' rescale, rows [nb][L]."""
    h, x, y, _ = S.rescale_profile(np.atleast_2d(h), np.atleast_2d(x), np.atleast_2d(y), 0.3, 0.95, 0.93, os_nb)
    return h, x, y


def _group(c, prof, nt=None):
    h = prof[0]
    return dict(c=c, prof=prof, nt=np.full(h.shape[0], h.shape[1] - 1, dtype=np.int32) if nt is None else np.asarray(nt, np.int32))


def _layout_cell(i, route, n, lp):
    sun_last = i % 2 == 1
    mu, w, n0 = vm._angles(n, sun_last)
    rows = [np.zeros((2, lp)) for _ in range(3)]
    for b, (nt, k) in enumerate(zip((1, lp - 1), K_ABS)):
        h, x, y, _ = S.profile(nt, tau_a=0.3, k_abs=k)
        for a, v in zip(rows, _rescaled(h, x, y)):
            a[b, :nt + 1] = v[0]
    return dict(name=_name(route), route=route, n=n, lp=lp, sun="last" if sun_last else "first",
                ctxs=[_ctx(mu, w, n0, **GROUNDS[i % 3])], groups=[_group(0, tuple(rows), nt=(1, lp - 1))], ctx_of_group=[0])


def _user_ctx(theta, **kw):
    return _ctx(*T._user_angles(*S.gauss_angles(24, theta), (12.5, 61.0)), **kw)


def _build():
    cells = [_layout_cell(i, *row) for i, row in enumerate(LAYOUT_TABLE)]
    # what SHAPES of test_trans_many / test_albedo_many hold only bit for bit against the per-direction loop
    for nt, lp in ((20, 32), (70, 80)):
        cells.append(dict(name="user_angles_nt%d" % nt, route=None, n=27, lp=lp, sun="interior",
                          ctxs=[_ctx(*T._angles("n27_user"), g=0.6, ro=0.2)], groups=[_group(0, T._profiles(3, nt, OS_NB))],
                          ctx_of_group=[0]))
    cells.append(dict(name="sun_on_node", route=None, n=24, lp=32, sun="interior",
                      ctxs=[_ctx(*T._angles("n24_sun_on_node"), g=0.6, ro=0.2)], groups=[_group(0, T._profiles(2, 20, OS_NB, seed=3))],
                      ctx_of_group=[0]))
    # three parents of N = 27 (24 Gauss nodes, the sun, two user directions) that differ in OS_NB, g, solar angle, polarisation
    # and ground; six groups, so ctx_of_bin = 2 0 1 1 0 2 1; the NT = 20 bins ride the streamed kernel next to the NT = 70 ones
    ctxs = [_user_ctx(35.0, os_nb=16, g=0.6, ro=0.1, ifresnel=1, ind_surf=1.34),
            _user_ctx(62.0, os_nb=48, g=0.75, ro=0.05, matrices=True),
            _user_ctx(8.0, os_nb=24, g=0.5, ro=0.1, ipolar=0)]
    plan = [(2, 1, 20, 21), (0, 1, 70, 22), (1, 2, 20, 23), (0, 1, 20, 24), (2, 1, 70, 25), (1, 1, 70, 26)]
    cells.append(dict(name="table", route=None, n=27, lp=80, sun="interior", ctxs=ctxs,
                      groups=[_group(c, T._profiles(nb, nt, ctxs[c]["os_nb"], seed=seed)) for c, nb, nt, seed in plan],
                      ctx_of_group=[c for c, _, _, _ in plan]))
    # total depths ~30 and ~200: tau / mu_J reaches ~1e4 at the smallest node, the direct beam underflows inside the column
    # (NT = 70: the same two bins in the streamed kernel, which has its own copy of the scattering-order loop)
    for name, nt, lp in (("opaque", 20, 32), ("opaque_streamed", 70, 80)):
        rows = [np.concatenate(a) for a in zip(*[_rescaled(*S.profile(nt, tau_a=0.3, k_abs=k)[:3]) for k in (30.0, 200.0)])]
        cells.append(dict(name=name, route=None, n=41, lp=lp, sun="interior", ctxs=[_ctx(*T._angles("n41"), g=0.6, ro=0.2)],
                          groups=[_group(0, tuple(rows))], ctx_of_group=[0]))
    for c in cells:
        c["bins"] = [dict(c=g["c"], nt=int(g["nt"][r]), h=g["prof"][0][r, :g["nt"][r] + 1], x=g["prof"][1][r, :g["nt"][r] + 1],
                          y=g["prof"][2][r, :g["nt"][r] + 1]) for g in c["groups"] for r in range(len(g["nt"]))]
        c["cob"] = np.array([b["c"] for b in c["bins"]], dtype=np.int32)
    return cells


CELLS = _build()
NAMES = [c["name"] for c in CELLS]
LAYOUT_CELLS = [c for c in CELLS if c["route"] is not None]


def by_name(name):
    return CELLS[NAMES.index(name)]


def route_multi(pkg, n, lp, nitems):
    """Route of the launch sosgpu_trans_spectrum and sosgpu_albedo_spectrum make for `nitems` (bin, direction) items of N
    directions at the padded level count lp -- Fourier order 0 only, no output slots, contexts from a device table -- as the
    library's plan names it (test_variant_matrix.route is the single-context form of this)."""
    import ctypes as C
    p = pkg.capi.SolvePlan()
    pkg.capi.check(pkg.capi.lib().sosgpu_debug_solve_plan(n, 0, nitems, lp, 0, 1, lp - 1, C.byref(p)), "sosgpu_debug_solve_plan")
    if p.big:
        assert p.form == pkg.capi.FORM_STREAM, (n, lp, p.form)             # a table launch takes the plain streamed form
        return "stream<%d,%d,%d>" % (p.nw, p.rtw, p.kht)
    assert p.form == pkg.capi.FORM_LDS
    tiles = (vm._round_up(3 * n, 8) + 15) // 16                             # rtph, as sosgpu_create derives it from N
    return "os<%d,%d,%d%s>" % (p.nw, p.rtw, p.ct, ",SPLIT" if p.split else "") + (":%d" % tiles if p.split else "")


# ---- the oracle's side ----------------------------------------------------------------------------------------------------

def solve(oracle, cell, b, j, mirrored=False, **change):
    """oracle.sos_os of bin b of the cell with direction j (1-based) as the incidence: Fourier order 0, black ground, the phase
    coefficients and ipolar of the bin's own context; `change` replaces keywords (the separation test's wrong inputs)."""
    bn = cell["bins"][b]
    cx = cell["ctxs"][bn["c"]]
    h, x, y = bn["h"], bn["x"], bn["y"]
    if mirrored:
        h, x, y = (a[0] for a in A.mirror(h, x, y))
    kw = dict(n0=j, ro=0.0, iborm=0, ipolar=cx["ipolar"])
    kw.update(change)
    return oracle.sos_os(cx["mu"], cx["w"], cx["os_nb"], h, x, y, *cx["phase"], **kw)


_REFS = {}


def queue(oracle, cell):
    """Every direction of every bin, on the profile and on its host mirror, queued once per session on the pool of
    test_variant_matrix (the oracle is plain C behind ctypes)."""
    if cell["name"] not in _REFS:
        _REFS[cell["name"]] = {m: [[vm._POOL.submit(solve, oracle, cell, b, j, m) for j in range(1, cell["n"] + 1)]
                                   for b in range(len(cell["bins"]))] for m in (False, True)}


def reference(oracle, cell):
    """dict(ier [2][nb][N], em, ep [nb][N] on the profile, em_below, ep_below [nb][N] on the mirror)."""
    queue(oracle, cell)
    r = _REFS[cell["name"]]
    if "em" not in r:
        res = {m: [[f.result() for f in row] for row in r[m]] for m in (False, True)}
        grid = lambda m, k: np.array([[x[k] for x in row] for row in res[m]])
        r = dict(ier=np.array([grid(False, "ier"), grid(True, "ier")]), em=grid(False, "emoins"), ep=grid(False, "eplus"),
                 em_below=grid(True, "emoins"), ep_below=grid(True, "eplus"))
        _REFS[cell["name"]] = r
    return r
