"""Flux conservation: a check of the interior-altitude outputs that needs none of this project's code as its reference.

In a conservatively scattering atmosphere (single-scattering albedo 1, no gas) over a black or a Lambert ground nothing is
absorbed above the ground, so the net flux

    F_net(z) = exp(-TAUOUT(z) / mu_s) + E-(z) - E+(z)

is the same at every altitude z.  What is left of max - min over the altitudes is the tau-discretisation of the successive-orders
integration.  The other tests of an interior altitude compare the device with sos_oracle_os_levels -- an extension of the oracle
written here, the Fortran reference only outputs the ground and the top of the atmosphere -- or with another path of the same
code; an error the two share (a field paired with the optical depth of the level next to it, exchanged hemispheres, the direct
term at the wrong depth, slots weighted with the aik of another altitude) passes them all and breaks this constant.

Black and Lambert grounds only.  With a Fresnel interface (and likewise with glitter or land matrices) the specularly reflected
direct beam is not part of the diffuse field E+, so F_net as formed above is not constant: the oracle gives 0.8714 at the top
and 0.8767 at the ground for the first cell with ifresnel = 1.

CPU (oracle only; these hold the conditions that keep the GPU tests honest): for every cell the oracle's own spread is at most
1 / 20 of the smallest direct-beam difference between neighbouring levels (the detection condition); its limits are exact
(E- = 0 at the top, E+ there and E- at the ground == the solve's own EPLUS / EMOINS, the two numbers the Fortran produces);
the bar of the GPU tests (4 x the oracle's spread) is exceeded by each of the errors above applied to the oracle's own numbers,
and 100-fold by a gas.
The standard-output row of a flux table (altitude -1) pairs the ground's down-going flux with the top's up-going one: its
flux_net is no net flux, which the oracle's own EMOINS / EPLUS state here for every cell.
GPU: A the kernel chain per cell, B the table launches with one flux call over contexts of two N in shuffled order, C the whole
pipeline (sos_proc_levels, sos_spectrum_levels with fluxes=True) at altitudes between levels."""
import math

import numpy as np
import pytest

import cases
import test_variant_matrix as vm
from test_level_flux import GOLD, host_flux

S = cases.S
PARITY = 1e-9                                  # the project's bar for records against the oracle
DETECT = 20                                    # detection condition: spread <= step / DETECT
BAR = 4                                        # GPU bar: device spread <= BAR x the oracle's spread


def _cell(name, ng=8, sun=35.0, nt=30, os_nb=16, g=0.6, tau_a=(0.3,), aik=(1.0,), ro=0.3, a_tronc=0.0, ipolar=1, levels=None):
    if levels is None:
        levels = (0, 1, 3, nt // 2, nt - 1, nt)
    return dict(name=name, ng=ng, sun=sun, nt=nt, os_nb=os_nb, g=g, tau_a=tau_a, aik=aik, ro=ro, a_tronc=a_tronc, ipolar=ipolar,
                levels=tuple(levels))


# Level indices, not kilometres: level 0 is the top (120 km), level NT the ground.  NT = 30 and 45 run in the LDS-resident
# solver (tau_a = 1 under a sun at 60 degrees needs the 45 levels: at NT = 30 its spread is 1 / 19 of its step), NT >= 64 in the
# streamed one, whose chunks hold 32 levels: 31 | 32 | 33 and 63 | 64 | 65 are both sides of its first two
# chunk edges (test_output_capture.positions), NT = 65 ends in a chunk of two levels, NT = 130 in one of three.
EDGES = (0, 1, 31, 32, 33, 63, 64, 65)
CELLS = [
    _cell("black", ro=0.0),
    _cell("lambert"),
    _cell("white", ro=1.0),
    _cell("thick_sun60_n13_nt45", ng=12, sun=60.0, nt=45, os_nb=24, g=0.7, tau_a=(1.0,)),
    _cell("n25", ng=24, os_nb=40, g=0.7),
    _cell("truncated", a_tronc=0.25),
    _cell("nopolar_nt90", nt=90, ipolar=0),
    _cell("rayleigh", tau_a=(0.0,)),                                   # IBORM = 2: the molecular operator pack
    _cell("nt65", nt=65, levels=EDGES),
    _cell("nt130", nt=130, levels=EDGES + (130,)),
    _cell("three_bins", tau_a=(0.1, 0.3, 0.8), aik=(0.5, 0.3, 0.2)),
    _cell("rayleigh_sun60_n13_nt65", ng=12, sun=60.0, nt=65, os_nb=24, tau_a=(0.0,), ro=0.1),   # ... in the streamed solver
]
IDS = [c["name"] for c in CELLS]
TABLE_GROUPS = (("black", "white"), ("n25",))                          # test B: one table launch per N (9 and 25)


def _by_name(name):
    return CELLS[IDS.index(name)]


_INPUTS = {}


def inputs(c, k_abs=0.0):
    """Angles, phase coefficients and the bins (h, xdel, ydel, iborm) of a cell.  The bins of one cell share the level
    altitudes of the first (their own differ with tau_a): the altitudes only choose level indices."""
    key = (c["name"], k_abs)
    if key not in _INPUTS:
        mu, w, n0 = S.gauss_angles(c["ng"], c["sun"])
        bins, zprof = [], None
        for ta in c["tau_a"]:
            h, x, y, z = S.profile(c["nt"], tau_a=ta, k_abs=k_abs)
            h, x, y, ib = S.rescale_profile(h, x, y, c["a_tronc"], 1.0, 1.0, c["os_nb"])
            bins.append((h, x, y, ib))
            zprof = z if zprof is None else zprof
        assert np.all(np.diff(zprof) < 0) and all(np.all(np.diff(b[0]) > 0) for b in bins), key
        _INPUTS[key] = dict(mu=mu, w=w, n0=n0, mus=float(mu[n0 - 1]), phase=S.hg_phase(c["os_nb"], c["g"]), bins=bins,
                            zprof=zprof, alts=[float(zprof[j]) for j in c["levels"]], aik=np.array(c["aik"], dtype=np.float64))
    return _INPUTS[key]


def _oracle_bin(oracle, c, p, b):
    h, x, y, ib = p["bins"][b]
    return oracle.sos_os_levels(p["mu"], p["w"], c["os_nb"], h, x, y, *p["phase"], p["alts"], n0=p["n0"], zprof=p["zprof"],
                                ro=c["ro"], iborm=ib, ipolar=c["ipolar"])


def direct(p, j):
    """The direct beam at level j: every bin's own exp(-h[j] / mu_s), weighted with its aik."""
    return float(sum(a * math.exp(-float(b[0][j]) / p["mus"]) for a, b in zip(p["aik"], p["bins"])))


def net(dirs, e):
    return np.array([d + em - ep for d, (em, ep) in zip(dirs, e)])


def spread(f):
    return float(np.max(f) - np.min(f))


def _reference(c, p, per_bin):
    """The oracle's numbers of a cell: rows[K][W] the aik-weighted order-0 intensity rows (summed in bin order, as the aggregate
    does), e[K][2] = host_flux of them, e_bin[nb][K][2], dirs[K], fnet[K], spread, and step: the smallest direct-beam difference
    between a requested level and a neighbour of it."""
    nt = c["nt"]
    rows = []
    for k in range(len(c["levels"])):
        row = np.zeros(2 * len(p["mu"]) + 1)
        for a, r in zip(p["aik"], per_bin):
            row = row + a * r["records"][k, 0, 0]
        rows.append(row)
    e = np.array([host_flux(p["mu"], p["w"], p["n0"], row) for row in rows])
    e_bin = np.array([[host_flux(p["mu"], p["w"], p["n0"], r["records"][k, 0, 0]) for k in range(len(c["levels"]))]
                      for r in per_bin])
    dirs = np.array([direct(p, j) for j in c["levels"]])
    step = min(abs(direct(p, j) - direct(p, i)) for j in c["levels"] for i in (j - 1, j + 1) if 0 <= i <= nt)
    f = net(dirs, e)
    return dict(per_bin=per_bin, rows=rows, e=e, e_bin=e_bin, dirs=dirs, fnet=f, spread=spread(f), step=step)


_REFS = {}


def reference(oracle, c, k_abs=0.0):
    """The oracle solves of every cell are queued on first use (vm._POOL: plain C behind ctypes), one levels call per bin."""
    if not _REFS:
        for cc in CELLS:
            pp = inputs(cc)
            _REFS[(cc["name"], 0.0)] = [vm._POOL.submit(_oracle_bin, oracle, cc, pp, b) for b in range(len(pp["bins"]))]
    key = (c["name"], k_abs)
    p = inputs(c, k_abs)
    if key not in _REFS:
        _REFS[key] = [vm._POOL.submit(_oracle_bin, oracle, c, p, b) for b in range(len(p["bins"]))]
    if isinstance(_REFS[key], list):
        _REFS[key] = _reference(c, p, [f.result() for f in _REFS[key]])
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_cells_are_what_they_claim(pkg):
    assert len(set(IDS)) == len(CELLS) == 12
    lds, streamed = set(), set()
    for c in CELLS:
        p = inputs(c)
        nt, lv = c["nt"], c["levels"]
        assert len(p["mu"]) == c["ng"] + 1 <= 25 and nt <= 130 and len(p["bins"]) <= 3, c["name"]
        assert lv[0] == 0 and lv[-1] == nt and list(lv) == sorted(set(lv)) and len(lv) <= 9, c["name"]
        assert abs(sum(c["aik"]) - 1.0) < 1e-15 and len(c["aik"]) == len(c["tau_a"])
        assert c["ro"] in (0.0, 0.1, 0.3, 1.0)                            # black or Lambert: no ifresnel, no surface matrices
        for h, x, y, ib in p["bins"]:
            assert len(h) == nt + 1 and ib == (2 if c["tau_a"] == (0.0,) else c["os_nb"])
            assert np.abs(x[1:] + y[1:] - 1.0).max() < 1e-7                # conservative: nothing but scattering in a layer
        # the altitudes land on the levels: level 0 as (1, weight 0), level j as (j, weight 1)
        jout, zz = pkg.solver.output_levels_host(p["zprof"][None, :], p["alts"])
        assert jout[:, 0].tolist() == [max(1, j) for j in lv] and zz[:, 0].tolist() == [0.0] + [1.0] * (len(lv) - 1), c["name"]
        (streamed if vm.route(len(p["mu"]), vm._round_up(nt + 1, 16)).startswith("stream") else lds).add(c["name"])
    assert {"nt65", "nt130", "nopolar_nt90", "rayleigh_sun60_n13_nt65"} == streamed and "rayleigh" in lds
    assert vm.route(9, vm._round_up(63 + 1, 16)).startswith("os")          # NT = 65 is two levels past the last LDS-resident grid
    for group in TABLE_GROUPS:                                             # a table launch: one N, one slot count, one IBORM_max
        cs = [_by_name(n) for n in group]
        assert len({(c["ng"], c["os_nb"], len(c["levels"]), c["nt"]) for c in cs}) == 1
        assert len({(c["ro"], c["g"]) for c in cs}) == len(cs)
    assert {_by_name(g[0])["ng"] + 1 for g in TABLE_GROUPS} == {9, 25}


@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_oracle_residual_and_detection_condition(oracle, c):
    """The oracle's spread of F_net is at most 1 / 20 of the smallest direct-beam step between neighbouring levels: a capture
    or a depth one level off moves F_net by at least 20 spreads.  A condition on the cell, not a measurement."""
    ref = reference(oracle, c)
    assert all(r["ier"] == 0 and r["records"].shape[:2][0] == len(c["levels"]) and r["records"].shape[1] > 0 for r in ref["per_bin"])
    print("%s: F_net %s spread %.3e step %.3e ratio %.1f" % (c["name"], ref["fnet"].tolist(), ref["spread"], ref["step"],
                                                             ref["step"] / ref["spread"]))
    assert np.isfinite(ref["fnet"]).all() and np.isfinite(ref["spread"])
    assert ref["spread"] <= ref["step"] / DETECT, (ref["spread"], ref["step"])


@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_oracle_limits_are_exact(oracle, c):
    """Bin by bin: no diffuse light comes down through the top, and the quadrature of the captured rows at the top and at the
    ground is the solve's own EPLUS / EMOINS, to the bit."""
    ref = reference(oracle, c)
    for b, r in enumerate(ref["per_bin"]):
        e = ref["e_bin"][b]
        assert e[0, 0] == 0.0, (c["name"], b)
        assert e[0, 1] == r["eplus"] and e[-1, 0] == r["emoins"], (c["name"], b, e[0, 1], r["eplus"], e[-1, 0], r["emoins"])
        assert r["emoins"] > 0.0 and r["eplus"] > 0.0


@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_bar_separates_right_from_wrong(oracle, c):
    """On the oracle's own numbers: the direct term one level up, one level down (all altitudes, then one altitude alone), the
    hemispheres exchanged -- each exceeds the bar of the GPU tests; a gas (k_abs = 0.3) exceeds it 100-fold."""
    ref = reference(oracle, c)
    p = inputs(c)
    nt, lv = c["nt"], c["levels"]
    bar = BAR * ref["spread"]
    for shift in (-1, 1):
        moved = np.array([direct(p, min(nt, max(0, j + shift))) for j in lv])
        assert spread(net(moved, ref["e"])) > bar, (c["name"], shift)
        for k, j in enumerate(lv):
            if 0 <= j + shift <= nt:
                one = ref["dirs"].copy()
                one[k] = moved[k]
                assert spread(net(one, ref["e"])) > bar, (c["name"], shift, j)
    swapped = np.array([host_flux(p["mu"], p["w"], p["n0"], row[::-1]) for row in ref["rows"]])
    assert np.array_equal(swapped, ref["e"][:, ::-1])
    assert spread(net(ref["dirs"], swapped)) > bar, c["name"]
    for k in range(len(lv)):                                               # ... and at one altitude alone
        one = ref["e"].copy()
        one[k] = swapped[k]
        assert spread(net(ref["dirs"], one)) > bar, (c["name"], lv[k])
    gas = reference(oracle, c, 0.3)
    print("%s: spread %.3e, with k_abs = 0.3 %.3e (F_net %.4f at the top, %.4f at the ground)"
          % (c["name"], ref["spread"], gas["spread"], gas["fnet"][0], gas["fnet"][-1]))
    assert gas["spread"] > 100 * bar and gas["fnet"][0] > gas["fnet"][-1]


@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_standard_output_row_is_no_net_flux(oracle, c):
    """The standard output pairs EMOINS at the ground with EPLUS at the top.  direct(ground) + EMOINS - EPLUS is therefore not
    the constant: it misses it by E+(top) - E+(ground), far beyond the bar (the pipeline test C forms the net fluxes at the
    ground and at the top from that row and the rows of 0 and 120 km instead)."""
    ref = reference(oracle, c)
    p = inputs(c)
    emoins = float(sum(a * r["emoins"] for a, r in zip(p["aik"], ref["per_bin"])))
    eplus = float(sum(a * r["eplus"] for a, r in zip(p["aik"], ref["per_bin"])))
    literal = ref["dirs"][-1] + emoins - eplus
    gap = ref["e"][0, 1] - ref["e"][-1, 1]
    print("%s: F_net %.6f, standard-output row %.6f, E+(top) - E+(ground) %.6f" % (c["name"], ref["fnet"][-1], literal, gap))
    assert abs(ref["fnet"][-1] - literal - gap) <= 1e-12
    assert abs(gap) > 100 * BAR * ref["spread"], (c["name"], gap)
    # ... while the two net fluxes that row takes part in are values of the constant
    both = np.append(ref["fnet"], [ref["dirs"][-1] + emoins - ref["e"][-1, 1], ref["dirs"][0] + ref["e"][0, 0] - eplus])
    assert spread(both) <= ref["spread"] + 1e-12


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _context(gpu_pkg, c, p):
    return gpu_pkg.SosContext(p["mu"], p["w"], p["n0"], *p["phase"], iborm_max=max(b[3] for b in p["bins"]), ro=c["ro"],
                              ipolar=c["ipolar"])


def _upload(cx, c, p):
    """upload_bins, plus the level altitudes on the device in make_profiles' layout [nb][lp]: output_levels then runs
    sosgpu_output_levels (k_output_levels) instead of the host rule."""
    import torch
    nb = len(p["bins"])
    bins = cx.upload_bins(np.array([b[0] for b in p["bins"]]), np.array([b[1] for b in p["bins"]]),
                          np.array([b[2] for b in p["bins"]]), iborm=np.array([b[3] for b in p["bins"]], dtype=np.int32),
                          zprof=np.tile(p["zprof"], (nb, 1)))
    z = np.zeros((nb, bins["lp"]))
    z[:, :c["nt"] + 1] = p["zprof"]
    bins["zprof"] = torch.from_numpy(z).to(cx.device)
    return bins


def _check_levels(c, lv):
    """The device's level table points at the cell's levels."""
    want = [max(1, j) for j in c["levels"]]
    assert (lv["jout"].cpu().numpy() == np.array(want, dtype=np.int32)[:, None]).all(), c["name"]
    assert (lv["zz"].cpu().numpy() == np.array([0.0] + [1.0] * (len(want) - 1))[:, None]).all(), c["name"]


def _check_cell(c, p, ref, e, tauout, flux_bins, what):
    """The assertions of test A on one context: e[K][2] of the flux kernel on the aggregated slots, tauout[K][nb] of
    output_levels, flux_bins[nb][2] the solve's own (EMOINS, EPLUS) per bin."""
    aik = p["aik"]
    dirs = np.array([float(sum(a * math.exp(-float(t) / p["mus"]) for a, t in zip(aik, tk))) for tk in tauout])
    f = net(dirs, e)
    print("%s: device spread %.3e, oracle spread %.3e, step %.3e (step / 20 over the device spread: %.1f)"
          % (what, spread(f), ref["spread"], ref["step"], ref["step"] / DETECT / max(spread(f), 1e-300)))
    print("%s: worst relative deviation of E-/E+ from the oracle %.3e" % (what, np.abs(e[ref["e"] != 0] / ref["e"][ref["e"] != 0] - 1).max()))
    assert np.isfinite(f).all() and spread(f) <= BAR * ref["spread"], (what, spread(f), ref["spread"], f.tolist())
    assert np.all(np.abs(e - ref["e"]) <= PARITY * np.abs(ref["e"])), (what, e.tolist(), ref["e"].tolist())
    emoins, eplus = float(np.sum(aik * flux_bins[:, 0])), float(np.sum(aik * flux_bins[:, 1]))
    assert e[0, 0] == 0.0, (what, e[0, 0])
    assert abs(e[0, 1] - eplus) <= PARITY * abs(eplus), (what, e[0, 1], eplus)
    assert abs(e[-1, 0] - emoins) <= PARITY * abs(emoins), (what, e[-1, 0], emoins)
    assert emoins > 0.0 and eplus > 0.0


def _check_scal(p, scal, tauout, flux_bins, what):
    """Columns 1, 2 and 5 of the aggregate's scalars per slot: sum aik EMOINS, sum aik EPLUS, sum aik exp(-TAUOUT) of THAT
    slot's TAUOUT.  <= 3 positive terms and one exp each: 1e-14 is some 40 ulp, a neighbouring level's depth is 1e-3 off."""
    aik = p["aik"]
    for k in range(len(tauout)):
        want = (float(np.sum(aik * flux_bins[:, 0])), float(np.sum(aik * flux_bins[:, 1])),
                float(sum(a * math.exp(-float(t)) for a, t in zip(aik, tauout[k]))))
        got = (scal[k][1], scal[k][2], scal[k][5])
        assert all(abs(g - w) <= 1e-14 * abs(w) for g, w in zip(got, want)), (what, k, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_kernel_chain_conserves_flux(gpu_pkg, oracle, c):
    """A: output_levels (on the device) -> solve_levels -> aggregate_levels -> level_flux_many per cell.  The direct term comes
    from the device's own TAUOUT.  Conservation within 4 x the oracle's spread of this cell (room for the 1e-9 parity of the
    records, far from the 20 x of the detection condition), E- and E+ within 1e-9 of the oracle's, E-(top) == 0.0, E+(top) and
    E-(ground) within 1e-9 of the solve's own EPLUS / EMOINS.  The NT = 65 and NT = 130 cells carry 8 and 9 altitudes: both
    sides of the streamed solver's first two chunk edges."""
    p = inputs(c)
    ref = reference(oracle, c)
    cx = _context(gpu_pkg, c, p)
    try:
        bins = _upload(cx, c, p)
        lv = cx.output_levels(bins, p["alts"])
        out = cx.solve_levels(bins, lv)
        rec, scal = cx.aggregate_levels(out, lv, p["aik"])
        e = gpu_pkg.solver.level_flux_many([(cx, rec[k, 0]) for k in range(len(p["alts"]))]).cpu().numpy()
        tauout, flux_bins = lv["tauout"].cpu().numpy(), out["flux"].cpu().numpy()
        levels = {k: lv[k].cpu() for k in ("jout", "zz")}
        assert (out["norders"].cpu().numpy() > 0).all()
        scal = scal[:, 0].cpu().numpy()
    finally:
        cx.close()
    _check_cell(c, p, ref, e, tauout, flux_bins, c["name"])
    _check_scal(p, scal, tauout, flux_bins, c["name"])
    # (after the physics: what the level table should hold, restated)
    _check_levels(c, levels)
    assert np.array_equal(tauout, np.array([[b[0][j] for b in p["bins"]] for j in c["levels"]])), c["name"]


@pytest.mark.gpu
def test_table_launches_and_one_flux_call_conserve_flux(gpu_pkg, oracle):
    """B: contexts of N = 9 (black and white ground) in one solve_spectrum_levels launch, the N = 25 cell in another -- a context
    table holds one N, sosgpu_ctx_table refuses a mixed one -- then the fluxes of all (context, altitude) jobs of both N in ONE
    level_flux_many call in shuffled job order.  The assertions of A per context: a slot, a segment or a job landing on its
    neighbour breaks the constant of that context."""
    import torch
    sv = gpu_pkg.solver
    ctxs, jobs = [], []
    try:
        for group in TABLE_GROUPS:
            cs = [_by_name(n) for n in group]
            cxs = [_context(gpu_pkg, c, inputs(c)) for c in cs]
            ctxs += cxs
            parts = [_upload(cx, c, inputs(c)) for cx, c in zip(cxs, cs)]
            lvs = [cx.output_levels(b, inputs(c)["alts"]) for cx, b, c in zip(cxs, parts, cs)]
            for c, lv in zip(cs, lvs):
                _check_levels(c, lv)
            table = sv.ContextTable(cxs)
            bins, cob, seg = sv.concat_bins(parts)
            levels = sv.concat_levels(lvs)
            nz, nb = levels["nz"], bins["nb"]
            aik = torch.ones(nb, dtype=torch.float64, device=cxs[0].device)
            out = cxs[0].alloc_outputs(nb)
            out["rec"] = torch.full((nz, nb, cxs[0].smax + 1, 3, cxs[0].w), float("nan"), dtype=torch.float64, device=cxs[0].device)
            rec, scal = sv.solve_spectrum_levels(table, bins, cob, seg, aik, levels, out=out)
            assert tuple(rec.shape)[:2] == (nz, len(cs))
            for g, (c, cx) in enumerate(zip(cs, cxs)):
                jobs += [(c, k, cx, rec[k, g], levels["tauout"][k, g:g + 1], out["flux"][g:g + 1], scal[k, g]) for k in range(nz)]
        with pytest.raises(gpu_pkg.capi.SosgpuError) as refused:
            sv.ContextTable([ctxs[0], ctxs[-1]])                           # N = 9 with N = 25
        assert refused.value.code == -1
        order = np.random.default_rng(5).permutation(len(jobs))
        assert not np.array_equal(order, np.arange(len(jobs)))
        got = sv.level_flux_many([(jobs[i][2], jobs[i][3]) for i in order]).cpu().numpy()
        e = np.empty_like(got)
        e[order] = got
        fetched = [(j[0], j[1], j[4].cpu().numpy(), j[5].cpu().numpy(), j[6].cpu().numpy()) for j in jobs]
    finally:
        for cx in ctxs:
            cx.close()
    assert len({j[0]["ng"] for j in jobs}) == 2
    for name in [n for g in TABLE_GROUPS for n in g]:
        c = _by_name(name)
        rows = [i for i, j in enumerate(fetched) if j[0] is c]
        assert [fetched[i][1] for i in rows] == list(range(len(c["levels"])))
        tauout = np.array([fetched[i][2] for i in rows])
        flux_bins = fetched[rows[0]][3]
        _check_cell(c, inputs(c), reference(oracle, c), e[rows], tauout, flux_bins, "table launch, " + name)
        _check_scal(inputs(c), [fetched[i][4] for i in rows], tauout, flux_bins, "table launch, " + name)


# C: the whole pipeline.  -1 is the standard output, 0 km the ground, 0.7, 3 and 8.5 km lie between levels of the product's own
# profile, the high one is the top itself (the -SOS.OutputAlt rule admits [0, 120] km): the standard output needs it, see nets().
PIPE_ALTS = [-1, 0.0, 0.7, 3.0, 8.5, 120.0]
PIPE_WA = (0.55, 0.67)
PIPE_BASE = {"-ANG.Rad.NbGauss": 24, "-ANG.Thetas": 35.0, "-SOS.View": 1, "-SOS.View.Phi": 0.0, "-AP.Psurf": 1013.0, "-AP.HR": 8.0,
             "-AP.AerHS.HA": 2.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.0, "-AER.Waref": 0.55, "-SURF.Type": 0,
             "-SURF.Alb": 0.1, "-SOS.IGmax": 100, "-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT"}
# the aerosol call: the model keywords the parameter checks ask for (those of the golden cfg2_lnd_lambert); aer_phase replaces it
PIPE_AER = {"-AER.AOTref": 0.3, "-ANG.Aer.NbGauss": 40, "-AER.Tronca": 1, "-AER.Model": 0, "-AER.MMD.SDtype": 1,
            "-AER.MMD.LNDradius": 0.3, "-AER.MMD.LNDvar": 0.6, "-AER.MMD.MRwa": 1.45, "-AER.MMD.MIwa": -0.003,
            "-AER.MMD.MRwaref": 1.45, "-AER.MMD.MIwaref": -0.003}
# the gas settings of the golden ckd_h2o_o2_25bins_flatsea (a 25-bin band at 15925 cm-1), on the Lambert ground
PIPE_GAS = {"-SOS_Main.Wa": 0.6279434850863422, "-AP.AbsProfile.Type": 1, "-AP.H2O": 2.5, "-AP.O3": 310.0, "-AP.SpectralResol": 10.0}


def _pipe_kwargs(rs, extra):
    return rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), dict(PIPE_BASE, **extra)), trace=False)


def nets(flux):
    """The values of the constant in the flux rows [K][5] of PIPE_ALTS: column flux_net of every altitude, and the two the
    standard output takes part in.  Row -1 pairs the down-going flux AT THE GROUND with the up-going flux AT THE TOP (elements 20
    and 21 of the 23-tuple), so its own flux_net is the net flux of no altitude: it falls short of the constant by
    E+(top) - E+(ground), conservative column or not (test_standard_output_row_is_no_net_flux: the oracle's EMOINS and EPLUS,
    the numbers the Fortran produces, say the same; on the MI355X the Rayleigh call at 0.55 um gives 0.8105 in that row against
    0.85759 in every other).  Its three numbers enter where they belong: its down-going total less the up-going flux of the 0 km
    row is the net flux at the ground, the down-going total of the 120 km row less its up-going flux the net flux at the top."""
    by = dict(zip(PIPE_ALTS, flux))
    return np.array([by[a][4] for a in PIPE_ALTS if a >= 0] + [by[-1][2] - by[0.0][3], by[120.0][2] - by[-1][3]])


def _span_and_d(flux):
    """Span of nets() -- all rows, the -1 row included -- and d: the smallest difference of flux_dir_down_tronc between two
    adjacent requested altitudes (the -1 row is the standard output, whose direct term is the ground's again: not an altitude)."""
    rows = sorted((a, r) for a, r in zip(PIPE_ALTS, flux) if a >= 0)
    d = min(abs(hi[1][0] - lo[1][0]) for lo, hi in zip(rows, rows[1:]))
    return spread(nets(flux)), float(d)


def _pipeline(rs, what, kws, aer):
    spec_tuples, spec_flux = rs.sos_spectrum_levels(PIPE_ALTS, kws, aer_phases=None if aer is None else [aer] * len(kws), fluxes=True)
    assert len(spec_flux) == len(kws)
    out = []
    for i, kw in enumerate(kws):
        _, flux = rs.sos_proc_levels(PIPE_ALTS, aer_phase=aer, fluxes=True, **kw)
        assert flux.shape == (len(PIPE_ALTS), 5) and np.isfinite(flux).all()
        assert np.array_equal(flux, spec_flux[i]), (what, i)
        span, d = _span_and_d(flux)
        print("%s, call %d: nets %s (flux_net of row -1: %.6f) span %.3e, d %.3e, d / 20 over the span %.1f"
              % (what, i, nets(flux).tolist(), flux[0, 4], span, d, d / DETECT / max(span, 1e-300)))
        out.append((span, d))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["rayleigh", "aerosol"])
def test_pipeline_conserves_flux_between_levels(gpu_pkg, what):
    """C: sos_proc_levels and sos_spectrum_levels (two wavelengths) with fluxes=True on a Rayleigh-only and on a conservative
    aerosol call (aer_phase with piz = piztr = 1, a_tronc = 0.25), no gas, Lambert ground: the net fluxes of nets() -- column
    flux_net of every altitude, and the -1 row through the net fluxes at the ground and at the top it takes part in -- span at most
    d / 20, and the rows of the two entry points are equal.  There is no CPU reference of the pipeline's own profile: the bar
    is the detection condition itself."""
    rs = gpu_pkg.run_sos
    aer, extra = None, {}
    if what == "aerosol":
        al, be, ga, ze = S.hg_phase(80, 0.7)                               # OS_NB = 2 x -ANG.Aer.NbGauss
        aer = dict(alpha=al, beta=be, gamma=ga, zeta=ze, piz=1.0, piztr=1.0, a_tronc=0.25)
        extra = PIPE_AER
    kws = [_pipe_kwargs(rs, dict(extra, **{"-SOS_Main.Wa": wa})) for wa in PIPE_WA]
    for span, d in _pipeline(rs, what, kws, aer):
        assert span <= d / DETECT, (what, span, d)


@pytest.mark.gpu
def test_pipeline_control_a_gas_breaks_the_constant(gpu_pkg, monkeypatch):
    """The Rayleigh call of C with the H2O / O3 / O2 absorption of a 25-bin band: the same nets span more than d."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    rs = gpu_pkg.run_sos
    (span, d), = _pipeline(rs, "rayleigh with gas", [_pipe_kwargs(rs, PIPE_GAS)], None)
    assert span > d, (span, d)
