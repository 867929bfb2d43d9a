"""Actinic flux and absorbed power at every output altitude of a levels call (sosgpu_level_absorption, k_level_absorption of
csrc/absorb.hip; SosContext.level_absorption, solver.level_absorption_spectrum; absorption=True of run_sos.sos_proc_levels and
sos_spectrum_levels).

The reference everywhere is host_terms, a host restatement of the definitions in include/sosgpu.h, applied to the per-bin records
of the CPU oracle (oracle.sos_os_levels) -- never device output.  What makes it a check of the physics and not of itself is the
divergence theorem with absorption: for layer j

    F_net(z_{j-1}) - F_net(z_j) = power absorbed in layer j = sum_b aik_b q_b(z_mid) dz,

whose left side is built from the hemispheric fluxes (weight mu, test_level_flux.host_flux) and the bins' own direct beams, the
right side from the moment without mu, the level single-scattering albedo and the layer slope.  test_level_conservation states
the conservative case (both sides 0); the cells here absorb, by a gas, by the aerosol, or both.

CPU (oracle only): the residual r of the identity per cell; the detection condition (each of the errors the identity is meant to
catch -- omega one level off, the direct depth one level off, the neighbouring layer's slope -- moves every layer's ratio by at
least DETECT x r) and the separation by the GPU bar BAR x r; the hemisphere symmetry of the restatement; the C surface and its
refusals; the keyword rules.
GPU: A the kernel chain per cell, B the table form over two contexts in one launch, C the band sum alone on synthetic records,
D the pipeline (sos_proc_levels, sos_spectrum_levels), E two ranks on one GPU."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import cases
import spectrum_cases
from spectrum_cases import assert_tuples_equal
import test_level_conservation as tlc
import test_variant_matrix as vm
from dist_launch import run_ranks
from test_level_flux import GOLD, host_flux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = cases.S
PARITY, DETECT, BAR = tlc.PARITY, tlc.DETECT, tlc.BAR
E_ARG = -1
GUARD = 8                                     # doubles behind d_out, preset to NaN


def _cell(name, levels, nt=30, ng=8, sun=35.0, os_nb=16, g=0.6, tau_a=0.3, k_abs=(0.3,), aik=(1.0,), piz=1.0, a_tronc=0.0, ro=0.3):
    return dict(name=name, nt=nt, ng=ng, sun=sun, os_nb=os_nb, g=g, tau_a=tau_a, k_abs=tuple(k_abs), aik=tuple(aik), piz=piz,
                a_tronc=a_tronc, ro=ro, ipolar=1, first=levels)


# `first`: the first of 8 consecutive levels (level 0 is the top, level NT the ground).  The cells keep away from the top two
# layers and from the last two above the ground, where the oracle's own residual is 3e-3 and 7e-4.
CELLS = [
    _cell("gas", 10),
    _cell("absaer_j8", 8, k_abs=(0.0,), piz=0.85),
    _cell("absaer_weakgas", 14, k_abs=(0.05,), piz=0.85),
    _cell("trunc_gas", 20, piz=0.9, a_tronc=0.25),
    _cell("nt65", 29, nt=65, ro=0.0),                                     # streamed solver; chunk edge 31 | 32 | 33
    _cell("three_bins", 12, k_abs=(0.05, 0.3, 1.0), aik=(0.5, 0.3, 0.2), piz=0.95),
    _cell("n25_sun60_nt45", 20, nt=45, ng=24, sun=60.0, os_nb=40, g=0.7, tau_a=1.0, piz=0.9, ro=0.1),
]
IDS = [c["name"] for c in CELLS]
NLEV = 8


def _by_name(name):
    return CELLS[IDS.index(name)]


_INPUTS = {}


def inputs(c):
    """test_level_conservation.inputs for an absorbing cell (same keys, so that its _context and _upload serve here): the bins of
    a cell share the level altitudes of the first.  alts: the 8 levels, then the 7 mid-layer altitudes between them; slots: the
    (jout, zz) the output-level rule gives for them; layers: (level j, slot of level j - 1, slot of level j, slot of the middle)."""
    if c["name"] not in _INPUTS:
        mu, w, n0 = S.gauss_angles(c["ng"], c["sun"])
        piz, a = c["piz"], c["a_tronc"]
        piztr = piz * (1 - a / 2) / (1 - piz * a / 2)
        bins, zprof = [], None
        for k in c["k_abs"]:
            h, x, y, z = S.profile(c["nt"], tau_a=c["tau_a"], k_abs=k)
            h, x, y, ib = S.rescale_profile(h, x, y, a, piz, piztr, c["os_nb"])
            bins.append((h, x, y, ib))
            zprof = z if zprof is None else zprof
        assert np.all(np.diff(zprof) < 0) and all(np.all(np.diff(b[0]) > 0) for b in bins), c["name"]
        lv = list(range(c["first"], c["first"] + NLEV))
        alts = [float(zprof[j]) for j in lv] + [float((zprof[j - 1] + zprof[j]) / 2) for j in lv[1:]]
        layers = [(j, i - 1, i, NLEV + i - 1) for i, j in enumerate(lv) if i > 0]
        _INPUTS[c["name"]] = dict(mu=mu, w=w, n0=n0, mus=float(mu[n0 - 1]), phase=S.hg_phase(c["os_nb"], c["g"]), bins=bins,
                                  zprof=zprof, alts=alts, aik=np.array(c["aik"], dtype=np.float64), levels=lv, layers=layers)
    return _INPUTS[c["name"]]


def host_slots(zprof, alts):
    """(jout, zz) per altitude by the output-level rule (SOS_OS.F:1514-1520): the first level j with z >= zprof[j]."""
    out = []
    for z in alts:
        j = 1
        while z < zprof[j]:
            j += 1
        out.append((j, (z - zprof[j - 1]) / (zprof[j] - zprof[j - 1])))
    return out


def host_terms(mu, ga, n0, row, h, xdel, ydel, zprof, j, zz, tauout, om_shift=0, slope_shift=0):
    """(a_dir, a_dn, a_up, q) of one bin at one slot: the statements of include/sosgpu.h, left to right in doubles.  om_shift,
    slope_shift: the errors of the detection condition (omega from the level pair / the slope of the layer that far off)."""
    n = len(mu)
    s_dn = s_up = 0.0
    for jj in range(1, n + 1):
        s_dn = s_dn + float(ga[jj - 1]) * float(row[n - jj])
    for jj in range(1, n + 1):
        s_up = s_up + float(ga[jj - 1]) * float(row[n + jj])
    tab = -float(mu[n0 - 1])
    a_dn, a_up = -s_dn * 2 / tab, -s_up * 2 / tab
    mus = float(mu[n0 - 1])
    a_dir = math.exp(-float(tauout) / mus) / mus
    zz = float(zz)
    jo, js = j + om_shift, j + slope_shift
    om = (1 - zz) * (float(xdel[jo - 1]) + float(ydel[jo - 1])) + zz * (float(xdel[jo]) + float(ydel[jo]))
    if float(zprof[js - 1]) <= float(zprof[js]):
        slope = 0.0
    else:
        slope = (float(h[js]) - float(h[js - 1])) / (float(zprof[js - 1]) - float(zprof[js]))
    return a_dir, a_dn, a_up, slope * (1 - om) * (a_dn + a_up + a_dir)


def host_tauout(h, j, zz):
    return (1 - zz) * float(h[j - 1]) + zz * float(h[j])


def band_sum(aik, terms):
    """sum aik * term over the bins, left to right (a = a + w * x), per column."""
    acc = [0.0] * 4
    for w, t in zip(aik, terms):
        acc = [a + float(w) * float(x) for a, x in zip(acc, t)]
    return acc


def _oracle_bin(oracle, c, p, b):
    h, x, y, ib = p["bins"][b]
    return oracle.sos_os_levels(p["mu"], p["w"], c["os_nb"], h, x, y, *p["phase"], p["alts"], n0=p["n0"], zprof=p["zprof"],
                                ro=c["ro"], iborm=ib, ipolar=c["ipolar"])


def cell_terms(p, rows, slots, tauout, **err):
    """terms[slot][bin] = host_terms of every slot and bin: rows[slot][bin] the order-0 intensity rows, slots[slot] = (j, zz),
    tauout[slot][bin]."""
    return [[host_terms(p["mu"], p["w"], p["n0"], rows[k][b], *p["bins"][b][:3], p["zprof"], slots[k][0], slots[k][1],
                        tauout[k][b], **err) for b in range(len(p["bins"]))] for k in range(len(slots))]


def ratios(p, out, fnet):
    """Per layer: sum_b aik q_b(z_mid) dz / (F_net(j-1) - F_net(j)); out[slot] = the band sums, fnet[slot] of the 8 levels."""
    z = p["zprof"]
    return np.array([out[m][3] * float(z[j - 1] - z[j]) / (fnet[a] - fnet[b]) for j, a, b, m in p["layers"]])


def fnet_levels(p, e, tauout):
    """F_net at the 8 level slots: every bin's own direct beam exp(-tauout / mu_s), weighted with its aik, + E- - E+."""
    return np.array([float(sum(a * math.exp(-float(t) / p["mus"]) for a, t in zip(p["aik"], tauout[k]))) + e[k][0] - e[k][1]
                     for k in range(NLEV)])


def _reference(c, p, per_bin):
    nz, nb = len(p["alts"]), len(p["bins"])
    slots = host_slots(p["zprof"], p["alts"])
    rows = [[per_bin[b]["records"][k, 0, 0] for b in range(nb)] for k in range(nz)]
    tauout = [[host_tauout(p["bins"][b][0], *slots[k]) for b in range(nb)] for k in range(nz)]
    terms = cell_terms(p, rows, slots, tauout)
    out = [band_sum(p["aik"], terms[k]) for k in range(nz)]
    agg = []
    for k in range(nz):
        row = np.zeros(2 * len(p["mu"]) + 1)
        for a, r in zip(p["aik"], rows[k]):
            row = row + a * r
        agg.append(row)
    e = np.array([host_flux(p["mu"], p["w"], p["n0"], row) for row in agg])
    fnet = fnet_levels(p, e, tauout)
    rat = ratios(p, out, fnet)
    return dict(per_bin=per_bin, slots=slots, rows=rows, tauout=tauout, terms=terms, out=np.array(out), e=e, fnet=fnet, ratios=rat,
                r=float(np.abs(rat - 1).max()))


_REFS = {}


def reference(oracle, c):
    """The oracle solves of every cell are queued on first use (plain C behind ctypes), one levels call per bin."""
    if not _REFS:
        for cc in CELLS:
            pp = inputs(cc)
            _REFS[cc["name"]] = [vm._POOL.submit(_oracle_bin, oracle, cc, pp, b) for b in range(len(pp["bins"]))]
    if c["name"] not in _REFS:                                             # (a cell made by a test: test B's second sun)
        p = inputs(c)
        _REFS[c["name"]] = [vm._POOL.submit(_oracle_bin, oracle, c, p, b) for b in range(len(p["bins"]))]
    if isinstance(_REFS[c["name"]], list):
        _REFS[c["name"]] = _reference(c, inputs(c), [f.result() for f in _REFS[c["name"]]])
    return _REFS[c["name"]]


def wrong(p, ref):
    """The errors the identity is meant to catch, applied to the oracle's own numbers: {name: ratios per layer}."""
    nz, nb = len(p["alts"]), len(p["bins"])
    out = {}
    for shift in (-1, 1):
        for what, err, tau in (("omega %+d" % shift, dict(om_shift=shift), ref["tauout"]),
                               ("slope %+d" % shift, dict(slope_shift=shift), ref["tauout"]),
                               ("direct depth %+d" % shift, {}, [[host_tauout(p["bins"][b][0], ref["slots"][k][0] + shift, ref["slots"][k][1])
                                                                   for b in range(nb)] for k in range(nz)])):
            terms = cell_terms(p, ref["rows"], ref["slots"], tau, **err)
            out[what] = ratios(p, [band_sum(p["aik"], terms[k]) for k in range(nz)], ref["fnet"])
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_cells_are_what_they_claim(pkg):
    assert len(set(IDS)) == len(CELLS) == 7
    for c in CELLS:
        p = inputs(c)
        nt, lv = c["nt"], p["levels"]
        assert len(p["alts"]) == 15 <= pkg.capi.MAX_OUTPUT_LEVELS and len(p["layers"]) == 7
        assert lv[0] - 1 >= 2 and lv[-1] <= nt - 2, c["name"]             # away from the top two and the last two layers
        assert abs(sum(c["aik"]) - 1.0) < 1e-15 and len(c["aik"]) == len(c["k_abs"]) == len(p["bins"])
        jout, zz = pkg.solver.output_levels_host(p["zprof"][None, :], p["alts"])
        assert jout[:, 0].tolist() == lv + lv[1:] and zz[:NLEV, 0].tolist() == [1.0] * NLEV, c["name"]
        assert np.abs(zz[NLEV:, 0] - 0.5).max() < 1e-3, c["name"]
        assert [(j, zv) for j, zv in zip(jout[:, 0], zz[:, 0])] == host_slots(p["zprof"], p["alts"])
        for h, x, y, ib in p["bins"]:                                      # every layer of the cell absorbs
            om = x[lv[0] - 1:lv[-1] + 1] + y[lv[0] - 1:lv[-1] + 1]
            assert len(h) == nt + 1 and ib == c["os_nb"] and (om < 1 - 1e-3).all() and (om > 0).all(), c["name"]
    streamed = {c["name"] for c in CELLS if vm.route(len(inputs(c)["mu"]), vm._round_up(c["nt"] + 1, 16)).startswith("stream")}
    assert streamed == {"nt65"} and set(inputs(_by_name("nt65"))["levels"]) >= {31, 32, 33}
    assert len(inputs(_by_name("n25_sun60_nt45"))["mu"]) == 25


@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_oracle_residual_and_detection_condition(oracle, c):
    """The identity on the oracle's own records, and the condition that keeps the GPU test honest: omega one level up or down,
    the depth of the direct term one level up or down, the slope of the neighbouring layer -- each moves EVERY layer's ratio by
    at least DETECT x r.  A condition on the cell, not a measurement."""
    ref = reference(oracle, c)
    p = inputs(c)
    assert all(r["ier"] == 0 and r["records"].shape[0] == 15 and r["records"].shape[1] > 0 for r in ref["per_bin"])
    assert np.isfinite(ref["ratios"]).all() and (ref["fnet"][:-1] > ref["fnet"][1:]).all()     # absorption: F_net falls downwards
    moved = {k: np.abs(v - ref["ratios"]) for k, v in wrong(p, ref).items()}
    smallest = min(float(m.min()) for m in moved.values())
    print("%s: ratios %s r %.2e; smallest move %.3e = %.0f r (%s)" % (c["name"], ref["ratios"].tolist(), ref["r"], smallest,
                                                                     smallest / ref["r"], {k: float(m.min() / ref["r"]) for k, m in moved.items()}))
    assert ref["r"] < 1e-3
    for what, m in moved.items():
        assert (m >= DETECT * ref["r"]).all(), (c["name"], what, (m / ref["r"]).tolist())


@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_bar_separates_right_from_wrong(oracle, c):
    """The bar of the GPU test, BAR x r, is missed by each of those errors in every layer."""
    ref = reference(oracle, c)
    assert (np.abs(ref["ratios"] - 1) <= ref["r"]).all()
    for what, rat in wrong(inputs(c), ref).items():
        assert (np.abs(rat - 1) > BAR * ref["r"]).all(), (c["name"], what, rat.tolist())


@pytest.mark.parametrize("c", [CELLS[0], CELLS[5]], ids=[IDS[0], IDS[5]])
def test_restatement_hemisphere_symmetry(oracle, c):
    """Exchanging the hemispheres of the rows swaps the two diffuse columns and leaves the direct one, the total and the absorbed
    power unchanged (an addition commutes)."""
    ref = reference(oracle, c)
    p = inputs(c)
    flipped = cell_terms(p, [[r[::-1] for r in rk] for rk in ref["rows"]], ref["slots"], ref["tauout"])
    for tk, fk in zip(ref["terms"], flipped):
        for t, f in zip(tk, fk):
            assert f[0] == t[0] and f[1] == t[2] and f[2] == t[1] and t[1] != t[2]
            assert f[3] == t[3] > 0 and f[1] + f[2] + f[0] == t[1] + t[2] + t[0]


def test_surface_is_declared_exported_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int sosgpu_level_absorption(sosgpu_ctx *cx, const void *d_table , const int32_t *d_ctx_of_bin , int nb, int lp, "
            "const int32_t *d_nt, const double *d_prof, const double *d_zprof , int nz, const int32_t *d_jout, const double *d_zz, "
            "const double *d_tauout , const double *d_rec , const int32_t *d_norders, int nseg, const int32_t *d_seg, "
            "const double *d_aik, double *d_out , void *stream);") in flat
    assert "sosgpu_level_absorption" in pkg.capi.EXPORTS and hasattr(pkg.capi.lib(), "sosgpu_level_absorption")
    assert len(pkg.capi.lib().sosgpu_level_absorption.argtypes) == 19
    assert pkg.run_sos.LEVEL_ABSORPTION_NAMES == ["actinic_dir", "actinic_diff_down", "actinic_diff_up", "actinic_tot",
                                                  "absorbed_per_km"]
    row = pkg.run_sos._level_absorption_row(3.0, (0.5, 0.25, 0.125, 0.0625))
    assert row == (0.5, 0.25, 0.125, 0.875, 0.0625) and len(row) == 5
    assert all(math.isnan(x) for x in pkg.run_sos._level_absorption_row(-1.0, (0.0, 0.0, 0.0, 0.0)))


def test_arguments_are_refused_without_a_device(pkg):
    """Every refusal of the header, and the two empty calls, before any device is looked for: the pointers are never
    dereferenced, nothing is queued."""
    f = pkg.capi.lib().sosgpu_level_absorption
    p = C.c_void_p(4096)
    #       cx table cob nb lp nt prof zprof nz jout zz tauout rec norders nseg seg aik out stream
    good = [p, None, None, 3, 16, p, p, p, 2, p, p, p, p, p, 1, p, p, p, None]
    for i in (0, 5, 6, 7, 9, 10, 11, 12, 13, 15, 16, 17):                   # a NULL required pointer
        bad = list(good)
        bad[i] = None
        assert f(*bad) == E_ARG, i
    for i, v in ((8, 0), (8, 17), (8, -1), (4, 1), (4, 0), (3, -1), (14, -1)):   # nz, lp, nb, nseg out of range
        bad = list(good)
        bad[i] = v
        assert f(*bad) == E_ARG, (i, v)
    bad = list(good)
    bad[1] = p                                                             # a table without d_ctx_of_bin
    assert f(*bad) == E_ARG
    for i in (3, 14):                                                      # nb = 0, nseg = 0: nothing queued
        ok = list(good)
        ok[i] = 0
        assert f(*ok) == 0
        ok[1], ok[2] = p, p
        assert f(*ok) == 0
        ok[8] = 17                                                         # ... but still checked
        assert f(*ok) == E_ARG


def test_keyword_rules_before_any_library_call(pkg, monkeypatch):
    rs = pkg.run_sos
    monkeypatch.setattr(pkg.capi, "lib", lambda: pytest.fail("a keyword rule reached the library"))
    kw = rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), {"-SOS_Main.Wa": 0.55, "-AER.AOTref": 0.0}), trace=False)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="absorption must be True or False"):
            rs.sos_proc_levels([1.0], fluxes=True, absorption=bad, **kw)
        with pytest.raises(ValueError, match="absorption must be True or False"):
            rs.sos_spectrum_levels([1.0], [kw], fluxes=True, absorption=bad)
    with pytest.raises(ValueError, match="needs fluxes=True"):
        rs.sos_proc_levels([1.0], absorption=True, **kw)
    with pytest.raises(ValueError, match="needs fluxes=True"):
        rs.sos_spectrum_levels([1.0], [kw], absorption=True)
    with pytest.raises(ValueError, match="needs fluxes=True"):
        rs.sos_spectrum_levels([1.0], [], absorption=True)                 # ... before the empty-spectrum shortcut
    for alts in ([1.0], None):
        with pytest.raises(ValueError, match="not available for sensor channels"):
            rs.sos_spectrum_channels([kw], [[1.0]], altitudes=alts, fluxes=alts is not None, absorption=True)
    # a band whose bins are sharded over ranks: sos_proc_levels under torchrun
    monkeypatch.setattr(rs, "_dist_rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="sharded over ranks"):
        rs.sos_proc_levels([1.0], fluxes=True, absorption=True, **kw)
    # (the spectrum pass deals whole wavelengths: in scope, its arguments pass)
    assert rs._levels_arguments("sos_spectrum_levels", [1.0], [kw], True, False, True) == [1.0]
    monkeypatch.undo()
    assert rs.sos_spectrum_levels([-1.0, 3.0], [], fluxes=True, absorption=True) == ([], [], [])


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _device_chain(gpu_pkg, cx, c, p):
    """output_levels (on the device) -> solve_levels -> aggregate_levels + level_flux_many, level_absorption: everything the
    assertions need, on the host."""
    bins = tlc._upload(cx, c, p)
    lv = cx.output_levels(bins, p["alts"])
    out = cx.solve_levels(bins, lv)
    rec, _ = cx.aggregate_levels(out, lv, p["aik"])
    e = gpu_pkg.solver.level_flux_many([(cx, rec[k, 0]) for k in range(NLEV)])
    ab = cx.level_absorption(bins, lv, out, p["aik"])
    assert tuple(ab.shape) == (len(p["alts"]), 1, 4)
    assert (out["norders"].cpu().numpy() > 0).all()
    return dict(ab=ab[:, 0].cpu().numpy(), e=e.cpu().numpy(), rows=out["rec"][:, :, 0, 0].cpu().numpy(),
                jout=lv["jout"].cpu().numpy(), zz=lv["zz"].cpu().numpy(), tauout=lv["tauout"].cpu().numpy())


def _check_chain(c, p, ref, d, what):
    """The assertions of test A on one context."""
    nz, nb = len(p["alts"]), len(p["bins"])
    ab = d["ab"]
    # the device's level table is the host rule's
    assert (d["jout"] == np.array([s[0] for s in ref["slots"]], dtype=np.int32)[:, None]).all(), what
    assert (d["zz"][:NLEV] == 1.0).all() and (np.abs(d["zz"][NLEV:] - 0.5) < 1e-3).all(), what
    # 1. against the restatement on the ORACLE's records
    dev = np.abs(ab[:, 1:] / ref["out"][:, 1:] - 1)
    print("%s: worst relative deviation of (a_dn, a_up, q) from the oracle's %s" % (what, dev.max(axis=0).tolist()))
    assert (ref["out"][NLEV:, 1:] > 0).all() and (dev <= PARITY).all(), (what, dev.max())
    # 2. against the restatement on the DEVICE's own records, slots and depths
    slots = [(int(d["jout"][k, 0]), float(d["zz"][k, 0])) for k in range(nz)]
    terms = cell_terms(p, d["rows"], slots, d["tauout"])
    own = np.array([band_sum(p["aik"], terms[k]) for k in range(nz)])
    if nb == 1:
        assert p["aik"][0] == 1.0 and np.array_equal(ab[:, 1:3], own[:, 1:3]), (what, np.argwhere(ab[:, 1:3] != own[:, 1:3])[:4].tolist())
    print("%s: worst relative deviation from the restatement on the device's records %s"
          % (what, np.abs(ab / own - 1).max(axis=0).tolist()))
    assert (np.abs(ab - own) <= 1e-14 * np.abs(own)).all(), (what, np.abs(ab / own - 1).max(axis=0).tolist())
    # 3. the divergence identity, from device numbers alone
    rat = ratios(p, ab, fnet_levels(p, d["e"], d["tauout"]))
    print("%s: device ratios - 1 %s, oracle r %.2e (bar %.2e)" % (what, (rat - 1).tolist(), ref["r"], BAR * ref["r"]))
    assert np.isfinite(rat).all() and (np.abs(rat - 1) <= BAR * ref["r"]).all(), (what, (rat - 1).tolist(), ref["r"])


@pytest.mark.gpu
@pytest.mark.parametrize("c", CELLS, ids=IDS)
def test_kernel_chain_obeys_the_divergence_identity(gpu_pkg, oracle, c):
    """A: per cell, 15 slots in one solve.  (a_dn, a_up, q) within 1e-9 of the restatement on the oracle's records; on the
    device's own records the diffuse sums of a one-bin cell equal the host's sequential sums bit for bit, and every column agrees
    within 1e-14 (one exp per term, at most 3 positive terms); F_net(j-1) - F_net(j) of the device's own fluxes and depths equals
    q(z_mid) dz within BAR x the oracle's residual of the cell, in each of the 7 layers."""
    p = inputs(c)
    ref = reference(oracle, c)
    cx = tlc._context(gpu_pkg, c, p)
    try:
        d = _device_chain(gpu_pkg, cx, c, p)
    finally:
        cx.close()
    _check_chain(c, p, ref, d, c["name"])


def _table_round(gpu_pkg, oracle, cells, perms):
    """One level_absorption_spectrum launch over the bins of two contexts of equal N and different mu: the second context's bins
    first (the segments are not in context order), each context's bins permuted; against the per-context chains, bit for bit."""
    import torch
    sv = gpu_pkg.solver
    ps = [inputs(c) for c in cells]
    assert len({len(p["mu"]) for p in ps}) == 1 and ps[0]["mus"] != ps[1]["mus"]
    cxs = [tlc._context(gpu_pkg, c, p) for c, p in zip(cells, ps)]
    try:
        singles, parts, lvs, aiks = [], [], [], []
        for cx, c, p, perm in zip(cxs, cells, ps, perms):
            q = dict(p, bins=[p["bins"][i] for i in perm], aik=p["aik"][list(perm)])
            bins = tlc._upload(cx, c, q)
            lv = cx.output_levels(bins, q["alts"])
            out = cx.solve_levels(bins, lv)
            singles.append(cx.level_absorption(bins, lv, out, q["aik"])[:, 0].cpu().numpy())
            parts.append(bins)
            lvs.append(lv)
            aiks.append(q["aik"])
        order = [1, 0]                                                     # segment 0 is context 1
        table = sv.ContextTable(cxs)
        bins, _, seg = sv.concat_bins([parts[i] for i in order])
        cob = torch.tensor(np.repeat(order, [parts[i]["nb"] for i in order]).astype(np.int32), device=cxs[0].device)
        bins["zprof"] = torch.cat([sv.level_altitudes(parts[i], bins["lp"]) for i in order])
        levels = sv.concat_levels([lvs[i] for i in order])
        aik = torch.from_numpy(np.concatenate([aiks[i] for i in order])).to(cxs[0].device)
        out = cxs[0].alloc_outputs(bins["nb"])
        out["rec"] = torch.full((levels["nz"], bins["nb"], cxs[0].smax + 1, 3, cxs[0].w), float("nan"), dtype=torch.float64,
                                device=cxs[0].device)
        sv.solve_spectrum_levels(table, bins, cob, seg, aik, levels, out=out, order=None)
        got = sv.level_absorption_spectrum(table, bins, cob, seg, aik, levels, out).cpu().numpy()
    finally:
        for cx in cxs:
            cx.close()
    assert got.shape == (15, 2, 4) and np.isfinite(got).all()
    for g, i in enumerate(order):
        assert np.array_equal(got[:, g], singles[i]), (cells[i]["name"], np.argwhere(got[:, g] != singles[i])[:4].tolist())
        ref = reference(oracle, cells[i])                                  # ... and they are the cell's values
        assert (np.abs(got[:, g, 1:] / ref["out"][:, 1:] - 1) <= PARITY).all(), cells[i]["name"]
    assert not np.array_equal(got[:, 0], got[:, 1])


@pytest.mark.gpu
def test_table_form_equals_the_per_context_calls(gpu_pkg, oracle):
    """B: N = 9, the three-bin cell under two suns (35 and 50 degrees: two mu tables, two n0) in one launch, bins shuffled;
    then N = 25 (suns of 60 and 35 degrees)."""
    three = _by_name("three_bins")
    other = dict(three, name="three_bins_sun50", sun=50.0)
    _table_round(gpu_pkg, oracle, [three, other], [(2, 0, 1), (1, 2, 0)])
    n25 = _by_name("n25_sun60_nt45")
    other = dict(n25, name="n25_sun35_nt45", sun=35.0)
    _table_round(gpu_pkg, oracle, [n25, other], [(0,), (0,)])


SEG_SIZES = (1, 2, 255, 256, 257, 300)


@pytest.mark.gpu
def test_band_sum_alone_on_synthetic_records(gpu_pkg):
    """C: the entry point on records made here (N = 2, an unbuilt context, no solve): segments of 1, 2, 255, 256, 257 and 300
    bins, one failed bin inside each segment of two or more, one bin with jout = NT + 1; slot 0 interior levels, slot 1 the
    standard output, slot 2 other levels with depth 0.  Against a left-to-right host sum at 1e-12 (positive terms); the one-bin
    segment is aik * term exactly; the standard-output slot is zeros; coinciding altitudes give slope 0 and a finite sum; the
    NaNs behind d_out are untouched."""
    import torch
    rng = np.random.default_rng(7)
    mu, ga, n0 = S.gauss_angles(1, 35.0)
    assert len(mu) == 2
    al, be, gm, ze = S.hg_phase(4, 0.5)
    n, w, s1, lp, nt_, nz = 2, 5, 5, 16, 9, 3
    seg = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)
    nb = int(seg[-1])
    h = np.cumsum(rng.uniform(0.01, 0.2, (nb, lp)), axis=1)
    prof = np.stack([h, rng.uniform(0.05, 0.45, (nb, lp)), rng.uniform(0.05, 0.45, (nb, lp))], axis=1)
    zprof = np.round(120.0 - np.cumsum(rng.uniform(0.5, 5.0, (nb, lp)), axis=1), 5)
    zprof[:, 0] = 120.0
    flat_bins = np.arange(nb) % 5 == 1                                      # every fifth bin: levels 3 and 4 coincide
    zprof[flat_bins, 4] = zprof[flat_bins, 3]
    nt = np.full(nb, nt_, dtype=np.int32)
    jout = np.stack([rng.integers(1, nt_ + 1, nb), np.zeros(nb, dtype=np.int64), rng.integers(1, nt_ + 1, nb)]).astype(np.int32)
    jout[0, flat_bins] = 4
    zz = rng.uniform(0.0, 1.0, (nz, nb))
    tauout = rng.uniform(0.0, 2.0, (nz, nb))
    tauout[2] = 0.0
    rec = np.full((nz, nb, s1, 3, w), np.nan)
    rec[:, :, 0, 0, :] = rng.uniform(0.0, 1.0, (nz, nb, w)) * 10.0 ** rng.integers(-6, 1, (nz, nb, w))
    norders = np.full(nb, 3, dtype=np.int32)
    failed = [int(seg[g] + (seg[g + 1] - seg[g]) // 2) for g in range(1, len(SEG_SIZES))]
    norders[failed] = -1
    seg1 = int(seg[1])
    assert failed[0] == seg1 + 1
    zprof[seg1, 4], jout[0, seg1] = zprof[seg1, 3], 4                       # the two-bin segment: slope 0 next to the failed bin
    beyond = int(seg[3]) + 7
    jout[0, beyond] = nt_ + 1
    aik = rng.uniform(0.1, 1.0, nb)
    # the reference
    want = np.zeros((nz, len(SEG_SIZES), 4))
    one = None
    for k in (0, 2):
        for g in range(len(SEG_SIZES)):
            terms, wts = [], []
            for b in range(int(seg[g]), int(seg[g + 1])):
                if norders[b] < 0 or not 1 <= jout[k, b] <= nt[b]:
                    continue
                terms.append(host_terms(mu, ga, n0, rec[k, b, 0, 0], prof[b, 0], prof[b, 1], prof[b, 2], zprof[b], int(jout[k, b]),
                                        zz[k, b], tauout[k, b]))
                wts.append(aik[b])
            want[k, g] = band_sum(wts, terms)
            if g == 0 and k == 2:
                one = [aik[0] * x for x in terms[0]]
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cx = gpu_pkg.SosContext(mu, ga, n0, al, be, gm, ze, build=False)
    assert cx.smax + 1 == s1 and cx.w == w
    try:
        d = dict(nt=t(nt), prof=t(prof), zprof=t(zprof), jout=t(jout), zz=t(zz), tauout=t(tauout), rec=t(rec), norders=t(norders),
                 seg=t(seg), aik=t(aik))
        out = torch.full((nz * len(SEG_SIZES) * 4 + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        rc = gpu_pkg.capi.lib().sosgpu_level_absorption(cx._h, None, None, nb, lp, ptr(d["nt"]), ptr(d["prof"]), ptr(d["zprof"]), nz,
                                                        ptr(d["jout"]), ptr(d["zz"]), ptr(d["tauout"]), ptr(d["rec"]),
                                                        ptr(d["norders"]), len(SEG_SIZES), ptr(d["seg"]), ptr(d["aik"]), ptr(out),
                                                        cx._stream())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        # the wrapper on the same tensors
        bins = dict(nb=nb, lp=lp, nt=d["nt"], prof=d["prof"], zprof=d["zprof"])
        again = cx.level_absorption(bins, dict(nz=nz, jout=d["jout"], zz=d["zz"], tauout=d["tauout"]),
                                    dict(rec=d["rec"], norders=d["norders"]), d["aik"], seg=seg).cpu().numpy()
    finally:
        cx.close()
    assert rc == 0
    got, guard = out[:-GUARD].reshape(nz, len(SEG_SIZES), 4), out[-GUARD:]
    assert guard.size == GUARD and np.isnan(guard).all()
    assert np.array_equal(again, got)
    assert np.isfinite(got).all()
    assert (got[1] == 0.0).all()                                            # the standard-output slot
    assert (want[[0, 2]][:, :, :3] > 0).all()
    err = np.abs(got - want)
    print("band sums: worst relative deviation from the left-to-right host sum %.3e" % (err[want > 0] / want[want > 0]).max())
    assert (err <= 1e-12 * np.abs(want)).all(), np.argwhere(err > 1e-12 * np.abs(want))[:4].tolist()
    assert got[2, 0].tolist() == one and one[0] == aik[0] * (1.0 / float(mu[n0 - 1]))   # one bin, depth 0: exact in every column
    assert got[0, 1, 3] == 0.0 and got[0, 1, 0] > 0.0                       # slope 0 next to a failed bin: q is 0, not NaN


# D: the pipeline.  0.7, 3 and 8.5 km lie between levels of the product's own profile.
PIPE_ALTS = [-1, 0.0, 0.7, 3.0, 8.5]


def _pipe_calls(rs, tmp_path):
    """(name, kwargs, aer_phase): a no-gas call with an absorbing aerosol (one bin), and the 5-bin CKD golden band."""
    al, be, ga, ze = S.hg_phase(80, 0.7)
    piz, a = 0.9, 0.25
    aer = dict(alpha=al, beta=be, gamma=ga, zeta=ze, piz=piz, piztr=piz * (1 - a / 2) / (1 - piz * a / 2), a_tronc=a)
    nogas = tlc._pipe_kwargs(rs, dict(tlc.PIPE_AER, **{"-SOS_Main.Wa": 0.55}))
    (band,), _, _, _ = spectrum_cases.build(rs, tmp_path, names=["ckd_o2a_5bins"])
    band = dict(band, fictrans="NO_OUTPUT", ficflux="NO_OUTPUT", zout=-1.0)
    return [("absorbing aerosol, no gas", nogas, aer), ("ckd_o2a_5bins", band, None)]


def _pipe_chain(rs, kw, aer, alts):
    """The kernel chain on the call's own plan: (rows [K][4] of level_absorption, per-bin H rows, jout [K][nb], mu_s)."""
    pl = rs._prepare(kw, aer, 0, shard_bins=True)
    try:
        lv = pl.ctx.output_levels(pl.bins, alts)
        out = pl.ctx.solve_levels(pl.bins, lv)
        ab = pl.ctx.level_absorption(pl.bins, lv, out, pl.aik)[:, 0].cpu().numpy()
        return ab, pl.bins["prof"][:, 0].cpu().numpy(), lv["jout"].cpu().numpy(), float(pl.mu[pl.n0 - 1]), pl.bins["nb"]
    finally:
        pl.ctx.close()


@pytest.mark.gpu
def test_sos_proc_levels_rows(gpu_pkg, tmp_path, monkeypatch):
    """D: sos_proc_levels(alts, fluxes=True, absorption=True).  The rows equal the kernel chain's on the call's own plan; the
    row of -1 is NaN; for the one-bin call actinic_dir * cos(theta_s) restates flux_dir_down_tronc within 1e-12 (the two form
    the cosine differently: the 14-digit mu table against cos(pi tetas / 180)) while the direct beam at a neighbouring level is
    at least 1e-3 off; the 23-tuples and the flux rows are those of the call without the keyword, bit for bit."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    for what, kw, aer in _pipe_calls(rs, tmp_path):
        tuples, flux, absorb = rs.sos_proc_levels(PIPE_ALTS, aer_phase=aer, fluxes=True, absorption=True, **kw)
        plain_t, plain_f = rs.sos_proc_levels(PIPE_ALTS, aer_phase=aer, fluxes=True, **kw)
        assert np.array_equal(flux, plain_f) and len(tuples) == len(plain_t) == len(PIPE_ALTS)
        for a, b in zip(tuples, plain_t):
            assert_tuples_equal(a, b)
        assert absorb.shape == (len(PIPE_ALTS), 5) and absorb.dtype == np.float64
        assert np.isnan(absorb[0]).all() and np.isfinite(absorb[1:]).all() and (absorb[1:] > 0).all(), (what, absorb.tolist())
        ab, hrows, jout, mus, nb = _pipe_chain(rs, kw, aer, PIPE_ALTS)
        assert nb == (1 if aer is not None else 5), (what, nb)
        assert (ab[0] == 0.0).all() and (jout[0] == 0).all() and (jout[1:] >= 1).all()
        want = np.array([rs._level_absorption_row(z, ab[k]) for k, z in enumerate(PIPE_ALTS)])
        assert np.array_equal(absorb[1:], want[1:]), (what, absorb.tolist(), want.tolist())
        assert np.array_equal(absorb[1:, 3], absorb[1:, 1] + absorb[1:, 2] + absorb[1:, 0])
        print("%s: absorbed_per_km %s actinic_tot %s" % (what, absorb[1:, 4].tolist(), absorb[1:, 3].tolist()))
        if nb == 1:
            cs = math.cos(math.pi * float(kw["tetas"]) / 180.0)
            rel = np.abs(absorb[1:, 0] * cs / flux[1:, 0] - 1)
            print("%s: actinic_dir cos(theta_s) / flux_dir_down_tronc - 1: %s" % (what, rel.tolist()))
            assert (rel <= 1e-12).all(), rel.tolist()
            for k in range(2, len(PIPE_ALTS)):                             # (0 km is the ground: it has one neighbour)
                j = int(jout[k, 0])
                for i in (j - 1, j + 1):
                    off = abs(math.exp(-(hrows[0, i] - hrows[0, j]) / mus) - 1)
                    assert off >= 1e-3, (what, PIPE_ALTS[k], i, off)


def _count(monkeypatch, pkg):
    """A counting wrapper round the entry point of the library: (calls, their (nb, nz, nseg))."""
    n = dict(calls=0, shapes=[])
    L = pkg.capi.lib()
    f = L.sosgpu_level_absorption

    def counted(*a):
        n["calls"] += 1
        n["shapes"].append((int(a[3]), int(a[8]), int(a[14])))
        return f(*a)

    monkeypatch.setattr(L, "sosgpu_level_absorption", counted)
    return n


@pytest.mark.gpu
def test_sos_spectrum_levels_rows_and_launch_counts(gpu_pkg, tmp_path, monkeypatch):
    """D: sos_spectrum_levels([-1, 0, 3], six calls, fluxes=True, absorption=True) equals the per-call rows of sos_proc_levels bit
    for bit, with the default chunk and with chunk=6 (two wavelengths per chunk at K = 3); ONE sosgpu_level_absorption call per
    solved group or single wavelength, each with all K slots, their segments adding up to the six calls; none at all with the
    default, whose tuples and flux rows are those of the run with the keyword."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=spectrum_cases.RANDOM_CASES[:6])
    kws = [dict(kw, zout=-1.0) for kw in kws]
    alts = [-1, 0.0, 3.0]
    n = _count(monkeypatch, gpu_pkg)
    solves = []
    real_group, real_single = gpu_pkg.solver.solve_spectrum_levels, gpu_pkg.SosContext.solve_levels
    monkeypatch.setattr(gpu_pkg.solver, "solve_spectrum_levels", lambda *a, **k: (solves.append("group"), real_group(*a, **k))[1])
    monkeypatch.setattr(gpu_pkg.SosContext, "solve_levels", lambda *a, **k: (solves.append("single"), real_single(*a, **k))[1])
    got, flux, absorb = rs.sos_spectrum_levels(alts, kws, fluxes=True, absorption=True)
    assert n["calls"] == len(solves) >= 1 and all(s[1] == 3 for s in n["shapes"]) and sum(s[2] for s in n["shapes"]) == 6, (n, solves)
    n.update(calls=0, shapes=[])
    del solves[:]
    got2, flux2, absorb2 = rs.sos_spectrum_levels(alts, kws, fluxes=True, absorption=True, chunk=6)
    assert n["calls"] == len(solves) >= 3 and sum(s[2] for s in n["shapes"]) == 6, (n, solves)
    n.update(calls=0, shapes=[])
    ref, ref_flux = rs.sos_spectrum_levels(alts, kws, fluxes=True)
    assert n["calls"] == 0
    assert len(absorb) == len(absorb2) == 6
    for i in range(6):
        for k in range(3):
            assert_tuples_equal(got[i][k], ref[i][k])
            assert_tuples_equal(got2[i][k], ref[i][k])
        assert np.array_equal(flux[i], ref_flux[i]) and np.array_equal(flux2[i], ref_flux[i])
        assert absorb[i].shape == (3, 5) and np.isnan(absorb[i][0]).all() and np.isfinite(absorb[i][1:]).all()
        assert np.array_equal(absorb[i][1:], absorb2[i][1:]), i
    n.update(calls=0, shapes=[])
    for i in range(6):
        _, f1, a1 = rs.sos_proc_levels(alts, fluxes=True, absorption=True, **kws[i])
        assert np.array_equal(f1, flux[i]) and np.array_equal(a1[1:], absorb[i][1:]), (i, a1.tolist(), absorb[i].tolist())
        assert (a1[1:, :4] > 0).all()
    assert n["calls"] == 6 and all(s[1:] == (3, 1) for s in n["shapes"]), n


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_return_the_same_rows(gpu_pkg, tmp_path, monkeypatch):
    """E: two ranks on cuda:0 (tests/dist_level_absorption_worker.py): the wavelengths are dealt whole, and with gather=True
    every rank returns the rows of this process, bit for bit; gather=False leaves None in the slots of the other rank."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    out = str(tmp_path / "res.json")
    run_ranks("dist_level_absorption_worker.py", ("--out", out), timeout=600)
    r = json.load(open(out))
    kws = dist_kws(rs, tmp_path / "single")
    _, flux, absorb = rs.sos_spectrum_levels(DIST_ALTS, kws, fluxes=True, absorption=True)
    assert r["world"] == 2 and r["digests"] == [rows_digest(flux, absorb)] * 2, r["digests"]
    assert sorted(i for own in r["owners"] for i in own) == list(range(len(kws))) and all(len(own) > 0 for own in r["owners"])
    assert r["partial_ok"] == [True, True]


DIST_ALTS = [-1, 0.0, 3.0]
DIST_NAMES = ["ckd_o2a_5bins", "cfg1_lambert", "rand_00", "rand_13", "rand_05"]


def dist_kws(rs, workdir):
    kws, _, _, _ = spectrum_cases.build(rs, workdir, names=DIST_NAMES)
    return [dict(kw, zout=-1.0, fictrans="NO_OUTPUT", ficflux="NO_OUTPUT") for kw in kws]


def rows_digest(flux, absorb):
    import hashlib
    h = hashlib.sha256()
    for f, a in zip(flux, absorb):
        h.update(np.ascontiguousarray(f, dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())       # (NaN rows: the same bits on every rank)
    return h.hexdigest()
