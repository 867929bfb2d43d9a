"""The true direct / diffuse split of the down-going flux at every output altitude, on the device: the untruncated depth row
of the profile kernels (sosgpu_profile_true, sosgpu_profile_spectrum_true), the depth at an altitude (sosgpu_output_depths),
its band transmission (sosgpu_level_transmission) and split=True of run_sos.sos_proc_levels / sos_spectrum_levels.
The CPU side is tests/test_level_split.py, two ranks are tests/test_level_split_dist.py."""
import ctypes as C
import math

import numpy as np
import pytest

import profile_cells as PC
import spectrum_cases
from spectrum_cases import assert_tuples_equal

GOLD = spectrum_cases.GOLD
OUT = ("nt", "iborm", "prof", "zprof", "scal", "jout", "zz")
CELLS = ["base_nogas", "base_gas", "base_gas_thin", "grid_two", "grid_low30", "ray_smax2", "dropped", "scan_ng_65",
         "base_very_strong", "lp_short", "lp_tight"]
TABLE_CELLS = [n for n in CELLS if PC.CELLS[n]["grid"] is None and PC.CELLS[n]["lp"] == 608]
GUARD = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ctx(gpu_pkg, smax=16):
    S = gpu_pkg.synth
    mu, w, n0 = S.gauss_angles(8, 35.0)
    al, be, ga, ze = S.hg_phase(16, 0.5)
    return gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=smax, ro=0.1)


def _equal_outputs(a, b, what):
    import torch
    for k in OUT:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (what, k)


def _depth_at(z, h, nt, zout):
    """SOS.F:570-582: the first level J >= 1 (stopping at NT) with ZOUT >= Z(J), the linear weight, the depth of row h there."""
    if zout == -1.0:
        return h[0]
    j = 1
    while j < nt and zout < z[j]:
        j += 1
    zz = (zout - z[j - 1]) / (z[j] - z[j - 1])
    return (1 - zz) * h[j - 1] + zz * h[j]


# ------------------------------------------------------------------------------------------------------------- profile cells

@pytest.mark.gpu
@pytest.mark.parametrize("name", CELLS)
def test_true_depth_row_of_a_cell(gpu_pkg, monkeypatch, name):
    """hvrai of the dressed run (the cell's a_tronc, piz, piztr, zout) == H of the PLAIN run of the same inputs, the run
    test_profile_cell holds to the oracle; wave form == one-lane form; every other output == the run without the row;
    hvrai[b][nt] has the bits of TTOT_VRAI; a flagged bin keeps the caller's zeros.  Then six altitudes (standard output,
    ground, on a level, between levels, below the last, above the first): tauvrai == the host statements on the device's own
    zprof and hvrai; sosgpu_output_depths on prof with stride 3 lp == tauout; without rescale tauvrai == tauout; at 0 km
    tauvrai has the bits of TTOT_VRAI."""
    import torch
    c = PC.CELLS[name]
    alt, tabs = PC.cell_inputs(c)
    nb = 1 if tabs is None else len(tabs)
    lp = c["lp"]
    cx = _ctx(gpu_pkg, c["smax"])
    try:
        geo = (nb, c["tr"], c["hr"], c["ta"], c["ha"], alt, tabs)
        kw = dict(a_tronc=c["a_tronc"], piz=c["piz"], piztr=c["piztr"], zout=c["zout"], lp=lp)
        off = cx.make_profiles(*geo, **kw)
        on = cx.make_profiles(*geo, true_depth=True, **kw)
        monkeypatch.setenv("SOSGPU_PROFILE_LANES", "1")
        lanes = cx.make_profiles(*geo, true_depth=True, **kw)
        monkeypatch.delenv("SOSGPU_PROFILE_LANES")
        plain = cx.make_profiles(*geo, lp=lp)
        torch.cuda.synchronize()
        assert "hvrai" not in off and tuple(on["hvrai"].shape) == (nb, lp)
        _equal_outputs(on, off, name)
        _equal_outputs(lanes, off, name)
        assert torch.equal(on["hvrai"], lanes["hvrai"]), name
        nt = on["nt"].cpu().numpy()
        flagged = nt < 0
        assert bool(flagged.any()) == (name == "lp_short"), (name, nt)
        hv, scal, zp = on["hvrai"].cpu().numpy(), on["scal"].cpu().numpy(), on["zprof"].cpu().numpy()
        for b in range(nb):
            if flagged[b]:
                assert not hv[b].any(), name
                continue
            assert torch.equal(on["hvrai"][b], plain["prof"][b, 0]), (name, b)
            assert _bits(hv[b, nt[b]]) == _bits(scal[b, 2]), (name, b)
            assert not hv[b, nt[b] + 1:].any()
        # (with a_tronc != 0 and no aerosol the rescale re-accumulates H without shrinking it: neither claim below applies)
        plain_cell, rescaled = c["a_tronc"] == 0.0, c["a_tronc"] != 0.0 and c["ta"] != 0.0
        if rescaled and not flagged.all():
            assert not torch.equal(on["hvrai"], on["prof"][:, 0]), name            # (the row is not the truncated one)
        # ---- the six altitudes
        zs = zp[0, :nt[0] + 1] if not flagged[0] else np.array([120.0, 50.0, 0.0])
        alts = [-1.0, 0.0, float(zs[len(zs) // 2]), 0.5 * float(zs[1] + zs[2]), -0.5, 119.0]
        lev, lev_off = cx.output_levels(on, alts), cx.output_levels(off, alts)
        dep = torch.full((len(alts) * nb + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        rc = gpu_pkg.capi.lib().sosgpu_output_depths(0, nb, lp, C.c_void_p(on["prof"].data_ptr()), 3 * lp,
                                                     C.c_void_p(on["zprof"].data_ptr()), C.c_void_p(on["nt"].data_ptr()),
                                                     len(alts), (C.c_double * len(alts))(*alts), C.c_void_p(dep.data_ptr()),
                                                     cx._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert "tauvrai" not in lev_off and all(torch.equal(lev[k], lev_off[k]) for k in ("jout", "zz", "tauout"))
        assert torch.equal(dep[:len(alts) * nb].view(len(alts), nb), lev["tauout"]) and bool(torch.isnan(dep[-GUARD:]).all())
        tv = lev["tauvrai"].cpu().numpy()
        assert tv.shape == (len(alts), nb)
        for b in range(nb):
            if flagged[b]:
                assert not tv[:, b].any(), name
                continue
            for k, zo in enumerate(alts):
                assert _bits(tv[k, b]) == _bits(_depth_at(zp[b], hv[b], int(nt[b]), zo)), (name, b, zo)
            assert _bits(tv[1, b]) == _bits(scal[b, 2]), (name, b)
        if plain_cell:
            assert torch.equal(lev["tauvrai"], lev["tauout"]), name
        elif rescaled and not flagged.all():
            assert bool((lev["tauvrai"] >= lev["tauout"]).all()) and not torch.equal(lev["tauvrai"], lev["tauout"]), name
    finally:
        cx.close()


@pytest.mark.gpu
def test_true_depth_rows_of_the_table_form(gpu_pkg):
    """The no-gas cells of the list as ONE part of make_profiles_spectrum(true_depth=True): hvrai of every wavelength ==
    the per-wavelength call's, every other output == the part made without the row; concat_bins carries the rows."""
    import torch
    assert len(TABLE_CELLS) >= 3
    reqs = [dict({k: PC.CELLS[n][k] for k in ("tr", "hr", "ta", "ha", "a_tronc", "piz", "piztr", "zout", "smax")}, ik=None)
            for n in TABLE_CELLS]
    part, part_off = {}, {}
    bins = gpu_pkg.solver.make_profiles_spectrum(reqs, part=part, true_depth=True)
    bins_off = gpu_pkg.solver.make_profiles_spectrum(reqs, part=part_off)
    torch.cuda.synchronize()
    assert tuple(part["bins"]["hvrai"].shape) == (len(reqs), 608) and "hvrai" not in part_off["bins"]
    ctx = {}
    try:
        for n, tb, tb_off in zip(TABLE_CELLS, bins, bins_off):
            c = PC.CELLS[n]
            if c["smax"] not in ctx:
                ctx[c["smax"]] = _ctx(gpu_pkg, c["smax"])
            cx = ctx[c["smax"]]
            one = cx.make_profiles(1, c["tr"], c["hr"], c["ta"], c["ha"], a_tronc=c["a_tronc"], piz=c["piz"], piztr=c["piztr"],
                                   zout=c["zout"], true_depth=True)
            torch.cuda.synchronize()
            _equal_outputs(tb, tb_off, n)
            _equal_outputs(tb, one, n)
            assert "hvrai" not in tb_off and torch.equal(tb["hvrai"], one["hvrai"]), n
            assert float(tb["hvrai"][0, int(tb["nt"][0])]) == float(tb["scal"][0, 2]) > 0.0, n
        z = [dict(b, jout=None, zz=None) for b in bins]
        cat, _, _ = gpu_pkg.solver.concat_bins(z)
        assert torch.equal(cat["hvrai"], part["bins"]["hvrai"])
        assert "hvrai" not in gpu_pkg.solver.concat_bins([dict(b, jout=None, zz=None) for b in bins_off])[0]
    finally:
        for cx in ctx.values():
            cx.close()


# ------------------------------------------------------------------------------------------------------ transmission kernel

SEG_SIZES = (1, 2, 5, 125, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [1, 16])
def test_level_transmission(gpu_pkg, nz):
    """Segments of 1, 2, 5, 125 and 300 bins (the last crosses the 256 threads of the shared reduction), random positive aik,
    a few failed bins (norders = -1), nz = 1 and 16, the slots 3 doubles apart with NaNs between and around them:
    element 9 of a slot fed TTOT_VRAI == element 4 of sosgpu_aggregate's block bit for bit; every slot within 1e-12 relative
    of a numpy left-to-right sum (<= 300 positive terms and one ulp of exp: about 3e-14); nothing else is written."""
    import torch
    rng = np.random.default_rng(100 + nz)
    seg = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)
    nb, nseg = int(seg[-1]), len(SEG_SIZES)
    cx = _ctx(gpu_pkg)
    try:
        sw = gpu_pkg.capi.SCAL_BASE + cx.n
        aik = rng.uniform(0.01, 1.0, nb)
        norders = rng.integers(1, cx.smax + 2, nb).astype(np.int32)
        norders[[3, 40, 200, 390, 432]] = -1
        scal = np.zeros((nb, 4))
        scal[:, 1:] = rng.uniform(0.0, 6.0, (nb, 3))
        tau = rng.uniform(0.0, 6.0, (nz, nb))
        tau[0] = scal[:, 2]
        tau[-1] = scal[:, 2]
        out = dict(rec=torch.from_numpy(rng.standard_normal((nb, cx.smax + 1, 3, cx.w))).cuda(),
                   norders=torch.from_numpy(norders).cuda(), flux=torch.from_numpy(rng.uniform(0.0, 1.0, (nb, 2))).cuda())
        seg_t, aik_t, tau_t = torch.from_numpy(seg).cuda(), torch.from_numpy(aik).cuda(), torch.from_numpy(tau).cuda()
        _, base = cx.aggregate(out, aik_t, seg=seg_t, scal=torch.from_numpy(scal).cuda())
        assert tuple(base.shape) == (nseg, sw) and not base[:, 9].any()
        stride = nseg * sw + 3
        buf = torch.full((GUARD + nz * stride + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        slots = buf[GUARD:GUARD + nz * stride].view(nz, stride)
        slots[:, :nseg * sw] = base.reshape(-1)
        before = buf.cpu().numpy().copy()
        rc = gpu_pkg.capi.lib().sosgpu_level_transmission(0, nb, nseg, C.c_void_p(seg_t.data_ptr()), C.c_void_p(aik_t.data_ptr()),
                                                          C.c_void_p(out["norders"].data_ptr()), nz, C.c_void_p(tau_t.data_ptr()),
                                                          C.c_void_p(slots.data_ptr()), stride, sw, cx._stream())
        torch.cuda.synchronize()
        assert rc == 0
        after = buf.cpu().numpy()
        written = np.zeros(after.size, dtype=bool)
        base_h = base.cpu().numpy()
        worst = 0.0
        for k in range(nz):
            for g in range(nseg):
                pos = GUARD + k * stride + g * sw + 9
                written[pos] = True
                ref = 0.0
                for b in range(seg[g], seg[g + 1]):
                    if norders[b] >= 0:
                        ref = ref + aik[b] * math.exp(-tau[k, b])
                assert ref > 0.0 or SEG_SIZES[g] == 1
                err = abs(after[pos] - ref) / ref if ref > 0.0 else abs(after[pos])
                worst = max(worst, err)
                assert err <= 1e-12, (k, g, after[pos], ref)
                if k in (0, nz - 1):
                    assert _bits(after[pos]) == _bits(base_h[g, 4]), (k, g, after[pos], base_h[g, 4])
        print("nz %d: worst relative difference to the left-to-right sum %.2e" % (nz, worst))
        assert np.array_equal(_bits(after[~written]), _bits(before[~written]))
        assert np.isnan(after[:GUARD]).all() and np.isnan(after[-GUARD:]).all()
        # through the solver: aggregate_levels with tauvrai fills element 9 of its stacked blocks, without it leaves the 0
        lv = dict(nz=nz, tauout=torch.from_numpy(rng.uniform(0.0, 6.0, (nz, nb))).cuda(), tauvrai=tau_t)
        outk = dict(out, rec=out["rec"][None].expand(nz, *out["rec"].shape))
        _, s_on = cx.aggregate_levels(outk, lv, aik_t, seg=seg_t, scal=torch.from_numpy(scal).cuda())
        _, s_off = cx.aggregate_levels(outk, dict(nz=nz, tauout=lv["tauout"]), aik_t, seg=seg_t, scal=torch.from_numpy(scal).cuda())
        torch.cuda.synchronize()
        assert not s_off[:, :, 9].any()
        assert torch.equal(s_on[:, :, 9].cpu(), torch.from_numpy(after[GUARD:GUARD + nz * stride].reshape(nz, stride)
                                                                 [:, :nseg * sw].reshape(nz, nseg, sw)[:, :, 9]))
        keep = [i for i in range(sw) if i != 9]
        assert torch.equal(s_on[:, :, keep], s_off[:, :, keep])
    finally:
        cx.close()


# ---------------------------------------------------------------------------------------------------------------- end to end

BAND_CASES = ["cfg1_lambert", "cfg4_glitter_bilnd", "ckd_o2a_5bins", "ckd_o2a_mode2", "layer_1_3km_lnd"]
ALTS = [-1, 0.0, 3.0]
_BAND = {}                                     # name -> (keywords, tuples, flux rows [3][7], a_tronc): computed once, shared


def _band(gpu_pkg, workdir, monkeypatch, name):
    """sos_proc_levels(ALTS, fluxes=True, split=True) of a case, with the a_tronc its plan used."""
    if name not in _BAND:
        rs = gpu_pkg.run_sos
        monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
        kws, _, _, _ = spectrum_cases.build(rs, workdir, names=[name])
        kw = dict(kws[0], zout=-1.0)
        seen = []
        real = rs._prepare

        def keep(*a, **k):
            pl = real(*a, **k)
            seen.append(pl)
            return pl

        monkeypatch.setattr(rs, "_prepare", keep)
        tuples, flux = rs.sos_proc_levels(ALTS, fluxes=True, split=True, **kw)
        monkeypatch.setattr(rs, "_prepare", real)
        assert len(seen) == 1
        _BAND[name] = (kw, tuples, flux, float(seen[0].a_tronc), len(np.atleast_1d(seen[0].aik)))
    return _BAND[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", BAND_CASES)
def test_split_rows_of_a_band(gpu_pkg, tmp_path, monkeypatch, name):
    """sos_proc_levels([-1, 0, 3], fluxes=True, split=True): tuples and the first five columns == the split=False call;
    row -1 restates elements 18 (bits) and 19 (1e-12 of flux_tot_down, the bar of test_standard_output_row_vs_sos_proc: E-
    comes from the flux kernel there and from the solver here); row 0 km == row -1 in column 5 (bits: one process, a band of
    at most 128 bins, tau = TTOT_VRAI through the shared reduction) and within 1e-9 in column 6 (the records' parity bar
    through another slot); in every row columns 5 + 6 == column 2 within 4 ulp, 0 < column 5 <= column 0, strictly below at
    0 km with a truncated phase function and equal without."""
    rs = gpu_pkg.run_sos
    kw, tuples, flux, a_tronc, nbins = _band(gpu_pkg, tmp_path, monkeypatch, name)
    ref_t, ref_f = rs.sos_proc_levels(ALTS, fluxes=True, **kw)
    assert flux.shape == (3, 7) and flux.dtype == np.float64 and ref_f.shape == (3, 5) and np.isfinite(flux).all()
    for k in range(3):
        assert_tuples_equal(tuples[k], ref_t[k])
    assert np.array_equal(flux[:, :5], ref_f)
    print("%s: a_tronc %.5f, %d bin(s)\n%s" % (name, a_tronc, nbins, flux))
    assert _bits(flux[0, 5]) == _bits(float(tuples[0][18]))
    assert abs(flux[0, 6] - float(tuples[0][19])) <= 1e-12 * flux[0, 2]
    assert nbins <= 128
    assert _bits(flux[1, 5]) == _bits(flux[0, 5])
    assert abs(flux[1, 6] - flux[0, 6]) <= 1e-9 * abs(flux[0, 6])
    for k in range(3):
        assert abs((flux[k, 5] + flux[k, 6]) - flux[k, 2]) <= 4 * np.spacing(flux[k, 2]), k
        assert 0.0 < flux[k, 5] <= flux[k, 0], k
    if name == "cfg4_glitter_bilnd":
        assert a_tronc != 0.0
    if a_tronc != 0.0:
        assert flux[1, 5] < flux[1, 0]
    else:
        assert np.array_equal(flux[:, 5], flux[:, 0])
    assert flux[2, 5] > flux[1, 5]                                     # less air above 3 km than above the ground


@pytest.mark.gpu
def test_split_of_the_five_bin_band_vs_the_oracle(gpu_pkg, oracle, tmp_path, monkeypatch):
    """Independent reference for flux_dir_down at 3 km of ckd_o2a_5bins: the band's profile inputs captured from make_profiles,
    the CPU oracle's profile of every bin (exact exp), its H interpolated at 3 km in numpy, -ln sum aik exp(-tau) -- within
    1e-9 relative (a last-digit difference of one printed H entry, 1e-8 relative on one level of one bin under the sensitive
    rule of profile_cells.rule, weighs less than that in the band value)."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=["ckd_o2a_5bins"])
    kw = dict(kws[0], zout=-1.0)
    calls, plans = [], []
    real_mp, real_prep = gpu_pkg.SosContext.make_profiles, rs._prepare

    def mp(self, *a, **k):
        calls.append((a, k))
        return real_mp(self, *a, **k)

    def prep(*a, **k):
        plans.append(real_prep(*a, **k))
        return plans[-1]

    monkeypatch.setattr(gpu_pkg.SosContext, "make_profiles", mp)
    monkeypatch.setattr(rs, "_prepare", prep)
    _, flux = rs.sos_proc_levels(ALTS, fluxes=True, split=True, **kw)
    assert len(calls) == 1 and len(plans) == 1 and calls[0][1].get("true_depth") is True
    (nb, tr, hr, ta, ha, altabs, tabs), k = calls[0]
    tabs = tabs.cpu().numpy() if hasattr(tabs, "cpu") else np.asarray(tabs)
    aik = np.asarray(plans[0].aik, dtype=np.float64)
    assert nb == 5 == len(aik) == len(tabs)
    trs = 0.0
    for b in range(nb):
        info = oracle.sos_profile_info(tr, hr, ta, ha, np.asarray(altabs), tabs[b], absprofil=k["absprofil"], exp_mode="exact")
        assert info["ier"] == 0
        trs = trs + aik[b] * math.exp(-_depth_at(info["zprof"], info["h"], info["nt"], 3.0))
    cs = math.cos(math.pi * float(plans[0].p["tetas"]) / 180.0)
    want = math.exp(-(-math.log(trs)) / cs)
    print("flux_dir_down at 3 km: device %.17g, oracle %.17g, relative difference %.2e" % (flux[2, 5], want, abs(flux[2, 5] / want - 1)))
    assert abs(flux[2, 5] - want) <= 1e-9 * want


def _count(monkeypatch, pkg):
    """Counting wrappers round the four new entry points of the library."""
    n = dict(profile=0, spectrum=0, depths=0, trans=[])
    L = pkg.capi.lib()
    real = {k: getattr(L, k) for k in ("sosgpu_profile_true", "sosgpu_profile_spectrum_true", "sosgpu_output_depths",
                                       "sosgpu_level_transmission")}

    def wrap(name, key):
        def f(*a):
            if key == "trans":
                n["trans"].append((int(a[2]), int(a[6])))              # (segments, slots) of the launch
            else:
                n[key] += 1
            return real[name](*a)
        monkeypatch.setattr(L, name, f)

    wrap("sosgpu_profile_true", "profile")
    wrap("sosgpu_profile_spectrum_true", "spectrum")
    wrap("sosgpu_output_depths", "depths")
    wrap("sosgpu_level_transmission", "trans")
    return n


@pytest.mark.gpu
def test_split_rows_of_a_spectrum(gpu_pkg, tmp_path, monkeypatch):
    """The five cases, two of them twice, as one spectrum of one part: the rows == sos_proc_levels' bit for bit; the
    transmission launch comes once per solved group or single wavelength with all three slots, never once per altitude, and
    at least one launch covers several wavelengths; with split=False none of the new entry points is called."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    names = BAND_CASES + ["ckd_o2a_5bins", "cfg4_glitter_bilnd"]
    want = [_band(gpu_pkg, tmp_path, monkeypatch, n) for n in names]
    kws = [w[0] for w in want]
    n = _count(monkeypatch, gpu_pkg)
    solves = []
    real = gpu_pkg.SosContext.aggregate_levels

    def agg(self, out, levels, *a, **k):
        solves.append(levels["nz"])
        return real(self, out, levels, *a, **k)

    monkeypatch.setattr(gpu_pkg.SosContext, "aggregate_levels", agg)
    spec, flux = rs.sos_spectrum_levels(ALTS, kws, fluxes=True, split=True)
    print("transmission launches (segments, slots):", n["trans"], "profile launches", n["profile"], n["spectrum"], "depths", n["depths"])
    assert len(n["trans"]) == len(solves) < len(names) and all(nz == 3 for _, nz in n["trans"])
    assert sum(g for g, _ in n["trans"]) == len(names) and max(g for g, _ in n["trans"]) >= 2
    assert n["spectrum"] == 1 and n["profile"] >= 1                   # one part; mode 2 makes its own profile launch
    for i, (kw, tuples, rows, _, _) in enumerate(want):
        assert flux[i].shape == (3, 7) and np.array_equal(flux[i], rows), names[i]
        for k in range(3):
            assert_tuples_equal(spec[i][k], tuples[k])
    n.update(profile=0, spectrum=0, depths=0, trans=[])
    spec0, flux0 = rs.sos_spectrum_levels(ALTS, kws, fluxes=True)
    one_t, one_f = rs.sos_proc_levels(ALTS, fluxes=True, **kws[2])
    assert (n["profile"], n["spectrum"], n["depths"], n["trans"]) == (0, 0, 0, []), n
    for i in range(len(names)):
        assert flux0[i].shape == (3, 5) and np.array_equal(flux0[i], flux[i][:, :5])
    assert np.array_equal(one_f, flux0[2])
    one_t, one_f = rs.sos_proc_levels(ALTS, fluxes=True, split=True, **kws[2])
    assert (n["profile"], n["spectrum"], n["depths"], n["trans"]) == (1, 0, 1, [(1, 3)]), n
