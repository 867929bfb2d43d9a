"""The aerosol-layer profile (-AP.AerProfile.Type 2) on the device: sosgpu_profile_layer and sosgpu_profile_layer_spectrum
against the host chain of layer_cells.host_chain -- no tolerance: nt, iborm, jout, zz, scal, prof, zprof and hvrai are equal
(test_layer_profile.py states why the last bit of the device's exp / log cannot show) -- then the calls that reach them:
sos_proc, sos_proc_levels and the spectrum passes, held to SOS_LAYER_PROFILE_HOST=1 and to the launch counts."""
import ctypes as C
import itertools

import numpy as np
import pytest

import layer_cells
import spectrum_cases
from layer_cells import LP, PARAMS, PIZ, TAIL_CELLS, host_chain
from spectrum_cases import assert_tuples_equal

GOLD = spectrum_cases.GOLD
KEYS = ("nt", "iborm", "prof", "zprof", "scal")
SMAX = 8
GUARD = 7.5


def _ctx(pkg):
    S = pkg.synth
    mu, w, n0 = S.gauss_angles(4, 35.0)
    al, be, ga, ze = S.hg_phase(SMAX, 0.6)
    return pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=SMAX, build=False)


def _host(b, w=0):
    """Bin w of a device bins dict as numpy: the entries of host_chain (jout / zz 0 where the dict has none)."""
    out = {k: b[k][w].cpu().numpy() for k in KEYS}
    out["nt"], out["iborm"] = int(out["nt"]), int(out["iborm"])
    out["jout"] = int(b["jout"][w]) if b["jout"] is not None else 0
    out["zz"] = float(b["zz"][w]) if b["zz"] is not None else 0.0
    if b.get("hvrai") is not None:
        out["hvrai"] = b["hvrai"][w].cpu().numpy()
    return out


def _assert_same(got, want, where, hvrai=True):
    for k in ("nt", "iborm", "jout", "zz"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("scal", "zprof", "prof") + (("hvrai",) if hvrai else ()):
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(got[k] != want[k])[:8].tolist())


def _request(cell, **kw):
    r = dict(zip(("tr", "hr", "ta", "zmin", "zmax"), cell), a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, smax=SMAX)
    r.update(kw)
    return r


@pytest.mark.gpu
def test_plain_profiles_single_and_table_form(gpu_pkg):
    """Every cell with a_tronc = 0, piztr = 1, zout = -1: the single form, and the table form with all cells in one call in
    shuffled order, equal the host chain and each other; one refused cell among them: bad_wl, nothing queued, outputs untouched."""
    import torch
    S, L = gpu_pkg.solver, gpu_pkg.capi.lib()
    cx = _ctx(gpu_pkg)
    want = [host_chain(gpu_pkg, c, smax=SMAX) for c in PARAMS]
    single = [_host(cx.make_layer_profile(*c, true_depth=True)) for c in PARAMS]
    order = np.random.default_rng(3).permutation(len(PARAMS))
    part = {}
    made = S.make_layer_profiles_spectrum([_request(PARAMS[i]) for i in order], part=part, true_depth=True)
    torch.cuda.synchronize()
    assert part["bins"]["nb"] == len(PARAMS) and part["seg"].tolist() == list(range(len(PARAMS) + 1))
    for k, i in enumerate(order):
        _assert_same(single[i], want[i], ("single", PARAMS[i]))
        _assert_same(_host(made[k]), want[i], ("table", PARAMS[i]))
        _assert_same(_host(part["bins"], k), single[i], ("table vs single", PARAMS[i]))
        assert made[k]["jout"] is None and made[k]["zz"] is None and made[k]["nb"] == 1 and made[k]["lp"] == LP
    # --- a refused cell in the middle: its index, its code, nothing written
    reqs = [_request(PARAMS[i]) for i in order]
    reqs.insert(5, _request(layer_cells.REFUSALS[0][0]))
    pk = S.pack_layer_requests(reqs, LP, True)
    n = len(reqs)
    fb = torch.full((pk["doubles"],), GUARD, dtype=torch.float64, device="cuda")
    ib = torch.full((3 * n,), -77, dtype=torch.int32, device="cuda")
    off = pk["off"]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    bad = C.c_int(-1)
    need = int(L.sosgpu_profile_layer_spectrum_work_bytes(n))
    rc = L.sosgpu_profile_layer_spectrum(0, n, pk["wl"].ctypes.data_as(C.c_void_p), LP, ptr(fb[off["work"]:]), need, ptr(fb),
                                         ptr(ib), ptr(ib[n:]), ptr(fb[off["zprof"]:]), ptr(ib[2 * n:]), ptr(fb[off["zz"]:]),
                                         ptr(fb[off["scal"]:]), ptr(fb[off["hvrai"]:]), C.byref(bad), None)
    torch.cuda.synchronize()
    assert (rc, bad.value) == (layer_cells.E_UNSUPPORTED, 5)
    assert bool((fb == GUARD).all()) and bool((ib == -77).all())
    with pytest.raises(gpu_pkg.capi.SosgpuError):
        info = {}
        try:
            S.make_layer_profiles_spectrum(reqs, part=info)
        finally:
            assert info.get("bad") == 5
    cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell", TAIL_CELLS, ids=lambda c: "nt%d" % (int((c[0] + c[2]) / 0.005) if c[0] + c[2] < 3 else 600))
def test_tail_of_the_profile(gpu_pkg, cell):
    """a_tronc x piztr x zout x (hvrai given or NULL): rescale, IBORM (piztr = 0: min(2, smax)), output level and TAUOUT of
    both forms equal the host chain; without hvrai everything else keeps its bits."""
    import torch
    S = gpu_pkg.solver
    cx = _ctx(gpu_pkg)
    combos = list(itertools.product((0.0, 0.35), (1.0, 0.93, 0.0), layer_cells.tail_zouts(cell)))
    want = [host_chain(gpu_pkg, cell, a_tronc=a, piz=PIZ, piztr=p, zout=z, smax=SMAX) for a, p, z in combos]
    reqs = [_request(cell, a_tronc=a, piz=PIZ, piztr=p, zout=z) for a, p, z in combos]
    for true_depth in (True, False):
        made = S.make_layer_profiles_spectrum(reqs, true_depth=true_depth)
        single = [cx.make_layer_profile(*cell, a_tronc=a, piz=PIZ, piztr=p, zout=z, true_depth=true_depth) for a, p, z in combos]
        torch.cuda.synchronize()
        for k, (a, p, z) in enumerate(combos):
            where = (cell, a, p, z, true_depth)
            _assert_same(_host(made[k]), want[k], ("table",) + where, hvrai=true_depth)
            _assert_same(_host(single[k]), want[k], ("single",) + where, hvrai=true_depth)
            assert ("hvrai" in made[k]) == ("hvrai" in single[k]) == true_depth
            assert (made[k]["jout"] is None) == (single[k]["jout"] is None) == (z == -1.0)
            if p == 0.0:
                assert want[k]["iborm"] == 2
    cx.close()


def _raw_single(pkg, cx, cell, lp, zout=-1.0):
    """sosgpu_profile_layer on outputs preset to guard values; the outputs as numpy."""
    import torch
    fb = torch.full((6 * lp + 5,), GUARD, dtype=torch.float64, device="cuda")
    ib = torch.full((3,), -77, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = pkg.capi.lib().sosgpu_profile_layer(cx._h, *cell, 0.35, PIZ, 0.93, zout, lp, ptr(fb), ptr(ib), ptr(ib[1:]), ptr(fb[3 * lp:]),
                                            ptr(ib[2:]), ptr(fb[4 * lp:]), ptr(fb[4 * lp + 1:]), ptr(fb[4 * lp + 5:]), cx._stream())
    torch.cuda.synchronize()
    f, i = fb.cpu().numpy(), ib.cpu().numpy()
    return rc, dict(nt=int(i[0]), iborm=int(i[1]), jout=int(i[2]), prof=f[:3 * lp].reshape(3, lp), zprof=f[3 * lp:4 * lp],
                    zz=float(f[4 * lp]), scal=f[4 * lp + 1:4 * lp + 5], hvrai=f[4 * lp + 5:5 * lp + 5], beyond=f[5 * lp + 5:])


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [PARAMS[0], PARAMS[9], PARAMS[11]], ids=["nt8", "nt64", "nt600"])
def test_lp_edges(gpu_pkg, cell):
    """lp = NT + 1 holds the profile (and nothing is written beyond it); lp = NT comes back with nt = -1, zero scalars and
    untouched rows."""
    cx = _ctx(gpu_pkg)
    nt = gpu_pkg.geometry.layer_grid(*cell)[0]
    zout = 0.5 * (cell[3] + cell[4])
    rc, got = _raw_single(gpu_pkg, cx, cell, nt + 1, zout)
    assert rc == 0
    _assert_same(got, host_chain(gpu_pkg, cell, a_tronc=0.35, piz=PIZ, piztr=0.93, zout=zout, smax=SMAX, lp=nt + 1), cell)
    assert np.all(got["beyond"] == GUARD)
    rc, got = _raw_single(gpu_pkg, cx, cell, nt, zout)
    assert rc == 0 and (got["nt"], got["iborm"], got["jout"], got["zz"]) == (-1, 0, 0, 0.0)
    assert np.all(got["scal"] == 0.0)
    assert all(np.all(got[k] == GUARD) for k in ("prof", "zprof", "hvrai", "beyond"))
    cx.close()


# ------------------------------------------------------------------------------------------------------------- end to end

ALTS = [-1, 0, 2, 8.5]


def _hg_aer(pkg, kw, piz=0.95):
    al, be, ga, ze = pkg.synth.hg_phase(pkg.run_sos._angle_counts(kw)[2], 0.7)
    return dict(alpha=al, beta=be, gamma=ga, zeta=ze, piz=piz, piztr=piz, a_tronc=0.0)


def _single_calls(pkg, workdir):
    """(name, keywords, aer_phase): the golden layer call, a ground layer, a layer seen from -SOS.OutputAlt 2.0, a layer over a
    rough sea, a layer of an aerosol given without truncation."""
    rs = pkg.run_sos
    (layer, glitter), _, _, _ = spectrum_cases.build(rs, workdir, names=["layer_1_3km_lnd", "cfg4_glitter_bilnd"])
    layer = dict(layer, fictrans="NO_OUTPUT", ficflux="NO_OUTPUT")
    plain = dict(layer, zout=-1.0)
    return [("layer_1_3km_lnd", layer, None),
            ("thin ground layer", dict(plain, zmin=0.0, zmax=2.0, aot_ref=0.05), None),           # 29 levels: rows of 32
            ("output at 2 km", dict(plain, zmin=0.5, zmax=4.0, aot_ref=0.2, zout=2.0), None),
            ("glitter", dict(glitter, iprofil=2, zmin=1.0, zmax=3.0, zout=-1.0, fictrans="NO_OUTPUT", ficflux="NO_OUTPUT"), None),
            ("no truncation", plain, _hg_aer(pkg, plain))]


@pytest.mark.gpu
def test_single_calls_equal_the_host_profile(gpu_pkg, tmp_path, monkeypatch):
    """sos_proc and sos_proc_levels with the device profile give the bits of SOS_LAYER_PROFILE_HOST=1, in all 23 elements and
    in the flux and absorption rows; the default reads no profile back for its output levels."""
    rs, S = gpu_pkg.run_sos, gpu_pkg.solver
    L = gpu_pkg.capi.lib()
    calls = _single_calls(gpu_pkg, tmp_path)
    n = dict(host_levels=0, layer=0)
    hol, single = S.host_output_levels, L.sosgpu_profile_layer

    def counted_hol(*a, **k):
        n["host_levels"] += 1
        return hol(*a, **k)

    def counted_single(*a):
        n["layer"] += 1
        return single(*a)

    monkeypatch.setattr(S, "host_output_levels", counted_hol)
    monkeypatch.setattr(L, "sosgpu_profile_layer", counted_single)
    for name, kw, aer in calls:
        monkeypatch.delenv("SOS_LAYER_PROFILE_HOST", raising=False)
        n.update(host_levels=0, layer=0)
        dev = rs.sos_proc(aer_phase=aer, **kw)
        lv_kw = dict(kw, zout=-1.0)
        dev_lv = rs.sos_proc_levels(ALTS, aer_phase=aer, fluxes=True, split=True, absorption=True, **lv_kw)
        assert (n["host_levels"], n["layer"]) == (0, 2), (name, n)
        monkeypatch.setenv("SOS_LAYER_PROFILE_HOST", "1")
        host = rs.sos_proc(aer_phase=aer, **kw)
        host_lv = rs.sos_proc_levels(ALTS, aer_phase=aer, fluxes=True, split=True, absorption=True, **lv_kw)
        assert n["host_levels"] == 1 and n["layer"] == 2, (name, n)
        assert_tuples_equal(dev, host, name)
        for k in range(len(ALTS)):
            assert_tuples_equal(dev_lv[0][k], host_lv[0][k], (name, ALTS[k]))
        assert np.array_equal(dev_lv[1], host_lv[1]) and np.array_equal(dev_lv[2], host_lv[2], equal_nan=True), name
    # the refusals keep their texts, before any device work
    with pytest.raises(rs.SosProcError, match="ERROR 1020"):
        rs.sos_proc(**dict(calls[1][1], aot_ref=2e-5))
    assert n["layer"] == 2


def _spectrum_calls(rs, workdir):
    """Twelve calls, ten of them layer calls: three wavelengths x (ground layer, lifted layer) with equal angle sets, a layer
    with another NbGauss, one with -SOS.OutputAlt, an exponential-profile call, the 5-bin band, a -SOS.Trans layer, a glitter
    layer.  Returns (keywords, indices of the six equal-key layer calls, index of the -SOS.Trans call)."""
    (layer, glitter, expo, band), _, _, _ = spectrum_cases.build(
        rs, workdir, names=["layer_1_3km_lnd", "cfg4_glitter_bilnd", "cfg2_lnd_lambert", "ckd_o2a_5bins"])
    quiet = dict(fictrans="NO_OUTPUT", ficflux="NO_OUTPUT")
    plain = dict(layer, zout=-1.0, **quiet)
    six = [dict(plain, wa_simu=wa, waref_aot=wa, zmin=zmin, zmax=zmax) for wa in (0.50, 0.55, 0.65) for zmin, zmax in ((0.0, 2.0), (1.0, 3.0))]
    kws = six[:3] + [dict(expo, **quiet)] + six[3:] + [
        dict(plain, nbmu_gauss_lum=16), dict(plain, zout=2.0), dict(band, zout=-1.0, **quiet),
        dict(plain, fictrans="SOS_Transm.txt"),
        dict(glitter, iprofil=2, zmin=1.0, zmax=3.0, zout=-1.0, **quiet)]
    return kws, [0, 1, 2, 4, 5, 6], 10


COUNTED = ("sosgpu_profile_layer_spectrum", "sosgpu_profile_layer", "sosgpu_os_solve_multi", "sosgpu_os_solve",
           "sosgpu_profile_spectrum", "sosgpu_profile_spectrum_true", "sosgpu_profile", "sosgpu_profile_true")


@pytest.fixture(scope="module")
def spectrum(gpu_pkg, tmp_path_factory):
    """The calls and the loop of sos_proc over them, computed once."""
    import os
    rs = gpu_pkg.run_sos
    old = os.environ.get("SOS_ABS_ROOT")
    os.environ["SOS_ABS_ROOT"] = GOLD
    try:
        kws, six, trans = _spectrum_calls(rs, tmp_path_factory.mktemp("layer_spectrum"))
        loop = [rs.sos_proc(**kw) for kw in kws]
    finally:
        if old is None:
            del os.environ["SOS_ABS_ROOT"]
        else:
            os.environ["SOS_ABS_ROOT"] = old
    return dict(kws=kws, six=six, trans=trans, loop=loop)


def _count(monkeypatch, L):
    n = {}

    def counted(name):
        f = getattr(L, name)
        n[name] = 0

        def g(*a):
            n[name] += 1
            return f(*a)
        return g

    for name in COUNTED:
        monkeypatch.setattr(L, name, counted(name))
    return n


@pytest.mark.gpu
def test_spectrum_equals_the_loop_and_groups_the_layer_calls(gpu_pkg, spectrum, monkeypatch):
    """sos_spectrum equals the loop of sos_proc for chunk 1, 2 and 256; one sosgpu_profile_layer_spectrum per part that holds a
    layer call, one sosgpu_profile_layer for the -SOS.Trans call only, and at chunk 256 ONE sosgpu_os_solve_multi over the six
    equal-key layer calls; with SOS_LAYER_PROFILE_HOST=1 the same tuples from one solve per layer call."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, loop = spectrum["kws"], spectrum["loop"]
    n = _count(monkeypatch, gpu_pkg.capi.lib())
    layer_calls = [i for i, kw in enumerate(kws) if int(kw["iprofil"]) == 2 and i != spectrum["trans"]]
    assert len(layer_calls) == 9 and len(kws) == 12
    for chunk in (1, 2, 256):
        for k in n:
            n[k] = 0
        got = rs.sos_spectrum(kws, chunk=chunk, parts=1)
        for i, (a, b) in enumerate(zip(got, loop)):
            assert_tuples_equal(a, b, (chunk, i))
        chunks = [range(c, min(c + chunk, len(kws))) for c in range(0, len(kws), chunk)]
        assert n["sosgpu_profile_layer_spectrum"] == sum(any(i in layer_calls for i in c) for c in chunks), (chunk, n)
        assert n["sosgpu_profile_layer"] == 1, (chunk, n)
        if chunk == 256:
            # the six layer calls of equal key in one launch; the other three deferred layer and no-gas calls alone
            assert n["sosgpu_os_solve_multi"] == 1, n
            multi256, single256 = n["sosgpu_os_solve_multi"], n["sosgpu_os_solve"]
    monkeypatch.setenv("SOS_LAYER_PROFILE_HOST", "1")
    for k in n:
        n[k] = 0
    got = rs.sos_spectrum(kws, chunk=256, parts=1)
    for i, (a, b) in enumerate(zip(got, loop)):
        assert_tuples_equal(a, b, ("host", i))
    assert n["sosgpu_profile_layer_spectrum"] == 0 and n["sosgpu_profile_layer"] == 0, n
    assert n["sosgpu_os_solve_multi"] == multi256 - 1 and n["sosgpu_os_solve"] == single256 + 6, (n, multi256, single256)


@pytest.mark.gpu
def test_spectrum_levels_and_irradiances(gpu_pkg, spectrum, monkeypatch):
    """sos_spectrum_levels gives the tuples and rows of sos_proc_levels of each call; sos_spectrum_irradiances the rows of the
    levels pass for the layer calls (one-bin calls: every column keeps its bits).  No profile is read back."""
    rs, S = gpu_pkg.run_sos, gpu_pkg.solver
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    keep = [i for i, kw in enumerate(spectrum["kws"]) if i != spectrum["trans"] and float(kw["zout"]) == -1.0]
    kws = [spectrum["kws"][i] for i in keep]
    hol = S.host_output_levels
    monkeypatch.setattr(S, "host_output_levels", lambda *a, **k: pytest.fail("host_output_levels on the device route"))
    spec, flux, absorb = rs.sos_spectrum_levels(ALTS, kws, fluxes=True, split=True, absorption=True, parts=1)
    irr_flux, irr_abs = rs.sos_spectrum_irradiances(ALTS, kws, split=True, absorption=True, parts=1)
    monkeypatch.setattr(S, "host_output_levels", hol)
    for g, kw in enumerate(kws):
        ref, rf, ra = rs.sos_proc_levels(ALTS, fluxes=True, split=True, absorption=True, **kw)
        for k in range(len(ALTS)):
            assert_tuples_equal(spec[g][k], ref[k], (g, ALTS[k]))
        assert np.array_equal(flux[g], rf) and np.array_equal(absorb[g], ra, equal_nan=True), g
        if int(kw["iprofil"]) == 2:
            assert np.array_equal(irr_flux[g], flux[g]) and np.array_equal(irr_abs[g], absorb[g], equal_nan=True), g
