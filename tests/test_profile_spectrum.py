"""The profile stage of a whole part of a spectrum in three launches (sosgpu_profile_spectrum, solver.make_profiles_spectrum):
packing on the host, the table kernels against the per-wavelength entry points bit for bit and against the oracle, and the
wiring into run_sos.sos_spectrum / sos_spectrum_levels (launch counts, outputs, errors)."""
import os
import re

import numpy as np
import pytest

import cases
import spectrum_cases
from spectrum_cases import assert_tuples_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = spectrum_cases.GOLD
ALT = np.concatenate([np.linspace(120.0, 30.0, 10), np.linspace(28.0, 0.0, 40)])      # the grid of cases.profile_case


def _gas_tables(nterm, k0, k6, hg0=7.0, hg6=5.0, alt=ALT):
    """xk[8][nterm][nlev-1], ro[8][nlev-1] of two absorbers (gases 0 and 6; the other six have zero coefficients): gas g with
    term t gives the cumulative optical depth k[t] * (exp(-z / hg) - exp(-120 / hg)), the synthetic column of
    cases.profile_case."""
    nl1 = len(alt) - 1
    xk, ro = np.zeros((8, nterm, nl1)), np.ones((8, nl1))
    ro[0] = np.exp(-alt[1:] / hg0) - np.exp(-alt[:-1] / hg0)
    ro[6] = np.exp(-alt[1:] / hg6) - np.exp(-alt[:-1] / hg6)
    xk[0] = np.asarray(k0, dtype=np.float64)[:, None]
    xk[6] = np.asarray(k6, dtype=np.float64)[:, None]
    return xk, ro


def _ik(pairs):
    ik = np.ones((len(pairs), 8), dtype=np.int32)
    for b, (i0, i6) in enumerate(pairs):
        ik[b, 0], ik[b, 6] = i0, i6
    return ik


def _requests():
    """Ten wavelengths: no gas with aerosol; molecules only (closed form); weak gas; strong gas (the zlim branch) with a
    truncation rescale; 25 bins over five terms; molecules + gas; a band with a bin that needs more than 600 levels; the thin
    branch; no gas with a rescale and an output level; a one-bin strong band.  nterm 1, 3, 5; bands of 1, 5, 25 bins; zout
    inside the atmosphere on five of them.  `smax` of a request chooses one of the two contexts of the tests."""
    plain = dict(a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0)
    r = []
    r.append(dict(tr=0.0948, hr=8.0, ta=0.3, ha=2.0, ik=None, absprofil=7, smax=16, **plain))
    r.append(dict(tr=0.0948, hr=8.0, ta=0.0, ha=1.0, ik=None, absprofil=7, smax=8, a_tronc=0.0, piz=0.0, piztr=0.0, zout=2.5))
    xk, ro = _gas_tables(1, [0.4], [0.0])
    r.append(dict(tr=0.0948, hr=8.0, ta=0.3, ha=2.0, ik=_ik([(1, 1)]), xk=xk, ro=ro, altabs=ALT, absprofil=1, smax=16, **plain))
    xk, ro = _gas_tables(3, [0.1, 2.0, 8.0], [0.05, 0.9, 0.0])
    r.append(dict(tr=0.0948, hr=8.0, ta=0.3, ha=2.0, ik=_ik([(1, 1), (2, 1), (3, 2), (2, 2), (1, 3)]), xk=xk, ro=ro, altabs=ALT,
                  absprofil=2, smax=16, a_tronc=0.3, piz=0.96, piztr=0.94, zout=3.2))
    xk, ro = _gas_tables(5, [0.01, 0.3, 1.2, 9.0, 60.0], [0.0, 0.02, 0.2, 1.0, 3.0], hg0=5.0, hg6=7.0)
    r.append(dict(tr=0.0948, hr=8.0, ta=0.1, ha=3.0, ik=_ik([(i, j) for i in range(1, 6) for j in range(1, 6)]), xk=xk, ro=ro,
                  altabs=ALT, absprofil=3, smax=8, **plain))
    xk, ro = _gas_tables(3, [0.7, 0.2, 4.0], [0.0, 0.1, 0.3])
    r.append(dict(tr=0.0948, hr=8.0, ta=0.0, ha=1.0, ik=_ik([(1, 1), (2, 2), (3, 3), (3, 1), (1, 3)]), xk=xk, ro=ro, altabs=ALT,
                  absprofil=4, smax=8, a_tronc=0.0, piz=0.0, piztr=0.0, zout=7.5))
    xk, ro = _gas_tables(3, [0.0, 1.4, 0.3], [0.0, 0.0, 0.0])
    r.append(dict(tr=0.0948, hr=8.0, ta=2.8, ha=2.0, ik=_ik([(1, 1), (2, 1), (3, 1), (2, 2), (1, 3)]), xk=xk, ro=ro, altabs=ALT,
                  absprofil=1, smax=16, a_tronc=0.2, piz=0.9, piztr=0.88, zout=0.0))
    xk, ro = _gas_tables(1, [0.003], [0.0])
    r.append(dict(tr=0.004, hr=8.0, ta=0.002, ha=2.0, ik=_ik([(1, 1)]), xk=xk, ro=ro, altabs=ALT, absprofil=5, smax=16, **plain))
    r.append(dict(tr=0.0948, hr=8.0, ta=1.5, ha=1.5, ik=None, absprofil=7, smax=16, a_tronc=0.4, piz=0.95, piztr=0.93, zout=1.0))
    xk, ro = _gas_tables(1, [6.0], [1.0], hg0=2.0)
    r.append(dict(tr=0.02, hr=8.0, ta=0.15, ha=2.0, ik=_ik([(1, 1)]), xk=xk, ro=ro, altabs=ALT, absprofil=6, smax=8, a_tronc=0.1,
                  piz=0.97, piztr=0.95, zout=12.0))
    return r


def test_pack_profile_requests_reproduces_every_request(pkg):
    """The host packing of make_profiles_spectrum: offsets, per-bin wavelength index and packed buffer give back each request's
    arrays exactly (nterm 1, 3, 5; 1, 5 and 25 bins; requests without gas in between)."""
    S = pkg.solver
    reqs = _requests()
    pk = S.pack_profile_requests(reqs)
    counts = [1 if r["ik"] is None else len(r["ik"]) for r in reqs]
    assert sorted(set(counts)) == [1, 5, 25]
    assert sorted({r["xk"].shape[1] for r in reqs if r["ik"] is not None}) == [1, 3, 5]
    nb = sum(counts)
    wl, buf = pk["wl"], pk["buf"]
    assert wl.dtype == S.PROFILE_WL_DTYPE and wl.dtype.itemsize == 104 and wl.shape == (len(reqs),) and wl.flags.c_contiguous
    assert pk["nb"] == nb and pk["nblev"] == 50 and buf.dtype == np.float64 and buf.ndim == 1
    assert np.array_equal(pk["seg"], np.concatenate([[0], np.cumsum(counts)]))
    assert pk["ik_off"] == pk["gas_doubles"] and pk["wob_off"] == pk["ik_off"] + 4 * nb
    assert buf.size == pk["wob_off"] + (nb + 1) // 2
    wob = buf[pk["wob_off"]:].view(np.int32)[:nb]
    assert np.array_equal(wob, np.repeat(np.arange(len(reqs)), counts))
    ik_all = buf[pk["ik_off"]:pk["wob_off"]].view(np.int32).reshape(nb, 8)
    used = np.zeros(pk["gas_doubles"], dtype=bool)
    for w, r in enumerate(reqs):
        e = wl[w]
        for k in ("tr", "hr", "ta", "ha", "a_tronc", "piz", "piztr", "zout"):
            assert e[k] == r[k], (w, k)
        assert e["smax"] == r["smax"] and e["nbins"] == counts[w]
        b0 = int(pk["seg"][w])
        if r["ik"] is None:
            assert e["nterm"] == 0 and e["absprofil"] == 7 and (ik_all[b0] == 0).all()
            continue
        nterm = r["xk"].shape[1]
        assert e["nterm"] == nterm and e["absprofil"] == r["absprofil"]
        xo, ro_, ao = int(e["xk_off"]), int(e["ro_off"]), int(e["alt_off"])
        assert np.array_equal(buf[xo:xo + 8 * nterm * 49].reshape(8, nterm, 49), r["xk"])
        assert np.array_equal(buf[ro_:ro_ + 8 * 49].reshape(8, 49), r["ro"])
        assert np.array_equal(buf[ao:ao + 50], r["altabs"])
        assert np.array_equal(ik_all[b0:b0 + counts[w]], r["ik"])
        for o, n in ((xo, 8 * nterm * 49), (ro_, 8 * 49), (ao, 50)):
            assert not used[o:o + n].any()                  # no two tables overlap
            used[o:o + n] = True
    assert used.all()                                       # ... and nothing else is in the gas part
    # only requests without gas: no gas part at all
    pk0 = S.pack_profile_requests([reqs[0], reqs[1]])
    assert pk0["nblev"] == 0 and pk0["gas_doubles"] == 0 and pk0["nb"] == 2 and pk0["buf"].size == 2 * 4 + 1
    with pytest.raises(ValueError):
        S.pack_profile_requests([dict(reqs[2], ro=np.ones((8, 10)))])


def test_new_symbols_in_header_and_export_list(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    declared = set(re.findall(r"\b(sosgpu_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("sosgpu_profile_spectrum", "sosgpu_profile_spectrum_work_bytes", "sosgpu_profile_nogas_levels"):
        assert sym in declared and sym in pkg.capi.EXPORTS and hasattr(pkg.capi.lib(), sym), sym
    import ctypes as C
    assert C.sizeof(pkg.capi.ProfileWl) == pkg.solver.PROFILE_WL_DTYPE.itemsize
    # the level count of the no-gas grid needs no device: 100 levels for a thin atmosphere, refused beyond CTE_OS_NT
    L = pkg.capi.lib()
    assert L.sosgpu_profile_nogas_levels(0.004, 0.002) == 100 and L.sosgpu_profile_nogas_levels(0.0948, 0.3) > 50
    assert L.sosgpu_profile_nogas_levels(2.0, 1.5) == -1 and L.sosgpu_profile_nogas_levels(0.0, 0.0) == -1
    # argument rules are checked before any device work
    wl = (pkg.capi.ProfileWl * 1)()
    assert L.sosgpu_profile_spectrum(0, 0, wl, 1, None, None, None, 0, 0, 608, None, 0, None, None, None, None, None, None,
                                     None, None, None, None) == -1


def _contexts(gpu_pkg):
    S = gpu_pkg.synth
    mu, w, n0 = S.gauss_angles(8, 35.0)
    al, be, ga, ze = S.hg_phase(16, 0.5)
    return {16: gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=16, ro=0.1),
            8: gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=8, ro=0.1)}


def _per_wavelength(cxs, r):
    """The per-wavelength entry points for one request: (bins of make_profiles, tabs of absorption_profiles or None)."""
    cx = cxs[r["smax"]]
    kw = dict(a_tronc=r["a_tronc"], piz=r["piz"], piztr=r["piztr"], zout=r["zout"])
    if r["ik"] is None:
        return cx.make_profiles(1, r["tr"], r["hr"], r["ta"], r["ha"], None, None, absprofil=7, **kw), None
    tabs = cx.absorption_profiles(r["ik"], r["xk"], r["ro"])
    return cx.make_profiles(len(r["ik"]), r["tr"], r["hr"], r["ta"], r["ha"], r["altabs"], tabs, absprofil=r["absprofil"],
                            **kw), tabs


@pytest.mark.gpu
def test_table_form_equals_per_wavelength_entry_points_bitwise(gpu_pkg):
    """Every wavelength of _requests through ONE make_profiles_spectrum call equals SosContext.absorption_profiles +
    make_profiles of that wavelength alone: torch.equal on prof, zprof, nt, iborm, scal, jout, zz and tabs.  The batch runs
    twice, on two different streams (fresh blocks each time: nothing may depend on what a block held before)."""
    import torch
    reqs = _requests()
    cxs = _contexts(gpu_pkg)
    ref = [_per_wavelength(cxs, r) for r in reqs]
    torch.cuda.synchronize()
    # the cases the list is meant to cover are really in it
    tg = [None if t is None else t[:, -1].cpu().numpy() for _, t in ref]
    nts = np.concatenate([b["nt"].cpu().numpy() for b, _ in ref])
    assert (nts == -1).sum() >= 1 and (nts[nts != -1] > 50).all()
    assert any(t is not None and (t > 1.5).any() for t in tg) and any(t is not None and (t <= 1.5).all() and (t > 0).all()
                                                                          for t in tg)
    assert int(ref[6][0]["nt"].min()) == -1 and float(tg[6][0]) == 0.0          # too many levels; a gas band's bin without gas
    for attempt in range(2):
        st = torch.cuda.Stream()
        info = {}
        got = gpu_pkg.solver.make_profiles_spectrum(reqs, 0, stream=st, part=info)
        st.synchronize()
        assert len(got) == len(reqs)
        for w, (r, g, (b, tabs)) in enumerate(zip(reqs, got, ref)):
            assert set(g) == set(b) == {"nb", "lp", "perm", "nt", "iborm", "prof", "jout", "zz", "zprof", "scal"}
            assert g["nb"] == b["nb"] and g["lp"] == b["lp"] and g["perm"] is None
            for k in ("prof", "zprof", "nt", "iborm", "scal"):
                assert g[k].dtype == b[k].dtype and g[k].shape == b[k].shape and g[k].is_contiguous(), (w, k)
                assert torch.equal(g[k], b[k]), (attempt, w, k)
            if r["zout"] == -1.0:
                assert g["jout"] is None and g["zz"] is None and b["jout"] is None
            else:
                assert g["jout"].dtype == b["jout"].dtype and g["zz"].dtype == b["zz"].dtype
                assert torch.equal(g["jout"], b["jout"]) and torch.equal(g["zz"], b["zz"]), (attempt, w)
            if tabs is None:
                assert info["tabs"][w] is None
            else:
                assert torch.equal(info["tabs"][w], tabs), (attempt, w)
        assert info["bins"]["nb"] == sum(g["nb"] for g in got)
    for cx in cxs.values():
        cx.close()


@pytest.mark.gpu
def test_table_form_vs_oracle(gpu_pkg, oracle):
    """The gas wavelengths of _requests through the table form against the oracle's SOS_PROFILE, at the tolerances of
    tests/test_profile.py (test_device_profile_vs_golden, test_device_profile_random_columns): NT and the level altitudes
    identical, H / XDEL / YDEL at rtol = 2e-8 (one unit of the last digit of the E15.8 round trip); a bin the oracle refuses
    (IER != 0) has nt = -1.  The oracle routine stops at the PROFIL file, so the requests run without the truncation rescale
    of SOS.F (a_tronc = 0, piz = piztr = 1); gas inputs, optical thicknesses and scale heights are those of _requests."""
    import torch
    reqs = [dict(r, a_tronc=0.0, piz=1.0, piztr=1.0) for r in _requests() if r["ik"] is not None]
    assert len(reqs) >= 6
    info = {}
    got = gpu_pkg.solver.make_profiles_spectrum(reqs, 0, part=info)
    torch.cuda.synchronize()
    refused = exact = total = 0
    for w, (r, g) in enumerate(zip(reqs, got)):
        tabs = info["tabs"][w].cpu().numpy()
        nt, prof, z = g["nt"].cpu().numpy(), g["prof"].cpu().numpy(), g["zprof"].cpu().numpy()
        for b in range(g["nb"]):
            o = oracle.sos_profile(r["tr"], r["hr"], r["ta"], r["ha"], r["altabs"], tabs[b])
            total += 1
            if o["ier"] != 0:
                assert nt[b] == -1, (w, b)
                refused += 1
                continue
            assert nt[b] == o["nt"], (w, b, nt[b], o["nt"])
            k = o["nt"] + 1
            assert np.array_equal(z[b, :k], o["zprof"]), (w, b)
            for row, key in enumerate(("h", "xdel", "ydel")):
                assert np.allclose(prof[b, row, :k], o[key], rtol=2e-8, atol=1e-300), (w, b, key)
                assert (prof[b, row, k:] == 0).all()
            exact += int(all(np.array_equal(prof[b, row, :k], o[key]) for row, key in enumerate(("h", "xdel", "ydel"))))
    print("table form vs oracle: %d bins, %d refused by both, %d bit-identical" % (total, refused, exact))
    assert refused >= 1 and total - refused >= 30


QUALIFYING = ["cfg1_lambert", "cfg2_lnd_lambert", "ckd_h2o_o2_25bins_flatsea", "rand_12", "rand_14", "flatsea_zout", "rand_38"]


def _count(monkeypatch, pkg):
    """Counting wrappers round the batched helper and the two per-wavelength methods."""
    n = dict(batch=0, make=0, absp=0, wavelengths=[])
    S = pkg.solver
    f0, m0, a0 = S.make_profiles_spectrum, S.SosContext.make_profiles, S.SosContext.absorption_profiles

    def batch(requests, *a, **k):
        n["batch"] += 1
        n["wavelengths"].append(len(requests))
        return f0(requests, *a, **k)

    def make(self, *a, **k):
        n["make"] += 1
        return m0(self, *a, **k)

    def absp(self, *a, **k):
        n["absp"] += 1
        return a0(self, *a, **k)

    monkeypatch.setattr(S, "make_profiles_spectrum", batch)
    monkeypatch.setattr(S.SosContext, "make_profiles", make)
    monkeypatch.setattr(S.SosContext, "absorption_profiles", absp)
    return n


@pytest.mark.gpu
def test_spectrum_pass_makes_the_profiles_once_per_part(gpu_pkg, tmp_path, monkeypatch):
    """sos_spectrum of qualifying calls with parts=1: solver.make_profiles_spectrum runs once per chunk and the per-wavelength
    SosContext.make_profiles / absorption_profiles not at all; a -SOS.Trans call and a -SOS.AbsModeCKD 2 call added to the
    list are exactly the two that go through the per-wavelength methods."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_PROFILES_PER_CALL", raising=False)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=QUALIFYING + ["ckd_o2a_5bins", "ckd_o2a_mode2"])
    good, trans, mode2 = kws[:len(QUALIFYING)], kws[-2], kws[-1]
    assert str(trans["fictrans"]).strip() != "NO_OUTPUT" and int(mode2["imode_ckd_calcul"]) == 2
    n = _count(monkeypatch, gpu_pkg)
    rs.sos_spectrum(good, parts=1)
    assert (n["batch"], n["make"], n["absp"]) == (1, 0, 0) and n["wavelengths"] == [len(good)], n
    n.update(batch=0, wavelengths=[])
    rs.sos_spectrum(good, parts=1, chunk=3)
    assert (n["batch"], n["make"], n["absp"]) == (3, 0, 0) and n["wavelengths"] == [3, 3, 1], n
    n.update(batch=0, wavelengths=[])
    rs.sos_spectrum(good[:3] + [trans] + good[3:] + [mode2], parts=1)
    assert (n["batch"], n["make"], n["absp"]) == (1, 2, 2) and n["wavelengths"] == [len(good)], n
    n.update(batch=0, make=0, absp=0, wavelengths=[])
    rs.sos_spectrum_levels([-1, 2.0], [dict(kw, zout=-1.0) for kw in good], parts=1)
    assert (n["batch"], n["make"], n["absp"]) == (1, 0, 0), n


END_TO_END = ["ckd_o2a_5bins", "ckd_h2o_o2_25bins_flatsea", "cfg1_lambert", "flatsea_zout", "rand_38", "cfg2_lnd_lambert",
              "rand_12", "cfg5_ckd_maignan_25bins"]


@pytest.mark.gpu
def test_spectrum_outputs_equal_sequential_calls_bitwise(gpu_pkg, tmp_path, monkeypatch):
    """End to end with the batched profile stage: the 5- and 25-bin CKD goldens, no-gas calls, output levels and -SOS.Trans
    calls through sos_spectrum (one chunk, chunk=3, three parts) equal the sequential sos_proc calls on all 23 outputs, and
    sos_spectrum_levels equals sos_proc with each altitude."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_PROFILES_PER_CALL", raising=False)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=END_TO_END)
    assert any(str(kw["fictrans"]).strip() != "NO_OUTPUT" for kw in kws) and any(kw["zout"] != -1.0 for kw in kws)
    seq = [rs.sos_proc(**kw) for kw in kws]
    for a, b in zip(seq, rs.sos_spectrum(kws)):
        assert_tuples_equal(a, b)
    for a, b in zip(seq, rs.sos_spectrum(kws, chunk=3)):
        assert_tuples_equal(a, b)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    for a, b in zip(seq, rs.sos_spectrum(kws, parts=3)):
        assert_tuples_equal(a, b)
    monkeypatch.delenv("SOS_SPECTRUM_MIN_PART")
    alts = [-1, 0.0, 3.0]
    kws_levels = [dict(kw, zout=-1.0) for kw in kws]
    lev = rs.sos_spectrum_levels(alts, kws_levels)
    assert len(lev) == len(kws)
    for i, kw in enumerate(kws_levels):
        for k, z in enumerate(alts):
            assert_tuples_equal(rs.sos_proc(**dict(kw, zout=float(z))), lev[i][k])


@pytest.mark.gpu
def test_spectrum_raises_what_the_call_alone_raises(gpu_pkg, tmp_path, monkeypatch):
    """A call whose no-gas grid needs more than CTE_OS_NT levels, in the middle of a list: sos_spectrum raises the exception
    class, message and ier sos_proc raises for that call alone; the contexts of the other calls are closed and a following
    sos_spectrum of the good calls is right."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=["cfg2_lnd_lambert", "ckd_h2o_o2_25bins_flatsea", "flatsea_zout"])
    bad = dict(kws[0], tr=3.6)                              # (3.6 + 0.3) / 0.005 = 780 levels
    with pytest.raises(rs.SosProcError) as alone:
        rs.sos_proc(**bad)
    assert alone.value.ier == -1 and str(alone.value).startswith("SOS_PROFILE:")
    with pytest.raises(rs.SosProcError) as inlist:
        rs.sos_spectrum([kws[0], kws[1], bad, kws[2]])
    assert type(inlist.value) is type(alone.value) and str(inlist.value) == str(alone.value)
    assert inlist.value.ier == alone.value.ier
    outs = rs.sos_spectrum(kws)
    for kw, o in zip(kws, outs):
        assert_tuples_equal(rs.sos_proc(**kw), o)
