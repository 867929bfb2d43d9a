"""run_sos.sos_spectrum_channels end to end: the channel tuples against the host convolution of sos_spectrum's (or
sos_spectrum_levels') tuples -- ascending call index, a = a + w * x, np.array_equal on the summed tables and scalars --, the
derived tables against oracle.polar at the tolerances of test_surface_trphi.test_trphi_gpu_vs_oracle, independence of `chunk`
and `parts`, the library calls counted, and every ValueError raised before any library call (CPU)."""
import os
import re

import numpy as np
import pytest

import spectrum_cases
from spectrum_cases import assert_tuples_equal

GOLD = spectrum_cases.GOLD
ALTS = [-1, 0.0, 3.0]
# wavenumbers (cm-1) inside the two fixture intervals of tests/golden/fic: 13123 and 13127 lie in the 5-bin interval of the O2 A
# band, 15925 and 15922 in the 25-bin interval; at the others the tables hold one term per gas (no gas absorption: one bin)
WAVENUMBERS = [13255.0, 13123.0, 15925.0, 15605.0, 13127.0, 15922.0, 13405.0]
VARIANTS = {
    "lambert": dict(itrphi=2, pas_phi=120),
    "glitter": dict(isurf=1, wind=5.0, surf_ind=1.34, rho=0.0, itrphi=1, phios=40.0),
    "nopolar": dict(ipolar=0),
}
I_UP, Q_UP, U_UP, I_DN, Q_DN, U_DN = 5, 6, 7, 12, 13, 14
SUMMED = (I_UP, Q_UP, U_UP, I_DN, Q_DN, U_DN)
# (sca, i, q, u, ang, rate, lpol) of the up-going and of the down-going tables
SIDES = ((4, 5, 6, 7, 8, 9, 10), (11, 12, 13, 14, 15, 16, 17))


def weights(n):
    """Six channels on n >= 7 calls: three overlapping ones, one on every call, one on a single call, one with negative side
    lobes."""
    w = np.zeros((6, n))
    w[0, 0:4] = (0.2, 0.5, 1.0, 0.4)
    w[1, 2:6] = (0.3, 1.0, 0.7, 0.1)
    w[2, 3:7] = (0.6, 0.9, 1.0, 0.25)
    w[3, :] = np.linspace(0.5, 1.5, n)
    w[4, 5] = 2.0
    w[5, 1:5] = (-0.1, 0.6, 1.0, -0.05)
    return w


def spectrum(rs, workdir, variant):
    """The calls of one variant: the keyword set of the golden ckd_o2a_5bins (without its -SOS.Trans / -SOS.Flux files) at the
    wavelengths of WAVENUMBERS."""
    (base,), _, _, _ = spectrum_cases.build(rs, workdir, names=["ckd_o2a_5bins"])
    base = dict(base, fictrans="NO_OUTPUT", ficflux="NO_OUTPUT", zout=-1.0, **VARIANTS[variant])
    return [dict(base, wa_simu=1e4 / nu) for nu in WAVENUMBERS]


def applied(w, normalize):
    return np.array([row / np.cumsum(row)[-1] for row in w]) if normalize else w.copy()


def host_sum(w_row, values):
    """a = a + w * x over the calls with a non-zero weight, in ascending call index."""
    a = np.zeros_like(np.asarray(values[0], dtype=np.float64))
    for i, w in enumerate(w_row):
        if w != 0.0:
            a = a + w * np.asarray(values[i], dtype=np.float64)
    return a


def thresholds(t, idx):
    t = t.copy()
    if idx in (I_UP, I_DN):
        t[t <= 1e-99] = 0.0
    else:
        t[np.abs(t) < 1e-15] = 0.0
    return t


def check_channel(oracle, got, w_row, calls, nrow, where):
    """One channel tuple against the calls' tuples (`calls`: the 23-tuples in call order; nrow: azimuth rows of the view).
    Returns whether the channel holds polarised light."""
    assert len(got) == 23
    for e in range(4):
        assert np.array_equal(np.asarray(got[e]), np.asarray(calls[0][e])), (where, e)
    for e in SUMMED:
        ref = thresholds(host_sum(w_row, [t[e] for t in calls]), e)
        assert np.array_equal(got[e], ref), (where, e, np.abs(got[e] - ref).max())
    for e in (18, 19, 20, 21, 22):
        ref = host_sum(w_row, [t[e] for t in calls])
        assert got[e] == float(ref), (where, e, got[e], float(ref))
    n = int(got[0])
    some_polar = False
    for sca, i, q, u, ang, rate, lpol in SIDES:
        assert np.array_equal(got[sca], calls[-1][sca]), (where, sca)
        assert got[i].shape == (361, 81) and np.all(got[i][nrow:] == 0) and np.all(got[i][:, n:] == 0)
        for r in range(nrow):
            for j in range(n):
                xan, tpol, lp = oracle.polar(got[i][r, j], got[q][r, j], got[u][r, j])
                assert abs(got[ang][r, j] - xan) <= 1e-9 * max(1.0, abs(xan)), (where, r, j)
                assert abs(got[rate][r, j] - tpol) <= 1e-9 * max(1.0, abs(tpol)), (where, r, j)
                assert abs(got[lpol][r, j] - lp) <= 1e-12 + 1e-9 * abs(lp), (where, r, j)
                some_polar = some_polar or lp > 0.0
    return some_polar


# ---------------------------------------------------------------------------------------------------------------- CPU test


def test_every_value_error_comes_before_any_library_call(pkg, tmp_path, monkeypatch):
    """The shape of the weights, a non-finite entry, a row of zeros, a row that sums to zero under normalize=True, a call that
    differs in each of the keywords that shape a block (and in -SOS.OutputAlt without `altitudes`), a result root, and the
    altitude / fluxes / split rules: ValueError naming the channel or call, with the library never touched."""
    rs = pkg.run_sos

    def no_library():
        raise AssertionError("the library was reached before the arguments were refused")

    monkeypatch.setattr(pkg.capi, "lib", no_library)
    kws = spectrum(rs, tmp_path, "lambert")
    n = len(kws)
    w = weights(n)

    def refused(match, kws_=kws, w_=w, **kw):
        with pytest.raises(ValueError, match=match):
            rs.sos_spectrum_channels(kws_, w_, **kw)

    refused(r"weights must be \[C\]\[7\]", w_=w[:, :-1])
    refused(r"weights must be \[C\]\[7\]", w_=w[0])
    refused(r"weights must be", w_=[["a"] * n])
    bad = w.copy()
    bad[2, 4] = np.nan
    refused("channel 2 for call 4 is not finite", w_=bad)
    bad[2, 4] = np.inf
    refused("channel 2 for call 4 is not finite", w_=bad, normalize=False)
    bad = w.copy()
    bad[1] = 0.0
    refused("channel 1 has no non-zero weight", w_=bad)
    bad = w.copy()
    bad[5] = 0.0
    bad[5, 1:3] = (1.0, -1.0)
    refused("channel 5 sum to 0.0", w_=bad)
    refused("normalize must be True or False", normalize=1)
    changes = {"-ANG.Rad.NbGauss": dict(nbmu_gauss_lum=12), "-ANG.Thetas": dict(tetas=30.0),
               "-ANG.Rad.UserAngFile": dict(ficangles_user_lum="angles.txt"), "-SOS.View": dict(itrphi=1),
               "-SOS.View.Phi": dict(phios=10.0), "-SOS.View.Dphi": dict(pas_phi=90), "-SOS.Ipolar": dict(ipolar=0),
               "-SOS.OutputAlt": dict(zout=2.0)}
    for name, change in changes.items():
        other = list(kws)
        other[3] = dict(kws[3], **change)
        refused(r"call 3 differs from call 0 in %s \(" % re.escape(name), kws_=other)
    other = list(kws)
    other[2] = dict(kws[2], resroot=str(tmp_path))
    refused("ResRoot of call 2 must be empty", kws_=other)
    refused("give `altitudes`", fluxes=True)
    refused("fluxes must be True or False", altitudes=ALTS, fluxes=1)
    refused("needs fluxes=True", altitudes=ALTS, split=True)
    refused("1 to 16 altitudes", altitudes=[])
    other[2] = dict(kws[2], zout=2.0)
    refused("zout must be -1", kws_=other, altitudes=ALTS)
    with pytest.raises(rs.SosProcError, match="2611"):
        rs.sos_spectrum_channels(kws, w, altitudes=[-1, 130.0])


# ---------------------------------------------------------------------------------------------------------------- GPU tests


@pytest.fixture(scope="module")
def spectra(gpu_pkg, tmp_path_factory):
    """Per variant: the calls and the 23-tuples of sos_spectrum, made once and left unchanged."""
    rs = gpu_pkg.run_sos
    old = os.environ.get("SOS_ABS_ROOT")
    os.environ["SOS_ABS_ROOT"] = GOLD
    made = {}
    try:
        for variant in VARIANTS:
            kws = spectrum(rs, tmp_path_factory.mktemp(variant), variant)
            made[variant] = (kws, rs.sos_spectrum(kws))
    finally:
        if old is None:
            os.environ.pop("SOS_ABS_ROOT")
        else:
            os.environ["SOS_ABS_ROOT"] = old
    return made


def test_the_spectrum_is_what_it_claims(pkg, monkeypatch):
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    bins = [pkg.absorption.band_bin_count(1e4 / nu, 10.0) for nu in WAVENUMBERS]
    assert len(bins) >= 6 and sum(b > 1 for b in bins) >= 4 and sum(b == 1 for b in bins) >= 2
    assert {5, 25} <= set(bins)
    assert all(13000 < nu < 13500 or 15500 < nu < 16000 for nu in WAVENUMBERS)
    w = weights(len(WAVENUMBERS))
    assert np.all(w[3] != 0) and np.count_nonzero(w[4]) == 1 and (w[5] < 0).sum() == 2
    assert all(np.any((w[a] != 0) & (w[b] != 0)) for a, b in ((0, 1), (1, 2), (0, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_channels_equal_the_host_convolution(gpu_pkg, oracle, spectra, monkeypatch, variant, normalize):
    """Lambert ground with -SOS.View 2 / Dphi 120, glitter with -SOS.View 1 (the direct term is in the blocks), -SOS.Ipolar 0:
    the summed tables equal the thresholded host sums bit for bit, sca equals a call's, ang / rate / lpol follow oracle.polar
    of the channel's own i, q, u, elements 18..22 equal the host sums bit for bit."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, ref = spectra[variant]
    w = weights(len(kws))
    got = gpu_pkg.run_sos.sos_spectrum_channels(kws, w, normalize=normalize)
    assert len(got) == len(w)
    wa = applied(w, normalize)
    nrow = 4 if variant == "lambert" else 2                 # azimuths 0, 120, 240, 360 | phi, phi + 180
    polar = [check_channel(oracle, got[c], wa[c], ref, nrow, (variant, normalize, c)) for c in range(len(w))]
    assert polar == [variant != "nopolar"] * len(w)


@pytest.mark.gpu
def test_chunk_and_parts_do_not_change_a_bit(gpu_pkg, spectra, monkeypatch):
    """chunk=2 and chunk=256, parts=1 and parts=4 (parts of one call each): all 23 elements of every channel are equal."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "1")
    rs = gpu_pkg.run_sos
    kws, _ = spectra["lambert"]
    w = weights(len(kws))
    base = rs.sos_spectrum_channels(kws, w, chunk=256, parts=1)
    for kw in (dict(chunk=2, parts=1), dict(chunk=256, parts=4), dict(chunk=3, parts=4)):
        other = rs.sos_spectrum_channels(kws, w, **kw)
        for c in range(len(w)):
            assert_tuples_equal(base[c], other[c], (kw, c))


@pytest.mark.gpu
def test_levels_and_fluxes(gpu_pkg, oracle, spectra, monkeypatch):
    """altitudes = [-1, 0, 3] with fluxes=True: chan[c][k] equals the convolution of sos_spectrum_levels' spec[i][k], the flux
    rows the host sums of its rows, bit for bit; without fluxes the tuples are the same; chunk=6 (two calls per chunk) too."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    rs = gpu_pkg.run_sos
    kws, _ = spectra["lambert"]
    w = weights(len(kws))
    spec, sflux = rs.sos_spectrum_levels(ALTS, kws, fluxes=True)
    chan, flux = rs.sos_spectrum_channels(kws, w, altitudes=ALTS, fluxes=True, split=False)
    wa = applied(w, True)
    assert len(chan) == len(flux) == len(w)
    for c in range(len(w)):
        assert len(chan[c]) == len(ALTS) and flux[c].shape == (len(ALTS), 5)
        for k in range(len(ALTS)):
            check_channel(oracle, chan[c][k], wa[c], [spec[i][k] for i in range(len(kws))], 4, ("levels", c, k))
        assert np.array_equal(flux[c], host_sum(wa[c], sflux)), c
    plain = rs.sos_spectrum_channels(kws, w, altitudes=ALTS)
    small, sflux2 = rs.sos_spectrum_channels(kws, w, altitudes=ALTS, fluxes=True, chunk=6)
    for c in range(len(w)):
        assert np.array_equal(sflux2[c], flux[c])
        for k in range(len(ALTS)):
            assert_tuples_equal(chan[c][k], plain[c][k], ("plain", c, k))
            assert_tuples_equal(chan[c][k], small[c][k], ("chunk 6", c, k))


@pytest.mark.gpu
def test_levels_with_split_fluxes(gpu_pkg, spectra, monkeypatch):
    """split=True: flux[c] is [K][7], the host sums of the [K][7] rows of sos_spectrum_levels(..., split=True) bit for bit."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    rs = gpu_pkg.run_sos
    kws, _ = spectra["lambert"]
    w = weights(len(kws))
    wa = applied(w, False)
    chan, flux = rs.sos_spectrum_channels(kws, w, normalize=False, altitudes=ALTS, fluxes=True, split=True)
    spec, sflux = rs.sos_spectrum_levels(ALTS, kws, fluxes=True, split=True)
    for c in range(len(w)):
        assert flux[c].shape == (len(ALTS), 7) and np.array_equal(flux[c], host_sum(wa[c], sflux)), c
        for k in range(len(ALTS)):
            for e in SUMMED + (18, 19, 20, 21, 22):
                ref = host_sum(wa[c], [spec[i][k][e] for i in range(len(kws))])
                assert np.array_equal(np.asarray(chan[c][k][e]), thresholds(ref, e) if e in SUMMED else ref), (c, k, e)


def _count(monkeypatch, pkg):
    n = dict(accumulate=0, finish=0, trphi=0, jobs=[])
    L = pkg.capi.lib()
    fa, ff, ft = L.sosgpu_channel_accumulate, L.sosgpu_channel_finish, L.sosgpu_trphi_spectrum

    def accumulate(*a):
        n["accumulate"] += 1
        n["jobs"].append(int(a[2]))
        return fa(*a)

    def finish(*a):
        n["finish"] += 1
        return ff(*a)

    def trphi(*a):
        n["trphi"] += 1
        return ft(*a)

    monkeypatch.setattr(L, "sosgpu_channel_accumulate", accumulate)
    monkeypatch.setattr(L, "sosgpu_channel_finish", finish)
    monkeypatch.setattr(L, "sosgpu_trphi_spectrum", trphi)
    return n


@pytest.mark.gpu
def test_library_calls(gpu_pkg, spectra, monkeypatch):
    """sosgpu_channel_accumulate once per chunk (with the chunk's calls as jobs), sosgpu_channel_finish once, behind one
    sosgpu_trphi_spectrum call per chunk; sos_spectrum and sos_spectrum_levels call neither, make their one recomposition call
    per chunk as before and return the tuples of the module's reference run, array by array."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    rs = gpu_pkg.run_sos
    kws, ref = spectra["lambert"]
    w = weights(len(kws))
    n = _count(monkeypatch, gpu_pkg)
    rs.sos_spectrum_channels(kws, w)
    assert (n["accumulate"], n["finish"], n["trphi"], n["jobs"]) == (1, 1, 1, [7]), n
    n.update(accumulate=0, finish=0, trphi=0, jobs=[])
    rs.sos_spectrum_channels(kws, w, chunk=2)
    assert (n["accumulate"], n["finish"], n["trphi"], n["jobs"]) == (4, 1, 4, [2, 2, 2, 1]), n
    n.update(accumulate=0, finish=0, trphi=0, jobs=[])
    rs.sos_spectrum_channels(kws, w, altitudes=ALTS, fluxes=True, chunk=6)
    assert (n["accumulate"], n["finish"], n["trphi"], n["jobs"]) == (4, 1, 4, [2, 2, 2, 1]), n
    n.update(accumulate=0, finish=0, trphi=0, jobs=[])
    again = rs.sos_spectrum(kws, chunk=2)
    assert (n["accumulate"], n["finish"], n["trphi"]) == (0, 0, 4), n
    for i, (a, b) in enumerate(zip(again, ref)):
        assert_tuples_equal(a, b, ("sos_spectrum", i))
    n.update(trphi=0)
    rs.sos_spectrum_levels(ALTS, kws)
    assert (n["accumulate"], n["finish"], n["trphi"]) == (0, 0, 1), n
