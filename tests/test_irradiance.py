"""The irradiance-only spectrum pass, without a device: the C surface of sosgpu_level_irradiance and its refusals, the argument
rules of run_sos.sos_spectrum_irradiances (each raised before any library call), the weighted sums against an explicit host
loop, the altitude groups, and the one statement of the -ln of the band transmissions that dist.finish_scalars and
dist.finish_irradiance share."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def test_surface_is_declared_exported_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"#define\s+SOSGPU_IRRADIANCE_COLS\s+14\b", hdr) and pkg.capi.IRRADIANCE_COLS == 14
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int sosgpu_level_irradiance(sosgpu_ctx *cx, const void *d_table , const int32_t *d_ctx_of_bin , int nb, int lp, "
            "const int32_t *d_nt, const double *d_prof, const double *d_zprof , int nz, const int32_t *d_jout, const double *d_zz, "
            "const double *d_tauout , const double *d_rec , const int32_t *d_norders, const double *d_flux , "
            "const double *d_scal , const double *d_tauvrai , int nseg, const int32_t *d_seg, const double *d_aik, "
            "double *d_out , void *stream);") in flat
    assert "iborm_max of the context may be 0" in re.sub(r"\s+", " ", hdr)
    assert "sosgpu_level_irradiance" in pkg.capi.EXPORTS and hasattr(pkg.capi.lib(), "sosgpu_level_irradiance")
    assert len(pkg.capi.lib().sosgpu_level_irradiance.argtypes) == 22
    assert callable(pkg.run_sos.sos_spectrum_irradiances) and callable(pkg.solver.level_irradiance_spectrum)
    assert callable(pkg.SosContext.level_irradiance)


def test_arguments_are_refused_without_a_device(pkg):
    """Every refusal of the header -- sosgpu_level_absorption's list, plus a NULL d_flux or d_scal -- and the two empty calls,
    before any device is looked for: the pointers are never dereferenced, nothing is queued.  d_tauvrai may be NULL."""
    f = pkg.capi.lib().sosgpu_level_irradiance
    p = C.c_void_p(4096)
    #       cx table cob nb lp nt prof zprof nz jout zz tauout rec norders flux scal tauvrai nseg seg aik out stream
    good = [p, None, None, 3, 16, p, p, p, 2, p, p, p, p, p, p, p, None, 1, p, p, p, None]
    for i in (0, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 18, 19, 20):          # a NULL required pointer
        bad = list(good)
        bad[i] = None
        assert f(*bad) == E_ARG, i
    for i, v in ((8, 0), (8, 17), (8, -1), (4, 1), (4, 0), (3, -1), (17, -1)):   # nz, lp, nb, nseg out of range
        bad = list(good)
        bad[i] = v
        assert f(*bad) == E_ARG, (i, v)
    bad = list(good)
    bad[1] = p                                                             # a table without d_ctx_of_bin
    assert f(*bad) == E_ARG
    for i in (3, 17):                                                      # nb = 0, nseg = 0: nothing queued
        for tv in (None, p):
            ok = list(good)
            ok[i], ok[16] = 0, tv
            assert f(*ok) == 0
            ok[1], ok[2] = p, p
            assert f(*ok) == 0
            ok[8] = 17                                                     # ... but still checked
            assert f(*ok) == E_ARG


def _kw(rs):
    return rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), {"-SOS_Main.Wa": 0.55, "-AER.AOTref": 0.0}), trace=False)


def test_keyword_rules_before_any_library_call(pkg, monkeypatch):
    rs = pkg.run_sos
    monkeypatch.setattr(pkg.capi, "lib", lambda: pytest.fail("a keyword rule reached the library"))
    monkeypatch.setattr(rs, "_spectrum_pass", lambda *a, **k: pytest.fail("a keyword rule reached the pass"))
    kw = _kw(rs)
    f = rs.sos_spectrum_irradiances
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="split must be True or False"):
            f([1.0], [kw], split=bad)
        with pytest.raises(ValueError, match="absorption must be True or False"):
            f([1.0], [kw], absorption=bad)
        with pytest.raises(ValueError, match="normalize must be True or False"):
            f([1.0], [kw], weights=[[1.0]], normalize=bad)
    with pytest.raises(ValueError, match="at least one altitude"):
        f([], [kw])
    with pytest.raises(ValueError, match="at least one altitude"):
        f([], [])                                                          # ... before the empty-spectrum shortcut
    # weights of the wrong shape: [R][calls] or [R][K][calls] only
    for w in ([1.0, 2.0], [[1.0]], [[1.0, 2.0, 3.0]], [[[1.0, 2.0]]], [[[1.0, 2.0]] * 3], np.ones((1, 2, 2, 2)), [["a", "b"]],
              np.ones((0, 2))):
        with pytest.raises(ValueError, match="weights must be"):
            f([1.0, 2.0], [kw, kw], weights=w)
    for v in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="sum 1 at altitude 0 for call 1 is not finite"):
            f([1.0, 2.0], [kw, kw], weights=[[1.0, 1.0], [1.0, v]])
        with pytest.raises(ValueError, match="sum 0 at altitude 1 for call 0 is not finite"):
            f([1.0, 2.0], [kw, kw], weights=[[[1.0, 1.0], [v, 1.0]]])
    with pytest.raises(ValueError, match="cannot be normalised"):
        f([1.0], [kw, kw], weights=[[1.0, -1.0]], normalize=True)
    # the rules of the calls: those of sos_spectrum_levels, and -SOS.Trans at NO_OUTPUT
    with pytest.raises(ValueError, match="zout must be -1"):
        f([1.0], [dict(kw, zout=2.0)])
    with pytest.raises(ValueError, match="ResRoot must be empty"):
        f([1.0], [dict(kw, resroot="/tmp/x")])
    with pytest.raises(ValueError, match="call 1 asks for the -SOS.Trans file"):
        f([1.0], [kw, dict(kw, fictrans="Trans.txt")])
    with pytest.raises(rs.SosProcError) as e:
        f([1.0] * 16 + [130.0], [kw])                                      # the -SOS.OutputAlt rule holds in every group
    assert e.value.code == 2611
    monkeypatch.undo()
    assert rs.sos_spectrum_irradiances([-1.0, 3.0], []) == []
    assert rs.sos_spectrum_irradiances([-1.0, 3.0], [], split=True, absorption=True) == ([], [])


def test_existing_entry_points_take_no_new_keyword(pkg):
    import inspect
    rs = pkg.run_sos
    for fn in (rs.sos_spectrum, rs.sos_spectrum_levels, rs.sos_spectrum_channels, rs.sos_proc_levels):
        names = set(inspect.signature(fn).parameters)
        assert not names & {"irr", "order0", "irradiances"}, fn.__name__
    assert inspect.signature(rs._spectrum_pass).parameters["irr"].default is False
    assert inspect.signature(rs._prepare).parameters["order0"].default is False


def _host_loop(wts, rows):
    """The sums the issue defines: per sum r, altitude k and column c, a = a + w * x over the calls in ascending index, a call
    of weight 0 skipped -- in Python floats, one element at a time."""
    nr, nk, nwl = wts.shape
    ncol = rows[0].shape[1]
    out = np.zeros((nr, nk, ncol))
    for r in range(nr):
        for k in range(nk):
            for c in range(ncol):
                a = 0.0
                for i in range(nwl):
                    w = float(wts[r, k, i])
                    if w == 0.0:
                        continue
                    a = a + w * float(rows[i][k, c])
                out[r, k, c] = a
    return out


def test_weighted_sums_equal_the_host_loop(pkg):
    """normalize, a weight-0 call, per-altitude weights and a NaN row: bit for bit against the explicit loop."""
    rs = pkg.run_sos
    rng = np.random.default_rng(11)
    nwl, nk, ncol = 7, 3, 5
    rows = [rng.uniform(0.0, 1.0, (nk, ncol)) * 10.0 ** rng.integers(-8, 3, (nk, ncol)) for _ in range(nwl)]
    for i in range(nwl):
        rows[i][0] = np.nan                                                # the absorption row of altitude -1
    rows[4][2] = np.nan                                                    # ... and one NaN row that only weight 0 keeps out
    flat = rng.uniform(-2.0, 3.0, (2, nwl))
    flat[0, 2] = 0.0                                                       # a weight-0 call
    flat[1, 4] = 0.0                                                       # ... the one whose row 2 is NaN
    per_alt = rng.uniform(0.1, 3.0, (2, nk, nwl))
    per_alt[0, 1, :3] = 0.0
    per_alt[1, 2, 4] = 0.0
    for weights, normalize in ((flat, False), (flat, True), (per_alt, False), (per_alt, True)):
        wts = rs._irradiance_weights("t", weights, normalize, nwl, nk)
        assert wts.shape == (2, nk, nwl) and wts.dtype == np.float64
        if normalize:                                                      # each weight row divided by its left-to-right sum
            w3 = np.repeat(weights[:, None, :], nk, axis=1) if weights.ndim == 2 else weights
            for r in range(2):
                for k in range(nk):
                    tot = 0.0
                    for x in w3[r, k]:
                        tot = tot + float(x)
                    assert wts[r, k].tolist() == [float(x) / tot for x in w3[r, k]]
        elif weights.ndim == 2:
            assert all(np.array_equal(wts[:, k], weights) for k in range(nk))
        else:
            assert np.array_equal(wts, weights)
        got = rs._weighted_rows(wts, rows)
        want = _host_loop(wts, rows)
        assert got.shape == want.shape == (2, nk, ncol)
        assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4]
        assert np.isnan(got[:, 0]).all()                                   # a NaN row stays NaN
        assert np.isnan(got[0, 2]).all() and np.isfinite(got[1, 2]).all()  # ... unless its weight is 0: the call is skipped
        assert np.isfinite(got[:, 1]).all()
    # the order of the additions is the call index: a sum that rounds differently backwards
    w = rs._irradiance_weights("t", [[1.0, 1.0, 1.0]], False, 3, 1)
    r3 = [np.array([[1.0]]), np.array([[2.0 ** -53]]), np.array([[2.0 ** -53]])]
    assert rs._weighted_rows(w, r3)[0, 0, 0] == 1.0 and (2.0 ** -53 + 2.0 ** -53) + 1.0 > 1.0


def test_altitude_groups(pkg):
    rs = pkg.run_sos
    size = pkg.capi.MAX_OUTPUT_LEVELS
    assert size == 16
    assert rs._altitude_groups(1, size) == [(0, 1)]
    assert rs._altitude_groups(16, size) == [(0, 16)]
    assert rs._altitude_groups(17, size) == [(0, 16), (16, 17)]
    assert rs._altitude_groups(33, size) == [(0, 16), (16, 32), (32, 33)]
    for k in (1, 16, 17, 33):
        g = rs._altitude_groups(k, size)
        assert [i for k0, k1 in g for i in range(k0, k1)] == list(range(k)) and all(1 <= k1 - k0 <= size for k0, k1 in g)


def test_groups_are_one_pass_each_over_the_same_calls(pkg, monkeypatch):
    """K = 17 and 33: one irradiance pass per group of 16, each over the whole call list with its own altitudes; the rows are
    joined in the order of `altitudes`, and the weighted sums are formed from the joined rows."""
    rs = pkg.run_sos
    kw = _kw(rs)
    seen = []

    def fake_pass(fn, kwargs_list, aer_phases, device, gather, chunk, timings, prep_streams, parts, alts, fluxes, split, **k):
        assert fn == "sos_spectrum_irradiances" and fluxes is True and k["irr"] is True
        seen.append((list(alts), len(kwargs_list), gather, k["absorption"]))
        flux = [np.array([[z + 100.0 * i] * (7 if split else 5) for z in alts]) for i in range(len(kwargs_list))]
        absorb = [np.array([[math.nan if z == -1.0 else z - 100.0 * i] * 5 for z in alts]) for i in range(len(kwargs_list))]
        return (flux, absorb) if k["absorption"] else flux

    monkeypatch.setattr(rs, "_spectrum_pass", fake_pass)
    for nk in (1, 16, 17, 33):
        del seen[:]
        alts = [-1.0] + [0.5 * j for j in range(1, nk)]
        flux = rs.sos_spectrum_irradiances(alts, [kw, kw, kw])
        assert [s[0] for s in seen] == [alts[k0:k1] for k0, k1 in rs._altitude_groups(nk, 16)]
        assert all(s[1:] == (3, True, False) for s in seen)
        assert len(flux) == 3 and all(f.shape == (nk, 5) for f in flux)
        assert all(flux[i][:, 0].tolist() == [z + 100.0 * i for z in alts] for i in range(3))
    del seen[:]
    alts = [-1.0] + [0.5 * j for j in range(1, 17)]
    w = np.array([[1.0, 0.0, 2.0]])
    fs, ab = rs.sos_spectrum_irradiances(alts, [kw, kw, kw], split=True, absorption=True, weights=w, gather=False)
    assert len(seen) == 2 and all(s[2] is True and s[3] is True for s in seen)     # (weights: the rows are gathered)
    assert fs.shape == (1, 17, 7) and ab.shape == (1, 17, 5)
    assert fs[0, :, 0].tolist() == [1.0 * z + 2.0 * (z + 200.0) for z in alts]
    assert math.isnan(ab[0, 0, 0]) and ab[0, 1:, 4].tolist() == [1.0 * z + 2.0 * (z - 200.0) for z in alts[1:]]


def test_depths_are_stated_once(pkg):
    """finish_scalars and finish_irradiance apply the same -ln statements (dist.finish_depths) to their columns."""
    d = pkg.dist
    rng = np.random.default_rng(3)
    n = 4
    scal = rng.uniform(0.01, 1.0, (3, 10 + n))
    scal[:, 7], scal[:, 8] = 3.0, [-3.0, 1.0, -0.0]
    scal[1, 9] = 0.0                                                       # (no true depth written: inf)
    fin = d.finish_scalars(scal)
    assert set(fin) == {"tdifmus", "emoins", "eplus", "ttot_tronc", "ttot_vrai", "tauout", "sum_aik", "n_orders", "min_orders",
                        "tdifmug", "tauvrai_out"}
    block = np.zeros((3, pkg.capi.IRRADIANCE_COLS))
    block[:, 6:9], block[:, 9], block[:, 10], block[:, 11] = scal[:, 3:6], scal[:, 6], scal[:, 8], scal[:, 9]
    irr = d.finish_irradiance(block)
    assert set(irr) == {"ttot_tronc", "ttot_vrai", "tauout", "tauvrai_out", "min_orders", "sum_aik"}
    for k in irr:
        assert np.array_equal(irr[k], fin[k]) and irr[k].dtype == fin[k].dtype, k
    assert fin["min_orders"].tolist() == [3, -1, 0] and math.isinf(fin["tauvrai_out"][1])
    assert np.array_equal(fin["ttot_tronc"], -np.log(scal[:, 3]))
