"""The aerosol-layer profile (-AP.AerProfile.Type 2) without a GPU: the level grid stated once in Python (geometry.layer_grid)
and once in C (sosgpu_profile_layer_grid), the condition that makes "bit for bit" a fair bar for the device (no entry of a
committed cell moves when every exp / log result moves by an ulp or two), the packing of a spectrum's layer requests, and the
refusals the two entry points decide before any device call."""
import ctypes as C
import math
import os
import zlib

import numpy as np
import pytest

import layer_cells
from layer_cells import CELLS, E_ARG, E_UNSUPPORTED, PARAMS, REFUSALS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _c_grid(L, cell):
    counts = (C.c_int32 * 4)(-7, -7, -7, -7)
    return int(L.sosgpu_profile_layer_grid(*[float(v) for v in cell], counts)), tuple(int(c) for c in counts)


def test_cells_have_the_counts_they_claim(pkg):
    for cell, nt, counts in CELLS:
        got = pkg.geometry.layer_grid(*cell)
        assert got[0] == nt, (cell, got)
        assert counts is None or got[1:] == counts, (cell, got)
        assert got[0] == (1 if cell[3] == 0.0 else 2) + sum(got[1:]) and 8 <= nt <= 600
    assert sorted({c[1] for c in CELLS})[:2] == [8, 14] and max(c[1] for c in CELLS) == 600


def test_c_grid_equals_the_python_grid(pkg):
    """Equal integers and equal refusals: on every cell, on the refusals (both codes) and on 2000 seeded random draws."""
    L, G = pkg.capi.lib(), pkg.geometry
    for cell in PARAMS:
        nt, counts = _c_grid(L, cell)
        assert (nt,) + counts[1:] == G.layer_grid(*cell) and counts[0] == nt, cell
    for cell, code, text in REFUSALS:
        rc, counts = _c_grid(L, cell)
        assert rc == code and counts == (-7, -7, -7, -7), (cell, rc, counts)
        with pytest.raises(pkg.run_sos.SosProcError, match=text):
            G.layer_grid(*cell)
    assert L.sosgpu_profile_layer_grid(0.1, 8.0, 0.3, 1.0, 3.0, None) == E_ARG
    rng = np.random.default_rng(20260)
    refused = 0
    for _ in range(2000):
        tr, ta, hr = rng.uniform(0.01, 0.4), 10 ** rng.uniform(-5, math.log10(3.5)), rng.uniform(6.0, 9.0)
        zmin = 0.0 if rng.random() < 0.3 else rng.uniform(0.02, 10.0)
        cell = (tr, hr, ta, zmin, zmin + rng.uniform(0.2, 5.0))
        rc, counts = _c_grid(L, cell)
        try:
            want = G.layer_grid(*cell)
        except pkg.run_sos.SosProcError as e:
            refused += 1
            assert rc == (E_UNSUPPORTED if "1020" in str(e) else E_ARG), (cell, rc, str(e))
            continue
        assert rc == want[0] and counts == want, (cell, rc, counts, want)
    assert 0 < refused < 2000                     # (the draws reach both sides)


def test_profile_layer_keeps_its_lengths_and_the_golden(pkg):
    G = pkg.geometry
    for cell in PARAMS:
        h, xdel, ydel, z = G.profile_layer(*cell)
        nt = G.layer_grid(*cell)[0]
        assert len(h) == len(xdel) == len(ydel) == len(z) == nt + 1, cell
    g = np.load(os.path.join(GOLD, "profile_layer.npz"))
    for i, case in enumerate(g["cases"]):
        h, xdel, ydel, z = G.profile_layer(*[float(v) for v in case])
        assert len(h) == G.layer_grid(*[float(v) for v in case])[0] + 1 == len(g["h_%d" % i])
        assert np.array_equal(h, g["h_%d" % i]) and np.array_equal(z, g["zprof_%d" % i]), i


class _PushedMath:
    """geometry.math with every exp and log result moved: by a fixed number of ulps, or by a pseudo-random +-1 ulp (key)."""

    def __init__(self, ulps=0, key=None):
        self.ulps, self.key, self.calls = ulps, key, 0

    def _push(self, name, x, v):
        self.calls += 1
        k = self.ulps
        if self.key is not None:
            k = 1 if zlib.crc32(("%s %r %d" % (name, x, self.key)).encode()) & 1 else -1
        for _ in range(abs(k)):
            v = math.nextafter(v, math.inf if k > 0 else -math.inf)
        return v

    def exp(self, x):
        return self._push("exp", x, math.exp(x))

    def log(self, x):
        return self._push("log", x, math.log(x))

    def __getattr__(self, name):
        return getattr(math, name)


VARIANTS = [dict(ulps=1), dict(ulps=-1), dict(ulps=2), dict(ulps=-2), dict(key=1), dict(key=2)]


def test_no_entry_of_a_cell_depends_on_the_last_bits_of_exp_and_log(pkg, monkeypatch):
    """The condition of the bit-for-bit bar: profile_layer with every exp / log result moved by +1, -1, +2, -2 ulp and by a
    pseudo-random +-1 ulp (two keys) returns the entries of the exact run, all of them, on every committed cell; NT and the
    counts do not move; zprof is strictly decreasing.  No entry is excused."""
    G = pkg.geometry
    exact = {cell: (G.layer_grid(*cell), G.profile_layer(*cell)) for cell in PARAMS}
    entries = moved = 0
    for v in VARIANTS:
        stand_in = _PushedMath(**v)
        monkeypatch.setattr(G, "math", stand_in)
        for cell in PARAMS:
            grid, prof = exact[cell]
            assert G.layer_grid(*cell) == grid, (v, cell)
            got = G.profile_layer(*cell)
            for a, b in zip(got, prof):
                entries += a.size
                moved += int((a != b).sum())
                # (values: a ground layer's last altitude is hr log(tr / (tr exp(-0 / hr))), a zero whose sign follows the push)
                assert np.array_equal(a, b), (v, cell, np.flatnonzero(a != b).tolist())
        assert stand_in.calls > 0
        monkeypatch.undo()
    assert G.math is math
    print("entries compared: %d, moved: %d" % (entries, moved))
    assert moved == 0
    for cell in PARAMS:
        z = exact[cell][1][3]
        assert np.all(np.diff(z) < 0.0), (cell, np.flatnonzero(np.diff(z) >= 0.0).tolist())


def _request(cell, **kw):
    r = dict(zip(("tr", "hr", "ta", "zmin", "zmax"), cell), a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, smax=8)
    r.update(kw)
    return r


def test_packing_of_layer_requests(pkg):
    """One record per wavelength in one buffer, a bin per wavelength, sections of the one block that neither overlap nor leave
    the int32 block misaligned; the work section is what the library asks for."""
    S, L = pkg.solver, pkg.capi.lib()
    reqs = [_request(PARAMS[4], zout=2.0, smax=5), _request(PARAMS[0], a_tronc=0.35, piz=0.9, piztr=0.93), _request(PARAMS[11])]
    for true_depth in (False, True):
        pk = S.pack_layer_requests(reqs, lp=608, true_depth=true_depth)
        wl = pk["wl"]
        assert wl.dtype == pkg.capi.LAYER_WL_DTYPE and wl.dtype.itemsize == C.sizeof(pkg.capi.LayerWl) == 80
        assert wl.flags.c_contiguous and wl.shape == (3,)
        assert [tuple(float(w[k]) for k in ("tr", "hr", "ta", "zmin", "zmax")) for w in wl] == [PARAMS[4], PARAMS[0], PARAMS[11]]
        assert wl["zout"].tolist() == [2.0, -1.0, -1.0] and wl["smax"].tolist() == [5, 8, 8] and wl["reserved"].tolist() == [0, 0, 0]
        assert (wl["a_tronc"][1], wl["piz"][1], wl["piztr"][1]) == (0.35, 0.9, 0.93)
        assert pk["nb"] == 3 and pk["seg"].tolist() == [0, 1, 2, 3]
        off, nb, lp = pk["off"], 3, 608
        sizes = dict(prof=nb * 3 * lp, zprof=nb * lp, scal=4 * nb, zz=nb, hvrai=nb * lp if true_depth else 0,
                     work=pk["work_doubles"], ints=2 * nb - nb // 2)
        at = 0
        for name in ("prof", "zprof", "scal", "zz", "hvrai", "work", "ints"):
            assert off[name] == at, (name, off)
            at += sizes[name]
        assert pk["doubles"] == at and 2 * sizes["ints"] >= 3 * nb
        assert 8 * pk["work_doubles"] == L.sosgpu_profile_layer_spectrum_work_bytes(nb) == nb * pkg.capi.LAYER_ENTRY_BYTES
    assert L.sosgpu_profile_layer_spectrum_work_bytes(0) == 0 and L.sosgpu_profile_layer_spectrum_work_bytes(-3) == 0
    assert pkg.solver.pack_layer_requests([], lp=16)["doubles"] == 0


def test_row_length_keeps_the_level_class_of_the_host_profile(pkg):
    """solver.layer_lp(nt) holds the profile and falls in the class (lp <= 32, <= 64, above: what selects the solver kernel) of
    the row upload_bins gives the host profile of nt levels."""
    cls = lambda lp: 0 if lp <= 32 else 1 if lp <= 64 else 2
    for nt in range(1, 601):
        lp = pkg.solver.layer_lp(nt)
        assert nt < lp <= 608 and cls(lp) == cls(-(-(nt + 1) // 16) * 16), nt
    assert {pkg.solver.layer_lp(nt) for nt in (8, 31, 32, 63, 64, 600)} == {32, 64, 608}


def test_refusals_decided_before_any_device_call(pkg):
    """Argument, work-area and grid refusals of the two entry points: returned on the host (this test has no device), with
    the index of the refused wavelength."""
    L = pkg.capi.lib()
    S = pkg.solver
    host = np.zeros(4096, dtype=np.float64)                     # (never dereferenced: the calls end before the device)
    p = C.c_void_p(host.ctypes.data)
    fake_ctx = C.c_void_p(host.ctypes.data)
    cell = PARAMS[4]
    # --- single form
    outs = [p] * 7 + [None]
    assert L.sosgpu_profile_layer(None, *cell, 0.0, 1.0, 1.0, -1.0, 608, *outs, None) == E_ARG
    assert L.sosgpu_profile_layer(fake_ctx, *cell, 0.0, 1.0, 1.0, -1.0, 1, *outs, None) == E_ARG                  # lp < 2
    assert L.sosgpu_profile_layer(fake_ctx, *cell, 0.0, 1.0, 1.0, -1.0, 608, None, *outs[1:], None) == E_ARG      # no d_prof
    assert L.sosgpu_profile_layer(fake_ctx, *cell, 0.0, 1.0, 1.0, -1.0, 608, p, p, p, p, p, None, p, None, None) == E_ARG
    assert L.sosgpu_profile_layer(fake_ctx, *cell, 0.0, 1.0, 1.0, 2.0, 608, p, p, p, p, None, None, p, None, None) == E_ARG
    for bad, code, _ in REFUSALS:
        assert L.sosgpu_profile_layer(fake_ctx, *bad, 0.0, 1.0, 1.0, -1.0, 608, *outs, None) == code, bad
    # --- table form
    pk = S.pack_layer_requests([_request(c) for c in PARAMS[:3]])
    wl = pk["wl"].ctypes.data_as(C.c_void_p)
    need = int(L.sosgpu_profile_layer_spectrum_work_bytes(3))
    bad = C.c_int(5)
    tail = [p] * 7 + [None, C.byref(bad), None]

    def call(nwl=3, table=wl, lp=608, work=p, nbytes=need, outs=None):
        bad.value = 5
        return L.sosgpu_profile_layer_spectrum(0, nwl, table, lp, work, nbytes, *(outs or tail))

    assert call(nwl=0) == E_ARG and call(table=None) == E_ARG and call(lp=1) == E_ARG
    assert call(work=None) == E_ARG and call(nbytes=need - 1) == E_ARG and bad.value == -1
    assert call(work=C.c_void_p(host.ctypes.data + 4)) == E_ARG                                    # misaligned
    assert call(outs=[None] + tail[1:]) == E_ARG and call(outs=[p, p, p, p, p, None, p, None, C.byref(bad), None]) == E_ARG
    for k, (cellk, code, _) in enumerate(REFUSALS):
        reqs = [_request(c) for c in PARAMS[:3]]
        reqs[k % 3] = _request(cellk)
        pkb = S.pack_layer_requests(reqs)
        assert call(table=pkb["wl"].ctypes.data_as(C.c_void_p)) == code and bad.value == k % 3, (cellk, bad.value)
    # an output altitude without d_jout / d_zz, a negative smax
    pkz = S.pack_layer_requests([_request(PARAMS[0]), _request(PARAMS[1], zout=0.5), _request(PARAMS[2])])
    assert call(table=pkz["wl"].ctypes.data_as(C.c_void_p), outs=[p, p, p, p, None, None, p, None, C.byref(bad), None]) == E_ARG
    assert bad.value == 1
    pks = S.pack_layer_requests([_request(PARAMS[0]), _request(PARAMS[1]), _request(PARAMS[2], smax=-1)])
    assert call(table=pks["wl"].ctypes.data_as(C.c_void_p)) == E_ARG and bad.value == 2


def test_layer_cells_host_chain_shapes(pkg):
    """The host chain of the GPU tests on the smallest cell: the layout and the statements of run_sos._layer_profile."""
    cell = PARAMS[0]
    for zout in layer_cells.tail_zouts(cell):
        c = layer_cells.host_chain(pkg, cell, a_tronc=0.35, piz=layer_cells.PIZ, piztr=0.93, zout=zout)
        assert c["nt"] == 8 and c["prof"].shape == (3, 608) and c["iborm"] == 8
        assert (c["jout"] == 0) == (zout == -1.0) and 0 <= c["jout"] <= 8
        assert c["scal"][2] == c["hvrai"][8] and c["scal"][1] == c["prof"][0, 8] and c["scal"][1] < c["scal"][2]
    assert layer_cells.host_chain(pkg, cell, piztr=0.0)["iborm"] == 2
