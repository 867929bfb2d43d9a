"""The true direct / diffuse split of the down-going flux at every output altitude (split=True of run_sos.sos_proc_levels and
sos_spectrum_levels): the CPU side -- the C ABI of the four entry points it adds (declared, exported, listed; the refusals
before any device work), the keyword rules, the columns of a split row, the new key of dist.finish_scalars.
The GPU side is tests/test_level_split_gpu.py."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NEW = ("sosgpu_profile_true", "sosgpu_profile_spectrum_true", "sosgpu_output_depths", "sosgpu_level_transmission")


def test_symbols_are_declared_exported_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"\bint\s+sosgpu_profile_true\s*\(sosgpu_ctx \*cx, int nb,[^;]*const double \*d_nogas, double \*d_hvrai,\s*"
                     r"void \*stream\);", hdr)
    assert re.search(r"\bint\s+sosgpu_profile_spectrum_true\s*\(int device, int nwl,[^;]*int \*bad_wl, double \*d_hvrai,\s*"
                     r"void \*stream\);", hdr)
    assert re.search(r"\bint\s+sosgpu_output_depths\s*\(int device, int nb, int lp, const double \*d_h, size_t h_stride,\s*"
                     r"const double \*d_zprof,\s*const int32_t \*d_nt, int nz, const double \*zout, double \*d_tau,\s*"
                     r"void \*stream\);", hdr)
    assert re.search(r"\bint\s+sosgpu_level_transmission\s*\(int device, int nb, int nseg, const int32_t \*d_seg,\s*"
                     r"const double \*d_aik,\s*const int32_t \*d_norders,\s*int nz, const double \*d_tau, double \*d_out_scal,\s*"
                     r"size_t slot_stride,\s*int block_width,\s*void \*stream\);", hdr)
    L = pkg.capi.lib()
    for sym in NEW:
        assert sym in pkg.capi.EXPORTS
        assert hasattr(L, sym) and getattr(L, sym).argtypes is not None
    # the old entry points keep their signatures: one argument fewer than their twins
    assert len(L.sosgpu_profile_true.argtypes) == len(L.sosgpu_profile.argtypes) + 1
    assert len(L.sosgpu_profile_spectrum_true.argtypes) == len(L.sosgpu_profile_spectrum.argtypes) + 1
    rs = pkg.run_sos
    assert rs.LEVEL_FLUX_SPLIT_NAMES == rs.LEVEL_FLUX_NAMES + ["flux_dir_down", "flux_diff_down"]
    assert rs.LEVEL_FLUX_NAMES == ["flux_dir_down_tronc", "flux_diff_down_tronc", "flux_tot_down", "flux_diff_up", "flux_net"]


def test_arguments_are_refused_without_a_device(pkg):
    """Every NULL pointer, nz = 0 and 17, nb = -1 of sosgpu_output_depths and sosgpu_level_transmission; a stride shorter than
    a row, a block narrower than the scalar base and slots that would overlap; nb = 0 is accepted and queues nothing -- all
    before any device is looked for."""
    L = pkg.capi.lib()
    p = C.c_void_p(4096)                                     # never dereferenced: nothing is queued by these calls
    z = (C.c_double * 16)(*([-1.0] * 16))
    good = [0, 4, 32, p, 32, p, p, 2, z, p, None]
    assert L.sosgpu_output_depths(*[0, 0] + good[2:]) == 0
    for i in (3, 5, 6, 8, 9):                                # d_h, d_zprof, d_nt, zout, d_tau
        a = list(good)
        a[i] = None
        assert L.sosgpu_output_depths(*a) == E_ARG, i
    for i, v in ((1, -1), (7, 0), (7, 17), (2, 1), (4, 31)):  # nb, nz, nz, lp, h_stride
        a = list(good)
        a[i] = v
        assert L.sosgpu_output_depths(*a) == E_ARG, (i, v)
    good = [0, 4, 2, p, p, p, 3, p, p, 2 * 19, 19, None]
    assert L.sosgpu_level_transmission(*[0, 0] + good[2:]) == 0
    for i in (3, 4, 5, 7, 8):                                # d_seg, d_aik, d_norders, d_tau, d_out_scal
        a = list(good)
        a[i] = None
        assert L.sosgpu_level_transmission(*a) == E_ARG, i
    for i, v in ((1, -1), (6, 0), (6, 17), (2, 0), (2, 5), (10, 9), (9, 37)):   # nb, nz, nz, nseg, nseg > nb, width, stride
        a = list(good)
        a[i] = v
        assert L.sosgpu_level_transmission(*a) == E_ARG, (i, v)
    # the twins of the profile entry points keep their neighbours' refusals (NULL context / no wavelength)
    assert L.sosgpu_profile_true(None, 1, 0.1, 8.0, 0.1, 2.0, 7, 0, None, None, 0.0, 1.0, 1.0, -1.0, 608, p, p, p, p, None, None,
                                 p, None, p, None) == E_ARG
    assert L.sosgpu_profile_spectrum_true(0, 0, p, 1, p, None, None, 0, 0, 608, p, 1 << 30, None, p, p, p, p, None, None, p, None, p,
                                          None) == E_ARG


def test_split_must_be_a_bool_and_needs_fluxes(pkg):
    rs = pkg.run_sos
    kw = rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), {"-SOS_Main.Wa": 0.55, "-AER.AOTref": 0.0}),
                            trace=False)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError):
            rs.sos_proc_levels([1.0], fluxes=True, split=bad, **kw)
        with pytest.raises(ValueError):
            rs.sos_spectrum_levels([1.0], [kw], fluxes=True, split=bad)
    with pytest.raises(ValueError):
        rs.sos_proc_levels([1.0], fluxes=False, split=True, **kw)
    with pytest.raises(ValueError):
        rs.sos_proc_levels([1.0], split=True, **kw)
    with pytest.raises(ValueError):
        rs.sos_spectrum_levels([1.0], [kw], split=True)
    assert rs.sos_spectrum_levels([-1.0, 3.0], [], fluxes=True, split=True) == ([], [])


def test_split_row_columns(pkg):
    """The first five columns are _level_flux_row's; column 5 uses tauvrai_out at an altitude and ttot_vrai for -1; column 6
    is (E- + column 0) - column 5, the statement of _finish.  Columns 5 + 6 against column 2: column 6 is one rounding of
    column 2 - column 5 and the sum is one more, each at most half an ulp of a number no larger than column 2 -- so the sum
    is within ONE ulp of column 2 (not always equal to the last bit), asserted over many depths."""
    rs = pkg.run_sos
    pl = types.SimpleNamespace(p=dict(tetas=40.0))
    cs = math.cos(math.pi * 40.0 / 180.0)
    fin = dict(ttot_tronc=np.array([0.0, 0.5]), tauout=np.array([0.0, 0.2]), ttot_vrai=np.array([0.0, 0.7]),
               tauvrai_out=np.array([0.0, 0.3]))
    for alt, tau, tv in ((3.0, 0.2, 0.3), (-1.0, 0.5, 0.7)):
        row = rs._level_flux_split_row(pl, alt, fin, 1, (0.125, 0.0625))
        assert len(row) == len(rs.LEVEL_FLUX_SPLIT_NAMES) == 7
        assert row[:5] == rs._level_flux_row(pl, alt, fin, 1, (0.125, 0.0625))
        assert row[5] == math.exp(-tv / cs)
        assert row[6] == (0.125 + math.exp(-tau / cs)) - math.exp(-tv / cs)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(2000):
        t = float(rng.uniform(0.0, 3.0))
        fin = dict(ttot_tronc=np.array([t]), tauout=np.array([t]), ttot_vrai=np.array([t * rng.uniform(1.0, 1.5)]),
                   tauvrai_out=np.array([t * rng.uniform(1.0, 1.5)]))
        for alt in (-1.0, 2.0):
            row = rs._level_flux_split_row(pl, alt, fin, 0, (float(rng.uniform(0.0, 0.6)), 0.05))
            assert 0.0 < row[5] <= row[0]
            err = abs((row[5] + row[6]) - row[2]) / np.spacing(row[2])
            worst = max(worst, err)
            assert err <= 1.0
    print("columns 5 + 6 against column 2: at most %.1f ulp" % worst)


def test_finish_scalars_has_the_true_depth_of_the_slot(pkg):
    """tauvrai_out is -ln of element 9 (inf where sosgpu_level_transmission wrote nothing: the aggregate's 0), and no other
    key of the dictionary depends on that element."""
    fs = pkg.dist.finish_scalars
    rng = np.random.default_rng(5)
    blk = rng.uniform(0.1, 0.9, (3, 10 + 4))
    blk[:, 7], blk[:, 8], blk[:, 9] = 5.0, -3.0, 0.0
    unset = fs(blk)
    assert "tauvrai_out" in unset and np.all(np.isposinf(unset["tauvrai_out"]))
    blk2 = blk.copy()
    blk2[:, 9] = [0.5, 1.0, 1e-300]
    got = fs(blk2)
    assert np.array_equal(got["tauvrai_out"], -np.log(np.array([0.5, 1.0, 1e-300])))
    assert set(got) == set(unset)
    for k in got:
        if k != "tauvrai_out":
            assert np.array_equal(got[k], unset[k]), k
    assert set(got) - {"tauvrai_out"} == {"tdifmus", "emoins", "eplus", "ttot_tronc", "ttot_vrai", "tauout", "sum_aik",
                                          "n_orders", "min_orders", "tdifmug"}
    assert np.array_equal(got["ttot_vrai"], -np.log(blk[:, 4])) and np.array_equal(got["tdifmug"], blk[:, 10:])
