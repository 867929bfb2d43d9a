"""transmissions=True of run_sos.sos_spectrum / sos_spectrum_levels: the diffuse transmissions of the -SOS.Trans option for every
call of a spectrum as arrays, from one order-0 solve per part and direction count (solver.diffuse_transmissions_many), against
what sequential sos_proc calls with the -SOS.Trans file hand to write_trans_file.  The golden CKD fixtures through
spectrum_cases.build."""
import math
import os
import re

import numpy as np
import pytest

import spectrum_cases
from spectrum_cases import assert_tuples_equal

GOLD = spectrum_cases.GOLD
# the 5- and the 25-bin band, a no-gas call, a -SOS.AbsModeCKD 2 call and an aerosol-layer call among qualifying calls
NAMES = ["rand_12", "ckd_o2a_5bins", "cfg1_lambert", "ckd_h2o_o2_25bins_flatsea", "rand_14", "ckd_o2a_mode2", "layer_1_3km_lnd",
         "cfg2_lnd_lambert"]
KEYS = ("thetas", "thetav", "ttot_tronc", "ttot_vrai", "tdifmus", "tdifmug", "t_dir_down", "t_dif_down", "t_dif_up")


def spectrum_keywords(rs, workdir):
    """The calls as transmissions=True takes them: no -SOS.Trans file, no result directory, the standard output."""
    kws, _, _, _ = spectrum_cases.build(rs, workdir, names=NAMES)
    return [dict(kw, fictrans="NO_OUTPUT", zout=-1.0) for kw in kws]


def same_entry(a, b):
    assert set(a) == set(b) == set(KEYS)
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.fixture(scope="module")
def reference(gpu_pkg, tmp_path_factory):
    """Sequential sos_proc of every call WITH the -SOS.Trans file: the arguments write_trans_file received, the file's text; and
    sos_spectrum of the calls without the keyword.  Computed once, read only."""
    rs = gpu_pkg.run_sos
    mp = pytest.MonkeyPatch()
    mp.setenv("SOS_ABS_ROOT", GOLD)
    mp.setenv("SOS_SPECTRUM_MIN_PART", "2")
    try:
        work = tmp_path_factory.mktemp("trans_ref")
        with_files, _, _, _ = spectrum_cases.build(rs, work, names=NAMES, resroot=True)
        with_files = [dict(kw, fictrans="SOS_Transm.txt", zout=-1.0) for kw in with_files]
        seen = []
        write = rs.write_trans_file

        def capture(path, tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug):
            seen.append(dict(path=path, tetas=tetas, mu=np.array(mu), ttot_tronc=ttot_tronc, ttot_vrai=ttot_vrai, tdifmus=tdifmus,
                             tdifmug=np.array(tdifmug)))
            return write(path, tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug)

        mp.setattr(rs, "write_trans_file", capture)
        for kw in with_files:
            rs.sos_proc(**kw)
        assert len(seen) == len(NAMES)
        for s in seen:
            s["text"] = open(s["path"]).read()
        mp.setattr(rs, "write_trans_file", write)
        kws = spectrum_keywords(rs, work / "spectrum")
        assert any(int(kw["imode_ckd_calcul"]) == 2 for kw in kws) and any(int(kw["iprofil"]) == 2 for kw in kws)
        assert any(int(kw["absprofil"]) == 7 and int(kw["iprofil"]) == 1 for kw in kws)
        plain = rs.sos_spectrum(kws)
        return dict(seen=seen, kws=kws, plain=plain)
    finally:
        mp.undo()


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")


def _check_against_sequential(trans, seen, rs):
    assert len(trans) == len(seen)
    for t, s in zip(trans, seen):
        assert set(t) == set(KEYS)
        # the aggregated values, bit for bit
        assert t["ttot_tronc"] == s["ttot_tronc"] and t["ttot_vrai"] == s["ttot_vrai"] and t["tdifmus"] == s["tdifmus"]
        assert np.array_equal(t["tdifmug"], s["tdifmug"]) and t["tdifmug"].shape == s["mu"].shape
        assert t["thetas"] == s["tetas"] and np.array_equal(t["thetav"], [math.degrees(math.acos(m)) for m in s["mu"]])
        # the printed quantities: the statements of the file writer ...
        cs = math.cos(math.pi * s["tetas"] / 180.0)
        assert t["t_dir_down"] == math.exp(-s["ttot_vrai"] / cs)
        assert t["t_dif_down"] == s["tdifmus"] + math.exp(-s["ttot_tronc"] / cs) - math.exp(-s["ttot_vrai"] / cs)
        up = [s["tdifmug"][j] + math.exp(-s["ttot_tronc"] / m) - math.exp(-s["ttot_vrai"] / m) for j, m in enumerate(s["mu"])]
        assert np.array_equal(t["t_dif_up"], up)
        direct, down, ups = rs.trans_quantities(s["tetas"], s["mu"], s["ttot_tronc"], s["ttot_vrai"], s["tdifmus"], s["tdifmug"])
        assert (direct, down) == (t["t_dir_down"], t["t_dif_down"]) and np.array_equal(ups, t["t_dif_up"])
        # ... and, rounded to four decimals, the numbers of the file the sequential call wrote
        text = s["text"]
        assert re.search(r"Direct transmission TOA -> surface : +(\S+)", text).group(1) == ("%8.4f" % t["t_dir_down"]).strip()
        assert re.search(r"td\(thetas\) = +(\S+)", text).group(1) == ("%7.4f" % t["t_dif_down"]).strip()
        assert re.findall(r"td\(thetav\) = +(\S+)", text) == [("%7.4f" % v).strip() for v in t["t_dif_up"]]
        assert 0.0 < t["t_dif_down"] < 1.0 and np.all(t["t_dif_up"] > 0.0) and np.all(t["t_dif_up"] < 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 4])
@pytest.mark.parametrize("chunk", [2, 3, 256])
def test_trans_equals_sequential_calls_bitwise(gpu_pkg, reference, env, chunk, parts):
    rs = gpu_pkg.run_sos
    tuples, trans = rs.sos_spectrum(reference["kws"], chunk=chunk, parts=parts, transmissions=True)
    _check_against_sequential(trans, reference["seen"], rs)
    assert len(tuples) == len(reference["plain"])
    for a, b in zip(tuples, reference["plain"]):
        assert_tuples_equal(a, b)


@pytest.mark.gpu
def test_levels_return_the_same_trans_behind_spec_and_flux(gpu_pkg, reference, env):
    rs = gpu_pkg.run_sos
    kws, alts = reference["kws"], [-1, 2.0]
    spec0, flux0 = rs.sos_spectrum_levels(alts, kws, fluxes=True)
    spec, flux, trans = rs.sos_spectrum_levels(alts, kws, fluxes=True, transmissions=True)
    _check_against_sequential(trans, reference["seen"], rs)
    assert len(spec) == len(spec0) == len(kws)
    for a, b, fa, fb in zip(spec, spec0, flux, flux0):
        assert np.array_equal(fa, fb)
        for k in range(len(alts)):
            assert_tuples_equal(a[k], b[k])
    spec1, trans1 = rs.sos_spectrum_levels(alts, kws[:3], transmissions=True)
    assert len(spec1) == 3
    for a, b in zip(trans1, trans[:3]):
        same_entry(a, b)


@pytest.mark.gpu
def test_one_call_per_chunk_and_direction_count(gpu_pkg, reference, env, monkeypatch):
    """parts=1: solver.diffuse_transmissions_many once per chunk and group of equal N, no per-direction loop, and one context
    per wavelength (the loop would make N more for each)."""
    rs, S = gpu_pkg.run_sos, gpu_pkg.solver
    kws = reference["kws"]
    n_of = [int(t[0]) for t in reference["plain"]]
    seen = dict(many=[], loop=0, contexts=0)
    many0, init0 = S.diffuse_transmissions_many, S.SosContext.__init__

    def many(ctxs, bins, ctx_of_bin=None):
        ctxs = list(ctxs)
        seen["many"].append((ctxs[0].n, len(ctxs), int(bins["nb"])))
        assert len({cx.n for cx in ctxs}) == 1
        return many0(ctxs, bins, ctx_of_bin)

    def loop(self, bins):
        seen["loop"] += 1
        raise AssertionError("the per-direction loop must not run")

    def init(self, *a, **k):
        seen["contexts"] += 1
        return init0(self, *a, **k)

    monkeypatch.setattr(S, "diffuse_transmissions_many", many)
    monkeypatch.setattr(S.SosContext, "diffuse_transmissions", loop)
    monkeypatch.setattr(S.SosContext, "__init__", init)
    for chunk in (256, 3):
        seen.update(many=[], loop=0, contexts=0)
        rs.sos_spectrum(kws, chunk=chunk, parts=1, transmissions=True)
        chunks = [n_of[c:c + chunk] for c in range(0, len(kws), chunk)]
        assert len(seen["many"]) == sum(len(set(c)) for c in chunks), seen
        assert sorted(m[0] for m in seen["many"]) == sorted(n for c in chunks for n in set(c))
        assert sum(m[1] for m in seen["many"]) == len(kws)
        assert (seen["loop"], seen["contexts"]) == (0, len(kws)), seen
    # without the keyword: not called at all
    seen.update(many=[])
    rs.sos_spectrum(kws[:3], parts=1)
    assert seen["many"] == []


def test_a_call_with_the_trans_file_is_refused_before_any_library_call(pkg, tmp_path, monkeypatch):
    rs = pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws = spectrum_keywords(rs, tmp_path)[:3]

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(pkg.capi, "lib", no_library)
    bad = [kws[0], dict(kws[1], fictrans="SOS_Transm.txt"), kws[2]]
    for call in (lambda **k: rs.sos_spectrum(bad, **k), lambda **k: rs.sos_spectrum_levels([-1, 2.0], bad, **k)):
        with pytest.raises(ValueError, match="call 1 .*-SOS.Trans"):
            call(transmissions=True)
        with pytest.raises(ValueError, match="transmissions must be True or False"):
            call(transmissions=1)
    assert rs.sos_spectrum([], transmissions=True) == ([], [])
