"""spherical_albedo=True of run_sos.sos_spectrum / sos_spectrum_levels: the key s_alb of the transmission entries, the band
value sum aik * S_b of the spherical albedo of the atmosphere seen from the ground (solver.spherical_albedo_many +
solver.albedo_band per part and direction count).  The golden CKD fixtures through spectrum_cases.build, the calls of
test_spectrum_transmissions."""
import numpy as np
import pytest

import spectrum_cases
import test_albedo_many
import test_spectrum_transmissions as TT

GOLD = spectrum_cases.GOLD
KEYS = TT.KEYS
ALTS = [-1, 2.0]


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")


@pytest.fixture(scope="module")
def reference(gpu_pkg, tmp_path_factory):
    """The calls, their pass with transmissions=True alone and the pass with spherical_albedo=True.  Computed once, read only."""
    rs = gpu_pkg.run_sos
    mp = pytest.MonkeyPatch()
    mp.setenv("SOS_ABS_ROOT", GOLD)
    mp.setenv("SOS_SPECTRUM_MIN_PART", "2")
    try:
        kws = TT.spectrum_keywords(rs, tmp_path_factory.mktemp("albedo_ref"))
        tuples0, trans0 = rs.sos_spectrum(kws, transmissions=True)
        tuples, trans = rs.sos_spectrum(kws, transmissions=True, spherical_albedo=True)
        return dict(kws=kws, tuples0=tuples0, trans0=trans0, tuples=tuples, trans=trans)
    finally:
        mp.undo()


def test_keyword_rules_are_checked_before_any_library_call(pkg, tmp_path, monkeypatch):
    rs = pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws = TT.spectrum_keywords(rs, tmp_path)[:3]

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(pkg.capi, "lib", no_library)
    for call in (lambda **k: rs.sos_spectrum(kws, **k), lambda **k: rs.sos_spectrum_levels(ALTS, kws, **k)):
        with pytest.raises(ValueError, match="spherical_albedo=True requires transmissions=True"):
            call(spherical_albedo=True)
        with pytest.raises(ValueError, match="spherical_albedo=True requires transmissions=True"):
            call(spherical_albedo=True, transmissions=False)
        for bad in (1, "yes", None):
            with pytest.raises(ValueError, match="spherical_albedo must be True or False"):
                call(spherical_albedo=bad, transmissions=True)
    assert rs.sos_spectrum([], transmissions=True, spherical_albedo=True) == ([], [])


@pytest.mark.gpu
def test_one_more_key_and_every_other_bit_unchanged(gpu_pkg, reference):
    assert len(reference["trans"]) == len(reference["trans0"]) == len(reference["kws"])
    for t0, t in zip(reference["trans0"], reference["trans"]):
        assert set(t0) == set(KEYS)                                     # without the keyword: exactly the keys there were
        assert set(t) == set(KEYS) | {"s_alb"}
        TT.same_entry(t0, {k: t[k] for k in KEYS})
        assert isinstance(t["s_alb"], float) and 0.0 < t["s_alb"] < 1.0
    for a, b in zip(reference["tuples"], reference["tuples0"]):
        spectrum_cases.assert_tuples_equal(a, b)


@pytest.mark.gpu
def test_band_value_is_the_weighted_sum_of_the_bins(gpu_pkg, reference, env):
    """Every call prepared on its own: s_alb against sum aik * S_b of a separate spherical_albedo_many call on that call's bins
    -- bit for bit for a single bin (aik * S exactly), at 1e-12 relative for a band (ckd_o2a_5bins, the 25-bin band: positive
    terms, the tree only reassociates them)."""
    import torch
    rs, solver = gpu_pkg.run_sos, gpu_pkg.solver
    counts = []
    for kw, t in zip(reference["kws"], reference["trans"]):
        pl = rs._prepare(kw, None, 0, shard_bins=False)
        try:
            salb, _ = solver.spherical_albedo_many([pl.ctx], pl.bins)
            torch.cuda.synchronize()
            salb, aik = salb.cpu().numpy(), np.asarray(pl.aik, dtype=np.float64)
            assert len(salb) == len(aik) == pl.bins["nb"]
            s = 0.0
            for b in range(len(aik)):
                s = s + aik[b] * salb[b]
            if len(aik) == 1:
                assert t["s_alb"] == s and aik[0] == 1.0 and t["s_alb"] == salb[0]
            else:
                assert abs(t["s_alb"] - s) <= 1e-12 * s
            counts.append(len(aik))
        finally:
            pl.ctx.close()
    assert 1 in counts and 5 in counts


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,parts", [(2, 1), (3, 4)])
def test_chunks_and_parts_do_not_change_the_value(gpu_pkg, reference, env, chunk, parts):
    rs = gpu_pkg.run_sos
    _, trans = rs.sos_spectrum(reference["kws"], chunk=chunk, parts=parts, transmissions=True, spherical_albedo=True)
    assert [t["s_alb"] for t in trans] == [t["s_alb"] for t in reference["trans"]]


@pytest.mark.gpu
def test_levels_give_the_same_values(gpu_pkg, reference, env):
    rs = gpu_pkg.run_sos
    kws = reference["kws"]
    spec, trans = rs.sos_spectrum_levels(ALTS, kws, transmissions=True, spherical_albedo=True)
    assert len(spec) == len(kws)
    for a, b in zip(trans, reference["trans"]):
        assert set(a) == set(b) and a["s_alb"] == b["s_alb"]
        TT.same_entry({k: a[k] for k in KEYS}, {k: b[k] for k in KEYS})


@pytest.mark.gpu
def test_one_call_per_chunk_and_direction_count(gpu_pkg, reference, env, monkeypatch):
    """parts=1: solver.spherical_albedo_many once per chunk and group of equal N, seen from the ground; never without the
    keyword."""
    rs, solver = gpu_pkg.run_sos, gpu_pkg.solver
    kws = reference["kws"]
    n_of = [int(t[0]) for t in reference["tuples0"]]
    seen = []
    many0 = solver.spherical_albedo_many

    def many(ctxs, bins, ctx_of_bin=None, from_below=True):
        ctxs = list(ctxs)
        seen.append((ctxs[0].n, len(ctxs), bool(from_below)))
        return many0(ctxs, bins, ctx_of_bin, from_below)

    monkeypatch.setattr(solver, "spherical_albedo_many", many)
    rs.sos_spectrum(kws, chunk=3, parts=1, transmissions=True, spherical_albedo=True)
    chunks = [n_of[c:c + 3] for c in range(0, len(kws), 3)]
    assert len(seen) == sum(len(set(c)) for c in chunks), seen
    assert sum(m[1] for m in seen) == len(kws) and all(m[2] for m in seen)
    del seen[:]
    rs.sos_spectrum(kws[:3], parts=1, transmissions=True)
    assert seen == []


@pytest.mark.gpu
def test_ground_flux_obeys_the_coupling_formula(gpu_pkg, env, tmp_path):
    """The physics, end to end: the no-gas Lambert call cfg1_lambert (one bin) at ground albedo 0, 0.1 and 0.5, three calls of
    one spectrum.  The total down-going flux at the ground (element 20 of the tuples) obeys E(a) (1 - a s_alb) = E(0) within
    the bound measured for the oracle in test_albedo_many (1.26e-7); measured on the MI355X: 1.8e-9 at a = 0.1, 8.0e-8 at a = 0.5 (s_alb = 0.080707)."""
    rs = gpu_pkg.run_sos
    kw = spectrum_cases.build(rs, tmp_path, names=["cfg1_lambert"])[0][0]
    kw = dict(kw, fictrans="NO_OUTPUT", zout=-1.0)
    assert int(kw["isurf"]) == 0 and int(kw["absprofil"]) == 7
    albedos = (0.0, 0.1, 0.5)
    tuples, trans = rs.sos_spectrum([dict(kw, rho=a) for a in albedos], transmissions=True, spherical_albedo=True)
    s = trans[0]["s_alb"]
    assert s == trans[1]["s_alb"] == trans[2]["s_alb"]                  # the ground plays no part in it
    e = [float(t[20]) for t in tuples]
    for a, ea in zip(albedos[1:], e[1:]):
        miss = abs(ea * (1.0 - a * s) / e[0] - 1.0)
        print("a = %.1f: E(a) %.12f E(0) %.12f s_alb %.12f identity %.3e" % (a, ea, e[0], s, miss))
        assert ea > e[0]
        assert miss <= test_albedo_many.IDENTITY_BOUND
