"""The surface matrices of a spectrum whose surface changes with the wavelength, queued once per chunk of the pass
(run_sos._prefetch_surfaces -> surface.surface_matrices_many): sos_spectrum / sos_spectrum_levels against sequential
sos_proc / sos_proc_levels bit for bit, the call counts of the batch and of the per-call entry points, and a failing call."""
import pytest

import spectrum_cases
from spectrum_cases import assert_tuples_equal
from test_surface_matrix import NEGATIVE_TRIPLE, TRIPLES


def _calls(rs, workdir):
    """Ten calls on the angle and aerosol settings of three fast goldens: land_roujean (12 Gauss angles, molecules only),
    cfg5_roujean_maignan (16 / 20 angles, aerosols from the reference's Aerosols.txt: all os_nb + 1 orders) and glitter_polar
    (16 / 20 angles, the same sun: its sea calls share an angle set with the aerosol land call).  Six land calls of types 3
    and 7 with a triple each, four sea calls over two winds with an index each."""
    kws, _, _, _ = spectrum_cases.build(rs, workdir, names=["land_roujean", "cfg5_roujean_maignan", "glitter_polar"])
    lnd, aer, sea = kws

    def roujean(kw, t, **more):
        return dict(kw, k0_roujean=t[0], k1_roujean=t[1], k2_roujean=t[2], **more)

    maignan = dict(isurf=7, surf_ind=1.5, coef_c_maignan=4.0)
    calls = [roujean(lnd, TRIPLES[0]),
             dict(sea, wind=7.0, surf_ind=1.343),
             roujean(lnd, TRIPLES[2], **maignan),
             dict(sea, wind=2.0, surf_ind=1.337),
             roujean(aer, (0.22, 0.03, 0.25)),
             roujean(lnd, TRIPLES[1]),
             dict(sea, wind=7.0, surf_ind=1.331),
             roujean(lnd, TRIPLES[3], **maignan),
             dict(sea, wind=2.0, surf_ind=1.325),
             roujean(lnd, (0.2, 0.03, 0.25))]
    assert [int(kw["isurf"]) for kw in calls] == [3, 1, 7, 1, 7, 3, 1, 7, 1, 3] and float(aer["aot_ref"]) > 0.0
    return calls


def _groups(chunk):
    return len({(kw["nbmu_gauss_lum"], kw["nbmu_gauss_mie"], kw["tetas"]) for kw in chunk})


def _count(monkeypatch, pkg):
    n = dict(many=0, glitter=0, land=0, jobs=[])
    S = pkg.surface
    m0, g0, l0 = S.surface_matrices_many, S.glitter_matrices, S.land_matrices

    def many(jobs, *a, **k):
        n["many"] += 1
        n["jobs"].append(len(jobs))
        return m0(jobs, *a, **k)

    def glitter(*a, **k):
        n["glitter"] += 1
        return g0(*a, **k)

    def land(*a, **k):
        n["land"] += 1
        return l0(*a, **k)

    monkeypatch.setattr(S, "surface_matrices_many", many)
    monkeypatch.setattr(S, "glitter_matrices", glitter)
    monkeypatch.setattr(S, "land_matrices", land)
    return n


@pytest.fixture(scope="module")
def sequential(gpu_pkg, tmp_path_factory):
    """The calls and their sequential sos_proc results, computed once for the module."""
    rs = gpu_pkg.run_sos
    calls = _calls(rs, tmp_path_factory.mktemp("surface_spectrum"))
    rs._SURF_CACHE.clear()
    return calls, [rs.sos_proc(**kw) for kw in calls]


@pytest.mark.gpu
def test_spectrum_equals_sequential_calls_and_batches_once_per_chunk(gpu_pkg, sequential, monkeypatch):
    """chunk=5 and two parts per chunk: the default path asks surface_matrices_many once per (chunk, angle set) and the
    per-call entry points never; SOS_SPECTRUM_SURFACE_PER_CALL=1 does the opposite; both give sos_proc's 23 outputs."""
    rs = gpu_pkg.run_sos
    calls, seq = sequential
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    monkeypatch.delenv("SOS_SPECTRUM_SURFACE_PER_CALL", raising=False)
    n = _count(monkeypatch, gpu_pkg)
    rs._SURF_CACHE.clear()
    out = rs.sos_spectrum(calls, chunk=5, parts=2)
    for a, b in zip(seq, out):
        assert_tuples_equal(a, b)
    assert n["many"] == _groups(calls[:5]) + _groups(calls[5:]) == 4 and sum(n["jobs"]) == len(calls), n
    assert (n["glitter"], n["land"]) == (0, 0), n
    n.update(many=0, jobs=[])
    rs._SURF_CACHE.clear()
    monkeypatch.setenv("SOS_SPECTRUM_SURFACE_PER_CALL", "1")
    out = rs.sos_spectrum(calls, chunk=5, parts=2)
    for a, b in zip(seq, out):
        assert_tuples_equal(a, b)
    assert n["many"] == 0 and (n["glitter"], n["land"]) == (4, 6), n


@pytest.mark.gpu
def test_spectrum_levels_equals_sequential_level_calls(gpu_pkg, sequential, monkeypatch):
    rs = gpu_pkg.run_sos
    calls, _ = sequential
    alts = [-1, 2.0]
    kws = [dict(kw, zout=-1.0) for kw in calls]
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    monkeypatch.delenv("SOS_SPECTRUM_SURFACE_PER_CALL", raising=False)
    rs._SURF_CACHE.clear()
    ref = [rs.sos_proc_levels(alts, **kw) for kw in kws]
    n = _count(monkeypatch, gpu_pkg)
    rs._SURF_CACHE.clear()
    lev = rs.sos_spectrum_levels(alts, kws, chunk=10, parts=2)       # chunk // K = 5 calls per chunk, as above
    assert n["many"] == _groups(kws[:5]) + _groups(kws[5:]) == 4 and (n["glitter"], n["land"]) == (0, 0), n
    for i in range(len(kws)):
        for k in range(len(alts)):
            assert_tuples_equal(ref[i][k], lev[i][k])


@pytest.mark.gpu
def test_keys_of_the_prefetch_are_the_keys_of_prepare(gpu_pkg, sequential, monkeypatch):
    """Every key _prepare hands to _surface_cached is one the request function formed for the chunk."""
    rs = gpu_pkg.run_sos
    calls, _ = sequential
    monkeypatch.delenv("SOS_SPECTRUM_SURFACE_PER_CALL", raising=False)
    asked, c0 = [], rs._surface_cached

    def cached(key, make, device):
        asked.append(key)
        return c0(key, make, device)

    monkeypatch.setattr(rs, "_surface_cached", cached)
    rs._SURF_CACHE.clear()
    rs.sos_spectrum(calls[:5])
    formed = [k for g in rs._surface_requests([rs._validated(kw) for kw in calls[:5]], device=0) for k in g["keys"]]
    assert len(asked) == 5 and sorted(map(repr, asked)) == sorted(map(repr, formed))


@pytest.mark.gpu
def test_gas_requests_of_the_prefetch_are_the_calls_of_prepare(gpu_pkg, tmp_path, monkeypatch):
    """Five gas calls in one chunk: the argument tuples _prepare hands to prepa_absprofile are the requests the prefetch formed."""
    rs, A = gpu_pkg.run_sos, gpu_pkg.absorption
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    kw = spectrum_cases.build(rs, tmp_path, names=["ckd_o2a_5bins"])[0][0]
    calls = [dict(kw, psurf=ps) for ps in (1013.0, 1005.0, 995.0, 985.0, 975.0)]
    asked, formed, p0, f0 = [], [], A.prepa_absprofile, A.prefetch_gas_tables

    def prepa(*a, **k):
        if not k:                                        # (the prefetch itself calls it with root=...)
            asked.append(a)
        return p0(*a, **k)

    def prefetch(requests, device_tables=()):
        formed.extend(requests)
        return f0(requests, device_tables=device_tables)

    monkeypatch.setattr(A, "prepa_absprofile", prepa)
    monkeypatch.setattr(A, "prefetch_gas_tables", prefetch)
    out = rs.sos_spectrum(calls, chunk=5, parts=2)
    assert len(out) == 5 and len(formed) == 5 and len(set(formed)) == 5
    assert list(map(repr, asked)) == list(map(repr, formed))


@pytest.mark.gpu
def test_aerosol_runs_of_the_prefetch_leave_none_to_prepare(gpu_pkg, monkeypatch):
    """Five model-aerosol calls away from -AER.Waref in one chunk: the prefetch forms the simulation-wavelength run of every one
    (aerosols_many), so _prepare makes none of its own."""
    from test_mie_batch import _kw, _wmo_user
    rs, A = gpu_pkg.run_sos, gpu_pkg.aerosols
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    calls = [_kw(rs, _wmo_user(wa, 2)) for wa in (0.49, 0.56, 0.67, 0.78, 0.865)]
    n = dict(inside=False, own=0, many=0, made=0)
    a0, m0, p0 = A.aerosols, A.aerosols_many, rs._prepare

    def aerosols(p, wa, ta, *a, at_waref=False, **k):
        n["own"] += n["inside"] and not at_waref
        return a0(p, wa, ta, *a, at_waref=at_waref, **k)

    def many(jobs, *a, **k):
        res = m0(jobs, *a, **k)
        n["many"] += len(jobs)
        n["made"] += sum(r is not None for r in res)
        return res

    def prepare(*a, **k):
        n["inside"] = True
        try:
            return p0(*a, **k)
        finally:
            n["inside"] = False

    monkeypatch.setattr(A, "aerosols", aerosols)
    monkeypatch.setattr(A, "aerosols_many", many)
    monkeypatch.setattr(rs, "_prepare", prepare)
    out = rs.sos_spectrum(calls, chunk=5, parts=2)
    assert len(out) == 5 and (n["many"], n["made"], n["own"]) == (5, 5, 0), n


@pytest.mark.gpu
def test_flagged_call_raises_what_sos_proc_raises(gpu_pkg, sequential, monkeypatch):
    rs = gpu_pkg.run_sos
    calls, seq = sequential
    monkeypatch.delenv("SOS_SPECTRUM_SURFACE_PER_CALL", raising=False)
    t = NEGATIVE_TRIPLE
    bad = dict(calls[0], k0_roujean=t[0], k1_roujean=t[1], k2_roujean=t[2])
    rs._SURF_CACHE.clear()
    with pytest.raises(rs.SosProcError) as alone:
        rs.sos_proc(**bad)
    assert alone.value.ier == -1
    n = _count(monkeypatch, gpu_pkg)
    with pytest.raises(rs.SosProcError) as inlist:
        rs.sos_spectrum(calls[:3] + [bad] + calls[3:5])
    assert n["many"] >= 1 and (n["glitter"], n["land"]) == (0, 0), n
    assert type(inlist.value) is type(alone.value) and str(inlist.value) == str(alone.value)
    assert inlist.value.ier == alone.value.ier
    rs._SURF_CACHE.clear()
    for a, b in zip(seq[:5], rs.sos_spectrum(calls[:5])):
        assert_tuples_equal(a, b)
