"""sosgpu_mie_batch (csrc/mie.hip k_mie_batch): the Mie records of many refractive indices as one pool of (job, size parameter)
items, queued without a host wait -- and the host path built on it (aerosols.prefetch_mie_records, the byte-budgeted record
cache, the spectrum prefetch).

The batch runs the device function sosgpu_mie runs per size parameter, so every comparison with sosgpu_mie is `torch.equal`
/ `np.array_equal`: no tolerance anywhere in the bit-identity tests.  The oracle comparison uses the rule and the helpers of
tests/test_mie_granu.py unchanged.  Size-parameter lists are hand-made and sit on the edges of the batch's own structure: the
four LDS classes (alpha <= 64 | 200 | 420 | 850), the scratch form beyond, more scratch items than resident slots, job counts
either side of 32 and 64."""
import ctypes as C
import functools
import importlib
import math
import os

import numpy as np
import pytest

import test_mie_granu as T               # xmu_of, record_report, run_mie, the constants: the existing sweep's own helpers

GOLD = T.GOLD
A = importlib.import_module("radiativetransfer-sos_amd.aerosols")
E_ARG, E_NODEVICE, E_UNSUPPORTED = -1, -2, -3
NBMU = 12                                # A.mie_angles(12): W = 25
CLASS_LIMITS = [64.0, 200.0, 420.0, 850.0]

INDICES = [(1.53, -0.008), (1.381, 0.0), (1.75, -0.44), (1.05, -1e-6)]
LISTS = dict(
    one=np.array([1e-4]),
    ramp300=np.linspace(0.1, 60.0, 300),
    lds_limit=np.array([849.0, 850.0, T.ABOVE, 851.0, 900.0]),
    onsets=np.array([745.5, 746.5, 768.5, 769.0, 770.0]),                   # first rescale / first break of the recurrences, LDS form
    onsets_scr=np.array([851.0, 851.5, 852.0, 875.5, 899.5, 900.0]),        # ... past them, scratch form (both branches taken)
    last=np.array([T.ALPHA_LAST]),
    classes=np.array([v for k in CLASS_LIMITS for v in (T.before(k), k, float(np.nextafter(k, np.inf)))]),
    more_than_slots=T.stride_alphas(T.SLOTS + 1),
)
# the pool a call of `count` jobs cycles through: every list, the indices rotating
POOL = [(INDICES[i % 4], name) for i, name in enumerate(["ramp300", "lds_limit", "one", "onsets", "last", "classes", "onsets_scr",
                                                         "more_than_slots", "lds_limit", "ramp300", "onsets"])]


def jobs_of(count):
    return [POOL[k % len(POOL)] for k in range(count)]


@functools.lru_cache(maxsize=None)
def direct(nbmu, idx, name):
    """sosgpu_mie for one job, once per session: (rec, g) device tensors."""
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rc, rec, g = T.run_mie(pkg, nbmu, idx[0], idx[1], LISTS[name], fill=float("nan"))
    assert rc == 0, rc
    return rec, g


def run_batch(pkg, nbmu, jobs, short=0, mutate=None, count=None):
    """sosgpu_mie_batch through capi; jobs: [((rn, in), alphas array)].  All records go into ONE NaN-filled float32 allocation
    with a spare row behind each job's records, all g into one float64 allocation with a spare element behind each job's.
    Returns (rc, [rec views], [g views], spare rows, spare g, status) as device tensors; status is pre-filled with -77."""
    import torch
    xmu = np.ascontiguousarray(T.xmu_of(nbmu), dtype=np.float64)
    rs = 4 + 3 * len(xmu)
    dev = torch.device("cuda", 0)
    lists = [np.ascontiguousarray(al, dtype=np.float64) for _, al in jobs]
    rows = sum(len(al) + 1 for al in lists)
    rec = torch.full((max(rows, 1), rs), float("nan"), dtype=torch.float32, device=dev)
    g = torch.full((max(rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((max(len(jobs), 1),), -77, dtype=torch.int32, device=dev)
    cj = (pkg.capi.MieJob * max(len(jobs), 1))()
    views, r0 = [], 0
    for k, ((rn, in_), _) in enumerate(jobs):
        al = lists[k]
        cj[k] = pkg.capi.MieJob(rn, in_, al.ctypes.data, len(al), 0, rec[r0].data_ptr(), g[r0:].data_ptr())
        views.append((r0, len(al)))
        r0 += len(al) + 1
    if mutate:
        mutate(cj)
    L = pkg.capi.lib()
    n = len(jobs) if count is None else count
    nbytes = L.sosgpu_mie_batch_work_bytes(nbmu, n, cj)
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = L.sosgpu_mie_batch(0, nbmu, xmu.ctypes.data_as(C.c_void_p), n, cj, C.c_void_p(work.data_ptr()), max(nbytes - short, 0),
                            C.c_void_p(status.data_ptr()), st)
    torch.cuda.synchronize()
    recs = [rec[a:a + m] for a, m in views]
    gs = [g[a:a + m] for a, m in views]
    spare = torch.stack([rec[a + m] for a, m in views]) if views else rec[:0]
    spare_g = torch.stack([g[a + m] for a, m in views]) if views else g[:0]
    return rc, recs, gs, spare, spare_g, status, nbytes


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the structure and the order of validation
# ---------------------------------------------------------------------------------------------------------------------
def test_mie_job_layout_and_validation_before_device_work(pkg):
    """sosgpu_mie_job is 2 doubles, a pointer, 2 int32, 2 pointers = 48 bytes; a malformed job is SOSGPU_E_ARG on a machine
    without a device too (validation comes first), and count = 0 is SOSGPU_OK."""
    cap = pkg.capi
    assert C.sizeof(cap.MieJob) == 2 * 8 + 8 + 2 * 4 + 2 * 8 == 48
    assert [f[0] for f in cap.MieJob._fields_] == ["rn", "in_", "alphas", "nalpha", "reserved", "d_rec", "d_g"]
    L = cap.lib()
    xmu = np.ascontiguousarray(T.xmu_of(NBMU))
    al = np.array([1.0, 2.0])
    bad = (cap.MieJob * 2)()
    bad[0] = cap.MieJob(1.5, -0.01, al.ctypes.data, 2, 0, 8, 8)            # (never dereferenced: refused before any device work)
    bad[1] = cap.MieJob(1.5, -0.01, al.ctypes.data, 0, 0, 8, 8)            # nalpha = 0
    rc = L.sosgpu_mie_batch(0, NBMU, xmu.ctypes.data_as(C.c_void_p), 2, bad, C.c_void_p(8), 1 << 20, C.c_void_p(8), None)
    assert rc == E_ARG, rc
    assert L.sosgpu_mie_batch_work_bytes(NBMU, 2, bad) == 0
    assert L.sosgpu_mie_batch(0, NBMU, xmu.ctypes.data_as(C.c_void_p), 0, bad, None, 0, None, None) == 0
    desc = np.array([2.0, 1.0])
    bad[1] = cap.MieJob(1.5, -0.01, desc.ctypes.data, 2, 0, 8, 8)
    assert L.sosgpu_mie_batch(0, NBMU, xmu.ctypes.data_as(C.c_void_p), 2, bad, C.c_void_p(8), 1 << 20, C.c_void_p(8), None) == E_ARG
    # the work area of a good pair: angle set + ONE copy of the shared list + table (64 bytes a job) + item offsets, no scratch
    bad[1] = cap.MieJob(1.4, 0.0, al.ctypes.data, 2, 0, 8, 8)
    assert L.sosgpu_mie_batch_work_bytes(NBMU, 2, bad) == (25 + 2) * 8 + 2 * 64 + 5 * 3 * 4 + 4
    sc = np.array([900.0, 1000.0])
    bad[1] = cap.MieJob(1.4, 0.0, sc.ctypes.data, 2, 0, 8, 8)             # two scratch items: 2 slots of 11 (2 * 1000 + 24) doubles
    assert L.sosgpu_mie_batch_work_bytes(NBMU, 2, bad) == (25 + 4) * 8 + 2 * 64 + 64 + 2 * 11 * 2024 * 8


def test_lists_cover_the_batch_structure():
    """The hand-made lists sit where the batch takes another path (plain arithmetic on the tables above)."""
    cls = lambda a: int(np.searchsorted(CLASS_LIMITS, a, side="left"))          # first class whose limit is >= alpha; 4 = scratch
    assert [cls(a) for a in LISTS["classes"]] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4]
    assert [cls(a) for a in LISTS["lds_limit"]] == [3, 3, 4, 4, 4]
    assert len(LISTS["more_than_slots"]) > T.SLOTS and cls(LISTS["more_than_slots"][0]) == 4
    assert 2 * LISTS["last"][0] + 24 == 10000
    assert {i for i, _ in POOL} == set(INDICES) and {n for _, n in POOL} == set(LISTS)
    assert all(np.all(np.diff(v) >= 0) and v[0] > 0 for v in LISTS.values())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the batch equals sosgpu_mie bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _assert_equals_direct(nbmu, jobs, out):
    import torch
    rc, recs, gs, spare, spare_g, status, _ = out
    assert rc == 0, rc
    assert bool((status[:len(jobs)] == 0).all()), status
    assert bool(torch.isnan(spare).all()) and bool(torch.isnan(spare_g).all()), "a spare row behind a job's records was written"
    for k, (idx, name) in enumerate(jobs):
        rec, g = direct(nbmu, idx, name)
        assert torch.equal(recs[k], rec), (k, idx, name, "rec")
        assert torch.equal(gs[k], g), (k, idx, name, "g")
        assert not bool(torch.isnan(rec).any())


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 32, 33, 65])
def test_batch_equals_sosgpu_mie_bit_for_bit(gpu_pkg, count):
    jobs = jobs_of(count)
    out = run_batch(gpu_pkg, NBMU, [(idx, LISTS[name]) for idx, name in jobs])
    _assert_equals_direct(NBMU, jobs, out)


@pytest.mark.gpu
def test_batch_equals_sosgpu_mie_at_129_angles(gpu_pkg):
    jobs = jobs_of(len(POOL))
    out = run_batch(gpu_pkg, 64, [(idx, LISTS[name]) for idx, name in jobs])
    _assert_equals_direct(64, jobs, out)


@pytest.mark.gpu
def test_shared_list_pointer_is_uploaded_once_and_read_by_both_jobs(gpu_pkg):
    """Two jobs that pass the same host list (the cached alpha_grid of two indices) share one uploaded copy."""
    import torch
    al = np.ascontiguousarray(LISTS["ramp300"])                               # (no scratch item: the sizes differ by the table only)
    rc, recs, gs, spare, spare_g, status, nbytes = run_batch(gpu_pkg, NBMU, [(INDICES[0], al), (INDICES[2], al)])
    one = run_batch(gpu_pkg, NBMU, [(INDICES[0], al)])[6]
    assert rc == 0 and nbytes - one == 64 + 5 * 4 + 4                         # a table entry and a column of item offsets, no list
    for k, idx in enumerate((INDICES[0], INDICES[2])):
        rec, g = direct(NBMU, idx, "ramp300")
        assert torch.equal(recs[k], rec) and torch.equal(gs[k], g)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
ORACLE_JOBS = [((1.381, 0.0), "lds_limit"), ((1.53, -0.008), "onsets"), ((1.75, -0.44), "onsets_scr"), ((1.05, -1e-6), "classes"),
               ((1.381, 0.0), "last"), ((1.53, -0.008), "ramp300")]


@pytest.mark.gpu
def test_batch_records_vs_the_oracle(gpu_pkg, oracle):
    """Both forms, `in` = 0 and alpha = 4988 against sos_oracle_mie under record_report of tests/test_mie_granu.py (REAL*4 entries
    within its bar, g to 1e-13, the capped Q/U exception).  Measured on the MI355X: see the printed lines."""
    out = run_batch(gpu_pkg, NBMU, [(idx, LISTS[name]) for idx, name in ORACLE_JOBS])
    assert out[0] == 0
    for k, (idx, name) in enumerate(ORACLE_JOBS):
        ref = oracle.mie(T.xmu_of(NBMU), idx[0], idx[1], LISTS[name])
        fails, lines = T.record_report(out[1][k].cpu().numpy(), out[2][k].cpu().numpy(), ref)
        print("mie_batch %s %s: %s" % (idx, name, "; ".join(lines)))
        assert not fails, (idx, name, fails)


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals: nothing launched, nothing touched
# ---------------------------------------------------------------------------------------------------------------------
def _set(k, **kw):
    def f(cj):
        for name, v in kw.items():
            setattr(cj[k], name, v)
    return f


_DESC = np.array([3.0, 2.0, 4.0])
_OVER = np.array([10.0, T.ALPHA_OVER])
_NEG = np.array([-1.0, 2.0])
REFUSED = {
    "null-rec": (_set(1, d_rec=None), E_ARG),
    "null-g": (_set(1, d_g=None), E_ARG),
    "null-list": (_set(1, alphas=None), E_ARG),
    "nalpha-0": (_set(1, nalpha=0), E_ARG),
    "descending": (_set(1, alphas=_DESC.ctypes.data, nalpha=3), E_ARG),
    "not-positive": (_set(1, alphas=_NEG.ctypes.data, nalpha=2), E_ARG),
    "alpha-4989": (_set(1, alphas=_OVER.ctypes.data, nalpha=2), E_UNSUPPORTED),
}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(REFUSED))
def test_batch_refuses_on_the_host(gpu_pkg, cid):
    """A bad job between two good ones: the stated code, every output still NaN, d_status still its fill."""
    import torch
    mutate, code = REFUSED[cid]
    good = (INDICES[0], LISTS["lds_limit"])
    rc, recs, gs, spare, spare_g, status, _ = run_batch(gpu_pkg, NBMU, [good, (INDICES[1], LISTS["lds_limit"]), good], mutate=mutate)
    assert rc == code, (rc, code)
    assert all(bool(torch.isnan(r).all()) for r in recs) and all(bool(torch.isnan(x).all()) for x in gs)
    assert bool((status == -77).all())


@pytest.mark.gpu
def test_batch_refuses_a_short_work_area_and_takes_count_0(gpu_pkg):
    import torch
    jobs = [(INDICES[0], LISTS["lds_limit"]), (INDICES[1], LISTS["one"])]
    rc, recs, gs, _, _, status, nbytes = run_batch(gpu_pkg, NBMU, jobs, short=1)
    assert rc == E_UNSUPPORTED and nbytes > 0
    assert all(bool(torch.isnan(r).all()) for r in recs) and bool((status == -77).all())
    rc, recs, gs, _, _, status, _ = run_batch(gpu_pkg, NBMU, jobs, count=0)
    assert rc == 0
    assert all(bool(torch.isnan(r).all()) for r in recs) and bool((status == -77).all())
    assert run_batch(gpu_pkg, NBMU, jobs)[0] == 0                              # (the same call, whole)


@pytest.mark.gpu
def test_batch_takes_a_positive_imaginary_part_as_sosgpu_mie_does(gpu_pkg):
    """sosgpu_mie does not look at the sign of `in`: the batch gives the same return code and the same bits."""
    import torch
    al = np.array([0.5, 30.0, 860.0])
    rc0, rec, g = T.run_mie(gpu_pkg, NBMU, 1.5, 0.01, al, fill=float("nan"))
    rc, recs, gs, _, _, status, _ = run_batch(gpu_pkg, NBMU, [((1.5, 0.01), al)])
    assert rc == rc0 == 0 and int(status[0]) == 0
    assert torch.equal(recs[0], rec) and torch.equal(gs[0], g)


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6. the host path: streams, launch accounting, the byte budget
# ---------------------------------------------------------------------------------------------------------------------
def _fresh(A_):
    with A_._MIE_LOCK:
        A_._MIE_CACHE.clear()
    A_.drop_prefetched_size_integrals()


def _mkey(A_, xmu, rn, in_, alphaf, device=0):
    return (np.ascontiguousarray(xmu, dtype=np.float64).tobytes(), float(rn), float(in_), float(A_.MIE_ALPHAMIN), float(alphaf), device)


STREAM_KEYS = [(1.53, -0.008, 35.0), (1.381, 0.0, 120.0), (1.75, -0.44, 870.0)]


@pytest.mark.gpu
def test_records_prefetched_on_a_side_stream_are_ordered_before_the_default_stream(gpu_pkg, monkeypatch):
    """prefetch_mie_records on a side stream, then _mie_device_records and size_integral from the default stream with no
    synchronisation in between: the bits of the synchronous path."""
    import torch
    monkeypatch.delenv("SOS_MIE_DEVICE_BYTES", raising=False)
    Ap = gpu_pkg.aerosols
    xmu = T.xmu_of(NBMU)
    _fresh(Ap)
    want = []
    for rn, in_, af in STREAM_KEYS:
        rec, g = Ap._mie_device_records(xmu, rn, in_, Ap.MIE_ALPHAMIN, af)
        want.append((rec.clone(), g.clone(), Ap.size_integral(xmu, rn, in_, af, 1, 0.12, 0.45, -999.0, 0.55)))
    torch.cuda.synchronize()
    _fresh(Ap)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        made = Ap.prefetch_mie_records([_mkey(Ap, xmu, rn, in_, af) for rn, in_, af in STREAM_KEYS])
    assert len(made) == 3 and all(e.batch is not None and e.batch.stream == side for e in made.values())
    for (rn, in_, af), (rec0, g0, si0) in zip(STREAM_KEYS, want):
        rec, g = Ap._mie_device_records(xmu, rn, in_, Ap.MIE_ALPHAMIN, af)
        assert torch.equal(rec, rec0) and torch.equal(g, g0)
        si = Ap.size_integral(xmu, rn, in_, af, 1, 0.12, 0.45, -999.0, 0.55)
        assert si[:3] == si0[:3] and all(np.array_equal(a, b) for a, b in zip(si[3:], si0[3:]))
    _fresh(Ap)


def _wmo_user(wa, model, nb=12, rad=8):
    return {"-ANG.Rad.NbGauss": rad, "-ANG.Aer.NbGauss": nb, "-ANG.Thetas": 40.0, "-AP.Psurf": 1013.0, "-AP.HR": 8.0,
            "-AP.AerHS.HA": 2.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.25, "-AER.Waref": 0.55, "-AER.Tronca": 1,
            "-SOS.IGmax": 100, "-SOS.View": 1, "-SOS.View.Phi": 60.0, "-SURF.Type": 0, "-SURF.Alb": 0.08, "-SOS_Main.Wa": wa,
            "-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT", "-AER.Model": 1, "-AER.WMO.Model": model}


def _sf_user(wa, nb=12, rad=8):
    u = _wmo_user(wa, 0, nb, rad)
    del u["-AER.WMO.Model"]
    u.update({"-AER.Model": 2, "-AER.SF.Model": 3, "-AER.SF.RH": 70.0})
    return u


def _kw(rs, user):
    return rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False)


def _count_calls(monkeypatch, L):
    n = dict(mie=0, batch=0, jobs=[])
    f_mie, f_batch = L.sosgpu_mie, L.sosgpu_mie_batch

    def mie(*a):
        n["mie"] += 1
        return f_mie(*a)

    def batch(*a):
        n["batch"] += 1
        n["jobs"].append(a[3])
        return f_batch(*a)

    monkeypatch.setattr(L, "sosgpu_mie", mie)
    monkeypatch.setattr(L, "sosgpu_mie_batch", batch)
    return n


@pytest.mark.gpu
def test_prefetch_makes_one_mie_batch_per_32_integrals(gpu_pkg, monkeypatch):
    """20 wavelengths of the WMO maritime model: the prefetch makes no sosgpu_mie call and ceil(jobs / 32) sosgpu_mie_batch
    calls; SOS_SPECTRUM_MIE_PER_CALL=1 reverses the counts; the integrals of both and of plain size_integral calls are the
    same bits."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_MIE_PER_CALL", raising=False)
    monkeypatch.delenv("SOS_MIE_DEVICE_BYTES", raising=False)
    rs, Ap = gpu_pkg.run_sos, gpu_pkg.aerosols
    reqs = []
    for wa in np.linspace(0.45, 0.86, 20):
        v = rs._validated(_kw(rs, _wmo_user(float(round(wa, 4)), 2)))
        reqs += rs._size_integral_requests(rs._aerosol_call(v, None), 0)
    reqs = list(dict.fromkeys(reqs))
    assert len(reqs) >= 40, len(reqs)
    groups = [reqs[c:c + 32] for c in range(0, len(reqs), 32)]
    seen, expect_batches, expect_mie = set(), 0, 0
    for grp in groups:                                   # a group makes a batch call when it has a refractive index not met before
        new = {(k[1], k[2], k[3]) for k in grp} - seen
        expect_batches += bool(new)
        expect_mie += len(new)
        seen |= new
    assert expect_batches == math.ceil(len(reqs) / 32)    # (every group of this spectrum has one: the index moves with the wavelength)
    n = _count_calls(monkeypatch, gpu_pkg.capi.lib())

    def run(prefetch):
        _fresh(Ap)
        n.update(mie=0, batch=0, jobs=[])
        if prefetch:
            assert Ap.prefetch_size_integrals(reqs) == len(reqs)
        counts = (n["mie"], n["batch"], sum(n["jobs"]))
        out = [Ap.size_integral(np.frombuffer(k[0]), *k[1:9], device=k[9]) for k in reqs]
        if prefetch:
            assert (n["mie"], n["batch"]) == counts[:2]  # every integral came from the batch: nothing computed again
        _fresh(Ap)
        return counts, out

    c_batch, o_batch = run(True)
    monkeypatch.setenv("SOS_SPECTRUM_MIE_PER_CALL", "1")
    c_call, o_call = run(True)
    monkeypatch.delenv("SOS_SPECTRUM_MIE_PER_CALL")
    _, o_plain = run(False)
    print("mie launch accounting: %d integrals, %d indices; batch path %s, per-call path %s" % (len(reqs), expect_mie, c_batch, c_call))
    assert c_batch == (0, expect_batches, expect_mie), c_batch
    assert c_call == (expect_mie, 0, 0), c_call
    for a, b, c in zip(o_batch, o_call, o_plain):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.gpu
def test_record_cache_keeps_a_byte_budget_with_lru_eviction(gpu_pkg, monkeypatch):
    """A budget of two small record sets: the third evicts the least recently used, a re-request recomputes the same bits, and
    a set a pending integral batch reads stays valid until the result is read."""
    import torch
    Ap = gpu_pkg.aerosols
    xmu = T.xmu_of(NBMU)
    keys = [(1.53, -0.008, 20.0), (1.381, 0.0, 20.0), (1.75, -0.44, 20.0)]
    one = len(Ap.alpha_grid(Ap.MIE_ALPHAMIN, 20.0)) * ((4 + 3 * 25) * 4 + 8)
    monkeypatch.setenv("SOS_MIE_DEVICE_BYTES", str(2 * one + one // 2))
    monkeypatch.delenv("SOS_SPECTRUM_MIE_PER_CALL", raising=False)
    _fresh(Ap)
    first = Ap._mie_device_records(xmu, *keys[0][:2], Ap.MIE_ALPHAMIN, 20.0)
    first = (first[0].clone(), first[1].clone())
    Ap._mie_device_records(xmu, *keys[1][:2], Ap.MIE_ALPHAMIN, 20.0)
    Ap._mie_device_records(xmu, *keys[0][:2], Ap.MIE_ALPHAMIN, 20.0)             # touch 0: now 1 is the least recently used
    Ap._mie_device_records(xmu, *keys[2][:2], Ap.MIE_ALPHAMIN, 20.0)
    mk = [_mkey(Ap, xmu, rn, in_, af) for rn, in_, af in keys]
    assert list(Ap._MIE_CACHE) == [mk[0], mk[2]]
    assert sum(e.nbytes for e in Ap._MIE_CACHE.values()) == 2 * one
    Ap._mie_device_records(xmu, *keys[1][:2], Ap.MIE_ALPHAMIN, 20.0)             # evicts 0
    assert list(Ap._MIE_CACHE) == [mk[2], mk[1]]
    again = Ap._mie_device_records(xmu, *keys[0][:2], Ap.MIE_ALPHAMIN, 20.0)     # recomputed
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # a pending integral batch over all three sets: more than the budget holds, each integral still reads its own records
    _fresh(Ap)
    want = [Ap.size_integral(xmu, rn, in_, af, 1, 0.12, 0.45, -999.0, 0.55) for rn, in_, af in keys]
    _fresh(Ap)
    reqs = [Ap._granu_key(xmu, rn, in_, af, 1, 0.12, 0.45, -999.0, 0.55, 0) for rn, in_, af in keys]
    assert Ap.prefetch_size_integrals(reqs) == 3
    assert len(Ap._MIE_CACHE) == 2                                               # the budget held while the batch was queued
    for (rn, in_, af), w in zip(keys, want):
        got = Ap.size_integral(xmu, rn, in_, af, 1, 0.12, 0.45, -999.0, 0.55)
        assert got[:3] == w[:3] and all(np.array_equal(a, b) for a, b in zip(got[3:], w[3:]))
    _fresh(Ap)


# ---------------------------------------------------------------------------------------------------------------------
# 7. end to end: the Mie -> GRANU -> Legendre chain of a table-model spectrum
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_table_model_spectrum_equals_sos_proc_bit_for_bit(gpu_pkg, monkeypatch):
    """sos_spectrum over WMO maritime (LDS form only), WMO continental (dust-like: scratch form) and Shettle & Fenn maritime at
    70 % humidity == sos_proc of the same keywords one after the other, every element of every 23-tuple; and again with
    SOS_SPECTRUM_MIE_PER_CALL=1."""
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_MIE_PER_CALL", raising=False)
    monkeypatch.delenv("SOS_MIE_DEVICE_BYTES", raising=False)
    rs, Ap = gpu_pkg.run_sos, gpu_pkg.aerosols
    users = [_wmo_user(0.49, 2), _wmo_user(0.67, 2), _wmo_user(0.56, 1), _wmo_user(0.865, 1), _sf_user(0.67), _sf_user(0.78)]
    kws = [_kw(rs, u) for u in users]
    _fresh(Ap)
    seq = [rs.sos_proc(**kw) for kw in kws]
    assert all(len(o) == 23 for o in seq)

    def same(outs, what):
        assert len(outs) == len(seq)
        for i, (a, b) in enumerate(zip(seq, outs)):
            for j, (x, y) in enumerate(zip(a, b)):
                assert np.array_equal(np.asarray(x), np.asarray(y)), (what, i, j)

    n = _count_calls(monkeypatch, gpu_pkg.capi.lib())
    _fresh(Ap)
    same(rs.sos_spectrum(kws), "batch")
    print("table-model spectrum: %d sosgpu_mie_batch calls of %s jobs, %d sosgpu_mie calls" % (n["batch"], n["jobs"], n["mie"]))
    assert n["batch"] >= 1, n
    monkeypatch.setenv("SOS_SPECTRUM_MIE_PER_CALL", "1")
    n.update(mie=0, batch=0, jobs=[])
    _fresh(Ap)
    same(rs.sos_spectrum(kws), "per call")
    assert n["batch"] == 0 and n["mie"] >= 1, n
    _fresh(Ap)
