"""The surface matrices of many jobs in one asynchronous call (sosgpu_surface_batch, surface.surface_matrices_many) against
the per-call entry points sosgpu_glitter / sosgpu_land_surface, bit for bit: those are held to the oracle and the reference's
files by test_surface_matrix.py and test_land.py, so equality with them carries those bars over.  The CPU part checks the
refusals, the work-area size and the request grouping of the spectrum prefetch (run_sos._surface_requests)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_surface_matrix import NEGATIVE_TRIPLE, TRIPLES, angles

ORDERS = (24, 24, 48)
PATTERN = 0x7FC0DEAD                               # a quiet NaN no kernel produces


def sea(wind, ind):
    return dict(isurf=1, wind=float(wind), ind=float(ind), k0=0.0, k1=0.0, k2=0.0, coef_c=0.0)


def land(isurf, triple, ind=1.5, coef_c=0.0):
    k0, k1, k2 = triple
    return dict(isurf=int(isurf), wind=0.0, ind=float(ind) if isurf >= 4 else 1.0, k0=float(k0), k1=float(k1), k2=float(k2),
                coef_c=float(coef_c))


# test 1: what is shared and what is not -- two winds, two indices, a repeated job, every land model, two Maignan C
MIXED = [sea(2, 1.33), sea(2, 1.34), sea(7, 1.34), sea(2, 1.33),
         land(3, TRIPLES[1]), land(3, TRIPLES[3]), land(4, TRIPLES[0]), land(5, TRIPLES[2]),
         land(7, TRIPLES[1], coef_c=4.0), land(7, TRIPLES[3], coef_c=4.0), land(7, TRIPLES[1], coef_c=8.0)]


def _key(job):
    return tuple(sorted(job.items()))


@functools.lru_cache(maxsize=None)
def _per_call_cached(n, sun, orders, key):
    """The block of one job from the per-call entry point (computed once per (angles, orders, job), kept on the host)."""
    import importlib
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    job = dict(key)
    mu, w, _ = angles(n, sun)
    os_nb, os_ns, os_nm = orders
    if job["isurf"] == 1:
        r = pkg.surface.glitter_matrices(mu, w, job["wind"], job["ind"], os_nb, os_ns, os_nm)["rsurf"]
    else:
        lm = pkg.surface.land_model(job["isurf"], job["k0"], job["k1"], job["k2"], coef_c=job["coef_c"])
        r = pkg.surface.land_matrices(lm, mu, w, job["ind"], os_nb, os_ns, os_nm)
    return r.cpu().numpy()


def per_call(n, sun, orders, job):
    return _per_call_cached(n, sun, orders, _key(job))


def batch(pkg, n, sun, orders, jobs):
    import torch
    mu, w, _ = angles(n, sun)
    blocks, status = pkg.surface.surface_matrices_many(jobs, mu, w, *orders)
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in blocks], status.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.gpu
def test_mixed_list_equals_the_per_call_entry_points(gpu_pkg):
    blocks, status = batch(gpu_pkg, 13, 40.0, ORDERS, MIXED)
    assert len(blocks) == len(MIXED) and np.array_equal(status, np.zeros(len(MIXED), dtype=np.int32))
    for j, job in enumerate(MIXED):
        assert same_bits(blocks[j], per_call(13, 40.0, ORDERS, job)), (j, job)
    assert MIXED[0] == MIXED[3] and same_bits(blocks[0], blocks[3])
    assert not same_bits(blocks[0], blocks[1]) and not same_bits(blocks[8], blocks[10])


@pytest.mark.gpu
def test_order_of_jobs_does_not_matter(gpu_pkg):
    fwd, _ = batch(gpu_pkg, 13, 40.0, ORDERS, MIXED)
    rev, status = batch(gpu_pkg, 13, 40.0, ORDERS, MIXED[::-1])
    assert not status.any()
    for a, b in zip(fwd, rev[::-1]):
        assert same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n,orders,jobs", [
    (3, (129, 130, 259), [sea(7, 1.34), land(7, TRIPLES[3], coef_c=4.0)]),     # second trip of the 128-thread and 64-lane loops
    (85, (2, 2, 4), [sea(7, 1.34), land(3, TRIPLES[3])]),                      # 3655 / 7225 pairs per set
    (13, ORDERS, [sea(2, 1.33)]),                                              # one job: first = last entry of every table
    (13, ORDERS, [land(3, TRIPLES[1])]),
], ids=["N3-second-trip", "N85", "single-sea", "single-roujean"])
def test_stride_and_grid_edges(gpu_pkg, n, orders, jobs):
    blocks, status = batch(gpu_pkg, n, 40.0, orders, jobs)
    assert not status.any()
    for j, job in enumerate(jobs):
        assert same_bits(blocks[j], per_call(n, 40.0, orders, job)), (j, job)


@pytest.mark.gpu
def test_negative_roujean_flags_its_job_alone(gpu_pkg):
    jobs = [land(3, TRIPLES[0]), land(7, TRIPLES[1], coef_c=4.0), land(3, NEGATIVE_TRIPLE), land(4, TRIPLES[2]),
            land(7, TRIPLES[3], coef_c=4.0)]
    blocks, status = batch(gpu_pkg, 3, 40.0, ORDERS, jobs)
    assert status.tolist() == [0, 0, -1, 0, 0]
    for j in (0, 1, 3, 4):
        assert same_bits(blocks[j], per_call(3, 40.0, ORDERS, jobs[j])), j
    # the flag belongs to the triple, whatever the model that carries it
    _, status = batch(gpu_pkg, 3, 40.0, ORDERS, [land(7, NEGATIVE_TRIPLE, coef_c=4.0), land(3, TRIPLES[0])])
    assert status.tolist() == [-1, 0]


@pytest.mark.gpu
def test_guards_and_work_area(gpu_pkg):
    """Blocks in one allocation pre-filled with a NaN pattern, guard rows between and after them, a work area larger than asked
    for: every element of every block is written, no guard row and nothing beyond work_bytes is touched."""
    import torch
    S, L = gpu_pkg.surface, gpu_pkg.capi.lib()
    n, (os_nb, os_ns, os_nm) = 5, ORDERS
    mu, w, _ = angles(n, 40.0)
    jobs = [sea(2, 1.33), land(3, TRIPLES[1]), land(7, TRIPLES[3], coef_c=4.0), land(4, TRIPLES[0]), sea(7, 1.33)]
    cnt, guard = (os_nb + 1) * 9 * n * n, 64
    dev = torch.device("cuda", 0)
    out = torch.full((len(jobs), cnt + guard), PATTERN, dtype=torch.int32, device=dev)
    arr = S.surface_job_array(jobs, [out[j].data_ptr() for j in range(len(jobs))])
    need = L.sosgpu_surface_batch_work_bytes(n, os_nb, os_ns, os_nm, arr, len(jobs))
    assert need > 0 and need % 8 == 0
    extra = 4096
    work = torch.full((need + extra,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((len(jobs) + 2,), 77, dtype=torch.int32, device=dev)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = L.sosgpu_surface_batch(0, n, dp(mu), dp(w), os_nb, os_ns, os_nm, arr, len(jobs), C.c_void_p(status.data_ptr()),
                                C.c_void_p(work.data_ptr()), need, st)
    assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert not (o[:, :cnt] == PATTERN).any()
    assert (o[:, cnt:] == PATTERN).all()
    assert (work[need:] == 0xA5).all().item()
    assert status.cpu().tolist() == [0] * len(jobs) + [77, 77]
    for j, job in enumerate(jobs):
        assert np.array_equal(o[j, :cnt], per_call(n, 40.0, ORDERS, job).view(np.int32).ravel()), j


# ---------------------------------------------------------------------------------------------------------------------
# CPU: refusals, the size of the work area, the request grouping of the spectrum prefetch
# ---------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20                                     # a non-NULL, 8-byte aligned address: a refused call touches nothing


def _call(pkg, jobs, n=13, orders=ORDERS, mu=True, chr_=True, status=FAKE, work=FAKE, work_bytes=None, njobs=None, ptr=FAKE,
          null_jobs=False):
    L = pkg.capi.lib()
    m, w, _ = angles(min(max(n, 3), 85), 40.0)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    arr = pkg.surface.surface_job_array(jobs, [ptr] * len(jobs))
    nj = len(jobs) if njobs is None else njobs
    if work_bytes is None:
        work_bytes = 1 << 40
    return L.sosgpu_surface_batch(0, n, dp(m) if mu else None, dp(w) if chr_ else None, orders[0], orders[1], orders[2],
                                  None if null_jobs else arr, nj, C.c_void_p(status) if status else None,
                                  C.c_void_p(work) if work else None, work_bytes, None)


def _bytes(pkg, jobs, n=13, orders=ORDERS, njobs=None, null_jobs=False):
    arr = pkg.surface.surface_job_array(jobs)
    return pkg.capi.lib().sosgpu_surface_batch_work_bytes(n, orders[0], orders[1], orders[2], None if null_jobs else arr,
                                                          len(jobs) if njobs is None else njobs)


def test_refusals_come_before_any_device_work(pkg):
    E_ARG, E_UNSUPPORTED = -1, -3
    jobs = [sea(2, 1.33), land(7, TRIPLES[1], coef_c=4.0)]
    refused = [dict(n=0), dict(n=86), dict(orders=(-1, 24, 48)), dict(orders=(24, 1, 48)), dict(orders=(24, 24, 47)),
               dict(orders=(24, 24, 2001)), dict(orders=(2, 1575, 1577)), dict(null_jobs=True), dict(njobs=-1)]
    for kw in refused:
        assert _call(pkg, jobs, **kw) == E_ARG, kw
        assert _bytes(pkg, jobs, **kw) == 0, kw
    assert _call(pkg, [sea(2, 1.33)] * 4, njobs=65536) == E_ARG and _bytes(pkg, [sea(2, 1.33)] * 4, njobs=65536) == 0
    for bad in (0, 2, 8, -1):
        assert _call(pkg, jobs + [dict(sea(2, 1.33), isurf=bad)]) == E_ARG
        assert _bytes(pkg, jobs + [dict(sea(2, 1.33), isurf=bad)]) == 0
    nadal = jobs + [land(6, TRIPLES[0])]
    assert _call(pkg, nadal) == E_UNSUPPORTED and _bytes(pkg, nadal) == 0
    assert _call(pkg, nadal + [dict(sea(2, 1.33), isurf=2)]) == E_ARG       # a bad argument outranks the unsupported model
    for kw in (dict(mu=False), dict(chr_=False), dict(status=0), dict(work=0), dict(ptr=None), dict(work=FAKE + 4)):
        assert _call(pkg, jobs, **kw) == E_ARG, kw
    need = _bytes(pkg, jobs)
    assert need > 0
    assert _call(pkg, jobs, work_bytes=need - 1) == E_ARG and _call(pkg, jobs, work_bytes=0) == E_ARG
    # no job: nothing to do, whatever the device
    assert _call(pkg, [], njobs=0) == 0 and _bytes(pkg, [], njobs=0) > 0
    # the LDS edge of sosgpu_glitter is accepted
    assert _bytes(pkg, jobs, n=3, orders=(2, 1574, 1576)) > 0


def test_work_bytes_grows_with_what_is_distinct(pkg):
    n, (os_nb, os_ns, os_nm) = 13, ORDERS
    npairs, nn, cnt = n * (n + 1) // 2, n * n, (os_nb + 1) * 9 * n * n
    sizes, jobs = [], []
    for job in MIXED:
        jobs.append(job)
        sizes.append(_bytes(pkg, jobs))
    assert all(b > 0 and b % 8 == 0 for b in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    job_entry = sizes[3] - sizes[2]                 # the repeated sea job adds its table entry and nothing else
    assert 0 < job_entry <= 64
    analysis, block, roujean = npairs * (os_nm + 1) * 8, cnt * 4, nn * (os_nb + 1) * 8
    # a new index on a known wind: a Fresnel set and a reflexion block, no analysis
    assert block + 4 * (os_ns + 1) * 8 <= sizes[1] - sizes[0] + 8 < block + analysis
    # a new wind on a known index: an analysis and a reflexion block
    assert sizes[2] - sizes[1] + 8 >= analysis + block
    # a second Roujean triple: its analysis, no reflexion block
    assert roujean <= sizes[5] - sizes[4] < roujean + block


def _kwargs(rs, **user):
    base = {"-SOS_Main.Wa": 0.67, "-ANG.Rad.NbGauss": 12, "-ANG.Aer.NbGauss": 12, "-ANG.Thetas": 40.0, "-AP.Psurf": 1013.0,
            "-AP.HR": 8.0, "-AP.AerHS.HA": 2.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.0, "-AER.Waref": 0.67, "-SURF.Alb": 0.0,
            "-SOS.IGmax": 100, "-SOS.View": 2, "-SOS.View.Dphi": 60, "-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT"}
    base.update(user)
    return rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), base), trace=False)


def _roujean(t):
    return {"-SURF.Roujean.K0": t[0], "-SURF.Roujean.K1": t[1], "-SURF.Roujean.K2": t[2]}


def test_surface_requests_of_a_call_list(pkg, tmp_path):
    rs = pkg.run_sos
    f = tmp_path / "surf.bin"
    f.write_bytes(b"")
    sea_kw = {"-SURF.Type": 1, "-SURF.Ind": 1.34, "-SURF.Glitter.Wind": 7.0}
    calls = [
        _kwargs(rs, **{"-SURF.Type": 3}, **_roujean(TRIPLES[0])),
        _kwargs(rs, **sea_kw),
        _kwargs(rs, **{"-SURF.Type": 0}),                                                   # Lambert: left out
        _kwargs(rs, **{"-SURF.Type": 7, "-SURF.Ind": 1.5, "-SURF.Maignan.C": 4.0}, **_roujean(TRIPLES[1])),
        _kwargs(rs, **{"-SURF.Type": 2, "-SURF.Ind": 1.34}),                                # flat sea: left out
        _kwargs(rs, **dict(sea_kw, **{"-SURF.File": str(f)})),                              # the user's matrices: left out
        _kwargs(rs, **dict(sea_kw, **{"-SURF.Ind": 1.33, "-ANG.Rad.NbGauss": 16})),         # another angle set
        _kwargs(rs, **sea_kw),                                                              # a repeated surface: one job
        _kwargs(rs, **{"-SURF.Type": 4, "-SURF.Ind": 1.5, "-ANG.Thetas": 30.0}, **_roujean(TRIPLES[2])),   # another sun
        _kwargs(rs, **{"-SURF.Type": 3}),                                                   # no coefficients: refused, the pass reports
    ]
    valid = [rs._validated(kw) for kw in calls]
    assert [v is None for v in valid] == [False] * 9 + [True]
    groups = rs._surface_requests(valid, device=0)
    assert [len(g["keys"]) for g in groups] == [3, 1, 1]
    assert [(g["os_nb"], g["os_ns"], g["os_nm"]) for g in groups] == [(24, 24, 48), (24, 32, 56), (24, 24, 48)]
    mu12, ga12, _, _ = rs.angles(12, 40.0, "NO_USER_ANGLES")
    mu16, ga16, _, _ = rs.angles(16, 40.0, "NO_USER_ANGLES")
    mu30, ga30, _, _ = rs.angles(12, 30.0, "NO_USER_ANGLES")
    for g, (m, w) in zip(groups, [(mu12, ga12), (mu16, ga16), (mu30, ga30)]):
        assert np.array_equal(g["mu"], m) and np.array_equal(g["ga"], w)
    D = rs.SOS_NOT_DEFINED_VALUE_DBLE
    t0, t1, t2 = TRIPLES[0], TRIPLES[1], TRIPLES[2]
    # the keys as _prepare forms them for _surface_cached
    assert groups[0]["keys"] == [
        ("land", 3, t0[0], t0[1], t0[2], D, D, D, mu12.tobytes(), ga12.tobytes(), 1.0, 24, 24, 48, 0),
        ("glitter", mu12.tobytes(), ga12.tobytes(), 7.0, 1.34, 24, 24, 48, 0),
        ("land", 7, t1[0], t1[1], t1[2], D, D, 4.0, mu12.tobytes(), ga12.tobytes(), 1.5, 24, 24, 48, 0)]
    assert groups[1]["keys"] == [("glitter", mu16.tobytes(), ga16.tobytes(), 7.0, 1.33, 24, 32, 56, 0)]
    assert groups[2]["keys"] == [("land", 4, t2[0], t2[1], t2[2], D, D, D, mu30.tobytes(), ga30.tobytes(), 1.5, 24, 24, 48, 0)]
    assert groups[0]["jobs"] == [land(3, t0, coef_c=D), sea(7.0, 1.34), land(7, t1, coef_c=4.0)]
    assert groups[2]["jobs"] == [land(4, t2, coef_c=D)]
    assert rs._surface_requests([None, valid[2]], device=0) == []
