"""Diffuse and total fluxes at every output altitude of a levels call (sosgpu_level_flux, sosgpu_level_flux_spectrum,
solver.level_flux_many; k_level_flux / k_level_flux_table of csrc/flux.hip; fluxes=True of run_sos.sos_proc_levels and
sos_spectrum_levels).

CPU: the C ABI (declared, exported, listed; the job structure; the refusals before any device work; the work area), the
fluxes keyword, the columns of a flux row.
GPU: both kernels bit for bit against a sequential host restatement at every edge of the 32-jobs-per-workgroup mapping; the
call counts of the entry points; the standard-output row against sos_proc's own fluxes; interior altitudes against the oracle;
the flag off changes nothing."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

import cases
import spectrum_cases
from spectrum_cases import assert_tuples_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = spectrum_cases.GOLD
S = cases.S
E_ARG = -1
GUARD = 8                                     # doubles behind d_out, preset to NaN


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_symbols_are_declared_exported_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"\bint\s+sosgpu_level_flux\s*\(sosgpu_ctx \*cx, const double \*d_rec, double \*d_out[^,)]*, void \*stream\);",
                     hdr)
    assert re.search(r"typedef struct sosgpu_flux_job \{\s*sosgpu_ctx \*cx;\s*const double \*d_rec;\s*\} sosgpu_flux_job;", hdr)
    assert re.search(r"\bsize_t\s+sosgpu_level_flux_spectrum_work_bytes\s*\(int njobs\);", hdr)
    assert re.search(r"\bint\s+sosgpu_level_flux_spectrum\s*\(const sosgpu_flux_job \*jobs, int njobs, double \*d_out[^,)]*,\s*"
                     r"void \*d_work, size_t work_bytes, void \*stream\);", hdr)
    for sym in ("sosgpu_level_flux", "sosgpu_level_flux_spectrum", "sosgpu_level_flux_spectrum_work_bytes"):
        assert sym in pkg.capi.EXPORTS
        assert hasattr(pkg.capi.lib(), sym)
    # the ctypes job is the header's structure: two pointers
    assert [f[0] for f in pkg.capi.FluxJob._fields_] == ["cx", "d_rec"]
    assert C.sizeof(pkg.capi.FluxJob) == 2 * C.sizeof(C.c_void_p) == 16
    assert pkg.run_sos.LEVEL_FLUX_NAMES == ["flux_dir_down_tronc", "flux_diff_down_tronc", "flux_tot_down", "flux_diff_up",
                                            "flux_net"]


def test_arguments_are_refused_without_a_device(pkg):
    """NULL cx, d_rec and d_out of the single call; NULL jobs, d_out and d_work, njobs = -1, a job with a NULL context or a NULL
    record and a misaligned work area of the spectrum call are refused, and njobs = 0 is accepted, before any device is looked
    for (the rule for contexts on different devices needs two devices and is not exercised here)."""
    L = pkg.capi.lib()
    p, nw = C.c_void_p(4096), 1 << 30                        # never dereferenced: nothing is queued by these calls
    assert L.sosgpu_level_flux(None, p, p, None) == E_ARG
    assert L.sosgpu_level_flux(p, None, p, None) == E_ARG
    assert L.sosgpu_level_flux(p, p, None, None) == E_ARG
    jobs = (pkg.capi.FluxJob * 2)()
    assert L.sosgpu_level_flux_spectrum(None, 1, p, p, nw, None) == E_ARG
    assert L.sosgpu_level_flux_spectrum(jobs, 1, None, p, nw, None) == E_ARG
    assert L.sosgpu_level_flux_spectrum(jobs, 1, p, None, nw, None) == E_ARG
    assert L.sosgpu_level_flux_spectrum(jobs, -1, p, p, nw, None) == E_ARG
    assert L.sosgpu_level_flux_spectrum(jobs, 2, p, p, nw, None) == E_ARG            # both jobs empty: NULL context
    jobs[0].cx, jobs[0].d_rec = 4096, None
    assert L.sosgpu_level_flux_spectrum(jobs, 1, p, p, nw, None) == E_ARG            # NULL record
    jobs[0].cx, jobs[0].d_rec = None, 4096
    assert L.sosgpu_level_flux_spectrum(jobs, 1, p, p, nw, None) == E_ARG            # NULL context
    assert L.sosgpu_level_flux_spectrum(jobs, 1, p, C.c_void_p(4100), nw, None) == E_ARG
    assert L.sosgpu_level_flux_spectrum(jobs, 0, p, p, nw, None) == 0


def test_work_bytes(pkg):
    f = pkg.capi.lib().sosgpu_level_flux_spectrum_work_bytes
    assert f(0) == 0 and f(-1) == 0
    sizes = [f(n) for n in (0, 1, 2, 3, 33, 100, 65535)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 8 == 0 for s in sizes)


def test_fluxes_must_be_a_bool(pkg):
    rs = pkg.run_sos
    kw = rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), {"-SOS_Main.Wa": 0.55, "-AER.AOTref": 0.0}),
                            trace=False)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError):
            rs.sos_proc_levels([1.0], fluxes=bad, **kw)
        with pytest.raises(ValueError):
            rs.sos_spectrum_levels([1.0], [kw], fluxes=bad)
    assert rs.sos_spectrum_levels([-1.0, 3.0], [], fluxes=True) == ([], [])


def test_flux_row_columns(pkg):
    """The direct term of an interior altitude uses TAUOUT, that of altitude -1 the whole truncated depth; the total is the sum
    of the direct and the diffuse down-going columns, the net the total minus the up-going column."""
    rs = pkg.run_sos
    pl = types.SimpleNamespace(p=dict(tetas=40.0))
    fin = dict(ttot_tronc=np.array([0.0, 0.5]), tauout=np.array([0.0, 0.2]))
    cs = math.cos(math.pi * 40.0 / 180.0)
    for alt, tau in ((3.0, 0.2), (-1.0, 0.5)):
        row = rs._level_flux_row(pl, alt, fin, 1, (0.125, 0.0625))
        assert len(row) == len(rs.LEVEL_FLUX_NAMES)
        assert row[0] == math.exp(-tau / cs) and row[1] == 0.125 and row[3] == 0.0625
        assert row[2] == 0.125 + math.exp(-tau / cs) and row[4] == row[2] - row[3]


# ---------------------------------------------------------------------------------------------------------------- GPU tests

NS = (2, 9, 41, 85)                           # directions of the contexts (the library's range is 1..85)
JOB_COUNTS = (1, 31, 32, 33, 64, 65)          # round the 32 jobs of a 64-thread workgroup


def host_flux(mu, ga, n0, row):
    """(E-, E+) of an order-0 intensity row: the reference's statements (SOS_OS.F:1447-1456), left to right in doubles."""
    n = len(mu)
    out = []
    for sign in (-1, 1):
        e = 0.0
        for j in range(1, n + 1):
            e = e + float(mu[j - 1]) * float(ga[j - 1]) * float(row[n + sign * j])
        tab = -float(mu[n0 - 1])
        out.append(-e * 2 / tab)
    return out


def _contexts(gpu_pkg, order):
    """Contexts of N = NS in `order`, unbuilt: the flux kernels read mu, ga and n0 only."""
    al, be, ga, ze = S.hg_phase(8, 0.6)
    ctxs = {}
    for n in order:
        mu, w, n0 = S.gauss_angles(n - 1, 35.0)
        assert len(mu) == n
        ctxs[n] = gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, build=False)
    return ctxs


def _records(seed):
    """Two records [2][3][W] per N: random doubles of both signs over many magnitudes, some zero, some 1e-300."""
    rng = np.random.default_rng(seed)
    recs = {}
    for n in NS:
        w = 2 * n + 1
        for v in range(2):
            r = rng.standard_normal((2, 3, w)) * 10.0 ** rng.integers(-12, 4, (2, 3, w))
            r[rng.random((2, 3, w)) < 0.15] = 0.0
            r[rng.random((2, 3, w)) < 0.15] = 1e-300
            r[0, 0, rng.integers(0, w)] = -1e-300
            recs[(n, v)] = r
    return recs


def _flux_call(gpu_pkg, items):
    """One sosgpu_level_flux_spectrum call made by hand for items (ctx, device record): the output followed by a guard of NaNs.
    Returns (return code, out [njobs][2], guard) on the host."""
    import torch
    L, cap = gpu_pkg.capi.lib(), gpu_pkg.capi
    n = len(items)
    jobs = (cap.FluxJob * n)()
    for j, (cx, rec) in zip(jobs, items):
        j.cx, j.d_rec = cx._h.value, rec.data_ptr()
    out = torch.full((2 * n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    nw = int(L.sosgpu_level_flux_spectrum_work_bytes(n))
    work = torch.empty(nw, dtype=torch.uint8, device="cuda")
    rc = L.sosgpu_level_flux_spectrum(jobs, n, C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), nw,
                                      items[0][0]._stream())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return rc, out[:2 * n].reshape(n, 2), out[2 * n:]


def _check(gpu_pkg, items, refs, what):
    rc, out, guard = _flux_call(gpu_pkg, items)
    assert rc == 0, what
    assert guard.size == GUARD and np.isnan(guard).all(), what
    assert np.array_equal(out, refs), (what, np.argwhere(out != refs)[:4].tolist())
    many = gpu_pkg.solver.level_flux_many(items)
    assert tuple(many.shape) == (len(items), 2) and np.array_equal(many.cpu().numpy(), refs), what


def _round(gpu_pkg, ctxs, seed):
    """Every job count, the mixed orders, shared records and the by-value kernel on the contexts `ctxs`."""
    import torch
    host = _records(seed)
    dev = {k: torch.from_numpy(r).cuda() for k, r in host.items()}
    ref = {(n, v): host_flux(ctxs[n].mu, ctxs[n].ga, ctxs[n].n0, host[(n, v)][0, 0]) for n, v in host}
    assert all(np.isfinite(r).all() for r in ref.values()) and len({tuple(r) for r in ref.values()}) == len(ref)
    pool = [(n, v) for n in NS for v in range(2)]
    # the by-value kernel, one job each
    for n, v in pool:
        got = ctxs[n].level_flux(dev[(n, v)]).cpu().numpy()
        assert np.array_equal(got, np.array(ref[(n, v)])), ("by value", n, v)
    # the table kernel at the edges of the workgroup mapping: jobs cycle through the four N, so a workgroup mixes them all
    for count in JOB_COUNTS:
        keys = [pool[(3 * i) % len(pool)] for i in range(count)]
        _check(gpu_pkg, [(ctxs[n], dev[(n, v)]) for n, v in keys], np.array([ref[k] for k in keys]), "count %d" % count)
    # all four N in shuffled and in reverse order; two jobs (one context, and two contexts of one N) share one record
    twin = _contexts(gpu_pkg, (41,))[41]
    try:
        rng = np.random.default_rng(seed + 1)
        keys = [pool[i] for i in rng.permutation(len(pool))] + [(9, 0), (9, 0)]
        for what, ks in (("shuffled", keys), ("reversed", keys[::-1])):
            items = [(ctxs[n], dev[(n, v)]) for n, v in ks] + [(twin, dev[(41, 1)]), (ctxs[41], dev[(41, 1)])]
            _check(gpu_pkg, items, np.array([ref[k] for k in ks] + [ref[(41, 1)]] * 2), what)
    finally:
        twin.close()


@pytest.mark.gpu
def test_kernels_equal_the_host_restatement_bitwise(gpu_pkg):
    """k_level_flux and k_level_flux_table against host_flux, np.array_equal on the doubles: N = 2, 9, 41 and 85, records with
    both signs, zeros and 1e-300; 1, 31, 32, 33, 64 and 65 jobs; one call mixing the four N in shuffled and in reverse order with
    shared records; the 8 NaNs behind d_out untouched.  After close() of the contexts a second round runs on fresh ones, created
    largest first, whose tables reuse the recycled blocks."""
    ctxs = _contexts(gpu_pkg, NS)
    try:
        _round(gpu_pkg, ctxs, 11)
    finally:
        for cx in ctxs.values():
            cx.close()
    ctxs = _contexts(gpu_pkg, NS[::-1])
    try:
        _round(gpu_pkg, ctxs, 23)
    finally:
        for cx in ctxs.values():
            cx.close()


def _count(monkeypatch, pkg):
    """Counting wrappers round the two entry points of the library."""
    n = dict(single=0, spectrum=0, jobs=[])
    L = pkg.capi.lib()
    f1, fn = L.sosgpu_level_flux, L.sosgpu_level_flux_spectrum

    def single(*a):
        n["single"] += 1
        return f1(*a)

    def spectrum(*a):
        n["spectrum"] += 1
        n["jobs"].append(int(a[1]))
        return fn(*a)

    monkeypatch.setattr(L, "sosgpu_level_flux", single)
    monkeypatch.setattr(L, "sosgpu_level_flux_spectrum", spectrum)
    return n


@pytest.mark.gpu
def test_one_call_per_chunk_and_the_flag_off_is_free(gpu_pkg, tmp_path, monkeypatch):
    """sos_spectrum_levels([-1, 0, 3], six calls, fluxes=True): one sosgpu_level_flux_spectrum call of 18 jobs; with chunk=6
    (two wavelengths per chunk at K = 3) one call of 6 jobs per chunk; sos_proc_levels: one call of K jobs for K = 3 and K = 1;
    never a sosgpu_level_flux call.  With fluxes=False there is no call at all, and the 23-tuples equal those of fluxes=True
    array by array; the flux rows do not depend on the chunking and equal those of sos_proc_levels; `timings` has the phase."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=spectrum_cases.RANDOM_CASES[:6])
    kws = [dict(kw, zout=-1.0) for kw in kws]
    alts = [-1, 0.0, 3.0]
    n = _count(monkeypatch, gpu_pkg)
    tm = {}
    got, flux = rs.sos_spectrum_levels(alts, kws, fluxes=True, timings=tm)
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 1, [18]), n
    assert "fluxes" in tm and tm["fluxes"] > 0.0
    assert len(got) == len(flux) == 6 and all(f.shape == (3, 5) and f.dtype == np.float64 for f in flux)
    n.update(spectrum=0, jobs=[])
    got2, flux2 = rs.sos_spectrum_levels(alts, kws, fluxes=True, chunk=6)
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 3, [6, 6, 6]), n
    n.update(spectrum=0, jobs=[])
    got1, flux1 = rs.sos_proc_levels(alts, fluxes=True, **kws[0])
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 1, [3]), n
    n.update(spectrum=0, jobs=[])
    gotk, fluxk = rs.sos_proc_levels([3.0], fluxes=True, **kws[0])
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 1, [1]), n
    n.update(spectrum=0, jobs=[])
    tm = {}
    ref = rs.sos_spectrum_levels(alts, kws, timings=tm)
    ref1 = rs.sos_proc_levels(alts, **kws[0])
    assert (n["single"], n["spectrum"]) == (0, 0), n
    assert tm["fluxes"] == 0.0
    assert isinstance(ref, list) and isinstance(ref1, list) and len(ref) == 6 and len(ref1) == 3
    for i in range(6):
        for k in range(3):
            assert_tuples_equal(got[i][k], ref[i][k])
            assert_tuples_equal(got2[i][k], ref[i][k])
        assert np.array_equal(flux[i], flux2[i])
    for k in range(3):
        assert_tuples_equal(got1[k], ref1[k])
    assert_tuples_equal(gotk[0], ref1[2])
    assert flux1.shape == (3, 5) and np.array_equal(flux1, flux[0]) and np.array_equal(fluxk[0], flux1[2])
    for f in flux:
        assert np.isfinite(f).all()
        assert np.array_equal(f[:, 2], f[:, 1] + f[:, 0]) and np.array_equal(f[:, 4], f[:, 2] - f[:, 3])
        assert (f[:, 0] > 0).all() and (f[:, 0] <= 1).all() and (f[:, 1] >= 0).all() and (f[:, 3] >= 0).all()
        # the direct beam: -1 and 0 km are both the ground (one column depth through two paths, the records' parity bar), then 3 km
        assert abs(f[0, 0] - f[1, 0]) <= 1e-9 * f[0, 0] and f[1, 0] < f[2, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg1_lambert", "ckd_h2o_o2_25bins_flatsea"])
def test_standard_output_row_vs_sos_proc(gpu_pkg, tmp_path, monkeypatch, name):
    """Row 0 of sos_proc_levels([-1, 0, 3], fluxes=True) against sos_proc's own flux_tot_down (element 20) and flux_diff_up
    (element 21), on a Lambert case of one bin and a flat-sea CKD band of 25 bins, within 1e-12 relative.

    The bound is derived: the kernel adds the <= 85 quadrature terms after the aggregate has added the <= 125 bins, the solver
    and the aggregate add in the other order; with every term a product of positive weights and a non-negative intensity the
    relative difference is at most about (85 + 125) 2^-53 = 2.3e-14.  The premise is checked on the record the kernel was
    given (its order-0 intensity row must hold no negative entry) and its smallest entry is printed."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=[name])
    kw = dict(kws[0], zout=-1.0)
    rows = []
    real = gpu_pkg.solver.level_flux_many

    def keep(items):
        rows.extend(rec[0, 0].cpu().numpy() for _, rec in items)
        return real(items)

    monkeypatch.setattr(gpu_pkg.solver, "level_flux_many", keep)
    tuples, flux = rs.sos_proc_levels([-1, 0.0, 3.0], fluxes=True, **kw)
    assert len(rows) == 3 and flux.shape == (3, 5)
    print("%s: smallest order-0 intensity of the standard-output record %.3e" % (name, rows[0].min()))
    assert (rows[0] >= 0.0).all(), "a negative order-0 intensity: the bound's premise does not hold for this case"
    ref = rs.sos_proc(**kw)
    assert_tuples_equal(tuples[0], ref)
    tot, up = float(ref[20]), float(ref[21])
    print("%s: flux_tot_down %.17g vs %.17g, flux_diff_up %.17g vs %.17g" % (name, flux[0, 2], tot, flux[0, 3], up))
    assert tot > 0 and up > 0
    assert abs(flux[0, 2] - tot) <= 1e-12 * tot
    assert abs(flux[0, 3] - up) <= 1e-12 * up
    # altitude 0 km is the ground as well: the same down-going flux as the standard output, from another output slot
    assert abs(flux[1, 2] - tot) <= 1e-9 * tot


@pytest.mark.gpu
def test_interior_altitudes_vs_oracle(gpu_pkg, oracle):
    """One bin at N = 9, NT = 30: E-(z) and E+(z) of solve_levels + aggregate_levels (aik = 1) + level_flux_many at 0, 1, 3 and
    8.5 km against host_flux of the oracle's order-0 records at those altitudes, 1e-9 relative (the parity bar of the records;
    the quadrature of <= 9 positive terms adds no larger error)."""
    alts = [0.0, 1.0, 3.0, 8.5]
    mu, w, n0 = S.gauss_angles(8, 35.0)
    os_nb = 16
    al, be, ga, ze = S.hg_phase(os_nb, 0.6)
    h, x, y, z = S.profile(30, k_abs=0.3)
    h, x, y, ib = S.rescale_profile(h, x, y, 0.0, 0.95, 0.95, os_nb)
    assert len(mu) == 9 and len(h) == 31
    ref = oracle.sos_os_levels(mu, w, os_nb, h, x, y, al, be, ga, ze, alts, n0=n0, zprof=z, ro=0.1, iborm=ib)
    assert ref["ier"] == 0 and ref["records"].shape[0] == len(alts) and ref["records"].shape[1] > 0
    want = np.array([host_flux(mu, w, n0, ref["records"][k, 0, 0]) for k in range(len(alts))])
    cx = gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=ib, ro=0.1)
    try:
        bins = cx.upload_bins(h[None], x[None], y[None], iborm=np.array([ib], dtype=np.int32), zprof=z[None])
        lv = cx.output_levels(bins, alts)
        out = cx.solve_levels(bins, lv)
        rec, _ = cx.aggregate_levels(out, lv, np.ones(1))
        got = gpu_pkg.solver.level_flux_many([(cx, rec[k, 0]) for k in range(len(alts))]).cpu().numpy()
    finally:
        cx.close()
    print("oracle E-/E+ per altitude", want.tolist(), "device", got.tolist())
    assert (want > 0).all()
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), np.abs(got / want - 1).max()
    assert want[0, 1] > want[3, 1] or want[0, 0] > want[3, 0]        # the altitudes really differ
