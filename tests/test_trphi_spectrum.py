"""The azimuth recompositions of a spectrum part in one launch (sosgpu_trphi_spectrum, solver.trphi_many; the table form
k_trphi_table of csrc/trphi.hip): against SosContext.trphi of every job bit for bit on a batch that mixes every size, flag and
surface term, against the oracle, the refusals of the entry point, and the wiring into run_sos.sos_spectrum /
sos_spectrum_levels / sos_proc_levels (call counts, outputs with and without SOS_SPECTRUM_TRPHI_PER_CALL)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectrum_cases
from spectrum_cases import assert_tuples_equal
from test_surface_matrix import TR_LAND, TR_OS_NB, angles, trphi_azimuths, trphi_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = spectrum_cases.GOLD
E_ARG, E_UNSUPPORTED = -1, -3
GUARD = 1024
TAU = 0.4

# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_symbols_are_declared_exported_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"typedef struct sosgpu_trphi_job \{\s*sosgpu_ctx \*cx;[^}]*const double \*d_rec;[^}]*int32_t nf, igli;[^}]*"
                     r"int32_t phi_off, nphi;[^}]*double tau, tauout, wind;[^}]*const sosgpu_land \*land;[^}]*\} sosgpu_trphi_job;",
                     hdr)
    assert re.search(r"\bsize_t\s+sosgpu_trphi_spectrum_work_bytes\s*\(int njobs\);", hdr)
    assert re.search(r"\bint\s+sosgpu_trphi_spectrum\s*\(const sosgpu_trphi_job \*jobs, int njobs, const double \*d_phi, "
                     r"int nphi_total,\s*double \*d_out, void \*d_work, size_t work_bytes, void \*stream\);", hdr)
    for sym in ("sosgpu_trphi_spectrum", "sosgpu_trphi_spectrum_work_bytes"):
        assert sym in pkg.capi.EXPORTS
        assert hasattr(pkg.capi.lib(), sym)
    names = [f[0] for f in pkg.capi.TrphiJob._fields_]
    assert names == ["cx", "d_rec", "nf", "igli", "phi_off", "nphi", "tau", "tauout", "wind", "land"]
    assert C.sizeof(pkg.capi.TrphiJob) == 2 * 8 + 4 * 4 + 3 * 8 + 8


def test_arguments_are_refused_without_a_device(pkg):
    """NULL jobs, d_phi, d_out and d_work, njobs = -1 and 65536 and a misaligned work area are refused, and njobs = 0 is
    accepted, before any device is looked for."""
    L = pkg.capi.lib()
    jobs = (pkg.capi.TrphiJob * 1)()
    p, nw = C.c_void_p(4096), 1 << 30                        # never dereferenced: nothing is queued by these calls
    assert L.sosgpu_trphi_spectrum(None, 1, p, 1, p, p, nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, 1, None, 1, p, p, nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, 1, p, 1, None, p, nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, 1, p, 1, p, None, nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, -1, p, 1, p, p, nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, 65536, p, 1, p, p, nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, 1, p, 1, p, C.c_void_p(4100), nw, None) == E_ARG
    assert L.sosgpu_trphi_spectrum(jobs, 0, p, 0, p, p, nw, None) == 0


def test_work_bytes(pkg):
    f = pkg.capi.lib().sosgpu_trphi_spectrum_work_bytes
    assert f(0) == 0 and f(-1) == 0
    sizes = [f(n) for n in (0, 1, 2, 3, 100, 65535)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 8 == 0 for s in sizes)


# the contexts of the mixed batch: name -> (N, ipolar, ifresnel); n13 / n13np have the golden's directions
CTX = {"n2": (2, 1, 0), "n13": (13, 1, 1), "n13np": (13, 0, 1), "n42": (42, 0, 0), "n85": (85, 1, 1)}
PHI = {"sun": np.array([0.0]), "one": np.array([-0.7]), "pair": np.array([0.3, 0.3 + np.pi]), "full": trphi_azimuths(361)}
SMAX1 = TR_OS_NB + 1
# (context, record, nf, azimuth list, tauout, igli, wind, land type); the first job has the smallest W, the last the largest
JOBS = [
    ("n2", "r2", 1, "pair", 0.0, 0, 0.0, 0),
    ("n13", "r13", SMAX1, "sun", 0.05, 0, 0.0, 0),            # cos(phi) == 1.0 on a Fresnel context: the sun-glint branch
    ("n13", "r13", SMAX1, "pair", 0.05, 0, 0.0, 0),           # \ one record and one azimuth range,
    ("n13np", "r13", SMAX1, "pair", 0.05, 0, 0.0, 0),         # / two jobs (and two contexts)
    ("n42", "r42", 1, "full", 0.1, 0, 0.0, 3),
    ("n42", "r42", SMAX1, "one", 0.0, 0, 0.0, 4),
    ("n13", "r13", 2, "pair", 0.0, 0, 0.0, 5),
    ("n85", "r85", SMAX1, "pair", 0.3, 0, 0.0, 7),
    ("n2", "r2", SMAX1, "full", 0.05, 1, 2.0, 0),
    ("n42", "r42", 7, "pair", 0.2, 1, 2.0, 0),
    ("n85", "r85", SMAX1, "full", 0.05, 1, 7.0, 0),
]


def test_batch_covers_the_mix_it_claims():
    ws = [2 * CTX[j[0]][0] + 1 for j in JOBS]
    assert ws[0] == min(ws) == 5 and ws[-1] == max(ws) == 171 and {27, 85} <= set(ws)
    assert {c[1] for c in CTX.values()} == {0, 1} and {c[2] for c in CTX.values()} == {0, 1}
    assert {1, SMAX1} <= {j[2] for j in JOBS}
    assert {len(PHI[j[3]]) for j in JOBS} == {1, 2, 361}
    assert JOBS[2][1:4] == JOBS[3][1:4]
    assert {(j[5], j[6]) for j in JOBS if j[5]} == {(1, 2.0), (1, 7.0)}
    assert {j[7] for j in JOBS} == {0, 3, 4, 5, 7}
    assert any(j[4] == 0.0 for j in JOBS) and any(0.0 < j[4] < TAU for j in JOBS)
    assert any(CTX[j[0]][2] == 1 and np.any(np.cos(PHI[j[3]]) == 1.0) for j in JOBS)
    assert np.cos(PHI["sun"][0]) == 1.0 and abs(PHI["pair"][1] - PHI["pair"][0] - np.pi) < 1e-15


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _golden():
    return np.load(os.path.join(GOLD, "trphi_n13.npz"))


def _context(gpu_pkg, mu, w, n0, ipolar, ifresnel):
    al, be, ga, ze = gpu_pkg.synth.hg_phase(TR_OS_NB, 0.6)
    return gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, ifresnel=ifresnel, ipolar=ipolar, ind_surf=1.34)


def _land(gpu_pkg, isurf):
    if not isurf:
        return None
    return gpu_pkg.surface.land_model(isurf, TR_LAND["k0"], TR_LAND["k1"], TR_LAND["k2"], coef_c=TR_LAND["coef_c"])


def _spectrum_call(gpu_pkg, items, work_offset=0, mutate=None, nphi_total=None):
    """One sosgpu_trphi_spectrum call made by hand for items (ctx, rec, nf, tau, tauout, phis, igli, wind, land): every
    distinct azimuth list uploaded once, the output followed by a guard of NaNs.  mutate(jobs) may spoil the job array.
    Returns (return code, blocks [nphi][7][W] or None, guard)."""
    import torch
    L, cap = gpu_pkg.capi.lib(), gpu_pkg.capi
    lists, total = {}, 0
    for it in items:
        key = np.asarray(it[5], dtype=np.float64).tobytes()
        if key not in lists:
            lists[key] = total
            total += len(it[5])
    phis = torch.from_numpy(np.concatenate([np.frombuffer(k, dtype=np.float64) for k in lists])).cuda()
    jobs = (cap.TrphiJob * len(items))()
    shapes = []
    for j, (cx, rec, nf, tau, tauout, ph, igli, wind, land) in zip(jobs, items):
        j.cx, j.d_rec, j.nf, j.igli = cx._h.value, rec.data_ptr(), nf, igli
        j.phi_off, j.nphi = lists[np.asarray(ph, dtype=np.float64).tobytes()], len(ph)
        j.tau, j.tauout, j.wind = tau, tauout, wind
        if land is not None:
            j.land = C.pointer(land)
        shapes.append((len(ph), 7, cx.w))
    if mutate:
        mutate(jobs)
    count = sum(a * b * c for a, b, c in shapes)
    out = torch.full((count + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    nw = int(L.sosgpu_trphi_spectrum_work_bytes(len(items)))
    work = torch.empty(nw + 8, dtype=torch.uint8, device="cuda")
    rc = L.sosgpu_trphi_spectrum(jobs, len(items), C.c_void_p(phis.data_ptr()), total if nphi_total is None else nphi_total,
                                 C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr() + work_offset), nw,
                                 items[0][0]._stream())
    torch.cuda.synchronize()
    if rc:
        return rc, None, out[count:]
    blocks, pos = [], 0
    for shp in shapes:
        m = shp[0] * shp[1] * shp[2]
        blocks.append(out[pos:pos + m].view(shp))
        pos += m
    return rc, blocks, out[count:]


@pytest.fixture(scope="module")
def mixed(gpu_pkg):
    """The contexts, records, items and per-job references (SosContext.trphi) of JOBS, made once."""
    import torch
    g = _golden()
    ctxs = {}
    for name, (n, ipolar, ifresnel) in CTX.items():
        if n == 13:
            mu, w, n0 = g["mu"], gpu_pkg.synth.gauss_angles(12, 35.0)[1], int(g["n0"])
        else:
            mu, w, n0 = angles(n, 35.0)
        ctxs[name] = _context(gpu_pkg, mu, w, n0, ipolar, ifresnel)
    recs = {"r%d" % n: torch.from_numpy(trphi_records(n, 1.0, 2000 + n)).cuda() for n in (2, 13, 42, 85)}
    items = [(ctxs[c], recs[r], nf, TAU, tauout, PHI[p], igli, wind, _land(gpu_pkg, isurf))
             for c, r, nf, p, tauout, igli, wind, isurf in JOBS]
    refs = [cx.trphi(rec, nf, tau, tauout, ph, igli=igli, wind=wind, land=land).clone()
            for cx, rec, nf, tau, tauout, ph, igli, wind, land in items]
    torch.cuda.synchronize()
    yield dict(items=items, refs=refs)
    for cx in ctxs.values():
        cx.close()


def _assert_blocks(blocks, refs, what):
    import torch
    assert len(blocks) == len(refs)
    for k, (b, r) in enumerate(zip(blocks, refs)):
        assert b.shape == r.shape and not torch.isnan(b).any(), (what, k)
        assert torch.equal(b, r), (what, k, int((b != r).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["smallest first", "largest first"])
def test_one_call_equals_the_single_calls_bitwise(gpu_pkg, mixed, order):
    """One sosgpu_trphi_spectrum call over JOBS -- W 5, 27, 85 and 171, IPOLAR 0 and 1, Fresnel or not, nf 1 and smax + 1,
    azimuth lists of 1, 2 and 361, a shared record and azimuth range, the glint at two winds, the four land models, tauout 0
    and inside the layer, the sun-glint azimuth -- gives block by block the bits of SosContext.trphi of each job; in both
    orders (the smallest-W job first and the largest-W job last, and the reverse); the guard behind the last block is
    untouched.  solver.trphi_many gives the same views."""
    import torch
    sel = slice(None) if order == "smallest first" else slice(None, None, -1)
    items, refs = mixed["items"][sel], mixed["refs"][sel]
    rc, blocks, guard = _spectrum_call(gpu_pkg, items)
    assert rc == 0
    _assert_blocks(blocks, refs, order)
    assert guard.numel() == GUARD and bool(torch.isnan(guard).all())
    flat, views = gpu_pkg.solver.trphi_many(items)
    _assert_blocks(views, refs, order + ", trphi_many")
    assert flat.numel() == sum(r.numel() for r in refs) and flat.data_ptr() == views[0].data_ptr()


@pytest.mark.gpu
def test_one_call_vs_oracle(gpu_pkg, oracle):
    """The four cases of tests/golden/trphi_n13.npz and one land job per type on the golden's directions and records, in one
    call: rows 0..3 against oracle.trphi / oracle.trphi_land at the tolerance of test_trphi_gpu_vs_oracle
    (1e-9 |ref| + 1e-12 max(1, max |ref|)), rows 4..6 against oracle.polar of the rows 0..2 at that test's tolerances."""
    import torch
    g = _golden()
    mu, n0, rec, phis = g["mu"], int(g["n0"]), g["rec"], g["phis"]
    w = gpu_pkg.synth.gauss_angles(12, 35.0)[1]
    d_rec = torch.from_numpy(rec).cuda()
    nf = rec.shape[0]
    cases = [dict(igli=int(g["igli%d" % i]), wind=float(g["wind%d" % i]), ifresnel=int(g["ifresnel%d" % i]),
                  ipolar=int(g["ipolar%d" % i]), isurf=0) for i in range(int(g["ncases"]))]
    cases += [dict(igli=0, wind=0.0, ifresnel=0, ipolar=1, isurf=s) for s in (3, 4, 5, 7)]
    ctxs = []
    try:
        ctxs = [_context(gpu_pkg, mu, w, n0, c["ipolar"], c["ifresnel"]) for c in cases]
        items = [(cx, d_rec, nf, 0.4, 0.05, phis, c["igli"], c["wind"], _land(gpu_pkg, c["isurf"])) for cx, c in zip(ctxs, cases)]
        rc, blocks, _ = _spectrum_call(gpu_pkg, items)
        assert rc == 0
        outs = [b.cpu().numpy() for b in blocks]
    finally:
        for cx in ctxs:
            cx.close()
    n = len(mu)
    for i, (c, out) in enumerate(zip(cases, outs)):
        kw = dict(igli=c["igli"], n0=n0, wind=c["wind"], ifresnel=c["ifresnel"], ipolar=c["ipolar"])
        for k, phi in enumerate(phis):
            if c["isurf"]:
                ref = oracle.trphi_land(mu, rec, 0.4, 0.05, float(phi), isurf=c["isurf"], ind_surf=1.34, **TR_LAND, **kw)["out"]
            else:
                ref = oracle.trphi(mu, rec, 0.4, 0.05, float(phi), **kw)
            for q in range(4):
                tol = 1e-9 * np.abs(ref[q]) + 1e-12 * max(1.0, np.abs(ref[q]).max())
                assert np.all(np.abs(out[k, q] - ref[q]) <= tol), (i, k, q, np.abs(out[k, q] - ref[q]).max())
            for jj in list(range(0, n)) + list(range(n + 1, 2 * n + 1)):
                xan, tpol, lpol = oracle.polar(out[k, 0, jj], out[k, 1, jj], out[k, 2, jj])
                assert abs(out[k, 4, jj] - xan) <= 1e-9 * max(1.0, abs(xan))
                assert abs(out[k, 5, jj] - tpol) <= 1e-9 * max(1.0, abs(tpol))
                assert abs(out[k, 6, jj] - lpol) <= 1e-12 + 1e-9 * abs(lpol)


@pytest.mark.gpu
def test_refusals_change_nothing(gpu_pkg, mixed):
    """nf = smax + 2, an azimuth range past nphi_total, a NULL context inside the list and a misaligned work area give
    SOSGPU_E_ARG, land type 6 SOSGPU_E_UNSUPPORTED; the guard-filled output of a refused call is untouched and a valid call
    that follows gives the right bits."""
    import torch
    items, refs = mixed["items"][:4], mixed["refs"][:4]
    nadal = gpu_pkg.capi.Land(isurf=6)

    def nf_too_large(jobs):
        jobs[2].nf = SMAX1 + 1

    def null_context(jobs):
        jobs[1].cx = None

    def land_six(jobs):
        jobs[3].land = C.pointer(nadal)

    total = sum(len(PHI[k]) for k in ("pair", "sun"))
    for what, kw, code in (("nf", dict(mutate=nf_too_large), E_ARG), ("range", dict(nphi_total=total - 1), E_ARG),
                           ("context", dict(mutate=null_context), E_ARG), ("work", dict(work_offset=4), E_ARG),
                           ("nadal", dict(mutate=land_six), E_UNSUPPORTED)):
        rc, _, guard = _spectrum_call(gpu_pkg, items, **kw)
        assert rc == code, what
        assert bool(torch.isnan(guard).all())
        rc, blocks, _ = _spectrum_call(gpu_pkg, items)
        assert rc == 0
        _assert_blocks(blocks, refs, "after " + what)


def _count(monkeypatch, pkg):
    """Counting wrappers round the two entry points of the library."""
    n = dict(single=0, spectrum=0, jobs=[])
    L = pkg.capi.lib()
    f1, fn = L.sosgpu_trphi, L.sosgpu_trphi_spectrum

    def single(*a):
        n["single"] += 1
        return f1(*a)

    def spectrum(*a):
        n["spectrum"] += 1
        n["jobs"].append(int(a[1]))
        return fn(*a)

    monkeypatch.setattr(L, "sosgpu_trphi", single)
    monkeypatch.setattr(L, "sosgpu_trphi_spectrum", spectrum)
    return n


@pytest.mark.gpu
def test_spectrum_pass_makes_one_call_per_chunk(gpu_pkg, tmp_path, monkeypatch):
    """sos_spectrum over the call list of spectrum_cases: one sosgpu_trphi_spectrum call per chunk (one chunk, and chunk=24:
    one per 24 calls) and no sosgpu_trphi call; with SOS_SPECTRUM_TRPHI_PER_CALL=1 one sosgpu_trphi call per wavelength and none of the
    other; all 23 outputs of every call are equal in the two runs."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_TRPHI_PER_CALL", raising=False)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path)
    n = _count(monkeypatch, gpu_pkg)
    got = rs.sos_spectrum(kws)
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 1, [len(kws)]), n
    n.update(spectrum=0, jobs=[])
    rs.sos_spectrum(kws, chunk=24)
    chunks = [len(kws[c:c + 24]) for c in range(0, len(kws), 24)]
    assert len(chunks) > 1 and (n["single"], n["spectrum"], n["jobs"]) == (0, len(chunks), chunks), n
    n.update(spectrum=0, jobs=[])
    monkeypatch.setenv("SOS_SPECTRUM_TRPHI_PER_CALL", "1")
    ref = rs.sos_spectrum(kws)
    assert (n["single"], n["spectrum"]) == (len(kws), 0), n
    assert len(got) == len(ref) == len(kws)
    for a, b in zip(got, ref):
        assert_tuples_equal(a, b)


@pytest.mark.gpu
def test_levels_make_one_call(gpu_pkg, tmp_path, monkeypatch):
    """sos_spectrum_levels([-1, 0, 3]) of the first six calls: one sosgpu_trphi_spectrum call of 18 jobs, no sosgpu_trphi call;
    sos_proc_levels of one call: one call of 3 jobs; the outputs equal those under SOS_SPECTRUM_TRPHI_PER_CALL=1, which makes
    one sosgpu_trphi call per wavelength and altitude and none of the other."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_TRPHI_PER_CALL", raising=False)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path)
    kws = [dict(kw, zout=-1.0) for kw in kws[:6]]
    alts = [-1, 0.0, 3.0]
    n = _count(monkeypatch, gpu_pkg)
    got = rs.sos_spectrum_levels(alts, kws)
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 1, [18]), n
    n.update(spectrum=0, jobs=[])
    got1 = rs.sos_proc_levels(alts, **kws[0])
    assert (n["single"], n["spectrum"], n["jobs"]) == (0, 1, [3]), n
    n.update(spectrum=0, jobs=[])
    monkeypatch.setenv("SOS_SPECTRUM_TRPHI_PER_CALL", "1")
    ref = rs.sos_spectrum_levels(alts, kws)
    assert (n["single"], n["spectrum"]) == (18, 0), n
    ref1 = rs.sos_proc_levels(alts, **kws[0])
    assert (n["single"], n["spectrum"]) == (21, 0), n
    assert len(got) == len(ref) == 6 and len(got1) == len(ref1) == 3
    for a, b in zip(got, ref):
        for k in range(3):
            assert_tuples_equal(a[k], b[k])
    for k in range(3):
        assert_tuples_equal(got1[k], ref1[k])
