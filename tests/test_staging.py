"""The pinned staging path of the table-form entry points (the Staged blocks of csrc/api_mem.hip, counted by
sosgpu_debug_stage_blocks): the number of blocks stays bounded on a living context, a block is not reused before its copy has
passed on a backlogged stream, no context owns a block, a refused call takes none, and sosgpu_trim frees the idle ones."""
import ctypes as C

import numpy as np
import pytest

import cases
from test_surface_matrix import trphi_records

S = cases.S
E_ARG = -1
N = 9                                         # directions of every context here (W = 19); nothing depends on the size
OS_NB = 8
NF = 2                                        # Fourier orders of the azimuth jobs
PHIS = np.array([0.3, 0.3 + np.pi])
TAU, TAUOUT = 0.4, 0.05


def _context(gpu_pkg, sun=35.0):
    mu, w, n0 = S.gauss_angles(N - 1, sun)
    assert len(mu) == N
    al, be, ga, ze = S.hg_phase(OS_NB, 0.6)
    return gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze)


def _record(seed):
    import torch
    return torch.from_numpy(trphi_records(N, 1.0, seed)).cuda()


def _blocks(gpu_pkg):
    """(total, idle) of device 0."""
    total, idle = C.c_int(-1), C.c_int(-1)
    assert gpu_pkg.capi.lib().sosgpu_debug_stage_blocks(0, C.byref(total), C.byref(idle)) == 0
    assert 0 <= idle.value <= total.value
    return total.value, idle.value


def _trphi_item(cx, rec, tau=TAU):
    return (cx, rec, NF, tau, TAUOUT, PHIS, 0, 0.0, None)


def _trphi_single(item):
    cx, rec, nf, tau, tauout, phis, igli, wind, land = item
    return cx.trphi(rec, nf, tau, tauout, phis, igli=igli, wind=wind, land=land)


def _trphi_args(gpu_pkg, items, phis):
    """What one sosgpu_trphi_spectrum call of `items` needs, made beforehand: (jobs, out, work); every job reads `phis`."""
    import torch
    L, cap = gpu_pkg.capi.lib(), gpu_pkg.capi
    jobs = (cap.TrphiJob * len(items))()
    for j, (cx, rec, nf, tau, tauout, ph, igli, wind, _) in zip(jobs, items):
        j.cx, j.d_rec, j.nf, j.igli, j.phi_off, j.nphi = cx._h.value, rec.data_ptr(), nf, igli, 0, len(ph)
        j.tau, j.tauout, j.wind = tau, tauout, wind
    out = torch.full((len(items), len(PHIS), 7, 2 * N + 1), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(int(L.sosgpu_trphi_spectrum_work_bytes(len(items))), dtype=torch.uint8, device="cuda")
    return jobs, out, work


def _trphi_call(gpu_pkg, items, phis, args):
    jobs, out, work = args
    return gpu_pkg.capi.lib().sosgpu_trphi_spectrum(jobs, len(items), C.c_void_p(phis.data_ptr()), int(phis.numel()),
                                                    C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), work.numel(),
                                                    items[0][0]._stream())


def _flux_args(gpu_pkg, items):
    import torch
    L, cap = gpu_pkg.capi.lib(), gpu_pkg.capi
    jobs = (cap.FluxJob * len(items))()
    for j, (cx, rec) in zip(jobs, items):
        j.cx, j.d_rec = cx._h.value, rec.data_ptr()           # (the order-0 intensity row is the record's first)
    out = torch.full((len(items), 2), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(int(L.sosgpu_level_flux_spectrum_work_bytes(len(items))), dtype=torch.uint8, device="cuda")
    return jobs, out, work


def _flux_call(gpu_pkg, items, args):
    jobs, out, work = args
    return gpu_pkg.capi.lib().sosgpu_level_flux_spectrum(jobs, len(items), C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()),
                                                         work.numel(), items[0][0]._stream())


@pytest.fixture()
def ctxs(gpu_pkg):
    """Three built contexts of N = 9 with different suns, on an idle device."""
    import torch
    made = [_context(gpu_pkg, sun) for sun in (35.0, 20.0, 50.0)]
    torch.cuda.synchronize()
    yield made
    for cx in made:
        cx.close()


@pytest.mark.gpu
def test_blocks_stay_bounded_on_a_living_context(gpu_pkg, ctxs):
    """50 rounds of ContextTable, level_flux_many of two jobs and trphi_many of two jobs on the same living contexts, each call
    followed by a stream synchronise: the library holds as many blocks after round 50 as after round 1."""
    import torch
    sv = gpu_pkg.solver
    recs = [_record(1), _record(2)]
    flux_items = [(ctxs[0], recs[0]), (ctxs[1], recs[1])]
    trphi_items = [_trphi_item(ctxs[0], recs[0]), _trphi_item(ctxs[1], recs[1])]
    st = torch.cuda.current_stream()
    after = []
    for _ in range(50):
        table = sv.ContextTable(ctxs)
        st.synchronize()
        flux = sv.level_flux_many(flux_items)
        st.synchronize()
        flat, views = sv.trphi_many(trphi_items)
        st.synchronize()
        after.append(_blocks(gpu_pkg)[0])
    assert table.table.numel() > 0 and flux.shape == (2, 2) and len(views) == 2
    assert after[0] >= 1
    assert after[49] == after[0], after


@pytest.mark.gpu
def test_backlogged_stream_reuses_no_block_early(gpu_pkg, ctxs):
    """Behind a device-side delay, 16 sosgpu_level_flux_spectrum calls (16 records) and 16 sosgpu_trphi_spectrum calls (16
    optical depths) of one job each are queued without a synchronise: at least two blocks are then not reusable, and every
    result equals that of sosgpu_level_flux / sosgpu_trphi bit for bit."""
    import torch
    cx = ctxs[0]
    recs = [_record(100 + k) for k in range(16)]
    phis = torch.from_numpy(PHIS).cuda()
    flux_items = [[(cx, recs[k])] for k in range(16)]
    trphi_items = [[_trphi_item(ctxs[k % 3], recs[0], tau=0.1 + 0.02 * k)] for k in range(16)]
    flux_args = [_flux_args(gpu_pkg, it) for it in flux_items]
    trphi_args = [_trphi_args(gpu_pkg, it, phis) for it in trphi_items]
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)             # some tens of milliseconds; the length does not matter
    rcs = [_flux_call(gpu_pkg, it, a) for it, a in zip(flux_items, flux_args)]
    rcs += [_trphi_call(gpu_pkg, it, phis, a) for it, a in zip(trphi_items, trphi_args)]
    total, idle = _blocks(gpu_pkg)
    torch.cuda.synchronize()
    assert rcs == [0] * 32
    print("blocks behind the backlog: total %d, idle %d" % (total, idle))
    assert total - idle >= 2, "no backlog formed: the test would prove nothing"
    assert _blocks(gpu_pkg) == (total, total)
    for k in range(16):
        assert torch.equal(flux_args[k][1][0], cx.level_flux(recs[k])), ("flux", k)
        assert torch.equal(trphi_args[k][1][0], _trphi_single(trphi_items[k][0])), ("trphi", k)


@pytest.mark.gpu
def test_no_context_owns_a_block(gpu_pkg):
    """One sosgpu_trphi_spectrum call of three jobs on three contexts; the first context is closed at once.  The other two
    jobs equal their per-call results bit for bit and the close frees no block."""
    import torch
    made = [_context(gpu_pkg, sun) for sun in (35.0, 20.0, 50.0)]
    try:
        recs = [_record(200 + k) for k in range(3)]
        phis = torch.from_numpy(PHIS).cuda()
        items = [_trphi_item(cx, rec) for cx, rec in zip(made, recs)]
        args = _trphi_args(gpu_pkg, items, phis)
        torch.cuda.synchronize()
        assert _trphi_call(gpu_pkg, items, phis, args) == 0
        before = _blocks(gpu_pkg)[0]
        made[0].close()
        assert _blocks(gpu_pkg)[0] == before >= 1
        torch.cuda.synchronize()
        for k in (1, 2):
            assert torch.equal(args[1][k], _trphi_single(items[k])), k
    finally:
        for cx in made:
            cx.close()


@pytest.mark.gpu
def test_refusals_take_nothing(gpu_pkg, ctxs):
    """A refused call of each of sosgpu_ctx_table (contexts of two N), sosgpu_noyaux_spectrum (a NULL context in the list),
    sosgpu_trphi_spectrum (nf = smax + 2) and sosgpu_level_flux_spectrum (a NULL record) leaves total and idle as they were."""
    import torch
    L = gpu_pkg.capi.lib()
    mu, w, n0 = S.gauss_angles(4, 35.0)
    other = gpu_pkg.SosContext(mu, w, n0, *S.hg_phase(OS_NB, 0.6))
    try:
        rec = _record(300)
        phis = torch.from_numpy(PHIS).cuda()
        work = torch.empty(4 * (int(L.sosgpu_ctx_table_entry_bytes()) + 8), dtype=torch.uint8, device="cuda")
        wp, st = C.c_void_p(work.data_ptr()), ctxs[0]._stream()
        t_items = [_trphi_item(ctxs[0], rec), _trphi_item(ctxs[1], rec)]
        t_args = _trphi_args(gpu_pkg, t_items, phis)
        t_args[0][1].nf = OS_NB + 2
        f_items = [(ctxs[0], rec), (ctxs[1], rec)]
        f_args = _flux_args(gpu_pkg, f_items)
        f_args[0][1].d_rec = None
        gpu_pkg.solver.level_flux_many(f_items)               # (so that there is a block a refused call could take)
        torch.cuda.synchronize()
        before = _blocks(gpu_pkg)
        assert before[0] >= 1
        refused = {
            "sosgpu_ctx_table": lambda: L.sosgpu_ctx_table((C.c_void_p * 2)(ctxs[0]._h, other._h), 2, wp, st),
            "sosgpu_noyaux_spectrum": lambda: L.sosgpu_noyaux_spectrum((C.c_void_p * 2)(ctxs[0]._h, None), 2, None, wp,
                                                                       work.numel(), st),
            "sosgpu_trphi_spectrum": lambda: _trphi_call(gpu_pkg, t_items, phis, t_args),
            "sosgpu_level_flux_spectrum": lambda: _flux_call(gpu_pkg, f_items, f_args),
        }
        for name, call in refused.items():
            assert call() == E_ARG, name
            assert _blocks(gpu_pkg) == before, name
    finally:
        other.close()


@pytest.mark.gpu
def test_trim_frees_the_idle_blocks(gpu_pkg, ctxs):
    """After a synchronise sosgpu_trim leaves no block; the next level_flux_many call succeeds, on one new block."""
    import torch
    rec = _record(400)
    items = [(ctxs[0], rec), (ctxs[1], rec)]
    gpu_pkg.solver.level_flux_many(items)
    torch.cuda.synchronize()
    assert _blocks(gpu_pkg)[0] >= 1
    gpu_pkg.solver.release_scratch()
    assert _blocks(gpu_pkg) == (0, 0)
    got = gpu_pkg.solver.level_flux_many(items)
    torch.cuda.synchronize()
    assert _blocks(gpu_pkg) == (1, 1)
    for k, (cx, r) in enumerate(items):
        assert torch.equal(got[k], cx.level_flux(r)), k
