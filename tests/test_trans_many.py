"""solver.diffuse_transmissions_many / sosgpu_trans_spectrum: the diffuse transmissions of -SOS.Trans (SOS.F:600-635) for every
direction and every bin of many contexts in ONE order-0 solve.  The checker is SosContext.diffuse_transmissions, the loop over
one order-0 context per direction: the new path must give its bits.  Synthetic inputs (synth)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases

S = cases.S
E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _user_angles(mu, w, n0, extra_deg):
    """mu, w, n0 with zero-weight directions inserted (the user angles of SOS_ANGLES), mu staying descending."""
    mus = mu[n0 - 1]
    for t in extra_deg:
        m = np.cos(np.deg2rad(t))
        pos = int(np.sum(mu > m))
        mu, w = np.insert(mu, pos, m), np.insert(w, pos, 0.0)
    return mu, w, int(np.where(mu == mus)[0][0]) + 1


def _angles(kind):
    if kind == "n24_sun_on_node":
        mu, w, _ = S.gauss_angles(24, 35.0)
        w_node = [i for i in range(len(mu)) if w[i] != 0.0][9]
        mu, w, n0 = S.gauss_angles(24, float(np.rad2deg(np.arccos(mu[w_node]))))
        assert len(mu) == 24 and np.all(w != 0.0)
        return mu, w, n0
    if kind == "n27_user":
        mu, w, n0 = _user_angles(*S.gauss_angles(24, 35.0), (12.5, 61.0))
        assert len(mu) == 27 and int(np.sum(w == 0.0)) == 3
        return mu, w, n0
    mu, w, n0 = S.gauss_angles({"n9": 8, "n25": 24, "n41": 40}[kind], 35.0)
    assert len(mu) == int(kind[1:])
    return mu, w, n0


def _context(pkg, kind, os_nb, g=0.6, **kw):
    mu, w, n0 = _angles(kind)
    al, be, ga, ze = S.hg_phase(os_nb, g)
    if kw.pop("matrices", False):
        rng = np.random.default_rng(7)
        kw.update(imat_surf=1, rsurf=(0.02 * rng.random((os_nb + 1, 9, len(mu), len(mu)))).astype(np.float32))
    cx = pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=os_nb, **kw)
    cx.test_phase = (al, be, ga, ze)
    return cx


def _profiles(nb, nt, os_nb, seed=11, tau_a=0.3):
    b = S.ckd_bins(nb, nt, seed=seed, tau_a=tau_a)
    h, x, y, _ = S.rescale_profile(b["h"], b["xdel"], b["ydel"], 0.3 if tau_a else 0.0, 0.95, 0.93, os_nb)
    return h, x, y


def _many(pkg, ctxs, prof, cob=None, nt=None):
    """(tdifmus, tdifmug) host arrays of diffuse_transmissions_many for the concatenated bins `prof` = (h, x, y)."""
    import torch
    bins = ctxs[0].upload_bins(*prof, nt=nt)
    tdifmus, tdifmug = pkg.solver.diffuse_transmissions_many(ctxs, bins, cob)
    torch.cuda.synchronize()
    return tdifmus.cpu().numpy(), tdifmug.cpu().numpy()


def _loop(ctxs, prof, cob=None, nt=None):
    """The same from the per-direction loop of every context, on the rows of its bins."""
    import torch
    h, x, y = prof
    nb = h.shape[0]
    cob = np.zeros(nb, dtype=np.int32) if cob is None else np.asarray(cob)
    tdifmus, tdifmug = np.full(nb, np.nan), np.full((nb, ctxs[0].n), np.nan)
    for c, cx in enumerate(ctxs):
        sel = np.where(cob == c)[0]
        if not len(sel):
            continue
        sub = cx.upload_bins(h[sel], x[sel], y[sel], nt=None if nt is None else np.asarray(nt)[sel])
        s, g = cx.diffuse_transmissions(sub)
        torch.cuda.synchronize()
        tdifmus[sel], tdifmug[sel] = s.cpu().numpy(), g.cpu().numpy()
    return tdifmus, tdifmug


def _same(got, ref):
    assert np.array_equal(got[1], ref[1]), "tdifmug: %d of %d differ, worst %.3e" % (
        int(np.sum(got[1] != ref[1])), ref[1].size, float(np.max(np.abs(got[1] - ref[1]))))
    assert np.array_equal(got[0], ref[0])
    assert np.all(np.isfinite(ref[1]))


# ------------------------------------------------------------------------------------------------------------------ CPU tests


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"\bsize_t\s+sosgpu_trans_spectrum_work_bytes\s*\(sosgpu_ctx \*const \*ctxs, int nctx, int nb, int lp\);", hdr)
    assert re.search(r"\bint\s+sosgpu_trans_spectrum\s*\(sosgpu_ctx \*const \*ctxs, int nctx, const int32_t \*d_ctx_of_bin, int nb, "
                     r"int lp,\s*const int32_t \*d_nt, const double \*d_prof,\s*double \*d_tdifmug /\*\[nb\]\[N\]\*/, void \*d_work, "
                     r"size_t work_bytes, void \*stream\);", hdr)
    for name in ("sosgpu_trans_spectrum", "sosgpu_trans_spectrum_work_bytes"):
        assert name in pkg.capi.EXPORTS
        assert hasattr(pkg.capi.lib(), name)
    assert callable(pkg.solver.diffuse_transmissions_many)


def test_refusals_without_a_context(pkg):
    """What can be refused without a device: NULL ctxs and nctx < 1; the size query answers 0 for them."""
    L = pkg.capi.lib()
    one = (C.c_void_p * 1)(None)
    for hs, nctx in ((None, 1), (one, 0), (one, 1)):
        assert L.sosgpu_trans_spectrum_work_bytes(hs, nctx, 1, 32) == 0
        assert L.sosgpu_trans_spectrum(hs, nctx, None, 1, 32, 8, 8, 8, 8, 1 << 20, None) == E_ARG


# ------------------------------------------------------------------------------------------------------------------ GPU tests

# kind of angles, OS_NB, NT, bins, context keywords, aerosol optical thickness
SHAPES = {
    "n9_nt20": ("n9", 16, 20, 5, {}, 0.3),
    "n25_nt20": ("n25", 48, 20, 5, {}, 0.3),
    "n41_nt20": ("n41", 48, 20, 5, {}, 0.3),
    "n9_nt70_streamed": ("n9", 16, 70, 5, {}, 0.3),
    "n25_nt70_streamed": ("n25", 16, 70, 5, {}, 0.3),
    "n41_nt70_streamed": ("n41", 16, 70, 5, {}, 0.3),
    "n24_sun_on_a_gauss_node": ("n24_sun_on_node", 16, 20, 5, {}, 0.3),
    "n27_two_user_angles": ("n27_user", 16, 20, 5, {}, 0.3),
    "n27_two_user_angles_streamed": ("n27_user", 16, 70, 5, {}, 0.3),
    "no_polarisation": ("n25", 16, 20, 5, dict(ipolar=0), 0.3),
    "molecular": ("n25", 16, 20, 5, {}, 0.0),
    "one_bin": ("n9", 16, 20, 1, {}, 0.3),
    "bins_33": ("n25", 16, 20, 33, {}, 0.3),
    "bins_33_streamed": ("n9", 16, 70, 33, {}, 0.3),
    "parent_fresnel": ("n25", 16, 20, 5, dict(ifresnel=1, ind_surf=1.34, ro=0.1), 0.3),
    "parent_surface_matrices": ("n9", 16, 20, 5, dict(matrices=True, ro=0.05), 0.3),
    "parent_surface_matrices_streamed": ("n9", 16, 70, 5, dict(matrices=True, ro=0.05), 0.3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_context_gives_the_bits_of_the_loop(gpu_pkg, shape):
    kind, os_nb, nt, nb, kw, tau_a = SHAPES[shape]
    cx = _context(gpu_pkg, kind, os_nb, **dict(kw))
    try:
        prof = _profiles(nb, nt, os_nb, tau_a=tau_a)
        if tau_a == 0.0:
            assert not np.any(prof[1])                    # purely molecular: no aerosol share at any level
        _same(_many(gpu_pkg, [cx], prof), _loop([cx], prof))
    finally:
        cx.close()


def _three_contexts(pkg, kind="n25"):
    """Different OS_NB, albedo, polarisation and flags, one N."""
    return [_context(pkg, kind, 16, g=0.6, ro=0.3), _context(pkg, kind, 48, g=0.75, ro=0.0, ifresnel=1),
            _context(pkg, kind, 24, g=0.5, ro=0.1, ipolar=0)]


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 70])
def test_three_contexts_in_one_call(gpu_pkg, nt):
    """ctx_of_bin neither trivial nor sorted: the bins of the three contexts interleaved, 1, 5 and 33 of them."""
    ctxs = _three_contexts(gpu_pkg)
    try:
        cob = np.array([2] + [0] * 20 + [1] * 5 + [0] * 13, dtype=np.int32)
        cob[[3, 30]] = cob[[30, 3]]
        assert [int(np.sum(cob == c)) for c in range(3)] == [33, 5, 1]
        prof = _profiles(len(cob), nt, 16, seed=5)
        _same(_many(gpu_pkg, ctxs, prof, cob), _loop(ctxs, prof, cob))
    finally:
        for cx in ctxs:
            cx.close()


@pytest.mark.gpu
def test_level_grids_of_two_lengths_in_one_call(gpu_pkg):
    """What a spectrum part does with calls of different level grids (solver.concat_profiles): the short rows are padded to the
    longest, so the NT = 20 bins, which the loop of their own context solves with the LDS-resident kernel, ride the streamed
    kernel next to the NT = 70 bins.  They must still get the loop's bits."""
    import torch
    ctxs = _three_contexts(gpu_pkg)
    try:
        profs = [_profiles(5, 20, 16, seed=21), _profiles(3, 70, 16, seed=22), _profiles(2, 20, 16, seed=23)]
        each = [cx.upload_bins(*p) for cx, p in zip(ctxs, profs)]
        assert [b["lp"] <= 64 for b in each] == [True, False, True]
        bins, cob = gpu_pkg.solver.concat_profiles(each)
        assert bins["lp"] == each[1]["lp"] and cob.cpu().tolist() == [0] * 5 + [1] * 3 + [2] * 2
        tdifmus, tdifmug = gpu_pkg.solver.diffuse_transmissions_many(ctxs, bins, cob)
        torch.cuda.synchronize()
        got = (tdifmus.cpu().numpy(), tdifmug.cpu().numpy())
        ref = [_loop([cx], p) for cx, p in zip(ctxs, profs)]
        _same(got, (np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref])))
    finally:
        for cx in ctxs:
            cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 70])
def test_malformed_bin_gets_the_zero_of_the_loop(gpu_pkg, nt):
    cx = _context(gpu_pkg, "n9", 16)
    try:
        prof = _profiles(5, nt, 16)
        nts = np.full(5, nt, dtype=np.int32)
        nts[2] = 0
        got, ref = _many(gpu_pkg, [cx], prof, nt=nts), _loop([cx], prof, nt=nts)
        _same(got, ref)
        assert not np.any(got[1][2]) and np.all(got[1][[0, 1, 3, 4]] > 0.0)
    finally:
        cx.close()


@pytest.mark.gpu
def test_against_the_oracle(gpu_pkg, oracle):
    """The values themselves: oracle.sos_os with every direction as incidence, order 0, black ground, at the tolerance
    test_diffuse_transmissions_vs_oracle uses for this quantity."""
    os_nb = 16
    cx = _context(gpu_pkg, "n9", os_nb, ro=0.2)
    try:
        mu, w, n0 = _angles("n9")
        prof = _profiles(2, 20, os_nb, seed=3)
        tdifmus, tdifmug = _many(gpu_pkg, [cx], prof)
        for b in range(2):
            for j in range(1, len(mu) + 1):
                r = oracle.sos_os(mu, w, os_nb, prof[0][b], prof[1][b], prof[2][b], *cx.test_phase, n0=j, ro=0.0, iborm=0)
                assert abs(tdifmug[b, j - 1] - r["emoins"]) <= 1e-9 * abs(r["emoins"]) + 1e-300, (b, j)
            assert tdifmus[b] == tdifmug[b, n0 - 1]
    finally:
        cx.close()


def _stage_blocks(pkg):
    total, idle = C.c_int(-1), C.c_int(-1)
    assert pkg.capi.lib().sosgpu_debug_stage_blocks(0, C.byref(total), C.byref(idle)) == 0
    return total.value, idle.value


def _raw_call(pkg, own, bins, own_cob=None, **change):
    """sosgpu_trans_spectrum with buffers of its own: returns (code, tdifmug buffer, work buffer, bytes asked for); `change`
    replaces arguments by name."""
    import torch
    L = pkg.capi.lib()
    d = own[0].device
    hs = (C.c_void_p * len(own))(*[None if cx is None else cx._h for cx in own])
    nb, lp, n = bins["nb"], bins["lp"], own[0].n
    need = int(L.sosgpu_trans_spectrum_work_bytes(hs, len(own), nb, lp))
    guard = 64
    work = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=d)
    out = torch.full((nb * n + 8,), -7.0, dtype=torch.float64, device=d)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = dict(ctxs=hs, nctx=len(own), cob=ptr(own_cob), nb=nb, lp=lp, nt=ptr(bins["nt"]), prof=ptr(bins["prof"]), out=ptr(out),
             work=ptr(work), work_bytes=need, stream=C.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    a.update(change)
    code = L.sosgpu_trans_spectrum(a["ctxs"], a["nctx"], a["cob"], a["nb"], a["lp"], a["nt"], a["prof"], a["out"], a["work"],
                                   a["work_bytes"], a["stream"])
    return code, out, work, need


@pytest.mark.gpu
def test_guard_words_staging_and_closed_context(gpu_pkg):
    """Nothing is written behind d_tdifmug or behind the work area; a second call on the recycled staging block gives the same
    bits and makes no new block; closing a context after the call (and creating another in its memory) leaves the queued
    result as it was."""
    import torch
    ctxs = _three_contexts(gpu_pkg, "n9")
    try:
        cob_h = np.array([1, 0, 2, 0, 1, 1, 2], dtype=np.int32)
        prof = _profiles(len(cob_h), 70, 16, seed=9)
        ref = _loop(ctxs, prof, cob_h)
        bins = ctxs[0].upload_bins(*prof)
        cob = gpu_pkg.solver._dev_i32(cob_h, ctxs[0].device)
        n, nb = ctxs[0].n, len(cob_h)
        code, out, work, need = _raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0
        torch.cuda.synchronize()
        first = out.cpu().numpy()
        assert np.array_equal(first[:nb * n].reshape(nb, n), ref[1])
        assert np.all(first[nb * n:] == -7.0)
        assert bool(torch.all(work[need:] == 0xA5))
        blocks = _stage_blocks(gpu_pkg)
        code, out2, work2, _ = _raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0
        # the result is queued: close a context of the call, and let a new one take its memory from the pool
        ctxs[1].close()
        extra = _context(gpu_pkg, "n9", 48, g=0.3)
        torch.cuda.synchronize()
        extra.close()
        assert np.array_equal(out2.cpu().numpy(), first)
        assert bool(torch.all(work2[need:] == 0xA5))
        assert _stage_blocks(gpu_pkg)[0] == blocks[0]
    finally:
        for cx in ctxs:
            cx.close()


@pytest.mark.gpu
def test_refusals_queue_nothing_and_take_no_staging_block(gpu_pkg):
    import torch
    ctxs = _three_contexts(gpu_pkg, "n9")
    other_n = _context(gpu_pkg, "n25", 16)
    unbuilt = gpu_pkg.SosContext(*_angles("n9"), *S.hg_phase(16, 0.6), iborm_max=16, build=False)
    try:
        cob = gpu_pkg.solver._dev_i32(np.array([0, 1, 2, 1], dtype=np.int32), ctxs[0].device)
        bins = ctxs[0].upload_bins(*_profiles(4, 20, 16))
        code, _, _, need = _raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0 and need > 0
        torch.cuda.synchronize()
        work_ptr = lambda w: C.c_void_p(w.data_ptr() + 4)
        refusals = {
            "NULL ctxs": dict(ctxs=None), "NULL d_nt": dict(nt=None), "NULL d_prof": dict(prof=None),
            "NULL d_tdifmug": dict(out=None), "NULL d_work": dict(work=None),
            "nctx < 1": dict(nctx=0), "nb < 0": dict(nb=-1), "lp < 2": dict(lp=1),
            "no ctx_of_bin with three contexts": dict(cob=None),
            "work_bytes too small": None, "misaligned d_work": None,
        }
        before = _stage_blocks(gpu_pkg)
        for what, change in refusals.items():
            if what == "work_bytes too small":
                code = _raw_call(gpu_pkg, ctxs, bins, cob, work_bytes=need - 1)[0]
            elif what == "misaligned d_work":
                spare = torch.zeros(1 << 22, dtype=torch.uint8, device=ctxs[0].device)
                code = _raw_call(gpu_pkg, ctxs, bins, cob, work=work_ptr(spare), work_bytes=(1 << 22) - 4)[0]
            else:
                code = _raw_call(gpu_pkg, ctxs, bins, cob, **change)[0]
            assert code == E_ARG, what
            assert _stage_blocks(gpu_pkg) == before, what
        for what, bad in (("a NULL context", [ctxs[0], None, ctxs[2]]), ("an unbuilt context", [ctxs[0], unbuilt, ctxs[2]]),
                          ("another N", [ctxs[0], other_n, ctxs[2]])):
            hs = (C.c_void_p * 3)(*[None if cx is None else cx._h for cx in bad])
            assert gpu_pkg.capi.lib().sosgpu_trans_spectrum_work_bytes(hs, 3, 4, bins["lp"]) == 0, what
            assert _raw_call(gpu_pkg, ctxs, bins, cob, ctxs=hs, work_bytes=1 << 30)[0] == E_ARG, what
            assert _stage_blocks(gpu_pkg) == before, what
        if torch.cuda.device_count() > 1:
            far = gpu_pkg.SosContext(*_angles("n9"), *S.hg_phase(16, 0.6), iborm_max=16, device=1)
            hs = (C.c_void_p * 3)(ctxs[0]._h, far._h, ctxs[2]._h)
            code = _raw_call(gpu_pkg, ctxs, bins, cob, ctxs=hs, work_bytes=1 << 30)[0]
            far.close()
            assert code == E_ARG and _stage_blocks(gpu_pkg) == before
        # nb = 0: accepted, nothing queued, no block taken
        assert _raw_call(gpu_pkg, ctxs, bins, cob, nb=0)[0] == 0
        assert _stage_blocks(gpu_pkg) == before
        with pytest.raises(RuntimeError, match="build_operators"):
            gpu_pkg.solver.diffuse_transmissions_many([unbuilt], bins)
        with pytest.raises(ValueError, match="ctx_of_bin"):
            gpu_pkg.solver.diffuse_transmissions_many(ctxs, bins)
    finally:
        for cx in ctxs + [other_n, unbuilt]:
            cx.close()
