"""solver.spherical_albedo_many / sosgpu_albedo_spectrum / sosgpu_albedo_band: the spherical albedo of the atmosphere,
S = 2 sum_j ga_j mu_j A_j with A_j the up-going flux of an order-0 solve over a black ground lit from direction j, for every
bin of many contexts in ONE solve.  Seen from the ground (from_below=True) the profile of every item is mirrored in the
vertical; `mirror` below restates that on the host, and the oracle (oracle.sos_os) pins both the definition and the values.
Synthetic inputs (synth), the contexts and profiles of test_trans_many."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases
import test_trans_many as T

S = cases.S
E_ARG = -1
ROOT = T.ROOT
ALBEDOS = (0.1, 0.5, 0.9)
# |E_down(a) (1 - a S) / E_down(0) - 1| of the oracle itself on the bin of test_mirrored_profile_gives_the_coupling_albedo:
# worst 2.521e-8 over the three albedos (the remainder is the stop test of the scattering orders); the bound is 5 times that
IDENTITY_MEASURED = 2.521e-8
IDENTITY_BOUND = 5 * IDENTITY_MEASURED


def mirror(h, x, y, nt=None):
    """The profile seen from the ground, level by level: h'[k] = h[nt] - h[nt-k], xdel'[k] = xdel[nt-k], ydel'[k] =
    ydel[nt-k] for k <= nt and zeros past nt; rows [nb][L], nt[nb] (None: L - 1)."""
    h, x, y = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (h, x, y))
    nb, lmax = h.shape
    nt = np.full(nb, lmax - 1) if nt is None else np.asarray(nt)
    hm, xm, ym = np.zeros_like(h), np.zeros_like(x), np.zeros_like(y)
    for b in range(nb):
        n = int(nt[b])
        for k in range(n + 1):
            hm[b, k] = h[b, n] - h[b, n - k]
            xm[b, k] = x[b, n - k]
            ym[b, k] = y[b, n - k]
    return hm, xm, ym


def gauss_sum(mu, ga, plane):
    """salb of every row of plane[nb][N] in the order of k_albedo_sum: s = s + ((2 ga_j) mu_j) A_j, ascending j."""
    out = np.zeros(plane.shape[0])
    for b in range(plane.shape[0]):
        s = 0.0
        for j in range(len(mu)):
            s = s + ((2.0 * ga[j]) * mu[j]) * plane[b, j]
        out[b] = s
    return out


def oracle_plane(oracle, mu, ga, os_nb, h, x, y, phase, ipolar=1):
    """A_j of one bin from the oracle, 0 where ga_j = 0."""
    return np.array([0.0 if ga[j - 1] == 0.0 else
                     oracle.sos_os(mu, ga, os_nb, h, x, y, *phase, n0=j, ro=0.0, iborm=0, ipolar=ipolar)["eplus"]
                     for j in range(1, len(mu) + 1)])


# ------------------------------------------------------------------------------------------------------------------ CPU tests


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"\bsize_t\s+sosgpu_albedo_spectrum_work_bytes\s*\(sosgpu_ctx \*const \*ctxs, int nctx, int nb, int lp\);", hdr)
    assert re.search(r"\bint\s+sosgpu_albedo_spectrum\s*\(sosgpu_ctx \*const \*ctxs, int nctx, const int32_t \*d_ctx_of_bin, int nb, "
                     r"int lp,\s*const int32_t \*d_nt, const double \*d_prof, int from_below,\s*double \*d_plane /\*\[nb\]\[N\], may "
                     r"be NULL\*/, double \*d_salb /\*\[nb\]\*/,\s*void \*d_work, size_t work_bytes, void \*stream\);", hdr)
    assert re.search(r"\bint\s+sosgpu_albedo_band\s*\(int nseg, const int32_t \*d_seg /\*\[nseg\+1\]\*/, const double \*d_aik, "
                     r"const double \*d_salb,\s*double \*d_out /\*\[nseg\]\*/, int device, void \*stream\);", hdr)
    for name in ("sosgpu_albedo_spectrum", "sosgpu_albedo_spectrum_work_bytes", "sosgpu_albedo_band"):
        assert name in pkg.capi.EXPORTS
        assert hasattr(pkg.capi.lib(), name)
    assert callable(pkg.solver.spherical_albedo_many)


def test_refusals_without_a_context(pkg):
    """What can be refused without a device: NULL ctxs and nctx < 1 (the size query answers 0 for them); a negative segment
    count and NULL pointers of the band sum."""
    L = pkg.capi.lib()
    one = (C.c_void_p * 1)(None)
    for hs, nctx in ((None, 1), (one, 0), (one, 1)):
        assert L.sosgpu_albedo_spectrum_work_bytes(hs, nctx, 1, 32) == 0
        for from_below in (0, 1):
            assert L.sosgpu_albedo_spectrum(hs, nctx, None, 1, 32, 8, 8, from_below, 8, 8, 8, 1 << 20, None) == E_ARG
    assert L.sosgpu_albedo_band(-1, 8, 8, 8, 8, 0, None) == E_ARG
    for hole in range(4):
        ptrs = [8, 8, 8, 8]
        ptrs[hole] = None
        assert L.sosgpu_albedo_band(1, *ptrs, 0, None) == E_ARG
    assert L.sosgpu_albedo_band(0, 8, 8, 8, 8, 0, None) == 0                    # nothing to do, nothing queued


def test_mirrored_profile_gives_the_coupling_albedo(oracle):
    """The definition, without a GPU.  On one N = 9 / NT = 20 aerosol bin the S formed from the oracle's EPLUS on the MIRRORED
    profile satisfies the flux identity of the coupling formula, E_down(a) (1 - a S) = E_down(0) with E_down = EMOINS +
    exp(-h[nt] / mu_s) of the full solve over a Lambert ground of albedo a.  Measured: 2.521e-8 worst over a = 0.1, 0.5, 0.9
    (bound: 5 times that, 1.26e-7).  The same sum on the profile as it stands (S seen from space) misses the identity by
    4.4e-3, so the test tells the two apart."""
    os_nb = 16
    mu, ga, n0 = T._angles("n9")
    phase = S.hg_phase(os_nb, 0.6)
    h, x, y = (a[0] for a in T._profiles(1, 20, os_nb, seed=3))
    hm, xm, ym = (a[0] for a in mirror(h, x, y))
    s_below = gauss_sum(mu, ga, oracle_plane(oracle, mu, ga, os_nb, hm, xm, ym, phase)[None])[0]
    s_above = gauss_sum(mu, ga, oracle_plane(oracle, mu, ga, os_nb, h, x, y, phase)[None])[0]
    direct = np.exp(-h[-1] / mu[n0 - 1])
    e0 = oracle.sos_os(mu, ga, os_nb, h, x, y, *phase, n0=n0, ro=0.0)["emoins"] + direct
    worst, worst_above = 0.0, 0.0
    for a in ALBEDOS:
        ea = oracle.sos_os(mu, ga, os_nb, h, x, y, *phase, n0=n0, ro=a)["emoins"] + direct
        worst = max(worst, abs(ea * (1.0 - a * s_below) / e0 - 1.0))
        worst_above = max(worst_above, abs(ea * (1.0 - a * s_above) / e0 - 1.0))
    print("flux identity: S_below %.12f S_above %.12f worst %.3e (unmirrored %.3e) bound %.3e"
          % (s_below, s_above, worst, worst_above, IDENTITY_BOUND))
    assert 0.0 < s_below < 1.0
    assert worst <= IDENTITY_BOUND
    assert worst_above > 1e3 * IDENTITY_BOUND


# ------------------------------------------------------------------------------------------------------------------ GPU tests


def _salb(pkg, ctxs, prof, cob=None, nt=None, from_below=True):
    """(salb, plane) host arrays of spherical_albedo_many for the concatenated bins `prof` = (h, x, y)."""
    import torch
    bins = ctxs[0].upload_bins(*prof, nt=nt)
    salb, plane = pkg.solver.spherical_albedo_many(ctxs, bins, cob, from_below=from_below)
    torch.cuda.synchronize()
    return salb.cpu().numpy(), plane.cpu().numpy()


def _same(got, ref):
    for g, r, what in zip(got, ref, ("salb", "plane")):
        assert np.array_equal(g, r), "%s: %d of %d differ, worst %.3e" % (what, int(np.sum(g != r)), r.size,
                                                                          float(np.max(np.abs(g - r))))
        assert np.all(np.isfinite(r))


def _weights(cx_kind):
    return T._angles(cx_kind)[1]


# kind of angles, OS_NB, NT, bins, context keywords, aerosol optical thickness
SHAPES = {
    "n9_nt20": ("n9", 16, 20, 5, {}, 0.3),
    "n9_nt70_streamed": ("n9", 16, 70, 5, {}, 0.3),
    "n25_nt20": ("n25", 48, 20, 5, {}, 0.3),
    "n41_nt70_streamed": ("n41", 16, 70, 5, {}, 0.3),
    "n24_sun_on_a_gauss_node": ("n24_sun_on_node", 16, 20, 5, {}, 0.3),
    "n27_two_user_angles": ("n27_user", 16, 20, 5, {}, 0.3),
    "no_polarisation": ("n25", 16, 20, 5, dict(ipolar=0), 0.3),
    "molecular": ("n25", 16, 20, 5, {}, 0.0),
    "one_bin": ("n9", 16, 20, 1, {}, 0.3),
    "bins_33": ("n9", 16, 20, 33, {}, 0.3),
    "bins_33_streamed": ("n9", 16, 70, 33, {}, 0.3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mirror_on_the_device_is_the_mirror_on_the_host(gpu_pkg, shape):
    """from_below=True on P gives the bits of from_below=False on the host mirror of P, salb and plane alike; the columns of
    weight-0 directions are zero, every other plane albedo lies in (0, 1)."""
    kind, os_nb, nt, nb, kw, tau_a = SHAPES[shape]
    cx = T._context(gpu_pkg, kind, os_nb, **dict(kw))
    try:
        prof = T._profiles(nb, nt, os_nb, tau_a=tau_a)
        got = _salb(gpu_pkg, [cx], prof, from_below=True)
        _same(got, _salb(gpu_pkg, [cx], mirror(*prof), from_below=False))
        w = _weights(kind)
        assert got[1].shape == (nb, len(w))
        assert not np.any(got[1][:, w == 0.0])
        assert np.all(got[1][:, w != 0.0] > 0.0) and np.all(got[1][:, w != 0.0] < 1.0)
        assert np.all(got[0] > 0.0) and np.all(got[0] < 1.0)
    finally:
        cx.close()


@pytest.mark.gpu
def test_level_grids_of_two_lengths_in_one_call(gpu_pkg):
    """NT = 20 and NT = 70 bins padded to one lp (solver.concat_profiles): the mirror is about every bin's own nt, not lp."""
    import torch
    ctxs = T._three_contexts(gpu_pkg, "n9")
    try:
        profs = [T._profiles(5, 20, 16, seed=21), T._profiles(3, 70, 16, seed=22), T._profiles(2, 20, 16, seed=23)]
        out = []
        for below, ps in ((True, profs), (False, [mirror(*p) for p in profs])):
            each = [cx.upload_bins(*p) for cx, p in zip(ctxs, ps)]
            bins, cob = gpu_pkg.solver.concat_profiles(each)
            assert bins["lp"] == each[1]["lp"] > each[0]["lp"]
            salb, plane = gpu_pkg.solver.spherical_albedo_many(ctxs, bins, cob, from_below=below)
            torch.cuda.synchronize()
            out.append((salb.cpu().numpy(), plane.cpu().numpy()))
        _same(*out)
        assert np.all(out[0][0] > 0.0)
    finally:
        for cx in ctxs:
            cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 70])
def test_against_the_oracle(gpu_pkg, oracle, nt):
    """The values themselves, for both directions of illumination: plane against the EPLUS of oracle.sos_os with every
    weighted direction as incidence, order 0, black ground (for from_below the oracle gets the mirrored rows), at the 1e-9
    relative of test_trans_many.test_against_the_oracle for the sibling flux; salb is the host loop over the downloaded plane,
    bit for bit."""
    os_nb = 16
    cx = T._context(gpu_pkg, "n9", os_nb, ro=0.2)
    try:
        mu, ga, n0 = T._angles("n9")
        prof = T._profiles(2, nt, os_nb, seed=3)
        for below, rows in ((False, prof), (True, mirror(*prof))):
            salb, plane = _salb(gpu_pkg, [cx], prof, from_below=below)
            for b in range(2):
                ref = oracle_plane(oracle, mu, ga, os_nb, rows[0][b], rows[1][b], rows[2][b], cx.test_phase)
                assert np.all(np.abs(plane[b] - ref) <= 1e-9 * np.abs(ref)), (below, b, np.max(np.abs(plane[b] / ref - 1.0)))
            assert np.array_equal(salb, gauss_sum(mu, ga, plane))
    finally:
        cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 70])
def test_from_below_differs_from_above(gpu_pkg, nt):
    """On aerosol bins the two spherical albedos are more than 1e-3 apart: the mirror cannot silently be dropped."""
    cx = T._context(gpu_pkg, "n9", 16)
    try:
        prof = T._profiles(5, nt, 16)
        below, above = _salb(gpu_pkg, [cx], prof, from_below=True)[0], _salb(gpu_pkg, [cx], prof, from_below=False)[0]
        print("S below", below, "S above", above)
        assert np.all(np.abs(below - above) > 1e-3)
    finally:
        cx.close()


def _context_at(pkg, theta, os_nb, g, **kw):
    """An N = 9 context (8 Gauss nodes and the sun) for the solar zenith angle theta."""
    mu, w, n0 = S.gauss_angles(8, theta)
    assert len(mu) == 9 and w[n0 - 1] == 0.0
    return pkg.SosContext(mu, w, n0, *S.hg_phase(os_nb, g), iborm_max=os_nb, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 70])
def test_three_contexts_in_one_call(gpu_pkg, nt):
    """Interleaved, unsorted ctx_of_bin over contexts of different OS_NB, albedo, flags and SOLAR ANGLES -- the weight-0 column
    sits elsewhere in each -- against the one-context calls, bit for bit."""
    ctxs = [_context_at(gpu_pkg, 35.0, 16, 0.6, ro=0.3), _context_at(gpu_pkg, 62.0, 48, 0.75, ro=0.0, ifresnel=1),
            _context_at(gpu_pkg, 8.0, 24, 0.5, ro=0.1, ipolar=0)]
    try:
        assert len({cx.n0 for cx in ctxs}) == 3
        cob = np.array([2] + [0] * 20 + [1] * 5 + [0] * 13, dtype=np.int32)
        cob[[3, 30]] = cob[[30, 3]]
        assert [int(np.sum(cob == c)) for c in range(3)] == [33, 5, 1]
        prof = T._profiles(len(cob), nt, 16, seed=5)
        salb, plane = _salb(gpu_pkg, ctxs, prof, cob)
        for c, cx in enumerate(ctxs):
            sel = np.where(cob == c)[0]
            _same((salb[sel], plane[sel]), _salb(gpu_pkg, [cx], tuple(a[sel] for a in prof)))
            assert not np.any(plane[sel][:, cx.n0 - 1]) and np.all(np.delete(plane[sel], cx.n0 - 1, axis=1) > 0.0)
    finally:
        for cx in ctxs:
            cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 70])
def test_malformed_bin_gives_zeros_and_leaves_its_neighbours(gpu_pkg, nt):
    cx = T._context(gpu_pkg, "n9", 16)
    try:
        prof = T._profiles(5, nt, 16)
        nts = np.full(5, nt, dtype=np.int32)
        ref = _salb(gpu_pkg, [cx], prof, nt=nts)
        nts[2] = 0
        for below in (True, False):
            got = _salb(gpu_pkg, [cx], prof, nt=nts, from_below=below)
            assert got[0][2] == 0.0 and not np.any(got[1][2])
            if below:
                keep = [0, 1, 3, 4]
                _same((got[0][keep], got[1][keep]), (ref[0][keep], ref[1][keep]))
    finally:
        cx.close()


@pytest.mark.gpu
def test_band_sum(gpu_pkg):
    """sosgpu_albedo_band on segments of 1, 5, 33 and 300 bins (the last beyond one stride of the 256 threads) against the
    left-to-right host sum at 1e-12 relative -- the terms are positive, the tree only reassociates them --; segments of one
    bin bit for bit."""
    import torch
    counts = [1, 5, 33, 300, 1]
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rng = np.random.default_rng(17)
    aik, salb = rng.random(seg[-1]) / 7.0, 0.05 + 0.3 * rng.random(seg[-1])
    dev = torch.device("cuda", 0)
    out = gpu_pkg.solver.albedo_band(seg, gpu_pkg.solver._dev_f64(aik, dev), gpu_pkg.solver._dev_f64(salb, dev))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for g, cnt in enumerate(counts):
        s = 0.0
        for b in range(seg[g], seg[g + 1]):
            s = s + aik[b] * salb[b]
        if cnt == 1:
            assert out[g] == s
        assert abs(out[g] - s) <= 1e-12 * s, (g, out[g], s)


def _raw_call(pkg, own, bins, own_cob=None, from_below=1, with_plane=True, **change):
    """sosgpu_albedo_spectrum with buffers of its own: returns (code, salb buffer, plane buffer, work buffer, bytes asked for);
    `change` replaces arguments by name."""
    import torch
    L = pkg.capi.lib()
    d = own[0].device
    hs = (C.c_void_p * len(own))(*[None if cx is None else cx._h for cx in own])
    nb, lp, n = bins["nb"], bins["lp"], own[0].n
    need = int(L.sosgpu_albedo_spectrum_work_bytes(hs, len(own), nb, lp))
    guard = 64
    work = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=d)
    salb = torch.full((nb + 8,), -7.0, dtype=torch.float64, device=d)
    plane = torch.full((nb * n + 8,), -7.0, dtype=torch.float64, device=d)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = dict(ctxs=hs, nctx=len(own), cob=ptr(own_cob), nb=nb, lp=lp, nt=ptr(bins["nt"]), prof=ptr(bins["prof"]),
             plane=ptr(plane) if with_plane else None, salb=ptr(salb), work=ptr(work), work_bytes=need,
             stream=C.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    a.update(change)
    code = L.sosgpu_albedo_spectrum(a["ctxs"], a["nctx"], a["cob"], a["nb"], a["lp"], a["nt"], a["prof"], from_below, a["plane"],
                                    a["salb"], a["work"], a["work_bytes"], a["stream"])
    return code, salb, plane, work, need


@pytest.mark.gpu
def test_guard_words_staging_and_closed_context(gpu_pkg):
    """Nothing is written behind d_salb, d_plane or the work area; d_plane = NULL is accepted and leaves salb as it was; a
    second call on the recycled staging block gives the same bits and makes no new block; closing a context after the call
    (and creating another in its memory) leaves the queued result as it was."""
    import torch
    ctxs = T._three_contexts(gpu_pkg, "n9")
    try:
        cob_h = np.array([1, 0, 2, 0, 1, 1, 2], dtype=np.int32)
        prof = T._profiles(len(cob_h), 70, 16, seed=9)
        ref = _salb(gpu_pkg, ctxs, prof, cob_h)
        bins = ctxs[0].upload_bins(*prof)
        cob = gpu_pkg.solver._dev_i32(cob_h, ctxs[0].device)
        n, nb = ctxs[0].n, len(cob_h)
        code, salb, plane, work, need = _raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0
        torch.cuda.synchronize()
        s1, p1 = salb.cpu().numpy(), plane.cpu().numpy()
        assert np.array_equal(s1[:nb], ref[0]) and np.array_equal(p1[:nb * n].reshape(nb, n), ref[1])
        assert np.all(s1[nb:] == -7.0) and np.all(p1[nb * n:] == -7.0)
        assert bool(torch.all(work[need:] == 0xA5))
        code, salb0, plane0, work0, _ = _raw_call(gpu_pkg, ctxs, bins, cob, with_plane=False)
        assert code == 0
        torch.cuda.synchronize()
        assert np.array_equal(salb0.cpu().numpy(), s1) and bool(torch.all(plane0 == -7.0)) and bool(torch.all(work0[need:] == 0xA5))
        blocks = T._stage_blocks(gpu_pkg)
        code, salb2, plane2, work2, _ = _raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0
        # the result is queued: close a context of the call, and let a new one take its memory from the pool
        ctxs[1].close()
        extra = T._context(gpu_pkg, "n9", 48, g=0.3)
        torch.cuda.synchronize()
        extra.close()
        assert np.array_equal(salb2.cpu().numpy(), s1) and np.array_equal(plane2.cpu().numpy(), p1)
        assert bool(torch.all(work2[need:] == 0xA5))
        assert T._stage_blocks(gpu_pkg)[0] == blocks[0]
    finally:
        for cx in ctxs:
            cx.close()


@pytest.mark.gpu
def test_refusals_queue_nothing_and_take_no_staging_block(gpu_pkg):
    import torch
    ctxs = T._three_contexts(gpu_pkg, "n9")
    other_n = T._context(gpu_pkg, "n25", 16)
    unbuilt = gpu_pkg.SosContext(*T._angles("n9"), *S.hg_phase(16, 0.6), iborm_max=16, build=False)
    try:
        cob = gpu_pkg.solver._dev_i32(np.array([0, 1, 2, 1], dtype=np.int32), ctxs[0].device)
        bins = ctxs[0].upload_bins(*T._profiles(4, 20, 16))
        code, _, _, _, need = _raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0 and need > 0
        torch.cuda.synchronize()
        work_ptr = lambda w: C.c_void_p(w.data_ptr() + 4)
        refusals = {
            "NULL ctxs": dict(ctxs=None), "NULL d_nt": dict(nt=None), "NULL d_prof": dict(prof=None),
            "NULL d_salb": dict(salb=None), "NULL d_work": dict(work=None),
            "nctx < 1": dict(nctx=0), "nb < 0": dict(nb=-1), "lp < 2": dict(lp=1),
            "no ctx_of_bin with three contexts": dict(cob=None),
            "work_bytes too small": None, "misaligned d_work": None,
        }
        before = T._stage_blocks(gpu_pkg)
        for what, change in refusals.items():
            if what == "work_bytes too small":
                code = _raw_call(gpu_pkg, ctxs, bins, cob, work_bytes=need - 1)[0]
            elif what == "misaligned d_work":
                spare = torch.zeros(1 << 22, dtype=torch.uint8, device=ctxs[0].device)
                code = _raw_call(gpu_pkg, ctxs, bins, cob, work=work_ptr(spare), work_bytes=(1 << 22) - 4)[0]
            else:
                code = _raw_call(gpu_pkg, ctxs, bins, cob, **change)[0]
            assert code == E_ARG, what
            assert T._stage_blocks(gpu_pkg) == before, what
        for what, bad in (("a NULL context", [ctxs[0], None, ctxs[2]]), ("an unbuilt context", [ctxs[0], unbuilt, ctxs[2]]),
                          ("another N", [ctxs[0], other_n, ctxs[2]])):
            hs = (C.c_void_p * 3)(*[None if cx is None else cx._h for cx in bad])
            assert gpu_pkg.capi.lib().sosgpu_albedo_spectrum_work_bytes(hs, 3, 4, bins["lp"]) == 0, what
            assert _raw_call(gpu_pkg, ctxs, bins, cob, ctxs=hs, work_bytes=1 << 30)[0] == E_ARG, what
            assert T._stage_blocks(gpu_pkg) == before, what
        # nb = 0: accepted, nothing queued, no block taken
        code, salb, plane, _, _ = _raw_call(gpu_pkg, ctxs, bins, cob, nb=0)
        torch.cuda.synchronize()
        assert code == 0 and bool(torch.all(salb == -7.0)) and bool(torch.all(plane == -7.0))
        assert T._stage_blocks(gpu_pkg) == before
        with pytest.raises(RuntimeError, match="build_operators"):
            gpu_pkg.solver.spherical_albedo_many([unbuilt], bins)
        with pytest.raises(ValueError, match="ctx_of_bin"):
            gpu_pkg.solver.spherical_albedo_many(ctxs, bins)
    finally:
        for cx in ctxs + [other_n, unbuilt]:
            cx.close()
