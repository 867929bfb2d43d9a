"""The irradiance-only spectrum pass on the device.

Kernel (sosgpu_level_irradiance, k_level_irradiance of csrc/irradiance.hip) on synthetic records, by the method of
test_level_absorption's test C: every column against the kernel whose statements it executes, run on the same inputs --
sosgpu_level_absorption, sosgpu_aggregate's scalar block (with sosgpu_level_transmission's element) and sosgpu_level_flux of the
aggregated record.  Equal bits everywhere except the two flux sums of a segment of several bins, which add aik * E(bin) where
the chain takes E(sum aik * bin): all terms non-negative, at most nbins + 2 N roundings apart, bar 1e-12.

End to end (run_sos.sos_spectrum_irradiances): the reference is sos_spectrum_levels(..., fluxes=True, split=True,
absorption=True), code the pass does not touch."""
import ctypes as C
import math

import numpy as np
import pytest

import cases
import spectrum_cases
import test_level_absorption as tla
import test_level_conservation as tlc
from test_level_flux import GOLD

S = cases.S
E_ARG = -1
GUARD = 8
SEG_SIZES = tla.SEG_SIZES
LP, NZ, NT = 40, 3, 33
COLS = 14                                                                  # SOSGPU_IRRADIANCE_COLS
BAR = 1e-12


def _synthetic(ng, sun, seed, s1):
    """Records and profiles made here for the segments of SEG_SIZES: slot 0 interior levels, slot 1 the standard output
    (jout = 0), slot 2 other levels.  One failed bin inside every segment of two or more, one bin with jout = NT + 1 in slots 0, 2,
    every fifth bin with two coinciding altitudes; the one-bin segment has aik = 1."""
    rng = np.random.default_rng(seed)
    mu, ga, n0 = S.gauss_angles(ng, sun)
    n = len(mu)
    w = 2 * n + 1
    seg = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)
    nb = int(seg[-1])
    h = np.cumsum(rng.uniform(0.01, 0.1, (nb, LP)), axis=1)
    prof = np.stack([h, rng.uniform(0.05, 0.45, (nb, LP)), rng.uniform(0.05, 0.45, (nb, LP))], axis=1)
    zprof = np.round(120.0 - np.cumsum(rng.uniform(0.5, 3.0, (nb, LP)), axis=1), 5)
    zprof[:, 0] = 120.0
    flat_bins = np.arange(nb) % 5 == 1
    zprof[flat_bins, 4] = zprof[flat_bins, 3]
    nt = np.full(nb, NT, dtype=np.int32)
    jout = np.stack([rng.integers(1, NT + 1, nb), np.zeros(nb, dtype=np.int64), rng.integers(1, NT + 1, nb)]).astype(np.int32)
    jout[0, flat_bins] = 4
    zz = rng.uniform(0.0, 1.0, (NZ, nb))
    tauout = rng.uniform(0.0, 2.0, (NZ, nb))
    tauvrai = tauout * rng.uniform(1.0, 1.3, (NZ, nb))
    rec = np.zeros((NZ, nb, s1, 3, w))
    rec[:, :, 0, 0, :] = rng.uniform(0.0, 1.0, (NZ, nb, w)) * 10.0 ** rng.integers(-6, 1, (NZ, nb, w))
    rec[:, :, 1:] = 7.0                                                     # (orders above 0: never read)
    norders = np.full(nb, 1, dtype=np.int32)
    failed = [int(seg[g] + (seg[g + 1] - seg[g]) // 2) for g in range(1, len(SEG_SIZES))]
    norders[failed] = -1
    beyond = int(seg[3]) + 7
    jout[[0, 2], beyond] = NT + 1                                           # (both interior slots: _run's flux reference drops the bin)
    aik = rng.uniform(0.1, 1.0, nb)
    aik[0] = 1.0
    flux = rng.uniform(0.05, 0.9, (nb, 2))
    scal = np.stack([rng.uniform(0.0, 0.5, nb), h[:, NT], h[:, NT] * 1.1, np.full(nb, 99.0)], axis=1)   # (column 3: not read)
    return dict(mu=mu, ga=ga, n0=n0, n=n, w=w, seg=seg, nb=nb, prof=prof, zprof=zprof, nt=nt, jout=jout, zz=zz, tauout=tauout,
                tauvrai=tauvrai, rec=rec, norders=norders, aik=aik, flux=flux, scal=scal, failed=failed, beyond=beyond)


def _run(gpu_pkg, cx, d, table=None, cob=None):
    """The kernel and its three reference chains on one set of inputs.  Returns host arrays: irr / irr_tv (d_tauvrai NULL /
    given) [NZ][nseg][14], ab [NZ][nseg][4], scal [NZ][nseg][10+N] (element 9 from tauvrai), e [NZ][nseg][2] (sosgpu_level_flux
    of the aggregated records, the bin with jout past NT taken out as the kernel takes it out)."""
    import torch
    sv = gpu_pkg.solver
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    nseg = len(d["seg"]) - 1
    bins = dict(nb=d["nb"], lp=LP, nt=t(d["nt"]), prof=t(d["prof"]), zprof=t(d["zprof"]), scal=t(d["scal"]))
    lv = dict(nz=NZ, jout=t(d["jout"]), zz=t(d["zz"]), tauout=t(d["tauout"]))
    lv_tv = dict(lv, tauvrai=t(d["tauvrai"]))
    out = dict(rec=t(d["rec"]), norders=t(d["norders"]), flux=t(d["flux"]))
    aik, seg = t(d["aik"]), t(d["seg"])
    res = {}
    if table is None:
        res["irr"] = cx.level_irradiance(bins, lv, out, aik, seg=seg)
        res["irr_tv"] = cx.level_irradiance(bins, lv_tv, out, aik, seg=seg)
        res["ab"] = cx.level_absorption(bins, lv, out, aik, seg=seg)
        rec_all, res["scal"] = cx.aggregate_levels(out, lv_tv, aik, seg=seg, scal=bins["scal"])
        no_e = d["norders"].copy()
        no_e[d["beyond"]] = -1                                             # (its jout is past NT in slots 0 and 2, 0 in slot 1)
        rec_e, _ = cx.aggregate_levels(dict(out, norders=t(no_e)), lv, aik, seg=seg, scal=bins["scal"])
        res["e"] = sv.level_flux_many([(cx, (rec_all if k == 1 else rec_e)[k, g]) for k in range(NZ)
                                       for g in range(nseg)]).reshape(NZ, nseg, 2)
    else:
        res["irr_tv"] = sv.level_irradiance_spectrum(table, bins, t(cob), seg, aik, lv_tv, out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("ng,sun,s1", [(8, 35.0, 5), (24, 60.0, 1)], ids=["n9_five_orders", "n25_order0_context"])
def test_columns_have_the_bits_of_the_kernels_they_restate(gpu_pkg, ng, sun, s1):
    d = _synthetic(ng, sun, 5 + ng, s1)
    al, be, gm, ze = S.hg_phase(4, 0.5)
    cx = gpu_pkg.SosContext(d["mu"], d["ga"], d["n0"], al, be, gm, ze, build=False, **(dict(iborm_max=0) if s1 == 1 else {}))
    assert d["n"] == ng + 1 and cx.smax + 1 == s1 and cx.w == d["w"]
    try:
        r = _run(gpu_pkg, cx, d)
    finally:
        cx.close()
    nseg = len(SEG_SIZES)
    irr, tv, ab, scal, e = r["irr"], r["irr_tv"], r["ab"], r["scal"], r["e"]
    assert irr.shape == tv.shape == (NZ, nseg, COLS) and np.isfinite(tv).all()
    # d_tauvrai NULL: column 11 is 0 and nothing else moves
    rest = [c for c in range(COLS) if c != 11]
    assert (irr[:, :, 11] == 0.0).all() and np.array_equal(irr[:, :, rest], tv[:, :, rest]) and (tv[:, :, 11] > 0).all()
    # columns 0..3: sosgpu_level_absorption's block (zeros in the standard-output slot)
    assert np.array_equal(tv[:, :, 0:4], ab), np.argwhere(tv[:, :, 0:4] != ab)[:4].tolist()
    assert (ab[1] == 0.0).all() and (ab[[0, 2]][:, :, :3] > 0).all()
    # columns 6..10 and 11: elements 3, 4, 5, 6, 8 and 9 of sosgpu_aggregate's scalar block of the slot
    # ... and 12, 13: elements 1 and 2, sum aik {EMOINS, EPLUS} of the solve, in every slot
    for col, el in ((6, 3), (7, 4), (8, 5), (9, 6), (10, 8), (11, 9), (12, 1), (13, 2)):
        assert np.array_equal(tv[:, :, col], scal[:, :, el]), (col, el, np.argwhere(tv[:, :, col] != scal[:, :, el])[:4].tolist())
    assert tv[0, 0, 10] == -1.0 and (tv[:, 1:, 10] == 1.0).all()            # -(min norders): a failed bin in the segments >= 2
    # every slot, the standard output included: sosgpu_level_flux of the aggregated record -- the one-bin segment with aik = 1
    # bit for bit
    for k in range(NZ):
        assert np.array_equal(tv[k, 0, 4:6], e[k, 0]), (k, tv[k, 0, 4:6].tolist(), e[k, 0].tolist())
    rel = np.abs(tv[:, :, 4:6] / e - 1)
    worst = float(rel.max())
    print("N = %d: worst relative deviation of e_dn / e_up from sosgpu_level_flux of the aggregated record %.3e" % (d["n"], worst))
    assert (e > 0).all() and worst <= BAR, "worst relative deviation %.3e" % worst


@pytest.mark.gpu
def test_table_form_equals_the_per_context_calls(gpu_pkg):
    """Two contexts of N = 9 and different mu (suns of 35 and 50 degrees) in one launch: the segments alternate between the
    contexts, context 1 first, so no context's bins are contiguous; every segment has the bits of the call on its own context."""
    import torch
    d = _synthetic(8, 35.0, 21, 2)
    mu2, ga2, n02 = S.gauss_angles(8, 50.0)
    assert len(mu2) == d["n"] and float(mu2[n02 - 1]) != float(d["mu"][d["n0"] - 1])
    al, be, gm, ze = S.hg_phase(4, 0.5)
    cxs = [gpu_pkg.SosContext(d["mu"], d["ga"], d["n0"], al, be, gm, ze, iborm_max=1),
           gpu_pkg.SosContext(mu2, ga2, n02, al, be, gm, ze, iborm_max=1)]
    ctx_of_seg = [1, 0, 1, 0, 1, 0]
    cob = np.repeat(ctx_of_seg, SEG_SIZES).astype(np.int32)
    try:
        table = gpu_pkg.solver.ContextTable(cxs)
        got = _run(gpu_pkg, cxs[0], d, table, cob)["irr_tv"]
        for i, cx in enumerate(cxs):
            mine = [g for g, c in enumerate(ctx_of_seg) if c == i]
            keep = np.concatenate([np.arange(d["seg"][g], d["seg"][g + 1]) for g in mine])
            sub = dict(d, nb=len(keep), seg=np.concatenate([[0], np.cumsum([SEG_SIZES[g] for g in mine])]).astype(np.int32),
                       beyond=int(np.flatnonzero(keep == d["beyond"])[0]) if d["beyond"] in keep else 0)
            for k in ("prof", "zprof", "nt", "norders", "aik", "flux", "scal"):
                sub[k] = d[k][keep]
            for k in ("jout", "zz", "tauout", "tauvrai", "rec"):
                sub[k] = d[k][:, keep]
            own = _run(gpu_pkg, cx, sub)["irr_tv"]
            for j, g in enumerate(mine):
                assert np.array_equal(got[:, g], own[:, j]), (i, g, np.argwhere(got[:, g] != own[:, j])[:4].tolist())
    finally:
        for cx in cxs:
            cx.close()
    assert np.isfinite(got).all() and (got[[0, 2]][:, :, [0, 1, 2, 4, 5]] > 0).all()      # (q is 0 where two altitudes coincide)


@pytest.mark.gpu
def test_refusals_queue_nothing_and_the_guard_stays(gpu_pkg):
    """Every refusal of the header on real device pointers: SOSGPU_E_ARG and d_out untouched; then the good call, which leaves
    the doubles behind d_out alone."""
    import torch
    d = _synthetic(8, 35.0, 2, 1)
    al, be, gm, ze = S.hg_phase(4, 0.5)
    cx = gpu_pkg.SosContext(d["mu"], d["ga"], d["n0"], al, be, gm, ze, iborm_max=0, build=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    ptr = lambda x: C.c_void_p(x.data_ptr())
    nseg = len(SEG_SIZES)
    try:
        k = {n: t(d[n]) for n in ("nt", "prof", "zprof", "jout", "zz", "tauout", "rec", "norders", "flux", "scal", "tauvrai", "seg", "aik")}
        out = torch.full((NZ * nseg * COLS + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        f = gpu_pkg.capi.lib().sosgpu_level_irradiance
        good = [cx._h, None, None, d["nb"], LP, ptr(k["nt"]), ptr(k["prof"]), ptr(k["zprof"]), NZ, ptr(k["jout"]), ptr(k["zz"]),
                ptr(k["tauout"]), ptr(k["rec"]), ptr(k["norders"]), ptr(k["flux"]), ptr(k["scal"]), ptr(k["tauvrai"]), nseg,
                ptr(k["seg"]), ptr(k["aik"]), ptr(out), cx._stream()]
        for i in (0, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 18, 19, 20):
            bad = list(good)
            bad[i] = None
            assert f(*bad) == E_ARG, i
        for i, v in ((8, 0), (8, 17), (4, 1), (3, -1), (17, -1), (1, ptr(k["prof"]))):
            bad = list(good)
            bad[i] = v
            assert f(*bad) == E_ARG, (i, v)
        for i in (3, 17):                                                  # nb = 0, nseg = 0: SOSGPU_OK, nothing queued
            ok = list(good)
            ok[i] = 0
            assert f(*ok) == 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
        assert f(*good) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        again = cx.level_irradiance(dict(nb=d["nb"], lp=LP, nt=k["nt"], prof=k["prof"], zprof=k["zprof"], scal=k["scal"]),
                                    dict(nz=NZ, jout=k["jout"], zz=k["zz"], tauout=k["tauout"], tauvrai=k["tauvrai"]),
                                    dict(rec=k["rec"], norders=k["norders"], flux=k["flux"]), k["aik"], seg=k["seg"]).cpu().numpy()
    finally:
        cx.close()
    assert np.isnan(got[-GUARD:]).all() and np.isfinite(got[:-GUARD]).all()
    assert np.array_equal(got[:-GUARD].reshape(NZ, nseg, COLS), again)


# ------------------------------------------------------------------------------------------------------------- end to end

ALTS = [-1, 0.0, 3.0, 8.5]
NAMES = ["rayleigh", "absorbing aerosol, truncation", "cfg4_glitter_bilnd", "ckd_o2a_5bins", "layer_1_3km_lnd", "ckd_o2a_mode2"]
BAND = 3                                                                   # the one call of several bins
DIFFUSE = {1, 2, 3, 4, 6}                                                  # flux columns formed from E-, E+ (LEVEL_FLUX_SPLIT_NAMES)


def _calls(rs, workdir):
    """Six calls: a conservative Rayleigh call, an absorbing aerosol with truncation (aer_phase), a rough-sea call, the 5-bin
    CKD band of tests/golden/fic, and two that keep their per-wavelength preparation: an aerosol layer and -SOS.AbsModeCKD 2."""
    (_, nogas, aer), _ = tla._pipe_calls(rs, workdir)
    fixed, _, _, _ = spectrum_cases.build(rs, workdir, names=NAMES[2:])
    fixed = [dict(kw, zout=-1.0, fictrans="NO_OUTPUT", ficflux="NO_OUTPUT") for kw in fixed]
    kws = [tlc._pipe_kwargs(rs, {"-SOS_Main.Wa": 0.55}), nogas] + fixed
    return kws, [None, aer] + [None] * len(fixed)


@pytest.fixture(scope="module")
def e2e(gpu_pkg, tmp_path_factory):
    """The calls, the reference rows of sos_spectrum_levels and the rows of the pass at the default chunk, computed once."""
    import os
    rs = gpu_pkg.run_sos
    old = os.environ.get("SOS_ABS_ROOT")
    os.environ["SOS_ABS_ROOT"] = GOLD
    try:
        kws, aers = _calls(rs, tmp_path_factory.mktemp("irr"))
        _, ref_flux, ref_absorb = rs.sos_spectrum_levels(ALTS, kws, aer_phases=aers, fluxes=True, split=True, absorption=True)
        flux, absorb = rs.sos_spectrum_irradiances(ALTS, kws, aer_phases=aers, split=True, absorption=True)
    finally:
        if old is None:
            del os.environ["SOS_ABS_ROOT"]
        else:
            os.environ["SOS_ABS_ROOT"] = old
    return dict(kws=kws, aers=aers, ref_flux=ref_flux, ref_absorb=ref_absorb, flux=flux, absorb=absorb)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.gpu
def test_rows_against_the_levels_pass(gpu_pkg, e2e):
    """One-bin calls: equal bits in every column.  The band: 1e-12 in the two diffuse-flux columns and those formed from them,
    equal bits elsewhere (the absorption rows are per-bin sums in both passes)."""
    rs = gpu_pkg.run_sos
    assert rs.LEVEL_FLUX_SPLIT_NAMES[1] == "flux_diff_down_tronc" and rs.LEVEL_FLUX_SPLIT_NAMES[3] == "flux_diff_up"
    worst = 0.0
    for i, name in enumerate(NAMES):
        f, a, rf, ra = e2e["flux"][i], e2e["absorb"][i], e2e["ref_flux"][i], e2e["ref_absorb"][i]
        assert f.shape == rf.shape == (len(ALTS), 7) and a.shape == ra.shape == (len(ALTS), 5), name
        assert np.isnan(a[0]).all() and np.isfinite(a[1:]).all() and np.isfinite(f).all(), name
        assert _same(a, ra), (name, a.tolist(), ra.tolist())              # per-bin products in both passes: equal bits
        if i != BAND:
            assert _same(f, rf), (name, np.argwhere(f != rf).tolist(), f.tolist(), rf.tolist())
            continue
        keep = [c for c in range(7) if c not in DIFFUSE]
        assert _same(f[:, keep], rf[:, keep]), (name, f.tolist(), rf.tolist())
        rel = np.abs(f[:, sorted(DIFFUSE)] / rf[:, sorted(DIFFUSE)] - 1)
        worst = float(rel.max())
        print("%s: worst relative deviation of the diffuse-flux columns %.3e" % (name, worst))
        assert worst <= BAR, "worst relative deviation %.3e" % worst


@pytest.mark.gpu
def test_chunks_and_launch_counts(gpu_pkg, e2e, monkeypatch):
    """chunk = 1, 2 and 256 give the same rows; per solved group (or single call) ONE sosgpu_level_irradiance and no
    sosgpu_aggregate, sosgpu_trphi_spectrum, sosgpu_level_flux_spectrum (nor their single forms), counted at the library."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    L = gpu_pkg.capi.lib()
    n = {}
    names = ("sosgpu_level_irradiance", "sosgpu_os_solve_multi_levels", "sosgpu_os_solve_levels", "sosgpu_aggregate",
             "sosgpu_trphi_spectrum", "sosgpu_trphi", "sosgpu_level_flux_spectrum", "sosgpu_level_flux", "sosgpu_level_absorption",
             "sosgpu_level_transmission", "sosgpu_channel_accumulate", "sosgpu_channel_finish")

    def counted(name):
        f = getattr(L, name)
        n[name] = 0

        def g(*a):
            n[name] += 1
            return f(*a)
        return g

    for name in names:
        monkeypatch.setattr(L, name, counted(name))
    for chunk in (1, 2, 256):
        for k in n:
            n[k] = 0
        flux, absorb = rs.sos_spectrum_irradiances(ALTS, e2e["kws"], aer_phases=e2e["aers"], split=True, absorption=True, chunk=chunk)
        solves = n["sosgpu_os_solve_multi_levels"] + n["sosgpu_os_solve_levels"]
        assert n["sosgpu_level_irradiance"] == solves >= 1, (chunk, n)
        assert (solves == 6) if chunk < 256 else (1 <= solves <= 6), (chunk, n)
        assert all(n[k] == 0 for k in names[3:]), (chunk, n)
        for i in range(len(NAMES)):
            assert _same(flux[i], e2e["flux"][i]) and _same(absorb[i], e2e["absorb"][i]), (chunk, NAMES[i])
    # without split and absorption: the first five columns alone, the same bits
    plain = rs.sos_spectrum_irradiances(ALTS, e2e["kws"], aer_phases=e2e["aers"])
    assert all(p.shape == (len(ALTS), 5) and _same(p, f[:, :5]) for p, f in zip(plain, e2e["flux"]))


@pytest.mark.gpu
def test_seventeen_altitudes_and_weighted_sums(gpu_pkg, e2e):
    """17 altitudes on the two no-gas calls equal two reference calls of 16 + 1 altitudes, bit for bit; the weighted sums for
    R = 2 (one row per altitude) equal the host loop over the unweighted rows of the same pass."""
    from test_irradiance import _host_loop
    rs = gpu_pkg.run_sos
    kws, aers = e2e["kws"][:2], e2e["aers"][:2]
    alts = [-1, 0.0] + [0.25 + 0.75 * j for j in range(14)] + [120.0]
    assert len(alts) == 17
    flux, absorb = rs.sos_spectrum_irradiances(alts, kws, aer_phases=aers, split=True, absorption=True)
    for part in (slice(0, 16), slice(16, 17)):
        _, rf, ra = rs.sos_spectrum_levels(alts[part], kws, aer_phases=aers, fluxes=True, split=True, absorption=True)
        for i in range(2):
            assert _same(flux[i][part], rf[i]) and _same(absorb[i][part], ra[i]), (i, part)
    rng = np.random.default_rng(1)
    w = np.stack([np.repeat(rng.uniform(0.5, 2.0, (1, 2)), 17, axis=0), rng.uniform(0.0, 2.0, (17, 2))])
    w[1, 3, 0] = 0.0
    fs, ab = rs.sos_spectrum_irradiances(alts, kws, aer_phases=aers, split=True, absorption=True, weights=w)
    assert fs.shape == (2, 17, 7) and ab.shape == (2, 17, 5)
    assert _same(fs, _host_loop(w, flux)) and _same(ab, _host_loop(w, absorb))
    assert np.isnan(ab[:, 0]).all() and np.isfinite(ab[:, 1:]).all() and _same(ab[1, 3], w[1, 3, 1] * absorb[1][3])
    flat = rs.sos_spectrum_irradiances(alts, kws, aer_phases=aers, weights=w[0, :1], normalize=True)
    wn = rs._irradiance_weights("t", w[0, :1], True, 2, 17)
    assert flat.shape == (1, 17, 5) and _same(flat, _host_loop(wn, [f[:, :5] for f in flux]))


@pytest.mark.gpu
def test_net_flux_of_a_conservative_rayleigh_call_is_constant(gpu_pkg):
    """The independent check: without absorption flux_net does not depend on the altitude (test_level_conservation's nets()
    and bar: the span at most d / DETECT, d the smallest step of the direct flux between adjacent altitudes)."""
    rs = gpu_pkg.run_sos
    flux = rs.sos_spectrum_irradiances(tlc.PIPE_ALTS, [tlc._pipe_kwargs(rs, {"-SOS_Main.Wa": 0.55})])[0]
    assert flux.shape == (len(tlc.PIPE_ALTS), 5) and np.isfinite(flux).all()
    span, d = tlc._span_and_d(flux)
    print("rayleigh: nets %s span %.3e d %.3e" % (tlc.nets(flux).tolist(), span, d))
    assert span <= d / tlc.DETECT, (span, d)
