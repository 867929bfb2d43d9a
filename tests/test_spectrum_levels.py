"""Output slots in the multi-wavelength launch (sosgpu_os_solve_multi_levels, solver.solve_spectrum_levels,
run_sos.sos_spectrum_levels).

A spectrum at K output altitudes is one preparation per wavelength and one launch per kernel variant whose bins carry K output
slots.  Slot k of every bin must equal, bit for bit, what the single-context slot solve of its own wavelength gives
(sosgpu_os_solve_levels, itself equal to a single-altitude solve: test_output_levels.py).
CPU: the argument rules of sos_spectrum_levels, the slot-table concatenation.
GPU: every layout x SURF cell split over two contexts in one launch, with and without the cost order, a split into
sub-launches; a flagged slot level; sos_spectrum_levels against sos_proc end to end and on two ranks."""
import hashlib
import json

import numpy as np
import pytest

import spectrum_cases
from spectrum_cases import assert_tuples_equal
import test_output_levels as tol
import test_variant_matrix as vm
from dist_launch import run_ranks

GOLD = spectrum_cases.GOLD


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_sos_spectrum_levels_argument_errors_before_any_device_work(pkg):
    rs = pkg.run_sos
    base = {"-SOS_Main.Wa": 0.55, "-ANG.Thetas": 30.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.0, "-SURF.Alb": 0.1,
            "-AP.HR": 8.0, "-SOS.View": 1, "-SOS.View.Phi": 0.0}
    kw = tol._user_kwargs(rs, base)
    kws = [kw, tol._user_kwargs(rs, dict(base, **{"-SOS_Main.Wa": 0.67}))]
    for bad in (-2.0, 121.0, -0.5):
        with pytest.raises(rs.SosProcError) as e:
            rs.sos_spectrum_levels([1.0, bad], kws)
        assert e.value.code == 2611
    with pytest.raises(ValueError):
        rs.sos_spectrum_levels([], kws)
    with pytest.raises(ValueError):
        rs.sos_spectrum_levels([1.0] * 17, kws)
    # the rules hold for every call of the list, also past the first one
    with pytest.raises(ValueError):
        rs.sos_spectrum_levels([1.0], kws + [tol._user_kwargs(rs, dict(base, **{"-SOS.OutputAlt": 3.0}))])
    with pytest.raises(ValueError):
        rs.sos_spectrum_levels([1.0], kws + [tol._user_kwargs(rs, dict(base, **{"-SOS_Main.ResRoot": "/nonexistent/results"}))])
    # ... and before the empty-spectrum shortcut
    with pytest.raises(ValueError):
        rs.sos_spectrum_levels([1.0] * 17, [])
    assert rs.sos_spectrum_levels([-1.0, 3.0, 3.0], []) == []


def _host_batch(pkg, lp, profiles):
    """A bin dict shaped like upload_bins' (on the CPU) from (h, zprof) pairs of the aerosol-layer profile."""
    import torch
    nb = len(profiles)
    prof = np.zeros((nb, 3, lp))
    zp = np.zeros((nb, max(len(z) for _, z in profiles)))
    nt = np.zeros(nb, dtype=np.int32)
    for b, (h, z) in enumerate(profiles):
        prof[b, 0, :len(h)] = h
        zp[b, :len(z)] = z
        nt[b] = len(h) - 1
    return dict(nb=nb, lp=lp, perm=None, nt=torch.from_numpy(nt), iborm=torch.zeros(nb, dtype=torch.int32),
                prof=torch.from_numpy(prof), jout=None, zz=None, zprof_host=zp)


def test_concat_levels_orders_and_pads_like_concat_bins(pkg):
    """Two batches of different padded widths -- one with device-style levels, one with host level altitudes (zprof_host,
    host_output_levels) -- concatenated: the slots follow concat_bins' bin order, and every slot still points at the same two
    levels of the (padded) concatenated profile, whose TAUOUT interpolation it carries."""
    import torch
    rs, sv = pkg.run_sos, pkg.solver
    alts = [-1.0, 0.0, 2.0, 120.0, 2.0]
    layers = [rs.profile_layer(0.0973, 8.0, ta, zmin, zmax)            # 80, 40 and 30 levels
              for ta, zmin, zmax in ((0.3, 1.0, 3.0), (0.1, 0.0, 2.0), (0.05, 0.5, 1.0))]
    a = _host_batch(pkg, 48, [(h, z) for h, _, _, z in layers[1:]])
    b = _host_batch(pkg, 80, [(h, z) for h, _, _, z in layers])
    la = sv.host_output_levels(a, alts)
    lb = sv.host_output_levels(b, alts)
    lv = sv.concat_levels([la, lb])
    bins, cob, seg = sv.concat_bins([a, b])
    assert bins["lp"] == 80 and bins["nb"] == 5 and lv["nz"] == len(alts)
    for key in ("jout", "zz", "tauout"):
        assert tuple(lv[key].shape) == (len(alts), 5)
        assert torch.equal(lv[key][:, :2], la[key]) and torch.equal(lv[key][:, 2:], lb[key]), key
    assert lv["jout"].dtype == torch.int32 and lv["zz"].dtype == torch.float64
    assert cob.tolist() == [0, 0, 1, 1, 1] and seg.tolist() == [0, 2, 5]
    h = bins["prof"][:, 0, :].numpy()
    zh = np.concatenate([np.pad(a["zprof_host"], ((0, 0), (0, b["zprof_host"].shape[1] - a["zprof_host"].shape[1]))),
                         b["zprof_host"]])
    jl, zl = pkg.solver.output_levels_host(zh, alts)
    assert np.array_equal(lv["jout"].numpy(), jl) and np.array_equal(lv["zz"].numpy(), zl)
    for k, z in enumerate(alts):
        for i in range(5):
            j, w = int(jl[k, i]), float(zl[k, i])
            assert j <= int(bins["nt"][i])
            want = h[i, 0] if z == -1.0 else (1 - w) * h[i, j - 1] + w * h[i, j]
            assert float(lv["tauout"][k, i]) == want, (k, i)
    # a batch without bins (no tensors) drops out; mixed altitude counts are refused
    assert sv.concat_levels([la, dict(nz=len(alts), jout=None, zz=None, tauout=None)])["jout"].shape == (len(alts), 2)
    with pytest.raises(ValueError):
        sv.concat_levels([la, sv.host_output_levels(b, alts[:2])])


def _scratch_numbers(n, lp, nz):
    """Doubles of one work region of the streamed kernel at lp padded levels (stream_scratch_doubles, csrc/solve_variant.h) and
    of the lane-private state of nz output slots of that region (lv_stride, csrc/solve_plan.h)."""
    kh = vm._round_up(3 * n, 8)
    nw, kht = (8, 16) if kh > 128 else (4, 4) if kh <= 64 else (4, 5 if kh <= 80 else 6 if kh <= 96 else 8)
    khm, cols, vpad = 16 * kht, 32, 8
    fs, ns = 2 * khm + 2, (khm // 3 + 1) & ~1
    lpb = vm._round_up(lp, 32)
    d = lpb * fs + (lpb + 1) * ns + 7 * (lpb + vpad) + (lpb // cols) * (2 * khm + 2 * ns) + 2 * 64 * nw + 8
    per_bin = (d + 15) & ~15
    lv = nz * 8 * 64 * nw                                  # [nz][SOS_LV_N][threads]
    return per_bin, lv


def _scratch_split(n, lp, nb, nz, gib):
    """Bins per launch of a streamed table launch (solve_plan, csrc/solve_plan.h), with and without output slots: the
    SOSGPU_SCRATCH_GIB budget over a work region plus the slots' lane-private state.  An independent restatement:
    test_solve_plan.py compares it with what the library reports (sosgpu_debug_solve_plan)."""
    per_bin, lv = _scratch_numbers(n, lp, nz)
    cap = (gib << 30) // 8
    return min(nb, max(1, cap // (per_bin + lv))), min(nb, max(1, cap // per_bin))


def test_scratch_split_restatement():
    # the 16-tile layout at 608 levels: about 3 MB of scratch per bin, a few hundred bins per GiB
    with_slots, without = _scratch_split(43, 608, 340, 6, 1)
    assert with_slots < 340 <= without
    assert _scratch_split(21, 608, 340, 6, 64) == (340, 340)


# ---- GPU: kernels -----------------------------------------------------------------------------------------------------------

def _two_context_launch(pkg, b, rows, alts, orders, levels_hook=None):
    """The bins `rows` of batch b split over two contexts (as test_variant_matrix does for solve_spectrum): each context's own
    solve_levels, then one solve_spectrum_levels launch over both per order.  Returns (bins of context 0, refs, multi results
    per order)."""
    import torch
    sv = pkg.solver
    cx = vm._context(pkg, b)
    cx2 = vm._context(pkg, b, g=0.8, rscale=1.5)
    try:
        ra, rb = rows[0::2], rows[1::2]
        ba, bb = vm._upload(cx, b, ra), vm._upload(cx2, b, rb)
        la, lb = cx.output_levels(ba, alts), cx2.output_levels(bb, alts)
        if levels_hook:
            levels_hook(la, lb)
        refs = [vm._fetch(cx.solve_levels(ba, la)), vm._fetch(cx2.solve_levels(bb, lb))]
        table = sv.ContextTable([cx, cx2])
        bins, cob, seg = sv.concat_bins([ba, bb])
        levels = sv.concat_levels([la, lb])
        nb = bins["nb"]
        aik = torch.full((nb,), 1.0 / nb, dtype=torch.float64, device=cx.device)
        got = []
        for order in orders:
            out = cx.alloc_outputs(nb)
            out["rec"] = torch.zeros((len(alts), nb, cx.smax + 1, 3, cx.w), dtype=torch.float64, device=cx.device)
            rec, scal = sv.solve_spectrum_levels(table, bins, cob, seg, aik, levels, out=out, order=order)
            assert tuple(rec.shape) == (len(alts), 2, cx.smax + 1, 3, cx.w) and tuple(scal.shape)[:2] == (len(alts), 2)
            got.append(vm._fetch(out))
        return len(ra), refs, got
    finally:
        cx.close()
        cx2.close()


def _assert_slots_equal(na, refs, got, what, skip=()):
    for c, (ref, sl) in enumerate(zip(refs, (slice(0, na), slice(na, None)))):
        keep = [i for i in range(ref["norders"].shape[0]) if (c, i) not in skip]
        for key in ("norders", "iglast", "flux"):
            assert np.array_equal(got[key][sl][keep], ref[key][keep]), (what, c, key)
        assert np.array_equal(got["rec"][:, sl][:, keep], ref["rec"][:, keep]), (what, c)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", tol.CELLS, ids=lambda c: "%s-%s-N%d-lp%d" % (c[0], "SURF" if c[1] else "noSURF", c[2], c[3]))
def test_multi_levels_bitwise_vs_single_context_slots(gpu_pkg, cell):
    lay, surf, n, lp = cell
    b = tol._batch(lay, surf, n, lp)
    rows = list(range(len(b["bins"])))
    na, refs, got = _two_context_launch(gpu_pkg, b, rows, tol._slot_altitudes(b), ("cost", None))
    for ref in refs:
        assert (ref["norders"] > 0).all()
    for order, g in zip(("cost", None), got):
        _assert_slots_equal(na, refs, g, "%s surf=%s N=%d lp=%d order=%s" % (lay, surf, n, lp, order))


@pytest.mark.gpu
def test_multi_levels_split_into_sub_launches(gpu_pkg, monkeypatch):
    """A 1 GiB scratch budget splits a 340-bin table launch of the 16-tile streamed layout in two (329 + 11 bins): the second
    sub-launch reads its slot tables at offset b0 of the whole batch's [K][nb] tables.  (Without the slot state in the budget
    the 340 bins would have fitted in one launch.)"""
    lay, n, lp = "stream<8,2,16>", 43, 608
    b = vm.make_batch(lay, False, False, n, lp)
    nb = 340
    rows = [1 if i % 60 == 7 else 0 for i in range(nb)]        # mostly NT = 1, a few NT = 95 bins
    alts = tol._slot_altitudes(b)
    per_launch, without = _scratch_split(n, lp, nb, len(alts), 1)
    assert per_launch < nb <= without
    monkeypatch.setenv("SOSGPU_SCRATCH_GIB", "1")
    na, refs, got = _two_context_launch(gpu_pkg, b, rows, alts, ("cost",))
    for ref in refs:
        assert (ref["norders"] > 0).all()
    _assert_slots_equal(na, refs, got[0], "%s split at %d of %d bins" % (lay, per_launch, nb))


@pytest.mark.gpu
def test_multi_levels_flag_a_bin_whose_level_is_out_of_range(gpu_pkg):
    """Slot 1 of one bin of context 0 points past its NT: that bin is flagged (norders = -1); every other bin of the launch, of
    either context, is bit-identical to the single-context solves with valid levels."""
    b = tol._batch("os<4,1,2>", False, 21, 32)
    rows = list(range(len(b["bins"])))
    alts = [-1.0, 0.0]
    na, refs, _ = _two_context_launch(gpu_pkg, b, rows, alts, ())
    ra = rows[0::2]

    def corrupt(la, lb):
        la["jout"] = la["jout"].clone()
        la["jout"][1, 1] = int(b["nt"][ra[1]]) + 1

    _, _, got = _two_context_launch(gpu_pkg, b, rows, alts, ("cost",), levels_hook=corrupt)
    assert got[0]["norders"][1] == -1 and (np.delete(got[0]["norders"], 1) > 0).all()
    _assert_slots_equal(na, refs, got[0], "flagged bin", skip={(0, 1)})


# ---- GPU: end to end --------------------------------------------------------------------------------------------------------

ALTS = [-1, 0.0, 3.0, 120.0, 0.75, 3.0]
# the fixed goldens (CKD bands of 5 and 25 bins with -SOS.Trans, gas level grids with NT > 64, land and sea surfaces, polar
# views, the aerosol-layer profile) and six random keyword sets twice (groups of several wavelengths per launch)
E2E_NAMES = spectrum_cases.FIXED_CASES + spectrum_cases.RANDOM_CASES[:6] * 2


def _kws(rs, tmp, names=E2E_NAMES):
    kws, _, _, _ = spectrum_cases.build(rs, tmp, names=names)
    return [dict(kw, zout=-1.0) for kw in kws]


@pytest.mark.gpu
def test_sos_spectrum_levels_equals_sos_proc_per_altitude(gpu_pkg, tmp_path, monkeypatch):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws = _kws(rs, tmp_path)
    assert {"cfg5_ckd_maignan_25bins", "ckd_o2a_5bins", "glitter_polar", "land_breon", "flatsea_lnd"} <= set(E2E_NAMES)
    launches = []
    real = gpu_pkg.solver.solve_spectrum_levels

    def counted(table, bins, *a, **k):
        launches.append((len(table.ctxs), bins["lp"]))
        return real(table, bins, *a, **k)

    monkeypatch.setattr(gpu_pkg.solver, "solve_spectrum_levels", counted)
    tm = {}
    got = rs.sos_spectrum_levels(ALTS, kws, timings=tm)
    assert launches and all(lp == 608 for _, lp in launches), launches   # table launches on the products' level grids
    assert set(tm) >= {"prepare", "solve_launch", "wait", "trphi", "finish"}
    assert len(got) == len(kws) and all(len(g) == len(ALTS) for g in got)
    for i, kw in enumerate(kws):
        for k, z in enumerate(ALTS):
            assert_tuples_equal(got[i][k], rs.sos_proc(**dict(kw, zout=float(z))), "call %d zout=%g" % (i, z))
    spec = rs.sos_spectrum(kws)
    for i in range(len(kws)):
        assert_tuples_equal(got[i][0], spec[i], "call %d vs sos_spectrum" % i)
    # small chunks (one wavelength each at K = 6) and parts; then parts that still form groups
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    for kwargs, sub in ((dict(chunk=5, parts=3), slice(0, 12)), (dict(chunk=60, parts=3), slice(None))):
        again = rs.sos_spectrum_levels(ALTS, kws[sub], **kwargs)
        for i, g in enumerate(again):
            for k in range(len(ALTS)):
                assert_tuples_equal(g[k], got[sub][i][k], "%s call %d slot %d" % (kwargs, i, k))


def _digest(outs):
    h = hashlib.sha256()
    for per in outs:
        for t in per:
            for x in t:
                h.update(np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes())
    return h.hexdigest()


DIST_NAMES = ["ckd_h2o_o2_25bins_flatsea", "cfg1_lambert", "ckd_o2a_5bins", "rand_00", "rand_13", "rand_05", "flatsea_zout",
              "rand_17", "land_roujean", "rand_00", "rand_13"]


@pytest.mark.gpu
def test_sos_spectrum_levels_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """Two ranks on cuda:0 (tests/dist_spectrum_levels_worker.py): the gathered results equal this process's on every rank;
    a spectrum with one refused call makes every rank raise SosProcError -- no rank is left waiting in the gather."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    out = str(tmp_path / "res.json")
    run_ranks("dist_spectrum_levels_worker.py", ("--out", out), timeout=600)
    r = json.load(open(out))
    single = rs.sos_spectrum_levels(ALTS, _kws(rs, tmp_path / "single", DIST_NAMES))
    assert r["world"] == 2 and r["digests"] == [_digest(single)] * 2, r["digests"]
    assert sorted(i for own in r["owners"] for i in own) == list(range(len(DIST_NAMES)))
    assert all(len(own) > 0 for own in r["owners"])
    assert r["raised"] == [True, True] and all("wavelength 3" in m for m in r["messages"]), r["messages"]
