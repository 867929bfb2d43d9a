"""COEFF_ABS_CKD on the device (csrc/ckd.hip k_coeff_abs_ckd_table, C ABI sosgpu_ckd_layer_tables, solver.ckd_layer_tables) and
its place in front of SOS_ABSPROFILE in the spectrum pass.  The checker is the statement-for-statement host restatement
tests/test_absorption.py pins to the compiled reference (absorption.layer_tables_scalar / coeff_abs_ckd); every comparison
is equality of doubles -- the arithmetic is + - * / in a fixed order, there is no tolerance."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import ckd_cells
import spectrum_cases
from spectrum_cases import assert_tuples_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = spectrum_cases.GOLD
ABS_CASES = ["o2a_mls", "h2o_o2_trop_user", "h2o_o2_subarctic", "o2a_us62_nopsurf"]
same = ckd_cells.same_doubles


def _fixture_preps(A):
    g = np.load(os.path.join(GOLD, "absorption.npz"))
    out = []
    for name in ABS_CASES:
        wa, nustep, psurf, h2o, o3, co2, ch4, typ = g[name + "_args"]
        out.append(A.prepa_absprofile(wa, nustep, psurf, h2o, o3, co2, ch4, int(typ)))
    return out


@pytest.fixture()
def fic(monkeypatch):
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    return GOLD


_SCALAR = {}


def _scalar_tables(A):
    """layer_tables_scalar of the four fixture wavelengths, computed once for the module."""
    if not _SCALAR:
        os.environ["SOS_ABS_ROOT"], old = GOLD, os.environ.get("SOS_ABS_ROOT")
        try:
            _SCALAR["preps"] = _fixture_preps(A)
            _SCALAR["ref"] = [A.layer_tables_scalar(p) for p in _SCALAR["preps"]]
        finally:
            if old is None:
                del os.environ["SOS_ABS_ROOT"]
            else:
                os.environ["SOS_ABS_ROOT"] = old
    return _SCALAR["preps"], _SCALAR["ref"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_symbols_in_header_and_export_list(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    declared = set(re.findall(r"\b(sosgpu_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.capi.lib()
    for sym in ("sosgpu_ckd_layer_tables", "sosgpu_ckd_layer_tables_work_bytes"):
        assert sym in declared and sym in pkg.capi.EXPORTS and hasattr(L, sym), sym
    assert "sosgpu_ckd_wl" in hdr
    assert C.sizeof(pkg.capi.CkdWl) == pkg.solver.CKD_WL_DTYPE.itemsize == 72


def test_pack_ckd_requests_reproduces_every_request(pkg, fic):
    """Offsets, slot order and NULL slots of the host packing: every axis and layer state is found at its offset, the slot of
    (gas, term) is gas * 5 + term and points `term` tables into the gas's block, and is NULL exactly for a term >= NEXP and for
    an all-zero table.  The fixture facts the GPU tests lean on are asserted here: axes of 9 / 31 / 12 nodes, 42 of 49 layers
    below the top of the pressure table, temperatures above the table's 320 K, 7 or 12 absorbing pairs per wavelength."""
    A, S = pkg.absorption, pkg.solver
    preps = _fixture_preps(A)
    base = lambda prep, k: 0x7f0000000000 + 0x1000000 * (k + 1) + 8 * int(prep["lamb1"])
    xk_off = [5000, 0, 9000, 2500]
    for offs, shift in ((None, 0), (xk_off, 123)):
        pk = S.pack_ckd_requests(preps, base, xk_off=offs, base=shift)
        wl, ax, slots = pk["wl"], pk["axes"], pk["slots"].reshape(len(preps), 8, 5)
        assert wl.dtype == S.CKD_WL_DTYPE and wl.flags.c_contiguous and slots.dtype == np.uint64 and ax.dtype == np.float64
        assert pk["nlay"] == 49 and pk["nterm"] == 5
        for w, p in enumerate(preps):
            e = wl[w]
            assert (e["nterm"], e["nt"], e["np"], e["nc"]) == (5, 9, 31, 12)
            cut = lambda k, n: ax[int(e[k]) - shift:int(e[k]) - shift + n]
            assert np.array_equal(cut("pres_off", 31), p["tab_pres"]) and np.array_equal(cut("temp_off", 9), p["tab_temp"])
            assert np.array_equal(cut("conc_off", 12), p["tab_conc"])
            prs, tmp, conc = A.layer_state(p)
            assert np.array_equal(cut("prs_off", 49), prs) and np.array_equal(cut("tmp_off", 49), tmp)
            assert np.array_equal(cut("cl_off", 49), conc)
            assert int((prs > p["tab_pres"][0]).sum()) == 42 and tmp.max() > p["tab_temp"][-1] == 320.0
            assert e["xk_off"] == (1960 * w if offs is None else offs[w])
            pairs = 0
            for k in range(8):
                per = p["ki"][k][0].size * 8
                assert per == (12 if k == 0 else 1) * 31 * 9 * 8
                for term in range(5):
                    live = term < p["nexp"][k] and bool(p["ki"][k][term].any())
                    pairs += live
                    assert int(slots[w, k, term]) == (base(p, k) + term * per if live else 0), (w, k, term)
            assert pairs in (7, 12) and pairs == len(A._absorbing_pairs(p))
        assert pk["out_doubles"] == (4 * 1960 if offs is None else 9000 + 1960)
        assert ax.size <= 2 * (31 + 9 + 12) + 4 * 3 * 49          # shared axes and atmospheres are packed once
    # the layer state is the first statements of the scalar checker: its clamped form gives that checker's tables
    xk, ro = A.layer_tables_scalar(preps[1])
    assert np.array_equal(ro, A.layer_ro(preps[1])) and np.array_equal(A.layer_tables(preps[1])[0], xk)


def test_prefetch_can_leave_the_layer_tables_to_the_device(pkg, fic):
    A = pkg.absorption
    reqs = [(0.762, 10.0, 1013.0, -999., -999., -999., -999., 2, None), (1.0e4 / 15925.0, 10.0, 1013.0, 2.5, -999., -999., -999., 1, None)]
    try:
        assert A.prefetch_gas_tables(reqs, device_tables=reqs[1:]) == 2
        assert "_layer_tables" in A.prepa_absprofile(*reqs[0]) and "_layer_tables" not in A.prepa_absprofile(*reqs[1])
    finally:
        A.drop_prefetched_gas_tables()


def _entry(pkg, **kw):
    e = dict(pres_off=0, temp_off=31, conc_off=40, prs_off=52, tmp_off=101, cl_off=150, xk_off=0, nterm=5, nt=9, np=31, nc=12)
    e.update(kw)
    return pkg.capi.CkdWl(**e)


def test_argument_rules_and_limits_before_any_device_work(pkg):
    """SOSGPU_E_ARG (-1) for the argument rules, SOSGPU_E_UNSUPPORTED (-3) for the limits, the offending wavelength in *bad_wl;
    every call here is refused before the device is looked at (none of the pointers is real)."""
    L = pkg.capi.lib()
    fake = C.c_void_p(0x1000)
    slots = (C.c_uint64 * 80)()

    def call(entries, nslots=None, nlay=49, axes=199, out=2 * 1960, **nulls):
        wl = (pkg.capi.CkdWl * len(entries))(*entries)
        bad = C.c_int(-7)
        a = dict(wl=wl, ki=slots, d_axes=fake, d_work=fake, d_out=fake, d_status=fake)
        a.update(nulls)
        rc = L.sosgpu_ckd_layer_tables(0, len(entries), a["wl"], 40 * len(entries) if nslots is None else nslots, a["ki"],
                                       a["d_axes"], axes, nlay, a["d_work"], 1 << 30, a["d_out"], out, a["d_status"],
                                       C.byref(bad), None)
        return rc, bad.value

    ok = _entry(pkg)
    for name in ("wl", "ki", "d_axes", "d_work", "d_out", "d_status"):
        assert call([ok], **{name: None}) == (-1, -1), name
    assert call([ok], d_work=C.c_void_p(0x1004)) == (-1, -1)                       # work area not 8-byte aligned
    assert L.sosgpu_ckd_layer_tables(0, 0, None, 0, None, None, 0, 49, None, 0, None, 0, None, None, None) == -1
    assert call([ok, ok], nslots=79) == (-1, -1)                                   # nslots != sum of 8 * nterm
    assert call([ok, _entry(pkg, nterm=0)]) == (-1, 1)
    for k in ("pres_off", "temp_off", "conc_off", "prs_off", "tmp_off", "cl_off", "xk_off"):
        assert call([ok, ok, _entry(pkg, **{k: -1})], out=3 * 1960) == (-1, 2), k
    assert call([ok, _entry(pkg, cl_off=151)]) == (-1, 1)                          # conc[49] ends one double past d_axes
    assert call([_entry(pkg, pres_off=169)]) == (-1, 0)
    assert call([ok, _entry(pkg, xk_off=1961)]) == (-1, 1)                         # xk block ends past d_out
    for kw in (dict(nt=1), dict(nt=17), dict(np=1), dict(np=65), dict(nc=1), dict(nc=17)):
        assert call([ok, _entry(pkg, **kw)]) == (-3, 1), kw
    for nlay in (0, 64, -1):
        assert call([ok], nlay=nlay)[0] == -3, nlay


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_fixture_tables_equal_the_scalar_restatement(gpu_pkg, fic):
    """The four wavelengths of absorption.npz in one launch, and each alone: xk equals layer_tables_scalar, ro layer_tables',
    status 0.  1960 entries per wavelength, all but the 42 active layers of 7 or 12 pairs are zeros."""
    import torch
    A, S = gpu_pkg.absorption, gpu_pkg.solver
    preps, ref = _scalar_tables(A)
    A.drop_ckd_device_tables()
    xk, ro, status = S.ckd_layer_tables(preps, 0)
    torch.cuda.synchronize()
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0, 0, 0, 0]
    for w, (x, (xs, rs)) in enumerate(zip(xk, ref)):
        assert tuple(x.shape) == (8, 5, 49) and x.dtype == torch.float64
        got = x.cpu().numpy()
        assert same(got, xs), w
        assert np.array_equal(ro[w], rs)
        pairs = len(A._absorbing_pairs(preps[w]))
        assert pairs in (7, 12) and 100 < (got != 0).sum() <= pairs * 42 and got.size == 1960
    for w, p in enumerate(preps):
        x1, r1, s1 = S.ckd_layer_tables([p], 0, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        assert same(x1[0].cpu().numpy(), ref[w][0]) and s1.cpu().tolist() == [0]


def _rand_tables(rng, T, P, Cc, nterm, slots):
    tabs = {}
    for g, term in slots:
        shape = ((len(Cc),) if g == 0 else ()) + (len(P), len(T))
        tabs[(g, term)] = ckd_cells.smooth_table(rng, shape)
    return tabs


SHAPES = [  # nt, np, nc, nlay, nterm, slots with a table
    (2, 2, 2, 1, 1, [(0, 0), (6, 0)]),
    (3, 31, 12, 49, 5, [(0, 0), (0, 4), (2, 1), (6, 3), (7, 4)]),
    (9, 64, 16, 63, 5, [(0, 2), (1, 0), (6, 4)]),
    (16, 2, 2, 63, 1, [(0, 0), (3, 0)]),
    (16, 64, 16, 49, 5, [(0, 1), (5, 2)]),
    (9, 31, 12, 63, 1, [(0, 0), (7, 0)]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "nt%d_np%d_nc%d_nlay%d_nterm%d" % s[:5])
def test_synthetic_cells_on_every_edge_of_the_searches(gpu_pkg, shape):
    """Axis lengths at both limits and at the reference's, 1 / 49 / 63 layers, 1 and 5 terms; layer states on every edge of the
    three bracket searches (ckd_cells.edge_states).  Every slot without a table comes back +0.0."""
    A = gpu_pkg.absorption
    nt, npr, nc, nlay, nterm, slots = shape
    rng = np.random.default_rng(nt * 1000 + npr * 10 + nlay)
    T, P, Cc = ckd_cells.axes(nt, npr, nc)
    prs, tmp, conc = ckd_cells.edge_states(T, P, Cc, nlay)
    if nlay >= 49:
        assert (prs == P[0]).any() and (prs == np.nextafter(P[0], np.inf)).any() and (prs == P[-1]).any() and (prs > P[-1]).any()
        assert (tmp < T[0]).any() and (tmp > T[-1]).any() and all((tmp == t).any() for t in T[:min(nt, 9)])
        assert (conc < Cc[0]).any() and (conc > Cc[-1]).any() and (conc == Cc[len(Cc) // 2]).any()
    cell = ckd_cells.make_cell(T, P, Cc, nterm, _rand_tables(rng, T, P, Cc, nterm, slots), prs, tmp, conc)
    ref, st = ckd_cells.reference(A, cell)
    assert st == 0 and np.isfinite(ref).all()
    out, status = ckd_cells.run(gpu_pkg, [cell])
    assert status.tolist() == [0]
    assert same(out.reshape(8, nterm, nlay), ref)
    if nlay >= 49:
        assert (ref[[g for g, _ in slots], [t for _, t in slots]] == 0).any() and (ref != 0).sum() > 20


def _spike_cells():
    """Three wavelengths on the reference's 9-point axis: the spike table (the spline undershoots at 215 and 265 K, the linear
    fallback gives 0 there), its negation (ERROR_923) in the middle, and a smooth one."""
    T, P, Cc = ckd_cells.axes(9, 31, 12)
    spike = np.zeros((31, 9))
    spike[:, 4] = 1.0
    tmp = np.array([215.0, 225.0, 250.0, 265.0])
    prs = np.array([500.0, 30.0, 900.0, 2000.0])
    conc = np.full(4, 1e-3)
    rng = np.random.default_rng(7)
    smooth = _rand_tables(rng, T, P, Cc, 1, [(0, 0), (6, 0)])
    mk = lambda tabs: ckd_cells.make_cell(T, P, Cc, 1, tabs, prs, tmp, conc)
    return mk({(6, 0): spike, (0, 0): np.broadcast_to(spike, (12, 31, 9))}), mk({(6, 0): -spike}), mk(smooth)


@pytest.mark.gpu
def test_negative_spline_takes_the_linear_fallback_and_error_923_is_per_wavelength(gpu_pkg):
    A = gpu_pkg.absorption
    good, neg, smooth = _spike_cells()
    # the branch is really taken: the spline alone is negative at 215 and 265 K, the fallback returns exactly 0 there
    y = np.zeros(9)
    y[4] = 1.0
    sp = [A.interpo_splint(good["T"], y, t) for t in good["tmp"]]
    assert sp[0] < -0.12 and sp[3] < -0.12 and abs(sp[1] - 0.269) < 1e-3 and abs(sp[2] - 0.600) < 1e-3
    ref_good, st_good = ckd_cells.reference(A, good)
    assert st_good == 0 and ref_good[6, 0].tolist() == [0.0, sp[1], sp[2], 0.0]
    ref_neg, st_neg = ckd_cells.reference(A, neg)
    ref_smooth, st_smooth = ckd_cells.reference(A, smooth)
    assert st_neg == 2 and st_smooth == 0
    out, status = ckd_cells.run(gpu_pkg, [good, neg, smooth])
    assert status.tolist() == [0, 2, 0]
    out = out.reshape(3, 8, 1, 4)
    assert same(out[0], ref_good) and same(out[2], ref_smooth)
    # ... and the neighbours alone give the same doubles: the failing wavelength touched nothing of theirs
    alone, st = ckd_cells.run(gpu_pkg, [good, smooth])
    assert st.tolist() == [0, 0] and same(alone.reshape(2, 8, 1, 4)[0], out[0]) and same(alone.reshape(2, 8, 1, 4)[1], out[2])


@pytest.mark.gpu
def test_large_end_slopes_and_duplicated_temperature_node(gpu_pkg):
    """Entries of 1e32 make the end slopes exceed .99E30: SOS_SPLINE's other branch at either end (column 1 raises the first
    slope; the last slope is raised by the last column -- 1e32 in column nt-2 alone makes it negative).  A duplicated
    temperature node bracketing the layer's temperature gives status 1."""
    A = gpu_pkg.absorption
    T, P, Cc = ckd_cells.axes(9, 31, 12)
    big = float(np.float32(.99E30))
    rng = np.random.default_rng(11)
    t1 = ckd_cells.smooth_table(rng, (31, 9), scale=1.0)
    t1[:, 1] = 1e32
    t1[:, 7] = 1e32                                        # the issue's table: columns 1 and nt-2
    t2 = ckd_cells.smooth_table(rng, (31, 9), scale=1.0)
    t2[:, 8] = 1e32                                        # the last slope
    t3 = np.broadcast_to(t2, (12, 31, 9)).copy()
    t3[..., 1] = 1e32                                      # both, through the concentration interpolation as well
    prs, tmp, conc = ckd_cells.edge_states(T, P, Cc, 49)
    cell = ckd_cells.make_cell(T, P, Cc, 1, {(1, 0): t1, (6, 0): t2, (0, 0): t3}, prs, tmp, conc)
    d = T[1] - T[0]
    assert (t1[:, 1] - t1[:, 0]).min() / d > big and (t2[:, 8] - t2[:, 7]).min() / d > big and (t1[:, 8] - t1[:, 7]).max() < 0
    ref, st = ckd_cells.reference(A, cell)
    assert st == 0 and np.isfinite(ref).all() and ref.max() > 1e30
    out, status = ckd_cells.run(gpu_pkg, [cell])
    assert status.tolist() == [0] and same(out.reshape(8, 1, 49), ref)
    # duplicated node: T = 160, 240, 320, 320 and layers at and above 320 K -- SOS_SPLINT's bisection ends on the bracket
    # 320..320, h = 0 -- next to a clean wavelength
    Td = np.array([160.0, 240.0, 320.0, 320.0])
    tab = ckd_cells.smooth_table(rng, (31, 4))
    dup = ckd_cells.make_cell(Td, P, Cc, 1, {(6, 0): tab}, [500.0, 600.0], [320.0, 400.0], [1e-3, 1e-3])
    clean = ckd_cells.make_cell(T[:4], P, Cc, 1, {(6, 0): tab}, [500.0, 600.0], [320.0, 400.0], [1e-3, 1e-3])
    assert ckd_cells.reference(A, dup)[1] == 1
    ref_clean, st_clean = ckd_cells.reference(A, clean)
    out, status = ckd_cells.run(gpu_pkg, [dup, clean])
    assert st_clean == 0 and status.tolist() == [1, 0] and same(out.reshape(2, 8, 1, 2)[1], ref_clean)


@pytest.mark.gpu
def test_mixed_launch_writes_its_blocks_and_nothing_else(gpu_pkg):
    """One launch of wavelengths with different nterm and axis lengths into one block at non-contiguous xk_off: every entry of
    a wavelength's block is written (the block was NaN), every double between the blocks is still NaN."""
    A = gpu_pkg.absorption
    nlay = 49
    rng = np.random.default_rng(3)
    specs = [(9, 31, 12, 5, [(0, 0), (6, 4)]), (2, 2, 2, 1, [(0, 0)]), (16, 64, 16, 3, [(0, 2), (4, 1)]), (3, 5, 4, 2, [])]
    cells = []
    for nt, npr, nc, nterm, slots in specs:
        T, P, Cc = ckd_cells.axes(nt, npr, nc)
        cells.append(ckd_cells.make_cell(T, P, Cc, nterm, _rand_tables(rng, T, P, Cc, nterm, slots),
                                         *ckd_cells.edge_states(T, P, Cc, nlay)))
    sizes = [8 * c["nterm"] * nlay for c in cells]
    xk_off = [3000, 7, 5200, 0]                              # (not in launch order; gaps of 7 .. 392 doubles; one of 0)
    xk_off[3] = xk_off[1] + sizes[1]
    total = max(o + n for o, n in zip(xk_off, sizes)) + 11
    out, status = ckd_cells.run(gpu_pkg, cells, xk_off=xk_off, out_doubles=total)
    assert status.tolist() == [0, 0, 0, 0]
    written = np.zeros(total, dtype=bool)
    for c, o, n in zip(cells, xk_off, sizes):
        assert not written[o:o + n].any()
        written[o:o + n] = True
        assert same(out[o:o + n].reshape(8, c["nterm"], nlay), ckd_cells.reference(A, c)[0])
    assert (~written).sum() >= 18 and np.isnan(out[~written]).all() and not np.isnan(out[written]).any()


@pytest.mark.gpu
def test_resident_cache_uploads_each_file_once(gpu_pkg, tmp_path, monkeypatch):
    """A second call for the same files uploads nothing; a file whose size and mtime change is uploaded again; eviction at a
    small byte budget leaves the results unchanged."""
    import torch
    A, S = gpu_pkg.absorption, gpu_pkg.solver
    preps, ref = _scalar_tables(A)
    n = dict(up=0)
    up0 = A._ckd_upload

    def counting(ki, device):
        n["up"] += 1
        return up0(ki, device)

    monkeypatch.setattr(A, "_ckd_upload", counting)
    A.drop_ckd_device_tables()
    check = lambda res: all(same(x.cpu().numpy(), r[0]) for x, r in zip(res[0], ref)) and res[2].cpu().tolist() == [0] * 4
    assert check(S.ckd_layer_tables(preps, 0))
    assert n["up"] == 16                                   # eight gases, two spectral files each
    assert check(S.ckd_layer_tables(preps, 0)) and S.ckd_layer_tables(preps[::-1], 0)[2].cpu().tolist() == [0] * 4
    assert n["up"] == 16
    # a changed file: a copy of the tree whose O2 file grows by a trailing blank line
    root = tmp_path / "abs"
    shutil.copytree(os.path.join(GOLD, "fic"), str(root / "fic"))
    monkeypatch.setenv("SOS_ABS_ROOT", str(root))
    args = (0.762, 10.0, 1013.0, -999., -999., -999., -999., 2)
    p1 = A.prepa_absprofile(*args)
    x1, _, s1 = S.ckd_layer_tables([p1], 0)
    assert n["up"] == 24 and same(x1[0].cpu().numpy(), ref[0][0])
    S.ckd_layer_tables([A.prepa_absprofile(*args)], 0)
    assert n["up"] == 24
    f = root / "fic" / "COEFF_CKD" / "10cmm1" / "coef_O2_13500_13000_10cmm1"
    with open(str(f), "a") as fh:
        fh.write("\n")
    st = os.stat(str(f))
    os.utime(str(f), ns=(st.st_atime_ns, st.st_mtime_ns + 2_000_000_000))
    x2, _, s2 = S.ckd_layer_tables([A.prepa_absprofile(*args)], 0)
    assert n["up"] == 25 and same(x2[0].cpu().numpy(), ref[0][0])
    # eviction: a budget smaller than one H2O file keeps a single file resident
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.setattr(A, "CKD_DEVICE_BUDGET", 100_000)
    A.drop_ckd_device_tables()
    before = n["up"]
    assert check(S.ckd_layer_tables(preps, 0)) and len(A._CKD_DEV) == 1
    assert check(S.ckd_layer_tables(preps, 0)) and n["up"] >= before + 30
    torch.cuda.synchronize()
    A.drop_ckd_device_tables()


def _gas_requests(A, with_prep):
    """Profile requests of the four fixture wavelengths (and one without gas in between), tables from the host or `prep`."""
    preps, _ = _scalar_tables(A)
    reqs = []
    for w, p in enumerate(preps):
        ik, aik, _ = A.bins(p)
        r = dict(tr=0.0948 - 0.01 * w, hr=8.0, ta=0.3 if w % 2 else 0.0, ha=2.0 if w % 2 else 1.0, a_tronc=0.0,
                 piz=1.0 if w % 2 else 0.0, piztr=1.0 if w % 2 else 0.0, zout=-1.0 if w < 2 else 3.0, smax=16, ik=ik,
                 ro=A.layer_ro(p), altabs=p["altabs"], absprofil=int(p["absprofil"]))
        if with_prep and w != 2:
            r["prep"] = p                                   # (wavelength 2 keeps host tables: the two kinds mix in one part)
        else:
            r["xk"] = A.layer_tables(p)[0]
        reqs.append(r)
    reqs.insert(1, dict(tr=0.0948, hr=8.0, ta=0.3, ha=2.0, ik=None, absprofil=7, smax=16, a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0))
    return reqs


@pytest.mark.gpu
def test_make_profiles_spectrum_with_prep_equals_host_tables(gpu_pkg, fic):
    """Requests carrying `prep` against the same requests with host xk: tabs, prof, nt, iborm, zprof, scal bit for bit, on two
    streams; the status tensor speaks of the prep requests, in order."""
    import torch
    A, S = gpu_pkg.absorption, gpu_pkg.solver
    host_info = {}
    host = S.make_profiles_spectrum(_gas_requests(A, False), 0, part=host_info)
    torch.cuda.synchronize()
    assert host_info["ckd_status"] is None
    for attempt in range(2):
        st = torch.cuda.Stream()
        info = {}
        got = S.make_profiles_spectrum(_gas_requests(A, True), 0, stream=st, part=info)
        st.synchronize()
        assert info["ckd_index"] == [0, 2, 4] and info["ckd_status"].cpu().tolist() == [0, 0, 0]
        for w, (g, h) in enumerate(zip(got, host)):
            for k in ("prof", "nt", "iborm", "zprof", "scal"):
                assert torch.equal(g[k], h[k]), (attempt, w, k)
            for k in ("jout", "zz"):
                assert (g[k] is None) == (h[k] is None) and (g[k] is None or torch.equal(g[k], h[k])), (attempt, w, k)
            if host_info["tabs"][w] is None:
                assert info["tabs"][w] is None
            else:
                assert torch.equal(info["tabs"][w], host_info["tabs"][w]), (attempt, w)
                assert float(info["tabs"][w][:, -1].max()) > 0.0


END_TO_END = ["ckd_o2a_5bins", "ckd_h2o_o2_25bins_flatsea", "cfg1_lambert", "cfg5_ckd_maignan_25bins", "ckd_userprofile_25bins",
              "cfg2_lnd_lambert"]


def _watch(monkeypatch, pkg):
    """Wrappers round the host interpolation and the batched profile stage: which wavelengths (by wavenumber) were interpolated
    on the host, which were handed over with `prep`, which with host xk."""
    A, S = pkg.absorption, pkg.solver
    seen = dict(host={}, prep={}, xk=0)            # (the preps themselves are kept: an id stays its own)
    many0, one0, batch0 = A.layer_tables_many, A.layer_tables, S.make_profiles_spectrum

    def many(preps):
        seen["host"].update((id(p), p) for p in preps if p.get("_layer_tables") is None)
        return many0(preps)

    def one(prep):
        if prep.get("_layer_tables") is None:
            seen["host"][id(prep)] = prep
        return one0(prep)

    def batch(requests, *a, **k):
        for r in requests:
            if r.get("ik") is not None and r.get("xk") is None:
                seen["prep"][id(r["prep"])] = r["prep"]
            elif r.get("ik") is not None:
                seen["xk"] += 1
        return batch0(requests, *a, **k)

    monkeypatch.setattr(A, "layer_tables_many", many)
    monkeypatch.setattr(A, "layer_tables", one)
    monkeypatch.setattr(S, "make_profiles_spectrum", batch)
    return seen


@pytest.fixture(scope="module")
def sequential(tmp_path_factory):
    """sos_proc of the end-to-end calls, one after the other: computed once, shared."""
    import importlib
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    os.environ["SOS_ABS_ROOT"], old = GOLD, os.environ.get("SOS_ABS_ROOT")
    try:
        kws, _, _, _ = spectrum_cases.build(rs, tmp_path_factory.mktemp("e2e"), names=END_TO_END)
        seq = [rs.sos_proc(**kw) for kw in kws]
    finally:
        if old is None:
            del os.environ["SOS_ABS_ROOT"]
        else:
            os.environ["SOS_ABS_ROOT"] = old
    return kws, seq


@pytest.mark.gpu
@pytest.mark.parametrize("host_tables", [False, True], ids=["device_tables", "host_switch"])
def test_spectrum_equals_sequential_calls_bitwise(gpu_pkg, sequential, monkeypatch, host_tables):
    """sos_spectrum (one chunk and chunk=3) equals sequential sos_proc on all 23 outputs with the gas tables made on the device,
    and with SOS_SPECTRUM_HOST_GAS_TABLES=1.  The host interpolation runs for no deferred wavelength by default (the two
    -SOS.Trans calls are not deferred: they keep it) and for every one of them under the switch."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_PROFILES_PER_CALL", raising=False)
    if host_tables:
        monkeypatch.setenv("SOS_SPECTRUM_HOST_GAS_TABLES", "1")
    else:
        monkeypatch.delenv("SOS_SPECTRUM_HOST_GAS_TABLES", raising=False)
    kws, seq = sequential
    gas = [kw for kw in kws if int(kw["absprofil"]) != 7]
    trans = [kw for kw in gas if str(kw["fictrans"]).strip() != "NO_OUTPUT"]
    assert len(gas) == 4 and len(trans) == 2 and len(kws) == 6
    seen = _watch(monkeypatch, gpu_pkg)
    for a, b in zip(seq, rs.sos_spectrum(kws)):
        assert_tuples_equal(a, b)
    if host_tables:
        assert not seen["prep"] and seen["xk"] == 2 and len(seen["host"]) == 4
    else:
        assert len(seen["prep"]) == 2 and seen["xk"] == 0
        assert not (set(seen["host"]) & set(seen["prep"])) and len(seen["host"]) == 2            # only the two -SOS.Trans calls
    for a, b in zip(seq, rs.sos_spectrum(kws, chunk=3)):
        assert_tuples_equal(a, b)


@pytest.mark.gpu
def test_spectrum_levels_equal_sos_proc_per_altitude(gpu_pkg, sequential, monkeypatch):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_HOST_GAS_TABLES", raising=False)
    kws, seq = sequential
    alts = [-1, 0.0, 3.0]
    sub = [dict(kw, zout=-1.0) for kw in (kws[1], kws[2])]                  # a deferred gas call and a no-gas call
    lev = rs.sos_spectrum_levels(alts, sub)
    for i, kw in enumerate(sub):
        for k, z in enumerate(alts):
            assert_tuples_equal(rs.sos_proc(**dict(kw, zout=float(z))), lev[i][k])


def _negate_interval(path, nu, nustep=10.0):
    """Rewrite the CKD file at `path` (a gas other than H2O) with the coefficients of the interval holding wavenumber nu
    negated: the walk of absorption._read_ckd_file over the records."""
    lines = open(path).read().splitlines()
    pos = 18

    def rec(n):
        nonlocal pos
        vals = []
        while len(vals) < n:
            vals += lines[pos].replace(",", " ").split()
            pos += 1
        return vals

    numax, numin, res = (float(v) for v in rec(3)[:3])
    nt = int(rec(1)[0]); rec(nt)
    npr = int(rec(1)[0]); rec(npr)
    target = int((numax - nu) / nustep)
    done = 0
    for iwa in range(int((numax - numin) / res)):
        nmax = int(rec(6)[5])
        if nmax == 0:
            continue
        rec(nmax)
        for r in range(nmax * npr):
            if iwa == target:
                tok = lines[pos + r].split()
                lines[pos + r] = " ".join(tok[:2] + [repr(-float(v)) for v in tok[2:2 + nt]])
                done += 1
        pos += nmax * npr
    assert done > 0
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_error_923_in_a_spectrum_is_the_error_of_the_call_alone(gpu_pkg, tmp_path, monkeypatch):
    """A table tree whose O2 coefficients of the O2-A interval are negated: sos_proc of that call raises SosProcError with the
    ERROR_923 message; sos_spectrum with the call in the middle of a list raises the same class, message and ier; a following
    sos_spectrum of the good calls is right."""
    rs = gpu_pkg.run_sos
    root = tmp_path / "abs"
    shutil.copytree(os.path.join(GOLD, "fic"), str(root / "fic"))
    _negate_interval(str(root / "fic" / "COEFF_CKD" / "10cmm1" / "coef_O2_13500_13000_10cmm1"), 1.0e4 / 0.762)
    monkeypatch.setenv("SOS_ABS_ROOT", str(root))
    monkeypatch.delenv("SOS_SPECTRUM_HOST_GAS_TABLES", raising=False)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=["cfg2_lnd_lambert", "ckd_h2o_o2_25bins_flatsea", "ckd_o2a_5bins",
                                                             "cfg1_lambert"])
    kws[2] = dict(kws[2], fictrans="NO_OUTPUT")            # (deferred: its tables are the device's)
    bad, good = kws[2], [kws[0], kws[1], kws[3]]
    with pytest.raises(rs.SosProcError) as alone:
        rs.sos_proc(**bad)
    assert alone.value.ier == -1 and "ERROR_923" in str(alone.value)
    seen = _watch(monkeypatch, gpu_pkg)
    with pytest.raises(rs.SosProcError) as inlist:
        rs.sos_spectrum(kws)
    assert len(seen["prep"]) == 2 and not seen["host"] and seen["xk"] == 0      # the device found it, not the host
    assert type(inlist.value) is type(alone.value) and str(inlist.value) == str(alone.value)
    assert inlist.value.ier == alone.value.ier
    outs = rs.sos_spectrum(good)
    for kw, o in zip(good, outs):
        assert_tuples_equal(rs.sos_proc(**kw), o)
