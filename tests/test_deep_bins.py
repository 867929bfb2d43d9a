"""The full solve -- all Fourier orders, polarisation, a reflecting ground, output altitudes and output slots -- of optically
deep bins against the C oracle in every layout of the single-context solver, with BOTH halves of every record held to the
oracle (deep_cells.py).

Real CKD bands hold bins of total optical depth 30 to several hundred.  test_variant_matrix stays below 2.5 and
test_uneven_grids reaches 20 in one ground layer; deeper bins ran only through Fourier order 0 over a black ground
(test_incidence_sweep), where they found a defect (conv_exceeds).  The full solve has more: orders above 0 and
SOS_ARRET_FOURIER, the ground coupling under a direct beam of exp(-tau / mus) ~ 1e-212, the output altitude and the output
slots, the record store, a scattering loop of up to 70 orders, the band aggregate next to transparent bins.

And the suite's record bar cannot see one half of such a bin: cases.compare_records allows 1e-9 |ref| + 1e-12 max |I| with
the maximum over the whole record, and from depth 30 on the down half is below 1e-13 of the up half, so anything finite
passes there (test_whole_record_bar_is_blind_from_depth_30).  deep_cells.compare_halves takes the scale of each half from
that half.

Cells: one per row of incidence_cells.LAYOUT_TABLE, seven bins of NT = lp - 1 at total depths 0.4 ... 400.4 (tau / mus <=
489), the sun on an interior direction, grounds Lambert / Fresnel / matrices in turn, one cell without polarisation, output
altitudes 7 km (mid-layer everywhere, depth ~35 above it at k = 200) and `zlev` (a level of the k = 200 bin).

CPU: the cells are what they claim; the oracle decides every solve the GPU tests use (ier = 0, finite, tie margin > 1e-7);
the whole-record bar is blind from k = 30 where the per-half bar is not; one ulp on every cosine stays below 1e-2 of the
per-half bar.  GPU: every route through solve (ZOUT = -1 and an interior altitude), the output slots, the streamed launch
forms bit for bit, a two-context table, the band of the seven bins.

No bound here comes from the kernels: the bar is the project's 1e-9 with its 1e-12 floor, applied per half; the figures of
the CPU tests are measured on the oracle alone (profiles/deep_bins_parity.txt)."""
import numpy as np
import pytest

import cases
import deep_cells as dc
import test_variant_matrix as vm

S = cases.S
MARGIN = 1e-7                                   # the tie margin test_oracle asks of a decided solve
SOLVES = ("plain", "mid", "lev", "levels")      # what the GPU tests compare with, per cell


def _queue_all(oracle):
    for c in dc.CELLS:
        for what in SOLVES:
            dc.queue(oracle, c, what)
    for name in dc.TWIN_CELLS:
        dc.queue(oracle, dc.by_name(name), "g2")


def _what(c, k, zout=-1.0):
    return "%s (%s) bin %d k=%g NT=%d zout=%g" % (c["name"], c["route"], k, c["k_abs"][k], c["nt"][k], zout)


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_cells_reach_their_layouts(pkg, monkeypatch):
    """The routes are the library's: the single-context plan names the layout of every cell (needs the built library)."""
    monkeypatch.delenv("SOSGPU_STREAM_PERSIST", raising=False)                    # (route reads the plan as a solve would)
    for c in dc.CELLS:
        assert vm.route(c["n"], c["lp"]) == c["layout"], (c["name"], vm.route(c["n"], c["lp"]))


def test_cells_are_what_they_claim():
    assert len(dc.CELLS) == 12 and len(set(dc.NAMES)) == 12
    assert {c["layout"] for c in dc.CELLS} == set(vm.LAYOUTS) and len(dc.STREAMED) == 5
    assert dc.K_ABS == (0.0, 3.0, 10.0, 30.0, 100.0, 200.0, 400.0) and len(dc.DEPTHS) == 7
    assert abs(dc.AIK.sum() - 1.0) < 1e-15 and len(set(dc.AIK.tolist())) > 3 and len(dc.AIK) == 7
    grounds, ipolar0, worst = set(), [], 0.0
    for c in dc.CELLS:
        n, lp, fam = c["n"], c["lp"], c["layout"].split("<")[0]
        if ":" in c["route"]:
            assert (vm._round_up(3 * n, 8) + 15) // 16 == int(c["route"].split(":")[1])
        mu, w, n0 = S.gauss_angles(n - 1, 35.0)
        assert np.array_equal(mu, c["mu"]) and np.array_equal(w, c["w"]) and n0 == c["n0"] and 1 < n0 < n
        assert c["os_nb"] == 16 and np.all(c["iborm"] == 16) and c["zout"] == -1.0
        assert c["nt"].tolist() == [lp - 1] * 7 and vm._round_up(lp, 16) == lp
        for k, (h, x, y, z) in enumerate(c["bins"]):
            what = (c["name"], c["k_abs"][k])
            assert len(h) == lp and np.all(np.diff(h) > 0) and h[0] >= 0, what
            assert np.all(np.diff(z) < 0) and z[0] == 120.0 and z[-1] == 0.0, what
            assert np.all((x >= 0) & (y >= 0) & (x + y <= 1)), what
            assert abs(h[-1] - dc.DEPTHS[k]) < 0.05, (what, h[-1])            # (0.352 + k: the truncation takes 0.048)
            assert h[-1] / mu[n0 - 1] < dc.TAU_MUS_MAX, what                      # (beyond it the reference returns NaN)
            worst = max(worst, h[-1] / mu[n0 - 1])
            # both interior altitudes lie inside the grid: 7 km between two levels of every bin, zlev a level of one bin only
            assert z[-1] < c["zlev"] < z[0] and z[-1] < dc.Z_MID < z[0], what
            assert dc.Z_MID not in z, what
            assert (c["zlev"] in z) == (c["k_abs"][k] == dc.K_ZLEV), what
        k200 = c["k_abs"].index(dc.K_ZLEV)
        h, _, _, z = c["bins"][k200]
        assert c["zlev"] == z[(lp - 1) // 2] and 2.7 < c["zlev"] < 3.0, (c["name"], c["zlev"])
        j = int(np.searchsorted(-z, -dc.Z_MID))
        assert 30.0 < h[j - 1] < h[j] < 40.0, (c["name"], h[j - 1], h[j])        # the depth above 7 km in the k = 200 bin
        assert c["alts"] == [-1.0, 7.0, c["zlev"], 0.0] and c["zo"] == (7.0 if c["i"] % 2 == 0 else c["zlev"])
        kw = c["kw"]
        kind = "matrices" if kw.get("imat_surf") else "fresnel" if kw.get("ifresnel") else "lambert"
        assert kw["ro"] == dict(lambert=0.1, fresnel=0.05, matrices=0.02)[kind] and kind == ("lambert", "fresnel", "matrices")[c["i"] % 3]
        if kind == "matrices":
            assert np.array_equal(kw["rsurf"], cases._surf_matrices(n, 16, 71 + c["i"]))
        if kind == "fresnel":
            assert kw["ind_surf"] == 1.34
        grounds.add((fam, kind))
        if kw["ipolar"] == 0:
            ipolar0.append(c["layout"])
    assert worst < 489.5, worst
    assert grounds == {(f, g) for f in ("os", "stream") for g in ("lambert", "fresnel", "matrices")}
    assert ipolar0 == ["os<8,2,2>"]
    assert [dc.by_name(n)["layout"].split("<")[0] for n in dc.TWIN_CELLS] == ["os", "stream"]
    assert [(dc.by_name(n)["n"], dc.by_name(n)["lp"]) for n in dc.CONDITIONING_CELLS] == [(21, 32), (21, 80), (43, 48)]


def test_per_half_bar_is_the_record_bar_on_each_half():
    """compare_halves on literal records: the tolerance of a half is 1e-9 |ref| + 1e-12 max |I| of THAT half over all orders;
    NaN, a non-zero middle column and another order count are mismatches."""
    n = 3
    ref = np.zeros((2, 3, 7))
    ref[:, :, :n] = 1e-40 * np.arange(1, 19).reshape(2, 3, 3)
    ref[:, :, n + 1:] = 0.1 * np.arange(1, 19).reshape(2, 3, 3)
    ref[1, 0, :n] = 5e-39                                                          # the down half's max |I|, at order 1
    assert dc.small_half(ref, n) == "down"
    assert np.allclose(dc.half_tolerance(ref, n, "down"), 1e-9 * np.abs(ref[..., :n]) + 1e-12 * 5e-39, rtol=1e-14, atol=0)
    assert np.allclose(dc.half_tolerance(ref, n, "up"), 1e-9 * np.abs(ref[..., n + 1:]) + 1e-12 * ref[1, 0, 6], rtol=1e-14, atol=0)
    assert max(dc.compare_halves(ref.copy(), ref).values()) == 0.0
    for spoil in (0.0, 0.5, 1.0 + 1e-6):
        got = dc.spoiled(ref, n, spoil)
        assert np.array_equal(got[..., n:], ref[..., n:]) and not np.array_equal(got[..., :n], ref[..., :n])
        cases.compare_records(got, ref, 1e-9, "the whole-record bar")              # blind
        with pytest.raises(AssertionError, match="down half"):
            dc.compare_halves(got, ref)
        assert dc.half_excess(got, ref)["down"] > 1.0 and dc.half_excess(got, ref)["up"] == 0.0
    inside = ref.copy()
    inside[..., :n] *= 1.0 + 5e-10
    assert 0.0 < dc.compare_halves(inside, ref)["down"] < 1.0
    for bad in (np.nan, np.inf):
        got = ref.copy()
        got[0, 2, 1] = bad
        with pytest.raises(AssertionError):
            dc.compare_halves(got, ref)
        assert dc.half_excess(got, ref)["down"] == float("inf")
    got = ref.copy()
    got[1, 1, n] = 1e-300
    with pytest.raises(AssertionError, match="middle column"):
        dc.compare_halves(got, ref)
    with pytest.raises(AssertionError):
        dc.compare_halves(ref[:1], ref)
    got = ref.copy()
    got[0, 1, 5] *= 1.0 + 3e-9
    with pytest.raises(AssertionError, match="up half"):
        dc.compare_halves(got, ref)


def test_oracle_decides_every_solve(oracle):
    """Every solve the GPU tests compare with: ier = 0, everything finite, every stop decision further than 1e-7 from a tie;
    slot -1 of sos_os_levels is the plain solve bit for bit, and the order counts do not depend on the output altitude."""
    _queue_all(oracle)
    worst, deepest = (np.inf, None), (0, None)
    for c in dc.CELLS:
        plain = dc.reference(oracle, c)
        margins = []
        for what in SOLVES + (("g2",) if c["name"] in dc.TWIN_CELLS else ()):
            for k, r in enumerate(dc.reference(oracle, c, what)):
                tag = (c["name"], what, c["k_abs"][k])
                assert r["ier"] == 0 and np.all(np.isfinite(r["records"])), tag
                assert np.isfinite(r["emoins"]) and np.isfinite(r["eplus"]) and r["emoins"] >= 0 and r["eplus"] > 0, tag
                recs = r["records"] if what == "levels" else r["records"][None]
                assert recs.shape[1] >= 4 and len(r["ig_counts"]) == recs.shape[1], (tag, recs.shape)
                assert r["margin"] > MARGIN, (tag, r["margin"])
                margins.append(r["margin"])
                if what != "g2":
                    assert np.array_equal(r["ig_counts"], plain[k]["ig_counts"]), tag
                    assert r["emoins"] == plain[k]["emoins"] and r["eplus"] == plain[k]["eplus"], tag
                if what == "levels":
                    assert np.array_equal(recs[0], plain[k]["records"]), tag
                if r["ig_counts"].max() > deepest[0]:
                    deepest = (int(r["ig_counts"].max()), tag)
        if min(margins) < worst[0]:
            worst = (min(margins), c["name"])
        print("%-20s orders %s  scattering orders %s  tie margin min %.2e" % (
            c["name"], [len(r["records"]) for r in plain], [int(r["ig_counts"].max()) for r in plain], min(margins)))
    print("worst tie margin %.2e (%s); longest scattering loop %d orders %s" % (worst + deepest))
    assert deepest[0] < 100, deepest                                               # (igmax is 100: no series was cut)


def test_whole_record_bar_is_blind_from_depth_30(oracle):
    """The gap this module closes, on the oracle's own records: with the small half set to 0 or multiplied by 1 + 1e-6, a record
    of a bin with k >= 30 passes cases.compare_records against itself and fails compare_halves; for k <= 10 the whole-record
    bar still fails it.  (The small half is the down half: the radiance under the bin.)"""
    for c in dc.CELLS:
        dc.queue(oracle, c)
    for c in dc.CELLS:
        ratios = []
        for k, r in enumerate(dc.reference(oracle, c)):
            ref, n = r["records"], c["n"]
            assert dc.small_half(ref, n) == "down" or c["k_abs"][k] < 3.0, _what(c, k)
            small = np.abs(dc.half(ref[:, 0], n, dc.small_half(ref, n))).max()
            ratios.append(small / np.abs(ref[:, 0]).max())
            for factor in (0.0, 1.0 + 1e-6):
                got = dc.spoiled(ref, n, factor)
                with pytest.raises(AssertionError):
                    dc.compare_halves(got, ref, 1e-9, _what(c, k))
                if c["k_abs"][k] >= dc.K_BLIND:
                    cases.compare_records(got, ref, 1e-9, _what(c, k))
                else:
                    with pytest.raises(AssertionError):
                        cases.compare_records(got, ref, 1e-9, _what(c, k))
        print("%-20s max |I| of the small half / of the record: %s" % (c["name"], " ".join("%.1e" % q for q in ratios)))


def test_one_ulp_on_the_cosines_stays_inside_the_per_half_bar(oracle):
    """The conditioning the per-half bar rests on: every cosine moved up, and down, by one ulp moves no entry of either half
    by more than 1e-2 of that half's tolerance and leaves the order counts alone, at depths 30, 200 and 400 in an LDS-resident
    and two streamed cells.  So a miss at 1e-9 is not the oracle's rounding."""
    moved = []
    for name in dc.CONDITIONING_CELLS:
        c = dc.by_name(name)
        dc.queue(oracle, c)
        for way in (2.0, -2.0):
            mu = np.nextafter(c["mu"], way)
            assert np.all(mu != c["mu"]) and np.all((mu > 0) & (mu <= 1.0))
            for kabs in dc.CONDITIONING_K:
                k = c["k_abs"].index(kabs)
                moved.append((c, k, way, vm._POOL.submit(dc.solve, oracle, c, k, mu=mu)))
    worst = 0.0
    for c, k, way, fut in moved:
        ref, got = dc.reference(oracle, c)[k], fut.result()
        assert got["ier"] == 0 and np.array_equal(got["ig_counts"], ref["ig_counts"]), (_what(c, k), way)
        e = dc.compare_halves(got["records"], ref["records"], 1e-2 * 1e-9, "%s, cosines one ulp %s" % (_what(c, k), "up" if way > 0 else "down"))
        e = {h: 1e-2 * v for h, v in e.items()}                                    # (in units of the 1e-9 bar)
        print("%s, one ulp %-4s: |d record| / tolerance  down %.2e  up %.2e" % (_what(c, k), "up" if way > 0 else "down", e["down"], e["up"]))
        assert max(e.values()) < 1e-2, (_what(c, k), e)
        worst = max(worst, max(e.values()))
    print("one ulp on every cosine, worst |d record| / per-half tolerance: %.2e" % worst)


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _report(label, c, k, got, row, rec, ref, records):
    """The figure first: PARITY <label> <cell> k=<gas depth> down <x the bar> up <x the bar> flux <rel>."""
    f = len(records)
    if int(got["norders"][row]) == f:
        e = dc.half_excess(rec[:f], records)
        flux = max(abs(got["flux"][row, 0] - ref["emoins"]) / max(abs(ref["emoins"]), 1e-300),
                   abs(got["flux"][row, 1] - ref["eplus"]) / abs(ref["eplus"]))
        print("PARITY %-12s %-20s k=%-4g down %.3e up %.3e x the bar; flux %.3e rel (orders %d, scattering orders <= %d)" % (
            label, c["name"], c["k_abs"][k], e["down"], e["up"], flux, f, int(ref["ig_counts"].max())))
    else:
        print("PARITY %-12s %-20s k=%-4g norders %d against %d" % (label, c["name"], c["k_abs"][k], int(got["norders"][row]), f))


def _check_rows(label, c, rows, got, recs, refs, records_of, zout):
    """Every row against its oracle solve under the per-half bar; all figures printed before the first failure is raised."""
    failures = []
    for r, k in enumerate(rows):
        ref = refs[k]
        _report(label, c, k, got, r, recs[r], ref, records_of(ref))
        try:
            dc.assert_bin_vs_oracle(got, r, recs[r], ref, records_of(ref), "%s: %s" % (label, _what(c, k, zout)))
        except AssertionError as err:
            failures.append(str(err)[:400])
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.NAMES)
def test_route_vs_oracle(gpu_pkg, oracle, name):
    """The seven bins of a cell through SosContext.solve at ZOUT = -1, and at the cell's interior altitude (7 km on even
    cells, zlev on odd ones): every bin against the oracle, each half on its own scale."""
    c = dc.by_name(name)
    dc.queue(oracle, c)
    dc.queue(oracle, c, "zo")
    rows = range(len(c["bins"]))
    cx = vm._context(gpu_pkg, c, g=dc.G)
    try:
        plain = vm._fetch(cx.solve(vm._upload(cx, c)))
        zo = vm._fetch(cx.solve(vm._upload(cx, dc.at(c, c["zo"]))))
    finally:
        cx.close()
    for key in ("norders", "iglast", "flux"):                                      # (the output altitude does not enter the solve)
        assert np.array_equal(zo[key], plain[key]), (name, key)
    _check_rows("plain", c, rows, plain, plain["rec"], dc.reference(oracle, c), lambda r: r["records"], -1.0)
    _check_rows("zo", c, rows, zo, zo["rec"], dc.reference(oracle, c, "zo"), lambda r: r["records"], c["zo"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.NAMES)
def test_output_slots_vs_oracle(gpu_pkg, oracle, name):
    """solve_levels with the standard output, 7 km, zlev and 0 km as four slots of one solve: every slot of every bin against
    the oracle per half; slot -1 is the plain solve bit for bit (include/sosgpu.h), and the down half of the 0 km slot is the
    ground half of the plain solve at the bar (one column through two paths, as test_level_flux holds it)."""
    c = dc.by_name(name)
    dc.queue(oracle, c, "levels")
    nb, alts = len(c["bins"]), c["alts"]
    cx = vm._context(gpu_pkg, c, g=dc.G)
    try:
        bins = vm._upload(cx, c)
        lv = cx.output_levels(bins, alts)
        jout, zz = lv["jout"].cpu().numpy(), lv["zz"].cpu().numpy()
        got = vm._fetch(cx.solve_levels(bins, lv))
        plain = vm._fetch(cx.solve(bins))
    finally:
        cx.close()
    k200 = c["k_abs"].index(dc.K_ZLEV)
    assert (jout[0] == 0).all() and (jout[1:] > 0).all() and (jout[3] == c["lp"] - 1).all() and (zz[3] == 1.0).all()
    assert ((zz[1] > 0) & (zz[1] < 1)).all()                                       # 7 km: between two levels of every bin
    assert [z in (0.0, 1.0) for z in zz[2]] == [k == k200 for k in range(nb)]      # zlev: on a level of the k = 200 bin only
    refs = dc.reference(oracle, c, "levels")
    for key in ("norders", "iglast", "flux"):
        assert np.array_equal(got[key], plain[key]), (name, key)
    for k in range(nb):
        f = int(plain["norders"][k])
        assert f > 0 and np.array_equal(got["rec"][0, k], plain["rec"][k]), (name, k)
        dc.compare_half(got["rec"][3, k, :f], plain["rec"][k, :f], "down", 1e-9, "0 km slot against the ground half, %s" % _what(c, k))
    for slot, z in enumerate(alts):
        _check_rows("slot%d" % slot, c, range(nb), got, got["rec"][slot], refs, lambda r, s=slot: r["records"][s], z)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.STREAMED)
def test_launch_forms_equal_bits(gpu_pkg, monkeypatch, name):
    """The plain solve of a streamed batch is the order-parallel form, which replays the stop tests of the orders it ran ahead
    -- here on series of 17 Fourier orders next to series of 4 in one batch.  One workgroup per bin, the persistent form (on the widened layout where
    the cell's own has none) and one Fourier order per launch return its bits: records of the orders run, order counts, fluxes."""
    c = dc.by_name(name)
    rows = list(range(len(c["bins"])))
    for var in ("SOSGPU_STREAM_SPEC", "SOSGPU_STREAM_PERSIST", "SOSGPU_STREAM_ORDERS_PER_LAUNCH"):
        monkeypatch.delenv(var, raising=False)
    cx = vm._context(gpu_pkg, c, g=dc.G)
    try:
        ref = vm._fetch(cx.solve(vm._upload(cx, c)))
        assert (ref["norders"] >= 4).all() and int(ref["norders"].min()) < int(ref["norders"].max())   # (17 orders down to 4)
        for var, val in (("SOSGPU_STREAM_SPEC", "0"), ("SOSGPU_STREAM_PERSIST", "1"), ("SOSGPU_STREAM_ORDERS_PER_LAUNCH", "1")):
            monkeypatch.setenv(var, val)
            got = vm._fetch(cx.solve(vm._upload(cx, c)))
            monkeypatch.delenv(var)
            print("PARITY forms        %-20s %s=%s: records %s" % (name, var, val, "equal bits" if all(
                np.array_equal(got["rec"][k, :ref["norders"][k]], ref["rec"][k, :ref["norders"][k]]) for k in rows) else "DIFFER"))
            vm._assert_same(got, ref, rows, "%s %s=%s" % (name, var, val))
    finally:
        cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.TWIN_CELLS)
def test_table_twin_vs_oracle(gpu_pkg, oracle, name):
    """The bins dealt alternately to two contexts with different phase functions (g = 0.7 and 0.8) and solved in ONE
    solve_spectrum launch -- the multi-context twin of the cell's kernel -- against the oracle's solves with each g, per half."""
    import torch
    c = dc.by_name(name)
    dc.queue(oracle, c)
    dc.queue(oracle, c, "g2")
    nb = len(c["bins"])
    ra, rb = list(range(nb))[0::2], list(range(nb))[1::2]
    cx, cx2 = vm._context(gpu_pkg, c, g=dc.G), vm._context(gpu_pkg, c, g=0.8)
    try:
        table = gpu_pkg.solver.ContextTable([cx, cx2])
        bins, cob, seg = gpu_pkg.solver.concat_bins([vm._upload(cx, c, ra), vm._upload(cx2, c, rb)])
        out = cx.alloc_outputs(bins["nb"])
        gpu_pkg.solver.solve_spectrum(table, bins, cob, seg, torch.full((nb,), 1.0 / nb, dtype=torch.float64, device=cx.device),
                                      out=out)
        got = vm._fetch(out)
    finally:
        cx.close()
        cx2.close()
    first, second = dc.reference(oracle, c), dc.reference(oracle, c, "g2")
    refs = {k: (first if k in ra else second)[k] for k in range(nb)}
    _check_rows("twin", c, ra + rb, got, got["rec"], refs, lambda r: r["records"], -1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.NAMES)
def test_band_of_deep_and_transparent_bins(gpu_pkg, oracle, name):
    """The seven bins as one band with the weights deep_cells.AIK (solve_band: solve + sosgpu_aggregate): the aggregated record
    against oracle.aggregate of the oracle's own records per half, the fluxes and the band's optical depths
    -log sum aik exp(-tau) at 1e-9 |ref| + 1e-300, everything finite."""
    c = dc.by_name(name)
    dc.queue(oracle, c)
    nb, n = len(c["bins"]), c["n"]
    tau = np.array([b[0][-1] for b in c["bins"]])
    tau_vrai = tau * 1.05                                                          # (three different columns: any depths do)
    tau_out = np.array([b[0][(c["lp"] - 1) // 2] for b in c["bins"]])
    cx = vm._context(gpu_pkg, c, g=dc.G)
    try:
        bins = vm._upload(cx, c)
        bins["scal"] = np.stack([np.zeros(nb), tau, tau_vrai, tau_out], axis=1)
        rec, fin = cx.solve_band(bins, dc.AIK, reduce=False)
        rec = rec.cpu().numpy()[0]
    finally:
        cx.close()
    refs = dc.reference(oracle, c)
    nf = np.array([len(r["records"]) for r in refs], dtype=np.int32)
    recs = np.zeros((nb, c["os_nb"] + 1, 3, 2 * n + 1))
    sb = np.zeros((nb, 7))
    for k, r in enumerate(refs):
        recs[k, :nf[k]] = r["records"]
        sb[k] = [0.0, r["emoins"], r["eplus"], tau[k], tau_vrai[k], tau_out[k], 0.0]
    exp_rec, exp_scal = oracle.aggregate(recs, nf, dc.AIK, sb)
    f = len(exp_rec)
    assert f == nf.max() == int(fin["n_orders"][0]) and int(fin["min_orders"][0]) == nf.min()
    assert np.isfinite(rec).all() and not rec[f:].any()
    got_scal = [fin[key][0] for key in ("emoins", "eplus", "ttot_tronc", "ttot_vrai", "tauout")]
    assert np.isfinite(got_scal).all() and abs(fin["sum_aik"][0] - 1.0) < 1e-15
    e = dc.half_excess(rec[:f], exp_rec)
    dev = [abs(g - r) / abs(r) for g, r in zip(got_scal, exp_scal[1:6])]
    print("PARITY %-12s %-20s down %.3e up %.3e x the bar; emoins %.3e eplus %.3e ttot_tronc %.3e ttot_vrai %.3e tauout %.3e rel" % (
        ("band", name, e["down"], e["up"]) + tuple(dev)))
    dc.compare_halves(rec[:f], exp_rec, 1e-9, "band of %s" % name)
    for key, g, r in zip(("emoins", "eplus", "ttot_tronc", "ttot_vrai", "tauout"), got_scal, exp_scal[1:6]):
        assert abs(g - r) <= 1e-9 * abs(r) + 1e-300, (name, key, g, r)
