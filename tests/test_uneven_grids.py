"""Every layout of the single-context solver against the C oracle on level grids whose layers differ in optical depth by up to
nine decades (uneven_cells.py): levels placed on the no-gas profile with the gas added per bin, a slab of absorber whose edges
straddle the kernels' tile and chunk edges, a user's altitudes with layers of 1e-8 at the top and of 10 - 19 at the ground, the
same from the ground, and a two-layer bin.

Every other synthetic solver test places the levels of a bin by bisection on the bin's own depth, so all its layers have one
dtau and an index slip between the per-layer tables -- the attenuation row att = 1 - exp(-dtau / mu), the entry 1 / dtau, the
level vectors (one level ahead in the streamed kernel), the product of exp(-dtau / mu) carried across a 32-level chunk edge --
gives the same numbers.  Here neighbouring layers differ by factors of up to 240, and the layers of a bin by up to 1.6e9.

CPU: the cells are what they claim; the oracle decides every bin (ier = 0, finite, stop-test tie margin > 1e-7, the bar of
test_oracle); an equal grid of the same total depth, and the two layers at the straddled edge exchanged, each miss the 1e-9 bar
by more than 1000 x on the slab, user and mirrored bins; one ulp on every cosine stays below 1e-2 of the bar.
GPU: the batch of a cell through SosContext.solve per layout; the slab, thin and thick bins through the output-slot path at
altitudes inside and on the upper level of the slab; the streamed batches in every launch form, bit for bit.

No bound here comes from the kernels: the bar is the project's 1e-9 against the oracle (test_variant_matrix
._assert_bin_vs_oracle), the separation and conditioning figures are measured on the oracle alone (profiles/
uneven_grid_parity.txt)."""
import numpy as np
import pytest

import cases
import test_variant_matrix as vm
import uneven_cells as uc

S = cases.S
BAR = 1e-9
SEPARATION = 1e3
MARGIN = 1e-7                                   # the tie margin test_oracle asks of a decided solve


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_cells_reach_their_layouts(pkg, monkeypatch):
    """The routes are the library's: the single-context plan names the layout of every cell (needs the built library)."""
    monkeypatch.delenv("SOSGPU_STREAM_PERSIST", raising=False)                    # (route reads the plan as a solve would)
    for c in uc.CELLS:
        assert vm.route(c["n"], c["lp"]) == c["layout"], (c["name"], vm.route(c["n"], c["lp"]))


def test_cells_are_what_they_claim():
    assert len(uc.CELLS) == 12 and len(set(uc.NAMES)) == 12
    assert {c["layout"] for c in uc.CELLS} == set(vm.LAYOUTS) and len(uc.STREAMED) == 5
    grounds, zouts, ipolar0 = set(), set(), []
    for c in uc.CELLS:
        n, lp, fam = c["n"], c["lp"], c["layout"].split("<")[0]
        if ":" in c["route"]:
            assert (vm._round_up(3 * n, 8) + 15) // 16 == int(c["route"].split(":")[1])
        mu, w, n0 = S.gauss_angles(n - 1, 35.0)
        assert np.array_equal(mu, c["mu"]) and np.array_equal(w, c["w"]) and n0 == c["n0"] and 1 < n0 < n
        assert c["os_nb"] == 16 and np.all(c["iborm"] == 16)
        e = uc.edge(lp)
        assert e == (16 if lp == 32 else 32) and (e < lp - 1)
        slabs = [uc.slab_of(lp)] + [uc.SECOND_SLAB[r] for r in (c["route"],) if r in uc.SECOND_SLAB]
        assert c["kinds"] == [k for kind in uc.KINDS for k in [kind] * (len(slabs) if kind == "slab" else 1)]
        assert [s for s in c["slabs"] if s] == slabs and [uc.slab_edge(s) for s in slabs] == [e, 64][:len(slabs)]
        assert c["nt"].tolist() == [2 if k == "two_layers" else lp - 1 for k in c["kinds"]]
        assert vm._round_up(int(c["nt"].max()) + 1, 16) == lp
        for k, (kind, slab) in enumerate(zip(c["kinds"], c["slabs"])):
            h, x, y, z = c["bins"][k]
            what = (c["name"], kind, slab)
            d = np.diff(h)
            assert np.all(d > 0) and h[0] >= 0 and np.all(np.diff(z) < 0) and z[0] == 120.0 and z[-1] == 0.0, what
            assert np.all((x >= 0) & (y >= 0) & (x + y <= 1)), what
            assert h[-1] / mu[n0 - 1] < 700, what                                 # (beyond it the reference returns NaN)
            ratio = d.max() / d.min()
            if kind == "equal":
                assert ratio < 1.25, (what, ratio)                                # (the truncation rescale alone: 1 - 0.1425 xdel)
            elif kind == "nogas_grid":
                assert 2 < ratio < 10, (what, ratio)
            elif kind == "slab":
                j0, j1 = slab
                assert j0 < uc.slab_edge(slab) < j1 < lp - 1 and uc.slab_edge(slab) % 32 in (0, e), what
                r = d[1:] / d[:-1]                                                # r[i]: layer i + 1 over layer i
                # K_SLAB / 4 = 1 per slab layer over 0.3948 / NT per layer outside (less after the truncation rescale): 2.5 NT
                assert int(np.argmax(r)) + 1 == j0 and 50 < r[j0 - 1] < 500, (what, r[j0 - 1])
                assert int(np.argmin(r)) + 1 == j1 and 50 < 1 / r[j1 - 1] < 500, (what, r[j1 - 1])
                rest = np.delete(r, [j0 - 1, j1 - 1])
                assert np.all((rest > 0.5) & (rest < 2.0)), what
            elif kind == "user_thin":
                assert 1e-9 < d.min() < 1e-7 and 1e6 < ratio < 1e9 and int(np.argmin(d)) == 0, (what, d.min(), ratio)
            elif kind == "user_thick":
                assert 1e8 < ratio < 1e10 and 5 < d[-1] < 20 and int(np.argmin(d)) == 0, (what, ratio, d[-1])
            elif kind == "mirror_thick":
                ref = c["bins"][c["kinds"].index("user_thick")][0]
                assert h[0] == 0.0 and np.array_equal(d, (ref[-1] - ref[::-1])[1:] - (ref[-1] - ref[::-1])[:-1]), what
                assert 5 < d[0] < 20 and int(np.argmax(d)) == 0 and d[-1] < 1e-7, what
            else:
                assert len(h) == 3 and 1e-9 < d[0] < 2e-8 and 8 < d[1] < 12 and ratio > 1e8, (what, d)
        # the boundary conditions
        kw = c["kw"]
        grounds.add((fam, "matrices" if kw.get("imat_surf") else "fresnel" if kw.get("ifresnel") else "lambert"))
        if kw["ipolar"] == 0:
            ipolar0.append(c["name"])
        assert (c["zout"] > 0) == (c["i"] % 2 == 1)
        if c["zout"] > 0:
            zouts.add((fam, "thin" if c["zout"] == uc.ZOUT_THIN else "slab"))
            for k, kind in enumerate(c["kinds"]):
                z, d = c["bins"][k][3], uc.dtau(c, k)
                j = int(np.searchsorted(-z, -c["zout"]))                          # the layer above level j holds zout
                assert 1 <= j <= len(d) and z[j] <= c["zout"] < z[j - 1]
                if c["zout"] == uc.ZOUT_THIN and kind in ("user_thin", "user_thick"):
                    assert d[j - 1] < 1e-4 * d.max(), (c["name"], kind, d[j - 1])
                if c["zout"] != uc.ZOUT_THIN and c["slabs"][k] == uc.slab_of(lp):
                    j0, j1 = c["slabs"][k]                                        # inside the slab: 2 km on the 31-layer grid, the
                    assert j0 < j <= j1, (c["name"], j, j0, j1)                   # middle of slab layer j0 on the finer ones
                    assert (c["zout"] == uc.ZOUT_SLAB) == (lp == 32) and (lp == 32 or (j == j0 + 1 and d[j0] > 50 * d[j0 - 1]))
    assert grounds == {(f, g) for f in ("os", "stream") for g in ("lambert", "fresnel", "matrices")}
    assert zouts == {(f, z) for f in ("os", "stream") for z in ("slab", "thin")}
    assert ipolar0 == [c["name"] for c in uc.CELLS if c["layout"] == uc.IPOLAR0] and len(ipolar0) == 1
    assert [uc.by_name(n)["layout"].split("<")[0] for n in uc.SEPARATION_CELLS] == ["os", "stream"]
    assert [uc.by_name(n)["layout"].split("<")[0] for n in uc.CAPTURE_CELLS] == ["os", "stream"]


def test_oracle_is_decided_on_every_cell(oracle):
    for c in uc.CELLS:
        uc.queue(oracle, c)
    for c in uc.CELLS:
        margins = []
        for k, r in enumerate(uc.reference(oracle, c)):
            what = (c["name"], c["kinds"][k], c["slabs"][k])
            assert r["ier"] == 0 and np.all(np.isfinite(r["records"])), what
            assert np.isfinite(r["emoins"]) and np.isfinite(r["eplus"]), what
            assert len(r["records"]) >= 4 and len(r["ig_counts"]) == len(r["records"]), (what, len(r["records"]))
            assert r["margin"] > MARGIN, (what, r["margin"])
            margins.append(r["margin"])
        print("%-20s orders %s  tie margin min %.2e" % (c["name"], [len(r["records"]) for r in uc.reference(oracle, c)], min(margins)))


def test_bar_separates_right_from_wrong(oracle):
    """What a kernel that read an equal grid would compute, and what one that took the 1 / dtau (or the attenuation) of the
    neighbouring layer at the straddled edge would compute, both as the oracle's own solves of the changed bin: each misses
    compare_records at 1e-9 by more than 1000 x on the slab, user and mirrored bins.  The edge is the one the bin's own slab
    straddles (16, 32, or 64 for the slab (62, 66)) in a slab bin, the layout's in the others."""
    seen = 0
    for name in uc.SEPARATION_CELLS:
        c = uc.by_name(name)
        for k, how, factor in uc.separation(oracle, c):
            print("%-14s %-13s %-8s %-13s misses the bar %.3e x" % (name, c["kinds"][k], c["slabs"][k] or "", how, factor))
            assert factor >= SEPARATION, (name, c["kinds"][k], how, factor)
            seen += 1
    assert seen == 2 * (4 + 5)


def test_one_ulp_on_the_cosines_stays_inside_the_bar(oracle):
    """The conditioning the 1e-9 bar rests on: every cosine moved up by one ulp moves no record of any bin by more than 1e-2 of
    compare_records' tolerance (measured: see profiles/uneven_grid_parity.txt) -- on the equal grid as on the uneven ones."""
    moved = {}
    for c in uc.CELLS:
        uc.queue(oracle, c)
        mu = np.nextafter(c["mu"], 2.0)
        assert np.all(mu > c["mu"]) and np.all(mu <= 1.0)
        moved[c["name"]] = [vm._POOL.submit(uc.solve, oracle, c, k, mu=mu) for k in range(len(c["bins"]))]
    worst = {}
    for c in uc.CELLS:
        for k, (ref, fut) in enumerate(zip(uc.reference(oracle, c), moved[c["name"]])):
            got = fut.result()
            assert got["ier"] == 0 and np.array_equal(got["ig_counts"], ref["ig_counts"]), (c["name"], c["kinds"][k])
            e = uc.excess(got["records"], ref["records"], BAR)
            cases.compare_records(got["records"], ref["records"], 1e-2 * BAR, "%s %s: %.3e of the tolerance" % (c["name"], c["kinds"][k], e))
            assert e < 1e-2, (c["name"], c["kinds"][k], e)       # (excess is compare_records' own ratio: the two agree)
            worst[c["kinds"][k]] = max(worst.get(c["kinds"][k], 0.0), e)
    print("one ulp on every mu, worst |d record| / tolerance per kind: " + "  ".join("%s %.2e" % kv for kv in worst.items()))


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _what(c, k):
    return "%s (%s) bin %d %s %s NT=%d zout=%g" % (c["name"], c["route"], k, c["kinds"][k], c["slabs"][k] or "", c["nt"][k], c["zout"])


def _flux_dev(got, k, ref):
    return max(abs(got["flux"][k, 0] - ref["emoins"]) / abs(ref["emoins"]), abs(got["flux"][k, 1] - ref["eplus"]) / abs(ref["eplus"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", uc.NAMES)
def test_layout_vs_oracle(gpu_pkg, oracle, name):
    c = uc.by_name(name)
    uc.queue(oracle, c)
    cx = vm._context(gpu_pkg, c, g=uc.G)
    try:
        got = vm._fetch(cx.solve(vm._upload(cx, c)))
    finally:
        cx.close()
    failures = []
    for k, ref in enumerate(uc.reference(oracle, c)):
        f = len(ref["records"])
        if int(got["norders"][k]) == f and np.isfinite(got["rec"][k, :f]).all():  # the figure first, then the assertion
            print("%s: records %.3e  fluxes %.3e  (x the bar: %.3e)" % (
                _what(c, k), float((np.abs(got["rec"][k, :f] - ref["records"]) / np.maximum(np.abs(ref["records"]),
                                    1e-3 * np.abs(ref["records"][:, 0]).max())).max()), _flux_dev(got, k, ref),
                uc.excess(got["rec"][k, :f], ref["records"], BAR)))
        else:
            print("%s: norders %d against %d" % (_what(c, k), int(got["norders"][k]), f))
        try:
            vm._assert_bin_vs_oracle(got, k, got["rec"][k], ref, ref["records"], _what(c, k))
        except AssertionError as err:
            failures.append(str(err)[:400])
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("name", uc.CAPTURE_CELLS)
def test_capture_on_uneven_levels(gpu_pkg, oracle, name):
    """The slab, thin and thick bins through the output slots: the standard output, an altitude inside the slab's first layer,
    the slab's upper level itself (weight exactly 0 or 1 in the slab bin) and 70 km, four slots of one solve."""
    c = uc.by_name(name)
    rows = [c["kinds"].index(k) for k in ("slab", "user_thin", "user_thick")]
    zs = c["bins"][rows[0]][3]
    j0, j1 = c["slabs"][rows[0]]
    alts = [-1.0, 0.5 * float(zs[j0] + zs[j0 + 1]), float(zs[j0]), uc.ZOUT_THIN]
    futs = [vm._POOL.submit(uc.solve, oracle, c, k, zouts=alts) for k in rows]
    cx = vm._context(gpu_pkg, c, g=uc.G)
    try:
        bins = vm._upload(cx, c, rows)
        lv = cx.output_levels(bins, alts)
        jout, zz = lv["jout"].cpu().numpy(), lv["zz"].cpu().numpy()
        got = vm._fetch(cx.solve_levels(bins, lv))
    finally:
        cx.close()
    assert jout[1, 0] == j0 + 1 and 0 < zz[1, 0] < 1                               # inside the slab's first layer
    assert jout[2, 0] in (j0, j0 + 1) and zz[2, 0] in (0.0, 1.0)                   # on its upper level
    assert (jout[1:] > 0).all() and (jout[0] == 0).all()
    for r, (k, fut) in enumerate(zip(rows, futs)):
        ref = fut.result()
        assert ref["margin"] > MARGIN, (_what(c, k), ref["margin"])
        for slot in range(len(alts)):
            what = "%s slot %d (%g km, jout %d zz %g)" % (_what(c, k), slot, alts[slot], jout[slot, r], zz[slot, r])
            f = len(ref["records"][slot])
            if int(got["norders"][r]) == f:
                print("%s: %.3e x the bar" % (what, uc.excess(got["rec"][slot, r, :f], ref["records"][slot], BAR)))
            vm._assert_bin_vs_oracle(got, r, got["rec"][slot, r], ref, ref["records"][slot], what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", uc.STREAMED)
def test_launch_forms_equal_bits(gpu_pkg, monkeypatch, name):
    """The plain solve of a streamed batch is the order-parallel form, which replays the stop tests of the orders it ran ahead.
    One workgroup per bin, one Fourier order per launch, the persistent form where the layout has it, and a one-entry context
    table through solve_spectrum return its bits."""
    import torch
    c = uc.by_name(name)
    nb = len(c["bins"])
    rows = list(range(nb))
    for var in ("SOSGPU_STREAM_SPEC", "SOSGPU_STREAM_PERSIST", "SOSGPU_STREAM_ORDERS_PER_LAUNCH"):
        monkeypatch.delenv(var, raising=False)
    cx = vm._context(gpu_pkg, c, g=uc.G)
    try:
        ref = vm._fetch(cx.solve(vm._upload(cx, c)))
        assert (ref["norders"] >= 4).all()
        forms = [("SOSGPU_STREAM_SPEC", "0"), ("SOSGPU_STREAM_ORDERS_PER_LAUNCH", "1")]
        if c["layout"] in vm.FULL_WIDTH:
            forms.append(("SOSGPU_STREAM_PERSIST", "1"))
        for var, val in forms:
            monkeypatch.setenv(var, val)
            vm._assert_same(vm._fetch(cx.solve(vm._upload(cx, c))), ref, rows, "%s %s=%s" % (name, var, val))
            monkeypatch.delenv(var)
        table = gpu_pkg.solver.ContextTable([cx])
        bins, cob, seg = gpu_pkg.solver.concat_bins([vm._upload(cx, c)])
        out = cx.alloc_outputs(nb)
        gpu_pkg.solver.solve_spectrum(table, bins, cob, seg, torch.full((nb,), 1.0 / nb, dtype=torch.float64, device=cx.device),
                                      out=out)
        vm._assert_same(vm._fetch(out), ref, rows, "%s one-entry context table" % name)
    finally:
        cx.close()
