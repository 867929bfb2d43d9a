"""The order-0 incidence solves of sosgpu_trans_spectrum / sosgpu_albedo_spectrum against the C oracle, in every layout of the
multi-context solver and with the incidence at every position of the direction set.

Both entry points turn every (bin, direction J) pair into an item of one table launch with n0 = J, Fourier order 0 and a black
ground.  The per-direction loop they are held to elsewhere (SosContext.diffuse_transmissions) runs the same solver kernels with
tables from the same noyaux_dev.h, so an error the two share -- a source vector formed with a neighbour's cosine, a row tile of
the second half read with the wrong n0 row, the flux normalised with the parent's sun, a parent's ro / f11sun / matrices
surviving into a child -- passes every bit-for-bit test.  test_variant_matrix holds all layouts to the oracle, but its
incidence is a weight-0 direction at the first or last position; here the incidence is every direction, most of them weighted
Gauss nodes in the interior, down to the smallest node.

Cells (incidence_cells.py).  One per route of the table launch, at an end of the route's range of N and of padded level
counts lp (N = 21 for the one-tile layouts, the smallest N of every other), two bins (NT = 1 and NT = lp - 1) in one call, the parent's sun alternately first and last, the parent's ground
alternately Lambert, Fresnel and surface matrices.  The form has ELEVEN kernel instantiations (test_variant_matrix.LAYOUTS,
without output slots and surface matrices here): os<4,2,2,SPLIT> is one kernel whose shared-tile loop runs over the context's
five (N 22-26) or six (N 27-32) row tiles, and is counted as two routes, so the table has twelve rows.  No cell had to be
moved: the table launch routes every (N, lp) as the single-context solve does.  Six further cells: the N = 27 set with two
user directions at NT = 20 and at NT = 70 (two calls, so that both the LDS-resident and the streamed kernel see user
directions), the sun on a Gauss node (every direction weighted), a table of three parents with interleaved, unsorted
ctx_of_bin and level grids of two lengths, and two opaque bins (total depth ~30 and ~200) at NT = 20 and again at NT = 70,
because the two kernels each have a copy of the scattering-order loop.

CPU: the routes are the library's (the plan of the launch the entry points make) and cover every route the form has over
N = 3 ... 85 and lp = 16 ... 1024; every oracle solve has ier = 0 and finite fluxes on the profile and on its mirror; and each
error named above, applied to the oracle's own numbers, moves a value of every bin by more than 1000 x the GPU bar.
GPU: tdifmug against EMOINS for every direction, plane against EPLUS on the profile (from_below=False) and on the host mirror
(from_below=True) for every weighted direction, at the project's bar for these quantities, |got - ref| <= 1e-9 |ref| + 1e-300
(test_trans_many.test_against_the_oracle, test_gpu_parity.test_diffuse_transmissions_vs_oracle); NaN is a mismatch.

Finding.  The deeper opaque bin missed the bar in both kernels: tdifmug -6.3e-83 where the oracle has 9.6e-80 (all 41
directions, LDS-resident kernel), 3.3e-6 relative in the streamed one, and the plane albedos seen from above -- ordinary
numbers, 0.48 -- 2.9e-6 and 6.7e-7 off.  Cause: SOS_PARAM_CONV in product form (sos_dev.h conv_exceeds) multiplies four field
values; the down-going rows at the ground are 1e-80 there, their products underflow, and the rows that still prolong the
reference's series were ignored, so the series ended early and the geometric tail was added while g > d.  conv_exceeds now
repeats the test on operands scaled by one power of two when its denominator is below 1e-200; every other decision keeps its
bits.  No bar was widened for `opaque`.

Measured on one MI355X, 2026-10-20, worst relative deviation from the oracle (tdifmug / plane above / plane below; bar 1e-9;
3 565 values compared, none excused):
    os<4,1,2>           7.1e-16 / 5.7e-16 / 4.6e-16      stream<4,1,4>     2.3e-15 / 1.0e-15 / 4.8e-16
    os<4,2,2,SPLIT>:5   6.3e-16 / 7.8e-16 / 4.6e-16      stream<4,2,5>     7.9e-15 / 5.5e-15 / 4.7e-16
    os<4,2,2,SPLIT>:6   7.1e-16 / 6.3e-16 / 4.5e-16      stream<4,2,6>     3.1e-15 / 1.8e-15 / 4.5e-16
    os<4,2,2>           1.4e-15 / 6.9e-16 / 7.6e-16      stream<4,2,8>     2.3e-15 / 6.7e-16 / 5.6e-16
    os<8,2,2>           6.3e-16 / 6.1e-16 / 4.5e-16      stream<8,2,16>    1.8e-15 / 1.2e-15 / 1.8e-15
    os<4,1,4>           2.8e-15 / 9.2e-16 / 6.3e-16      os<8,1,4>         6.8e-15 / 2.2e-15 / 4.4e-16
    user_angles_nt20    7.1e-16 / 4.4e-16 / 1.0e-15      user_angles_nt70  8.8e-16 / 4.3e-16 / 8.2e-16
    sun_on_node         9.9e-16 / 3.9e-16 / 1.2e-15      table             2.2e-15 / 8.0e-16 / 6.8e-16
    opaque              6.1e-13 / 4.4e-16 / 3.9e-16      opaque_streamed   4.5e-15 / 5.5e-16 / 3.4e-16"""
import numpy as np
import pytest

import incidence_cells as ic
import test_albedo_many as A
import test_trans_many as T
import test_variant_matrix as vm

BAR = 1e-9
FLOOR = 1e-300
SEPARATION = 1000                               # an error must move a value by more than SEPARATION x the bar
CELLS, NAMES = ic.CELLS, ic.NAMES
FURTHER_ROUTES = {"user_angles_nt20": "os<4,2,2,SPLIT>:6", "user_angles_nt70": "stream<4,2,6>", "sun_on_node": "os<4,2,2,SPLIT>:5",
                  "table": "stream<4,2,6>", "opaque": "os<4,2,2>", "opaque_streamed": "stream<4,2,8>"}
GUARD_CELLS = ("user_angles_nt20", "table")     # one LDS-resident, one streamed; each has a middle bin


def _bar(ref):
    return BAR * np.abs(ref) + FLOOR


def _moved(wrong, ref):
    """Whether `wrong` lies further than SEPARATION x the bar from `ref`, element by element."""
    return np.abs(np.asarray(wrong) - ref) > SEPARATION * _bar(ref)


def _weighted(cell, b):
    return cell["ctxs"][cell["bins"][b]["c"]]["w"] != 0.0


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_cells_are_what_they_claim(pkg, oracle, monkeypatch):
    monkeypatch.delenv("SOSGPU_STREAM_PERSIST", raising=False)                    # (the plan is read as a solve would)
    for c in CELLS:
        ic.queue(oracle, c)
    assert len(set(NAMES)) == len(CELLS) == 18 and len(ic.LAYOUT_CELLS) == 12
    # the routes: what the form has, and that the twelve cells reach each of them
    has = {ic.route_multi(pkg, n, lp, 2 * n) for n in range(3, 86) for lp in range(16, 1025, 16)}
    assert len(has) == 12 and {r.split(":")[0] for r in has} == set(vm.LAYOUTS)
    routes = [ic.route_multi(pkg, c["n"], c["lp"], len(c["bins"]) * c["n"]) for c in ic.LAYOUT_CELLS]
    assert routes == [c["route"] for c in ic.LAYOUT_CELLS] == [r for r, _, _ in ic.LAYOUT_TABLE]
    assert len(set(routes)) == 12 and set(routes) == has
    for c in ic.LAYOUT_CELLS:                                                     # an end of the route's N range and of its lp range
        assert any(ic.route_multi(pkg, c["n"] + d, c["lp"], 2) != c["route"] for d in (-1, 1)), c["name"]
        assert any(ic.route_multi(pkg, c["n"], c["lp"] + d, 2) != c["route"] for d in (-16, 16)), c["name"]
    assert {c["name"]: ic.route_multi(pkg, c["n"], c["lp"], len(c["bins"]) * c["n"]) for c in CELLS if c["route"] is None} \
        == FURTHER_ROUTES
    # the inputs
    suns, grounds = set(), set()
    for c in CELLS:
        nts = [b["nt"] for b in c["bins"]]
        assert vm._round_up(max(nts) + 1, 16) == c["lp"], c["name"]
        assert len(c["ctxs"]) == len(set(c["ctx_of_group"])) and np.array_equal(c["cob"], [b["c"] for b in c["bins"]])
        for cx in c["ctxs"]:
            assert len(cx["mu"]) == len(cx["w"]) == c["n"] and np.all(np.diff(cx["mu"]) < 0) and 0 < cx["mu"][-1] and cx["mu"][0] <= 1
            assert cx["ground"]["ro"] != 0.0                                      # a parent's albedo can show in a child
        for b in c["bins"]:
            assert len(b["h"]) == b["nt"] + 1 and np.all(np.diff(b["h"]) > 0)
    for i, c in enumerate(ic.LAYOUT_CELLS):
        cx = c["ctxs"][0]
        assert [b["nt"] for b in c["bins"]] == [1, c["lp"] - 1]
        assert cx["os_nb"] == 16 and cx["g"] == 0.7 and cx["ipolar"] == 1
        # one weight-0 direction, the parent's sun, at the first or the last position: every other incidence of the cell is a
        # weighted Gauss node -- the first or the last one (whichever the sun is not), and N - 2 interior ones
        assert np.flatnonzero(cx["w"] == 0.0).tolist() == [cx["n0"] - 1] and cx["n0"] == (c["n"] if i % 2 else 1)
        suns.add((c["route"].split("<")[0], c["sun"]))
        grounds.add("matrices" if cx["ground"].get("matrices") else "fresnel" if cx["ground"].get("ifresnel") else "lambert")
    assert suns == {("os", "first"), ("os", "last"), ("stream", "first"), ("stream", "last")}
    assert grounds == {"lambert", "fresnel", "matrices"}
    for name in ("user_angles_nt20", "user_angles_nt70"):
        c = ic.by_name(name)
        cx = c["ctxs"][0]
        zero = np.flatnonzero(cx["w"] == 0.0).tolist()
        assert c["n"] == 27 and len(zero) == 3 and cx["n0"] - 1 in zero and 0 < min(zero) and max(zero) < 26   # all interior
        assert {b["nt"] for b in c["bins"]} == {int(name[-2:])} and len(c["bins"]) == 3
    c = ic.by_name("sun_on_node")
    cx = c["ctxs"][0]
    assert c["n"] == 24 and np.all(cx["w"] != 0.0) and 1 < cx["n0"] < 24
    c = ic.by_name("table")
    assert [(cx["os_nb"], cx["ipolar"]) for cx in c["ctxs"]] == [(16, 1), (48, 1), (24, 0)]
    assert len({cx["g"] for cx in c["ctxs"]}) == 3 and len({cx["n0"] for cx in c["ctxs"]}) == 3
    assert all(c["n"] == 27 and int(np.sum(cx["w"] == 0.0)) == 3 and 1 < cx["n0"] < 27 for cx in c["ctxs"])
    assert c["ctxs"][0]["ground"] == dict(ro=0.1, ifresnel=1, ind_surf=1.34) and c["ctxs"][1]["ground"].get("matrices")
    assert c["cob"].tolist() == [2, 0, 1, 1, 0, 2, 1]                             # interleaved, unsorted
    assert {(b["c"], b["nt"]) for b in c["bins"]} == {(k, nt) for k in range(3) for nt in (20, 70)}
    for name, nt in (("opaque", 20), ("opaque_streamed", 70)):
        c = ic.by_name(name)
        assert c["n"] == 41 and [b["nt"] for b in c["bins"]] == [nt, nt] and c["ctxs"][0]["g"] == 0.6
        assert 25 < c["bins"][0]["h"][-1] < 35 and 150 < c["bins"][1]["h"][-1] < 210
        assert c["bins"][1]["h"][-1] / c["ctxs"][0]["mu"][-1] > 5e3               # the direct beam underflows in the column
        # EMOINS of the deeper bin lies below 1e-77, where a product of four field values underflows (sos_dev.h conv_exceeds)
        assert 0 < ic.reference(oracle, c)["em"][1].max() < 1e-77
    # the oracle's side: a condition on the inputs
    total = 0
    for c in CELLS:
        r = ic.reference(oracle, c)
        total += r["ier"].size
        assert not r["ier"].any(), (c["name"], np.argwhere(r["ier"] != 0)[:4])
        for k in ("em", "ep", "em_below", "ep_below"):
            assert r[k].shape == (len(c["bins"]), c["n"]) and np.all(np.isfinite(r[k])), (c["name"], k)
    print("oracle solves: %d" % total)


def _probe_directions(cell, b):
    """The first and the middle weighted direction (1-based) of bin b's context."""
    w = _weighted(cell, b)
    first = int(np.flatnonzero(w)[0]) + 1
    mid = int(np.flatnonzero(w & (np.arange(cell["n"]) >= cell["n"] // 2))[0]) + 1
    return first, mid


def test_bar_separates_right_from_wrong(oracle):
    """Each error, applied to the oracle's own numbers, moves at least one value of every bin, in each output it can reach, by
    more than 1000 x the bar.  Outputs: tdifmug (EMOINS, every direction), plane above and below (EPLUS, weighted directions).
    One exception is stated, not excused: under 30 and 200 optical depths (`opaque`) a Lambert ground does not show in the
    light leaving the lit side, so there the parent's ro is caught by tdifmug alone."""
    for c in CELLS:
        ic.queue(oracle, c)
    extra = {}
    for c in CELLS:
        for b in range(len(c["bins"])):
            cx = c["ctxs"][c["bins"][b]["c"]]
            for j in _probe_directions(c, b):
                for m in (False, True):
                    extra[(c["name"], b, j, m, "ro")] = vm._POOL.submit(ic.solve, oracle, c, b, j, m, ro=cx["ground"]["ro"])
                    if c["name"] == "table":
                        extra[(c["name"], b, j, m, "ipolar")] = vm._POOL.submit(ic.solve, oracle, c, b, j, m, ipolar=1 - cx["ipolar"])
    for c in CELLS:
        r = ic.reference(oracle, c)
        for b in range(len(c["bins"])):
            what = "%s bin %d" % (c["name"], b)
            cx = c["ctxs"][c["bins"][b]["c"]]
            w = _weighted(c, b)
            em, ep, epb = r["em"][b], r["ep"][b], r["ep_below"][b]
            # column J replaced by column J - 1 / J + 1
            for v, cols in ((em, np.ones_like(w)), (ep, w), (epb, w)):
                assert np.any(_moved(v[:-1], v[1:])[cols[1:]]) and np.any(_moved(v[1:], v[:-1])[cols[:-1]]), what
            # EMOINS and EPLUS exchanged
            assert np.any(_moved(ep, em)) and np.any(_moved(em, ep)[w]) and np.any(_moved(r["em_below"][b], epb)[w]), what
            # from_below on the profile as it stands
            assert np.any(_moved(ep, epb)[w]) and np.any(_moved(epb, ep)[w]), what
            # the parent's sun in the normalisation: - em 2 / tab with tab = -mu_sun in place of -mu_J
            scale = cx["mu"] / cx["mu"][cx["n0"] - 1]
            assert np.any(_moved(em * scale, em)) and np.any(_moved(ep * scale, ep)[w]) and np.any(_moved(epb * scale, epb)[w]), what
            # the parent's ro in place of 0, and in `table` the ipolar of another context
            for kind in ("ro", "ipolar") if c["name"] == "table" else ("ro",):
                hit = dict(em=False, ep=False, epb=False)
                for j in _probe_directions(c, b):
                    above, below = (extra[(c["name"], b, j, m, kind)].result() for m in (False, True))
                    assert above["ier"] == 0 and below["ier"] == 0
                    hit["em"] |= bool(_moved(above["emoins"], em[j - 1]))
                    hit["ep"] |= bool(_moved(above["eplus"], ep[j - 1]))
                    hit["epb"] |= bool(_moved(below["eplus"], epb[j - 1]))
                if c["name"].startswith("opaque") and kind == "ro":
                    assert hit == dict(em=True, ep=False, epb=False), (what, hit)
                else:
                    assert all(hit.values()), (what, kind, hit)


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _contexts(pkg, cell):
    out = []
    for cx in cell["ctxs"]:
        kw = dict(cx["ground"])
        if kw.pop("matrices", False):
            rng = np.random.default_rng(7)
            kw.update(imat_surf=1, rsurf=(0.02 * rng.random((cx["os_nb"] + 1, 9, cell["n"], cell["n"]))).astype(np.float32))
        out.append(pkg.SosContext(cx["mu"], cx["w"], cx["n0"], *cx["phase"], iborm_max=cx["os_nb"], ipolar=cx["ipolar"], **kw))
    return out


def _bins(pkg, ctxs, cell, dead=None):
    """The cell's groups uploaded and joined (solver.concat_profiles); bin `dead` gets nt = 0.  Returns (bins, ctx_of_bin as a
    host array, or None with one context)."""
    each, k = [], 0
    for g in cell["groups"]:
        nt = g["nt"].copy()
        for r in range(len(nt)):
            if k == dead:
                nt[r] = 0
            k += 1
        each.append(ctxs[g["c"]].upload_bins(*g["prof"], nt=nt))
    bins, grp = pkg.solver.concat_profiles(each)
    assert bins["lp"] == cell["lp"] and bins["nb"] == len(cell["bins"])
    if len(ctxs) == 1:
        return bins, None
    cob = np.asarray(cell["ctx_of_group"], dtype=np.int32)[grp.cpu().numpy()]
    assert np.array_equal(cob, cell["cob"])
    return bins, cob


_GOT = {}


def _run(pkg, cell):
    """One call per entry point (and illumination), once per session: host arrays tdifmus, tdifmug, and (salb, plane) above and
    below."""
    import torch
    if cell["name"] not in _GOT:
        ctxs = _contexts(pkg, cell)
        try:
            bins, cob = _bins(pkg, ctxs, cell)
            tdifmus, tdifmug = pkg.solver.diffuse_transmissions_many(ctxs, bins, cob)
            above = pkg.solver.spherical_albedo_many(ctxs, bins, cob, from_below=False)
            below = pkg.solver.spherical_albedo_many(ctxs, bins, cob, from_below=True)
            torch.cuda.synchronize()
            host = lambda t: t.cpu().numpy()
            _GOT[cell["name"]] = dict(tdifmus=host(tdifmus), tdifmug=host(tdifmug), above=tuple(host(t) for t in above),
                                      below=tuple(host(t) for t in below))
        finally:
            for cx in ctxs:
                cx.close()
    return _GOT[cell["name"]]


def _compare(got, ref, cols, what):
    """got, ref [nb][N] in the columns `cols` [nb][N] at the bar; prints and returns the worst relative deviation."""
    ok = np.abs(got - ref) <= _bar(ref)                                           # (NaN on either side compares False)
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(cols, np.abs(got - ref) / np.abs(ref), 0.0)
    worst = float(np.max(dev))
    print("%s: worst relative deviation %.3e over %d values" % (what, worst, int(np.sum(cols))))
    bad = np.argwhere(cols & ~ok)
    assert not len(bad), (what, "%d of %d miss the bar" % (len(bad), int(np.sum(cols))),
                          [(int(b), int(j) + 1, float(got[b, j]), float(ref[b, j])) for b, j in bad[:6]])
    return worst


def _label(cell):
    return "%s (%s)" % (cell["name"], cell["route"] or FURTHER_ROUTES[cell["name"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_transmissions_against_the_oracle(gpu_pkg, oracle, name):
    cell = ic.by_name(name)
    ic.queue(oracle, cell)
    got = _run(gpu_pkg, cell)
    ref = ic.reference(oracle, cell)
    assert got["tdifmug"].shape == ref["em"].shape
    _compare(got["tdifmug"], ref["em"], np.ones(ref["em"].shape, dtype=bool), "tdifmug %s" % _label(cell))
    for b, bn in enumerate(cell["bins"]):
        assert got["tdifmus"][b] == got["tdifmug"][b, cell["ctxs"][bn["c"]]["n0"] - 1], (name, b)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ("above", "below"))
@pytest.mark.parametrize("name", NAMES)
def test_plane_albedos_against_the_oracle(gpu_pkg, oracle, name, side):
    cell = ic.by_name(name)
    ic.queue(oracle, cell)
    salb, plane = _run(gpu_pkg, cell)[side]
    ref = ic.reference(oracle, cell)["ep" if side == "above" else "ep_below"]
    cols = np.array([_weighted(cell, b) for b in range(len(cell["bins"]))])
    assert plane.shape == ref.shape
    _compare(plane, ref, cols, "plane %s %s" % (side, _label(cell)))
    assert np.all(plane[~cols] == 0.0) and not np.any(np.signbit(plane[~cols]))
    for b, bn in enumerate(cell["bins"]):
        cx = cell["ctxs"][bn["c"]]
        assert salb[b] == A.gauss_sum(cx["mu"], cx["w"], plane[b:b + 1])[0], (name, side, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GUARD_CELLS)
def test_guard_and_neighbours(gpu_pkg, name):
    """The middle bin with nt = 0, through the raw C calls on buffers of their own: its rows are zeros, every other bin keeps
    the bits of the plain call, and the eight doubles behind tdifmug, plane and salb stay as they were."""
    import torch
    cell = ic.by_name(name)
    ref = _run(gpu_pkg, cell)
    nb, n = len(cell["bins"]), cell["n"]
    dead = nb // 2
    keep = [b for b in range(nb) if b != dead]
    assert ic.route_multi(gpu_pkg, n, cell["lp"], nb * n).startswith("os" if name == GUARD_CELLS[0] else "stream")
    ctxs = _contexts(gpu_pkg, cell)
    try:
        bins, cob = _bins(gpu_pkg, ctxs, cell, dead=dead)
        cob = None if cob is None else gpu_pkg.solver._dev_i32(cob, ctxs[0].device)
        code, out, _, _ = T._raw_call(gpu_pkg, ctxs, bins, cob)
        assert code == 0
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        tdifmug = out[:nb * n].reshape(nb, n)
        assert np.all(out[nb * n:] == -7.0) and len(out) == nb * n + 8
        assert not np.any(tdifmug[dead]) and np.array_equal(tdifmug[keep], ref["tdifmug"][keep])
        for side, below in (("above", 0), ("below", 1)):
            code, salb, plane, _, _ = A._raw_call(gpu_pkg, ctxs, bins, cob, from_below=below)
            assert code == 0
            torch.cuda.synchronize()
            salb, plane = salb.cpu().numpy(), plane.cpu().numpy()
            assert np.all(salb[nb:] == -7.0) and len(salb) == nb + 8
            assert np.all(plane[nb * n:] == -7.0) and len(plane) == nb * n + 8
            plane = plane[:nb * n].reshape(nb, n)
            assert salb[dead] == 0.0 and not np.any(plane[dead]), (name, side)
            assert np.array_equal(salb[:nb][keep], ref[side][0][keep]) and np.array_equal(plane[keep], ref[side][1][keep]), (name, side)
    finally:
        for cx in ctxs:
            cx.close()
