"""Every single-context instantiation of the fused solver (44 = 11 layouts x ZO x SURF) and its multi-context twin, at the
first and last direction count its layout accepts, against the C oracle; the launch forms bit for bit against each other;
and the records independent of memory a kernel must not read (levels past a bin's NT, stale scratch).

The routing from (N, padded level count lp) to a layout is the library's: `route` below reads it from the plan a solve follows
(sosgpu_debug_solve_plan; the rule is solve_variant, csrc/solve_variant.h, and the launchers take the plan's variant).  The
literal tables LAYOUTS / N_RANGE / FULL_WIDTH are the independent statement; `test_table_covers_every_instantiation` (CPU)
checks them against the library for every N = 3 ... 85 at every padded level count of NTS."""
import ctypes as C
import importlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cases

S = cases.S


def _round_up(x, m):
    return (x + m - 1) // m * m


def route(n, lp):
    """Layout that sosgpu_os_solve launches for N directions and the padded level count lp (nt_max = lp - 1), as the library's
    plan names it -- under the switches of the environment: SOSGPU_STREAM_PERSIST widens <4,2,5> / <4,2,6> to <4,2,8>."""
    capi = importlib.import_module("radiativetransfer-sos_amd.capi")
    p = capi.SolvePlan()
    capi.check(capi.lib().sosgpu_debug_solve_plan(n, 0, 1, lp, 0, 0, lp - 1, C.byref(p)), "sosgpu_debug_solve_plan")
    if p.big:
        return "stream<%d,%d,%d>" % (p.nw, p.rtw, p.kht)
    return "os<%d,%d,%d%s>" % (p.nw, p.rtw, p.ct, ",SPLIT" if p.split else "")


# layout -> [(N, padded level counts of its batches)]: the first and last N of the layout (3 = the smallest N of
# synth.gauss_angles), both rtph values of SPLIT (N 22-26: 5, 27-32: 6).  A streamed N gets a batch at the smallest lp of
# the layout and one at the reference's NT = 600 (lp 608); <4,1,4> and <8,1,4> take lp 48 at one corner and 64 at the other.
LAYOUTS = {
    "os<4,1,2>": [(3, (32,)), (21, (32,))],
    "os<4,2,2,SPLIT>": [(22, (32,)), (26, (32,)), (27, (32,)), (32, (32,))],
    "os<4,2,2>": [(33, (32,)), (42, (32,))],
    "os<8,2,2>": [(43, (32,)), (85, (32,))],
    "os<4,1,4>": [(3, (48,)), (21, (64,))],
    "os<8,1,4>": [(22, (64,)), (42, (48,))],
    "stream<4,1,4>": [(3, (80, 608)), (21, (80, 608))],
    "stream<4,2,5>": [(22, (80, 608)), (26, (80, 608))],
    "stream<4,2,6>": [(27, (80, 608)), (32, (80, 608))],
    "stream<4,2,8>": [(33, (80, 608)), (42, (80, 608))],
    "stream<8,2,16>": [(43, (48, 608)), (85, (48, 608))],
}
N_RANGE = {"os<4,1,2>": (3, 21), "os<4,2,2,SPLIT>": (22, 32), "os<4,2,2>": (33, 42), "os<8,2,2>": (43, 85),
           "os<4,1,4>": (3, 21), "os<8,1,4>": (22, 42), "stream<4,1,4>": (3, 21), "stream<4,2,5>": (22, 26),
           "stream<4,2,6>": (27, 32), "stream<4,2,8>": (33, 42), "stream<8,2,16>": (43, 85)}
FULL_WIDTH = ("stream<4,1,4>", "stream<4,2,8>", "stream<8,2,16>")      # the layouts with a persistent form

# one batch = (layout, ZO, SURF, N, lp)
BATCHES = [(lay, zo, surf, n, lp) for lay, corners in LAYOUTS.items() for zo in (False, True) for surf in (False, True)
           for n, lps in corners for lp in lps]

# level counts of a batch: NT = 1 and NT = lp - 1 always; 64 / 32 are the first NT that leave the LDS-resident layouts, 95 / 96
# sit on either side of a 32-level chunk edge, 600 is the reference's CTE_OS_NT
NTS = {32: (1, 16, 31), 48: (1, 32, 47), 64: (1, 40, 63), 80: (1, 64, 79), 608: (1, 95, 96, 600, 607)}

# the (layout, ZO, SURF) cells that no oracle or golden comparison reached before this module
PREVIOUSLY_UNCHECKED = [("os<4,1,2>", True, False), ("os<4,2,2,SPLIT>", False, True), ("os<4,2,2,SPLIT>", True, True),
                        ("os<4,2,2>", True, False), ("os<4,2,2>", True, True), ("os<8,2,2>", True, False),
                        ("os<8,2,2>", True, True), ("os<4,1,4>", False, True), ("os<4,1,4>", True, True),
                        ("os<8,1,4>", False, True), ("os<8,1,4>", True, True), ("stream<4,1,4>", False, True),
                        ("stream<4,2,5>", True, True), ("stream<4,2,6>", False, True), ("stream<4,2,6>", True, False),
                        ("stream<4,2,8>", True, False), ("stream<4,2,8>", True, True), ("stream<8,2,16>", False, True),
                        ("stream<8,2,16>", True, True)]

# part 3: one LDS-resident batch and one streamed (lp 608) batch per layout, the largest N, spread over ZO / SURF
UNREAD_BATCHES = [(lay, j % 2 == 1, (j // 2) % 2 == 1, LAYOUTS[lay][-1][0], LAYOUTS[lay][-1][1][-1])
                  for j, lay in enumerate(LAYOUTS)]


def _batch_id(b):
    lay, zo, surf, n, lp = b
    return "%s-%s-%s-N%d-lp%d" % (lay.replace("<", "_").replace(">", "").replace(",", "_"), "ZO" if zo else "noZO",
                                  "SURF" if surf else "noSURF", n, lp)


def _settings(i, surf):
    """Boundary conditions of batch i of BATCHES, spread over the table: sun first / last, ground, ipolar, igmax."""
    sun_last = bin(i).count("1") % 2 == 1                     # (Thue-Morse: no period shared with the table's loops)
    kw = dict(ipolar=0 if i % 7 == 3 else 1, igmax=4 if i % 5 == 2 else 100)
    if surf:
        kw.update(ro=0.02, imat_surf=1)
    else:
        kw.update([dict(ro=0.1), dict(ro=0.0), dict(ro=0.05, ifresnel=1, ind_surf=1.34)][(i // 2) % 3])
    return sun_last, kw


def _angles(n, sun_last):
    """N directions as the product builds them: Gauss nodes plus the sun with weight 0 (SOS_ANGLES); above 81 directions the
    Gauss count stops at 80 and zero-weight user directions fill up (like cases user_angles_n28).  The sun is the first
    direction (n0 = 1) or the last (n0 = N)."""
    ng = min(n - 1, 80)
    x, _ = np.polynomial.legendre.leggauss(2 * ng)
    nodes = x[ng:]
    mus = 0.5 * nodes.min() if sun_last else 0.5 * (1.0 + nodes.max())
    mu, w, n0 = S.gauss_angles(ng, float(np.degrees(np.arccos(mus))))
    nu = n - 1 - ng
    if nu:
        extra = np.cos(np.radians(np.linspace(12.0, 70.0, nu)))
        mu_all = np.concatenate([mu, extra])
        w_all = np.concatenate([w, np.zeros(nu)])
        order = np.argsort(-mu_all, kind="stable")
        ms = mu[n0 - 1]
        mu, w = mu_all[order], w_all[order]
        n0 = int(np.where(mu == ms)[0][0]) + 1
    assert len(mu) == n and n0 == (n if sun_last else 1)
    return mu, w, n0


def make_batch(lay, zo, surf, n, lp):
    i = BATCHES.index((lay, zo, surf, n, lp))
    sun_last, kw = _settings(i, surf)
    mu, w, n0 = _angles(n, sun_last)
    os_nb = 24 if n <= 42 else 8
    nts = NTS[lp]
    nb = len(nts)
    iborm = np.roll(np.array([0, os_nb, os_nb // 2 + 1, 2, os_nb - 1][:nb], dtype=np.int32), i % nb)
    bins = []
    for k, nt in enumerate(nts):
        # (total optical depth <= 2.5: with the sun at the last direction, mus ~ 0.005 at N = 85, exp(-tau / mus) stays above
        #  the double range's end -- beyond tau / mus ~ 745 the reference formulation itself returns 0 / 0 = NaN)
        h, x, y, z = S.profile(nt, tau_a=0.2 + 0.1 * k, k_abs=[0.0, 0.3, 2.0, 0.05, 1.0][k])
        h, x, y, _ = S.rescale_profile(h, x, y, 0.0, 0.95, 0.95, os_nb)
        bins.append((h, x, y, z))
    if surf:
        kw["rsurf"] = cases._surf_matrices(n, os_nb, 11 + i)
    return dict(i=i, layout=lay, n=n, lp=lp, mu=mu, w=w, n0=n0, os_nb=os_nb, nt=np.array(nts, dtype=np.int32),
                iborm=iborm, bins=bins, kw=kw, zout=1.5 if zo else -1.0)


def _context(pkg, b, g=0.7, rscale=1.0):
    al, be, ga, ze = S.hg_phase(b["os_nb"], g)
    kw = dict(b["kw"])
    if "rsurf" in kw:
        kw["rsurf"] = (rscale * kw["rsurf"]).astype(np.float32)
    return pkg.SosContext(b["mu"], b["w"], b["n0"], al, be, ga, ze, iborm_max=b["os_nb"], **kw)


def _upload(cx, b, rows=None, nan_pad=False):
    """Bins `rows` of the batch, padded to lp levels (the full batch's width, so that every subset routes alike); nan_pad fills
    levels NT+1 ... lp-1 of every bin with NaN on the device."""
    import torch
    rows = list(range(len(b["bins"]))) if rows is None else list(rows)
    lp = b["lp"]
    arr = [np.zeros((len(rows), lp)) for _ in range(4)]
    for r, k in enumerate(rows):
        for a, v in zip(arr, b["bins"][k]):
            a[r, :len(v)] = v
    bins = cx.upload_bins(arr[0], arr[1], arr[2], nt=b["nt"][rows], iborm=b["iborm"][rows], zout=b["zout"], zprof=arr[3])
    assert bins["lp"] == lp
    if nan_pad:
        for r, k in enumerate(rows):
            bins["prof"][r, :, int(b["nt"][k]) + 1:] = float("nan")
        torch.cuda.synchronize()
    return bins


def _fetch(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, ref, rows, what):
    """Bit for bit: order counts, scattering-order counts, fluxes, and the records of the orders each bin ran."""
    for r, k in enumerate(rows):
        for key in ("norders", "iglast", "flux"):
            assert np.array_equal(got[key][r], ref[key][k]), (what, k, key, got[key][r], ref[key][k])
        f = int(ref["norders"][k])
        assert f > 0, (what, k, f)
        assert np.array_equal(got["rec"][r, :f], ref["rec"][k, :f]), (what, k)


_POOL = ThreadPoolExecutor(max_workers=5)     # the oracle is plain C called through ctypes (the GIL is released)


def _oracle_futures(oracle, b):
    al, be, ga, ze = S.hg_phase(b["os_nb"], 0.7)
    futs = []
    for k, (h, x, y, z) in enumerate(b["bins"]):
        kw = dict(b["kw"])
        ib = int(b["iborm"][k])
        if "rsurf" in kw:
            kw["rsurf"] = kw["rsurf"][:ib + 1]
        futs.append(_POOL.submit(oracle.sos_os, b["mu"], b["w"], b["os_nb"], h, x, y, al, be, ga, ze, n0=b["n0"], zprof=z,
                                 zout=b["zout"], iborm=ib, **kw))
    return futs


# ---- 4. the table itself (CPU) ------------------------------------------------------------------------------------------

def test_table_covers_every_instantiation(pkg, monkeypatch):
    monkeypatch.delenv("SOSGPU_STREAM_PERSIST", raising=False)                    # (route reads the plan as a solve would)
    assert len(LAYOUTS) == 11 and set(N_RANGE) == set(LAYOUTS)
    # every N at every padded level count: exactly one layout of the tables holds (N, lp) -- N in its range, lp between the
    # smallest and the largest lp of its batches -- and it is the one the library's plan names
    span = {lay: (min(lp for _, lps in c for lp in lps), max(lp for _, lps in c for lp in lps)) for lay, c in LAYOUTS.items()}
    for lp in NTS:
        for n in range(3, 86):
            held = [lay for lay, (lo, hi) in N_RANGE.items() if lo <= n <= hi and span[lay][0] <= lp <= span[lay][1]]
            assert held == [route(n, lp)], (n, lp, held, route(n, lp))
    cells = {(lay, zo, surf) for lay, zo, surf, _, _ in BATCHES}
    assert len(cells) == 44
    for lay, zo, surf, n, lp in BATCHES:
        assert route(n, lp) == lay, (lay, n, lp, route(n, lp))
        assert len(NTS[lp]) in (3, 4, 5) and 1 in NTS[lp] and lp - 1 in NTS[lp]
        assert _round_up(max(NTS[lp]) + 1, 16) == lp                             # (upload_bins pads to lp)
    for lay, (lo, hi) in N_RANGE.items():
        lps = {lp for _, lps in LAYOUTS[lay] for lp in lps}
        for lp in lps:                                                           # the corners are the layout's ends
            assert route(lo, lp) == lay and route(hi, lp) == lay
            assert lo == 3 or route(lo - 1, lp) != lay
            assert hi == 85 or route(hi + 1, lp) != lay
        for zo in (False, True):
            for surf in (False, True):
                ns = {n for l2, z2, s2, n, _ in BATCHES if (l2, z2, s2) == (lay, zo, surf)}
                assert {lo, hi} <= ns, (lay, zo, surf, ns)
                if lay.startswith("stream"):
                    for n in ns:
                        got = {lp for l2, z2, s2, n2, lp in BATCHES if (l2, z2, s2, n2) == (lay, zo, surf, n)}
                        assert got == {48 if n > 42 else 80, 608}, (lay, zo, surf, n, got)
    assert {n for l, _, _, n, _ in BATCHES if l == "os<4,2,2,SPLIT>"} == {22, 26, 27, 32}
    assert {(_round_up(3 * n, 8) + 15) // 16 for n in (22, 26, 27, 32)} == {5, 6}
    assert 85 in {n for _, _, _, n, _ in BATCHES}
    assert len(PREVIOUSLY_UNCHECKED) == 19 and set(PREVIOUSLY_UNCHECKED) <= cells
    # the boundary conditions are spread over the table
    seen = dict(first=set(), last=set())
    grounds, ipolar0, igmax = set(), 0, 0
    for i, (lay, zo, surf, n, lp) in enumerate(BATCHES):
        sun_last, kw = _settings(i, surf)
        seen["last" if sun_last else "first"].add(lay)
        if not surf:
            grounds.add("fresnel" if kw.get("ifresnel") else "black" if kw["ro"] == 0 else "lambert")
        ipolar0 += kw["ipolar"] == 0
        igmax += kw["igmax"] < 100
    assert seen["first"] == seen["last"] == set(LAYOUTS)
    assert grounds == {"lambert", "black", "fresnel"} and ipolar0 and igmax
    assert {route(n, lp) for lay, zo, surf, n, lp in UNREAD_BATCHES} == set(LAYOUTS)
    for lay, zo, surf, n, lp in UNREAD_BATCHES:
        assert (lay, zo, surf, n, lp) in BATCHES and (lay.startswith("os") or lp == 608)


def test_batch_angles_and_levels():
    """The inputs the GPU tests build: N directions with the sun where the table puts it, ragged NT and IBORM per batch."""
    for b in (make_batch(*BATCHES[0]), make_batch(*[x for x in BATCHES if x[3] == 85 and x[4] == 608][-1])):
        assert len(b["mu"]) == b["n"] and np.all(np.diff(b["mu"]) < 0) and b["w"][b["n0"] - 1] == 0.0
        assert {0, b["os_nb"]} <= set(b["iborm"].tolist())
        assert [len(x[0]) - 1 for x in b["bins"]] == b["nt"].tolist()
    b = make_batch(*[x for x in BATCHES if x[3] == 85][0])
    assert (b["w"] == 0).sum() == 5                    # the sun and four user directions


# ---- 1. the matrix against the oracle ----------------------------------------------------------------------------------

def _assert_bin_vs_oracle(got, k, rec, ref, records, what):
    """Row k of the fetched outputs `got`, its records `rec`, against the oracle's solve `ref` and its `records`."""
    f = len(records)
    assert np.isfinite(records).all() and np.isfinite(rec).all(), what
    assert ref["ier"] == 0 and int(got["norders"][k]) == f, (what, int(got["norders"][k]), f)
    assert np.array_equal(got["iglast"][k, :f], ref["ig_counts"]), (what, got["iglast"][k, :f], ref["ig_counts"])
    cases.compare_records(rec[:f], records, 1e-9, what)
    assert abs(got["flux"][k, 0] - ref["emoins"]) <= 1e-9 * abs(ref["emoins"]) + 1e-300, what
    assert abs(got["flux"][k, 1] - ref["eplus"]) <= 1e-9 * abs(ref["eplus"]) + 1e-300, what


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES, ids=_batch_id)
def test_instantiation_vs_oracle(gpu_pkg, oracle, batch):
    b = make_batch(*batch)
    futs = _oracle_futures(oracle, b)
    cx = _context(gpu_pkg, b)
    got = _fetch(cx.solve(_upload(cx, b)))
    cx.close()
    for k, fut in enumerate(futs):
        ref = fut.result()
        what = "%s bin %d NT=%d IBORM=%d n0=%d %s" % (_batch_id(batch), k, b["nt"][k], b["iborm"][k], b["n0"],
                                                    {a: v for a, v in b["kw"].items() if a != "rsurf"})
        _assert_bin_vs_oracle(got, k, got["rec"][k], ref, ref["records"], what)


# ---- 2. launch forms and the multi-context kernels, bit for bit -------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES, ids=_batch_id)
def test_launch_forms_and_multi_context_bitwise(gpu_pkg, monkeypatch, batch):
    """Streamed cells: the default (order-parallel for up to 128 bins) form against one workgroup per bin, and the persistent
    form of the full-width layouts.  Every cell: the bins split between two contexts with different phase functions (and
    surface matrices) in ONE solve_spectrum launch -- the _multi twin -- against the single-context solves of each half."""
    import torch
    b = make_batch(*batch)
    nb = len(b["bins"])
    cx = _context(gpu_pkg, b)
    ref = _fetch(cx.solve(_upload(cx, b)))
    rows = list(range(nb))
    if batch[0].startswith("stream"):
        forms = [("SOSGPU_STREAM_SPEC", "0")] + ([("SOSGPU_STREAM_PERSIST", "1")] if batch[0] in FULL_WIDTH else [])
        for var, val in forms:
            monkeypatch.setenv(var, val)
            _assert_same(_fetch(cx.solve(_upload(cx, b))), ref, rows, "%s %s=%s" % (_batch_id(batch), var, val))
            monkeypatch.delenv(var)
    cx2 = _context(gpu_pkg, b, g=0.8, rscale=1.5)
    ra, rb = rows[0::2], rows[1::2]
    ba, bb = _upload(cx, b, ra), _upload(cx2, b, rb)
    ref_a, ref_b = _fetch(cx.solve(ba)), _fetch(cx2.solve(bb))
    _assert_same(ref_a, ref, ra, "%s subset" % _batch_id(batch))                  # bins are independent
    table = gpu_pkg.solver.ContextTable([cx, cx2])
    bins, cob, seg = gpu_pkg.solver.concat_bins([ba, bb])
    out = cx.alloc_outputs(bins["nb"])
    gpu_pkg.solver.solve_spectrum(table, bins, cob, seg, torch.full((nb,), 1.0 / nb, dtype=torch.float64, device=cx.device),
                                  out=out)
    got = _fetch(out)
    _assert_same({k: v[:len(ra)] for k, v in got.items()}, ref_a, range(len(ra)), "%s multi ctx 0" % _batch_id(batch))
    _assert_same({k: v[len(ra):] for k, v in got.items()}, ref_b, range(len(rb)), "%s multi ctx 1" % _batch_id(batch))
    cx.close()
    cx2.close()


# ---- 2b. the widened layout in the plain form ------------------------------------------------------------------------------

WIDENED = [("stream<4,2,5>", 22, 80), ("stream<4,2,6>", 32, 80)]


def _oracle_levels(oracle, b, k, g, zouts):
    al, be, ga, ze = S.hg_phase(b["os_nb"], g)
    h, x, y, z = b["bins"][k]
    kw = dict(b["kw"])
    ib = int(b["iborm"][k])
    if "rsurf" in kw:
        kw["rsurf"] = kw["rsurf"][:ib + 1]
    return oracle.sos_os_levels(b["mu"], b["w"], b["os_nb"], h, x, y, al, be, ga, ze, zouts, n0=b["n0"], zprof=z, iborm=ib, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("surf", (False, True), ids=("noSURF", "SURF"))
@pytest.mark.parametrize("lay,n,lp", WIDENED, ids=("N22", "N32"))
def test_widened_layout_in_the_plain_form_vs_oracle(gpu_pkg, oracle, monkeypatch, lay, n, lp, surf):
    """SOSGPU_STREAM_PERSIST=1 widens the five- and six-tile layouts to eight tiles; a context table and output slots then run
    the plain form (one workgroup per bin) on that layout -- k_sos_stream<4,2,.,.,false,8> below its full row count, which no
    other test launches.  (i) the bins split over two contexts with different phase functions in one solve_spectrum launch,
    (ii) solve_levels with a standard and an interior slot; both against the oracle."""
    import torch
    b = make_batch(lay, False, surf, n, lp)
    nb, zint = len(b["bins"]), 1.5
    ra, rb = list(range(nb))[0::2], list(range(nb))[1::2]
    refs = [_POOL.submit(_oracle_levels, oracle, b, k, 0.7, [-1.0, zint]) for k in range(nb)]
    refs_b = {k: _POOL.submit(_oracle_levels, oracle, b, k, 0.8, [-1.0]) for k in rb}
    monkeypatch.setenv("SOSGPU_STREAM_PERSIST", "1")
    assert route(n, lp) == "stream<4,2,8>"
    cx, cx2 = _context(gpu_pkg, b), _context(gpu_pkg, b, g=0.8)
    try:
        ba, bb = _upload(cx, b, ra), _upload(cx2, b, rb)
        table = gpu_pkg.solver.ContextTable([cx, cx2])
        bins, cob, seg = gpu_pkg.solver.concat_bins([ba, bb])
        out = cx.alloc_outputs(bins["nb"])
        gpu_pkg.solver.solve_spectrum(table, bins, cob, seg, torch.full((nb,), 1.0 / nb, dtype=torch.float64, device=cx.device),
                                      out=out)
        multi = _fetch(out)
        full = _upload(cx, b)
        lv = cx.output_levels(full, [-1.0, zint])
        assert (lv["jout"][1] > 0).all()                                         # the second slot is interior in every bin
        slots = _fetch(cx.solve_levels(full, lv))
    finally:
        cx.close()
        cx2.close()
    what = "%s PERSIST=1" % _batch_id((lay, False, surf, n, lp))
    for r, k in enumerate(ra + rb):
        ref = (refs[k] if k in ra else refs_b[k]).result()
        _assert_bin_vs_oracle(multi, r, multi["rec"][r], ref, ref["records"][0], "%s table, bin %d" % (what, k))
    for k in range(nb):
        ref = refs[k].result()
        for slot in (0, 1):
            _assert_bin_vs_oracle(slots, k, slots["rec"][slot, k], ref, ref["records"][slot], "%s slot %d, bin %d" % (what, slot, k))


# ---- 3. results independent of memory the kernel must not read ---------------------------------------------------------

def _poison_scratch(pkg, cx):
    """Fill the context's whole streamed-solver scratch with 0xFF bytes (a NaN pattern), between two device synchronisations.
    hipMemset is resolved through libsosgpu.so's own dependencies: the HIP runtime the library (and torch) use."""
    import torch
    p, nd, off = C.c_void_p(), C.c_size_t(), C.c_size_t()
    pkg.capi.check(pkg.capi.lib().sosgpu_debug_scratch(cx._h, C.byref(p), C.byref(nd), C.byref(off)), "sosgpu_debug_scratch")
    assert p.value and nd.value > 0
    hip = C.CDLL(pkg.capi.SO_PATH)
    hip.hipMemset.restype = C.c_int
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipDeviceSynchronize.restype = C.c_int
    torch.cuda.synchronize()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemset(p, 0xFF, nd.value * 8) == 0
    assert hip.hipDeviceSynchronize() == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", UNREAD_BATCHES, ids=_batch_id)
def test_results_ignore_pad_levels_and_stale_scratch(gpu_pkg, monkeypatch, batch):
    """Levels NT+1 ... lp-1 of every bin hold NaN: the records are bit for bit those of the zero-padded upload.  Streamed
    layouts: after a solve, the scratch (reused from solve to solve without clearing, csrc/api_solve.hip) is overwritten with NaN
    bytes and the next solve is again bit for bit the clean one -- in the default and the one-workgroup-per-bin form."""
    b = make_batch(*batch)
    rows = range(len(b["bins"]))
    cx = _context(gpu_pkg, b)
    ref = _fetch(cx.solve(_upload(cx, b)))
    _assert_same(_fetch(cx.solve(_upload(cx, b, nan_pad=True))), ref, rows, "%s NaN pad" % _batch_id(batch))
    if batch[0].startswith("stream"):
        for form in ("default", "per-bin"):
            if form == "per-bin":
                monkeypatch.setenv("SOSGPU_STREAM_SPEC", "0")
                _fetch(cx.solve(_upload(cx, b)))                 # (sizes the scratch for this form)
            _poison_scratch(gpu_pkg, cx)
            _assert_same(_fetch(cx.solve(_upload(cx, b))), ref, rows, "%s %s form, 0xFF scratch" % (_batch_id(batch), form))
    cx.close()
