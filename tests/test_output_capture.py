"""The output-altitude capture of the fused solver against the C oracle, with the output level at every edge of the kernels'
level tiling: the streamed kernel's 32-level chunks (first / last level of a chunk, a pair jlo | jhi across a chunk edge and
across a batch boundary of the link pass, the last chunk holding one level / some / 32, the ground, the top layer) and the
LDS-resident kernel's 16-level column tiles.  Both output modes: the K output slots (solve_levels; mode 2) against the
oracle, the one-altitude form (solve with jout / zz; mode 1) bit for bit against the slots.

The oracle solves a bin once and applies the rule of SOS_OS.F:1514-1520 to its whole field once per altitude
(sos_oracle_os_levels); the CPU part pins that form to the single-altitude oracle bit for bit, checks that the table reaches
the positions it claims, that no profile has a layer of zero thickness and that no oracle solve sits near a stop-test tie."""
import numpy as np
import pytest

import cases
import test_variant_matrix as vm

S = cases.S
COLS = 32                                  # levels per chunk of the streamed kernel (csrc/sos_stream.hip)
MAX_SLOTS = 16                             # capi.MAX_OUTPUT_LEVELS

# (family, layout, SURF, N, lp, NT of the bins).  Streamed: the smallest N of each layout; NT 64 / 96 end in a chunk of one
# level, 95 in a full one, 300 in one of 13 levels behind two link batches (chunks 9..2, then 1); N = 3 adds NT = 607 (19
# chunks: link batches 18..11, 10..3, 2..1).  LDS-resident: one N per layout at its largest padded width.
STREAM_N = ((3, "stream<4,1,4>"), (22, "stream<4,2,5>"), (27, "stream<4,2,6>"), (33, "stream<4,2,8>"), (43, "stream<8,2,16>"))
LDS_N = (("os<4,1,2>", 3, 32), ("os<4,2,2,SPLIT>", 22, 32), ("os<4,2,2>", 33, 32), ("os<8,2,2>", 43, 32),
         ("os<4,1,4>", 3, 64), ("os<8,1,4>", 22, 64))
CELLS = [("stream", lay, surf, n, 608 if n == 3 else 304, (1, 64, 95, 96, 300) + ((607,) if n == 3 else ()))
         for n, lay in STREAM_N for surf in (False, True)] + \
        [("lds", lay, surf, n, lp, (1, 2, lp - 1)) for lay, n, lp in LDS_N for surf in (False, True)]
IGMAX4 = (4, 15)                           # cells that leave the scattering loop at IGMAX instead of the geometric tail


def _cell_id(c):
    return "%s-%s-N%d-lp%d" % (c[1].replace("<", "_").replace(">", "").replace(",", "_"), "SURF" if c[2] else "noSURF", c[3], c[4])


def _settings(i, surf):
    """Boundary conditions of cell i: sun first / last, Lambert / black / Fresnel ground, ipolar, igmax -- spread as
    test_variant_matrix._settings does, so that the N = 3 cells of both families hold a Fresnel and an ipolar = 0 cell."""
    sun_last = bin(i).count("1") % 2 == 1
    kw = dict(ipolar=0 if i % 5 == 1 else 1, igmax=4 if i in IGMAX4 else 100)
    if surf:
        kw.update(ro=0.02, imat_surf=1)
    else:
        kw.update([dict(ro=0.1), dict(ro=0.0), dict(ro=0.05, ifresnel=1, ind_surf=1.34)][(i // 2 + 2) % 3])
    return sun_last, kw


def positions(family, lp, nt):
    """Output levels jout of a bin of NT levels."""
    if family == "stream":
        if nt == 607:
            return [96, 97, 352, 353, 576, 577, 606, 607]
        c = nt // COLS                                     # the bin's last chunk
        want = [1, 2, 31, 32, 33, 63, 64, 65, 32 * c - 1, 32 * c, 32 * c + 1, nt - 1, nt]
    else:
        want = [1, 2, 15, 16, 17, 31, nt - 1, nt] + ([32, 33, 47, 48, 49] if lp == 64 else [])
    return sorted({j for j in want if 1 <= j <= nt})


def altitudes(family, lp, zprof):
    """Altitudes of one bin: per position the level itself (weight exactly 1) and the middle of the layer above it; 120 km at
    jout = 1 (weight 0)."""
    nt = len(zprof) - 1
    alts = []
    for j in positions(family, lp, nt):
        alts += [float(zprof[j]), 0.5 * float(zprof[j - 1] + zprof[j])]
        if j == 1:
            alts.append(120.0)
    return alts


_BATCH = {}


def make_cell(cell):
    """The batch of a cell in the form of test_variant_matrix.make_batch, plus alts[bin] and, per slot solve, the slot table
    sel[slot][bin] = index into alts[bin] (-1: the standard output)."""
    if cell in _BATCH:
        return _BATCH[cell]
    family, lay, surf, n, lp, nts = cell
    i = CELLS.index(cell)
    sun_last, kw = _settings(i, surf)
    mu, w, n0 = vm._angles(n, sun_last)
    os_nb = 24 if n <= 42 else 8
    nb = len(nts)
    iborm = np.roll(np.array([0, os_nb, os_nb // 2 + 1, 2, os_nb - 1, os_nb][:nb], dtype=np.int32), i % nb)
    bins = []
    for k, nt in enumerate(nts):
        h, x, y, z = S.profile(nt, tau_a=0.2 + 0.1 * (k % 5), k_abs=[0.0, 0.3, 2.0, 0.05, 1.0, 0.5][k])
        h, x, y, _ = S.rescale_profile(h, x, y, 0.0, 0.95, 0.95, os_nb)
        bins.append((h, x, y, z))
    if surf:
        kw["rsurf"] = cases._surf_matrices(n, os_nb, 31 + i)
    alts = [altitudes(family, lp, z) for _, _, _, z in bins]
    # slot solves: slot 0 is -1, the last slot repeats slot 1, 14 altitudes in between; a bin with fewer altitudes repeats its own
    kmax = max(len(a) for a in alts)
    solves = []
    for s0 in range(0, kmax, MAX_SLOTS - 2):
        ks = list(range(s0, min(s0 + MAX_SLOTS - 2, kmax)))
        sel = [[-1] * nb] + [[k % len(a) for a in alts] for k in ks]
        sel.append(list(sel[1]))
        solves.append(np.array(sel))
    b = dict(i=i, layout=lay, n=n, lp=lp, mu=mu, w=w, n0=n0, os_nb=os_nb, nt=np.array(nts, dtype=np.int32), iborm=iborm,
             bins=bins, kw=kw, zout=-1.0, alts=alts, solves=solves)
    _BATCH[cell] = b
    return b


def slot_levels(pkg, b, sel, rows=None):
    """jout[K][nb], zz[K][nb] of one slot solve from solver.output_levels_host, bin by bin."""
    rows = list(range(len(b["bins"]))) if rows is None else list(rows)
    jout = np.zeros((len(sel), len(rows)), dtype=np.int32)
    zz = np.zeros((len(sel), len(rows)))
    for r, k in enumerate(rows):
        z = [-1.0 if a < 0 else b["alts"][k][a] for a in sel[:, k]]
        j1, z1 = pkg.solver.output_levels_host(b["bins"][k][3][None, :], z)
        jout[:, r], zz[:, r] = j1[:, 0], z1[:, 0]
    return jout, zz


def classes(b):
    """(NT, chunk of jlo, chunk of jhi, position of jhi in its chunk, levels in the last chunk, link batch of jlo's chunk, link
    batch of jhi's chunk, weight is 1) of every altitude of a streamed batch, by the literal rule."""
    out = set()
    for (h, x, y, z), alts in zip(b["bins"], b["alts"]):
        nt = len(z) - 1
        nchunk = nt // COLS + 1
        batch = lambda c: -1 if c == 0 else (nchunk - 1 - c) // 8         # the link pass: chunks nchunk-1 .. 1, eight at a time
        for a in alts:
            j = 1
            while a < z[j]:
                j += 1
            zz = (a - z[j - 1]) / (z[j] - z[j - 1])
            out.add((nt, (j - 1) // COLS, j // COLS, j % COLS, nt - COLS * (nchunk - 1) + 1, batch((j - 1) // COLS),
                     batch(j // COLS), zz == 1.0))
    return out


# ---- the oracle: one levels call per bin, shared by every test of a cell ---------------------------------------------------

_REFS = {}


def _oracle_bin(oracle, b, k, zouts):
    al, be, ga, ze = S.hg_phase(b["os_nb"], 0.7)
    h, x, y, z = b["bins"][k]
    kw = dict(b["kw"])
    ib = int(b["iborm"][k])
    if "rsurf" in kw:
        kw["rsurf"] = kw["rsurf"][:ib + 1]
    return al, be, ga, ze, h, x, y, dict(kw, n0=b["n0"], zprof=z, iborm=ib)


def _levels_call(oracle, b, k):
    al, be, ga, ze, h, x, y, kw = _oracle_bin(oracle, b, k, None)
    return oracle.sos_os_levels(b["mu"], b["w"], b["os_nb"], h, x, y, al, be, ga, ze, [-1.0] + b["alts"][k], **kw)


def oracle_refs(oracle, cell):
    """Futures of the cell's oracle solves: bin k -> dict(records[1 + len(alts[k])][F][3][W], ig_counts, emoins, eplus, margin)."""
    if cell not in _REFS:
        b = make_cell(cell)
        _REFS[cell] = [vm._POOL.submit(_levels_call, oracle, b, k) for k in range(len(b["bins"]))]
    return _REFS[cell]


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_table_routes_and_reaches_its_positions(pkg):
    assert len(CELLS) == 22 and len(set(CELLS)) == 22
    seen = dict(first=set(), last=set())
    grounds = dict(stream=set(), lds=set())
    for i, cell in enumerate(CELLS):
        family, lay, surf, n, lp, nts = cell
        assert vm.route(n, lp) == lay and lay.startswith("stream" if family == "stream" else "os"), cell
        assert vm._round_up(max(nts) + 1, 16) == lp, cell
        assert n == vm.N_RANGE[lay][0] or family == "lds"                     # streamed: the smallest N of the layout
        sun_last, kw = _settings(i, surf)
        seen["last" if sun_last else "first"].add(family)
        if not surf:
            grounds[family].add("fresnel" if kw.get("ifresnel") else "black" if kw["ro"] == 0 else "lambert")
        b = make_cell(cell)
        for (h, x, y, z), alts, nt in zip(b["bins"], b["alts"], nts):
            assert len(z) == nt + 1 and np.all(np.diff(z) < 0), (cell, nt)    # no layer of zero thickness (0 / 0 in the rule)
            assert np.all(np.diff(h) > 0), (cell, nt)
            assert len(set(alts)) == len(alts), (cell, nt)
        for sel in b["solves"]:
            assert 3 <= len(sel) <= MAX_SLOTS and (sel[0] == -1).all() and (sel[-1] == sel[1]).all()
        for k, alts in enumerate(b["alts"]):                                 # every altitude of every bin is in a slot
            assert {a for sel in b["solves"] for a in sel[1:, k]} == set(range(len(alts))), (cell, k)
    assert seen["first"] == seen["last"] == {"stream", "lds"}
    assert grounds["stream"] == grounds["lds"] == {"lambert", "black", "fresnel"}
    assert {CELLS[i][0] for i in IGMAX4} == {"stream", "lds"}
    assert {lay for _, lay, _, _, _, _ in CELLS} == set(vm.LAYOUTS)
    # the positions, by the literal rule on the cells' own profiles (output_levels_host is pinned to it in test_output_levels)
    for cell in CELLS:
        family, lay, surf, n, lp, nts = cell
        b = make_cell(cell)
        for (h, x, y, z), alts, nt in zip(b["bins"], b["alts"], nts):
            jout, zz = pkg.solver.output_levels_host(z[None, :], alts)
            got = sorted(set(jout[:, 0].tolist()))
            assert got == positions(family, lp, nt), (cell, nt, got)
            k = 0
            for j in positions(family, lp, nt):
                assert jout[k, 0] == j and zz[k, 0] == 1.0, (cell, nt, j)       # on the level: weight exactly 1
                assert jout[k + 1, 0] == j and 0.25 < zz[k + 1, 0] < 0.75, (cell, nt, j, zz[k + 1, 0])
                k += 2
                if j == 1:
                    assert jout[k, 0] == 1 and zz[k, 0] == 0.0 and alts[k] == 120.0, (cell, nt)
                    k += 1
            assert k == len(alts)
    for cell in CELLS[:10]:
        cl = classes(make_cell(cell))
        nts = cell[5]
        has = lambda **kw: any(all(dict(zip(("nt", "clo", "chi", "pos", "last", "blo", "bhi", "one"), c))[a] == v
                                   for a, v in kw.items()) for c in cl)
        # a pair across every chunk edge: 31 | 32, 63 | 64 and the edge of each bin's last chunk; weight 1 isolates jhi
        for nt in (64, 95, 96, 300):
            c = nt // COLS
            for lo in (0, 1, c - 1):
                assert has(nt=nt, clo=lo, chi=lo + 1, pos=0, one=True) and has(nt=nt, clo=lo, chi=lo + 1, pos=0, one=False), (nt, lo)
                if COLS * (lo + 1) + 1 <= nt:
                    assert has(nt=nt, clo=lo + 1, chi=lo + 1, pos=1), (nt, lo)  # jlo the first level of a chunk
            assert has(nt=nt, clo=0, chi=0, pos=1) and has(nt=nt, clo=0, chi=0, pos=31)
        # the ground as jhi: in a chunk of one level, in a partial and in a full chunk
        assert has(nt=64, chi=2, pos=0, last=1) and has(nt=96, chi=3, pos=0, last=1)
        assert has(nt=300, chi=9, pos=12, last=13, clo=9) and has(nt=95, chi=2, pos=31, last=32, clo=2)
        assert has(nt=1, clo=0, chi=0, pos=1, last=2)
        # NT = 300: the last chunk of the first link batch (chunk 2) and the second batch (chunk 1)
        assert has(nt=300, clo=1, chi=2, blo=1, bhi=0) and has(nt=300, clo=2, chi=2, bhi=0) and has(nt=300, clo=0, chi=1, bhi=1)
        if 607 in nts:
            assert has(nt=607, clo=10, chi=11, blo=1, bhi=0, pos=0) and has(nt=607, clo=11, chi=11, bhi=0, pos=1)
            assert has(nt=607, clo=2, chi=3, blo=2, bhi=1, pos=0) and has(nt=607, clo=3, chi=3, bhi=1, pos=1)
            assert has(nt=607, clo=17, chi=18, pos=0) and has(nt=607, chi=18, pos=31, last=32, one=True)
    assert sum(607 in c[5] for c in CELLS) == 2


PIN_CELLS = [c for c in CELLS if c[3] == 3]          # the oracle costs milliseconds at N = 3


def test_pin_cells_cover_the_boundary_conditions():
    for family in ("stream", "lds"):
        kws = [_settings(CELLS.index(c), c[2])[1] for c in PIN_CELLS if c[0] == family]
        assert any(k.get("imat_surf") for k in kws) and any(k.get("ifresnel") for k in kws)
        assert any(k["ipolar"] == 0 for k in kws) and any(k["ipolar"] == 1 for k in kws)


@pytest.mark.parametrize("cell", PIN_CELLS, ids=_cell_id)
def test_oracle_levels_equal_single_altitude_oracle(oracle, cell):
    """Slot k of sos_oracle_os_levels == sos_oracle_os(zout = zouts[k]) bit for bit: records, order counts, ig_counts, fluxes."""
    b = make_cell(cell)
    for k, fut in enumerate(oracle_refs(oracle, cell)):
        lv = fut.result()
        al, be, ga, ze, h, x, y, kw = _oracle_bin(oracle, b, k, None)
        zouts = [-1.0] + b["alts"][k]
        assert lv["ier"] == 0 and lv["records"].shape[0] == len(zouts) and lv["records"].shape[1] > 0
        singles = [vm._POOL.submit(oracle.sos_os, b["mu"], b["w"], b["os_nb"], h, x, y, al, be, ga, ze, zout=z, **kw) for z in zouts]
        for s, z in enumerate(zouts):
            one = singles[s].result()
            what = (_cell_id(cell), k, z)
            assert one["ier"] == 0 and np.array_equal(one["ig_counts"], lv["ig_counts"]), what
            assert one["records"].shape == lv["records"][s].shape and np.array_equal(one["records"], lv["records"][s]), what
            assert one["emoins"] == lv["emoins"] and one["eplus"] == lv["eplus"], what
        # two altitudes of one bin differ (the slots are not copies of one another)
        assert not np.array_equal(lv["records"][1], lv["records"][2]), (_cell_id(cell), k)


def test_oracle_solves_are_away_from_stop_test_ties(oracle):
    """Equal order counts are a fair demand only where no stop decision of the oracle is a near tie (the rule of
    test_fixtures_are_away_from_stop_test_ties)."""
    for cell in CELLS:
        oracle_refs(oracle, cell)
    for cell in CELLS:
        for k, fut in enumerate(_REFS[cell]):
            ref = fut.result()
            assert ref["ier"] == 0 and np.isfinite(ref["records"]).all(), (_cell_id(cell), k)
            assert ref["margin"] > 1e-7, (_cell_id(cell), k, ref["margin"])


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def _levels_dict(pkg, cx, b, sel, rows=None):
    import torch
    jout, zz = slot_levels(pkg, b, sel, rows)
    d = cx.device
    return dict(nz=len(sel), jout=torch.as_tensor(jout, device=d), zz=torch.as_tensor(zz, device=d),
                tauout=torch.zeros(zz.shape, dtype=torch.float64, device=d)), jout, zz


def _nan_outputs(cx, nz, nb):
    import torch
    out = cx.alloc_outputs(nb)
    out["rec"] = torch.empty((nz, nb, cx.smax + 1, 3, cx.w), dtype=torch.float64, device=cx.device)
    out["rec"].fill_(float("nan"))
    out["flux"].fill_(float("nan"))
    return out


def _same_slots(got, ref, what):
    for key in ("norders", "iglast", "flux"):
        assert np.array_equal(got[key], ref[key]), (what, key)
    for k in range(ref["norders"].shape[0]):
        f = int(ref["norders"][k])
        assert np.array_equal(got["rec"][:, k, :f], ref["rec"][:, k, :f]), (what, k)


WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_output_capture_vs_oracle(gpu_pkg, oracle, monkeypatch, cell):
    import torch
    family, lay, surf, n, lp, nts = cell
    b = make_cell(cell)
    futs = oracle_refs(oracle, cell)
    nb = len(nts)
    cx = vm._context(gpu_pkg, b)
    worst, entries = 0.0, 0
    try:
        bins = vm._upload(cx, b)
        for si, sel in enumerate(b["solves"]):
            what = "%s solve %d" % (_cell_id(cell), si)
            lv, jout, zz = _levels_dict(gpu_pkg, cx, b, sel)
            # (a) + (e): the slots in the default launch form, into NaN-filled buffers, against the oracle
            got = vm._fetch(cx.solve_levels(bins, lv, out=_nan_outputs(cx, len(sel), nb)))
            for k, fut in enumerate(futs):
                ref = fut.result()
                f = ref["records"].shape[1]
                wk = "%s bin %d NT=%d IBORM=%d" % (what, k, nts[k], b["iborm"][k])
                assert ref["ier"] == 0 and f > 0 and ref["margin"] > 1e-7, (wk, ref["margin"])
                assert int(got["norders"][k]) == f, (wk, int(got["norders"][k]), f)
                assert np.array_equal(got["iglast"][k, :f], ref["ig_counts"]), (wk, got["iglast"][k, :f], ref["ig_counts"])
                assert abs(got["flux"][k, 0] - ref["emoins"]) <= 1e-9 * abs(ref["emoins"]) + 1e-300, wk
                assert abs(got["flux"][k, 1] - ref["eplus"]) <= 1e-9 * abs(ref["eplus"]) + 1e-300, wk
                for s in range(len(sel)):
                    ws = "%s slot %d jout=%d zz=%r" % (wk, s, jout[s, k], zz[s, k])
                    assert np.isfinite(got["rec"][s, k, :f]).all(), ws            # a slot or row never written stays NaN
                    worst = max(worst, cases.compare_records(got["rec"][s, k, :f], ref["records"][sel[s, k] + 1], 1e-9, ws))
                    entries += got["rec"][s, k, :f].size
            # (b) one workgroup per bin
            if family == "stream":
                monkeypatch.setenv("SOSGPU_STREAM_SPEC", "0")
                _same_slots(vm._fetch(cx.solve_levels(bins, lv, out=_nan_outputs(cx, len(sel), nb))), got, what + " SPEC=0")
                monkeypatch.delenv("SOSGPU_STREAM_SPEC")
            # (c) the one-altitude form of every slot, bit for bit the slot
            forms = [None] + (["SOSGPU_STREAM_PERSIST"] if lay in vm.FULL_WIDTH else [])
            for s in range(len(sel) - 1):                                         # (the last slot repeats slot 1)
                one = dict(bins, jout=None, zz=None) if s == 0 else \
                    dict(bins, jout=torch.as_tensor(jout[s], device=cx.device), zz=torch.as_tensor(zz[s], device=cx.device))
                for var in forms:
                    if var:
                        monkeypatch.setenv(var, "1")
                    m1 = vm._fetch(cx.solve(one))
                    if var:
                        monkeypatch.delenv(var)
                    ws = "%s slot %d mode 1 %s" % (what, s, var or "default")
                    for key in ("norders", "iglast", "flux"):
                        assert np.array_equal(m1[key], got[key]), (ws, key)
                    for k in range(nb):
                        f = int(got["norders"][k])
                        assert np.array_equal(m1["rec"][k, :f], got["rec"][s, k, :f]), (ws, k, jout[s, k], zz[s, k])
            for k in range(nb):                                                   # (orders >= norders are never written)
                f = int(got["norders"][k])
                assert np.array_equal(got["rec"][-1, k, :f], got["rec"][1, k, :f]), (what + " repeated slot", k)
    finally:
        cx.close()
    WORST[cell] = (worst, entries)
    print("output capture %s: %d entries, worst relative deviation %.3e" % (_cell_id(cell), entries, worst))


SPECTRUM_CELLS = [CELLS[3], CELLS[17]]              # streamed N = 22 with surface matrices, os<8,2,2> N = 43 with them


@pytest.mark.gpu
@pytest.mark.parametrize("cell", SPECTRUM_CELLS, ids=_cell_id)
def test_output_capture_two_contexts_bitwise(gpu_pkg, cell):
    """The bins split between two contexts of different phase functions in one solve_spectrum_levels launch: the records are
    bit for bit the slots of each context's own solve_levels."""
    import torch
    sv = gpu_pkg.solver
    b = make_cell(cell)
    rows = list(range(len(b["bins"])))
    ra, rb = rows[0::2], rows[1::2]
    cx, cx2 = vm._context(gpu_pkg, b), vm._context(gpu_pkg, b, g=0.8, rscale=1.5)
    try:
        ba, bb = vm._upload(cx, b, ra), vm._upload(cx2, b, rb)
        table = sv.ContextTable([cx, cx2])
        bins, cob, seg = sv.concat_bins([ba, bb])
        nb = bins["nb"]
        aik = torch.full((nb,), 1.0 / nb, dtype=torch.float64, device=cx.device)
        for si, sel in enumerate(b["solves"]):
            la, lb = _levels_dict(gpu_pkg, cx, b, sel, ra)[0], _levels_dict(gpu_pkg, cx2, b, sel, rb)[0]
            refs = [vm._fetch(cx.solve_levels(ba, la)), vm._fetch(cx2.solve_levels(bb, lb))]
            out = _nan_outputs(cx, len(sel), nb)
            sv.solve_spectrum_levels(table, bins, cob, seg, aik, sv.concat_levels([la, lb]), out=out)
            got = vm._fetch(out)
            for c, (ref, sl) in enumerate(zip(refs, (slice(0, len(ra)), slice(len(ra), None)))):
                assert (ref["norders"] > 0).all()
                _same_slots(dict(got, rec=got["rec"][:, sl], norders=got["norders"][sl], iglast=got["iglast"][sl],
                                 flux=got["flux"][sl]), ref, "%s solve %d context %d" % (_cell_id(cell), si, c))
    finally:
        cx.close()
        cx2.close()
