"""The operator tables of many contexts in one call (sosgpu_noyaux_spectrum, solver.build_operators): the table forms
k_gsf_table, k_pack_table, k_pack_ray_table, k_sv_table (csrc/noyaux.hip) and k_pack_ground_table (csrc/api_operators.hip) against the
per-context calls bit for bit and against the oracle, on batches that mix every size, next to other contexts' tables on
recycled pool blocks, the refusals of the entry point, and the wiring into run_sos.sos_spectrum / sos_spectrum_levels (call
counts, outputs).

The cells, their inputs and the oracle check are those of test_context_tables (CELLS, cell_inputs, check_tables); n43 and n85
stay out of the batches: their tables take hundreds of MB and that sweep covers them per context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectrum_cases
from spectrum_cases import assert_tuples_equal
from test_context_tables import CELLS, RECYCLE, _context, _size_class, cell_inputs, check_tables, coefficients, directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = spectrum_cases.GOLD
BATCH = [k for k in CELLS if k not in ("n43", "n85")]
ARRAYS = ("prt", "mp_aer", "mp_vt", "mp_uf", "sv", "rowmap", "mp_gnd", "rdir")
E_ARG = -1

# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_symbol_is_declared_exported_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"\bint\s+sosgpu_noyaux_spectrum\s*\(sosgpu_ctx \*const \*ctxs, int nctx, const float \*const \*d_rsurf, "
                     r"void \*d_work, size_t work_bytes,\s*void \*stream\);", hdr)
    assert re.search(r"\bsize_t\s+sosgpu_noyaux_spectrum_work_bytes\s*\(int nctx\);", hdr)
    for sym in ("sosgpu_noyaux_spectrum", "sosgpu_noyaux_spectrum_work_bytes"):
        assert sym in pkg.capi.EXPORTS and hasattr(pkg.capi.lib(), sym)


def test_arguments_are_refused_without_a_device(pkg):
    """NULL ctxs, NULL d_work and nctx = -1 are refused, and nctx = 0 is accepted, before any device is looked for."""
    L = pkg.capi.lib()
    hs = (C.c_void_p * 1)(None)
    work, nw = C.c_void_p(4096), 1 << 30                     # never dereferenced: nothing is queued by these calls
    assert L.sosgpu_noyaux_spectrum(None, 1, None, work, nw, None) == E_ARG
    assert L.sosgpu_noyaux_spectrum(hs, 1, None, None, nw, None) == E_ARG
    assert L.sosgpu_noyaux_spectrum(hs, -1, None, work, nw, None) == E_ARG
    assert L.sosgpu_noyaux_spectrum(hs, 65536, None, work, nw, None) == E_ARG
    assert L.sosgpu_noyaux_spectrum(hs, 0, None, work, nw, None) == 0


def test_batch_covers_the_mix_it_claims():
    assert len(BATCH) == 17 and BATCH == [k for k in CELLS][:13] + [k for k in CELLS][15:]
    c = [CELLS[k] for k in BATCH]
    ns = [len(cell_inputs(k)["mu"]) for k in BATCH]
    assert min(ns) == 2 and max(ns) == 42
    assert {x["os_nb"] for x in c} == {2, 3, 24, 80}
    assert {0, 1, 2, 3} <= {x["smax"] for x in c} and any(x["smax"] == x["os_nb"] - 1 for x in c)
    assert any(x["smax"] == x["os_nb"] for x in c)
    assert {x["ipolar"] for x in c} == {0, 1} and {x["ifresnel"] for x in c} == {0, 1}
    flags = [x["surf"] for x in c]
    assert sum(flags) == 4 and flags[-4:] == [True] * 4     # table order: the four surface cells follow the cells without
    # the extra order of the GPU test puts each surface cell between cells that have none
    order = _mixed(BATCH)
    flags = [CELLS[k]["surf"] for k in order]
    assert sorted(order) == sorted(BATCH) and not flags[0] and not flags[-1]
    assert sum(1 for a, b in zip(flags, flags[1:]) if a != b) == 8


def _mixed(names):
    """Every surface cell between two cells without matrices."""
    plain = [k for k in names if not CELLS[k]["surf"]]
    surf = [k for k in names if CELLS[k]["surf"]]
    return plain[:3] + surf[:1] + plain[3:6] + surf[1:2] + plain[6:9] + surf[2:3] + plain[9:12] + surf[3:] + plain[12:]


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _unbuilt(gpu_pkg, name, smax=None):
    """The context of test_context_tables._context, created only (build=False)."""
    c, i = CELLS[name], cell_inputs(name)
    al, be, ga, ze = i["coefs"]
    smax = c["smax"] if smax is None else smax
    rs = None if i["rsurf"] is None else i["rsurf"][:smax + 1]
    cx = gpu_pkg.SosContext(i["mu"], i["wt"], i["n0"], al, be, ga, ze, iborm_max=smax, ro=c["ro"],
                            imat_surf=1 if c["surf"] else 0, ifresnel=c["ifresnel"], ind_surf=1.34, ron=c["ron"],
                            ipolar=c["ipolar"], rsurf=rs, build=False)
    assert not cx._built
    return cx


_REFERENCE = {}


def reference_tables(gpu_pkg, name):
    """debug_tables of a context of the cell built the present way (sosgpu_set_surface_matrices_async + sosgpu_noyaux),
    made once per session and never changed."""
    if name not in _REFERENCE:
        cx = _context(gpu_pkg, name)
        try:
            t = cx.debug_tables()
        finally:
            cx.close()
        for k in ARRAYS:
            if k in t:
                t[k].setflags(write=False)
        _REFERENCE[name] = t
    return _REFERENCE[name]


def _close(ctxs):
    for cx in ctxs:
        cx.close()


def _assert_same_tables(gpu_pkg, cx, name, what):
    ref, got = reference_tables(gpu_pkg, name), cx.debug_tables()
    for k in ARRAYS:
        assert (k in ref) == (k in got) == (CELLS[name]["surf"] or k not in ("mp_gnd", "rdir")), (what, name, k)
        if k in ref:
            assert ref[k].shape == got[k].shape and np.array_equal(ref[k], got[k]), \
                (what, name, k, int(np.count_nonzero(ref[k] != got[k])))
    for k in ("n", "w", "kp", "kh", "ks2h", "rtph", "nwgt", "prow", "os_nb", "smax", "n0", "ipolar"):
        assert ref[k] == got[k], (what, name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["table order", "reversed", "one context", "surface cells apart"])
def test_batch_equals_the_per_context_calls_bitwise(gpu_pkg, order):
    """One sosgpu_noyaux_spectrum call over the 17 cells -- N 2..42, OS_NB 2, 3, 24, 80, smax 0, 1, 2, 3, OS_NB - 1 and OS_NB,
    IPOLAR 0, Fresnel, four surface cells after thirteen that have none -- leaves every array of debug_tables of every
    context equal to that of a context built by the two per-context calls; also with the list reversed (the owner of the
    largest grid changes place), with nctx = 1 (a cell without and a cell with surface matrices) and with every surface cell
    between two cells that have none."""
    S = gpu_pkg.solver
    lists = {"table order": [BATCH], "reversed": [BATCH[::-1]], "one context": [["n2"], ["gnd_n5"]],
             "surface cells apart": [_mixed(BATCH)]}[order]
    for names in lists:
        ctxs = []
        try:
            ctxs = [_unbuilt(gpu_pkg, k) for k in names]
            assert S.build_operators(ctxs) == len(names)
            assert all(cx._built for cx in ctxs) and S.build_operators(ctxs) == 0
            for k, cx in zip(names, ctxs):
                _assert_same_tables(gpu_pkg, cx, k, order)
        finally:
            _close(ctxs)


@pytest.mark.gpu
def test_batch_built_tables_vs_oracle(gpu_pkg, oracle):
    """check_tables of test_context_tables -- every entry against the oracle -- on contexts built in one batch."""
    names = ["n2", "n5", "n16", "n26", "gnd_n5", "gnd_n16", "gnd_n27"]
    ctxs = []
    try:
        ctxs = [_unbuilt(gpu_pkg, k) for k in names]
        gpu_pkg.solver.build_operators(ctxs)
        for k, cx in zip(names, ctxs):
            cnt, dist, _ = check_tables(oracle, cx, k)
            print(k, "entries compared:", cnt, "start distance %.3f ulp" % dist)
    finally:
        _close(ctxs)


@pytest.mark.gpu
def test_batch_on_recycled_blocks_next_to_smaller_neighbours(gpu_pkg, oracle):
    """The donors of test_context_tables.RECYCLE are built and destroyed; the recipients get their blocks from the pool and
    are built in ONE batch with neighbours of a smaller smax (so the grid is larger than a neighbour needs in every
    dimension).  check_tables on all of them: never-written entries were not needed, padding and the entries below the start
    order are 0 where the donor left numbers, and nothing was written outside a context's own tables."""
    L = gpu_pkg.capi.lib()
    L.sosgpu_trim()
    donors = []
    try:
        for name, smax, d in RECYCLE.values():
            dmu, dwt, dn0 = directions(d["ng"], d["sun"])
            rs = None
            if d["surf"]:
                rs = np.random.default_rng(d["seed"]).uniform(-5.0, 5.0, (d["smax"] + 1, 9, len(dmu), len(dmu))).astype(np.float32)
            donors.append(gpu_pkg.SosContext(dmu, dwt, dn0, *[1e3 * x for x in coefficients("random", d["os_nb"], d["seed"])],
                                             iborm_max=d["smax"], ro=d["ro"], imat_surf=1 if d["surf"] else 0, rsurf=rs))
        classes = [_size_class(L.sosgpu_ctx_bytes(cx._h)) for cx in donors]
    finally:
        _close(donors)                                       # (all alive until here: the two n22 donors are of one shape)
    todo = [(name, smax) for name, smax, _ in RECYCLE.values()]
    todo = [todo[0], ("n5", None), todo[1], todo[2], ("gnd_n5", None), todo[3], ("n16", None)]
    ctxs = []
    try:
        ctxs = [_unbuilt(gpu_pkg, k, smax) for k, smax in todo]
        got = [_size_class(L.sosgpu_ctx_bytes(ctxs[i]._h)) for i in (0, 2, 3, 5)]
        assert got == classes, "the recipients must be of the donors' size classes"
        gpu_pkg.solver.build_operators(ctxs)
        for (k, smax), cx in zip(todo, ctxs):
            cnt, _, _ = check_tables(oracle, cx, k, smax=smax)
            print(k, smax, "entries compared:", cnt)
    finally:
        _close(ctxs)


@pytest.mark.gpu
def test_refusals_change_nothing(gpu_pkg):
    """A NULL entry in ctxs, imat_surf = 1 with a NULL matrix pointer (the entry, and the whole argument) and a matrix pointer
    for a context without matrices give SOSGPU_E_ARG; the same contexts built properly afterwards hold the right tables."""
    import torch
    L, S = gpu_pkg.capi.lib(), gpu_pkg.solver
    nw = int(L.sosgpu_noyaux_spectrum_work_bytes(4))
    work = torch.empty(nw, dtype=torch.uint8, device="cuda")
    wp = C.c_void_p(work.data_ptr())
    for case in ("null context", "null matrices", "null matrix argument", "matrices for none"):
        plain, gnd = _unbuilt(gpu_pkg, "n5"), _unbuilt(gpu_pkg, "gnd_n5")
        try:
            st = plain._stream()
            r = C.c_void_p(gnd._rsurf.data_ptr())
            if case == "null context":
                rc = L.sosgpu_noyaux_spectrum((C.c_void_p * 3)(plain._h, gnd._h, None), 3, (C.c_void_p * 3)(None, r, None), wp, nw, st)
            elif case == "null matrices":
                rc = L.sosgpu_noyaux_spectrum((C.c_void_p * 2)(plain._h, gnd._h), 2, (C.c_void_p * 2)(None, None), wp, nw, st)
            elif case == "null matrix argument":
                rc = L.sosgpu_noyaux_spectrum((C.c_void_p * 2)(plain._h, gnd._h), 2, None, wp, nw, st)
            else:
                rc = L.sosgpu_noyaux_spectrum((C.c_void_p * 2)(plain._h, gnd._h), 2, (C.c_void_p * 2)(r, r), wp, nw, st)
            assert rc == E_ARG, case
            assert S.build_operators([plain, gnd]) == 2
            _assert_same_tables(gpu_pkg, plain, "n5", case)
            _assert_same_tables(gpu_pkg, gnd, "gnd_n5", case)
        finally:
            _close([plain, gnd])
    bad = torch.empty(nw + 8, dtype=torch.uint8, device="cuda")
    plain = _unbuilt(gpu_pkg, "n5")
    try:
        assert L.sosgpu_noyaux_spectrum((C.c_void_p * 1)(plain._h), 1, None, C.c_void_p(bad.data_ptr() + 4), nw,
                                        plain._stream()) == E_ARG
        with pytest.raises(RuntimeError):
            plain.solve(dict(nb=0))
    finally:
        plain.close()


QUALIFYING = ["cfg1_lambert", "cfg2_lnd_lambert", "ckd_h2o_o2_25bins_flatsea", "rand_12", "rand_14", "flatsea_zout", "rand_38"]


def _count(monkeypatch, pkg):
    n = dict(batch=0, contexts=[], noyaux=0)
    S = pkg.solver
    b0, n0 = S.build_operators, S.SosContext.noyaux

    def batch(ctxs):
        n["batch"] += 1
        n["contexts"].append(len(ctxs))
        return b0(ctxs)

    def noyaux(self):
        n["noyaux"] += 1
        return n0(self)

    monkeypatch.setattr(S, "build_operators", batch)
    monkeypatch.setattr(S.SosContext, "noyaux", noyaux)
    return n


@pytest.mark.gpu
def test_spectrum_pass_builds_the_operators_once_per_part(gpu_pkg, tmp_path, monkeypatch):
    """sos_spectrum of qualifying calls with parts=1: solver.build_operators runs once per chunk and SosContext.noyaux not at
    all; with SOS_SPECTRUM_OPERATORS_PER_CALL=1 it is the reverse; a -SOS.Trans call in the list builds its own operators
    (and those of the order-0 contexts of its diffuse transmissions, one per direction)."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_OPERATORS_PER_CALL", raising=False)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=QUALIFYING + ["ckd_o2a_5bins"])
    good, trans = kws[:len(QUALIFYING)], kws[-1]
    assert str(trans["fictrans"]).strip() != "NO_OUTPUT"
    n = _count(monkeypatch, gpu_pkg)
    rs.sos_spectrum(good, parts=1)
    assert (n["batch"], n["contexts"], n["noyaux"]) == (1, [len(good)], 0), n
    n.update(batch=0, contexts=[])
    rs.sos_spectrum(good, parts=1, chunk=3)
    assert (n["batch"], n["contexts"], n["noyaux"]) == (3, [3, 3, 1], 0), n
    n.update(batch=0, contexts=[])
    rs.sos_spectrum_levels([-1, 2.0], [dict(kw, zout=-1.0) for kw in good], parts=1)
    assert (n["batch"], n["contexts"], n["noyaux"]) == (1, [len(good)], 0), n
    n.update(batch=0, contexts=[])
    out = rs.sos_spectrum(good[:3] + [trans] + good[3:], parts=1)
    ndir = int(out[3][0])                                     # the -SOS.Trans call: its own context + one per direction
    assert (n["batch"], n["contexts"], n["noyaux"]) == (1, [len(good)], 1 + ndir), n
    n.update(batch=0, contexts=[], noyaux=0)
    monkeypatch.setenv("SOS_SPECTRUM_OPERATORS_PER_CALL", "1")
    rs.sos_spectrum(good, parts=1)
    assert (n["batch"], n["noyaux"]) == (0, len(good)), n


END_TO_END = ["ckd_o2a_5bins", "ckd_h2o_o2_25bins_flatsea", "cfg1_lambert", "flatsea_zout", "rand_38", "cfg2_lnd_lambert",
              "rand_12", "cfg5_ckd_maignan_25bins", "glitter_polar", "land_roujean"]


@pytest.mark.gpu
def test_spectrum_outputs_equal_sequential_calls_bitwise(gpu_pkg, tmp_path, monkeypatch):
    """End to end with the batched operators: CKD 5- and 25-bin calls, no-gas calls, -SOS.Trans, an output altitude, a
    Cox-Munk and two land surfaces through sos_spectrum (chunk=3, SOS_SPECTRUM_MIN_PART=2) and sos_spectrum_levels (two
    altitudes) equal the sequential sos_proc calls on all 23 outputs, and the same runs with
    SOS_SPECTRUM_OPERATORS_PER_CALL=1."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_OPERATORS_PER_CALL", raising=False)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=END_TO_END)
    assert any(str(kw["fictrans"]).strip() != "NO_OUTPUT" for kw in kws) and any(kw["zout"] != -1.0 for kw in kws)
    assert {1, 3} <= {int(kw["isurf"]) for kw in kws}
    alts = [-1, 3.0]
    kws_levels = [dict(kw, zout=-1.0) for kw in kws]
    seq = [rs.sos_proc(**kw) for kw in kws]
    seq_levels = [[rs.sos_proc(**dict(kw, zout=float(z))) for z in alts] for kw in kws_levels]
    for per_call in (False, True):
        if per_call:
            monkeypatch.setenv("SOS_SPECTRUM_OPERATORS_PER_CALL", "1")
        got = rs.sos_spectrum(kws, chunk=3)
        assert len(got) == len(kws)
        for a, b in zip(seq, got):
            assert_tuples_equal(a, b)
        lev = rs.sos_spectrum_levels(alts, kws_levels)
        assert len(lev) == len(kws)
        for a, b in zip(seq_levels, lev):
            for k in range(len(alts)):
                assert_tuples_equal(a[k], b[k])
