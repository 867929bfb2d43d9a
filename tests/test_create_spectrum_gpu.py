"""sosgpu_create_spectrum on the device (csrc/ctx_fill.hip k_ctx_fill; solver.create_contexts; the context stage of
run_sos._spectrum_pass).  The reference throughout is the per-call path on the same machine: a twin made by sosgpu_create
from the same inputs, and the pass under SOS_SPECTRUM_CONTEXTS_PER_CALL=1.  Everything is compared bit for bit -- the batch
form computes nothing, it moves what the shared host half of sosgpu_create formed -- and three cells also pass the oracle
sweep of test_context_tables on a batch-made context."""
import ctypes as C

import numpy as np
import pytest

import spectrum_cases
from test_context_tables import CELLS, RECYCLE, _context, _size_class, cell_inputs, check_tables, coefficients, directions
from test_create_spectrum import E_ARG, OK, spec_array, spec_of

INFO = ("n", "w", "kp", "kh", "ks2h", "rtph", "nwgt", "prow", "os_nb", "smax", "n0", "ipolar", "beta2", "gamma2", "alpha2",
        "f11sun", "f12sun", "mus", "ro")
SMALL = ("rowmap", "mp_vt", "mp_uf")
TABLES = ("prt", "mp_aer", "mp_vt", "mp_uf", "sv", "mp_gnd", "rdir", "rowmap")


def _smax(name):
    return 3 if CELLS[name]["os_nb"] == 400 else CELLS[name]["smax"]       # (the two OS_NB = 400 cells: iborm_max 3)


def _make(gpu_pkg, name, smax=None, coefs=None, create=True):
    """An unbuilt context of a cell: pending (create=False) or made by sosgpu_create."""
    c, i = CELLS[name], cell_inputs(name)
    al, be, ga, ze = coefs or i["coefs"]
    smax = _smax(name) if smax is None else smax
    rs = None if i["rsurf"] is None else i["rsurf"][:smax + 1]
    return gpu_pkg.SosContext(i["mu"], i["wt"], i["n0"], al, be, ga, ze, iborm_max=smax, ro=c["ro"],
                              imat_surf=1 if c["surf"] else 0, ifresnel=c["ifresnel"], ind_surf=1.34, ron=c["ron"],
                              ipolar=c["ipolar"], rsurf=rs, build=False, create=create)


def _build_per_call(gpu_pkg, cx):
    """What SosContext(build=True) queues: the surface packing and sosgpu_noyaux of this context alone."""
    if cx._rsurf is not None:
        gpu_pkg.capi.check(gpu_pkg.capi.lib().sosgpu_set_surface_matrices_async(cx._h, C.c_void_p(cx._rsurf.data_ptr()),
                                                                                 cx._stream()), "surface matrices")
    cx.noyaux()


def _small_tables(gpu_pkg, cx):
    """The layout numbers and scalars, rowmap, mp_vt and mp_uf of a context that is created and not built."""
    capi = gpu_pkg.capi
    L, info = capi.lib(), capi.TablesInfo()
    capi.check(L.sosgpu_debug_tables(cx._h, C.byref(info), *([None] * 8)), "sosgpu_debug_tables")
    t = {k: getattr(info, k) for k in INFO}
    t.update(rowmap=np.zeros(info.kh, dtype=np.int32), mp_vt=np.zeros((3, info.ks2h * 128)), mp_uf=np.zeros((3, info.rtph * 64)))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(L.sosgpu_debug_tables(cx._h, C.byref(info), None, None, p(t["mp_vt"]), p(t["mp_uf"]), None, None, None,
                                     p(t["rowmap"])), "sosgpu_debug_tables")
    t["bytes"] = L.sosgpu_ctx_bytes(cx._h)
    return t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_same(a, b, keys, where):
    for k in keys:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (where, k)
        else:
            assert np.array_equal(_bits(np.asarray(a[k])), _bits(np.asarray(b[k]))), (where, k, a[k], b[k])


def _assert_built_same(cx, twin, where):
    a, b = cx.debug_tables(), twin.debug_tables()
    assert set(a) == set(b), where
    _assert_same(a, b, INFO + tuple(k for k in TABLES if k in a), where)


def _close(ctxs):
    for cx in ctxs:
        cx.close()


# ------------------------------------------------------------------------------------------------ 1. all cells in one call
@pytest.mark.gpu
def test_all_cells_in_one_call(gpu_pkg, oracle, monkeypatch):
    S = gpu_pkg.solver
    L = gpu_pkg.capi.lib()
    names = [list(CELLS)[k] for k in np.random.default_rng(5).permutation(len(CELLS))]
    assert len(names) == 19
    calls = []
    real = L.sosgpu_create_spectrum
    monkeypatch.setattr(L, "sosgpu_create_spectrum", lambda *a: calls.append(a[3]) or real(*a))
    batch = [_make(gpu_pkg, k, create=False) for k in names]
    twins = []
    try:
        for cx in batch:
            with pytest.raises(RuntimeError, match="create_contexts"):
                cx._h
        assert S.create_contexts(batch) == 19 and calls == [19]
        small = [_small_tables(gpu_pkg, cx) for cx in batch]            # directly after the call
        twins = [_make(gpu_pkg, k) for k in names]
        for k, cx, tw, t in zip(names, batch, twins, small):
            _assert_same(t, _small_tables(gpu_pkg, tw), INFO + SMALL + ("bytes",), k)
        assert S.build_operators(batch) == 19
        for tw in twins:
            _build_per_call(gpu_pkg, tw)
        for k, cx, tw in zip(names, batch, twins):
            _assert_built_same(cx, tw, k)
        for k in ("n2", "n22", "gnd_n27"):
            check_tables(oracle, batch[names.index(k)], k, smax=_smax(k))
        with pytest.raises(ValueError, match="has its handle already"):
            S.create_contexts(batch[:2])
    finally:
        _close(batch + twins)


# ------------------------------------------------------------------------------------------------ 2. recycled blocks
@pytest.mark.gpu
@pytest.mark.parametrize("which", list(RECYCLE))
def test_batch_on_a_recycled_block(gpu_pkg, which):
    """test_context_tables.test_tables_on_a_recycled_block with the recipient made by the batch call: the donor's numbers lie
    in the block the pool hands back, and k_ctx_fill must clear all the memset of sosgpu_create clears."""
    name, smax, d = RECYCLE[which]
    S = gpu_pkg.solver
    L = gpu_pkg.capi.lib()
    L.sosgpu_trim()
    dmu, dwt, dn0 = directions(d["ng"], d["sun"])
    rs = None
    if d["surf"]:
        rs = np.random.default_rng(d["seed"]).uniform(-5.0, 5.0, (d["smax"] + 1, 9, len(dmu), len(dmu))).astype(np.float32)
    donor = gpu_pkg.SosContext(dmu, dwt, dn0, *[1e3 * x for x in coefficients("random", d["os_nb"], d["seed"])],
                               iborm_max=d["smax"], ro=d["ro"], imat_surf=1 if d["surf"] else 0, rsurf=rs)
    td = donor.debug_tables()
    assert np.any(td["mp_aer"] != 0) and np.any(td["mp_vt"] != 0) and np.any(td["mp_uf"] != 0)
    cls = _size_class(L.sosgpu_ctx_bytes(donor._h))
    donor.close()
    cx, twin = _make(gpu_pkg, name, smax=smax, create=False), None
    try:
        S.create_contexts([cx])
        assert _size_class(L.sosgpu_ctx_bytes(cx._h)) == cls, "the recipient must be of the donor's size class"
        before = _small_tables(gpu_pkg, cx)
        twin = _make(gpu_pkg, name, smax=smax)
        _assert_same(before, _small_tables(gpu_pkg, twin), INFO + SMALL + ("bytes",), which)
        S.build_operators([cx])
        _build_per_call(gpu_pkg, twin)
        _assert_built_same(cx, twin, which)
    finally:
        _close([cx] + ([twin] if twin is not None else []))


# ------------------------------------------------------------------------------------------------ 3. many contexts
@pytest.mark.gpu
def test_three_hundred_contexts_and_the_pool(gpu_pkg):
    """300 contexts of the smallest shape in one call (a job table of more than 256 entries); two of them carry other
    coefficients.  Destroyed and made again, the blocks come back from the pool and the result is the same."""
    S = gpu_pkg.solver
    other = {7: coefficients("random", 2, 11), 299: coefficients("random", 2, 12)}
    twins = {i: _make(gpu_pkg, "n2", coefs=other.get(i)) for i in (0, 7, 255, 256, 299)}
    try:
        for tw in twins.values():
            _build_per_call(gpu_pkg, tw)
        want = {i: tw.debug_tables() for i, tw in twins.items()}
        # (the operators carry the coefficients: the three sets are told apart)
        assert not np.array_equal(want[7]["mp_aer"], want[0]["mp_aer"])
        assert not np.array_equal(want[7]["mp_aer"], want[299]["mp_aer"])
        for round_ in range(2):
            batch = [_make(gpu_pkg, "n2", coefs=other.get(i), create=False) for i in range(300)]
            try:
                assert S.create_contexts(batch) == 300 and S.build_operators(batch) == 300
                for i in want:
                    got = batch[i].debug_tables()
                    _assert_same(got, want[i], INFO + tuple(k for k in TABLES if k in got), (round_, i))
            finally:
                _close(batch)
    finally:
        _close(twins.values())


# ------------------------------------------------------------------------------------------------ 4. lifetime
@pytest.mark.gpu
def test_destroy_at_once_and_another_stream(gpu_pkg, oracle):
    import torch
    S = gpu_pkg.solver
    names = ["n22", "gnd_n27", "n5", "n22", "n41", "n22"]
    batch = [_make(gpu_pkg, k, create=False) for k in names]
    S.create_contexts(batch)
    _close(batch)                                        # no synchronisation: the destroys wait for the fill themselves
    cx = _context(gpu_pkg, "n22")                        # a per-call context of a size class just given back
    try:
        check_tables(oracle, cx, "n22")
    finally:
        cx.close()
    st = torch.cuda.Stream()
    batch = [_make(gpu_pkg, k, create=False) for k in names]
    twins = []
    try:
        with torch.cuda.stream(st):
            S.create_contexts(batch)
            S.build_operators(batch)
        twins = [_make(gpu_pkg, k) for k in names]
        for tw in twins:
            _build_per_call(gpu_pkg, tw)
        for k, cx, tw in zip(names, batch, twins):
            _assert_built_same(cx, tw, k)
    finally:
        _close(batch + twins)


# ------------------------------------------------------------------------------------------------ 5. atomic refusal
@pytest.mark.gpu
def test_refusals_leave_nothing_behind(gpu_pkg):
    import torch
    capi, S = gpu_pkg.capi, gpu_pkg.solver
    L, keep = capi.lib(), []
    names = ["n2", "gnd_n5", "n22", "n5"]
    good = [spec_of(capi, k, keep, smax=_smax(k)) for k in names]
    bad = spec_of(capi, "n5", keep, n0=0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(specs, work, nbytes):
        arr = spec_array(capi, specs)
        out = (C.c_void_p * len(specs))(*([0xDEAD0] * len(specs)))
        return L.sosgpu_create_spectrum(out, 0, arr, len(specs), C.c_void_p(work), nbytes, st), list(out)

    need = L.sosgpu_create_spectrum_work_bytes(spec_array(capi, good), 4)
    work = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
    rc, out = call(good[:2] + [bad] + good[2:], work.data_ptr(), need + 4096)
    assert rc == E_ARG and out == [None] * 5
    rc, out = call(good, work.data_ptr(), need - 1)
    assert rc == E_ARG and out == [None] * 4
    rc, out = call(good, work.data_ptr() + 4, need + 8)
    assert rc == E_ARG and out == [None] * 4
    # an area that is 8-byte and not 256-byte aligned is taken: the layout keeps the bytes to start at a 256-byte address
    rc, out = call(good, work.data_ptr() + 8, need)
    assert rc == OK and all(out)
    for h in out:
        L.sosgpu_destroy(C.c_void_p(h))
    batch = [_make(gpu_pkg, k, create=False) for k in names]
    twins = []
    try:
        assert S.create_contexts(batch) == 4
        S.build_operators(batch)
        twins = [_make(gpu_pkg, k) for k in names]
        for tw in twins:
            _build_per_call(gpu_pkg, tw)
        for k, cx, tw in zip(names, batch, twins):
            _assert_built_same(cx, tw, k)
    finally:
        _close(batch + twins)


# ------------------------------------------------------------------------------------------------ 6. one solve
@pytest.mark.gpu
def test_one_solve_on_a_batch_made_context(gpu_pkg):
    """The smallest solvable shape: the directions of n5, orders 0..2, a three-level Rayleigh profile."""
    import torch
    S = gpu_pkg.solver
    h, x, y, _ = gpu_pkg.synth.profile(2, tau_a=0.0)
    assert h.shape == (3,) and not np.any(x) and np.all(y[1:] == 1.0)
    cx, twin = _make(gpu_pkg, "n5", smax=2, create=False), _make(gpu_pkg, "n5", smax=2)
    try:
        S.create_contexts([cx])
        S.build_operators([cx])
        _build_per_call(gpu_pkg, twin)
        outs = []
        for c in (cx, twin):
            o = c.solve(c.upload_bins(h[None], x[None], y[None]))
            torch.cuda.synchronize()
            outs.append({k: o[k].cpu().numpy() for k in ("rec", "flux", "iglast", "norders")})
        assert int(outs[0]["norders"][0]) >= 1 and np.any(outs[0]["rec"] != 0)
        _assert_same(outs[0], outs[1], ("rec", "flux", "iglast", "norders"), "solve")
    finally:
        _close([cx, twin])


# ------------------------------------------------------------------------------------------------ 7. the pass
ALTS = [-1, 3.0]
# a no-gas call, a CKD band, an aerosol layer, a surface-matrix call with aerosols (Roujean + Maignan, no -SOS.Trans), the
# no-gas call once more with the -SOS.Trans file (it builds its own operators: it does not defer) and a -SOS.AbsModeCKD 2 band
# (it does not defer its profiles)
NAMES = ["cfg1_lambert", "ckd_o2a_5bins", "layer_1_3km_lnd", "cfg5_roujean_maignan", "ckd_o2a_mode2", "nopolar_polar"]


@pytest.fixture(scope="module")
def calls(gpu_pkg, tmp_path_factory):
    import os
    rs = gpu_pkg.run_sos
    old = os.environ.get("SOS_ABS_ROOT")
    os.environ["SOS_ABS_ROOT"] = spectrum_cases.GOLD
    try:
        kws, _, _, _ = spectrum_cases.build(rs, tmp_path_factory.mktemp("ctx"), names=NAMES)
    finally:
        if old is None:
            del os.environ["SOS_ABS_ROOT"]
        else:
            os.environ["SOS_ABS_ROOT"] = old
    kws = [dict(kw, fictrans="NO_OUTPUT") for kw in kws]
    return kws + [dict(kws[0], fictrans="SOS_Transm.txt")]


def _count(monkeypatch, gpu_pkg):
    """Calls at the library; the pending contexts of every part as the context stage finds them; per _prepare, whether its
    context came back pending and the sosgpu_create calls it made (a -SOS.Trans call makes one per direction besides its own)."""
    L, rs = gpu_pkg.capi.lib(), gpu_pkg.run_sos
    n = dict(sosgpu_create=0, sosgpu_create_spectrum=0, parts=[], prepared=[])

    def counted(name):
        f = getattr(L, name)

        def g(*a):
            n[name] += 1
            return f(*a)
        return g

    for name in ("sosgpu_create", "sosgpu_create_spectrum"):
        monkeypatch.setattr(L, name, counted(name))
    real = rs._stage_contexts

    def stage(ch, part, *a, **k):
        n["parts"].append((len(part), sum(pl.ctx._pending is not None for pl in part)))
        return real(ch, part, *a, **k)

    monkeypatch.setattr(rs, "_stage_contexts", stage)
    real_prepare = rs._prepare

    def prepare(*a, **k):
        c0 = n["sosgpu_create"]
        pl = real_prepare(*a, **k)
        n["prepared"].append((pl.ctx._pending is not None, n["sosgpu_create"] - c0))
        return pl

    monkeypatch.setattr(rs, "_prepare", prepare)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,parts", [(256, 1), (256, 2), (3, 1), (3, 2)])
def test_pass_equals_the_per_call_contexts(gpu_pkg, calls, monkeypatch, chunk, parts):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "1")
    n = _count(monkeypatch, gpu_pkg)
    monkeypatch.delenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", raising=False)
    got = rs.sos_spectrum(calls, chunk=chunk, parts=parts)
    print("chunk %d parts %d:" % (chunk, parts), n)
    pending = sum(p for _, p in n["parts"])
    assert sum(m for m, _ in n["parts"]) == len(calls) and pending >= 4          # the four calls that defer everything, at least
    assert n["sosgpu_create_spectrum"] == sum(p > 0 for _, p in n["parts"]) >= 1
    # sosgpu_create: none for a call that defers, the call's own otherwise, and none outside _prepare
    assert len(n["prepared"]) == len(calls) and sum(p for p, _ in n["prepared"]) == pending
    assert all((made == 0) if p else (made >= 1) for p, made in n["prepared"]), n
    assert n["sosgpu_create"] == sum(made for _, made in n["prepared"]) and len(calls) - pending >= 2
    n.update(sosgpu_create=0, sosgpu_create_spectrum=0, parts=[], prepared=[])
    monkeypatch.setenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", "1")
    want = rs.sos_spectrum(calls, chunk=chunk, parts=parts)
    assert n["sosgpu_create_spectrum"] == 0 and not any(p for _, p in n["parts"])
    assert len(n["prepared"]) == len(calls) and all(not p and made >= 1 for p, made in n["prepared"]), n
    assert len(got) == len(want) == len(calls)
    for i, (a, b) in enumerate(zip(got, want)):
        spectrum_cases.assert_tuples_equal(a, b, i)


def _flat(x):
    """Every array of a nested result, in order."""
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [v for y in x for v in _flat(y)]
    return [np.asarray(x)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["levels", "irradiances", "transmissions"])
def test_other_passes_equal_the_per_call_contexts(gpu_pkg, calls, monkeypatch, mode):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "1")
    kws = [dict(kw, zout=-1.0) for kw in calls[:-1]]                 # (transmissions=True refuses the -SOS.Trans call)
    run = dict(levels=lambda: rs.sos_spectrum_levels(ALTS, kws, fluxes=True, split=True, absorption=True, parts=2),
               irradiances=lambda: rs.sos_spectrum_irradiances(ALTS, kws, parts=2),
               transmissions=lambda: rs.sos_spectrum(kws, transmissions=True, parts=2))[mode]
    n = _count(monkeypatch, gpu_pkg)
    monkeypatch.delenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", raising=False)
    got = _flat(run())
    assert n["sosgpu_create_spectrum"] == sum(p > 0 for _, p in n["parts"]) >= 1, n
    monkeypatch.setenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", "1")
    n.update(sosgpu_create_spectrum=0)
    want = _flat(run())
    assert n["sosgpu_create_spectrum"] == 0
    assert len(got) == len(want) >= len(kws)                           # (the irradiance pass: one array of rows per call)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (mode, i)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [False, True])
def test_refused_call_in_the_middle_is_named(gpu_pkg, calls, monkeypatch, switch):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "1")
    if switch:
        monkeypatch.setenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", "1")
    else:
        monkeypatch.delenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", raising=False)
    bad = dict(calls[1], tetas=95.0)
    with pytest.raises(rs.SosProcError) as alone:
        rs.sos_proc(**bad)
    chunks = []

    class Chunk(rs._Chunk):
        def __init__(self):
            chunks.append(self)

    monkeypatch.setattr(rs, "_Chunk", Chunk)
    with pytest.raises(rs.SosProcError) as inlist:
        rs.sos_spectrum(calls[:3] + [bad] + calls[3:5], parts=2)
    assert str(inlist.value) == str(alone.value) and inlist.value.ier == alone.value.ier
    assert len(chunks) == 1 and chunks[0].where == 3                  # the index the pass names (and the ranks agree on)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["the call fails", "the library refuses one spec"])
def test_failure_of_the_context_stage_is_named(gpu_pkg, calls, monkeypatch, how):
    """The except branch of run_sos._stage_contexts: a failure of solver.create_contexts becomes SosProcError and the pass names
    the first pending call of the part -- or, where the library refuses one spec of the list, the call that spec belongs to (found
    with the one-spec query).  Nothing is left pending-and-created: the contexts of the chunk are closed as after any failure."""
    rs, S = gpu_pkg.run_sos, gpu_pkg.solver
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.delenv("SOS_SPECTRUM_MIN_PART", raising=False)         # (the four calls are one part)
    monkeypatch.delenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", raising=False)
    chunks, seen = [], {}

    class Chunk(rs._Chunk):
        def __init__(self):
            chunks.append(self)

    monkeypatch.setattr(rs, "_Chunk", Chunk)
    real_stage, real_create = rs._stage_contexts, S.create_contexts

    def stage(ch, part, *a, **k):
        pending = [pl for pl in part if pl.ctx._pending is not None]
        if len(pending) >= 2 and not seen:
            seen.update(first=pending[0].index, second=pending[1].index)
            if how == "the library refuses one spec":
                pending[1].ctx._pending.wv.n0 = 0                      # (a spec _prepare could never hand over)
        return real_stage(ch, part, *a, **k)

    def create(ctxs):
        if how == "the call fails":
            raise RuntimeError("no contexts today")
        return real_create(ctxs)

    monkeypatch.setattr(rs, "_stage_contexts", stage)
    monkeypatch.setattr(S, "create_contexts", create)
    with pytest.raises(rs.SosProcError, match="SOS_PREPA_OS") as err:
        rs.sos_spectrum(calls[:4])
    assert seen and len(chunks) == 1
    assert chunks[0].where == (seen["first"] if how == "the call fails" else seen["second"]), (chunks[0].where, seen)
    assert ("no contexts today" in str(err.value)) == (how == "the call fails")
    monkeypatch.setattr(S, "create_contexts", real_create)
    monkeypatch.setattr(rs, "_stage_contexts", real_stage)
    assert len(rs.sos_spectrum(calls[:4])) == 4                        # the pass works again afterwards


@pytest.mark.gpu
def test_debug_switch_prints_the_context_stage(gpu_pkg, calls, monkeypatch, capsys):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_DEBUG", "1")
    monkeypatch.delenv("SOS_SPECTRUM_CONTEXTS_PER_CALL", raising=False)
    rs.sos_spectrum(calls[:3])
    assert "[sos_spectrum] contexts of wavelengths [0, 1, 2]" in capsys.readouterr().out
