"""The launch plan of the fused solver (csrc/solve_plan.h), as the library reports it (sosgpu_debug_solve_plan: no context, no
device, the environment switches read as a solve reads them).

CPU: the Python restatement of the bins-per-launch rule (test_spectrum_levels._scratch_split) against the library; the scratch
blocks of every plan of a grid disjoint, ordered and inside the allocation; one assertion per precedence rule of the
environment switches; the kernel variant in the plan (csrc/solve_variant.h) -- the row tiles of the streamed layout with and
without SOSGPU_STREAM_PERSIST, the shared-tile form -- against the table of test_variant_matrix.
GPU: a batch split into sub-launches by the scratch budget WITHOUT a context table (sosgpu_os_solve_levels), bit for bit the
unsplit solve."""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_output_levels as tol
import test_spectrum_levels as tsl
import test_variant_matrix as vm

VARS = ("SOSGPU_SCRATCH_GIB", "SOSGPU_STREAM_SPEC", "SOSGPU_STREAM_SPEC_MAXBINS", "SOSGPU_STREAM_SPEC_K",
        "SOSGPU_STREAM_PERSIST", "SOSGPU_STREAM_ORDERS_PER_LAUNCH", "SOSGPU_STREAM_QTAIL")


@pytest.fixture
def env(monkeypatch):
    """Sets the solver's switches to exactly the given ones (every other one unset)."""
    def set_(**kw):
        for v in VARS:
            monkeypatch.delenv(v, raising=False)
        for k, v in kw.items():
            assert "SOSGPU_" + k in VARS
            monkeypatch.setenv("SOSGPU_" + k, str(v))
    set_()
    return set_


def _plan(pkg, n, smax, nb, lp, nz=0, table=False, nt_max=None):
    p = pkg.capi.SolvePlan()
    pkg.capi.check(pkg.capi.lib().sosgpu_debug_solve_plan(n, smax, nb, lp, nz, int(table), lp - 1 if nt_max is None else nt_max,
                                                          C.byref(p)), "sosgpu_debug_solve_plan")
    return p


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_plan_argument_errors(pkg):
    L, p = pkg.capi.lib(), pkg.capi.SolvePlan()
    for args in ((43, 8, 0, 608, 0), (43, 8, 5, 1, 0), (43, 8, 5, 608, 17), (43, 8, 5, 608, -1), (43, -1, 5, 608, 0)):
        assert L.sosgpu_debug_solve_plan(*args, 0, 1, C.byref(p)) == -1, args                   # SOSGPU_E_ARG
    assert L.sosgpu_debug_solve_plan(43, 8, 5, 608, 0, 0, 1, None) == -1
    assert L.sosgpu_debug_solve_plan(86, 8, 5, 608, 0, 0, 1, C.byref(p)) == -3                  # SOSGPU_E_UNSUPPORTED
    assert L.sosgpu_debug_solve_plan(43, 8, 5, 1025, 0, 0, 1, C.byref(p)) == -3


# one (N, lp) per streamed shape class: the full-width layouts and the two narrow ones, at both ends of their N range and at
# both padded level counts of test_variant_matrix
STREAMED = [(n, lp) for lay, corners in vm.LAYOUTS.items() if lay.startswith("stream") for n, lps in corners for lp in lps]
RESTATED = [(43, 608, 340, 6, 1), (21, 608, 340, 6, 64)] + [(n, lp, 340, 6, 1) for n, lp in STREAMED]


def test_scratch_split_restatement_against_the_library(pkg, env):
    assert {vm.route(n, lp) for n, lp in STREAMED} == set(vm.FULL_WIDTH) | {"stream<4,2,5>", "stream<4,2,6>"}
    for n, lp, nb, nz, gib in RESTATED:
        env(SCRATCH_GIB=gib)
        with_slots, without = tsl._scratch_split(n, lp, nb, nz, gib)
        per_bin, lv = tsl._scratch_numbers(n, lp, nz)
        for table in (True, False):                    # (340 bins: no order-parallel form, the two plans agree)
            p, p0 = _plan(pkg, n, 8, nb, lp, nz, table), _plan(pkg, n, 8, nb, lp, 0, table)
            what = (n, lp, nb, nz, gib, table)
            assert p.big == 1 and p.form == p0.form == pkg.capi.FORM_STREAM, what
            assert (p.per_launch, p0.per_launch) == (with_slots, without), what
            assert p.per_bin == p0.per_bin == per_bin and p.lpb == vm._round_up(lp, 32), what
            assert p.slot_stride == lv and p0.slot_stride == 0 and p.threads * 8 * nz == lv, what


def _stream_numbers(p, lp, kht_n):
    """The streamed plan p against the restatement of test_spectrum_levels at a direction count kht_n of p's layout."""
    per_bin = tsl._scratch_numbers(kht_n, lp, 0)[0]
    khm, ns = 16 * p.kht, (16 * p.kht // 3 + 1) & ~1
    # k_sos_stream's LDS: a 32-level chunk of the field, the ground / flux / Gauss vectors, the attenuations, seven level vectors
    lds = 8 * (32 * (2 * khm + 2) + 3 * ns + 2 + 2 * ns + 16 + 2 * ns + 32 * ns + 7 * (32 + 8))
    return (p.per_bin, p.threads, p.lds_bytes, p.nw * p.rtw >= p.kht) == (per_bin, 64 * p.nw, lds, True)


def test_streamed_row_tiles_follow_the_table(pkg, env):
    """SOSGPU_STREAM_PERSIST unset or 0: KHT is the third number of the table's streamed layouts over their N ranges."""
    want = {n: int(lay[7:-1].split(",")[2]) for lay, (lo, hi) in vm.N_RANGE.items() if lay.startswith("stream")
            for n in range(lo, hi + 1)}
    assert sorted(set(want.values())) == [4, 5, 6, 8, 16] and sorted(want) == list(range(3, 86))
    for ov in (dict(), dict(STREAM_PERSIST=0)):
        env(**ov)
        for n, kht in want.items():
            for lp in (80, 608):
                for table, nz in itertools.product((False, True), (0, 2)):
                    p = _plan(pkg, n, 8, 340, lp, nz, table)
                    assert p.big == 1 and p.split == 0 and p.kht == kht, (ov, n, lp, table, nz, p.kht)
                    assert _stream_numbers(p, lp, n), (ov, n, lp, table, nz)


def test_persist_switch_widens_the_narrow_layouts_in_every_form(pkg, env):
    """SOSGPU_STREAM_PERSIST=1: the 8-tile layout for every N = 22 ... 32, with or without a table or output slots; the form
    is the persistent one only without either and with all orders in one launch."""
    capi = pkg.capi
    env(STREAM_PERSIST=1)
    for n in range(22, 33):
        for lp in (80, 608):
            for table, nz in itertools.product((False, True), (0, 2)):
                p = _plan(pkg, n, 8, 5, lp, nz, table)
                assert p.big == 1 and p.kht == 8 and (p.nw, p.rtw) == (4, 2), (n, lp, table, nz, p.kht)
                assert _stream_numbers(p, lp, 33), (n, lp, table, nz)                  # (N = 33: 8 tiles by the table)
                assert p.form == (capi.FORM_STREAM if table or nz else capi.FORM_PERSIST), (n, lp, table, nz, p.form)
            env(STREAM_PERSIST=1, STREAM_ORDERS_PER_LAUNCH=3)
            p = _plan(pkg, n, 8, 5, lp)
            assert p.kht == 8 and p.form == capi.FORM_STREAM and _stream_numbers(p, lp, 33), (n, lp)
            env(STREAM_PERSIST=1)
    assert tsl._scratch_numbers(33, 608, 0) != tsl._scratch_numbers(32, 608, 0)
    for n in (21, 33, 42, 43):                          # the other layouts are what they are without the switch
        assert _plan(pkg, n, 8, 5, 608).kht == {21: 4, 33: 8, 42: 8, 43: 16}[n]


def test_split_exactly_on_the_two_column_tile_route_of_n_22_to_32(pkg, env):
    for ov in (dict(), dict(STREAM_PERSIST=1)):
        env(**ov)
        for n in range(3, 86):
            for lp in vm.NTS:
                for table, nz in itertools.product((False, True), (0, 2)):
                    p = _plan(pkg, n, 8, 5, lp, nz, table)
                    assert p.split == (22 <= n <= 32 and lp == 32), (ov, n, lp, table, nz)
                    assert not (p.split and p.big) and (p.kht > 0) == (p.big == 1), (ov, n, lp, table, nz)
                    if p.split:
                        assert (p.nw, p.rtw, p.ct) == (4, 2, 2), (n, lp)


GRID = list(itertools.product((13, 21, 43, 85), (32, 64, 608), (1, 40, 41, 128, 129, 340), (0, 1, 6), (False, True)))
OVERRIDES = [dict(), dict(STREAM_SPEC=0), dict(STREAM_PERSIST=1), dict(STREAM_ORDERS_PER_LAUNCH=1),
             dict(STREAM_ORDERS_PER_LAUNCH=3), dict(STREAM_SPEC_K=1), dict(STREAM_SPEC_K=2), dict(SCRATCH_GIB=1)]


def _check_layout(capi, p, n, smax, nb, lp, nz, table, ov, what):
    cap = (int(ov.get("SCRATCH_GIB", 64)) << 30) // 8
    assert 1 <= p.per_launch <= nb, what
    assert p.off_slots % 8 == 0, what
    assert (p.form == capi.FORM_LDS) == (p.big == 0) and (p.form == capi.FORM_SPEC) == (p.spec_k > 0), what
    # regions | I3 block | queue ints | slot state: each starts at or behind the end of the one before, the last ends at `need`
    slots = p.slot_stride * p.regions
    assert (p.slot_stride > 0) == (nz > 0), what
    if p.big:
        assert p.per_bin > 0 and p.regions >= 1, what
        assert p.per_bin * p.regions <= p.off_i3, what
        assert p.off_i3 + p.i3_doubles <= p.off_queue, what
        assert 8 * p.queue_doubles >= 4 * (256 + p.per_launch), what          # 256 queue ints and a flag per bin of a launch
        if nz > 0:
            assert p.off_queue + p.queue_doubles <= p.off_slots and p.off_slots + slots == p.need, what
        else:
            assert p.off_queue + p.queue_doubles == p.need and p.off_slots == 0, what
        assert p.i3_doubles == (nb * (smax + 1) * p.threads if p.spec_k else 0), what
        assert p.regions == (nb * p.spec_k if p.spec_k else p.per_launch), what
    else:
        # the LDS-resident variant asks for scratch only for its output slots
        assert p.per_bin == p.i3_doubles == p.queue_doubles == p.off_slots == 0 and p.regions == nb, what
        assert p.need == slots and (p.need > 0) == (nz > 0), what
    if p.spec_k > 0:
        assert not table and p.needs_nt and nb * p.spec_k * p.per_bin <= cap, what
    if p.form == capi.FORM_PERSIST:
        assert not table and nz == 0 and p.opl == smax + 1, what
    if p.form in (capi.FORM_STREAM, capi.FORM_PERSIST):
        assert p.opl >= 1, what


def test_layout_invariants_over_the_grid(pkg, env):
    seen = set()
    for ov in OVERRIDES:
        env(**ov)
        for n, lp, nb, nz, table in GRID:
            for smax in (80, 0):
                p = _plan(pkg, n, smax, nb, lp, nz, table)
                assert p.big == vm.route(n, lp).startswith("stream"), (n, lp)
                for nt_max in ((lp - 1, 1) if p.needs_nt else (lp - 1,)):
                    p = _plan(pkg, n, smax, nb, lp, nz, table, nt_max)
                    _check_layout(pkg.capi, p, n, smax, nb, lp, nz, table, ov, (ov, n, smax, nb, lp, nz, table, nt_max))
                    seen.add(p.form)
    assert seen == {pkg.capi.FORM_LDS, pkg.capi.FORM_STREAM, pkg.capi.FORM_PERSIST, pkg.capi.FORM_SPEC}


def test_nt_is_asked_for_by_the_order_parallel_candidates_only(pkg, env):
    assert _plan(pkg, 43, 8, 128, 608).needs_nt == 1 and _plan(pkg, 43, 8, 129, 608).needs_nt == 0
    assert _plan(pkg, 43, 8, 5, 608, table=True).needs_nt == 0         # a context table
    assert _plan(pkg, 43, 0, 5, 608).needs_nt == 0                     # a single Fourier order
    assert _plan(pkg, 21, 8, 5, 32).needs_nt == 0                      # LDS-resident
    # ... and NT is not read otherwise
    assert bytes(_plan(pkg, 43, 8, 129, 608, nt_max=1)) == bytes(_plan(pkg, 43, 8, 129, 608, nt_max=607))


def test_order_parallel_regions_follow_the_batch_levels(pkg, env):
    capi = pkg.capi
    full = _plan(pkg, 43, 80, 5, 608, 6, table=True)
    p = _plan(pkg, 43, 80, 5, 608, 6, nt_max=95)
    assert p.form == capi.FORM_SPEC and p.spec_k == 48 and p.lpb == 96 and p.per_bin == tsl._scratch_numbers(43, 96, 0)[0]
    assert full.lpb == 608 and full.per_bin == tsl._scratch_numbers(43, 608, 0)[0]
    assert _plan(pkg, 43, 80, 41, 608, nt_max=95).spec_k == 24 and _plan(pkg, 43, 8, 41, 608, nt_max=95).spec_k == 9
    # the bins per launch are those of the unshrunk region, and the queue ints are budgeted in every form
    env(SCRATCH_GIB=1)
    full, p = _plan(pkg, 43, 80, 128, 608, 6, table=True), _plan(pkg, 43, 80, 128, 608, 6, nt_max=31)
    assert p.form == capi.FORM_SPEC and p.per_launch == full.per_launch == 128
    assert p.queue_doubles == full.queue_doubles == (256 + 128) // 2 + 1
    # over the budget the form is given up and the regions are the padded ones again
    env(SCRATCH_GIB=1, STREAM_SPEC_K=81)
    p = _plan(pkg, 43, 80, 128, 608, 6, nt_max=607)
    assert p.form == capi.FORM_STREAM and p.spec_k == 0 and p.needs_nt == 1
    assert (p.lpb, p.per_bin, p.per_launch, p.need) == (full.lpb, full.per_bin, full.per_launch, full.need)
    p = _plan(pkg, 43, 80, 128, 608, 6, nt_max=31)
    assert p.form == capi.FORM_STREAM and p.lpb == 608 and p.per_bin == full.per_bin
    # beyond 4 GiB of regions: fewer orders per round
    env()
    p = _plan(pkg, 43, 80, 128, 608, nt_max=607)
    assert p.form == capi.FORM_SPEC and p.spec_k == (4 << 27) // (128 * p.per_bin) and 8 < p.spec_k < 24


def test_override_precedence(pkg, env):
    capi = pkg.capi
    few = dict(n=43, smax=8, nb=5, lp=608)
    assert _plan(pkg, **few).form == capi.FORM_SPEC and _plan(pkg, **few).spec_k == 9 and _plan(pkg, **few).q_tail == -1
    # SOSGPU_STREAM_SPEC=0 turns the order-parallel form off; SOSGPU_STREAM_SPEC_MAXBINS moves its limit (and wins over SPEC=0)
    env(STREAM_SPEC=0)
    p = _plan(pkg, **few)
    assert p.form == capi.FORM_STREAM and p.opl == 9 and p.needs_nt == 0
    env(STREAM_SPEC=1)
    assert _plan(pkg, **few).form == capi.FORM_SPEC
    env(STREAM_SPEC_MAXBINS=4)
    assert _plan(pkg, **few).form == capi.FORM_STREAM and _plan(pkg, **dict(few, nb=4)).form == capi.FORM_SPEC
    env(STREAM_SPEC_MAXBINS=340)
    assert _plan(pkg, **dict(few, nb=340)).form == capi.FORM_SPEC
    env(STREAM_SPEC=0, STREAM_SPEC_MAXBINS=8)
    assert _plan(pkg, **few).form == capi.FORM_SPEC
    # an explicit SOSGPU_STREAM_PERSIST turns the order-parallel form off ...
    env(STREAM_PERSIST=1)
    p = _plan(pkg, **few)
    assert p.form == capi.FORM_PERSIST and p.spec_k == 0 and p.needs_nt == 0 and p.opl == 9
    env(STREAM_PERSIST=1, STREAM_SPEC_MAXBINS=8)
    assert _plan(pkg, **few).form == capi.FORM_PERSIST
    env(STREAM_PERSIST=0)
    assert _plan(pkg, **few).form == capi.FORM_SPEC
    # ... and so does an explicit SOSGPU_STREAM_ORDERS_PER_LAUNCH
    env(STREAM_ORDERS_PER_LAUNCH=3)
    p = _plan(pkg, **few)
    assert p.form == capi.FORM_STREAM and p.opl == 3 and p.needs_nt == 0
    env(STREAM_ORDERS_PER_LAUNCH=0)
    assert _plan(pkg, **few).form == capi.FORM_SPEC
    # SOSGPU_STREAM_SPEC_K clamps to [1, smax + 1]
    for k, want in ((0, 1), (-3, 1), (1, 1), (2, 2), (9, 9), (10, 9), (1000, 9)):
        env(STREAM_SPEC_K=k)
        assert _plan(pkg, **few).spec_k == want, k
    # the persistent form: only without a table, with all orders in one launch, and without output slots
    env(STREAM_PERSIST=1)
    assert _plan(pkg, table=True, **few).form == capi.FORM_STREAM
    assert _plan(pkg, nz=1, **few).form == capi.FORM_STREAM
    env(STREAM_PERSIST=1, STREAM_ORDERS_PER_LAUNCH=3)
    p = _plan(pkg, **few)
    assert p.form == capi.FORM_STREAM and p.opl == 3
    env(STREAM_PERSIST=1, STREAM_ORDERS_PER_LAUNCH=9)
    assert _plan(pkg, **few).form == capi.FORM_PERSIST
    # its queue sits behind the work regions of one launch
    p = _plan(pkg, **few)
    assert p.off_queue == p.off_i3 == p.per_bin * p.per_launch and p.regions == p.per_launch == 5
    # SOSGPU_STREAM_QTAIL is one number of the whole solve
    env(STREAM_PERSIST=1, STREAM_QTAIL=16)
    assert _plan(pkg, **few).q_tail == 16
    # SOSGPU_SCRATCH_GIB: a positive integer, anything else is the default of 64
    big = dict(n=43, smax=8, nb=100000, lp=608)
    per_bin = tsl._scratch_numbers(43, 608, 0)[0]
    for val, gib in ((None, 64), (1, 1), (2, 2), (0, 64), (-4, 64), ("x", 64)):
        env(**({} if val is None else dict(SCRATCH_GIB=val)))
        assert _plan(pkg, **big).per_launch == (gib << 27) // per_bin, val


# ---- GPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_split_into_sub_launches_without_a_table(gpu_pkg, env):
    """sosgpu_os_solve_levels of ONE context under a 1 GiB scratch budget: the plan reports 329 + 11 bins for the 340 bins of
    the 16-tile streamed layout with six output slots, and every output is bit for bit that of the same call under the default
    budget (one launch); the slot outputs also equal, row by row, a two-bin solve of the batch's two distinct bins.
    The plain solve (nz = 0) of the same bins does NOT split under 1 GiB -- 340 regions without slot state fit, and the
    variable is read as an integer -- so it runs as the unsplit companion: same layout as the default budget, same bits."""
    lay, n, lp = "stream<8,2,16>", 43, 608
    b = vm.make_batch(lay, False, False, n, lp)
    nb = 340
    rows = [1 if i % 60 == 7 else 0 for i in range(nb)]        # mostly NT = 1, a few NT = 95 bins
    alts = tol._slot_altitudes(b)
    cx = vm._context(gpu_pkg, b)
    try:
        bins = vm._upload(cx, b, rows)
        lv = cx.output_levels(bins, alts)
        assert _plan(gpu_pkg, n, cx.smax, nb, lp, len(alts)).per_launch == nb
        ref, ref_lv = vm._fetch(cx.solve(bins)), vm._fetch(cx.solve_levels(bins, lv))
        two = vm._upload(cx, b, [0, 1])
        ref_two = vm._fetch(cx.solve_levels(two, cx.output_levels(two, alts)))
        assert (ref["norders"] > 0).all() and (ref_lv["norders"] > 0).all() and (ref_two["norders"] > 0).all()
        env(SCRATCH_GIB=1)
        with_slots, without = tsl._scratch_split(n, lp, nb, len(alts), 1)
        p = _plan(gpu_pkg, n, cx.smax, nb, lp, len(alts))
        assert p.per_launch == with_slots < nb and p.form == gpu_pkg.capi.FORM_STREAM
        assert _plan(gpu_pkg, n, cx.smax, nb, lp, 0).per_launch == without == nb
        got, got_lv = vm._fetch(cx.solve(bins)), vm._fetch(cx.solve_levels(bins, lv))
    finally:
        cx.close()
    for key in ("norders", "iglast", "flux", "rec"):
        assert np.array_equal(got[key], ref[key]), key
        assert np.array_equal(got_lv[key], ref_lv[key]), key
    for key in ("norders", "iglast", "flux"):
        assert np.array_equal(got_lv[key], ref_two[key][rows]), key
    assert np.array_equal(got_lv["rec"], ref_two["rec"][:, rows])
