"""The work-area contract of the table-form entry points (include/sosgpu.h, "Work areas"): every one of them takes
`d_work, work_bytes`, its _work_bytes query knows the size, a short area is refused on the host before anything is queued, and
nothing beyond the queried size is touched.

The GPU tests drive each entry point through the smallest call its own test module makes (two or three contexts, jobs or
wavelengths) and reach the work-area arguments by wrapping the library function: the wrapper puts an area of its own in the
place of the caller's -- ample, exact with a guard behind it, or one byte short."""
import contextlib
import ctypes as C

import numpy as np
import pytest

E_ARG, E_UNSUPPORTED = -1, -3
GUARD = 256
PATTERN, SENTINEL = 0xA5, 0x5A

# What the parent commit stated, entry by entry.  Its library answered 256 / 80 / 120 for sosgpu_ctx_table_entry_bytes(),
# sosgpu_ckd_table_entry_bytes() and sosgpu_profile_table_entry_bytes() (the device-side entries: the host structures of 72 and
# 104 bytes plus slot0, and plus t_first, t_layer and nt_ng), and njobs * 144 / njobs * 40 for the two job tables
# (csrc/kernels.h: TrphiJobDev = 8 int32 + 4 pointers + 4 doubles + LandTerms of 4 int32 and 4 doubles; FluxJobDev = 2 int32 +
# 4 pointers).
CTX_ENTRY, CKD_ENTRY, PROFILE_ENTRY, TRPHI_ENTRY, FLUX_ENTRY = 256, 80, 120, 144, 40
NOGAS_LEVELS = 608
COUNTS = (0, 1, 2, 7, 64)


def test_queries_equal_the_sizes_the_parent_stated(pkg):
    """solver.build_operators: n * (sosgpu_ctx_table_entry_bytes() + 8); solver._ckd_launch: nwl * sosgpu_ckd_table_entry_bytes()
    + 8 * nslots; solver.make_profiles_spectrum: nwl * 4 * ng doubles of no-gas blocks, then -(-nwl * entry // 8) doubles of
    table; api_outputs.hip: njobs * sizeof(TrphiJobDev), njobs * sizeof(FluxJobDev).  A zero (or negative) count gives 0."""
    L = pkg.capi.lib()
    assert L.sosgpu_ctx_table_entry_bytes() == CTX_ENTRY
    for n in COUNTS:
        assert L.sosgpu_trphi_spectrum_work_bytes(n) == n * TRPHI_ENTRY, n
        assert L.sosgpu_level_flux_spectrum_work_bytes(n) == n * FLUX_ENTRY, n
        assert L.sosgpu_noyaux_spectrum_work_bytes(n) == n * (CTX_ENTRY + 8), n
        assert L.sosgpu_profile_spectrum_work_bytes(n) == 8 * (n * 4 * NOGAS_LEVELS + -(-n * PROFILE_ENTRY // 8)), n
        for nslots in (0, 8, 40, 80, 40 * n, 65535 * 8):
            want = n * CKD_ENTRY + 8 * nslots if n > 0 and nslots > 0 else 0
            assert L.sosgpu_ckd_layer_tables_work_bytes(n, nslots) == want, (n, nslots)
    for f in (L.sosgpu_trphi_spectrum_work_bytes, L.sosgpu_level_flux_spectrum_work_bytes, L.sosgpu_noyaux_spectrum_work_bytes,
              L.sosgpu_profile_spectrum_work_bytes):
        assert f(-1) == 0
    assert L.sosgpu_ckd_layer_tables_work_bytes(-1, 40) == 0 and L.sosgpu_ckd_layer_tables_work_bytes(2, -1) == 0


def test_python_takes_its_records_from_the_ctypes_structures(pkg):
    S, cap = pkg.solver, pkg.capi
    assert S.PROFILE_WL_DTYPE == np.dtype(cap.ProfileWl) and S.PROFILE_WL_DTYPE.itemsize == 104
    assert S.CKD_WL_DTYPE == np.dtype(cap.CkdWl) and S.CKD_WL_DTYPE.itemsize == 72


# ---------------------------------------------------------------------------------------------------------------- GPU
def _nbytes(x):
    return x.nbytes if isinstance(x, np.ndarray) else x.numel() * x.element_size()


def _bits(x):
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tobytes()
    return x.detach().cpu().contiguous().numpy().tobytes()


class _Area:
    """Wrapper round L.<name>: d_work is argument `iw`, work_bytes the next.  mode "ample": need + 4096 bytes, all of them
    offered; "exact": need bytes offered, GUARD bytes of PATTERN behind them; "short": need - 1 bytes offered, and every output
    pointer of `outs` (argument index, an array of the output's size) replaced by a block of SENTINEL bytes."""

    def __init__(self, L, name, iw, mode, outs=()):
        self.L, self.name, self.iw, self.mode, self.outs = L, name, iw, mode, outs
        self.calls = []

    def _stage(self):
        total, idle = C.c_int(-1), C.c_int(-1)
        assert self.L.sosgpu_debug_stage_blocks(0, C.byref(total), C.byref(idle)) == 0
        return total.value, idle.value

    def __call__(self, *a):
        import torch
        a = list(a)
        need = int(a[self.iw + 1])
        assert need > 0, "the driver must reach the library with a real size"
        buf = torch.full((need + (4096 if self.mode == "ample" else GUARD),), PATTERN, dtype=torch.uint8, device="cuda")
        a[self.iw] = C.c_void_p(buf.data_ptr())
        a[self.iw + 1] = {"ample": need + 4096, "exact": need, "short": need - 1}[self.mode]
        call = dict(need=need, buf=buf, sentinels=[])
        if self.mode == "short":
            for idx, like in self.outs:
                s = torch.full((_nbytes(like),), SENTINEL, dtype=torch.uint8, device="cuda")
                call["sentinels"].append(s)
                a[idx] = C.c_void_p(s.data_ptr())
            torch.cuda.synchronize()
            call["before"] = self._stage()
        call["rc"] = self.real(*a)
        if self.mode == "short":
            call["after"] = self._stage()
        self.calls.append(call)
        return call["rc"]

    def __enter__(self):
        self.real = getattr(self.L, self.name)
        setattr(self.L, self.name, self)
        return self

    def __exit__(self, *exc):
        setattr(self.L, self.name, self.real)


def _ctx(pkg, n=4, os_nb=8, **kw):
    S = pkg.synth
    mu, w, n0 = S.gauss_angles(n, 35.0)
    al, be, ga, ze = S.hg_phase(os_nb, 0.6)
    return pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=os_nb, **kw)


def _drive_noyaux(pkg):
    import test_noyaux_spectrum as TN
    ctxs = [TN._unbuilt(pkg, "n5"), TN._unbuilt(pkg, "gnd_n5")]
    try:
        pkg.solver.build_operators(ctxs)
        out = []
        for cx in ctxs:
            t = cx.debug_tables()
            out += [np.asarray(t[k]) for k in sorted(t) if isinstance(t[k], np.ndarray)]
        return out
    finally:
        TN._close(ctxs)


def _drive_trphi(pkg):
    import torch
    ctxs = [_ctx(pkg, 2, build=False), _ctx(pkg, 4, build=False)]
    try:
        rng = np.random.default_rng(3)
        recs = [torch.from_numpy(rng.standard_normal((2, 3, cx.w))).cuda() for cx in ctxs]
        phis = np.array([0.3, 0.3 + np.pi])
        items = [(ctxs[0], recs[0], 1, 0.4, 0.0, phis, 0, 0.0, None), (ctxs[1], recs[1], 2, 0.4, 0.1, phis, 0, 0.0, None),
                 (ctxs[1], recs[1], 1, 0.4, 0.0, np.array([-0.7]), 0, 0.0, None)]
        flat, _ = pkg.solver.trphi_many(items)
        torch.cuda.synchronize()
        return [flat]
    finally:
        for cx in ctxs:
            cx.close()


def _drive_flux(pkg):
    import torch
    ctxs = [_ctx(pkg, 2, build=False), _ctx(pkg, 8, build=False)]
    try:
        rng = np.random.default_rng(5)
        items = [(cx, torch.from_numpy(rng.standard_normal((2, 3, cx.w))).cuda()) for cx in (ctxs[0], ctxs[1], ctxs[0])]
        out = pkg.solver.level_flux_many(items)
        torch.cuda.synchronize()
        return [out]
    finally:
        for cx in ctxs:
            cx.close()


def _drive_channels(pkg):
    import torch
    rng = np.random.default_rng(9)
    njobs, K, nphi, W = 3, 2, 2, 5
    flat = torch.from_numpy(rng.standard_normal(njobs * K * nphi * 7 * W)).cuda()
    first, job = np.array([0, 3, 3, 5], dtype=np.int32), np.array([2, 0, 1, 1, 2], dtype=np.int32)
    acc = torch.zeros((3, K, nphi, 3, W), dtype=torch.float64, device="cuda")
    pkg.solver.channel_accumulate(flat, njobs, K, nphi, W, first, job, rng.uniform(0.1, 2.0, 5), acc)
    torch.cuda.synchronize()
    return [acc]


def _bins_of_two(pkg):
    import test_trans_many as TT
    ctxs = [_ctx(pkg, 4, os_nb=8), _ctx(pkg, 4, os_nb=4)]
    bins = ctxs[0].upload_bins(*TT._profiles(3, 10, 8))
    return ctxs, bins, np.array([0, 1, 0], dtype=np.int32)


def _drive_trans(pkg):
    import torch
    ctxs, bins, cob = _bins_of_two(pkg)
    try:
        _, tdifmug = pkg.solver.diffuse_transmissions_many(ctxs, bins, cob)
        torch.cuda.synchronize()
        return [tdifmug]
    finally:
        for cx in ctxs:
            cx.close()


def _drive_albedo(pkg):
    import torch
    ctxs, bins, cob = _bins_of_two(pkg)
    try:
        salb, plane = pkg.solver.spherical_albedo_many(ctxs, bins, cob)
        torch.cuda.synchronize()
        return [plane, salb]
    finally:
        for cx in ctxs:
            cx.close()


def _drive_surface(pkg):
    import torch
    from test_surface_batch import ORDERS, land, sea
    from test_surface_matrix import TRIPLES, angles
    mu, w, _ = angles(5, 35.0)
    jobs = [sea(2, 1.33), land(3, TRIPLES[1]), land(7, TRIPLES[1], coef_c=4.0)]
    blocks, status = pkg.surface.surface_matrices_many(jobs, mu, w, *ORDERS)
    torch.cuda.synchronize()
    return [status] + list(blocks)


def _drive_mie(pkg):
    import test_mie_batch as TM
    jobs = [((1.53, -0.008), TM.LISTS["one"]), ((1.381, 0.0), TM.LISTS["lds_limit"])]         # (two items past alpha = 850: scratch)
    rc, recs, gs, spare, spare_g, status, _ = TM.run_batch(pkg, TM.NBMU, jobs)
    if rc:
        raise pkg.capi.SosgpuError(rc, "sosgpu_mie_batch")
    return [status] + list(recs) + list(gs) + [spare, spare_g]


def _drive_ckd(pkg):
    import ckd_cells
    from test_ckd_device import _rand_tables
    rng = np.random.default_rng(2221)
    T, P, Cc = ckd_cells.axes(2, 2, 2)
    cells = []
    for nlay in (1, 1):
        prs, tmp, conc = ckd_cells.edge_states(T, P, Cc, nlay)
        cells.append(ckd_cells.make_cell(T, P, Cc, 1, _rand_tables(rng, T, P, Cc, 1, [(0, 0), (6, 0)]), prs, tmp, conc))
    out, status = ckd_cells.run(pkg, cells)
    return [out, status]


def _drive_profile(pkg, true_depth=False):
    import torch
    from test_profile_spectrum import _requests
    part = {}
    pkg.solver.make_profiles_spectrum(_requests()[:3], part=part, true_depth=true_depth)
    torch.cuda.synchronize()
    b = part["bins"]
    return [b["prof"], b["nt"], b["iborm"], b["zprof"], b["scal"]] + ([b["hvrai"]] if true_depth else [])


# name -> (index of d_work, driver, code of a short area, outputs that are arguments: (argument index, position in the driver's
# result)).  Outputs that live in job structures (surface blocks, Mie records) or in the contexts (operator tables) cannot be
# swapped for sentinel blocks: the Mie driver presets them itself (NaN, -77), the others are covered by the staging totals, the
# return code and the untouched status / output arguments.
ENTRY_POINTS = {
    "sosgpu_noyaux_spectrum": (3, _drive_noyaux, E_ARG, []),
    "sosgpu_trphi_spectrum": (5, _drive_trphi, E_ARG, [(4, 0)]),
    "sosgpu_level_flux_spectrum": (3, _drive_flux, E_ARG, [(2, 0)]),
    "sosgpu_channel_accumulate": (11, _drive_channels, E_ARG, [(10, 0)]),
    "sosgpu_trans_spectrum": (8, _drive_trans, E_ARG, [(7, 0)]),
    "sosgpu_albedo_spectrum": (10, _drive_albedo, E_ARG, [(8, 0), (9, 1)]),
    "sosgpu_surface_batch": (10, _drive_surface, E_ARG, [(9, 0)]),
    "sosgpu_mie_batch": (5, _drive_mie, E_UNSUPPORTED, [(7, 0)]),
    "sosgpu_ckd_layer_tables": (8, _drive_ckd, E_ARG, [(10, 0), (12, 1)]),
    "sosgpu_profile_spectrum": (10, _drive_profile, E_ARG, [(13, 0), (14, 1), (15, 2), (16, 3), (19, 4)]),
    "sosgpu_profile_spectrum_true": (10, lambda pkg: _drive_profile(pkg, True), E_ARG,
                                     [(13, 0), (14, 1), (15, 2), (16, 3), (19, 4), (21, 5)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_short_area_is_refused_and_nothing_beyond_the_area_is_touched(gpu_pkg, name):
    import torch
    iw, drive, code, outs = ENTRY_POINTS[name]
    L = gpu_pkg.capi.lib()
    with _Area(L, name, iw, "ample") as ample:
        ref = drive(gpu_pkg)
    assert len(ample.calls) == 1 and ample.calls[0]["rc"] == 0
    ref_bits = _bits(ref)
    # --- one byte short: the entry point's code, no staging block taken, no output touched
    with _Area(L, name, iw, "short", [(idx, ref[pos]) for idx, pos in outs]) as short:
        with contextlib.suppress(Exception):            # (the Python layer raises on the code; the wrapper has kept it)
            drive(gpu_pkg)
    torch.cuda.synchronize()
    assert len(short.calls) == 1
    call = short.calls[0]
    assert call["need"] == ample.calls[0]["need"]
    assert call["rc"] == code, call["rc"]
    assert call["after"][0] == call["before"][0] and call["after"][1] >= call["before"][1], (call["before"], call["after"])
    for s in call["sentinels"]:
        assert bool((s == SENTINEL).all())
    assert bool((call["buf"] == PATTERN).all())         # the area itself: nothing was copied there either
    # --- exactly the queried size: the guard behind it intact, the outputs those of the ample area, bit for bit
    with _Area(L, name, iw, "exact") as exact:
        got = drive(gpu_pkg)
    torch.cuda.synchronize()
    assert len(exact.calls) == 1 and exact.calls[0]["rc"] == 0
    buf, need = exact.calls[0]["buf"], exact.calls[0]["need"]
    assert buf.numel() == need + GUARD and bool((buf[need:] == PATTERN).all())
    assert _bits(got) == ref_bits
