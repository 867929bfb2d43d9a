"""Several output altitudes from one solve (sosgpu_os_solve_levels, sosgpu_output_levels, run_sos.sos_proc_levels).

The output altitude (-SOS.OutputAlt, ZOUT) only chooses which two levels of the field are captured and interpolated; the
solve itself does not depend on it.  One solve with K output slots must therefore give, for slot k, exactly what a
single-altitude solve gives: the records bit for bit, and the same order counts and fluxes.
CPU: the host output-level rule of the aerosol-layer profile, and the argument checks of sos_proc_levels.
GPU: every layout x SURF cell of test_variant_matrix in both launch forms against single-altitude solves; the zout cases of
cases.py against the oracle; sosgpu_output_levels against sosgpu_profile(zout); sos_proc_levels against sos_proc end to end."""
import json
import os

import numpy as np
import pytest

import cases
import test_variant_matrix as vm
from dist_launch import rank_env, run_ranks
from spectrum_cases import assert_tuples_equal

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _user_kwargs(rs, user):
    return rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False)


def _literal_rule(zprof, zout):
    """solver.upload_bins's rule for one altitude (SOS_OS.F:1514-1520), restated."""
    nb = zprof.shape[0]
    jout = np.zeros(nb, dtype=np.int32)
    zz = np.zeros(nb)
    for b in range(nb):
        j = 1
        while zout < zprof[b, j]:
            j += 1
        jout[b] = j
        zz[b] = (zout - zprof[b, j - 1]) / (zprof[b, j] - zprof[b, j - 1])
    return jout, zz


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_host_output_levels_match_the_single_altitude_rule(pkg):
    rs = pkg.run_sos
    rng = np.random.default_rng(7)
    profs = []
    for (ta, zmin, zmax) in ((0.3, 1.0, 3.0), (0.1, 0.0, 2.0), (0.8, 2.5, 6.0)):
        _, _, _, z = rs.profile_layer(0.0973, 8.0, ta, zmin, zmax)
        profs.append(z)
    L = max(len(z) for z in profs)
    zprof = np.zeros((len(profs), L))
    for b, z in enumerate(profs):
        zprof[b, :len(z)] = z
    levels = [float(profs[0][j]) for j in (1, 2, len(profs[0]) // 2, len(profs[0]) - 2)]
    alts = [-1.0, 0.0, 120.0] + levels + list(rng.uniform(0.0, 120.0, 6)) + [levels[0]]
    jout, zz = pkg.solver.output_levels_host(zprof, alts)
    assert jout.shape == zz.shape == (len(alts), len(profs)) and jout.dtype == np.int32
    for k, z in enumerate(alts):
        if z == -1.0:
            assert not jout[k].any() and not zz[k].any()
            continue
        j1, z1 = _literal_rule(zprof, z)
        assert np.array_equal(jout[k], j1) and np.array_equal(zz[k], z1), (k, z)
    # an altitude on a level j: the rule stops at j (ZOUT >= ZPROF(J)), so the weight is exactly 1 on that level
    assert (zz[3:3 + len(levels), 0] == 1.0).all() and (zz[2] == 0.0).all() and (jout[2] == 1).all()


def test_sos_proc_levels_argument_errors_before_any_device_work(pkg):
    rs = pkg.run_sos
    base = {"-SOS_Main.Wa": 0.55, "-ANG.Thetas": 30.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.0, "-SURF.Alb": 0.1,
            "-AP.HR": 8.0, "-SOS.View": 1, "-SOS.View.Phi": 0.0}
    kw = _user_kwargs(rs, base)
    for bad in (-0.5, 120.5, -2.0):
        with pytest.raises(rs.SosProcError) as e:
            rs.sos_proc_levels([1.0, bad], **kw)
        assert e.value.code == 2611
    with pytest.raises(ValueError):
        rs.sos_proc_levels([], **kw)
    with pytest.raises(ValueError):
        rs.sos_proc_levels([1.0] * 17, **kw)
    with pytest.raises(ValueError):
        rs.sos_proc_levels([1.0], **_user_kwargs(rs, dict(base, **{"-SOS.OutputAlt": 3.0})))
    with pytest.raises(ValueError):
        rs.sos_proc_levels([1.0], **_user_kwargs(rs, dict(base, **{"-SOS_Main.ResRoot": "/nonexistent/results"})))
    assert pkg.capi.MAX_OUTPUT_LEVELS == 16


# ---- GPU: kernels -----------------------------------------------------------------------------------------------------------

# one batch per layout x SURF: the layout's largest N at its largest padded level count
CELLS = [(lay, surf, corners[-1][0], corners[-1][1][-1]) for lay, corners in vm.LAYOUTS.items() for surf in (False, True)]


def _slot_altitudes(b):
    """-1, an altitude on a level of the last bin (weight exactly 1 there), a mid-layer altitude, 0 km, 120 km, and a duplicate."""
    z0 = b["bins"][-1][3]
    nt0 = len(z0) - 1
    on = float(z0[max(1, nt0 // 2)])
    mid = 0.5 * float(z0[0] + z0[1]) if nt0 >= 1 else 1.0
    return [-1.0, on, mid, 0.0, 120.0, on]


def _batch(lay, surf, n, lp):
    return vm.make_batch(lay, True, surf, n, lp)


def _check_cell(pkg, b, rows, what):
    import torch
    cx = vm._context(pkg, b)
    try:
        bins = vm._upload(cx, b, rows)
        alts = _slot_altitudes(b)
        lv = cx.output_levels(bins, alts)
        got = vm._fetch(cx.solve_levels(bins, lv))
        jout, zz = lv["jout"].cpu().numpy(), lv["zz"].cpu().numpy()
        assert zz[1, -1] == 1.0 and jout[1, -1] > 0                  # the last bin: the altitude sits on one of its levels
        for k, z in enumerate(alts):
            one = dict(bins, jout=None, zz=None) if z == -1.0 else \
                dict(bins, jout=torch.as_tensor(jout[k], device=cx.device), zz=torch.as_tensor(zz[k], device=cx.device))
            ref = vm._fetch(cx.solve(one))
            for key in ("norders", "iglast", "flux"):
                assert np.array_equal(got[key], ref[key]), (what, z, key)
            assert (ref["norders"] > 0).all(), (what, z)
            assert np.array_equal(got["rec"][k], ref["rec"]), (what, k, z)
    finally:
        cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "%s-%s-N%d-lp%d" % (c[0], "SURF" if c[1] else "noSURF", c[2], c[3]))
def test_levels_bitwise_vs_single_altitude_solves(gpu_pkg, monkeypatch, cell):
    lay, surf, n, lp = cell
    b = _batch(lay, surf, n, lp)
    nb = len(b["bins"])
    what = "%s surf=%s N=%d lp=%d" % cell
    _check_cell(gpu_pkg, b, range(nb), what + " full batch")
    if lay.startswith("stream"):
        _check_cell(gpu_pkg, b, [0, nb - 1], what + " two bins (order-parallel)")
        monkeypatch.setenv("SOSGPU_STREAM_SPEC", "0")
        _check_cell(gpu_pkg, b, range(nb), what + " one workgroup per bin")
        monkeypatch.delenv("SOSGPU_STREAM_SPEC")


@pytest.mark.gpu
def test_levels_flag_a_bin_whose_level_is_out_of_range(gpu_pkg):
    import torch
    b = _batch("os<4,1,2>", False, 21, 32)
    cx = vm._context(gpu_pkg, b)
    try:
        bins = vm._upload(cx, b)
        nb = bins["nb"]
        jout = torch.zeros((2, nb), dtype=torch.int32, device=cx.device)
        jout[1, 1] = int(b["nt"][1]) + 1
        lv = dict(nz=2, jout=jout, zz=torch.zeros((2, nb), dtype=torch.float64, device=cx.device))
        got = vm._fetch(cx.solve_levels(bins, lv))
        assert got["norders"][1] == -1 and (np.delete(got["norders"], 1) > 0).all()
    finally:
        cx.close()


ZOUT_CASES = [c for c in cases.ALL_CASES if "zout" in c]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZOUT_CASES)
def test_zout_cases_vs_oracle(gpu_pkg, oracle, name):
    """Each zout case of cases.py solved in one call with slots (-1, its zout, its zout again), slot 1 against the oracle."""
    case = cases.make_case(name)
    z = float(case["kw"]["zout"])
    ref = cases.run_cpu(oracle, case, 0)
    got = cases.run_gpu(gpu_pkg, case)[0]
    assert len(got["records"]) == len(ref["records"])
    # the same case through the slots: context and bins as cases.run_gpu builds them, then one solve with three slots
    kw = dict(case["kw"])
    kw.pop("zout")
    al, be, ga, ze = case["coefs"]
    cx = gpu_pkg.SosContext(case["rmu"], case["ga"], case["n0"], al, be, ga, ze, iborm_max=case["iborm"], **kw)
    try:
        H, X, Y, Z = (np.array([b[i] for b in case["bins"]]) for i in range(4))
        bins = cx.upload_bins(H, X, Y, iborm=np.full(len(H), case["iborm"], dtype=np.int32), zprof=Z)
        lv = cx.output_levels(bins, [-1.0, z, z])
        out = vm._fetch(cx.solve_levels(bins, lv))
        f = int(out["norders"][0])
        assert f == len(ref["records"])
        for k in (1, 2):
            cases.compare_records(out["rec"][k, 0, :f], ref["records"], 1e-9, "%s slot %d" % (name, k))
            assert np.array_equal(out["rec"][k, 0, :f], got["records"]), name
    finally:
        cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gas", [False, True])
def test_output_levels_kernel_vs_profile_zout(gpu_pkg, gas):
    """sosgpu_output_levels == sosgpu_profile(zout) bit for bit in jout, zz and TAUOUT."""
    import torch
    rs = gpu_pkg.run_sos
    cx = vm._context(gpu_pkg, _batch("os<4,1,2>", False, 21, 32))
    try:
        nb, tr, hr, ta, ha = 6, 0.0973, 8.0, 0.3, 2.0
        altabs = tabs = None
        if gas:
            altabs = np.linspace(100.0, 0.0, 50)
            rng = np.random.default_rng(3)
            tabs = np.cumsum(rng.uniform(0.0, 0.05, (nb, 50)) * np.linspace(0.0, 1.0, 50) ** 2, axis=1)
        base = cx.make_profiles(nb, tr, hr, ta, ha, altabs, tabs, a_tronc=0.1, piz=0.9, piztr=0.85)
        zp = base["zprof"].cpu().numpy()
        alts = [-1.0, 0.0, 120.0, float(zp[0, 3]), 0.5 * float(zp[0, 2] + zp[0, 3]), 2.7, 17.3, 2.7]
        lv = cx.output_levels(base, alts)
        jout, zz, tauout = (lv[k].cpu().numpy() for k in ("jout", "zz", "tauout"))
        for k, z in enumerate(alts):
            one = cx.make_profiles(nb, tr, hr, ta, ha, altabs, tabs, a_tronc=0.1, piz=0.9, piztr=0.85, zout=z)
            torch.cuda.synchronize()
            assert np.array_equal(one["prof"].cpu().numpy(), base["prof"].cpu().numpy())
            if z == -1.0:
                assert not jout[k].any() and not zz[k].any()
            else:
                assert np.array_equal(jout[k], one["jout"].cpu().numpy()), (gas, z)
                assert np.array_equal(zz[k], one["zz"].cpu().numpy()), (gas, z)
            assert np.array_equal(tauout[k], one["scal"][:, 3].cpu().numpy()), (gas, z)
    finally:
        cx.close()


# ---- GPU: end to end --------------------------------------------------------------------------------------------------------

PROC_CASES = ["cfg1_lambert", "ckd_h2o_o2_25bins_flatsea", "glitter_polar", "land_breon", "ckd_o2a_mode2",
              "layer_1_3km_lnd", "cfg5_ckd_maignan_25bins", "flatsea_zout"]


def _proc_inputs(rs, name):
    g = np.load(os.path.join(GOLD, "sos_proc_%s.npz" % name))
    user = json.loads(str(g["user_json"]))
    zout = float(user.pop("-SOS.OutputAlt", -1.0))
    user.update({"-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT", "-SOS_Main.ResRoot": ""})
    aer = {k: g["aer_" + k] for k in ("alpha", "beta", "gamma", "zeta", "a_tronc", "piztr", "piz")} if "aer_alpha" in g.files \
        else None
    return g, _user_kwargs(rs, user), aer, zout


@pytest.mark.gpu
@pytest.mark.parametrize("name", PROC_CASES)
def test_sos_proc_levels_equals_sos_proc_per_altitude(gpu_pkg, name, monkeypatch):
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)                   # the trimmed CKD data files of the gas cases
    rs = gpu_pkg.run_sos
    g, kw, aer, zg = _proc_inputs(rs, name)
    alts = [-1.0, 3.0, 0.0, 120.0, 0.75] + ([zg] if zg != -1.0 else [])
    got = rs.sos_proc_levels(alts, aer_phase=aer, **kw)
    assert len(got) == len(alts)
    for k, z in enumerate(alts):
        ref = rs.sos_proc(aer_phase=aer, **dict(kw, zout=z))
        assert_tuples_equal(got[k], ref, "%s zout=%g" % (name, z))
    if name == "flatsea_zout":
        cases.compare_proc_outputs(rs, got[-1], g)


@pytest.mark.gpu
def test_sos_proc_levels_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """torch.distributed with two ranks on one GPU (tests/dist_levels_worker.py): bins sharded, one all-reduce for the K
    record sets, the same outputs as one process."""
    res = str(tmp_path / "levels_dist.npz")
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    run_ranks("dist_levels_worker.py", ("--out", res), timeout=900, env=rank_env({"SOS_ABS_ROOT": GOLD}))
    rs = gpu_pkg.run_sos
    d = np.load(res, allow_pickle=True)
    _, kw, aer, _ = _proc_inputs(rs, "ckd_h2o_o2_25bins_flatsea")
    alts = [float(a) for a in d["alts"]]
    single = rs.sos_proc_levels(alts, aer_phase=aer, **kw)
    for k in range(len(alts)):
        for i in range(23):
            a, b = np.asarray(d["out_%d_%d" % (k, i)]), np.asarray(single[k][i])
            assert a.shape == b.shape, (k, i)
            assert np.allclose(a, b, rtol=1e-12, atol=1e-15, equal_nan=True), (k, i, np.max(np.abs(a - b)))
