"""Oracle and edge sweep of the profile-stage kernels (csrc/profile.hip): k_profile_nogas, k_profile<true> (one wavefront per
bin), k_profile<false> (one lane per bin, SOSGPU_PROFILE_LANES=1), the three *_table kernels, k_absprofile, k_output_levels and
the register form of the PROFIL file's decimal round trip (rt_e15_8 / rt_f10_5).

The bar.  NT, IBORM, the output level and the altitudes must equal the oracle's.  An H / XDEL / YDEL entry must be bit for bit the
oracle's wherever five builds of the oracle agree on it: exp as glibc gives it, every exp moved by +1 ulp, by -1 ulp, and by a
pseudo-random +-1 ulp for two keys (oracle_ctypes.EXP_MODES).  Where they disagree the reference itself says that the printed
digit hangs on the last bit of exp, and the device must give one of their values (profile_cells.rule).  CPU tests cap what may
be excused that way
(at most 1 % of the table's entries, no cell's NT) and show that the committed cells (profile_cells.py) hold the edges claimed.
The rescale, the scalars and the output level are then checked EXACTLY against the host restatement applied to the device's
own plain profile: no tolerance anywhere in this module except the existing bar of SOS_ABSPROFILE (-ln of a product near 1).

Findings written down here (and in DESIGN.md):
  * rt_e15_8 is exact from 1e-300 to the largest double and for 0, inf, nan after three fixes this sweep brought.  From
    1e8 up a value on or next to a tie was rounded the wrong way (the quotient was rounded before rint saw it):
    0x1.3b7fcf7c9e1acp+71 = 2.91027085e21, a tie neighbour of the test, came back as 2.9102708e21 where the C library
    gives 2.9102709e21.  From 1e30 up the power table was overrun (NaN).  Below 1e-15, where 10^m is not one double, 44 %
    of values came back as another double than the C library's for the same printed decimal, which showed in the XDEL of
    high levels (599 entries of this sweep): the scaling is now done on a pair of doubles.  Below 1e-300 (the last decades
    of normal numbers and the denormals) it still uses one double and is held to one unit of the eighth digit;
  * the ZMOY == 0 stop of SOS_DISC is unreachable (test_table_covers_the_edges_it_claims);
  * k_absprofile's second block of 64 layers cannot run (the API refuses nlev > 64);
  * an all-zero absorber column gives TAUABS = -0.0 below the top level (-ln 1), on the device as in C, and k_profile takes
    it for "no gas" (TGTOT == 0.0 holds for -0.0): test_absprofile_cells;
  * the refusal of the ground level of a strong-absorption bin (NT = 601 after the limit level) was searched for over
    TA x column strength and not found: forced levels are few above the limit altitude, so such bins stay near 300-450 levels.
"""
import functools

import numpy as np
import pytest

import cases
import profile_cells as PC

KEYS = ("h", "xdel", "ydel")
OUT = ("nt", "iborm", "prof", "zprof", "scal", "jout", "zz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _variants_of(name, b):
    from oracle import oracle_ctypes as O
    c = PC.CELLS[name]
    alt, tabs = PC.cell_inputs(c)
    return {m: O.sos_profile_info(c["tr"], c["hr"], c["ta"], c["ha"], alt, None if tabs is None else tabs[b], exp_mode=m)
            for m in O.EXP_MODES}


def _variants(oracle, tr, hr, ta, ha, alt, tab):
    return {m: oracle.sos_profile_info(tr, hr, ta, ha, alt, tab, exp_mode=m) for m in oracle.EXP_MODES}


def _bins_of(name):
    return range(max(1, len(PC.CELLS[name]["cols"])))


def _sensitive(var):
    """(NT differs between the variants, number of H / XDEL / YDEL entries that differ, number of entries)."""
    ex = var["exact"]
    if len({(v["ier"], v["nt"]) for v in var.values()}) != 1:
        return True, 0, 0
    if ex["ier"] != 0:
        return False, 0, 0
    n = sum(int(np.any([_bits(v[k]) != _bits(ex[k]) for v in var.values()], axis=0).sum()) for k in KEYS)
    return False, n, 3 * (ex["nt"] + 1)


# ------------------------------------------------------------------------------------------------------------ CPU: the oracle

@pytest.mark.parametrize("name", list(cases.PROFILE_CASES))
def test_info_form_is_the_pinned_oracle(oracle, name):
    """The info form in its default mode returns what sos_profile_oracle returns (pinned on sos_profile.npz by test_profile.py),
    its `raw` arrays are those values before the round trip, and the exp mode is off again after a moved run."""
    c = cases.profile_case(name)
    a = oracle.sos_profile(c["tr"], c["hr"], c["ta"], c["ha"], c["altabs"], c["tabs"])
    moved = oracle.sos_profile_info(c["tr"], c["hr"], c["ta"], c["ha"], c["altabs"], c["tabs"], exp_mode="plus")
    r = oracle.sos_profile_info(c["tr"], c["hr"], c["ta"], c["ha"], c["altabs"], c["tabs"])
    assert r["ier"] == 0 and r["nt"] == a["nt"] == moved["nt"]
    for k in ("zprof",) + KEYS:
        assert _same(r[k], a[k]), (name, k)
    for k in KEYS:
        assert _same(oracle.profile_roundtrip(r["raw"][k]), r[k]), (name, k)
    assert _same(oracle.profile_roundtrip(r["raw"]["zprof"], "f10.5"), r["zprof"])
    if c["ta"] != 0.0:                      # the moved run did move something before the rounding
        assert any(not _same(moved["raw"][k], r["raw"][k]) for k in KEYS)
    b = oracle.sos_profile(c["tr"], c["hr"], c["ta"], c["ha"], c["altabs"], c["tabs"])
    assert all(_same(a[k], b[k]) for k in KEYS)


def test_roundtrip_oracle_on_known_decimals(oracle):
    """snprintf / strtod through the oracle on values whose 8-digit rounding is known by hand."""
    v = np.array([1.0, 0.123456785, 99999999.5, 9.99999996, 1.5e-20, -2.00000005e10, 0.0, -0.0])
    exp = np.array([1.0, 0.12345678, 1.0e8, 10.0, 1.5e-20, -2.0000000e10, 0.0, -0.0])
    got = oracle.profile_roundtrip(v)
    assert _same(got[[0, 2, 3, 4, 6, 7]], exp[[0, 2, 3, 4, 6, 7]])
    assert got[1] in (0.12345678, 0.12345679) and got[5] in (-2.0000000e10, -2.0000001e10)
    assert _same(oracle.profile_roundtrip([1.0000051, -0.0000049, 119.95, 49.999996], "f10.5"), [1.00001, -0.0, 119.95, 50.0])


@pytest.mark.parametrize("name", ["o2a_mls", "h2o_o2_trop_user", "h2o_o2_subarctic", "o2a_us62_nopsurf"])
def test_absprofile_oracle_vs_reference(pkg, oracle, monkeypatch, name):
    """The plain-C SOS_ABSPROFILE against the reference's TAUABS of every bin, with the bar absprofile_host is pinned with
    (test_absorption.py), and against absprofile_host itself with the bar the device is held to against it."""
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    monkeypatch.setenv("SOS_ABS_ROOT", gold)
    A = pkg.absorption
    g = np.load(os.path.join(gold, "absorption.npz"))
    wa, nustep, psurf, h2o, o3, co2, ch4, typ = g[name + "_args"]
    p = A.prepa_absprofile(wa, nustep, psurf, h2o, o3, co2, ch4, int(typ))
    ik, _, _ = A.bins(p)
    xk, ro = A.layer_tables(p)
    ref = g[name + "_tau"]
    for b in range(len(ik)):
        tau = oracle.absprofile(xk, ro, ik[b])
        assert np.all(np.abs(tau - ref[b]) <= 2e-15 + 1e-13 * ref[b, -1]), (name, b)
        host = A.absprofile_host(xk, ro, ik[b])                       # (numpy's exp / log are not glibc's: the device's bar)
        assert np.all(np.abs(tau - host) <= 2e-15 + 1e-14 * host[-1]), (name, b)


# ----------------------------------------------------------------------------------------- CPU: the table holds what it claims

def test_table_covers_the_edges_it_claims():
    """Every edge the GPU tests are said to reach is in the table, by the oracle's own account of its run.

    The ZMOY == 0 stop of SOS_DISC is not among them because it cannot happen: a level is sought only while
    TAU(ZLIM) - H(previous) > T_LAYER, so its target TI lies below TAU(ZLIM); TAU is continuous, so the bisection closes in on a
    crossing above ZLIM and stops there by its 1e-6 test; and were it to descend without one, ZMOY would reach denormal
    altitudes where TAU(ZMOY) is TAU(0) exactly, above TI, which turns it upwards.  With strong absorption ZMIN = ZLIM > 0.
    The test asserts that no level of the table takes that stop."""
    I = {(n, b): _variants_of(n, b)["exact"] for n in PC.CELLS for b in _bins_of(n)}
    ok = {k: v for k, v in I.items() if v["ier"] == 0}
    scans_ng = {v["scan_steps_ng"] for v in I.values()} - {0}
    scans_gas = {v["scan_steps"] for v in ok.values() if v["regime"] >= 0}
    assert {1, 63, 64, 65} <= scans_ng                                  # lanes 0, 62, 63 of block one, lane 0 of block two
    for s in (scans_ng, scans_gas):                                     # and the same residues beyond three blocks
        assert {0, 1, 63} <= {x % 64 for x in s if x > 192}, sorted(s)
    steps = set()
    for v in ok.values():
        steps |= set(v["steps_ng"][2:v["nt_ng"]].tolist())
        if v["regime"] >= 0:
            steps |= set(v["steps"][2:v["nt_loop"]].tolist())
    steps.discard(0)                                                    # (the closed form of a profile without aerosols)
    assert min(steps) < 6 and {6, 7, 12, 13} <= steps and max(steps) >= 25, sorted(steps)
    gas_steps = set()
    for v in ok.values():
        if v["regime"] >= 0:
            gas_steps |= set(v["steps"][2:v["nt_loop"]].tolist())
    assert {6, 7, 12, 13} <= gas_steps and min(gas_steps) < 6 and max(gas_steps) >= 25, sorted(gas_steps)   # k_profile's own
    assert I[("deep_bisect", 0)]["steps"].max() >= 25
    assert not any(v["zero_stop"].any() or v["zero_stop_ng"].any() for v in ok.values())
    gas = [v for v in ok.values() if v["regime"] >= 0]
    assert any(v["forced"].any() for v in gas) and any(v["near_skip"].any() for v in gas)
    assert any(v["dropped"] and not v["dropped_first"] and not v["strong"] for v in gas)
    assert any(v["dropped"] and not v["dropped_first"] and v["strong"] for v in gas)
    assert I[("drop_first", 0)]["dropped_first"] == 1 and I[("drop_first", 0)]["nt"] == 2
    assert any(v["ing"] == v["nt_ng"] + 1 for v in gas)                 # ING one past the no-gas profile: the min() clamp
    # regimes on both sides of their boundaries, adjacent doubles of the total optical depth's last term
    r = [I[("regimes_gas", b)] for b in range(4)]
    assert [v["regime"] for v in r] == [0, 1, 1, 2]
    cols = PC.CELLS["regimes_gas"]["cols"]
    assert np.nextafter(cols[0][1], 1.0) == cols[1][1] and np.nextafter(cols[2][1], 1.0) == cols[3][1]
    assert r[0]["ttot"] / 100 <= PC.T_FIRST < r[1]["ttot"] / 100 and r[2]["ttot"] / 100 < PC.TCOUCHE <= r[3]["ttot"] / 100
    g = [I[(n, 0)] for n in ("regime_ng_0", "regime_ng_1lo", "regime_ng_1hi", "regime_ng_2")]
    assert [v["regime_ng"] for v in g] == [0, 1, 1, 2]
    ta = [PC.CELLS[n]["ta"] for n in ("regime_ng_0", "regime_ng_1lo", "regime_ng_1hi", "regime_ng_2")]
    assert np.nextafter(ta[0], 1.0) == ta[1] and np.nextafter(ta[2], 1.0) == ta[3]
    # strong-absorption threshold
    a, b = I[("tg_1p5", 0)], I[("tg_1p5", 1)]
    assert a["tgtot"] == 1.5 and a["strong"] == 0 and b["tgtot"] == np.nextafter(1.5, 2.0) and b["strong"] == 1
    assert any(v["strong"] and v["clamp"] for v in gas) and any(v["strong"] and not v["clamp"] for v in gas)
    assert I[("no_clamp", 0)]["t_layer_unclamped"] > PC.TCOUCHE
    # level count limits
    assert I[("ng_600", 0)]["nt_ng"] == 600 and I[("ng_600", 0)]["ier"] == 0
    from oracle import oracle_ctypes as O
    over = O.sos_profile_info(0.0948, 8.0, PC.NG601_TA, 2.0)
    assert over["ier"] == -1 and over["ier_from"] == 1 and over["nt_ng"] == 601
    assert I[("gas_600", 0)]["nt"] == 600 and I[("gas_600", 0)]["regime"] == 2
    assert I[("gas_600", 1)]["ier"] == -1 and I[("gas_600", 1)]["ier_from"] == 2 and I[("gas_600", 1)]["nt_loop"] == 600
    for short, tight in (("lp_short", "lp_tight"), ("lp_strong_short", "lp_strong_tight")):
        assert PC.CELLS[short]["lp"] + 1 == PC.CELLS[tight]["lp"]
        assert PC.expected_flag(I[(short, 0)], PC.CELLS[short]["lp"]) and not PC.expected_flag(I[(tight, 0)], PC.CELLS[tight]["lp"])
    # grids, scatterers, SOS.F parameters
    alt0 = {n: PC.grid(c["grid"])[0] for n, c in PC.CELLS.items() if c["grid"]}
    assert alt0["grid_low80"] < 120.0 and alt0["grid_low80"] > I[("grid_low80", 0)]["zprof"][1]
    assert alt0["grid_low30"] < I[("grid_low30", 0)]["zprof"][1] and alt0["grid_low30"] < I[("grid_low30", 1)]["zprof"][1]
    assert {len(PC.grid(c["grid"])) for c in PC.CELLS.values() if c["grid"]} >= {2, 50, 64}
    assert any(c["ta"] == 0.0 and c["grid"] for c in PC.CELLS.values()) and any(c["ta"] == 0.0 and not c["grid"] for c in PC.CELLS.values())
    assert {c["smax"] for c in PC.CELLS.values() if c["ta"] == 0.0 and not c["grid"]} >= {1, 2, 16}
    assert any(c["a_tronc"] == 0.0 for c in PC.CELLS.values()) and any(c["a_tronc"] != 0.0 for c in PC.CELLS.values())
    assert any(c["piztr"] == 0.0 and c["ta"] != 0.0 for c in PC.CELLS.values())
    assert not np.any(PC.cell_inputs(PC.CELLS["zero_col"])[1][0]) and I[("zero_col", 0)]["regime"] == -1
    # output altitudes: on the ground, below the last level of a strong bin, above the first level, between levels
    z = {c["zout"] for c in PC.CELLS.values()}
    assert {0.0, -0.5, -1.0} <= z and PC.CELLS["base_very_strong"]["zout"] == -0.5 and I[("base_very_strong", 0)]["strong"]
    assert PC.CELLS["scan_ng_1"]["zout"] > I[("scan_ng_63", 0)]["zprof"][1]


def test_sensitivity_to_the_last_bit_of_exp_is_capped():
    """From the reference alone: no cell's NT depends on the last bit of exp, and at most 1 % of the table's printed entries
    do.  (Measured when the table was fixed: see the figures this test prints.)"""
    tot = sens = 0
    worst = ("", 0)
    for n in PC.CELLS:
        for b in _bins_of(n):
            nt_moves, k, m = _sensitive(_variants_of(n, b))
            assert not nt_moves, (n, b)
            tot += m
            sens += k
            if k > worst[1]:
                worst = ("%s[%d]" % (n, b), k)
    print("sensitive entries: %d of %d (%.4f %%), most in %s: %d" % (sens, tot, 100.0 * sens / tot, worst[0], worst[1]))
    assert tot > 30000 and sens <= 0.01 * tot


# ------------------------------------------------------------------------------------------------------------------ GPU helpers

def _ctx(gpu_pkg, smax=16):
    S = gpu_pkg.synth
    mu, w, n0 = S.gauss_angles(8, 35.0)
    al, be, ga, ze = S.hg_phase(16, 0.5)
    return gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=smax, ro=0.1)


def _host(p):
    import torch
    torch.cuda.synchronize()
    return {k: (None if p[k] is None else p[k].cpu().numpy()) for k in OUT}


def _equal_outputs(a, b, what):
    import torch
    for k in OUT:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (what, k)


def _out_level(z, h, nt, zout):
    """SOS.F:570-582 / SOS_OS.F:1514-1520: the first level J >= 1 with ZOUT >= Z(J), the linear weight ZZ, TAUOUT.
    solver.output_levels_host states the same rule but could not serve here: it has no stop at NT (it is only given
    altitudes above the ground) and would run past the last level for the ZOUT below it that this sweep needs, and it does not
    form TAUOUT.  So the rule is restated with the stop the kernels document; where two levels print the same altitude
    (tg_1p5[1]) it divides by zero as they do."""
    if zout == -1.0:
        return 0, 0.0, h[0]
    j = 1
    while j < nt and zout < z[j]:
        j += 1
    with np.errstate(divide="ignore", invalid="ignore"):      # (tg_1p5[1]: limit level and ground on one printed altitude)
        zz = (zout - z[j - 1]) / (z[j] - z[j - 1])
        return j, zz, (1 - zz) * h[j - 1] + zz * h[j]


def _check_bin_against_variants(d, b, var, what):
    """NT, Z identical; H / XDEL / YDEL identical or one of the variants' values.  d: host copy of a PLAIN run."""
    ex = var["exact"]
    nt = ex["nt"]
    assert d["nt"][b] == nt, (what, d["nt"][b], nt)
    k = nt + 1
    assert _same(d["zprof"][b, :k], ex["zprof"]), what
    assert not d["zprof"][b, k:].any() and not d["prof"][b, :, k:].any(), what
    n = same = 0
    for row, key in enumerate(KEYS):
        ok, exact = PC.rule(d["prof"][b, row, :k], [ex[key]] + [v[key] for v in var.values()])
        bad = np.nonzero(~ok)[0]
        assert bad.size == 0, (what, key, bad[:5], d["prof"][b, row, bad[:5]], ex[key][bad[:5]])
        n += k
        same += int(exact.sum())
    return n, same


def _report(what, counts):
    """One line per test for the figures of DESIGN.md: entries compared, bit-identical to the exact oracle, excused as sensitive."""
    n, same = (sum(c[i] for c in counts) for i in (0, 1))
    print("%s: %d bins, %d entries, %d bit-identical, %d sensitive excused" % (what, len(counts), n, same, n - same))


def _check_dressed(oracle, plain, full, b, c, smax, what):
    """Rescale, IBORM, scalars and output level of run `full` == the host restatement on the plain profile of the device."""
    nt = int(plain["nt"][b])
    k = nt + 1
    h, x, y, ib = oracle.profile_rescale(plain["prof"][b, 0, :k], plain["prof"][b, 1, :k], plain["prof"][b, 2, :k],
                                         c["a_tronc"], c["piz"], c["piztr"], smax)
    assert full["nt"][b] == nt and _same(full["zprof"][b], plain["zprof"][b]), what
    assert _same(full["prof"][b, 0, :k], h) and _same(full["prof"][b, 1, :k], x) and _same(full["prof"][b, 2, :k], y), what
    assert not full["prof"][b, :, k:].any(), what
    assert full["iborm"][b] == (min(2, smax) if ib == 2 and not x.any() else smax), what
    j, zz, tau = _out_level(plain["zprof"][b], h, nt, c["zout"])
    assert _same(full["scal"][b], [0.0, h[nt], plain["prof"][b, 0, nt], tau]), (what, full["scal"][b], tau)
    if c["zout"] != -1.0:
        assert full["jout"][b] == j and _same(full["zz"][b], zz), (what, full["jout"][b], j)
    else:
        assert full["jout"] is None and full["zz"] is None


def _check_flagged(d, b, what):
    assert d["nt"][b] == -1 and d["iborm"][b] == 0 and not d["scal"][b].any(), what
    if d["jout"] is not None:
        assert d["jout"][b] == 0 and d["zz"][b] == 0.0, what


# ------------------------------------------------------------------------------------------------------------ GPU: round trip

def _roundtrip_values():
    rng = np.random.default_rng(20240607)
    sgn = lambda n: rng.choice([-1.0, 1.0], n)
    parts = [sgn(1000000) * 10.0 ** rng.uniform(-300.0, 300.0, 1000000),
             10.0 ** rng.uniform(-16.0, 1.0, 1000000)]
    # ties of the 8-digit rounding: (m + 1/2) 10^e for 200 random (m, e), every double within 40 ulps of each, and the
    # 8-digit decimals on both sides with their neighbours
    m = rng.integers(10000000, 99999999, 200).astype(np.float64)
    e = rng.integers(-30, 15, 200)
    for half in (0.5, 0.0, 1.0):
        t = (m + half) * 10.0 ** e.astype(np.float64)
        for _ in range(40):
            parts.append(t.copy())
            t = np.nextafter(t, np.inf)
        t = (m + half) * 10.0 ** e.astype(np.float64)
        for _ in range(40):
            t = np.nextafter(t, -np.inf)
            parts.append(t.copy())
    p10 = np.array([float("1e%d" % k) for k in range(-30, 23)])
    parts += [p10, np.nextafter(p10, np.inf), np.nextafter(p10, -np.inf), -p10]
    nines = np.array([float("9.9999999%se%d" % (tail, k)) for k in range(-25, 23) for tail in ("5", "49999999", "50000001", "4", "6")])
    parts += [nines, np.nextafter(nines, np.inf), np.nextafter(nines, -np.inf), -nines]
    parts.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -3e-320,
                           1.7976931348623157e308, 1e8, 99999999.5, 123456785.0, 1e-15, 9.9999999e-16, 1.00000005e-15]))
    return np.concatenate(parts)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["e15.8", "f10.5"])
def test_roundtrip_is_the_c_librarys(gpu_pkg, oracle, fmt):
    """rt_e15_8 / rt_f10_5 (sosgpu_debug_roundtrip, one thread per value) == snprintf + strtod, every value bit for bit: two
    million log-uniform values (1e-300..1e300, 1e-16..10), the neighbourhoods of 600 ties and 8-digit decimals, powers of ten
    1e-30..1e22 +- 1 ulp, 9.9999999|5 carries, negatives, +-0, subnormals, inf and nan.  Every value from 1e-300 up must be
    identical (no tolerance), 0, inf and nan too.  Below 1e-300 -- a part of the m > 22 branch that the pair of doubles
    for 10^m does not reach, because 10^m itself overflows -- the result is held to one unit of the eighth printed digit of
    the reference (plus one denormal step); measured: 1 of the 5 such values here differs.  F10.5 takes
    the values it can print in a field (|v| < 1e4) and must be exact on all of them."""
    import ctypes as C
    import torch
    v = _roundtrip_values()
    if fmt == "f10.5":
        v = v[~(np.abs(v) >= 1e4)]
        v = np.concatenate([v, np.round(np.random.default_rng(5).uniform(0, 120, 200000), 5) + 0.000005])
    assert v.size >= (2000000 if fmt == "e15.8" else 1000000)
    t = torch.from_numpy(v).cuda()
    out = torch.empty_like(t)
    gpu_pkg.capi.check(gpu_pkg.capi.lib().sosgpu_debug_roundtrip(0, 0 if fmt == "e15.8" else 1, v.size, C.c_void_p(t.data_ptr()),
                                                                 C.c_void_p(out.data_ptr()), None), "sosgpu_debug_roundtrip")
    torch.cuda.synchronize()
    got, ref = out.cpu().numpy(), oracle.profile_roundtrip(v, fmt)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    differ = (_bits(got) != _bits(ref)) & ~nan
    av = np.abs(v)
    low = (av < 1e-300) & (av != 0.0) if fmt == "e15.8" else np.zeros(v.size, dtype=bool)
    bad = np.nonzero(differ & ~low)[0]
    print("%s: %d values, %d differ from 1e-300 up; %d of %d below 1e-300 differ"
          % (fmt, v.size, bad.size, int((differ & low).sum()), int(low.sum())))
    assert bad.size == 0, [(float(v[i]).hex(), float(got[i]).hex(), float(ref[i]).hex()) for i in bad[:8]]
    sel = np.nonzero(differ & low)[0]
    unit = 10.0 ** (np.floor(np.log10(np.abs(ref[sel]))) - 7.0)          # one unit of the eighth printed digit
    over = sel[~(np.abs(got[sel] - ref[sel]) <= unit * (1 + 1e-9) + 5e-324)]
    assert over.size == 0, [(float(v[i]).hex(), float(got[i]).hex(), float(ref[i]).hex()) for i in over[:8]]


# ---------------------------------------------------------------------------------------------------------- GPU: profile cells

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PC.CELLS))
def test_profile_cell(gpu_pkg, oracle, monkeypatch, name):
    """One cell through sosgpu_profile by one wavefront per bin and by one lane per bin: equal outputs; the plain profile under
    the identical-or-sensitive rule; rescale, IBORM, scalars and output level exactly; sosgpu_output_levels at six altitudes
    (standard output, ground, exactly on a level, between levels, below the last level, above the first)."""
    import torch
    c = PC.CELLS[name]
    alt, tabs = PC.cell_inputs(c)
    nb = 1 if tabs is None else len(tabs)
    cx = _ctx(gpu_pkg, c["smax"])
    geo = (nb, c["tr"], c["hr"], c["ta"], c["ha"], alt, tabs)
    kw = dict(a_tronc=c["a_tronc"], piz=c["piz"], piztr=c["piztr"], zout=c["zout"], lp=c["lp"])
    wave = cx.make_profiles(*geo, **kw)
    monkeypatch.setenv("SOSGPU_PROFILE_LANES", "1")
    lanes = cx.make_profiles(*geo, **kw)
    monkeypatch.delenv("SOSGPU_PROFILE_LANES")
    plain = cx.make_profiles(*geo, lp=c["lp"])
    torch.cuda.synchronize()
    _equal_outputs(wave, lanes, name)
    full, pl = _host(wave), _host(plain)
    var = [_variants_of(name, b) for b in range(nb)]
    flagged = [PC.expected_flag(v["exact"], c["lp"]) for v in var]
    zs = var[0]["exact"]["zprof"] if not flagged[0] else np.array([120.0, 50.0, 0.0])
    alts = [-1.0, 0.0, float(zs[len(zs) // 2]), 0.5 * float(zs[1] + zs[2]), -0.5, 119.0]
    lev = cx.output_levels(wave, alts)
    torch.cuda.synchronize()
    lev = {k: lev[k].cpu().numpy() for k in ("jout", "zz", "tauout")}
    counts = []
    for b in range(nb):
        what = "%s[%d]" % (name, b)
        if flagged[b]:
            _check_flagged(full, b, what)
            _check_flagged(pl, b, what)
            assert not lev["jout"][:, b].any() and not lev["zz"][:, b].any() and not lev["tauout"][:, b].any(), what
            continue
        counts.append(_check_bin_against_variants(pl, b, var[b], what))
        _check_dressed(oracle, pl, full, b, c, c["smax"], what)
        nt = int(full["nt"][b])
        for k, zo in enumerate(alts):
            j, zz, tau = _out_level(full["zprof"][b], full["prof"][b, 0], nt, zo)
            assert lev["jout"][k, b] == j and _same(lev["zz"][k, b], zz) and _same(lev["tauout"][k, b], tau), (what, zo)
    _report("cell " + name, counts)
    cx.close()


@pytest.mark.gpu
def test_no_gas_grid_of_601_levels_is_refused(gpu_pkg):
    """The next double of TA after the 600-level cell: CTE_OS_NT + 1 levels, the reference's IER = -1, refused before a launch
    by sosgpu_profile, sosgpu_profile_nogas and sosgpu_profile_spectrum alike."""
    cx = _ctx(gpu_pkg)
    assert gpu_pkg.capi.lib().sosgpu_profile_nogas_levels(0.0948, PC.NG600_TA) == 600
    assert gpu_pkg.capi.lib().sosgpu_profile_nogas_levels(0.0948, PC.NG601_TA) == -1
    with pytest.raises(gpu_pkg.capi.SosgpuError) as e:
        cx.make_profiles(1, 0.0948, 8.0, PC.NG601_TA, 2.0)
    assert "unsupported" in str(e.value).lower() or e.value.code != 0
    with pytest.raises(gpu_pkg.capi.SosgpuError):
        gpu_pkg.solver.nogas_profile(0.0948, 8.0, PC.NG601_TA, 2.0)
    req = dict(tr=0.0948, hr=8.0, ta=PC.NG601_TA, ha=2.0, a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, smax=16, ik=None)
    part = {}
    with pytest.raises(gpu_pkg.capi.SosgpuError):
        gpu_pkg.solver.make_profiles_spectrum([dict(req, ta=0.3), req], part=part)
    assert part.get("bad") == 1
    cx.close()


NO_GAS_CELLS = [n for n, c in PC.CELLS.items() if c["grid"] is None]


@pytest.mark.gpu
def test_no_gas_cells_as_one_part_of_the_table_kernels(gpu_pkg):
    """Every cell that qualifies for solver.make_profiles_spectrum as wavelengths of ONE part: k_profile_nogas_table and the copy
    branch of k_profile_table at the scan edges (steps 1, 63, 64, 65, 1407-1409), the regime boundaries, 600 levels (against the
    nt_ng >= ngl guard), ta = 0, with rescale, piztr, output altitudes and SMAX 1, 2, 16 -- torch.equal, on every output, with
    the cell's wave-form and one-lane results (which test_profile_cell holds against the oracle).  A cell qualifies when it has
    no gas and the part's lp: the table entry takes a wavelength's gas as (ik, xk, ro) for k_absprofile_table, not as a TAUABS
    column, so the cells that fix TAUABS to the bit (thresholds, regimes, 600 levels of the gas step) cannot be stated as
    requests; the table's gas path is driven by test_absprofile_cells_and_table_kernels from its own TAUABS instead."""
    import torch
    assert len(NO_GAS_CELLS) >= 18 and all(PC.CELLS[n]["lp"] == 608 for n in NO_GAS_CELLS)
    reqs = [dict({k: PC.CELLS[n][k] for k in ("tr", "hr", "ta", "ha", "a_tronc", "piz", "piztr", "zout", "smax")}, ik=None)
            for n in NO_GAS_CELLS]
    part = {}
    bins = gpu_pkg.solver.make_profiles_spectrum(reqs, part=part)
    torch.cuda.synchronize()
    ctx = {}
    for n, tb in zip(NO_GAS_CELLS, bins):
        c = PC.CELLS[n]
        cx = ctx.setdefault(c["smax"], _ctx(gpu_pkg, c["smax"]))
        wave = cx.make_profiles(1, c["tr"], c["hr"], c["ta"], c["ha"], a_tronc=c["a_tronc"], piz=c["piz"], piztr=c["piztr"],
                                zout=c["zout"])
        torch.cuda.synchronize()
        _equal_outputs(wave, tb, n)
        assert int(tb["nt"][0]) >= 100, n
    assert int(bins[NO_GAS_CELLS.index("ng_600")]["nt"][0]) == 600
    for cx in ctx.values():
        cx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2049, 4097])
def test_batch_one_lane_form_equals_wave_form(gpu_pkg, oracle, monkeypatch, nb):
    """2 049 and 4 097 bins (five distinct columns, tiled): the one-lane form packs 2 and 3 bins per wavefront and leaves the last
    block partly empty (the threadIdx >= bpw guard, the b >= nb guard); every bin equals its wave-form twin, and the first five
    the oracle."""
    import torch
    c = PC.CELLS["base_gas"]
    alt = PC.grid("std")
    cols = np.array([PC.column(alt, s) for s in list(c["cols"]) + [("zero",), ("exp", 60.0, 5.0)]])
    tabs = cols[np.arange(nb) % len(cols)]
    cx = _ctx(gpu_pkg)
    kw = dict(a_tronc=c["a_tronc"], piz=c["piz"], piztr=c["piztr"], zout=c["zout"])
    wave = cx.make_profiles(nb, c["tr"], c["hr"], c["ta"], c["ha"], alt, tabs, **kw)
    monkeypatch.setenv("SOSGPU_PROFILE_LANES", "1")
    lanes = cx.make_profiles(nb, c["tr"], c["hr"], c["ta"], c["ha"], alt, tabs, **kw)
    monkeypatch.delenv("SOSGPU_PROFILE_LANES")
    torch.cuda.synchronize()
    _equal_outputs(wave, lanes, nb)
    n = (nb // len(cols)) * len(cols)
    for k in OUT:                                             # and every tile equals the first
        t = wave[k][:n].reshape((n // len(cols), len(cols)) + tuple(wave[k].shape[1:]))
        assert torch.equal(t, t[0:1].expand_as(t)), k
    assert int(wave["nt"].min()) >= 101
    plain = _host(cx.make_profiles(len(cols), c["tr"], c["hr"], c["ta"], c["ha"], alt, cols))
    full = {k: None if wave[k] is None else wave[k][:len(cols)].cpu().numpy() for k in OUT}
    for b in range(len(cols)):
        var = _variants(oracle, c["tr"], c["hr"], c["ta"], c["ha"], alt, cols[b])
        assert _check_bin_against_variants(plain, b, var, "batch[%d]" % b)[0] > 300
        _check_dressed(oracle, plain, full, b, c, 16, "batch[%d]" % b)
    cx.close()


# -------------------------------------------------------------------------------- GPU: SOS_ABSPROFILE cells and the table kernels

def _abs_part(nlev):
    """The wavelengths of one part of a spectrum on an absorption grid of nlev levels: requests for make_profiles_spectrum.
    Two absorbers (gases 1 and 7), NTERM 1 and 5, term indices 0 and NTERM + 1 (clamped), a column that underflows partway down,
    an all-zero column, wavelengths without gas, with and without rescale / output altitude, SMAX 1, 2 and 16."""
    alt = {2: PC.grid("two"), 50: PC.grid("std"), 64: PC.grid("g64")}[nlev]
    nl1 = nlev - 1
    d1 = np.diff(np.exp(-alt / 7.0))
    d7 = np.diff(np.exp(-alt / 5.0))
    reqs = []

    def gas(nterm, scales, ik, **kw):
        xk = np.zeros((8, nterm, nl1))
        ro = np.zeros((8, nl1))
        ro[0], ro[6] = 1.0, 0.5
        for t in range(nterm):
            xk[0, t], xk[6, t] = scales[t] * d1, 2.0 * scales[-1 - t] * d7
        base = dict(tr=0.0948, hr=8.0, ta=0.3, ha=2.0, a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, smax=16, absprofil=1)
        base.update(kw)
        reqs.append(dict(base, ik=np.array(ik, dtype=np.int32), xk=xk, ro=ro, altabs=alt))

    one = [1, 1, 1, 1, 1, 1, 1, 1]
    gas(1, [0.4], [one, [0, 1, 1, 1, 1, 1, 2, 1]], a_tronc=PC.A, piz=PC.P, piztr=PC.PT, zout=3.2)
    gas(5, [0.01, 0.3, 1.2, 9.0, 3000.0],
        [[1, 1, 1, 1, 1, 1, 5, 1], [2, 1, 1, 1, 1, 1, 4, 1], [3, 1, 1, 1, 1, 1, 3, 1], [4, 1, 1, 1, 1, 1, 2, 1],
         [5, 1, 1, 1, 1, 1, 1, 1], [0, 9, 9, 0, 6, 6, 6, 0], [6, 1, 1, 1, 1, 1, 0, 1]], zout=0.0)
    reqs.append(dict(tr=0.0948, hr=8.0, ta=0.0, ha=2.0, a_tronc=PC.A, piz=PC.P, piztr=PC.PT, zout=-1.0, smax=2, ik=None))
    gas(1, [0.0], [one], ta=0.1, ha=3.0, smax=2)                                  # all-zero absorbers
    gas(5, [0.2, 0.5, 0.9, 2.0, 5.0], [[1, 1, 1, 1, 1, 1, 1, 1], [5, 1, 1, 1, 1, 1, 5, 1]], tr=0.02, ta=0.15, zout=12.5, smax=1)
    reqs.append(dict(tr=0.01, hr=8.0, ta=0.005, ha=2.0, a_tronc=0.0, piz=1.0, piztr=1.0, zout=50.0, smax=16, ik=None))
    return alt, reqs


@pytest.mark.gpu
@pytest.mark.parametrize("nlev", [2, 50, 64])
def test_absprofile_cells_and_table_kernels(gpu_pkg, oracle, monkeypatch, nlev):
    """The wavelengths of _abs_part as ONE part through the three table kernels, and each wavelength through sosgpu_absprofile
    and sosgpu_profile (wave form and one-lane form): equal outputs, TAUABS included.  TAUABS against the plain-C oracle with the
    bar of test_absorption.py (2e-15 + 1e-14 of the column) and the 999 pattern exactly; an all-zero column gives -0.0 below
    the top level on both sides (-ln 1) and the no-gas profile from k_profile.  The profiles, made from the device's own
    TAUABS, under the identical-or-sensitive rule with the caps of the CPU test asserted here as well."""
    import torch
    alt, reqs = _abs_part(nlev)
    part = {}
    bins = gpu_pkg.solver.make_profiles_spectrum(reqs, part=part)
    torch.cuda.synchronize()
    saw_999 = saw_zero = False
    tot = sens = 0
    counts = []
    for w, r in enumerate(reqs):
        cx = _ctx(gpu_pkg, r["smax"])
        kw = dict(a_tronc=r["a_tronc"], piz=r["piz"], piztr=r["piztr"], zout=r["zout"])
        if r["ik"] is None:
            nb, t_alt, tabs, tabs_h = 1, None, None, None
            assert part["tabs"][w] is None
        else:
            nb, t_alt = len(r["ik"]), alt
            tabs = cx.absorption_profiles(r["ik"], r["xk"], r["ro"])
            torch.cuda.synchronize()
            assert torch.equal(tabs, part["tabs"][w]), w
            tabs_h = tabs.cpu().numpy()
            for b in range(nb):
                ref = oracle.absprofile(r["xk"], r["ro"], r["ik"][b])
                m = ref == 999.0
                assert np.array_equal(tabs_h[b] == 999.0, m), (w, b)
                fin = ref[~m]
                assert np.all(np.abs(tabs_h[b][~m] - fin) <= 2e-15 + 1e-14 * fin.max()), (w, b)
                if m.any():
                    saw_999 = True
                    assert nlev == 2 or (not m[1] and m[-1] and np.all(np.diff(m.astype(int)) >= 0)), (w, b)   # partway down
                if not r["xk"].any():
                    saw_zero = True
                    assert tabs_h[b, 0] == 0.0 and not np.signbit(tabs_h[b, 0])
                    assert np.all(tabs_h[b, 1:] == 0.0) and np.all(np.signbit(tabs_h[b, 1:])) and np.all(np.signbit(ref[1:]))
        geo = (nb, r["tr"], r["hr"], r["ta"], r["ha"], t_alt, tabs)
        wave = cx.make_profiles(*geo, **kw)
        monkeypatch.setenv("SOSGPU_PROFILE_LANES", "1")
        lanes = cx.make_profiles(*geo, **kw)
        monkeypatch.delenv("SOSGPU_PROFILE_LANES")
        plain = cx.make_profiles(*geo)
        torch.cuda.synchronize()
        _equal_outputs(wave, lanes, (nlev, w))
        _equal_outputs(wave, bins[w], (nlev, w, "table"))
        full, pl = _host(wave), _host(plain)
        for b in range(nb):
            what = "part %d wavelength %d bin %d" % (nlev, w, b)
            var = _variants(oracle, r["tr"], r["hr"], r["ta"], r["ha"], t_alt, None if tabs_h is None else tabs_h[b])
            nt_moves, k, m = _sensitive(var)
            assert not nt_moves, what
            tot += m
            sens += k
            assert not PC.expected_flag(var["exact"], 608), what
            if tabs_h is not None and not r["xk"].any():
                assert var["exact"]["regime"] == -1 and pl["nt"][b] == var["exact"]["nt_ng"], what
            counts.append(_check_bin_against_variants(pl, b, var, what))
            _check_dressed(oracle, pl, full, b, r, r["smax"], what)
        cx.close()
    assert saw_zero and (saw_999 or nlev == 2)
    assert sens <= 0.01 * tot, (sens, tot)
    _report("part %d" % nlev, counts)
