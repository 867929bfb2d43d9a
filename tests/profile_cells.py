"""Cells of tests/test_profile_edges.py: the inputs of the profile-stage sweep and the helpers that build them.

A profile cell is one call of sosgpu_profile: a wavelength (tr, hr, ta, ha), an absorption grid, one or more gas columns (the
bins), the SOS.F parameters (a_tronc, piz, piztr, zout), the order count of the context (smax) and the level capacity lp.
Every number below is fixed; the CPU tests of test_profile_edges.py show, with the oracle's info form, that the cells hold the
edges their names claim."""
import numpy as np

T_FIRST = float(np.float32(0.0002))
TCOUCHE = float(np.float32(0.005))
DZ = float(np.float32(0.001))
UP = float(np.nextafter(1.5, 2.0))


def grid(name):
    """Altitude grids of the absorption profile (descending, ground last)."""
    if name == "std":                    # the grid of cases.PROFILE_CASES: 50 levels, top at the top of the atmosphere
        return np.concatenate([np.linspace(120.0, 30.0, 10), np.linspace(28.0, 0.0, 40)])
    if name == "low80":                  # top below the top of the atmosphere, above the first level
        return np.concatenate([np.linspace(80.0, 30.0, 10), np.linspace(28.0, 0.0, 40)])
    if name == "low30":                  # top below the first level as well
        return np.linspace(30.0, 0.0, 50)
    if name == "two":                    # the smallest grid
        return np.array([120.0, 0.0])
    if name == "g64":                    # the largest the kernels keep in LDS
        return np.concatenate([np.linspace(120.0, 32.0, 12), np.linspace(31.0, 0.0, 52)])
    if name == "step":                   # 1.5 reached 50 m below the top: the limit level sits on the first level
        return np.concatenate([[120.0, 119.9], np.linspace(100.0, 0.0, 48)])
    raise KeyError(name)


def column(alt, spec):
    """A gas column on the grid: ("exp", k, hg) = k exp(-z / hg), zero at the top level; ("exp0", k, hg) the same with the top
    level kept; ("norm", last, hg) = exp(-z / hg) scaled so that the ground value is EXACTLY `last`; ("step", top) = `top`
    from the second level down to 2 `top` at the ground; ("zero",) all zero; ("raw", values)."""
    kind = spec[0]
    if kind == "exp" or kind == "exp0":
        tab = spec[1] * np.exp(-alt / spec[2])
        if kind == "exp":
            tab[0] = 0.0
        return tab
    if kind == "norm":
        sh = np.exp(-alt / spec[2])
        sh[0] = 0.0
        tab = sh / sh[-1] * spec[1]
        assert tab[-1] == spec[1]
        return tab
    if kind == "step":
        tab = np.linspace(spec[1], 2.0 * spec[1], len(alt))
        tab[0] = 0.0
        return tab
    if kind == "zero":
        return np.zeros(len(alt))
    if kind == "raw":
        return np.asarray(spec[1], dtype=np.float64)
    raise KeyError(kind)


def cell(tr, hr, ta, ha, grid_name=None, cols=(), a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, smax=16, lp=608):
    return dict(tr=tr, hr=hr, ta=ta, ha=ha, grid=grid_name, cols=tuple(cols), a_tronc=a_tronc, piz=piz, piztr=piztr, zout=zout,
                smax=smax, lp=lp)


def cell_inputs(c):
    """(altabs, tabs[nb][nblev]) of a cell, or (None, None) without gas."""
    if c["grid"] is None:
        return None, None
    alt = grid(c["grid"])
    return alt, np.array([column(alt, s) for s in c["cols"]])


NG600_TA = 2.9053999329397215
A, P, PT = 0.37, 0.95, 0.93           # a truncation coefficient and the two albedos of the cells that rescale

# name -> cell.  The comment of a cell names the edge it is in the table for (asserted in test_profile_edges.py).
CELLS = {
    # ---- the eleven columns of cases.PROFILE_CASES, with the rescale and an output altitude
    "base_nogas": cell(0.0948, 8.0, 0.3, 2.0, a_tronc=A, piz=P, piztr=PT, zout=3.2),
    "base_ray_only": cell(0.0948, 8.0, 0.0, 2.0, zout=0.0),                                  # ta = 0, XDEL all zero, smax 16
    "base_thin": cell(0.01, 8.0, 0.005, 2.0, a_tronc=A, piz=P, piztr=PT, zout=50.0),
    "base_thick_aer": cell(0.0948, 8.0, 1.5, 1.5, zout=1.0),
    "base_gas": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 0.4, 7.0), ("exp", 1.2, 7.0), ("exp", 8.0, 7.0)], a_tronc=A, piz=P,
                     piztr=PT, zout=3.2),
    "base_very_strong": cell(0.0948, 8.0, 0.1, 3.0, "std", [("exp", 60.0, 5.0)], zout=-0.5),    # zout below the last level
    "base_gas_ray": cell(0.0948, 8.0, 0.0, 2.0, "std", [("exp", 0.7, 7.0)], smax=2),
    "base_gas_thin": cell(0.004, 8.0, 0.002, 2.0, "std", [("exp", 0.003, 7.0)], a_tronc=A, piz=P, piztr=0.0),   # piztr = 0
    "base_h2o_like": cell(0.02, 8.0, 0.15, 2.0, "std", [("exp", 0.9, 2.0)], zout=0.0),
    # ---- strong-absorption threshold: TGTOT = 1.5 exactly (not strong) and the next double (strong)
    "tg_1p5": cell(0.0948, 8.0, 0.3, 2.0, "std", [("norm", 1.5, 7.0), ("norm", UP, 7.0)], zout=0.4),
    # ---- the other grids
    "grid_two": cell(0.0948, 8.0, 0.3, 2.0, "two", [("raw", [0.0, 0.6]), ("raw", [0.0, 4.0])], a_tronc=A, piz=P, piztr=PT, zout=7.0),
    "grid_64": cell(0.05, 8.0, 0.2, 2.5, "g64", [("exp", 0.5, 6.0), ("exp", 12.0, 4.0)], zout=12.5),
    "grid_low80": cell(0.0948, 8.0, 0.3, 2.0, "low80", [("exp", 0.8, 7.0), ("exp", 9.0, 7.0)]),
    "grid_low30": cell(0.0948, 8.0, 0.3, 2.0, "low30", [("exp0", 0.8, 7.0), ("exp0", 9.0, 7.0)], a_tronc=A, piz=P, piztr=PT),
    # ---- the limit level on the first level: the dropped level with NT - 1 == 0
    "drop_first": cell(0.0948, 8.0, 0.3, 2.0, "step", [("step", 3.0)], zout=60.0),
    # ---- all-zero columns: the no-gas profile is copied
    "zero_col": cell(0.0948, 8.0, 0.3, 2.0, "std", [("zero",), ("exp", 0.4, 7.0)]),
    "ray_smax1": cell(0.0948, 8.0, 0.0, 2.0, smax=1),
    "ray_smax2": cell(0.0948, 8.0, 0.0, 2.0, a_tronc=A, piz=P, piztr=PT, smax=2),
    # ---- first-level scan of the no-gas profile stopping at step 1, 63, 64, 65 (lane 0, 62, 63 of the first block; lane 0 of
    #      the second), and at 64 k - 1, 64 k, 64 k + 1 steps twenty blocks further down
    "scan_ng_1": cell(0.1, 19.301347461076734, 0.05, 2.0, zout=119.975),       # above the first level
    "scan_ng_63": cell(0.1, 18.80252275893996, 0.05, 2.0, zout=100.0),
    "scan_ng_64": cell(0.1, 18.794477199228076, 0.05, 2.0),
    "scan_ng_65": cell(0.1, 18.786381639516193, 0.05, 2.0, a_tronc=A, piz=P, piztr=PT),
    "scan_ng_1407": cell(0.0948, 8.0585, 0.3, 2.0),
    "scan_ng_1408": cell(0.0948, 8.0505, 0.3, 2.0),
    "scan_ng_1409": cell(0.0948, 8.0425, 0.3, 2.0),
    # ---- the same for the scan of the gas step: 1215, 1216, 1217 steps
    "scan_gas": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 0.608, 7.0), ("exp", 0.6, 7.0), ("exp", 0.59, 7.0)], zout=20.0),
    # ---- the last computed level within THRESHOLD_DZ of the limit level: dropped, its parts recomputed
    "dropped": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 0.311, 7.0), ("exp", 2.23, 7.0)], a_tronc=A, piz=P, piztr=PT, zout=0.0),
    # ---- the three T_FIRST / T_LAYER regimes of the gas step on both sides of TTOT = 0.02 and 0.5 (adjacent doubles of TGTOT)
    "regimes_gas": cell(0.004, 8.0, 0.002, 2.0, "std", [("norm", 0.013999999494757505, 7.0), ("norm", 0.013999999494757507, 7.0),
                                                        ("norm", 0.49399998882412904, 7.0), ("norm", 0.4939999888241291, 7.0)]),
    # ---- and of the no-gas profile (adjacent doubles of TA)
    "regime_ng_0": cell(0.004, 8.0, 0.015999999494757503, 2.0),
    "regime_ng_1lo": cell(0.004, 8.0, 0.015999999494757507, 2.0),
    "regime_ng_1hi": cell(0.004, 8.0, 0.49599998882412905, 2.0),
    "regime_ng_2": cell(0.004, 8.0, 0.4959999888241291, 2.0),
    # ---- 600 levels: the most the no-gas grid may have (the next double of TA gives 601: refused on the host), and a gas step
    #      that ends on level 600 next to one that needs level 601 (flagged)
    "ng_600": cell(0.0948, 8.0, NG600_TA, 2.0, zout=0.05),
    "gas_600": cell(0.0948, 8.0, 1.0, 1.5, "std", [("exp", 1.312, 7.0), ("exp", 1.332, 7.0)], zout=0.3),
    # ---- strong absorption over a thick aerosol: T_LAYER above TCOUCHE, the clamp not hit
    "no_clamp": cell(0.0948, 8.0, 1.4, 1.5, "std", [("exp", 8.0, 7.0)]),
    # ---- a thin aerosol layer under a weak gas: levels of the gas step that take 26 bisection steps
    "deep_bisect": cell(0.0948, 8.0, 0.8, 0.5, "std", [("exp", 0.3, 7.0)], zout=0.25),
    # ---- level capacity: one level too few (flagged) and just enough, for a weak and for a strong column
    "lp_short": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 0.4, 7.0)], zout=3.2, lp=228),
    "lp_tight": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 0.4, 7.0)], zout=3.2, lp=229),
    "lp_strong_short": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 8.0, 7.0)], lp=311),
    "lp_strong_tight": cell(0.0948, 8.0, 0.3, 2.0, "std", [("exp", 8.0, 7.0)], lp=312),
}
NG601_TA = float(np.nextafter(NG600_TA, 4.0))


def expected_flag(info, lp):
    """Whether sosgpu_profile must flag the bin (nt = -1): the reference's IER = -1 (more than CTE_OS_NT levels), or a level
    array of lp entries that cannot hold the profile -- the level loop may fill indices up to lp - 2 only (the limit level
    comes after it; a loop that reaches lp - 1 is refused even where its last level would then be dropped), and the ground
    level of a strong-absorption bin needs index NT < lp."""
    if info["ier"] != 0:
        return True
    if info["regime"] < 0:
        return False
    return info["nt_loop"] > lp - 1 or (info["strong"] == 1 and info["nt"] >= lp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rule(dev, variants):
    """The identical-or-sensitive rule for one printed row.  dev[k]: the device's values; variants: the same row from the
    oracle's exp modes, the exact one first.  Returns (ok[k], exact[k]): ok = equal, bit for bit, to one of the variants'
    values; exact = equal to the first."""
    d = bits(dev)
    exact = d == bits(variants[0])
    ok = exact.copy()
    for v in variants[1:]:
        ok |= d == bits(v)
    return ok, exact
