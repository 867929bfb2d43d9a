"""Oracle and edge sweep of the per-wavelength context tables: what k_gsf, k_pack, k_pack_ray, k_sv (csrc/noyaux.hip) and
k_pack_ground (csrc/api_operators.hip) build once per wavelength and every solve then reads as given -- prt, mp_aer, mp_vt, mp_uf, sv,
mp_gnd, rdir -- fetched with SosContext.debug_tables (sosgpu_debug_tables).

The bar.  Nothing is compared with a tolerance except two things that have a derived one:
  * the three start values of an order s >= 2 (a*xx**(s/2), b*(1+c*c)*xx**yy, 2*b*c*xx**yy), the one place where the device's
    pow and the host's may differ: distance in ulps (units of the smallest subnormal for subnormal results) from the same
    products of the same doubles evaluated by mpmath at 50 digits, held to the host oracle's own worst distance over this sweep
    plus 2 ulp (a faithful pow instead of a correctly rounded one, and the multiplication after it);
  * the operator-level test, which sums in another order than the reference: gamma_n sum |m_ij x_j|, n = 6N + 4, plus n units
    of the smallest subnormal (every product of the sum may underflow gradually).
Everything else is equality of doubles, entry by entry, no entry excused: prt of every order against the extended oracle run
with the device's own start values; mp_aer, mp_vt, mp_uf, sv, the fetched kernels against the oracle's sums over that prt;
mp_gnd and rdir against the formula of sos_common.h; padding exactly 0.  (+0 and -0 count as equal.)

The unpackers below are written from the layouts documented in sos_common.h and sos_dev.h, not from the kernels.

Measured on an MI355X: start values, host oracle at most 2.337 ulp from mpmath (29 277 values, 53 of them
subnormal), device at most 2.877 ulp (bar 4.337).

Finding of this sweep: the molecular order-1 vectors sv[1], sv[3] multiplied their three factors in another order than
SOS_FSOURCE_ORDRE1 / SOS_FSOURCE_DIFF_FRESNEL1 write them (gamma2*P(0)*R(j) for the reference's gamma2*R(j)*P(0), ...), one ulp
off in 142 of the 738 entries of sv[1] at N = 41 (e.g. -0x1.3a283042a2856p-5 for -0x1.3a283042a2855p-5, Q of s = 1 at
mu = 0.99422754096569); k_sv now follows the reference term by term.
Second finding: k_pack_ground fused the Lambertian term into the BRDF term (its unit, now api_operators.hip, is compiled with contraction on): 31 of
the 240 weighted I<-I entries of gnd_n16 (ro = 0.3, s = 0) were one ulp off the plain evaluation; the kernel now runs with
contraction off.
"""
import functools

import numpy as np
import pytest

MDF = float(np.float32(0.0279))
TINY = 2.0 ** -1074

# ---------------------------------------------------------------------------------------------------------------- the cells


def directions(ng, sun, users=()):
    """Positive half of the 2 ng-point Gauss rule (mu descending) plus zero-weight directions: the sun -- 'first' (above every
    node), 'mid', 'last' (below every node) -- and the user directions, all placed by value.  Returns mu, weights, n0."""
    x, w = np.polynomial.legendre.leggauss(2 * ng)
    mu, wt = x[ng:][::-1].copy(), w[ng:][::-1].copy()
    if sun == "first":
        mus = 0.5 * (mu[0] + 1.0)
    elif sun == "last":
        mus = 0.5 * mu[-1]
    else:
        mus = 0.5 * (mu[ng // 2 - 1] + mu[ng // 2]) if ng > 1 else 0.5 * mu[0]
    extra = sorted([mus] + list(users), reverse=True)
    for v in extra:
        pos = int(np.sum(mu > v))
        mu, wt = np.insert(mu, pos, v), np.insert(wt, pos, 0.0)
    n0 = int(np.where(mu == mus)[0][0]) + 1
    return mu, wt, n0


def user_mus(count, seed):
    """`count` zero-weight user directions, 1.0 and 1 - 1e-9 among them."""
    r = np.random.default_rng(seed)
    return [1.0, 1.0 - 1e-9] + list(np.round(r.uniform(0.05, 0.95, count - 2), 6))


def coefficients(kind, os_nb, seed=0):
    """'hg75' / 'hg95': the synthetic Henyey-Greenstein-like sets; 'random': independent signed ALPHA, BETA, GAMMA, ZETA per l
    (with them the six kernels, the ARR / ATT roles of ALPHA and ZETA and every mirror sign can be told apart)."""
    l = np.arange(os_nb + 1)
    if kind == "random":
        r = np.random.default_rng(1000 + seed)
        return tuple(r.uniform(-1.0, 1.0, os_nb + 1) * (2 * l + 1) * 0.97 ** l for _ in range(4))
    g = dict(hg75=0.75, hg95=0.95)[kind]
    beta = (2 * l + 1) * g ** l
    m = (l >= 2).astype(np.float64)
    return 0.9 * beta * m, beta, -0.08 * beta * m, 0.85 * beta * m


def _cell(ng, sun, os_nb, smax, coef, users=(), ipolar=1, ron=MDF, ifresnel=0, ro=0.0, surf=False, orders=None, seed=0):
    return dict(ng=ng, sun=sun, os_nb=os_nb, smax=smax, coef=coef, users=tuple(users), ipolar=ipolar, ron=ron,
                ifresnel=ifresnel, ro=ro, surf=surf, orders=orders, seed=seed)


BIG_ORDERS = (0, 1, 2, 3, 200, 399, 400)
# user directions whose start values of the orders 399 and 400 are subnormal: a (1 - mu^2)^(s/2) with a = 0.17 falls between
# 1e-323 and 1e-308 for mu between 0.98561 and 0.98791
SUBNORMAL_MUS = (0.9858, 0.9862, 0.9866, 0.987, 0.9874, 0.9878)
CELLS = {
    # name            ng  sun      OS_NB smax
    "n2":       _cell(1, "first", 2, 2, "random"),                                        # nwgt = 1, OS_NB = 2 = iborm_max
    "n3":       _cell(2, "last", 3, 3, "hg75"),                                           # prow >= 0
    "n4":       _cell(3, "last", 24, 2, "hg95"),                                          # prow == 3N: first padding row
    "n5":       _cell(4, "mid", 24, 0, "random"),                                         # cand < 3N; iborm_max 0
    "n16":      _cell(15, "first", 24, 1, "hg95", ipolar=0),                              # 3N = 48: no padding rows; iborm_max 1
    "n20":      _cell(19, "mid", 24, 24, "random", ipolar=0, ifresnel=1, seed=7),         # prow == 3N; Fresnel without polarisation
    "n21":      _cell(20, "mid", 24, 23, "random", ifresnel=1),                           # cand < 3N; iborm_max OS_NB - 1
    "n22":      _cell(20, "mid", 24, 24, "random", users=(1.0,), ifresnel=1, seed=1),     # prow >= 0, mu = 1 exactly
    "n26":      _cell(8, "mid", 24, 2, "random", users=user_mus(17, 26), seed=2),         # ks2h 3 of kh/8 = 10; iborm_max 2
    "n27":      _cell(26, "last", 80, 3, "hg75", ron=0.0),                                # prow >= 0; ron 0
    "n32":      _cell(31, "mid", 24, 24, "hg95"),                                         # 3N = 96: no padding rows
    "n41":      _cell(40, "mid", 80, 80, "hg75"),                                         # the benchmark shape
    "n42":      _cell(40, "mid", 80, 79, "random", users=(1.0 - 1e-9,), seed=3),          # cand < 3N
    "n43":      _cell(40, "mid", 400, 400, "hg95", users=(1.0, 1.0 - 1e-9), ifresnel=1, orders=BIG_ORDERS),
    "n85":      _cell(76, "mid", 400, 400, "random", users=(1.0, 1.0 - 1e-9) + SUBNORMAL_MUS, orders=BIG_ORDERS, seed=4),
    # ground matrices (random REAL*4 with negative entries)
    "gnd_n5":   _cell(4, "mid", 24, 0, "hg75", surf=True),                                # smax 0, ro 0
    "gnd_n16":  _cell(15, "first", 24, 1, "random", ipolar=0, ro=0.3, surf=True, seed=5),
    "gnd_n26":  _cell(8, "mid", 24, 2, "hg75", users=user_mus(17, 27), ro=0.1, surf=True),  # zero-weight heavy
    "gnd_n27":  _cell(26, "last", 24, 3, "random", ro=0.25, ifresnel=1, surf=True, seed=6),
}
# recycling: the donor is created, filled and destroyed; the recipient then gets its block from the pool.  The donor has other
# directions, another N and OS_NB (so its numbers lie where the recipient's never-written entries are) and the larger smax; the
# three contexts are of one size class of the pool (asserted on the device from sosgpu_ctx_bytes).
# name: (recipient cell, recipient smax, donor).  With surface matrices mp_gnd and rdir lie in the same block.
RECYCLE = {"same size": ("n22", 24, _cell(20, "last", 27, 27, "random", seed=9)),
           "smaller": ("n22", 23, _cell(20, "last", 27, 27, "random", seed=9)),
           "ground, same size": ("gnd_n27", 3, _cell(20, "mid", 26, 6, "random", ro=0.4, surf=True, seed=10)),
           "ground, smaller": ("gnd_n27", 2, _cell(20, "mid", 26, 4, "random", ro=0.4, surf=True, seed=11))}


@functools.lru_cache(maxsize=None)
def cell_inputs(name):
    c = CELLS[name]
    mu, wt, n0 = directions(c["ng"], c["sun"], c["users"])
    al, be, ga, ze = coefficients(c["coef"], c["os_nb"], c["seed"])
    rs = None
    if c["surf"]:
        r = np.random.default_rng(77 + c["seed"])
        rs = r.uniform(-0.5, 1.0, (c["smax"] + 1, 9, len(mu), len(mu))).astype(np.float32)
    return dict(mu=mu, wt=wt, n0=n0, coefs=(al, be, ga, ze), rsurf=rs)


def cell_orders(name, smax=None):
    c = CELLS[name]
    smax = c["smax"] if smax is None else smax
    return [s for s in (c["orders"] or range(smax + 1)) if s <= smax]


def layout(n, wt):
    """The layout numbers as sos_common.h documents them."""
    nwgt = int(np.count_nonzero(wt))
    kh = (3 * n + 7) // 8 * 8
    cand = ((3 * n - 1) // 16) * 16 + 12
    order = [c * n + j for p in (0, 1) for c in range(3) for j in range(n) if (wt[j] != 0.0) == (p == 0)]
    return dict(n=n, w=2 * n + 1, kp=(6 * n + 7) // 8 * 8, kh=kh, ks2h=(3 * nwgt + 7) // 8, rtph=(kh + 15) // 16, nwgt=nwgt,
                prow=cand if cand >= 3 * n else -1, rowmap=np.array(order + [-1] * (kh - 3 * n), dtype=np.int32))


# ------------------------------------------------------------------------------------------------------------ the unpackers


def unpack_a16(p, tiles, ks2h):
    """A operand of v_mfma_f64_16x16x4_f64 (sos_common.h): p[((rt*KS2H + m)*64 + lane)*2 + e] = M[rt*16 + (lane&15)][8m +
    2(lane>>4) + e].  Returns M [tiles*16][ks2h*8]."""
    rt, m, lane, e = np.meshgrid(np.arange(tiles), np.arange(ks2h), np.arange(64), np.arange(2), indexing="ij")
    out = np.zeros((tiles * 16, ks2h * 8), dtype=np.asarray(p).dtype)
    out[rt * 16 + (lane & 15), 8 * m + 2 * (lane >> 4) + e] = np.asarray(p).reshape(tiles, ks2h, 64, 2)
    return out


def unpack_a4(p, tiles, ks2h):
    """A operand of v_mfma_f64_4x4x4f64 (sos_dev.h ground_mfma): p[((tile*KS2H + m)*64 + lane)*2 + e] = G[tile*16 +
    4((lane>>2)&3) + (lane&3)][8m + 4e + (lane>>4)]."""
    rt, m, lane, e = np.meshgrid(np.arange(tiles), np.arange(ks2h), np.arange(64), np.arange(2), indexing="ij")
    out = np.zeros((tiles * 16, ks2h * 8), dtype=np.asarray(p).dtype)
    out[rt * 16 + 4 * ((lane >> 2) & 3) + (lane & 3), 8 * m + 4 * e + (lane >> 4)] = np.asarray(p).reshape(tiles, ks2h, 64, 2)
    return out


def unpack_uf(p, tiles):
    """uf[rt*64 + lane] = U[rt*16 + (lane&15)][lane>>4] (noyaux.hip k_pack_ray).  Returns U [tiles*16][4]."""
    rt, lane = np.meshgrid(np.arange(tiles), np.arange(64), indexing="ij")
    out = np.zeros((tiles * 16, 4), dtype=np.asarray(p).dtype)
    out[rt * 16 + (lane & 15), lane >> 4] = np.asarray(p).reshape(tiles, 64)
    return out


def _same(a, b):
    """Equality of doubles entry by entry (+0 == -0), nothing non-finite."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.isfinite(a))) and bool(np.all(a == b))


# ------------------------------------------------------------------------------------- the expected tables, restated in numpy


def fresnel_sun(mus, ind, ipolar):
    """F11, F12 of SOS_MAT_FRESNEL_PLAN_REFL at the solar incidence (SOS_OS.F:1753-1780)."""
    ind2, mu2 = ind * ind, mus * mus
    x = np.sqrt(ind2 - 1.0 + mu2)
    rl = (ind2 * mus - x) / (ind2 * mus + x)
    rr = (mus - x) / (mus + x)
    return (rl * rl + rr * rr) / 2., ((rl * rl - rr * rr) / 2. if ipolar else 0.)


# (component of the row, component of the column) -> kernel, (a, b) = (j, k) or (k, j), minus form, negated: the table of the
# half_element comment in noyaux.hip
HALF = {(0, 0): ("BP", "jk", False, False), (0, 1): ("GR", "kj", False, False), (0, 2): ("GT", "kj", True, True),
        (1, 0): ("GR", "jk", False, False), (1, 1): ("ARR", "jk", False, False), (1, 2): ("ART", "jk", False, True),
        (2, 0): ("GT", "jk", True, True), (2, 1): ("ART", "kj", False, True), (2, 2): ("ATT", "jk", True, False)}


def expected_half(kern, lay, wt, sysm):
    """M^sys [3N][3N] in half-system order: 0.25 w_j (X(a,b) +- X(a,-b)), same operation order as the kernel."""
    n, h = lay["n"], 3 * lay["n"]
    rm = lay["rowmap"][:h]
    co, k = rm // n, rm % n + 1
    sg = -1.0 if sysm else 1.0
    out = np.zeros((h, h))
    for (rc, cc), (x, ab, mns, neg) in HALF.items():
        rows, cols = np.where(co == rc)[0], np.where(co == cc)[0]
        kk, jj = np.meshgrid(k[rows], k[cols], indexing="ij")
        a, b = (jj, kk) if ab == "jk" else (kk, jj)
        same, opp = kern[x][a + n, b + n], kern[x][a + n, -b + n]
        v = same - sg * opp if mns else same + sg * opp
        if neg:
            v = -v
        out[np.ix_(rows, cols)] = 0.25 * wt[jj - 1] * v
    return out


def expected_vt(p2, r2, t2, lay, wt, s, b2g2a2):
    """V^T [4][3N] of the molecular operator (noyaux.hip k_pack_ray): w/2 (b2 P, g2 R, -g2 T), (g2 P, a2 R, -a2 T),
    (-g2 P, -a2 R, a2 T), (b0, 0, 0), half-system column order."""
    n, h = lay["n"], 3 * lay["n"]
    b2, g2, a2 = b2g2a2
    rm = lay["rowmap"][:h]
    ci, j = rm // n, rm % n + 1
    hw = 0.5 * wt[j - 1]
    f = np.where(ci == 0, p2[j + n], np.where(ci == 1, r2[j + n], t2[j + n]))
    c = np.array([[b2, g2, -g2], [g2, a2, -a2], [-g2, -a2, a2]])
    out = np.zeros((4, h))
    for r in range(3):
        out[r] = hw * c[r][ci] * f
    out[3] = np.where(ci == 0, hw * (1.0 if s == 0 else 0.0), 0.0)
    return out


def expected_uf(p2, r2, t2, lay, s):
    n, h = lay["n"], 3 * lay["n"]
    rm = lay["rowmap"][:h]
    co, k = rm // n, rm % n + 1
    out = np.zeros((h, 4))
    out[co == 0, 0] = p2[k[co == 0] + n]
    out[co == 0, 3] = 1.0 if s == 0 else 0.0
    out[co == 1, 1] = r2[k[co == 1] + n]
    out[co == 2, 2] = t2[k[co == 2] + n]
    return out


def state_rows(vec3, n):
    """[3][W] over jj = -N..N -> the 6N state order of sos_common.h: r = c*2N + d, d < N: +(d+1), d >= N: -(d-N+1)."""
    jj = np.concatenate([np.arange(1, n + 1), -np.arange(1, n + 1)])
    return np.concatenate([vec3[c][jj + n] for c in range(3)])


def expected_ground(rs, lay, mu, wt, n0, ro, ipolar):
    """G_s [3N][3N] (half-system order) and rdir [smax+1][3][N] as sos_common.h states them."""
    n, h = lay["n"], 3 * lay["n"]
    rm = lay["rowmap"][:h]
    shape = (h, h)
    cc, kk = np.broadcast_to((rm // n)[:, None], shape), np.broadcast_to((rm % n)[:, None], shape)      # row (c, k)
    bb, jj = np.broadcast_to((rm // n)[None, :], shape), np.broadcast_to((rm % n)[None, :], shape)      # column (b, j)
    g = np.zeros((rs.shape[0], h, h))
    rd = np.zeros((rs.shape[0], 3, n))
    for s in range(rs.shape[0]):
        r4 = rs[s].reshape(3, 3, n, n).astype(np.float64)          # [c][b][k][j] = R_cb(I = j, J = k)
        x = r4[cc, bb, kk, jj]
        if not ipolar:
            x = np.where((cc != 0) | (bb != 0), 0.0, x)
        v = (2. / mu[kk]) * wt[jj] * x
        if s == 0 and ro != 0.0:
            v = np.where((cc == 0) & (bb == 0), v + 2. * ro * wt[jj] * mu[jj], v)
        g[s] = v
        rd[s] = r4[:, 0, :, n0 - 1]
        if not ipolar:
            rd[s, 1:] = 0.0
    return g, rd


# --------------------------------------------------------------------------------------------------- start values and mpmath


def start_factors(s, c):
    """a, b, xx, yy of SOS_OS.F:2027-2046 for the directions c: sqrt, divide and multiply only, the same doubles on every
    IEEE machine."""
    a = 1.
    for i in range(1, s + 1):
        a = a * np.sqrt((i + s) / float(i)) * 0.5
    b = a * np.sqrt(s / (s + 1.0)) * np.sqrt((s - 1.0) / (s + 2.))
    c = np.asarray(c, dtype=np.float64)
    return a, b, 1. - c * c, s * 0.5 - 1.


def start_exact(s, c):
    """The three start expressions from the doubles a, b, c, xx with mpmath at 50 digits: [3][len(c)] mpf."""
    import mpmath
    a, b, xx, yy = start_factors(s, c)
    with mpmath.workdps(50):
        out = [[], [], []]
        for cj, xj in zip(np.asarray(c, dtype=np.float64), xx):
            cm, xm = mpmath.mpf(float(cj)), mpmath.mpf(float(xj))
            pw = xm ** mpmath.mpf(yy)
            out[0].append(mpmath.mpf(a) * xm ** (mpmath.mpf(s) / 2))
            out[1].append(mpmath.mpf(b) * (1 + cm * cm) * pw)
            out[2].append(2 * mpmath.mpf(b) * cm * pw)
    return out


def ulp_distance(got, exact):
    """max |got - exact| in units of the spacing of doubles at exact (the smallest subnormal below the normal range)."""
    import mpmath
    worst = 0.0
    with mpmath.workdps(50):
        for g, e in zip(np.ravel(got), [x for row in exact for x in row]):
            assert np.isfinite(g)
            unit = float(np.spacing(abs(float(e))))
            worst = max(worst, float(abs(mpmath.mpf(float(g)) - e) / mpmath.mpf(unit)))
    return worst


def start_orders(name):
    return [s for s in cell_orders(name) if s >= 2]


def _dirs0(name):
    i = cell_inputs(name)
    return np.concatenate([[-i["mu"][i["n0"] - 1]], i["mu"]])          # j = 0 (RMU(0) = -mus), 1..N


@functools.lru_cache(maxsize=None)
def oracle_start_distance():
    """Worst distance of the host oracle's start values from mpmath over every (cell, checked order >= 2, direction)."""
    from oracle import oracle_ctypes as O
    worst, count, subn = 0.0, 0, 0
    for name in CELLS:
        i, c = cell_inputs(name), CELLS[name]
        n = len(i["mu"])
        for s in start_orders(name):
            r = O.noyaux_ext(s, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"], kernels=False)
            got = np.stack([r[k][s, n:] for k in ("PSL", "RSL", "TSL")])
            worst = max(worst, ulp_distance(got, start_exact(s, _dirs0(name))))
            count += got.size
            subn += int(np.count_nonzero((got != 0) & (np.abs(got) < 2.0 ** -1022)))
    return worst, count, subn


# --------------------------------------------------------------------------------------------------------------- CPU tests


def test_extended_oracle_is_the_old_one(oracle):
    """Without the override the extended form is sos_oracle_noyaux bit for bit, and both reproduce noyaux_n13.npz."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noyaux_n13.npz"))
    for name in ("n3", "n22", "n26", "n41"):
        i, c = cell_inputs(name), CELLS[name]
        for s in cell_orders(name)[::7] + [c["smax"]]:
            a = oracle.noyaux(s, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"])
            b = oracle.noyaux_ext(s, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"])
            for k in a:
                assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), (name, s, k)
            assert _same(b["PSL"][2], b["XPL"]) and _same(b["RSL"][2], b["XRL"]) and _same(b["TSL"][2], b["XTL"])
            if s >= 2:                                   # the override with the function's own values changes nothing
                n = len(i["mu"])
                st = np.stack([b[k][s, n:] for k in ("PSL", "RSL", "TSL")])
                d = oracle.noyaux_ext(s, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"], start=st)
                assert all(np.array_equal(b[k].view(np.int64), d[k].view(np.int64)) for k in b), (name, s)
                st[0] *= 2.0                             # ... and another one is really taken
                e = oracle.noyaux_ext(s, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"], start=st, kernels=False)
                assert _same(e["PSL"][s:], 2.0 * b["PSL"][s:]) and _same(e["RSL"], b["RSL"])
    mu, n0 = g["mu"], int(g["n0"])
    for s in (0, 1, 2, 3, 12, 24):
        r = oracle.noyaux_ext(s, -mu[n0 - 1], mu, 24, g["alpha"], g["beta"], g["gamma"], g["zeta"])
        for k in ("BP", "GR", "GT", "ARR", "ART", "ATT", "XPL", "XRL", "XTL"):
            ref = g["is%d_%s" % (s, k)]
            assert np.abs(r[k] - ref).max() <= 1e-13 * (np.abs(ref).max() + 1e-300), (s, k)


def test_oracle_pieces_agree_with_each_other(oracle):
    """The exported pieces against one another: the single-level source sum applied to unit fields returns the kernels it was
    given (times w_j / 2), and the order-1 coefficients are the 0-row of the kernels."""
    name = "n5"
    i, c = cell_inputs(name), CELLS[name]
    n, wt = len(i["mu"]), i["wt"]
    bga = oracle.ray_coefs(c["ron"], 1)
    assert bga[0] > 0 > bga[1] and oracle.ray_coefs(c["ron"], 0)[1:] == (0.0, 0.0)
    for s in (0, 1, 2, 3):
        k = oracle.noyaux_ext(s, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"])
        rk = oracle.ray_kernels(s, k, bga)
        aer, ray = oracle.order1_coefs(s, k, bga)
        assert _same(aer[0], k["BP"][n]) and _same(aer[1], k["GR"][n]) and _same(aer[2], -k["GT"][n])
        assert _same(ray[1][n + 1:], bga[1] * k["XRL"][n + 1:] * k["XPL"][n]) or s > 2
        assert (s > 2) == (not np.any(rk["BP"])) and (s > 2) == (not np.any(ray))
        j = 2                                              # weighted direction +j carries a unit I
        assert wt[j - 1] != 0
        f = np.zeros((3, 2 * n + 1))
        f[0, n + j] = 1.0
        a, r = oracle.ordreig_level(s, wt, k, bga, f)
        kk = np.arange(1, n + 1)
        assert _same(a[0][n + kk], wt[j - 1] * k["BP"][n + j, n + kk] * 0.5)
        assert _same(a[1][n - kk], wt[j - 1] * k["GR"][n + j, n - kk] * 0.5)
        assert _same(r[0][n + kk], wt[j - 1] * rk["BP"][n + j, n + kk] * 0.5)
        fa, fr = oracle.fresnel1_coefs(s, k, bga, 0.25, -0.125)
        # the re-typed expressions of fresnel1_coefs are those of the routine itself (its COEFK = 1/4 is exact on these values)
        assert _same(0.25 * fa, oracle.fresnel1_routine(s, k, bga, 0.25, -0.125, 1.0, 0.0))
        assert _same(0.25 * fr, oracle.fresnel1_routine(s, k, bga, 0.25, -0.125, 0.0, 1.0))
        assert _same(fa[0][n + kk], 0.25 * k["BP"][n, n - kk] + -0.125 * k["GR"][n - kk, n])
        assert _same(fr[2][n - kk], 0.25 * rk["GT"][n, n + kk] + -0.125 * rk["ART"][n + kk, n])


def test_start_values_of_the_oracle_against_mpmath():
    """The measurement the device's bar is built on: runs, is not skipped, and is small."""
    pytest.importorskip("mpmath")
    worst, count, subn = oracle_start_distance()
    print("oracle start values: %d compared, %d subnormal, worst distance %.3f ulp" % (count, subn, worst))
    assert count > 20000 and subn >= 18        # the six SUBNORMAL_MUS, three values each
    assert worst <= 4.0          # two roundings and glibc's pow: were this larger the bar below would mean little


def test_unpackers_round_trip_a_synthetic_matrix():
    """Element by element with the documented index formulas, against the vectorised unpackers."""
    tiles, ks2h = 3, 5
    m = np.arange(tiles * 16 * ks2h * 8, dtype=np.float64).reshape(tiles * 16, ks2h * 8) + 1
    p16, p4 = np.zeros(tiles * ks2h * 128), np.zeros(tiles * ks2h * 128)
    for rt in range(tiles):
        for mm in range(ks2h):
            for lane in range(64):
                for e in range(2):
                    o = ((rt * ks2h + mm) * 64 + lane) * 2 + e
                    p16[o] = m[rt * 16 + (lane & 15), 8 * mm + 2 * (lane >> 4) + e]
                    p4[o] = m[rt * 16 + 4 * ((lane >> 2) & 3) + (lane & 3), 8 * mm + 4 * e + (lane >> 4)]
    assert np.array_equal(unpack_a16(p16, tiles, ks2h), m) and np.array_equal(unpack_a4(p4, tiles, ks2h), m)
    assert not np.array_equal(unpack_a4(p16, tiles, ks2h), m)          # the two orders do differ
    u = np.arange(tiles * 64, dtype=np.float64).reshape(tiles * 16, 4) + 1
    pu = np.zeros(tiles * 64)
    for rt in range(tiles):
        for lane in range(64):
            pu[rt * 64 + lane] = u[rt * 16 + (lane & 15), lane >> 4]
    assert np.array_equal(unpack_uf(pu, tiles), u)


def test_table_covers_the_edges_it_claims():
    L = {k: layout(len(cell_inputs(k)["mu"]), cell_inputs(k)["wt"]) for k in CELLS}
    ns = {k: v["n"] for k, v in L.items()}
    assert {ns[k] for k in CELLS if not CELLS[k]["surf"]} == {2, 3, 4, 5, 16, 20, 21, 22, 26, 27, 32, 41, 42, 43, 85}
    for k, v in L.items():
        n = v["n"]
        if n in (16, 32):
            assert 3 * n % 16 == 0 and v["prow"] == -1 and v["kh"] == 3 * n
        elif n in (5, 21, 26, 42, 85):
            assert v["prow"] == -1 and v["rtph"] * 16 > 3 * n
        elif n in (4, 20):                                              # the boundary: > for >= in the choice of prow shows here
            assert v["prow"] == 3 * n
        elif n in (3, 22, 27, 43):
            assert v["prow"] > 3 * n and v["prow"] + 4 <= v["rtph"] * 16 and v["prow"] % 4 == 0
    assert L["n2"]["nwgt"] == 1 and L["n2"]["n"] == 2
    for k in ("n26", "gnd_n26"):
        assert L[k]["ks2h"] == 3 and L[k]["kh"] // 8 == 10
    # position of the solar direction, alone at weight 0
    alone = {k: cell_inputs(k)["n0"] for k in CELLS if np.count_nonzero(cell_inputs(k)["wt"] == 0) == 1}
    assert {1} <= {v for v in alone.values()} and any(alone[k] == ns[k] for k in alone)
    assert any(1 < alone[k] < ns[k] for k in alone)
    gnd = [k for k in CELLS if CELLS[k]["surf"]]
    assert {1} <= {cell_inputs(k)["n0"] for k in gnd} and any(cell_inputs(k)["n0"] == ns[k] for k in gnd)
    assert any(1 < cell_inputs(k)["n0"] < ns[k] for k in gnd)
    # user directions at mu = 1 exactly and 1 - 1e-9, also with the highest orders
    for k in ("n43", "n85", "n26"):
        assert 1.0 in cell_inputs(k)["mu"] and 1.0 - 1e-9 in cell_inputs(k)["mu"]
    assert cell_inputs("n22")["mu"][0] == 1.0 and cell_inputs("n42")["mu"][0] == 1.0 - 1e-9
    assert {CELLS[k]["os_nb"] for k in CELLS} == {2, 3, 24, 80, 400}
    im = {(CELLS[k]["smax"], CELLS[k]["os_nb"]) for k in CELLS}
    assert {0, 1, 2, 3} <= {s for s, _ in im} and any(s == b - 1 for s, b in im) and any(s == b for s, b in im)
    assert {s for s, b in im if s < 2} == {0, 1}                        # the k_pack_ray grid shrinks
    for k in ("n43", "n85"):
        assert set(cell_orders(k)) == {0, 1, 2, 3, 200, 399, 400}
    assert {CELLS[k]["coef"] for k in CELLS} == {"hg75", "hg95", "random"}
    al, be, ga, ze = coefficients("random", 24)
    assert all(np.any(x < 0) and np.any(x > 0) for x in (al, be, ga, ze)) and not np.allclose(al / be, ze / be)
    assert {CELLS[k]["ipolar"] for k in CELLS} == {0, 1} and {CELLS[k]["ifresnel"] for k in CELLS} == {0, 1}
    assert any(CELLS[k]["ipolar"] == 0 and CELLS[k]["ifresnel"] == 1 for k in CELLS)      # the f12sun cut
    assert 0.0 in {CELLS[k]["ron"] for k in CELLS} and MDF in {CELLS[k]["ron"] for k in CELLS}
    assert {CELLS[k]["ro"] == 0 for k in gnd} == {True, False} and {CELLS[k]["ipolar"] for k in gnd} == {0, 1}
    assert {CELLS[k]["smax"] == 0 for k in gnd} == {True, False}
    assert all(np.any(cell_inputs(k)["rsurf"] < 0) for k in gnd)
    for surf in (False, True):
        rec = [(k, s, d) for k, s, d in RECYCLE.values() if CELLS[k]["surf"] == surf]
        assert {CELLS[k]["smax"] - s for k, s, _ in rec} == {0, 1}
        for k, s, d in rec:                          # the donor: larger smax, another N and OS_NB, surface matrices alike
            assert d["smax"] > s and d["ng"] + 1 != ns[k] and d["os_nb"] != CELLS[k]["os_nb"] and d["surf"] == surf


def test_subnormal_start_values_are_in_the_sweep(oracle):
    """Orders 399 and 400 with a direction at 1 - 1e-9 give subnormal and zero start values (and mu = 1 gives pow(0, 0))."""
    i, c = cell_inputs("n85"), CELLS["n85"]
    n = len(i["mu"])
    r = oracle.noyaux_ext(399, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"], kernels=False)
    a = np.concatenate([r[k].ravel() for k in ("PSL", "RSL", "TSL")])
    assert np.all(np.isfinite(a)) and np.count_nonzero((a != 0) & (np.abs(a) < 2.0 ** -1022)) >= 36
    r = oracle.noyaux_ext(2, -i["mu"][i["n0"] - 1], i["mu"], c["os_nb"], *i["coefs"], kernels=False)
    assert i["mu"][0] == 1.0 and r["PSL"][2, n + 1] == 0.0 and r["RSL"][2, n + 1] != 0.0 and r["TSL"][2, n + 1] != 0.0


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def _context(gpu_pkg, name, smax=None, coefs=None, sync_surface=False):
    c, i = CELLS[name], cell_inputs(name)
    al, be, ga, ze = coefs or i["coefs"]
    smax = c["smax"] if smax is None else smax
    rs = None if i["rsurf"] is None else i["rsurf"][:smax + 1]
    return gpu_pkg.SosContext(i["mu"], i["wt"], i["n0"], al, be, ga, ze, iborm_max=smax, ro=c["ro"],
                              imat_surf=1 if c["surf"] else 0, ifresnel=c["ifresnel"], ind_surf=1.34, ron=c["ron"],
                              ipolar=c["ipolar"], rsurf=rs)


def check_tables(oracle, cx, name, smax=None, coefs=None):
    """Every assertion of the module's header on the tables of one context.  Returns counts and the start-value distance."""
    c, i = CELLS[name], cell_inputs(name)
    smax = c["smax"] if smax is None else smax
    mu, wt, n0 = i["mu"], i["wt"], i["n0"]
    al, be, ga, ze = coefs or i["coefs"]
    if not c["ipolar"]:                                                  # SOS_OS.F:689-699
        al, ga, ze = np.zeros_like(al), np.zeros_like(ga), np.zeros_like(ze)
    n, w, B = len(mu), 2 * len(mu) + 1, c["os_nb"]
    h = 3 * n
    t = cx.debug_tables()
    lay = layout(n, wt)
    cnt = dict(prt=0, start=0, mp_aer=0, ray=0, sv=0, fetch=0, operator=0, ground=0)

    # --- layout numbers and scalars
    for k in ("n", "w", "kp", "kh", "ks2h", "rtph", "nwgt", "prow"):
        assert t[k] == lay[k], (name, k, t[k], lay[k])
    assert (t["os_nb"], t["smax"], t["n0"], t["ipolar"]) == (B, smax, n0, c["ipolar"])
    assert np.array_equal(t["rowmap"], lay["rowmap"]), name
    bga = oracle.ray_coefs(c["ron"], c["ipolar"])
    assert (t["beta2"], t["gamma2"], t["alpha2"]) == bga and t["mus"] == mu[n0 - 1] and t["ro"] == c["ro"]
    f11, f12 = fresnel_sun(mu[n0 - 1], 1.34, c["ipolar"]) if c["ifresnel"] else (0.0, 0.0)
    assert (t["f11sun"], t["f12sun"]) == (f11, f12), name
    tiles, ks2h, kp = lay["rtph"], lay["ks2h"], lay["kp"]
    ncol = min(h, ks2h * 8)
    zero_w = wt[lay["rowmap"][:ncol] % n] == 0.0                         # columns of zero-weight directions

    # --- prt: zeros below the start order, the recurrence from the device's own start values, the start values
    dist, orc = 0.0, {}
    checked = set(cell_orders(name, smax))
    for s in range(smax + 1):
        dev = t["prt"][s]                                               # [3][B+1][W]
        st = None
        if s >= 2:
            assert not np.any(dev[:, :s, :]), (name, s, "prt below the start order")
            st = dev[:, s, n:].copy()
        r = oracle.noyaux_ext(s, -mu[n0 - 1], mu, B, al, be, ga, ze, start=st, kernels=s in checked)
        for q, k in enumerate(("PSL", "RSL", "TSL")):
            assert _same(dev[q], r[k]), (name, s, k, int(np.count_nonzero(dev[q] != r[k])))
        cnt["prt"] += dev.size
        if s in checked:
            orc[s] = r
            if s >= 2:
                dist = max(dist, ulp_distance(st, start_exact(s, _dirs0(name))))
                cnt["start"] += st.size
    if smax >= 2 and cnt["start"]:
        bar = oracle_start_distance()[0] + 2.0
        print("%s: start values %d compared, device at most %.3f ulp from mpmath (bar %.3f)" % (name, cnt["start"], dist, bar))
        assert dist <= bar, (name, dist, bar)

    rng = np.random.default_rng(4242)
    gam = lambda m: m * 2.0 ** -53 / (1 - m * 2.0 ** -53)
    gc = np.array([1.0, 1.0, -1.0])
    for s in sorted(checked):
        k = orc[s]
        p2, r2, t2 = k["XPL"], k["XRL"], k["XTL"]
        # --- mp_aer: in-range elements, padding, projection rows, zero-weight columns
        exp_vt = expected_vt(p2, r2, t2, lay, wt, s, bga)
        halves = []
        for sysm in (0, 1):
            m = unpack_a16(t["mp_aer"][s, sysm], tiles, ks2h)
            exp = np.zeros_like(m)
            exp[:h, :ncol] = expected_half(k, lay, wt, sysm)[:, :ncol]
            if lay["prow"] >= 0 and s <= 2 and sysm == (s & 1):
                exp[lay["prow"]:lay["prow"] + 4, :ncol] = exp_vt[:, :ncol]
            assert _same(m, exp), (name, s, sysm, "mp_aer", int(np.count_nonzero(m != exp)))
            assert not np.any(m[:h, :ncol][:, zero_w]), (name, s, sysm, "zero-weight columns")
            cnt["mp_aer"] += m.size
            halves.append(m[:h, :ncol].astype(np.longdouble))
        # --- mp_vt, mp_uf
        if s <= 2:
            vt, uf = unpack_a16(t["mp_vt"][s], 1, ks2h), unpack_uf(t["mp_uf"][s], tiles)
            ev, eu = np.zeros_like(vt), np.zeros_like(uf)
            ev[:4, :ncol] = exp_vt[:, :ncol]
            eu[:h] = expected_uf(p2, r2, t2, lay, s)
            assert _same(vt, ev) and _same(uf, eu), (name, s, "mp_vt / mp_uf")
            cnt["ray"] += vt.size + uf.size
        # --- sv
        o1a, o1r = oracle.order1_coefs(s, k, bga)
        f1a, f1r = oracle.fresnel1_coefs(s, k, bga, f11, f12)
        for q, (what, e3) in enumerate((("aer", o1a), ("ray", o1r), ("fresnel aer", f1a), ("fresnel ray", f1r))):
            exp = np.zeros(kp)
            exp[:6 * n] = state_rows(e3, n)
            assert _same(t["sv"][s, q], exp), (name, s, "sv", what, int(np.count_nonzero(t["sv"][s, q] != exp)))
        if s > 2:
            assert not np.any(t["sv"][s, 1]) and not np.any(t["sv"][s, 3]), (name, s)
        cnt["sv"] += 4 * kp
        # --- k_noyaux_fetch: what the same prt implies
        got = cx.noyaux_fetch(s)
        for x in oracle.KERNEL_NAMES + ("XPL", "XRL", "XTL"):
            assert _same(got[x], k[x]), (name, s, "fetch", x)
            cnt["fetch"] += got[x].size
        # --- operator level: recombined systems on a random field against the reference's dense sum
        rm = lay["rowmap"][:h]
        comp, jd = rm // n, rm % n + 1                                    # half-system position -> (c, direction)
        A, Bm = halves
        ray = np.zeros((h, ncol), dtype=np.longdouble)
        if s <= 2:
            ray = unpack_uf(t["mp_uf"][s], tiles)[:h].astype(np.longdouble) @ \
                unpack_a16(t["mp_vt"][s], 1, ks2h)[:4, :ncol].astype(np.longdouble)
        zero = np.zeros_like(ray)
        field = rng.uniform(-1.0, 1.0, (3, w))
        xp, xm = field[comp[:ncol], n + jd[:ncol]], field[comp[:ncol], n - jd[:ncol]]
        gcol, grow = gc[comp[:ncol]], gc[comp]
        for part, (MA, MB), ref in (("aer", (A, Bm), 0), ("ray", (zero, ray) if s & 1 else (ray, zero), 1)):
            # S(+mu) = E^A + E^B, S(-mu) = g_c (E^A - E^B) with X^A = X(+) + g X(-), X^B = X(+) - g X(-)   (sos_common.h)
            cpp, cpm = MA + MB, (MA - MB) * gcol                         # coefficients of X(+j), X(-j) in S(+k)
            up = cpp @ xp + cpm @ xm
            dn = (((cpm * gcol) @ xp) + ((cpp * gcol) @ xm)) * grow      # ((MA - MB) X+ + g (MA + MB) X-) g_row
            mags = (np.abs(cpp) @ np.abs(xp) + np.abs(cpm) @ np.abs(xm), np.abs(cpm) @ np.abs(xp) + np.abs(cpp) @ np.abs(xm))
            want = oracle.ordreig_level(s, wt, k, bga, field)[ref]
            for sign, val, mag in ((1, up, mags[0]), (-1, dn, mags[1])):
                bound = (gam(6 * n + 4) * mag).astype(np.float64) + (6 * n + 4) * TINY
                w3 = want[comp, n + sign * jd]
                err = np.abs(val - w3.astype(np.longdouble)).astype(np.float64)
                assert np.all(err <= bound), (name, s, part, sign, float(np.max(err / bound)))
                cnt["operator"] += err.size

    # --- orders above smax of the molecular factors (smax < 2) stay cleared
    for s in range(smax + 1, 3):
        assert not np.any(t["mp_vt"][s]) and not np.any(t["mp_uf"][s]), (name, s)
        cnt["ray"] += t["mp_vt"][s].size + t["mp_uf"][s].size

    # --- ground operator
    if c["surf"]:
        g, rd = expected_ground(i["rsurf"][:smax + 1], lay, mu, wt, n0, c["ro"], c["ipolar"])
        for s in range(smax + 1):
            m = unpack_a4(t["mp_gnd"][s], tiles, ks2h)
            exp = np.zeros_like(m)
            exp[:h, :ncol] = g[s][:, :ncol]
            assert _same(m, exp), (name, s, "mp_gnd", int(np.count_nonzero(m != exp)))
            cnt["ground"] += m.size
        assert _same(t["rdir"], rd), (name, "rdir")
        cnt["ground"] += rd.size
    return cnt, dist, t


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CELLS))
def test_tables_vs_oracle(gpu_pkg, oracle, name):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    cx = _context(gpu_pkg, name)
    try:
        cnt, dist, t = check_tables(oracle, cx, name)
        if CELLS[name]["surf"]:                                          # the synchronous form packs the same bits
            import ctypes as C
            r = cx._rsurf
            gpu_pkg.capi.check(gpu_pkg.capi.lib().sosgpu_set_surface_matrices(cx._h, C.c_void_p(r.data_ptr())),
                               "sosgpu_set_surface_matrices")
            t2 = cx.debug_tables()
            for k in ("mp_gnd", "rdir"):
                assert np.array_equal(t[k].view(np.int64), t2[k].view(np.int64)), (name, k)
    finally:
        cx.close()
    print(name, "entries compared:", cnt, "start distance %.3f ulp" % dist)


def _size_class(nbytes):
    """Size classes of the table pool (api_mem.hip): 256 B steps up to 4 KiB, then eighths of the leading power of two."""
    if nbytes <= 4096:
        return (max(nbytes, 1) + 255) // 256 * 256
    step = (1 << (nbytes.bit_length() - 1)) >> 3
    return (nbytes + step - 1) // step * step


def _unbuilt_tables(gpu_pkg, name, smax):
    """prt, mp_aer and sv of a context of the cell's shape that was only created (sosgpu_create): nothing has written them,
    so they show what the block held before.  The context is destroyed again."""
    import ctypes as C
    capi = gpu_pkg.capi
    L, c, i = capi.lib(), CELLS[name], cell_inputs(name)
    ins = [np.ascontiguousarray(x, dtype=np.float64) for x in (i["mu"], i["wt"]) + tuple(i["coefs"])]
    wv = capi.Wave(n=len(i["mu"]), os_nb=c["os_nb"], n0=i["n0"], imat_surf=1 if c["surf"] else 0, ifresnel=c["ifresnel"],
                   ipolar=c["ipolar"], igmax=100, reserved=0, ro=c["ro"], ind_surf=1.34, ron=c["ron"])
    h = C.c_void_p()
    capi.check(L.sosgpu_create(C.byref(h), 0, C.byref(wv), *[x.ctypes.data_as(C.c_void_p) for x in ins], smax), "sosgpu_create")
    try:
        info = capi.TablesInfo()
        capi.check(L.sosgpu_debug_tables(h, C.byref(info), *([None] * 8)), "sosgpu_debug_tables")
        per = info.rtph * info.ks2h * 128
        prt = np.zeros((smax + 1, 3, info.os_nb + 1, info.w))
        aer, sv = np.zeros((smax + 1, 2, per)), np.zeros((smax + 1, 4, info.kp))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(L.sosgpu_debug_tables(h, C.byref(info), p(prt), p(aer), None, None, p(sv), None, None, None),
                   "sosgpu_debug_tables")
        return dict(prt=prt, mp_aer=aer, sv=sv, bytes=L.sosgpu_ctx_bytes(h), rtph=info.rtph, ks2h=info.ks2h, kp=info.kp)
    finally:
        L.sosgpu_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(RECYCLE))
def test_tables_on_a_recycled_block(gpu_pkg, oracle, which):
    """A context with other inputs and the larger smax is created, filled and destroyed; the next context of the same size
    class gets its block back from the pool with only [mp_vt | mp_uf] cleared.  That it does is shown first: a context of the
    recipient's shape that is created and not built finds the donor's numbers under the entries that must become 0.  Every
    assertion then holds on the recipient."""
    name, smax, d = RECYCLE[which]
    L = gpu_pkg.capi.lib()
    L.sosgpu_trim()
    dmu, dwt, dn0 = directions(d["ng"], d["sun"])
    rs = None
    if d["surf"]:
        rs = np.random.default_rng(d["seed"]).uniform(-5.0, 5.0, (d["smax"] + 1, 9, len(dmu), len(dmu))).astype(np.float32)
    donor = gpu_pkg.SosContext(dmu, dwt, dn0, *[1e3 * x for x in coefficients("random", d["os_nb"], d["seed"])],
                               iborm_max=d["smax"], ro=d["ro"], imat_surf=1 if d["surf"] else 0, rsurf=rs)
    td = donor.debug_tables()
    assert np.any(td["mp_aer"] != 0) and np.any(td["prt"] != 0) and np.any(td["sv"] != 0)
    assert not d["surf"] or (np.any(td["mp_gnd"] != 0) and np.any(td["rdir"] != 0))
    cls = _size_class(L.sosgpu_ctx_bytes(donor._h))
    donor.close()
    u = _unbuilt_tables(gpu_pkg, name, smax)
    assert _size_class(u["bytes"]) == cls, "the recipient must be of the donor's size class"
    n = len(cell_inputs(name)["mu"])
    if smax >= 2:
        assert np.any(u["prt"][smax, :, :smax, :] != 0), "no donor data under prt below the start order"
    pad = unpack_a16(u["mp_aer"][smax, 0], u["rtph"], u["ks2h"])[3 * n:]
    assert pad.size == 0 or np.any(pad != 0), "no donor data under the padding rows of mp_aer"
    cx = _context(gpu_pkg, name, smax=smax)
    try:
        assert _size_class(L.sosgpu_ctx_bytes(cx._h)) == cls
        cnt, dist, _ = check_tables(oracle, cx, name, smax=smax)
    finally:
        cx.close()
    print(which, "entries compared:", cnt)
