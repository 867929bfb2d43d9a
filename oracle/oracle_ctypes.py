"""ctypes wrapper of oracle/libsos_oracle.so (the plain-C restatement, oracle/sos_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
leg, never by the product package.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libsos_oracle.so")
_lib = None


def build():
    """Compile the C restatement (and, when the reference sources are present, oracle/_ref)."""
    subprocess.check_call(["make", "-s", "-C", HERE, "all"])


def lib():
    global _lib
    if _lib is None:
        # the library is git-ignored but may be carried along with a tree: make is a no-op when it is up to date and
        # rebuilds one that is older than its sources (and so may lack symbols)
        subprocess.check_call(["make", "-s", "-C", HERE, SO])
        _lib = C.CDLL(SO)
        _lib.sos_oracle_os.restype = C.c_int
        _lib.sos_oracle_os_levels.restype = C.c_int
        _lib.sos_oracle_stop_margin.restype = C.c_double
        _lib.sos_oracle_profile_rescale.restype = C.c_int
        _lib.sos_oracle_aggregate.restype = C.c_int
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


def noyaux(is_, rmu0, mu, os_nb, alpha, beta, gamma, zeta):
    n = len(mu)
    w = 2 * n + 1
    keep = []

    def inp(x):
        a, p = _d(x)
        keep.append(a)
        return p

    vec = [np.zeros(w) for _ in range(3)]
    mats = [np.zeros((w, w)) for _ in range(6)]
    lib().sos_oracle_noyaux(C.c_int(is_), C.c_int(n), C.c_double(rmu0), inp(mu), C.c_int(os_nb),
                            inp(alpha), inp(beta), inp(gamma), inp(zeta),
                            *[v.ctypes.data_as(C.c_void_p) for v in vec],
                            *[m.ctypes.data_as(C.c_void_p) for m in mats])
    out = dict(zip(["BP", "GR", "GT", "ARR", "ART", "ATT"], mats))
    out.update(dict(zip(["XPL", "XRL", "XTL"], vec)))
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def noyaux_ext(is_, rmu0, mu, os_nb, alpha, beta, gamma, zeta, start=None, kernels=True):
    """sos_oracle_noyaux_ext: as noyaux(), plus PSL/RSL/TSL [os_nb+1][W] of every l; start [3][n+1] (or None) replaces the three
    pow start values of is_ >= 2; kernels=False skips the six sums (their keys are then absent)."""
    n = len(mu)
    w = 2 * n + 1
    ins = [np.ascontiguousarray(x, dtype=np.float64) for x in (mu, alpha, beta, gamma, zeta)]
    st = None
    if start is not None:
        st = np.ascontiguousarray(start, dtype=np.float64)
        assert st.shape == (3, n + 1), st.shape
    prt = [np.zeros((os_nb + 1, w)) for _ in range(3)]
    vec = [np.zeros(w) for _ in range(3)]
    mats = [np.zeros((w, w)) for _ in range(6)] if kernels else []
    lib().sos_oracle_noyaux_ext(C.c_int(is_), C.c_int(n), C.c_double(rmu0), _p(ins[0]), C.c_int(os_nb),
                                _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(ins[4]), None if st is None else _p(st),
                                *[_p(a) for a in prt], *[_p(v) for v in vec],
                                *([_p(m) for m in mats] if kernels else [None] * 6))
    out = dict(zip(["BP", "GR", "GT", "ARR", "ART", "ATT"], mats))
    out.update(dict(zip(["XPL", "XRL", "XTL"], vec)))
    out.update(dict(zip(["PSL", "RSL", "TSL"], prt)))
    return out


KERNEL_NAMES = ("BP", "GR", "GT", "ARR", "ART", "ATT")


def _kern6(k):
    return np.ascontiguousarray(np.stack([k[x] for x in KERNEL_NAMES]), dtype=np.float64)


def _xprt3(k):
    return np.ascontiguousarray(np.stack([k["XPL"], k["XRL"], k["XTL"]]), dtype=np.float64)


def ray_coefs(ron, ipolar):
    """BETA2, GAMMA2, ALPHA2 (SOS_OS.F:678-699)."""
    out = np.zeros(3)
    lib().sos_oracle_ray_coefs(C.c_double(ron), C.c_int(ipolar), _p(out))
    return tuple(out)


def ray_kernels(is_, k, b2g2a2):
    """The molecular terms of SOS_OS.F:2859-2876 as six (W x W) kernels, from XPL/XRL/XTL of the dict k."""
    x3 = _xprt3(k)
    w = x3.shape[1]
    out = np.zeros((6, w, w))
    lib().sos_oracle_ray_kernels(C.c_int(is_), C.c_int((w - 1) // 2), _p(x3), *[C.c_double(v) for v in b2g2a2], _p(out))
    return dict(zip(KERNEL_NAMES, out))


def order1_coefs(is_, k, b2g2a2):
    """SOS_FSOURCE_ORDRE1 per direction: (aer[3][W], ray[3][W]) = I, Q, U coefficients (U with the routine's minus sign)."""
    k6, x3 = _kern6(k), _xprt3(k)
    w = x3.shape[1]
    aer, ray = np.zeros((3, w)), np.zeros((3, w))
    lib().sos_oracle_order1_coefs(C.c_int(is_), C.c_int((w - 1) // 2), _p(k6), _p(x3), C.c_double(b2g2a2[0]),
                                  C.c_double(b2g2a2[1]), _p(aer), _p(ray))
    return aer, ray


def fresnel1_coefs(is_, k, b2g2a2, f11sun, f12sun):
    """SOS_FSOURCE_DIFF_FRESNEL1 per field direction, without COEFK and the profile: (aer[3][W], ray[3][W])."""
    k6, x3 = _kern6(k), _xprt3(k)
    w = x3.shape[1]
    aer, ray = np.zeros((3, w)), np.zeros((3, w))
    lib().sos_oracle_fresnel1_coefs(C.c_int(is_), C.c_int((w - 1) // 2), C.c_double(f11sun), C.c_double(f12sun), _p(k6), _p(x3),
                                    *[C.c_double(v) for v in b2g2a2], _p(aer), _p(ray))
    return aer, ray


def fresnel1_routine(is_, k, b2g2a2, f11sun, f12sun, pcaer, pcray):
    """The static SOS_FSOURCE_DIFF_FRESNEL1 at H = 0, MUS = 1 (COEFK = 1/4) with the profile (pcaer, pcray): [3][W]."""
    k6, x3 = _kern6(k), _xprt3(k)
    w = x3.shape[1]
    out = np.zeros((3, w))
    lib().sos_oracle_fresnel1_routine(C.c_int(is_), C.c_int((w - 1) // 2), C.c_double(f11sun), C.c_double(f12sun), _p(k6), _p(x3),
                                      *[C.c_double(v) for v in b2g2a2], C.c_double(pcaer), C.c_double(pcray), _p(out))
    return out


def ordreig_level(is_, ga, k, b2g2a2, field):
    """SOS_FSOURCE_ORDREIG at one level applied to field [3][W] (I, Q, U over jj = -N..N): (aer[3][W], ray[3][W])."""
    k6, x3 = _kern6(k), _xprt3(k)
    w = x3.shape[1]
    g = np.ascontiguousarray(ga, dtype=np.float64)
    f = np.ascontiguousarray(field, dtype=np.float64)
    assert f.shape == (3, w) and len(g) == (w - 1) // 2
    aer, ray = np.zeros((3, w)), np.zeros((3, w))
    lib().sos_oracle_ordreig_level(C.c_int(is_), C.c_int(len(g)), _p(g), _p(k6), _p(x3), *[C.c_double(v) for v in b2g2a2],
                                   _p(f), _p(aer), _p(ray))
    return aer, ray


def sos_os(rmu, ga, os_nb, h, xdel, ydel, alpha, beta, gamma, zeta, *, n0, tetas=0.0, ro=0.0,
           imat_surf=0, ifresnel=0, ind_surf=1.34, zprof=None, ron=float(np.float32(0.0279)), zout=-1.0,
           igmax=100, iborm=None, ipolar=1, rsurf=None):
    """Same signature/return as oracle.ref_ctypes.sos_os (minus the log)."""
    n = len(rmu)
    nt = len(h) - 1
    w = 2 * n + 1
    if iborm is None:
        iborm = os_nb
    if zprof is None:
        zprof = np.linspace(120.0, 0.0, nt + 1)
    keep = []

    def inp(x):
        a, p = _d(x)
        keep.append(a)
        return p

    rec = np.zeros((iborm + 1, 3, w))
    n_orders = C.c_int(0)
    ig_last = np.zeros(iborm + 1, dtype=np.int32)
    emoins, eplus = C.c_double(0), C.c_double(0)
    rs_p = None
    if imat_surf == 1:
        rs = np.ascontiguousarray(rsurf, dtype=np.float32)
        assert rs.shape == (iborm + 1, 9, n, n), rs.shape
        keep.append(rs)
        rs_p = rs.ctypes.data_as(C.c_void_p)
    ier = lib().sos_oracle_os(
        C.c_int(n), inp(rmu), inp(ga), C.c_int(os_nb), C.c_int(nt), C.c_int(n0), C.c_double(tetas),
        C.c_double(ro), C.c_int(imat_surf), C.c_int(ifresnel), C.c_double(ind_surf),
        inp(h), inp(xdel), inp(ydel), inp(zprof), C.c_double(ron),
        inp(alpha), inp(beta), inp(gamma), inp(zeta), C.c_double(zout), C.c_int(igmax), C.c_int(iborm),
        C.c_int(ipolar), rs_p, rec.ctypes.data_as(C.c_void_p), C.byref(n_orders),
        ig_last.ctypes.data_as(C.c_void_p), C.byref(emoins), C.byref(eplus))
    f = n_orders.value
    return dict(records=rec[:f].copy(), emoins=emoins.value, eplus=eplus.value, ier=ier,
                ig_counts=ig_last[:f].copy())


def sos_os_levels(rmu, ga, os_nb, h, xdel, ydel, alpha, beta, gamma, zeta, zouts, *, n0, tetas=0.0, ro=0.0,
                  imat_surf=0, ifresnel=0, ind_surf=1.34, zprof=None, ron=float(np.float32(0.0279)),
                  igmax=100, iborm=None, ipolar=1, rsurf=None):
    """sos_os with several output altitudes from one solve: records [nz][F][3][W]; ig_counts, fluxes and ier as sos_os, plus
    margin = the tie audit of this very call (read on the calling thread, so it is valid under a thread pool)."""
    n = len(rmu)
    nt = len(h) - 1
    w = 2 * n + 1
    if iborm is None:
        iborm = os_nb
    if zprof is None:
        zprof = np.linspace(120.0, 0.0, nt + 1)
    ins = [np.ascontiguousarray(x, dtype=np.float64) for x in (rmu, ga, h, xdel, ydel, zprof, alpha, beta, gamma, zeta, zouts)]
    nz = len(ins[10])
    assert nz >= 1
    rec = np.zeros((nz, iborm + 1, 3, w))
    n_orders = C.c_int(0)
    ig_last = np.zeros(iborm + 1, dtype=np.int32)
    emoins, eplus = C.c_double(0), C.c_double(0)
    rs = None
    if imat_surf == 1:
        rs = np.ascontiguousarray(rsurf, dtype=np.float32)
        assert rs.shape == (iborm + 1, 9, n, n), rs.shape
    ier = lib().sos_oracle_os_levels(
        C.c_int(n), _p(ins[0]), _p(ins[1]), C.c_int(os_nb), C.c_int(nt), C.c_int(n0), C.c_double(tetas),
        C.c_double(ro), C.c_int(imat_surf), C.c_int(ifresnel), C.c_double(ind_surf),
        _p(ins[2]), _p(ins[3]), _p(ins[4]), _p(ins[5]), C.c_double(ron),
        _p(ins[6]), _p(ins[7]), _p(ins[8]), _p(ins[9]), C.c_int(nz), _p(ins[10]), C.c_int(igmax), C.c_int(iborm),
        C.c_int(ipolar), None if rs is None else _p(rs), _p(rec), C.byref(n_orders), _p(ig_last),
        C.byref(emoins), C.byref(eplus))
    margin = lib().sos_oracle_stop_margin()
    f = n_orders.value
    return dict(records=rec[:, :f].copy(), emoins=emoins.value, eplus=eplus.value, ier=ier, ig_counts=ig_last[:f].copy(),
                margin=margin)


def stop_margin():
    """Tie audit of the last sos_os / sos_os_levels call of this thread: min |Z1/threshold - 1| over all its stop decisions (sos_oracle.c audit)."""
    return lib().sos_oracle_stop_margin()


def profile_rescale(h, xdel, ydel, a_tronc, piz, piztr, os_nb):
    h = np.array(h, dtype=np.float64)
    xdel = np.array(xdel, dtype=np.float64)
    ydel = np.array(ydel, dtype=np.float64)
    iborm = lib().sos_oracle_profile_rescale(C.c_int(len(h) - 1), C.c_double(a_tronc), C.c_double(piz),
                                             C.c_double(piztr), C.c_int(os_nb),
                                             h.ctypes.data_as(C.c_void_p), xdel.ctypes.data_as(C.c_void_p),
                                             ydel.ctypes.data_as(C.c_void_p))
    return h, xdel, ydel, iborm


def aggregate(rec_bins, nf, aik, scal_bins):
    """rec_bins [nb][fmax][3][W], nf [nb], aik [nb], scal_bins [nb][7] -> (out_rec[F][3][W], out_scal[7])."""
    rec_bins = np.ascontiguousarray(rec_bins, dtype=np.float64)
    nb, fmax, _, w = rec_bins.shape
    nf = np.ascontiguousarray(nf, dtype=np.int32)
    aik = np.ascontiguousarray(aik, dtype=np.float64)
    scal_bins = np.ascontiguousarray(scal_bins, dtype=np.float64)
    out_rec = np.zeros((fmax, 3, w))
    out_scal = np.zeros(7)
    f = lib().sos_oracle_aggregate(C.c_int(nb), C.c_int(fmax), C.c_int(w), nf.ctypes.data_as(C.c_void_p),
                                   aik.ctypes.data_as(C.c_void_p), rec_bins.ctypes.data_as(C.c_void_p),
                                   scal_bins.ctypes.data_as(C.c_void_p), out_rec.ctypes.data_as(C.c_void_p),
                                   out_scal.ctypes.data_as(C.c_void_p))
    return out_rec[:f], out_scal


def sigma2(wind):
    lib().sos_oracle_sigma2.restype = C.c_double
    return lib().sos_oracle_sigma2(C.c_double(wind))


def glitter(rmu, chr_, wind, ind, os_nb, os_ns, os_nm):
    """SOS_GLITTER restatement: returns dict(rsurf float32[os_nb+1][9][N][N], il[npairs], e[npairs][os_nm+1],
    coef[4][os_ns+1])."""
    n = len(rmu)
    npairs = n * (n + 1) // 2
    a_mu, p_mu = _d(rmu)
    a_ch, p_ch = _d(chr_)
    out = np.zeros((os_nb + 1, 9, n, n), dtype=np.float32)
    il = np.zeros(npairs, dtype=np.int32)
    e = np.zeros((npairs, os_nm + 1))
    coef = np.zeros((4, os_ns + 1))
    lib().sos_oracle_glitter(C.c_int(n), p_mu, p_ch, C.c_double(wind), C.c_double(ind), C.c_int(os_nb), C.c_int(os_ns),
                             C.c_int(os_nm), out.ctypes.data_as(C.c_void_p), il.ctypes.data_as(C.c_void_p),
                             e.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p))
    return dict(rsurf=out, il=il, e=e, coef=coef)


def _margins(fn, k):
    m = (C.c_double * k)()
    fn(m)
    return np.array(m[:])


def glitter_margin():
    """Tie audit of the last glitter() call: min |tested / threshold - 1| of the per-level 1e-4 test, of the 1e-3 closure
    that sets IL and of the 1 % bisection test (1e300 where a test never ran)."""
    return _margins(lib().sos_oracle_quad_margin, 3)


def land(isurf, rmu, chr_, k0, k1, k2, coef_c, ind, os_nb, os_ns, os_nm):
    """Land-surface matrices (SOS_ROUJEAN / SOS_SURFACE_BPDF / SOS_BPDF_AJOUT_BRDF) for isurf 3, 4, 5, 7: dict(rsurf
    float32[os_nb+1][9][N][N], ier (0, or -1: negative Roujean BRDF), il_nn[N][N], e_nn[N][N][os_nb+1])."""
    n = len(rmu)
    a_mu, p_mu = _d(rmu)
    a_ch, p_ch = _d(chr_)
    out = np.zeros((os_nb + 1, 9, n, n), dtype=np.float32)
    il = np.zeros((n, n), dtype=np.int32)
    e = np.zeros((n, n, os_nb + 1))
    lib().sos_oracle_land.restype = C.c_int
    ier = lib().sos_oracle_land(C.c_int(int(isurf)), C.c_int(n), p_mu, p_ch, C.c_double(k0), C.c_double(k1), C.c_double(k2),
                                C.c_double(coef_c), C.c_double(ind), C.c_int(os_nb), C.c_int(os_ns), C.c_int(os_nm),
                                out.ctypes.data_as(C.c_void_p), il.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p))
    return dict(rsurf=out, ier=ier, il_nn=il, e_nn=e)


def land_margin():
    """Tie audit of the last land() call: Roujean B1 against 1e-3, B1 against the previous B1, then the three of the
    Maignan quadrature as glitter_margin()."""
    return _margins(lib().sos_oracle_land_margin, 5)


def calc_f_roujean(k0, k1, k2, c1, c2, phi):
    lib().sos_oracle_calc_f_roujean.restype = C.c_double
    return lib().sos_oracle_calc_f_roujean(*[C.c_double(x) for x in (k0, k1, k2, c1, np.sqrt(1 - c1 * c1), c2,
                                                                      np.sqrt(1 - c2 * c2), phi)])


def trphi_land(rmu, rec, tau, tauout, phi, *, igli=0, n0=1, wind=0.0, ind_surf=1.34, ifresnel=0, ipolar=1, isurf=0,
               k0=0.0, k1=0.0, k2=0.0, coef_c=0.0):
    """SOS_TRPHI with the direct term of a land surface.  Returns dict(out=[XIT, XQT, XUT, ANGDIFF], cosdif[W] (the cosine
    ANGDIFF is the acos of), pre[3][W] (XIT, XQT, XUT before the zeroing thresholds))."""
    n = len(rmu)
    w = 2 * n + 1
    a_mu, p_mu = _d(rmu)
    a_rec, p_rec = _d(rec)
    outs = [np.zeros(w) for _ in range(5)]
    pre = np.zeros((3, w))
    lib().sos_oracle_trphi_land(C.c_int(n), p_mu, C.c_int(a_rec.shape[0]), p_rec, C.c_double(tau), C.c_double(tauout),
                                C.c_double(phi), C.c_int(igli), C.c_int(n0), C.c_double(wind), C.c_double(ind_surf),
                                C.c_int(ifresnel), C.c_int(ipolar), C.c_int(int(isurf)), C.c_double(k0), C.c_double(k1),
                                C.c_double(k2), C.c_double(coef_c), *[o.ctypes.data_as(C.c_void_p) for o in outs],
                                pre.ctypes.data_as(C.c_void_p))
    return dict(out=outs[:4], cosdif=outs[4], pre=pre)


def trphi(rmu, rec, tau, tauout, phi, *, igli=0, n0=1, wind=0.0, ind_surf=1.34, ifresnel=0, ipolar=1):
    n = len(rmu)
    w = 2 * n + 1
    a_mu, p_mu = _d(rmu)
    a_rec, p_rec = _d(rec)
    outs = [np.zeros(w) for _ in range(4)]
    lib().sos_oracle_trphi(C.c_int(n), p_mu, C.c_int(a_rec.shape[0]), p_rec, C.c_double(tau), C.c_double(tauout),
                           C.c_double(phi), C.c_int(igli), C.c_int(n0), C.c_double(wind), C.c_double(ind_surf),
                           C.c_int(ifresnel), C.c_int(ipolar), *[o.ctypes.data_as(C.c_void_p) for o in outs])
    return outs


def polar(xi, xq, xu):
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    lib().sos_oracle_polar(C.c_double(xi), C.c_double(xq), C.c_double(xu), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def sos_profile(tr, hr, ta, ha, altabs=None, tabs=None, absprofil=1):
    """SOS_PROFILE for IPROFIL=1 (SOS_PROFIL.F:224) as read back from the PROFIL file: returns dict(ier, nt, zprof, h,
    xdel (=PCAER), ydel (=PCMOL)).  tabs=None or all-zero last level: no gas absorption."""
    n = 601
    z, h, pa, pm = (np.zeros(n) for _ in range(4))
    nt = C.c_int(0)
    if tabs is None:
        p_alt, p_tab, absprofil = None, None, 7
    else:
        a_alt = np.ascontiguousarray(altabs, dtype=np.float64); a_tab = np.ascontiguousarray(tabs, dtype=np.float64)
        assert a_alt.shape == (50,) and a_tab.shape == (50,)
        p_alt, p_tab = a_alt.ctypes.data_as(C.c_void_p), a_tab.ctypes.data_as(C.c_void_p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib().sos_profile_oracle.restype = C.c_int
    ier = lib().sos_profile_oracle(C.c_double(tr), C.c_double(hr), C.c_double(ta), C.c_double(ha), C.c_int(absprofil),
                                   p_alt, p_tab, C.byref(nt), vp(z), vp(h), vp(pa), vp(pm))
    k = nt.value + 1
    return dict(ier=ier, nt=nt.value, zprof=z[:k].copy(), h=h[:k].copy(), xdel=pa[:k].copy(), ydel=pm[:k].copy())


EXP_MODES = {"exact": (0, 0), "plus": (1, 0), "minus": (2, 0), "rand_a": (3, 0x243F6A8885A308D3), "rand_b": (3, 0x13198A2E03707344)}
INFO_BIN = ("regime", "strong", "clamp", "scan_steps", "dropped", "dropped_first", "ing", "nt_ng", "regime_ng", "scan_steps_ng",
            "ier_from", "nt_loop")
INFO_BINF = ("zlim", "t_first", "t_layer", "ttot", "tgtot", "t_layer_unclamped", "ttot_ng", "t_first_ng", "t_layer_ng")


def sos_profile_info(tr, hr, ta, ha, altabs=None, tabs=None, absprofil=1, exp_mode="exact"):
    """sos_profile for an absorption grid of any length (>= 2 levels), plus what the run did: the keys of INFO_BIN / INFO_BINF
    (sos_profile_oracle_info in sos_profile_oracle.c), per level of the gas step `steps`, `zero_stop`, `forced`, `near_skip`
    [nt + 1], per level of the no-gas profile `steps_ng`, `zero_stop_ng` [nt_ng + 1], and `raw` = dict(zprof, h, xdel, ydel)
    before the decimal round trip.  exp_mode: a key of EXP_MODES -- every exp of the run as glibc gives it ("exact"), moved by
    +1 / -1 ulp, or by a pseudo-random +-1 ulp keyed on the argument's bits."""
    n = 602
    z, h, pa, pm = (np.zeros(n) for _ in range(4))
    nt = C.c_int(0)
    nblev = 50
    if tabs is None:
        p_alt, p_tab, absprofil = None, None, 7
    else:
        a_alt = np.ascontiguousarray(altabs, dtype=np.float64); a_tab = np.ascontiguousarray(tabs, dtype=np.float64)
        nblev = int(a_alt.size)
        assert a_alt.shape == (nblev,) and a_tab.shape == (nblev,) and nblev >= 2
        p_alt, p_tab = a_alt.ctypes.data_as(C.c_void_p), a_tab.ctypes.data_as(C.c_void_p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ib, fb = np.zeros(len(INFO_BIN), dtype=np.int32), np.zeros(len(INFO_BINF))
    lev, lev_ng, raw = np.zeros((4, n), dtype=np.int32), np.zeros((2, n), dtype=np.int32), np.zeros((4, n))
    L = lib()
    L.sos_profile_oracle_info.restype = C.c_int
    mode, key = EXP_MODES[exp_mode]
    L.sos_profile_oracle_exp_mode(C.c_int(mode), C.c_ulonglong(key))
    try:
        ier = L.sos_profile_oracle_info(C.c_double(tr), C.c_double(hr), C.c_double(ta), C.c_double(ha), C.c_int(absprofil),
                                        C.c_int(nblev), p_alt, p_tab, C.byref(nt), vp(z), vp(h), vp(pa), vp(pm), vp(ib), vp(fb),
                                        vp(lev), vp(lev_ng), vp(raw))
    finally:
        L.sos_profile_oracle_exp_mode(C.c_int(0), C.c_ulonglong(0))
    k = nt.value + 1 if ier == 0 else 0
    out = dict(ier=ier, nt=nt.value if ier == 0 else -1, zprof=z[:k].copy(), h=h[:k].copy(), xdel=pa[:k].copy(), ydel=pm[:k].copy())
    out.update({name: int(v) for name, v in zip(INFO_BIN, ib)})
    out.update({name: float(v) for name, v in zip(INFO_BINF, fb)})
    kg = out["nt_ng"] + 1
    out.update(steps=lev[0, :k].copy(), zero_stop=lev[1, :k].copy(), forced=lev[2, :k].copy(), near_skip=lev[3, :k].copy(),
               steps_ng=lev_ng[0, :kg].copy(), zero_stop_ng=lev_ng[1, :kg].copy(),
               raw=dict(zprof=raw[0, :k].copy(), h=raw[1, :k].copy(), xdel=raw[2, :k].copy(), ydel=raw[3, :k].copy()))
    return out


def profile_roundtrip(values, fmt="e15.8"):
    """The PROFIL file's decimal round trip of each value: written with E15.8 (or F10.5) and read back, by snprintf / strtod."""
    a = np.ascontiguousarray(values, dtype=np.float64).ravel()
    out = np.empty_like(a)
    lib().sos_profile_oracle_roundtrip(C.c_int({"e15.8": 0, "f10.5": 1}[fmt]), C.c_long(a.size), a.ctypes.data_as(C.c_void_p),
                                       out.ctypes.data_as(C.c_void_p))
    return out


def absprofile(xk, ro, ik):
    """SOS_ABSPROFILE for one bin in plain C (sos_absprofile_oracle): xk[8][nterm][nlev-1], ro[8][nlev-1], ik[8] -> TAUABS[nlev]."""
    xk = np.ascontiguousarray(xk, dtype=np.float64); ro = np.ascontiguousarray(ro, dtype=np.float64)
    ik = np.ascontiguousarray(ik, dtype=np.int32)
    nterm, nlev = xk.shape[1], xk.shape[2] + 1
    assert xk.shape == (8, nterm, nlev - 1) and ro.shape == (8, nlev - 1) and ik.shape == (8,)
    tau = np.zeros(nlev)
    lib().sos_absprofile_oracle(C.c_int(nlev), C.c_int(nterm), ik.ctypes.data_as(C.c_void_p), xk.ctypes.data_as(C.c_void_p),
                                ro.ctypes.data_as(C.c_void_p), tau.ctypes.data_as(C.c_void_p))
    return tau


def mie(xmu, rn, in_, alphas):
    """SOS_MIE + SOS_FPHASE_MIE records for the size parameters `alphas` at the cosines xmu[2 nbmu + 1].  Returns dict(rec float32
    [na][4 + 3 W] in the layout of sosgpu_mie, g float64 [na], info int32 [na][4] = n2 finally used, overflow break taken,
    number of SNA rescales, n1) plus the record's fields as views: alpha, qext, qsca [na], imie, qmie, umie [na][W], and f64 [na][3 + 3 W] =
    Qext, Qsca, g, Imie, Qmie, Umie as doubles before the record's REAL*4 rounding."""
    a_mu, p_mu = _d(xmu)
    a_al, p_al = _d(np.atleast_1d(alphas))
    w, na = len(a_mu), len(a_al)
    assert w % 2 == 1 and w >= 3
    rec = np.zeros((na, 4 + 3 * w), dtype=np.float32)
    g = np.zeros(na)
    info = np.zeros((na, 4), dtype=np.int32)
    f64 = np.zeros((na, 3 + 3 * w))
    lib().sos_oracle_mie_f64.restype = C.c_int
    rc = lib().sos_oracle_mie_f64(C.c_int((w - 1) // 2), p_mu, C.c_double(rn), C.c_double(in_), C.c_int(na), p_al,
                                  rec.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p),
                                  f64.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("sos_oracle_mie: %d" % rc)
    return dict(rec=rec, g=g, info=info, f64=f64, alpha=rec[:, 0], qext=rec[:, 1], qsca=rec[:, 2], imie=rec[:, 4:4 + w],
                qmie=rec[:, 4 + w:4 + 2 * w], umie=rec[:, 4 + 2 * w:4 + 3 * w])


def granu(rec, igranu, v1, v2, v3, wa, alphaf):
    """SOS_GRANU on the records rec[na][4 + 3 W] (layout of sosgpu_mie).  Returns (out[3 + 3 W], nuse)."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    na, rs = rec.shape
    w = (rs - 4) // 3
    assert rs == 4 + 3 * w and w % 2 == 1
    out = np.zeros(3 + 3 * w)
    nuse = C.c_int(-1)
    lib().sos_oracle_granu.restype = C.c_int
    rc = lib().sos_oracle_granu(C.c_int((w - 1) // 2), C.c_int(na), rec.ctypes.data_as(C.c_void_p), C.c_int(int(igranu)),
                                C.c_double(v1), C.c_double(v2), C.c_double(v3), C.c_double(wa), C.c_double(alphaf),
                                out.ctypes.data_as(C.c_void_p), C.byref(nuse))
    if rc:
        raise ValueError("sos_oracle_granu: %d" % rc)
    return out, nuse.value
