"""Host-side restatements of the steps before the hot path: the Gauss angles of SOS_ANGLES, the Rayleigh optical thickness and
the no-gas profiles of SOS_PROFILE (the checkers of the device profile stage, and the aerosol-layer profile)."""
import collections
import functools
import math
import os
import threading

import numpy as np

from .params import (CTE_DELTA_Z, CTE_HT_STD_PSURF, CTE_OS_NBMU_MAX, CTE_OS_NT, CTE_OS_NT_MIN, CTE_TCOUCHE, CTE_TOA_ALT,
                     CTE_TOA_FIRST_LAYER, SosProcError, _F)
from .synth import _round_sig


def sos_gauss(nb_gauss):
    """(cached per order: the Newton iterations cost 2 ms of every call otherwise; fresh arrays are returned)"""
    mu, wt = _sos_gauss_nodes(int(nb_gauss))
    return np.array(mu), np.array(wt)


@functools.lru_cache(maxsize=32)
def _sos_gauss_nodes(nb_gauss):
    """SOS_GAUSS (SOS_ANGLES.F:1022-1103) for MM = nb_gauss + 1: the positive nodes and weights of the 2 nb_gauss-point
    Gauss-Legendre rule, ascending in the cosine -- the reference's own Newton iteration (asymptotic start, three-term
    recurrence, stop at |dx| <= 1e-15), statement for statement, so that the D21.14 digits of the angle files agree in
    their last place too (numpy's leggauss differs from it by an ulp here and there)."""
    n = 2 * nb_gauss
    pi = math.pi
    aa = 2.0 / pi ** 2
    ab = -62.0 / (3.0 * pi ** 4)
    ac = 15116.0 / (15.0 * pi ** 6)
    ad = -12554474.0 / (105.0 * pi ** 8)
    en = float(n)
    u = 1.0 - (2.0 / pi) ** 2
    d = 1.0 / math.sqrt((en + 0.5) ** 2 + u / 4.0)
    r, w = [], []
    for k in range(1, n + 1):
        az = 4.0 * k - 1.0
        z = 0.25 * pi * (az + aa / az + ab / az ** 3 + ac / az ** 5 + ad / az ** 7)
        x = math.cos(z * d)
        while True:
            pm2, pm1 = 1.0, x                              # PA(1), PA(2)
            for nn in range(3, n + 2):
                enn = nn - 1.0
                pm2, pm1 = pm1, ((2.0 * enn - 1.0) * x * pm1 - (enn - 1.0) * pm2) / enn
            pnp = en * (pm2 - x * pm1) / (1.0 - x * x)     # PA(N), PA(NP1)
            xi = x - pm1 / pnp
            if abs(xi - x) - 1.0e-15 <= 0.0:
                r.append(x)
                w.append(2.0 * (1.0 - x * x) / (en * pm2) ** 2)
                break
            x = xi
    # R(I), I = 1..MM-1, descend from the largest node: AMU(K = MM - I) -> ascending cosines for K = 1..nb_gauss
    mu = tuple([r[i] for i in range(nb_gauss)][::-1])
    wt = tuple([w[i] for i in range(nb_gauss)][::-1])
    return mu, wt


# ---------------------------------------------------------------------------------------------------------
# host-side restatements of the steps before the hot path (inputs of SOS_OS)
# ---------------------------------------------------------------------------------------------------------
_ANGLES_CACHE = collections.OrderedDict()
_ANGLES_LOCK = threading.Lock()


def angles(nbmu_gauss, tetas, user_file="NO_USER_ANGLES"):
    """SOS_ANGLES for the radiance angles (SOS_ANGLES.F:380-466, 713-866): Gauss nodes/weights of the
    2*NbGauss-point rule on [-1,1] (positive half), optional user angles (weight 0), solar angle inserted
    with weight 0 unless it coincides with a node, mu descending; values as re-read from SOS_UsedAngles.txt
    (D21.14).  Returns mu[N], ga[N], n0 (1-based), ind_angout[N] (1 = user angle).
    The last few angle sets are kept (the calls of a spectrum share theirs; a user file is keyed by its size and time stamp)."""
    key = (int(nbmu_gauss), float(tetas), str(user_file))
    if user_file != "NO_USER_ANGLES":
        try:
            st = os.stat(user_file)
            key += (st.st_size, st.st_mtime_ns)
        except OSError:
            key = None
    with _ANGLES_LOCK:
        hit = _ANGLES_CACHE.get(key) if key is not None else None
    if hit is None:
        hit = _angles(nbmu_gauss, tetas, user_file)
        if key is not None:
            with _ANGLES_LOCK:
                _ANGLES_CACHE[key] = hit
                while len(_ANGLES_CACHE) > 16:
                    _ANGLES_CACHE.popitem(last=False)
    mu, ga, n0, ind = hit
    return mu.copy(), ga.copy(), n0, ind.copy()


def _angles(nbmu_gauss, tetas, user_file):
    x, w = sos_gauss(nbmu_gauss)
    mu = list(x)
    wt = list(w)
    if user_file != "NO_USER_ANGLES":
        with open(user_file) as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                val = float(line.split()[0])
                if val < 0. or val > 90.:
                    raise SosProcError("user angle out of [0,90] in %s" % user_file)
                mu.append(math.cos(val * math.pi / 180.))
                wt.append(0.0)
    order = np.argsort(-np.asarray(mu), kind="stable")
    mu = np.asarray(mu)[order]
    wt = np.asarray(wt)[order]
    ind = (wt == 0.0).astype(np.int32)
    xmus = math.cos(tetas * math.pi / 180.)
    imus = -1
    for j in range(len(mu)):
        if abs(xmus - mu[j]) < _F(0.00001):       # CTE_SEUIL_ECART_MUS, SOS.h:561
            imus = j + 1
    if imus == -1:
        pos = int(np.sum(mu > xmus))
        mu = np.insert(mu, pos, xmus)
        wt = np.insert(wt, pos, 0.0)
        ind = np.insert(ind, pos, 0)
        imus = pos + 1
    if len(mu) > CTE_OS_NBMU_MAX:
        raise SosProcError("number of radiance angles > CTE_OS_NBMU_MAX")
    return _round_sig(mu, 14), _round_sig(wt, 14), imus, ind


def rayleigh_optical_thickness(wa_simu, psurf):
    """SOS_PROC.F:3333-3334 (CNES formulation); 84.35, 1.225, 1.4 are REAL*4 literals."""
    return (psurf / CTE_HT_STD_PSURF) * 1.e-4 * (_F(84.35) / wa_simu ** 4 - _F(1.225) / wa_simu ** 5 + _F(1.4) / wa_simu ** 6)


def _disc(dt, ta, ha, tr, hr, tim1, zmax_init):
    """SOS_DISC without gas (SOS_PROFIL.F:1260-1325): altitude where tau(z) = tim1 + dt, by bisection."""
    ti = tim1 + dt
    zmax, zmin = zmax_init, 0.0
    while True:
        zmoy = (zmax + zmin) / 2.
        tz = ta * math.exp(-zmoy / ha) + tr * math.exp(-zmoy / hr)
        xd = abs(ti - tz)
        if xd < _F(.000001) or zmoy == 0.0:
            return zmoy
        if (ti - tz) < 0.0:
            zmin = zmoy
        else:
            zmax = zmoy


def profile_nogas(tr, hr, ta, ha):
    """SOS_PROFILE for IPROFIL=1 without gas absorption (SOS_PROFIL.F:349-508), then the PROFIL_TMP text
    round trip (format 20 `2X,I5,F10.5,3(E15.8)`, SOS_PROFIL.F:1084,1150).  Returns h, xdel, ydel, zprof."""
    ttot = tr + ta
    if (ttot / CTE_OS_NT_MIN) <= CTE_TOA_FIRST_LAYER:
        nt = CTE_OS_NT_MIN
        t_layer = ttot / nt
        t_first = t_layer
    elif (ttot / CTE_OS_NT_MIN) < CTE_TCOUCHE:
        nt = CTE_OS_NT_MIN + 1
        t_first = CTE_TOA_FIRST_LAYER
        t_layer = (ttot - t_first) / CTE_OS_NT_MIN
    else:
        t_first = CTE_TOA_FIRST_LAYER
        nt = int((ttot - t_first) / CTE_TCOUCHE)
        t_layer = (ttot - t_first) / nt
        nt = nt + 1
    if nt > CTE_OS_NT:
        raise SosProcError("profile needs more than CTE_OS_NT levels")
    hmol = np.zeros(nt + 1); haer = np.zeros(nt + 1); z = np.zeros(nt + 1)
    pcmol = np.zeros(nt + 1); pcaer = np.zeros(nt + 1)
    if ta == 0.0:                                   # SOS_PROFIL.F:412-429
        hmol[1] = t_first
        for i in range(2, nt + 1):
            hmol[i] = (i - 1) * t_layer + t_first
        pcmol[:] = 1.0
        z[0] = CTE_TOA_ALT
        for i in range(1, nt + 1):
            z[i] = hr * math.log(tr / hmol[i])
    else:                                           # SOS_PROFIL.F:437-489
        z[0] = CTE_TOA_ALT
        dtau, zz = 0., CTE_TOA_ALT
        while dtau < t_first:
            zz = zz - CTE_DELTA_Z
            dtau = tr * math.exp(-zz / hr) + ta * math.exp(-zz / ha)
        z[1] = zz
        vr, va = tr * math.exp(-zz / hr), ta * math.exp(-zz / ha)
        hmol[1], haer[1] = vr, va
        pcmol[1], pcaer[1] = vr / dtau, va / dtau
        pcmol[0], pcaer[0] = pcmol[1], pcaer[1]
        hprev = dtau
        for i in range(2, nt):
            zz = _disc(t_layer, ta, ha, tr, hr, hprev, z[1])
            z[i] = zz
            vr, va = tr * math.exp(-zz / hr), ta * math.exp(-zz / ha)
            hmol[i], haer[i] = vr, va
            hprev = vr + va
            vr, va = vr - hmol[i - 1], va - haer[i - 1]
            pcmol[i], pcaer[i] = vr / (vr + va), va / (vr + va)
        z[nt] = 0.0
        hmol[nt], haer[nt] = tr, ta
        vr, va = tr - hmol[nt - 1], ta - haer[nt - 1]
        pcmol[nt], pcaer[nt] = vr / (vr + va), va / (vr + va)
    h = hmol + haer
    return _round_sig(h, 8), _round_sig(pcaer, 8), _round_sig(pcmol, 8), np.round(z, 5)


def layer_grid(tr, hr, ta, zmin, zmax):
    """The level counts of profile_layer (SOS_PROFIL.F:800-870): (nt, nbsc_c1, nbsc_c2, nbsc_c3), the levels of the profile
    and the sublayers above the layer, inside it and below it (0 for a layer on the ground).  Raises the routine's two refusals.
    The C library states the same closed forms (sosgpu_profile_layer_grid)."""
    if zmin < 0.0 or zmax <= zmin:
        raise SosProcError("SOS_PROFIL: -AP.AerLayer.Zmin / Zmax must satisfy 0 <= Zmin < Zmax", ier=-1)
    ttot = tr + ta
    nt = int(ttot / CTE_TCOUCHE)
    if nt > CTE_OS_NT:
        nt = CTE_OS_NT
    dzt = _F(0.010)                                   # CTE_DZTRANSI (REAL*4 literal, SOS.h:240)
    vr_c1 = tr * math.exp(-(zmax + dzt) / hr)
    if zmin == 0.0:
        vr_c3, nb_tr = 0.0, 1
    else:
        vr_c3, nb_tr = tr * (1.0 - math.exp(-(zmin - dzt) / hr)), 2
    nbsc_c1 = max(3, int((nt - nb_tr) * vr_c1 / (tr + ta)))              # CTE_PROFIL_MIN_NBC = 3
    nbsc_c3 = 0 if zmin == 0.0 else max(3, int((nt - nb_tr) * vr_c3 / (tr + ta)))
    nbsc_c2 = (nt - nb_tr) - nbsc_c1 - nbsc_c3
    if nbsc_c2 <= 0 or (ta / nbsc_c2) < _F(0.00001):
        raise SosProcError("SOS_PROFIL: not enough sublayers in the aerosol layer (ERROR 1020)", ier=-1)
    return nt, nbsc_c1, nbsc_c2, nbsc_c3


def profile_layer(tr, hr, ta, zmin, zmax):
    """SOS_PROFILE for IPROFIL=2 (SOS_PROFIL.F:800-946): a homogeneous aerosol + molecule layer between zmin and zmax (km)
    inside a molecular atmosphere, no gas absorption, then the PROFIL_TMP text round trip.  Returns h, xdel, ydel, zprof.

    The reference starts its recurrence `Hmol(I)=Hmol(I-1)+VR_SC` (:873) from an Hmol(0) it assigns only at :926 -- a local
    array element read before it is written.  On a fresh stack it is 0, which is also the evident intent (the optical
    depth at the top of the atmosphere, assigned TR*exp(-120/HR) ~ 1e-7 TR afterwards); this restatement starts from 0 and
    is pinned against the reference's routine called on a fresh stack (tests/golden/profile_layer.npz)."""
    nt, nbsc_c1, nbsc_c2, nbsc_c3 = layer_grid(tr, hr, ta, zmin, zmax)
    dzt = _F(0.010)                                   # CTE_DZTRANSI (REAL*4 literal, SOS.h:240)
    vr_c1 = tr * math.exp(-(zmax + dzt) / hr)
    vr_c2 = tr * (math.exp(-zmin / hr) - math.exp(-(zmax + dzt) / hr))
    vr_c3 = 0.0 if zmin == 0.0 else tr * (1.0 - math.exp(-(zmin - dzt) / hr))
    hmol = np.zeros(nt + 1); haer = np.zeros(nt + 1)
    vr_sc = vr_c1 / nbsc_c1
    for i in range(1, nbsc_c1 + 1):
        hmol[i] = hmol[i - 1] + vr_sc
    i = nbsc_c1 + 1
    hmol[i] = tr * math.exp(-zmax / hr)
    vr_sc = hmol[i] - hmol[i - 1]
    haer[i] = haer[i - 1] + (ta * vr_sc / vr_c2)
    delta_z = (zmax - zmin) / nbsc_c2
    z = zmax
    for i in range(nbsc_c1 + 2, nbsc_c1 + nbsc_c2 + 2):
        z = z - delta_z
        hmol[i] = tr * math.exp(-z / hr)
        vr_sc = hmol[i] - hmol[i - 1]
        haer[i] = haer[i - 1] + (ta * vr_sc / vr_c2)
    if zmin != 0.0:
        i = nbsc_c1 + nbsc_c2 + 2
        hmol[i] = tr * math.exp(-(zmin - dzt) / hr)
        haer[i] = haer[i - 1]
        vr_sc = vr_c3 / nbsc_c3
        for i in range(nbsc_c1 + nbsc_c2 + 3, nt + 1):
            hmol[i] = vr_sc + hmol[i - 1]
            haer[i] = haer[i - 1]
    zprof = np.zeros(nt + 1); h = np.zeros(nt + 1); pcaer = np.zeros(nt + 1); pcmol = np.zeros(nt + 1)
    zprof[0] = CTE_TOA_ALT
    hmol[0] = tr * math.exp(-CTE_TOA_ALT / hr)
    h[0] = hmol[0] + haer[0]
    pcmol[0] = 1.0
    for i in range(1, nt + 1):
        h[i] = hmol[i] + haer[i]
        zprof[i] = hr * math.log(tr / hmol[i])
        if haer[i] == haer[i - 1]:
            pcaer[i], pcmol[i] = 0.0, 1.0
        else:
            pcmol[i] = 1 / (1 + (ta / vr_c2))
            pcaer[i] = 1 - pcmol[i]
    return _round_sig(h, 8), _round_sig(pcaer, 8), _round_sig(pcmol, 8), np.round(zprof, 5)
