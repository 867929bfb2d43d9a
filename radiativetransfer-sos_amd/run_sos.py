"""Host-side mirror of the reference's Python front end `binding/run_sos.py`.

Same `-Group.Key` parameter dictionary (run_sos.py:459-559), same user-override merge (:606-609, unknown keys
dropped), same `set_sos_params` ordering (:319-441), same `sos_proc(**kwargs)` keyword names (:640-695) and
the same 23-tuple of outputs with the reference shapes (`PHI_FIN(0:360)`, `THETA_FIN(0:80)`, `(361,81)` tables,
SOS_PROC.F:1168-1204).  Behind that surface the hot path runs on the GPU through the C ABI:

    angles (host)  ->  [aerosol expansion: given]  ->  profile (host)  ->  SOS.F rescale (host)
      -> sosgpu_glitter (ISURF=1) -> sosgpu_noyaux -> sosgpu_os_solve -> sosgpu_aggregate -> sosgpu_trphi

Scope.  Supported: gas absorption by the CKD method (`-AP.AbsProfile.Type` 0..6, both
`-SOS.AbsModeCKD` modes, all bins of a band solved in one batch) or none (7); aerosols given by the reference's own
`-AER.UserFile` (an Aerosols.txt) or by the extension keyword `aer_phase`, or none; exponential profiles
(`-AP.AerProfile.Type 1`); surfaces `-SURF.Type` 0 (Lambert), 1 (+ Cox-Munk glitter), 2 (+ flat sea), 3 (Roujean),
4 / 5 / 7 (Roujean + Rondeaux-Herman / Breon / Maignan), or reflection matrices from a user file (`-SURF.File`, the format
SOS_SURFACE writes); `-SOS.Trans`, `-SOS.Flux`, `SOS_Result.bin` files.
Every aerosol model of `-AER.Model`: 0 (mono-modal log-normal / Junge), 1 (WMO), 2 (Shettle & Fenn), 3 (bimodal
log-normal), 4 (external phase functions), 5 (user mixture) -- Mie theory on the GPU (aerosols.py, csrc/mie.hip).
Both aerosol profiles: exponential (`-AP.AerProfile.Type 1`) and a layer between two altitudes (2; the reference reads an
unassigned Hmol(0) there -- see profile_layer).  Not built: `-SURF.Type 6` (Nadal), which the reference's SOS_PROC refuses
as well.

Differences from the reference script that are deliberate: errors raise exceptions instead of being
lost in an `intent(in)` `ier`; `gen_sos_output` imports `ceil` and uses `and` (the reference has `1 & updown == 2`);
files are written only when `-SOS_Main.ResRoot` is given (RESROOT/SOS/SOS_Result.bin, the -SOS.Trans / -SOS.Flux files).
"""
import collections
import math
import os
import threading

import numpy as np

from .geometry import angles, layer_grid, profile_layer, profile_nogas, rayleigh_optical_thickness, sos_gauss  # noqa: F401
from .params import (CTE_DEFAULT_IGMAX, CTE_DEFAULT_NBMU_LUM, CTE_DEFAULT_NBMU_MIE, CTE_DEFAULT_OS_NB,  # noqa: F401
                     CTE_DEFAULT_OS_NM, CTE_DEFAULT_OS_NS, CTE_DELTA_Z, CTE_HT_STD_PSURF, CTE_LENFIC2, CTE_OS_NBMU_MAX,
                     CTE_OS_NT, CTE_OS_NT_MIN, CTE_TCOUCHE, CTE_TOA_ALT, CTE_TOA_FIRST_LAYER, EXTRA_KEYS,
                     LEVEL_ABSORPTION_NAMES, LEVEL_FLUX_NAMES, LEVEL_FLUX_SPLIT_NAMES, OUTPUT_NAMES, PARAMS,
                     SOS_DEFAULT_AER_JUNGE_RMAX, SOS_DEFAULT_FICANGRESLUM, SOS_DEFAULT_FICANGRESMIE, SOS_DEFAULT_FICGRANU,
                     SOS_DEFAULT_RESBIN, SOS_DEFAULT_RESDOWN, SOS_DEFAULT_RESUP, SOS_NOT_DEFINED_VALUE_DBLE,
                     SOS_NOT_DEFINED_VALUE_INT, SOS_PROC_KWARGS, SosProcError, _D, _I, _angle_counts, default_parameters,
                     set_sos_params, sos_proc_kwargs, update_parameters, validate_parameters)
from .synth import MDF_DEFAULT, rescale_profile


# ---------------------------------------------------------------------------------------------------------
# file formats either side of the hot path
# ---------------------------------------------------------------------------------------------------------
def fortran_e(x, width, digits):
    """Fortran Ew.d edit descriptor: 0.ddddddddE+ee, right-justified in `width` columns.  The digits come from the correctly
    rounded decimal conversion of the binary value (C's %e, as the Fortran runtime's), shifted to the 0.d form."""
    if x == 0.0:
        body = ("-" if math.copysign(1.0, x) < 0 else "") + "0." + "0" * digits + "E+00"
    else:
        m, e = ("%.*e" % (digits - 1, abs(x))).split("e")
        body = ("-" if x < 0 else "") + "0." + m.replace(".", "") + "E%+03d" % (int(e) + 1)
    return body.rjust(width)


def fortran_d(x, width, digits):
    return fortran_e(x, width, digits).replace("E", "D")


def read_aerosols_file(path, os_nb):
    """Parse an `Aerosols.txt` (written by SOS_AEROSOLS.F:2864-2890, read by SOS_PREPA_OS.F:666-700): truncation
    coefficient A, truncated single-scattering albedo PIZTR (both after the ':' of their header line), three title
    lines, then ALPHA, BETA, GAMMA, ZETA for K = 0..OS_NB (list-directed read).  PIZ = PIZTR/(1 + A (PIZTR-1)/2)
    (SOS_PREPA_OS.F:699).  Returns the `aer_phase` dict sos_proc takes."""
    with open(path) as f:
        lines = f.read().splitlines()
    if len(lines) < 8 + os_nb + 1:
        raise SosProcError("aerosol file %s: %d coefficient rows expected" % (path, os_nb + 1))
    a = float(lines[3].split(":", 1)[1].replace("D", "E"))
    piztr = float(lines[4].split(":", 1)[1].replace("D", "E"))
    rows = np.array([[float(v.replace("D", "E")) for v in lines[8 + k].split()[:4]] for k in range(os_nb + 1)])
    return dict(alpha=rows[:, 0].copy(), beta=rows[:, 1].copy(), gamma=rows[:, 2].copy(), zeta=rows[:, 3].copy(),
                a_tronc=a, piztr=piztr, piz=piztr / (1 + 0.5 * a * (piztr - 1)))


def write_aerosols_file(path, aer_phase, kmat1=0.0, kmat2=0.0):
    """`Aerosols.txt` in the layout of SOS_AEROSOLS.F:2864-2890 (formats 40-50, :3049-3056)."""
    al, be, ga, ze = (np.asarray(aer_phase[k], dtype=np.float64) for k in ("alpha", "beta", "gamma", "zeta"))
    a, piztr = float(aer_phase.get("a_tronc", 0.0)), float(aer_phase["piztr"])
    with open(path, "w") as f:
        f.write("EXTINCTION CROSS SECTION (mic^2)     :" + fortran_e(kmat1, 13, 5) + "\n")
        f.write("SCATTERING CROSS SECTION (mic^2)     :" + fortran_e(kmat2, 13, 5) + "\n")
        f.write("ASYMMETRY FACTOR (no truncation)     :" + fortran_e(a / 2. + (1. - a / 2.) * be[1] / 3., 13, 5) + "\n")
        f.write("TRUNCATION COEFFICIENT               :%9.5f\n" % a)
        f.write("SINGLE SCATTERING ALBEDO (truncation):%9.5f\n" % piztr)
        f.write("-" * 33 + "\n")
        f.write("PHASE MATRIX COEFFICIENTS FOR K=0 TO%4d\n" % (len(be) - 1))
        f.write("ALPHA(K)        BETA11(K)       GAMMA12(K)      ZETA(K)\n")
        for k in range(len(be)):
            f.write(fortran_e(al[k], 15, 8) + "".join(" " + fortran_e(v[k], 15, 8) for v in (be, ga, ze)) + "\n")


def write_used_angles(path, mu, ga, n0, ind_ang, nb_gauss, tetas, os_nb, os_ns, os_nm, user_file="NO_USER_ANGLES"):
    """`SOS_UsedAngles.txt` (SOS_ANGLES.F:494-506 header, :639-647 rows `I4,1X,2D21.14,1X,I4`)."""
    with open(path, "w") as f:
        f.write("NB_TOTAL_ANGLES :%4d\n" % len(mu))
        f.write("NB_GAUSS_ANGLES :%4d\n" % nb_gauss)
        f.write("ANGLES_USERFILE :" + user_file.ljust(CTE_LENFIC2) + "\n")
        f.write("SOLAR ZENITH ANGLE :%7.3f\n" % tetas)
        f.write("INTERNAL_IMUS :%4d\n" % n0)
        f.write("INTERNAL_OS_NB :%4d\n" % os_nb)
        f.write("INTERNAL_OS_NS :%4d\n" % os_ns)
        f.write("INTERNAL_OS_NM :%4d\n" % os_nm)
        f.write("INDEX   COS_ANGLE            WEIGHT             USER_ANGLE\n")
        for j in range(len(mu)):
            f.write("%4d " % (j + 1) + fortran_d(mu[j], 21, 14) + fortran_d(ga[j], 21, 14) + " %4d\n" % ind_ang[j])


def write_mie_angles(path, nb_gauss, os_nb, user_file="NO_USER_ANGLES"):
    """`Aer_UsedAngles.txt` (SOS_ANGLES.F:367-376, rows `I4,1X,2D21.14`): the Gauss nodes of the phase-function angle set plus
    the user's angles (weight 0), cosines ascending."""
    x, w = sos_gauss(nb_gauss)
    mu, wt = list(x), list(w)
    if user_file != "NO_USER_ANGLES":
        with open(user_file) as f:
            for line in f:
                if line.strip():
                    val = float(line.split()[0])
                    if val < 0. or val > 90.:
                        raise SosProcError("user angle out of [0,90] in %s" % user_file)
                    mu.append(math.cos(val * math.pi / 180.))
                    wt.append(0.0)
    order = np.argsort(np.asarray(mu), kind="stable")
    with open(path, "w") as f:
        f.write("NB_TOTAL_ANGLES :%4d\n" % len(mu))
        f.write("NB_GAUSS_ANGLES :%4d\n" % nb_gauss)
        f.write("ANGLES_USERFILE :" + user_file.ljust(CTE_LENFIC2) + "\n")
        f.write("INTERNAL_OS_NB :%4d\n" % os_nb)
        f.write("INDEX   COS_ANGLE            WEIGHT\n")
        for i, j in enumerate(order):
            f.write("%4d " % (i + 1) + fortran_d(mu[j], 21, 14) + fortran_d(wt[j], 21, 14) + "\n")


def read_surface_file(path, n, os_nb):
    """A surface reflection-matrix file in the reference's format (what SOS_SURFACE writes and SOS_OS reads, SOS_OS.F:916-925):
    one sequential unformatted record per Fourier order IS = 0..OS_NB holding the nine REAL*4 matrices P11 P12 P13 P21 ...
    P33, each ((R(I,J), I=1,N), J=1,N).  Returns float32 [os_nb+1][9][N][N] (the layout of SosContext(rsurf=...))."""
    want = 9 * n * n * 4
    out = np.zeros((os_nb + 1, 9, n, n), dtype=np.float32)
    with open(path, "rb") as f:
        for s in range(os_nb + 1):
            head = f.read(4)
            if len(head) < 4:
                raise SosProcError("surface file %s: %d records, %d expected (OS_NB + 1)" % (path, s, os_nb + 1))
            nbytes = int(np.frombuffer(head, "<i4")[0])
            if nbytes != want:
                raise SosProcError("surface file %s: record of %d bytes, 9 x %d x %d REAL*4 expected -- made for another "
                                   "angle set?" % (path, nbytes, n, n))
            out[s] = np.frombuffer(f.read(nbytes), "<f4").reshape(9, n, n)
            f.read(4)
    return out


def write_surface_file(path, rsurf):
    """Inverse of read_surface_file (rsurf: float32 [F][9][N][N], e.g. surface.glitter_matrices(...)["rsurf"].cpu())."""
    rsurf = np.ascontiguousarray(rsurf, dtype="<f4")
    with open(path, "wb") as f:
        for s in range(rsurf.shape[0]):
            payload = rsurf[s].tobytes()
            m = np.array([len(payload)], "<i4").tobytes()
            f.write(m + payload + m)


def _dist_rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    return 0, 1


def _shard_range(nb, rank, world):
    from .dist import shard_range
    return shard_range(nb, rank, world)


# Surface reflection matrices of the last few (surface, angles) combinations: they do not depend on the wavelength, so a
# spectrum of calls over one surface computes them once (SOS_SURFACE has the same idea with its SURFACE/ directory of files,
# SOS_SURFACE.F:260-330).  The tensors are read-only after the stream that made them has been synchronised.
_SURF_CACHE = collections.OrderedDict()
_SURF_LOCK = threading.Lock()
_SURF_CACHE_MAX = 8


# The surface matrices of a spectrum chunk, queued ahead of its per-wavelength preparation (_prefetch_surfaces): the table of the
# calling thread, key of _prepare -> (block, slot of its status word).  _surface_cached consults it before the cache above.
_SURF_PREFETCH = threading.local()


def _surface_rule(p, mu, ga, counts, device):
    """The surface checks of the validated keyword set p (SOS_PREPA_OS.F:479-497), then (igli, ifresnel, imat, land, key, job):
    land = the capi.Land of -SURF.Type >= 3, key / job = the _surface_cached key and the surface.surface_job of a computed sea
    or land surface on the angles mu / ga and the counts of _angle_counts, None for -SURF.Type 0 / 2 and for a -SURF.File."""
    from . import surface as _surface
    _, _, os_nb, os_ns, os_nm = counts
    isurf = int(p["isurf"])
    igli, ifresnel, imat = int(isurf == 1), int(isurf == 2), int(isurf == 1 or isurf >= 3)
    land = key = job = None
    if (isurf in (1, 2) or isurf >= 4) and p["surf_ind"] == _D:
        raise SosProcError("-SURF.Ind must be defined for sea surfaces and BPDF models")
    if isurf >= 3:
        if _D in (p["k0_roujean"], p["k1_roujean"], p["k2_roujean"]):
            raise SosProcError("-SURF.Roujean.K0/K1/K2 must be defined for -SURF.Type >= 3")
        if isurf == 6:                                    # the reference's own SOS_PROC refuses it with this message
            raise SosProcError("The Nadal's BPDF model is not supported ==> Select another surface model")
        if isurf == 7 and p["coef_c_maignan"] == _D:
            raise SosProcError("-SURF.Maignan.C must be defined for -SURF.Type 7")
        land = _surface.land_model(isurf, p["k0_roujean"], p["k1_roujean"], p["k2_roujean"], p["alpha_nadal"], p["beta_nadal"],
                                   p["coef_c_maignan"])
    user_surf = str(p["ficsurf"]).strip()
    if imat and user_surf != "DEFAULT":
        # -SURF.File: the user's reflection matrices replace the surface computation (SOS_PROC.F:3186-3189,
        # SOS_PREPA_OS.F:605-658); the direct-beam terms of SOS_TRPHI still follow -SURF.Type
        if not os.path.exists(user_surf):
            raise SosProcError("-SURF.File %s does not exist (SOS_PREPA_OS ERROR_1020)" % user_surf, ier=-1)
    elif isurf == 1:
        if p["wind"] == _D:
            raise SosProcError("-SURF.Glitter.Wind must be defined")
        key = ("glitter", mu.tobytes(), ga.tobytes(), float(p["wind"]), float(p["surf_ind"]), os_nb, os_ns, os_nm, device)
        job = _surface.surface_job(1, wind=p["wind"], ind=p["surf_ind"])
    elif land is not None:
        ind_l = p["surf_ind"] if isurf >= 4 else 1.0
        k0, k1, k2, coef_c = float(land.k0), float(land.k1), float(land.k2), float(land.coef_c)
        key = ("land", isurf, k0, k1, k2, float(land.alpha), float(land.beta), coef_c, mu.tobytes(), ga.tobytes(), float(ind_l),
               os_nb, os_ns, os_nm, device)
        job = _surface.surface_job(isurf, ind=ind_l, k0=k0, k1=k1, k2=k2, coef_c=coef_c)
    return igli, ifresnel, imat, land, key, job


def _surface_request(p, device):
    """(group, key, job) of the surface matrices _prepare will ask for with the validated keyword set p: group = (mu bytes, weight
    bytes, os_nb, os_ns, os_nm), key and job = those of _surface_rule.  None for -SURF.Type 0 / 2, a -SURF.File call, or
    parameters the real pass refuses (it reports)."""
    try:
        counts = _angle_counts(p)
        mu, ga, _, _ = angles(counts[0], p["tetas"], p["ficangles_user_lum"])
        key, job = _surface_rule(p, mu, ga, counts, device)[4:]
        return None if key is None else ((mu.tobytes(), ga.tobytes()) + counts[2:], key, job)
    except Exception:
        return None


def _surface_requests(validated_calls, device=0):
    """The surface batches of a list of validated keyword sets (_validated): one entry per (angle set, os_nb, os_ns, os_nm), in
    order of first appearance -- dict(mu, ga, os_nb, os_ns, os_nm, keys, jobs) with the distinct keys of the group's calls, exactly
    as _prepare forms them, and the surface.surface_job of each.  -SURF.Type 0 / 2 and -SURF.File calls are left out."""
    groups = collections.OrderedDict()
    for p in validated_calls:
        r = _surface_request(p, device) if p is not None else None
        if r is None:
            continue
        g, key, job = r
        e = groups.get(g)
        if e is None:
            e = groups[g] = dict(mu=np.frombuffer(g[0], dtype=np.float64).copy(), ga=np.frombuffer(g[1], dtype=np.float64).copy(),
                                 os_nb=g[2], os_ns=g[3], os_nm=g[4], keys=[], jobs=[])
        if key not in e["keys"]:
            e["keys"].append(key)
            e["jobs"].append(job)
    return list(groups.values())


def _prefetch_surfaces(validated_calls, device):
    """Queues the surface matrices of a chunk's calls on the current stream: one surface.surface_matrices_many call per group of
    _surface_requests (keys the cache already holds are left out), then one pinned copy of all status words and an event.  The
    first _surface_cached that finds its key in the table waits for that event -- the one host wait of the chunk -- after
    which every block is complete for any stream."""
    import torch
    from . import surface as _surface
    groups = _surface_requests(validated_calls, device)
    with _SURF_LOCK:
        for e in groups:
            keep = [k not in _SURF_CACHE for k in e["keys"]]
            e["keys"] = [k for k, ok in zip(e["keys"], keep) if ok]
            e["jobs"] = [j for j, ok in zip(e["jobs"], keep) if ok]
    total = sum(len(e["keys"]) for e in groups)
    if not total:
        return
    dev = torch.device("cuda", device)
    status = torch.zeros(total, dtype=torch.int32, device=dev)
    blocks, pos = {}, 0
    for e in groups:
        nj = len(e["keys"])
        if not nj:
            continue
        try:
            made, _ = _surface.surface_matrices_many(e["jobs"], e["mu"], e["ga"], e["os_nb"], e["os_ns"], e["os_nm"], device=device,
                                                     status=status[pos:pos + nj])
        except Exception:                          # a refused group keeps the per-call path, whose error is the documented one
            made = None
        if made is not None:
            for j, (k, t) in enumerate(zip(e["keys"], made)):
                blocks[k] = (t, pos + j)
        pos += nj
    if not blocks:
        return
    host = torch.empty(total, dtype=torch.int32, pin_memory=True)
    host.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    # keep: a chunk of few surfaces (a spectrum over one surface) hands its blocks on to the cache, so that later chunks hit it
    _SURF_PREFETCH.table = dict(blocks=blocks, status=status, host=host, event=ev, codes=None, keep=total <= _SURF_CACHE_MAX)


def _drop_prefetched_surfaces():
    _SURF_PREFETCH.table = None


def _surface_cached(key, make, device):
    import torch
    pre = getattr(_SURF_PREFETCH, "table", None)
    if pre is not None and key in pre["blocks"]:
        r, slot = pre["blocks"][key]
        if pre["codes"] is None:
            pre["event"].synchronize()
            pre["codes"] = pre["host"].numpy()
        if pre["codes"][slot] != 0:
            from . import surface as _surface
            raise ValueError(_surface.NEGATIVE_ROUJEAN_MESSAGE)
        if pre["keep"]:
            with _SURF_LOCK:
                _SURF_CACHE[key] = r
                while len(_SURF_CACHE) > _SURF_CACHE_MAX:
                    _SURF_CACHE.popitem(last=False)
        return r
    with _SURF_LOCK:
        hit = _SURF_CACHE.get(key)
        if hit is not None:
            _SURF_CACHE.move_to_end(key)
            return hit
    r = make()
    torch.cuda.current_stream(torch.device("cuda", device)).synchronize()
    with _SURF_LOCK:
        _SURF_CACHE[key] = r
        while len(_SURF_CACHE) > _SURF_CACHE_MAX:
            _SURF_CACHE.popitem(last=False)
    return r


class _Plan:
    """One wavelength between its host preparation (_prepare) and its outputs (_finish): the parameters, what the host
    derived from them, the device context and the bins of its band."""


def _trphi_azimuths(itrphi, phios, pas_phi):
    """Azimuth list (radians), table rows and PHI_FIN of the view mode (SOS_TRPHI.F:431-615)."""
    phi_fin = np.zeros(361)
    if itrphi == 1:
        phis = [math.pi + phios * math.pi / 180.0, phios * math.pi / 180.0]
        rows = [0, 1]
        phi_fin[0] = phios            # set to PHIOS+180 then overwritten by PHIOS (SOS_TRPHI.F:445,504)
    elif itrphi == 2:
        iphis = list(range(0, 361, int(pas_phi)))
        phis = [math.pi * ip / 180.0 for ip in iphis]
        rows = list(range(len(iphis)))
        phi_fin[:len(iphis)] = iphis
    else:
        raise SosProcError("-SOS.View must be 1 or 2")
    return phis, rows, phi_fin


def _zero_pages(shape):
    """A large zeroed float64 array on small pages: the fixed-size (361,81) result tables of a spectrum are mostly padding that
    is never written, and numpy asks for transparent huge pages for large blocks -- the first row written into a table would
    then clear 2 MB."""
    import mmap
    nbytes = int(np.prod(shape)) * 8
    if nbytes < (8 << 20) or not hasattr(mmap, "MADV_NOHUGEPAGE"):
        return np.zeros(shape)
    m = mmap.mmap(-1, nbytes)
    try:
        m.madvise(mmap.MADV_NOHUGEPAGE)
    except OSError:
        pass
    return np.frombuffer(m, dtype=np.float64).reshape(shape)


def _trphi_pack(n, mu, out, rows, phi_fin, block=None):
    """sosgpu_trphi's [nphi][7][W] (host array) -> PHI_FIN, THETA_FIN and the fourteen (361,81) tables.
    block: zeroed (2,7,361,81) array to fill (sos_spectrum hands out slices of one allocation per chunk of wavelengths: 3.3 MB
    blocks allocated one by one come from the heap and are cleared by hand, 0.3 ms each; one large block is fresh zero pages)."""
    theta_fin = np.zeros(81)
    theta_fin[:n] = np.degrees(np.arccos(mu))
    names = ["i", "q", "u", "sca", "ang", "rate", "lpol"]       # order of sosgpu_trphi's 7 output rows
    if block is None:
        block = np.zeros((2, 7, 361, 81))                       # the fourteen tables in one allocation
    nr = len(rows)
    if rows != list(range(nr)):
        raise ValueError("azimuth rows must be 0..nr-1")                      # (both view modes of _trphi_azimuths)
    block[0, :, :nr, :n] = out[:nr, :, n + 1:].transpose(1, 0, 2)             # up-going jj = 1..N
    block[1, :, :nr, :n] = out[:nr, :, :n][:, :, ::-1].transpose(1, 0, 2)     # down-going jj = -1..-N
    tabs = {nm: block[0, qi] for qi, nm in enumerate(names)}
    tabs_dn = {nm: block[1, qi] for qi, nm in enumerate(names)}
    return phi_fin, theta_fin, tabs, tabs_dn


def trphi_tables(ctx, rec, nf, tau, tauout, itrphi, phios, pas_phi, igli, wind, land=None):
    """SOS_TRPHI_OPTION (SOS_TRPHI.F:431-615): run the azimuth recomposition on the GPU for the azimuth list of
    the view mode and pack the fourteen (361,81) tables plus PHI_FIN(361), THETA_FIN(81)."""
    phis, rows, phi_fin = _trphi_azimuths(itrphi, phios, pas_phi)
    out = ctx.trphi(rec, nf, tau, tauout, phis, igli=igli, wind=wind, land=land).cpu().numpy()
    return _trphi_pack(ctx.n, ctx.mu, out, rows, phi_fin)


# SOS_AEROSOLS at the REFERENCE wavelength (the first of the two runs SOS_PROC makes when -SOS_Main.Wa differs from -AER.Waref,
# SOS_PROC.F:2893): it depends on the aerosol keywords only, not on the simulation wavelength, so the calls of a spectrum share
# it (the reference recomputes it -- and re-reads its MIE cache file -- in every call).  Keyed by every -AER.* keyword.
_AER_REF_CACHE = collections.OrderedDict()
_AER_REF_LOCK = threading.Lock()


def _aerosols_at_waref(p, nb_mie, os_nb, device):
    from . import aerosols as _aer
    key = tuple((k, p[k]) for _, k, _ in PARAMS if k.startswith(("imod_aer", "rn_", "in_", "igranu", "lnd_", "jd_", "imodele_", "c_wmo_",
                                                                "rh", "mode_param", "user_cv", "rtauct", "bmd_", "ficextdata",
                                                                "ficmixture", "itronc", "waref_aot", "aot_ref"))) + (
        nb_mie, os_nb, device, os.environ.get("SOS_ABS_ROOT", ""))
    with _AER_REF_LOCK:
        hit = _AER_REF_CACHE.get(key)
        if hit is not None:
            _AER_REF_CACHE.move_to_end(key)
            return dict(hit)
    out = _aer.aerosols(p, p["waref_aot"], p["aot_ref"], nb_mie, os_nb, at_waref=True, device=device)
    with _AER_REF_LOCK:
        _AER_REF_CACHE[key] = dict(out)
        while len(_AER_REF_CACHE) > 16:
            _AER_REF_CACHE.popitem(last=False)
    return out


def _validated(kw):
    """The keyword set as _prepare sees it after the parameter checks (a copy with their side effects), or None when they refuse it."""
    try:
        p = dict(kw)
        validate_parameters(p)
        return p
    except Exception:
        return None


def _gas_rule(p):
    """None for -AP.AbsProfile.Type 7, else the gas checks of the validated keyword set p and the arguments of
    absorption.prepa_absprofile (SOS_PREPA_ABSPROFILE, SOS_PROC.F:3359-3416), which absorption.prefetch_gas_tables takes too."""
    absprofil = int(p["absprofil"])
    if absprofil == 7:
        return None
    if int(p["iprofil"]) == 2:                                                     # SOS_PROC.F:2352
        raise SosProcError("-AP.AerProfile.Type 2 requires -AP.AbsProfile.Type 7 (no gas absorption)")
    if p["nustep"] == _I:
        raise SosProcError("-AP.SpectralResol must be defined with -AP.AbsProfile.Type != 7")
    if absprofil == 0 and str(p["ficabsprofil"]).strip() == "NO_USER_ABS_PROFILE_FILE":
        raise SosProcError("-AP.AbsProfile.UserFile must be defined with -AP.AbsProfile.Type 0")
    return (p["wa_simu"], float(p["nustep"]), p["psurf"], p["h2o"], p["o3"], p["co2"], p["ch4"], absprofil,
            str(p["ficabsprofil"]).strip())


def _defers_by_keywords(p, use_gas):
    """The keyword part of "the pass makes the profiles of this call": -AP.AerProfile.Type 1 or 2 (an aerosol layer never has
    gas: ERROR 2513), no -SOS.Trans, -SOS.AbsModeCKD 1 where the call has gas.  (_prepare adds what needs the optical
    thicknesses, the rank split and the table sizes.)"""
    return int(p["iprofil"]) in (1, 2) and str(p["fictrans"]).strip() == "NO_OUTPUT" and \
        (not use_gas or p["imode_ckd_calcul"] == 1)


def _aerosol_rule(p, aer_phase):
    """(use_model, at_wa) of the validated keyword set p: SOS_AEROSOLS runs (aerosols, no given expansion, no -AER.UserFile), and
    it runs a second time at the simulation wavelength (-AER.Waref defined and different from -SOS_Main.Wa, SOS_PROC.F:2893)."""
    use_model = p["aot_ref"] != 0.0 and aer_phase is None and str(p["ficuser_aer"]).strip() == "NO_USER_AEROSOLS"
    if use_model and p["imod_aer"] not in (0, 1, 2, 3, 4, 5):
        raise SosProcError("-AER.Model must be in 0..5")
    return use_model, use_model and p["waref_aot"] != _D and p["wa_simu"] != p["waref_aot"]


def _gas_table_request(p):
    """The arguments of the SOS_PREPA_ABSPROFILE call _prepare will make for the validated keyword set p (_gas_rule), or None when
    the call has no gas absorption or its parameters are refused (the real pass reports)."""
    try:
        return _gas_rule(p)
    except Exception:
        return None


def _gas_tables_on_device(p):
    """True when, as far as the validated keyword set p tells, _prepare will defer the profiles of this gas call (the rest of its
    rule needs the optical thicknesses)."""
    try:
        return _defers_by_keywords(p, True)
    except Exception:
        return False


def _aerosol_call(p, aer_phase):
    """(p, nb_mie, os_nb) of the SOS_AEROSOLS run _prepare will make at the simulation wavelength for the validated keyword set p,
    or None when that step does not run or its parameters are refused (the real pass reports)."""
    try:
        if not _aerosol_rule(p, aer_phase)[1]:
            return None
        _, nb_mie, os_nb, _, _ = _angle_counts(p)
        return p, nb_mie, os_nb
    except Exception:
        return None


def _size_integral_requests(call, device):
    """The size integrals the aerosol run `call` (_aerosol_call) will ask for (keys of aerosols.prefetch_size_integrals)."""
    from . import aerosols as _aer
    try:
        p, nb_mie, os_nb = call
        with _aer.collect_size_integrals() as reqs:
            _aer.aerosols(p, p["wa_simu"], 0.1, nb_mie, os_nb, at_waref=False, device=device)
        return reqs
    except Exception:
        return []


# Host time of the segments of _prepare, summed over the calls (seconds; filled when SOS_PREPARE_SEGMENTS is set -- diagnostic of
# scripts/hyperspectral_bench.py): segment name -> time since the previous mark of the same call.
PREPARE_SEGMENTS = collections.OrderedDict() if os.environ.get("SOS_PREPARE_SEGMENTS") else None
_SEG_LAST = [0.0]


def _seg(name):
    if PREPARE_SEGMENTS is None:
        return True
    import time
    t = time.perf_counter()
    if name is not None:
        PREPARE_SEGMENTS[name] = PREPARE_SEGMENTS.get(name, 0.0) + t - _SEG_LAST[0]
    _SEG_LAST[0] = t
    return True


if PREPARE_SEGMENTS is not None:
    from . import solver as _solver_mod
    _solver_mod.SEG = _seg


def _profiles_deferrable(tr, hr, ta, ha):
    """True when sosgpu_profile_spectrum takes this wavelength: the argument rules of sosgpu_profile hold and its no-gas grid
    fits CTE_OS_NT levels.  A wavelength that fails here keeps the per-wavelength path, whose error is the documented one."""
    from . import capi
    try:
        ok = float(hr) > 0.0 and float(ha) > 0.0 and float(tr) >= 0.0 and float(ta) >= 0.0
        return bool(ok) and capi.lib().sosgpu_profile_nogas_levels(float(tr), float(ta)) >= 1
    except Exception:
        return False


def _layer_deferrable(tr, hr, ta, zmin, zmax):
    """True when sosgpu_profile_layer_spectrum takes this aerosol layer: its level grid exists (geometry.layer_grid, the closed
    forms the library states too).  A layer that fails here keeps the per-wavelength path, which raises the grid's refusal."""
    if os.environ.get("SOS_LAYER_PROFILE_HOST"):
        return False
    try:
        return float(hr) > 0.0 and float(tr) > 0.0 and layer_grid(tr, hr, ta, float(zmin), float(zmax))[0] >= 1
    except Exception:
        return False


def _prepare_checks(pl):
    """The parameter checks the hot path depends on (SOS_PROC.F:1310-2700 has many more; same messages' intent)."""
    p = pl.p
    if p["wa_simu"] == _D:
        raise SosProcError("-SOS_Main.Wa must be defined")
    if p["tetas"] == _D or not (0.0 <= p["tetas"] < 90.0):
        raise SosProcError("-ANG.Thetas must be defined in [0,90[")
    pl.iprofil = int(p["iprofil"])
    if pl.iprofil not in (1, 2):                                                   # SOS_PROC.F:2324-2325
        raise SosProcError("-AP.AerProfile.Type must be 1 or 2")
    if pl.iprofil == 2 and (p["zmin"] == _D or p["zmax"] == _D):                   # :2335-2338
        raise SosProcError("-AP.AerLayer.Zmin and -AP.AerLayer.Zmax must be defined for -AP.AerProfile.Type 2")
    pl.absprofil = int(p["absprofil"])
    if pl.absprofil == _I or not 0 <= pl.absprofil <= 7:
        raise SosProcError("-AP.AbsProfile.Type must be defined in 0..7")
    if p["isurf"] not in (0, 1, 2, 3, 4, 5, 6, 7):
        raise SosProcError("-SURF.Type must be in 0..7")
    if p["rho"] == _D:
        raise SosProcError("-SURF.Alb must be defined")
    if p["aot_ref"] == _D:
        raise SosProcError("-AER.AOTref must be defined")
    pl.use_model, pl.aer_at_wa = _aerosol_rule(p, pl.aer_phase)
    if p["hr"] == _D:
        raise SosProcError("-AP.HR must be defined")
    pl.itrphi = p["itrphi"]
    if pl.itrphi == 1 and p["phios"] == _D:
        raise SosProcError("-SOS.View.Phi must be defined for -SOS.View 1")
    if pl.itrphi == 2 and p["pas_phi"] == _I:
        raise SosProcError("-SOS.View.Dphi must be defined for -SOS.View 2")
    pl.igmax = CTE_DEFAULT_IGMAX if p["igmax"] == _I else int(p["igmax"])


def _prepare_angles(pl):
    """SOS_ANGLES (SOS_PROC.F:2738)."""
    pl.nb_lum, pl.nb_mie, pl.os_nb, pl.os_ns, pl.os_nm = _angle_counts(pl.p)
    pl.mu, pl.ga, pl.n0, pl.ind_ang = angles(pl.nb_lum, pl.p["tetas"], pl.p["ficangles_user_lum"])
    pl.n = len(pl.mu)


def _prepare_aerosols(pl, aer_stream, aer_at_wa):
    """Aerosols: none, a user Aerosols.txt (-AER.UserFile, SOS_PROC.F:2883-2934: SOS_AEROSOLS is not run, the file is read by
    SOS_PREPA_OS.F:666-700), or a given expansion (stands for SOS_AEROSOLS -> Aerosols.txt)."""
    import torch
    p, device = pl.p, pl.device
    pl.coef_tronca_out = None
    ta_model = None
    if pl.use_model:
        # SOS_AEROSOLS at the reference wavelength, and again at the simulation wavelength when they differ: the optical
        # thickness scales with the extinction cross sections (SOS_PROC.F:2883-3060)
        from . import aerosols as _aer
        if p["waref_aot"] == _D:
            raise SosProcError("-AER.Waref must be defined")
        import contextlib
        try:
            with (torch.cuda.stream(aer_stream) if aer_stream is not None else contextlib.nullcontext()):
                pl.aer_phase = _aerosols_at_waref(p, pl.nb_mie, pl.os_nb, device)
                ta_model = float(p["aot_ref"])
                if pl.aer_at_wa:
                    k_ref = pl.aer_phase["kmat1"]
                    pl.aer_phase = (aer_at_wa if aer_at_wa is not None else
                                    _aer.aerosols(p, p["wa_simu"], 0.1, pl.nb_mie, pl.os_nb, at_waref=False, device=device))
                    ta_model = (pl.aer_phase["kmat1"] / k_ref) * p["aot_ref"]
        except _aer.AerosolError as e:
            raise SosProcError(str(e), ier=-1)
        pl.coef_tronca_out = pl.aer_phase["coef_tronca"]
    elif p["aot_ref"] != 0.0 and pl.aer_phase is None:
        user_aer = str(p["ficuser_aer"]).strip()
        if not os.path.exists(user_aer):
            raise SosProcError("-AER.UserFile %s not found" % user_aer)
        pl.aer_phase = read_aerosols_file(user_aer, pl.os_nb)
        pl.coef_tronca_out = 0.0       # COEF_TRONCA is an output of SOS_AEROSOLS only: untouched (0) with a user file
    if p["aot_ref"] == 0.0 or pl.aer_phase is None:
        pl.ta = 0.0
        pl.phase = (np.zeros(pl.os_nb + 1),) * 4
        pl.piz, pl.piztr, pl.a_tronc = 0.0, 0.0, 0.0
    else:
        pl.ta = float(p["aot_ref"]) if ta_model is None else ta_model
        pl.phase = tuple(np.asarray(pl.aer_phase[k], dtype=np.float64) for k in ("alpha", "beta", "gamma", "zeta"))
        if len(pl.phase[1]) != pl.os_nb + 1:
            raise SosProcError("aer_phase arrays must have OS_NB+1 = %d entries" % (pl.os_nb + 1))
        pl.piz, pl.piztr = float(pl.aer_phase["piz"]), float(pl.aer_phase["piztr"])
        pl.a_tronc = float(pl.aer_phase.get("a_tronc", 0.0))
        if pl.iprofil == 1 and p["ha"] == _D:
            raise SosProcError("-AP.AerHS.HA must be defined")


def _prepare_thickness(pl, defer_profiles):
    """The molecular optical thickness (SOS_PROC.F:3331-3351), whether the pass makes the profiles, else their head start."""
    p = pl.p
    pl.tr = p["tr"]
    if pl.tr == _D:
        if p["psurf"] == _D:
            raise SosProcError("-AP.MOT or -AP.Psurf must be defined")
        pl.tr = rayleigh_optical_thickness(p["wa_simu"], p["psurf"])
    pl.ha = p["ha"] if pl.ta else 1.0
    pl.zout = float(p["zout"])
    # head start: the level placement of the wavelength's no-gas profile (a ~1 ms serial chain on one wavefront) is queued now and
    # runs while the host prepares gas tables, surface and context (a refused profile is reported by make_profiles below)
    pl.nogas = None
    pl.defer = bool(defer_profiles) and _defers_by_keywords(p, pl.absprofil != 7) and \
        (_profiles_deferrable(pl.tr, p["hr"], pl.ta, pl.ha) if pl.iprofil == 1 else
         _layer_deferrable(pl.tr, p["hr"], pl.ta, p["zmin"], p["zmax"]))
    if pl.iprofil == 1 and not pl.defer:
        try:
            from .solver import nogas_profile
            pl.nogas = nogas_profile(pl.tr, p["hr"], pl.ta, pl.ha, pl.device)
        except Exception:
            pl.nogas = None


def _prepare_gas(pl, shard_bins, device_gas_tables):
    """Gas absorption: SOS_PREPA_ABSPROFILE + the weights of the CKD bins (SOS_PROC.F:3359-3416); gas = (ik, aik, xk, ro_lay)."""
    from . import absorption as _abs
    request = _gas_rule(pl.p)
    pl.use_gas, pl.prep, pl.gas = request is not None, None, None
    if pl.use_gas:
        try:
            pl.prep = prep = _abs.prepa_absprofile(*request)
            ik, aik, _ = _abs.bins(prep)
            # (a sharded band; more levels than the kernels hold: the error is make_profiles')
            pl.defer = pl.defer and not (_dist_rank_world()[1] > 1 and shard_bins or len(prep["altabs"]) > 64 or not len(aik))
            if pl.defer and device_gas_tables and len(prep["altabs"]) == _abs.NLEVEL:
                xk, ro_lay = None, _abs.layer_ro(prep)                              # xk: made on the device, for the whole part
            else:
                xk, ro_lay = _abs.layer_tables(prep)
            pl.gas = (ik, aik, xk, ro_lay)
        except _abs.AbsorptionError as e:
            raise SosProcError(str(e), ier=-1)
    pl.mode_ckd = int(pl.p["imode_ckd_calcul"])
    if pl.mode_ckd not in (1, 2):
        raise SosProcError("-SOS.AbsModeCKD must be 1 or 2")


def _prepare_surface(pl):
    """The surface (_surface_rule) and its reflection matrices: a -SURF.File, or computed once per key (_surface_cached)."""
    from . import surface as _surface
    p, mu, ga, device = pl.p, pl.mu, pl.ga, pl.device
    os_nb, os_ns, os_nm = pl.os_nb, pl.os_ns, pl.os_nm
    pl.igli, pl.ifresnel, pl.imat, pl.land, key, job = _surface_rule(p, mu, ga, (pl.nb_lum, pl.nb_mie, os_nb, os_ns, os_nm), device)
    lta = pl.ta == 0.0 or pl.piztr == 0.0                                            # SOS.F:541-550: IBORM = 2 without aerosols
    pl.iborm = min(2, os_nb) if lta else os_nb
    rsurf = None
    if key is None:
        if pl.imat:                                                                  # -SURF.File
            import torch
            rsurf = torch.as_tensor(read_surface_file(str(p["ficsurf"]).strip(), pl.n, os_nb), device=torch.device("cuda", device))
    elif pl.igli:
        rsurf = _surface_cached(key, lambda: _surface.glitter_matrices(mu, ga, p["wind"], p["surf_ind"], os_nb, os_ns, os_nm,
                                                                        device=device)["rsurf"], device)
    else:
        try:
            rsurf = _surface_cached(key, lambda: _surface.land_matrices(pl.land, mu, ga, job["ind"], os_nb, os_ns, os_nm,
                                                                        device=device), device)
        except ValueError as e:
            raise SosProcError(str(e), ier=-1)
    if rsurf is not None and pl.iborm < os_nb:
        rsurf = rsurf[:pl.iborm + 1].contiguous()
    pl.rsurf = rsurf


def _prepare_context(pl, defer_operators, order0=False, defer_context=False):
    """The device context of the wavelength (SOS_PREPA_OS), unbuilt where the pass builds the operators of a whole part.
    defer_context: the context is left pending (SosContext(create=False)) where nothing in _prepare needs its handle -- a call
    that defers its profiles (pl.defer: _prepare_profiles then reads ctx.smax alone) and its operators; the pass makes the
    contexts of a whole part in one call (_stage_contexts).
    order0 (the irradiance pass): the context holds the Fourier order 0 alone -- iborm_max = 0, record 0 of the surface
    matrices (formed as they are: an order-limited sosgpu_surface_batch does not exist) -- and the profile stage, which takes
    the highest order from it, gives every bin iborm = 0."""
    from .solver import SosContext
    p = pl.p
    if order0:
        pl.iborm = 0
        if pl.rsurf is not None:
            pl.rsurf = pl.rsurf[:1].contiguous()
    isurf = int(p["isurf"])
    alpha, beta, gamma, zeta = pl.phase
    pl.want_trans = str(p["fictrans"]).strip() != "NO_OUTPUT"
    build = not (defer_operators and not pl.want_trans)
    pl.ctx = SosContext(pl.mu, pl.ga, pl.n0, alpha, beta, gamma, zeta, iborm_max=pl.iborm, ro=p["rho"], imat_surf=pl.imat,
                        ifresnel=pl.ifresnel, ind_surf=p["surf_ind"] if isurf in (1, 2) or isurf >= 4 else 1.34, ron=MDF_DEFAULT,
                        ipolar=int(p["ipolar"]), igmax=pl.igmax, rsurf=pl.rsurf, device=pl.device,
                        build=build, create=not (defer_context and pl.defer and not build))
    pl.tdifmug = None
    # (_spectrum_pass with trans: the plan's rows of the part's diffuse_transmissions_many; a scalar block that came from the host)
    pl.trans_rows = None
    pl.host_scal = False


def _layer_profile(pl, true_depth):
    """The single profile of an aerosol layer between -AP.AerLayer.Zmin and Zmax (-AP.AerProfile.Type 2, no gas): on the device
    (SosContext.make_layer_profile), after the refusals of its level grid.  SOS_LAYER_PROFILE_HOST=1 (environment, for A/B
    timing and as the checker): made on the host by geometry.profile_layer and uploaded.  Returns its bins."""
    p, zout = pl.p, pl.zout
    if not os.environ.get("SOS_LAYER_PROFILE_HOST"):
        from .solver import layer_lp
        nt = layer_grid(pl.tr, p["hr"], pl.ta, float(p["zmin"]), float(p["zmax"]))[0]
        try:
            return pl.ctx.make_layer_profile(pl.tr, p["hr"], pl.ta, float(p["zmin"]), float(p["zmax"]), a_tronc=pl.a_tronc,
                                             piz=pl.piz, piztr=pl.piztr, zout=zout, lp=layer_lp(nt), true_depth=bool(true_depth))
        except Exception as e:
            raise SosProcError("SOS_PROFILE: %s" % e, ier=-1)
    h, xdel, ydel, zprof = profile_layer(pl.tr, p["hr"], pl.ta, float(p["zmin"]), float(p["zmax"]))
    ttot_vrai = h[-1]
    h_kw = dict(hvrai=np.array(h, dtype=np.float64)[None]) if true_depth else {}   # H before the rescale
    h, xdel, ydel, ib = rescale_profile(h, xdel, ydel, pl.a_tronc, pl.piz, pl.piztr, pl.os_nb)   # SOS.F:523-550
    bins = pl.ctx.upload_bins(h[None], xdel[None], ydel[None], iborm=np.array([min(ib, pl.iborm)], dtype=np.int32),
                              zout=zout, zprof=zprof[None], **h_kw)
    if zout == -1.0:
        tauout = h[0]                                                        # SOS.F:567-568
    else:
        j = int(bins["jout"][0])
        zzv = float(bins["zz"][0])
        tauout = (1 - zzv) * h[j - 1] + zzv * h[j]                           # SOS.F:572-581
    bins["scal"] = np.array([[0.0, h[-1], ttot_vrai, tauout]])
    return bins


def _band_profiles(pl, shard_bins, true_kw):
    """The profiles of the CKD bins of a gas band that this call makes itself.  Several GPUs (torch.distributed initialised, one
    process per GPU): the bins of the band are dealt to the ranks by cost (dist.balanced_shards); solve_band's one all-reduce
    joins them and every rank returns the same 23 outputs.  A rank may hold no bin at all.  (-SOS.AbsModeCKD 2 has a single
    bin: not sharded.)"""
    from . import absorption as _abs
    ctx = pl.ctx
    ik, aik, xk, ro_lay = pl.gas
    rank, world = _dist_rank_world() if shard_bins else (0, 1)
    pl.band_sharded = world > 1 and pl.mode_ckd != 2
    tabs_last = None
    if pl.band_sharded:
        from . import dist as _dist
        tabs_last = ctx.absorption_profiles(ik[-1:], xk, ro_lay)             # TAUABS of the band's last bin (Flux file)
        mine = _dist.balanced_shards(_abs.bin_costs(ik, xk, ro_lay, pl.tr + pl.ta), world)[rank]
        ik, aik = ik[mine], aik[mine]
    tabs = ctx.absorption_profiles(ik, xk, ro_lay) if len(aik) else None     # SOS_ABSPROFILE of every bin of this rank
    if pl.mode_ckd == 2:
        # one profile from the band-mean transmission of every level (SOS_PROC.F:3609-3676)
        tb = tabs.cpu().numpy()
        trs = np.zeros(tb.shape[1])
        for b in range(tb.shape[0]):
            trs = trs + aik[b] * np.exp(-tb[b])
        tabs = np.maximum(-np.log(trs), 0.0)[None]
        aik = np.ones(1)
    try:
        if len(aik):
            pl.bins = ctx.make_profiles(len(aik), pl.tr, pl.p["hr"], pl.ta, pl.ha, pl.prep["altabs"], tabs, a_tronc=pl.a_tronc,
                                        piz=pl.piz, piztr=pl.piztr, zout=pl.zout, absprofil=pl.absprofil, nogas=pl.nogas,
                                        **true_kw)
        else:
            pl.bins = dict(nb=0, scal=None)
    except Exception as e:
        raise SosProcError("SOS_PROFILE: %s" % e, ier=-1)
    pl.aik = aik
    pl.tabs_flux = tabs_last if pl.band_sharded else tabs


def _prepare_profiles(pl, shard_bins, true_depth):
    """The CKD bin loop (SOS_PROC.F:3459-3594): profiles of every bin on the device, or profile_request, what
    solver.make_profiles_spectrum needs of a deferred wavelength.  band_sharded: every rank holds a slice of the band and the
    partials are all-reduced; tabs_flux: TAUABS of the band's last bin (Flux file), host array or [.][nlev] device tensor."""
    import torch
    p, ctx = pl.p, pl.ctx
    pl.band_sharded, pl.tabs_flux, pl.profile_request = False, None, None
    common = dict(tr=pl.tr, hr=p["hr"], ta=pl.ta, ha=pl.ha, a_tronc=pl.a_tronc, piz=pl.piz, piztr=pl.piztr, zout=pl.zout,
                  smax=ctx.smax)
    true_kw = dict(true_depth=True) if true_depth else {}      # (split=False: the calls as they were)
    if pl.defer and not pl.use_gas and pl.iprofil == 2:
        # (an aerosol layer: the request of solver.make_layer_profiles_spectrum -- `ha` has no meaning there)
        from .solver import layer_lp
        pl.profile_request = dict(common, zmin=float(p["zmin"]), zmax=float(p["zmax"]), layer=True,
                                  lp=layer_lp(layer_grid(pl.tr, p["hr"], pl.ta, float(p["zmin"]), float(p["zmax"]))[0]))
        pl.bins, pl.aik = None, np.ones(1)
    elif pl.defer and not pl.use_gas:
        pl.profile_request = dict(common, ik=None, absprofil=7)
        pl.bins, pl.aik = None, np.ones(1)
    elif pl.defer:
        ik, pl.aik, xk, ro_lay = pl.gas
        pl.profile_request = dict(common, ik=ik, xk=xk, ro=ro_lay, altabs=pl.prep["altabs"], absprofil=pl.absprofil)
        if xk is None:
            pl.profile_request["prep"] = pl.prep
        pl.bins = None
    elif not pl.use_gas and pl.iprofil == 1:
        # the single no-gas profile of the wavelength: SOS_PROFILE, the PROFIL-file round trip, the rescale, IBORM and the
        # output level all inside sosgpu_profile (the Python restatement profile_nogas costs 2-3 ms and stays as the checker
        # of tests/test_profile.py)
        try:
            pl.bins = ctx.make_profiles(1, pl.tr, p["hr"], pl.ta, pl.ha, None, None, a_tronc=pl.a_tronc, piz=pl.piz,
                                        piztr=pl.piztr, zout=pl.zout, absprofil=7, nogas=pl.nogas, **true_kw)
        except Exception as e:
            raise SosProcError("SOS_PROFILE: %s" % e, ier=-1)
        pl.aik = np.ones(1)
    elif not pl.use_gas:
        pl.bins, pl.aik = _layer_profile(pl, true_depth), np.ones(1)
    else:
        _band_profiles(pl, shard_bins, true_kw)
    bins = pl.bins
    if pl.want_trans and bins is not None and bins["nb"]:                            # SOS.F:600-635
        tdifmus_b, pl.tdifmug = ctx.diffuse_transmissions(bins)
        sc = bins["scal"] if hasattr(bins["scal"], "clone") else torch.from_numpy(np.asarray(bins["scal"])).to(ctx.device)
        sc = sc.clone()
        sc[:, 0] = tdifmus_b
        bins["scal"] = sc


def _prepare(kw, aer_phase=None, device=0, shard_bins=True, aer_stream=None, aer_at_wa=None, defer_profiles=False,
             device_gas_tables=False, defer_operators=False, true_depth=False, order0=False, defer_context=False):
    """Everything of one SOS_PROC call up to the CKD bin loop (SOS_PROC.F:1310-3458): parameter checks, SOS_ANGLES,
    SOS_AEROSOLS, SOS_SURFACE, SOS_PREPA_ABSPROFILE, SOS_PREPA_OS, and the profiles of every bin of the band on the device
    (SOS_ABSPROFILE + SOS_PROFILE + the rescale of SOS).  Every stage fills its fields of the _Plan that comes back, whose `ctx`
    the caller closes; what one decides from the keywords alone stands in the rule functions the prefetch's predictors read too.
    shard_bins: with torch.distributed initialised, keep only this rank's slice of the band's bins (sos_proc); False: the
    whole band stays on this rank (sos_spectrum distributes wavelengths, not bins).
    aer_stream: HIP stream (torch.cuda.Stream) for the aerosol step, whose device calls are host-synchronous -- sos_spectrum keeps
    them off the streams its asynchronous work is queued on.
    aer_at_wa: the result of SOS_AEROSOLS at the simulation wavelength when sos_spectrum has formed it already (aerosols_many).
    defer_profiles (_spectrum_pass only): a call that qualifies -- no -SOS.Trans, -SOS.AbsModeCKD 1 or no gas, band not sharded
    -- gets no profile launches here: the plan comes back with `bins` None and `profile_request`, the request
    solver.make_profiles_spectrum takes (for an aerosol layer: solver.make_layer_profiles_spectrum), and the pass makes the
    profiles of a whole part in three launches (the layers: one more).
    device_gas_tables (with defer_profiles): a deferred gas wavelength hands over its `prep` instead of the layer tables xk --
    COEFF_ABS_CKD then runs on the device for the whole part (sosgpu_ckd_layer_tables) and absorption.layer_tables not at all.
    true_depth (the levels calls with split=True): the bins also carry `hvrai`, the cumulative optical depth of every level
    before the truncation rescale (SosContext.make_profiles(true_depth=True); the aerosol-layer profile uploads its own).
    defer_operators (_spectrum_pass only): the context comes back unbuilt (SosContext(build=False)) and the pass fills the
    operator tables of a whole part in one solver.build_operators call -- unless this function uses the operators itself, which
    only a -SOS.Trans call does (diffuse_transmissions in _prepare_profiles).
    order0 (the irradiance mode of _spectrum_pass only): the context and the bins hold the Fourier order 0 alone
    (_prepare_context).
    defer_context (_spectrum_pass only): a call that defers both its profiles and its operators comes back with a PENDING context
    (SosContext(create=False)): nothing here needs its handle, and the pass creates the contexts of a whole part in one
    solver.create_contexts call.  Every other call makes its own sosgpu_create, as sos_proc does."""
    _seg(None)
    missing = [k for k in SOS_PROC_KWARGS if k not in kw]
    if missing:
        raise TypeError("sos_proc() missing keyword arguments: %s" % ", ".join(missing))
    pl = _Plan()
    pl.p, pl.device, pl.aer_phase = dict(kw), device, aer_phase
    validate_parameters(pl.p)
    _prepare_checks(pl)
    _seg('checks')
    _prepare_angles(pl)
    _seg('angles')
    _prepare_aerosols(pl, aer_stream, aer_at_wa)
    _seg('aerosols')
    _prepare_thickness(pl, defer_profiles)
    _prepare_gas(pl, shard_bins, device_gas_tables)
    _seg('gas tables')
    _prepare_surface(pl)
    _seg('surface')
    _prepare_context(pl, defer_operators, **(dict(order0=True) if order0 else {}),
                     **(dict(defer_context=True) if defer_context else {}))
    _seg('context')
    try:
        _prepare_profiles(pl, shard_bins, true_depth)
    except BaseException:
        pl.ctx.close()
        raise
    _seg('profiles')
    return pl


def _trphi_launch(pl, rec0, nf, tau, tauout):
    """Queue SOS_TRPHI for the azimuths of the view mode; returns the device tensor [nphi][7][W] (no synchronisation)."""
    phis, pl.rows, pl.phi_fin = _trphi_azimuths(pl.itrphi, pl.p["phios"], pl.p["pas_phi"])
    return pl.ctx.trphi(rec0, nf, tau, tauout, phis, igli=pl.igli, wind=pl.p["wind"] if pl.igli else 0.0, land=pl.land)


def _trphi_launch_many(jobs):
    """_trphi_launch for the jobs [(pl, rec0, nf, tau, tauout)] of a chunk or of the altitudes of a band: ONE launch
    (solver.trphi_many, sosgpu_trphi_spectrum) for all of them.  Returns the flat device tensor of the results and the shapes
    [nphi][7][W] of its blocks, in job order (no synchronisation).  SOS_SPECTRUM_TRPHI_PER_CALL=1 (environment, for A/B timing):
    one sosgpu_trphi launch per job, concatenated."""
    import torch
    from . import solver
    if os.environ.get("SOS_SPECTRUM_TRPHI_PER_CALL"):
        outs = [_trphi_launch(pl, rec0, nf, tau, tauout) for pl, rec0, nf, tau, tauout in jobs]
        return torch.cat([o.reshape(-1) for o in outs]), [tuple(o.shape) for o in outs]
    items = []
    for pl, rec0, nf, tau, tauout in jobs:
        phis, pl.rows, pl.phi_fin = _trphi_azimuths(pl.itrphi, pl.p["phios"], pl.p["pas_phi"])
        items.append((pl.ctx, rec0, nf, tau, tauout, phis, pl.igli, pl.p["wind"] if pl.igli else 0.0, pl.land))
    flat, views = solver.trphi_many(items)
    return flat, [tuple(v.shape) for v in views]


def _level_flux_row(pl, alt, fin, g, e):
    """One row of LEVEL_FLUX_NAMES for output altitude `alt` (km, -1 = the standard output) of plan pl: e = (E-, E+) of
    sosgpu_level_flux for that altitude's aggregated record, fin / g its finish_scalars dictionary and segment.  The direct term
    is formed as _finish forms tdir_tronc: exp(-tau / cos(theta_s)) of the truncated optical depth down to the altitude (the
    whole column for -1, where the down-going columns refer to the ground and the up-going one to the top of the atmosphere)."""
    cs = math.cos(math.pi * pl.p["tetas"] / 180.0)
    tau = float(fin["ttot_tronc"][g]) if alt == -1.0 else float(fin["tauout"][g])
    tdir = math.exp(-tau / cs)
    em, ep = float(e[0]), float(e[1])
    tot = em + tdir
    return (tdir, em, tot, ep, tot - ep)


def _level_flux_split_row(pl, alt, fin, g, e):
    """One row of LEVEL_FLUX_SPLIT_NAMES: _level_flux_row's five columns, then the split of the down-going flux as _finish
    forms it at the ground (SOS_PROC.F:3831-3837), at the altitude: flux_dir_down = exp(-tau_vrai / cos(theta_s)) of the
    UNTRUNCATED optical depth down to the altitude (fin["tauvrai_out"]; the whole column, fin["ttot_vrai"], for -1) and
    flux_diff_down = E- + tdir_tronc - flux_dir_down.  The two sum to flux_tot_down to within two roundings of it."""
    row = _level_flux_row(pl, alt, fin, g, e)
    cs = math.cos(math.pi * pl.p["tetas"] / 180.0)
    tau = float(fin["ttot_vrai"][g]) if alt == -1.0 else float(fin["tauvrai_out"][g])
    tdir_vrai = math.exp(-tau / cs)
    return row + (tdir_vrai, float(e[0]) + row[0] - tdir_vrai)


def _level_absorption_row(alt, a):
    """One row of LEVEL_ABSORPTION_NAMES for output altitude `alt` from a = the band sums (a_dir, a_dn, a_up, q) of
    sosgpu_level_absorption: the three parts of the actinic flux, their sum (down-going and up-going diffuse first, then the
    direct beam, the order the kernel adds them in per bin), and the absorbed power per km.  The standard output (altitude -1)
    mixes the ground and the top of the atmosphere: its row is NaN."""
    if alt == -1.0:
        return (float("nan"),) * len(LEVEL_ABSORPTION_NAMES)
    a_dir, a_dn, a_up, q = (float(x) for x in a)
    return (a_dir, a_dn, a_up, a_dn + a_up + a_dir, q)


def _finish_scalars(pl, fin, g=0):
    """Elements 18..22 of the 23-tuple of plan pl (SOS_PROC.F:3831-3837): flux_dir_down, flux_diff_down, flux_tot_down,
    flux_diff_up and coef_tronca, from the finish_scalars dictionary `fin` and the wavelength's segment g in it."""
    cs = math.cos(math.pi * pl.p["tetas"] / 180.0)
    tau_agg, ttot_vrai_agg = float(fin["ttot_tronc"][g]), float(fin["ttot_vrai"][g])
    emoins, eplus = float(fin["emoins"][g]), float(fin["eplus"][g])
    tdir_tronc = math.exp(-tau_agg / cs)                                          # SOS_PROC.F:3831-3837
    tdir_vrai = math.exp(-ttot_vrai_agg / cs)
    flux_diff_down = emoins + tdir_tronc - tdir_vrai
    flux_down = emoins + tdir_tronc
    return tdir_vrai, flux_diff_down, flux_down, eplus, pl.a_tronc if pl.coef_tronca_out is None else pl.coef_tronca_out


def _finish(pl, out, rec0, fin, g=0, block=None):
    """The tail of SOS_PROC (SOS_PROC.F:3755-3874) on the host: the (361,81) tables from sosgpu_trphi's output `out` (host
    array), fluxes, result files (rank 0 only), the 23-tuple.  rec0: aggregated records [S][3][W] of this wavelength
    (device); fin: dist.finish_scalars dictionary, g the wavelength's segment in it."""
    p, n, mu = pl.p, pl.n, pl.mu
    nf = int(fin["n_orders"][g])
    tau_agg, ttot_vrai_agg = float(fin["ttot_tronc"][g]), float(fin["ttot_vrai"][g])
    phi_fin, theta_fin, up, dn = _trphi_pack(n, mu, out, pl.rows, pl.phi_fin, block)
    from . import absorption as _abs
    resbin = str(p["ficsos_res_bin"]).strip()
    resroot = str(p["resroot"]).strip() if getattr(pl, "writes_files", _dist_rank_world()[0] == 0) else ""
    if resroot:                                   # SOS_PROC.F:1342-1500: results under RESROOT/SOS
        os.makedirs(os.path.join(resroot, "SOS"), exist_ok=True)
        # the two angle files SOS_ANGLES always writes (SOS_ANGLES.F:367-376, 494-506)
        write_mie_angles(os.path.join(resroot, "SOS", str(p["ficangles_res_mie"]).strip()), pl.nb_mie, pl.os_nb,
                         str(p["ficangles_user_mie"]).strip())
        write_used_angles(os.path.join(resroot, "SOS", str(p["ficangles_res_lum"]).strip()), mu, pl.ga, pl.n0, pl.ind_ang,
                          pl.nb_lum, p["tetas"], pl.os_nb, pl.os_ns, pl.os_nm, str(p["ficangles_user_lum"]).strip())
        if pl.use_model:
            write_aerosols_file(os.path.join(resroot, "SOS", str(p["ficgranu"]).strip()), pl.aer_phase, pl.aer_phase["kmat1"],
                                pl.aer_phase["kmat2"])
        elif p["aot_ref"] == 0.0:                 # SOS_AEROSOLS writes an all-zero file for an aerosol-free run
            z = np.zeros(pl.os_nb + 1)
            write_aerosols_file(os.path.join(resroot, "SOS", str(p["ficgranu"]).strip()),
                                dict(alpha=z, beta=z, gamma=z, zeta=z, a_tronc=0.0, piztr=0.0, piz=0.0))
        write_result_bin(os.path.join(resroot, "SOS", resbin), rec0[:nf].cpu().numpy())
    tdir_vrai, flux_diff_down, flux_down, eplus, coef_tronca = _finish_scalars(pl, fin, g)
    if resroot and pl.want_trans:
        write_trans_file(os.path.join(resroot, "SOS", str(p["fictrans"]).strip()), p["tetas"], mu, tau_agg, ttot_vrai_agg,
                         float(fin["tdifmus"][g]), fin["tdifmug"][g])
    if resroot and str(p["ficflux"]).strip() != "NO_OUTPUT":
        tl = pl.tabs_flux
        tabs_flux = np.zeros(_abs.NLEVEL) if tl is None else (tl[-1].cpu().numpy() if hasattr(tl, "cpu") else np.asarray(tl)[-1])
        zal = pl.prep["userprofil"][:, 0] if pl.use_gas else np.linspace(0., 0., _abs.NLEVEL)
        write_flux_file(os.path.join(resroot, "SOS", str(p["ficflux"]).strip()), p["tetas"], tdir_vrai, flux_diff_down, flux_down,
                        eplus, zal, pl.tr, p["hr"], pl.ta, pl.ha, tabs_flux)
    ind_angout = np.zeros(81, dtype=np.int32)
    ind_angout[:n] = pl.ind_ang
    return (n, ind_angout, phi_fin, theta_fin,
            up["sca"], up["i"], up["q"], up["u"], up["ang"], up["rate"], up["lpol"],
            dn["sca"], dn["i"], dn["q"], dn["u"], dn["ang"], dn["rate"], dn["lpol"],
            tdir_vrai, flux_diff_down, flux_down, eplus, coef_tronca)


def sos_proc(aer_phase=None, device=0, **kw):
    """Drop-in for `sos.sos_proc(**kwargs)` (f2py of SOS_PROC, SOS_PROC.F:415) on the MI355X hot path.
    Returns the reference's 23-tuple (names in OUTPUT_NAMES).

    aer_phase (extension, not a reference keyword): dict(alpha, beta, gamma, zeta [OS_NB+1 each], piz, piztr,
    a_tronc) -- the content of the reference's Aerosols.txt when `-AER.AOTref` > 0 (bypasses the Mie / size-distribution
    step).  With torch.distributed initialised the call is a collective: the band's CKD bins are sharded over the ranks
    (one all-reduce) and every rank returns the same outputs."""
    return _band_call("sos_proc", kw, aer_phase, device)[0]


def _band_call(fn, kw, aer_phase, device, alts=None, fluxes=False, split=False, absorption=False):
    """One band for sos_proc (alts None: solve_band, the kernels without output slots) or sos_proc_levels (alts: the K
    altitudes, solve_band_levels): prepare, let the ranks agree on an error flag, solve, SOS_TRPHI and _finish per output.
    Returns the list of 23-tuples (one without alts); with fluxes (alts only) the pair (that list, flux rows [K][5], or
    [K][7] with split: the bins then carry the untruncated depth rows and the aggregates their band transmission); with
    absorption (fluxes only) the triple (..., rows [K][5] of LEVEL_ABSORPTION_NAMES: one more launch behind the aggregates)."""
    import torch
    from . import solver
    from .solver import SosBinError
    pl, levels, err = None, None, None
    try:
        pl = _prepare(kw, aer_phase, device, shard_bins=True, **(dict(true_depth=True) if split else {}))
        if alts is not None:
            try:
                levels = pl.ctx.output_levels(pl.bins, alts)
            except BaseException:
                pl.ctx.close()
                raise
    except Exception as e:                         # noqa: BLE001 -- re-raised below, after the ranks have agreed
        err = e
    if _dist_rank_world()[1] > 1:
        # A failure that strikes one rank only (device memory, a HIP error) must not leave the others waiting in the band's
        # all-reduce: the ranks agree on an error flag first (one integer, MAX).  Parameter errors are the same on every rank.
        bad = _first_failed_index(-1 if err is None else 0, device) >= 0
        if bad and err is None:
            pl.ctx.close()
            raise SosProcError("%s: another rank failed while preparing this call" % fn, ier=-1)
    if err is not None:
        raise err
    try:
        # one fused solve of the band's bins, one aggregate per output (+ the all-reduce of a sharded band)
        try:
            if alts is None:
                rec, fin = pl.ctx.solve_band(pl.bins, pl.aik, tdifmug=pl.tdifmug, reduce=pl.band_sharded)
            else:
                ab = [] if absorption else None
                rec, fin = pl.ctx.solve_band_levels(pl.bins, levels, pl.aik, tdifmug=pl.tdifmug, reduce=pl.band_sharded,
                                                    **(dict(absorption=ab) if absorption else {}))
        except SosBinError as e:
            raise SosProcError(str(e), ier=-1)
        if alts is None:                           # sos_proc: the single call
            outs = [_trphi_launch(pl, rec[k], int(fin["n_orders"][k]), float(fin["ttot_tronc"][k]), float(fin["tauout"][k]))
                    .cpu().numpy() for k in range(len(rec))]
        else:                                      # the K altitudes in one launch, one download
            if fluxes:                             # (one more launch for the K flux pairs, on the reduced records)
                flux_dev = solver.level_flux_many([(pl.ctx, rec[k]) for k in range(len(rec))])
                if absorption:                     # (its block [K][4] comes down with the flux pairs)
                    flux_dev = torch.cat([flux_dev, ab[0]], dim=1)
            flat, shapes = _trphi_launch_many([(pl, rec[k], int(fin["n_orders"][k]), float(fin["ttot_tronc"][k]),
                                                float(fin["tauout"][k])) for k in range(len(rec))])
            outs = solver._flat_blocks(flat.cpu().numpy(), shapes)
        tuples = [_finish(pl, outs[k], rec[k], fin, k) for k in range(len(rec))]
        if not fluxes:
            return tuples
        e = flux_dev.cpu().numpy()                 # (complete: it was queued ahead of the recompositions just downloaded)
        row = _level_flux_split_row if split else _level_flux_row
        flux = np.array([row(pl, alts[k], fin, k, e[k]) for k in range(len(rec))], dtype=np.float64)
        if not absorption:
            return tuples, flux
        return tuples, flux, np.array([_level_absorption_row(alts[k], e[k][2:6]) for k in range(len(rec))], dtype=np.float64)
    finally:
        pl.ctx.close()


def _levels_arguments(fn, altitudes, kwargs_list, fluxes=False, split=False, absorption=False):
    """The argument rules of the output-slot entry points, checked before any device work: 1 to 16 altitudes, each passing the
    -SOS.OutputAlt rule (SosProcError 2611), and calls with zout = -1 and no -SOS_Main.ResRoot (ValueError).  Returns the
    altitudes as floats.  fluxes, split, absorption: the entry point's flags, bools, split and absorption only with fluxes;
    absorption not in a channel pass, nor on a band whose bins are sharded over ranks (ValueError)."""
    from . import capi
    if not isinstance(fluxes, (bool, np.bool_)):
        raise ValueError("%s: fluxes must be True or False, got %r" % (fn, fluxes))
    if not isinstance(split, (bool, np.bool_)):
        raise ValueError("%s: split must be True or False, got %r" % (fn, split))
    if split and not fluxes:
        raise ValueError("%s: split=True adds columns to the flux rows: it needs fluxes=True" % fn)
    if not isinstance(absorption, (bool, np.bool_)):
        raise ValueError("%s: absorption must be True or False, got %r" % (fn, absorption))
    if absorption and not fluxes:
        raise ValueError("%s: absorption=True returns its rows behind the flux rows: it needs fluxes=True" % fn)
    if absorption and fn == "sos_spectrum_channels":
        raise ValueError("%s: absorption=True is not available for sensor channels: the absorbed power is formed per CKD bin "
                         "and returned per call (use sos_spectrum_levels and weight its rows)" % fn)
    if absorption and fn == "sos_proc_levels" and _dist_rank_world()[1] > 1:
        raise ValueError("%s: absorption=True is not available for a band whose bins are sharded over ranks: the absorbed "
                         "power is a per-bin product that does not pass through the band's all-reduce (run the call on one "
                         "rank, or deal whole wavelengths with sos_spectrum_levels)" % fn)
    alts = [float(z) for z in altitudes]
    if not 1 <= len(alts) <= capi.MAX_OUTPUT_LEVELS:
        raise ValueError("%s: 1 to %d altitudes, got %d" % (fn, capi.MAX_OUTPUT_LEVELS, len(alts)))
    for kw in kwargs_list:
        if float(kw.get("zout", -1.0)) != -1.0:
            raise ValueError("%s: the altitudes are given by `altitudes`; zout must be -1" % fn)
        if str(kw.get("resroot", "")).strip():
            raise ValueError("%s writes no result files: -SOS_Main.ResRoot must be empty (use sos_proc)" % fn)
    for z in alts:                                 # the -SOS.OutputAlt rule of validate_parameters
        if (z < 0.0 and z != -1.0) or z > CTE_TOA_ALT:
            e = SosProcError("SOS_PROC : ERROR_2611 on parameters -- -SOS.OutputAlt must be -1 (standard levels) or within "
                             "[0, %g] km (got %g)" % (CTE_TOA_ALT, z))
            e.code = 2611
            raise e
    return alts


def sos_proc_levels(altitudes, aer_phase=None, device=0, fluxes=False, split=False, absorption=False, **kw):
    """sos_proc for several output altitudes (-SOS.OutputAlt, km; -1 = the standard TOA / ground output) at once: ONE
    profile, context and solve, whose K output slots capture the field at each altitude (sosgpu_os_solve_levels), then
    one aggregate and SOS_TRPHI per altitude.  Returns a list of K 23-tuples in the order of `altitudes`; element k equals
    sos_proc(aer_phase, device, **{**kw, "zout": altitudes[k]}) bit for bit.
    1 <= K <= 16, duplicates allowed; each altitude must pass the -SOS.OutputAlt rule (SosProcError 2611, raised before any
    device work).  kw is sos_proc's keyword set with zout = -1 (another zout: ValueError) and no -SOS_Main.ResRoot (result
    files stay sos_proc's: ValueError).  Under torch.distributed the call is a collective as sos_proc is: the bins are
    sharded and one all-reduce covers the K record sets.

    fluxes=True (a bool, ValueError otherwise, before any device work): returns (tuples, flux) with flux a numpy array [K][5],
    the irradiances at each altitude z in units of the incident solar irradiance on a horizontal plane, columns
    LEVEL_FLUX_NAMES: flux_dir_down_tronc = exp(-tauout / cos(theta_s)) of the truncated optical depth down to z;
    flux_diff_down_tronc = E-(z) and flux_diff_up = E+(z), the reference's EMOINS / EPLUS quadrature (SOS_OS.F:1447-1456) of
    the order-0 intensity captured at z (sosgpu_level_flux_spectrum: the K pairs in one launch on the aggregated -- under
    torch.distributed reduced -- records, every rank computing them); flux_tot_down, the sum of the first two, which does not
    depend on the truncation; flux_net = flux_tot_down - flux_diff_up.  For altitude -1 the down-going columns refer to the
    ground (direct term exp(-ttot_tronc / cos(theta_s))) and flux_diff_up to the top of the atmosphere: the row restates
    elements 20 and 21 of that altitude's 23-tuple (to rounding; with surface matrices, -SURF.Type 1 and 3..7, flux_diff_up
    agrees with element 21 to some 1e-9 only, as the reference's EPLUS and its own record do); its flux_net, ground minus top,
    is the net flux of no altitude (the net flux at the ground takes flux_diff_up of the 0 km row, that at the top flux_tot_down
    of the 120 km row).  With the default the return value, the launches and the bits are unchanged.

    split=True (a bool, and only with fluxes=True: ValueError otherwise, before any device work): flux is [K][7], columns
    LEVEL_FLUX_SPLIT_NAMES -- the five above, unchanged, then the split of the down-going flux into the TRUE direct beam and the
    TRUE diffuse light at z, which elements 18 and 19 of the tuple give at the ground only (SOS_PROC.F:3831-3837):
    flux_dir_down = exp(-tau_vrai(z) / cos(theta_s)) and flux_diff_down = E-(z) + flux_dir_down_tronc - flux_dir_down, with
    tau_vrai(z) the UNTRUNCATED optical depth down to z (the whole column for -1: that row restates elements 18 and 19).  The
    profile stage exports the depth of every level before the truncation rescale (sosgpu_profile_true), the depth at z is
    taken from it as TAUOUT is from the rescaled one (sosgpu_output_depths), and the band value -ln sum aik exp(-tau_vrai)
    comes from one more launch behind the aggregates (sosgpu_level_transmission), inside the existing all-reduce and download.
    Convention: the depth at z is the reference's own LINEAR interpolation between the two profile levels that bracket z,
    the one it uses for TAUOUT and for the field.  In a strongly absorbing CKD bin (gas depth above 1.5) everything below
    the limit altitude is ONE layer, and the interpolated depth there is far from the analytic one (up to 1.3 in optical
    depth in such a bin of the O2 A band): that is the reference's resolution at such altitudes, kept so that
    flux_dir_down + flux_diff_down equals flux_tot_down.  Without forward-peak truncation (a_tronc = 0) flux_dir_down equals
    flux_dir_down_tronc.

    absorption=True (a bool, and only with fluxes=True: ValueError otherwise, before any device work): returns (tuples, flux,
    absorb) with absorb a numpy array [K][5], columns LEVEL_ABSORPTION_NAMES, in the unit of the flux columns (relative to the
    irradiance mu_s E0 at the top of the atmosphere on a horizontal plane): the actinic flux at z -- 4 pi x the mean intensity,
    the moment of the captured order-0 field WITHOUT the weight mu -- as actinic_dir (the direct beam,
    sum aik exp(-tauout_b / mu_s) / mu_s), actinic_diff_down and actinic_diff_up (the two hemispheres of the diffuse field) and
    actinic_tot, their sum; and absorbed_per_km, the radiative power absorbed per kilometre at z,
    sum aik (1 - omega_b(z)) (dtau_b / dz) A_b(z): the shortwave heating rate up to the factor mu_s E0 / (rho c_p).  The
    absorbed power of a CKD band is not linear in the aggregated record, so one launch behind the aggregates
    (sosgpu_level_absorption) forms the products per bin and sums them with aik; its block comes down with the flux pairs.
    Conventions: omega and the field are interpolated linearly between the two profile levels that bracket z, as the reference
    interpolates the field, and dtau / dz is the slope of the layer between them, so that absorbed_per_km at the middle of a
    layer times its thickness is the layer's net-flux divergence F_net(top) - F_net(bottom) (to some 1e-4 away from the two
    layers next to the top and to the ground).  The truncation rescale leaves (1 - omega) dtau unchanged: absorbed_per_km
    belongs to the true atmosphere.  actinic_dir of a band of several bins is the exact band mean of the bins' direct beams,
    not flux_dir_down_tronc / mu_s, which the reference forms from the band-mean depth; the two agree for one bin.  The row of
    altitude -1 (ground and top of the atmosphere mixed) is NaN.  Not available for a band whose bins are sharded over ranks
    (ValueError: the per-bin products do not pass through the all-reduce).  With the default the return value, the launches
    and the bits are unchanged."""
    alts = _levels_arguments("sos_proc_levels", altitudes, [kw], fluxes, split, absorption)
    return _band_call("sos_proc_levels", kw, aer_phase, device, alts, bool(fluxes), bool(split), bool(absorption))


def sos_proc_many(kwargs_list, n_workers=8, device=0):
    """A spectrum of independent sos_proc calls (one per wavelength: the reference runs them one after the other,
    binding/run_sos.py:640): the list interface of sos_spectrum -- identical outputs to the sequential loop, bit for bit.
    Round 2 issued the calls from `n_workers` host threads with a HIP stream each; the Python host work under the interpreter
    lock bounded that form at 1.3 x the plain loop (and below it once the calls became cheaper).  Now: one host thread, the
    preparation kernels of the wavelengths spread over `n_workers` streams, all bins of all wavelengths in one launch per
    kernel variant (sos_spectrum).  Give each call its own `-SOS_Main.ResRoot` when result files are wanted (the file names
    inside are fixed, as in the reference).  Export GPU_MAX_HW_QUEUES=16 before the first GPU call.  Returns the list of
    23-tuples in order; a failing call raises its exception."""
    return sos_spectrum(kwargs_list, device=device, prep_streams=max(1, int(n_workers)))


# ---------------------------------------------------------------------------------------------------------
# A whole spectrum through the drop-in (BASELINE config 5: hyperspectral runs)
# ---------------------------------------------------------------------------------------------------------
_TABLE_NAMES = (4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)     # the fourteen (361,81) tables of the 23-tuple


def _compact_outputs(t, nrow):
    """A 23-tuple without the zero padding of its fixed-size tables (what travels between ranks): the (361,81) tables cut to
    the `nrow` azimuth rows and N columns in use."""
    n = int(t[0])
    return tuple(np.ascontiguousarray(x[:nrow, :n]) if i in _TABLE_NAMES else x for i, x in enumerate(t)) + (nrow,)


def _expand_outputs(c, block=None):
    """block: zeroed (14, 361, 81) array for the tables (a slice of one allocation per gather, _zero_pages)."""
    nrow = c[-1]
    out = []
    t = 0
    for i, x in enumerate(c[:-1]):
        if i in _TABLE_NAMES:
            full = np.zeros((361, 81)) if block is None else block[t]
            t += 1
            full[:nrow, :x.shape[1]] = x
            out.append(full)
        else:
            out.append(x)
    return tuple(out)


def _gather_results(results, mine, nrows, world, nz=None, flux=None, trans=None, absorb=None):
    """Every rank receives the 23-tuples of the wavelengths the other ranks computed (all_gather_object of the compacted
    tuples; the only exchange of a wavelength-partitioned spectrum).  nz: every result is a list of nz 23-tuples (output
    altitudes) instead of one tuple.  flux: the per-wavelength flux rows of sos_spectrum_levels(fluxes=True), which travel with
    the compact tuples and are filled in the same way.  trans: the per-wavelength transmission entries
    (transmissions=True), which travel and are filled like the flux rows; absorb: the rows of absorption=True, likewise."""
    import torch.distributed as dist
    per = 1 if nz is None else nz
    part = [(i, [_compact_outputs(t, nrows[i]) for t in ([results[i]] if nz is None else results[i])]) for i in mine]
    extras = [x for x in (flux, trans, absorb) if x is not None]
    if extras:
        part = [(i, (cs,) + tuple(x[i] for x in extras)) for i, cs in part]
    parts = [None] * world
    dist.all_gather_object(parts, part)
    if extras:
        for pr in parts:
            for i, row in pr:
                for x, v in zip(extras, row[1:]):
                    if x[i] is None:
                        x[i] = v
        parts = [[(i, row[0]) for i, row in pr] for pr in parts]
    todo = [(i, cs) for pr in parts for i, cs in pr if results[i] is None]
    blocks = _zero_pages((len(todo) * per, len(_TABLE_NAMES), 361, 81)) if todo else None
    for j, (i, cs) in enumerate(todo):
        full = [_expand_outputs(c, blocks[j * per + k]) for k, c in enumerate(cs)]
        results[i] = full[0] if nz is None else full


def spectrum_costs(kwargs_list):
    """Relative cost of every call of a spectrum, from its keywords alone (no aerosol, surface or profile work): number of CKD
    bins of the spectral interval (product of the gases' exponential-term counts, read from the CKD table headers -- 1 without
    gas absorption or in -SOS.AbsModeCKD 2) x dist.bin_cost of the wavelength's scattering optical depth (Rayleigh formula +
    -AER.AOTref) and a moderate gas column.  Used to deal the wavelengths to the ranks."""
    from . import absorption as _abs
    from .dist import bin_cost
    costs = np.zeros(len(kwargs_list))
    for i, kw in enumerate(kwargs_list):
        nb = 1
        try:
            if int(kw["absprofil"]) != 7 and int(kw["imode_ckd_calcul"]) == 1:
                nb = _abs.band_bin_count(kw["wa_simu"], float(kw["nustep"]))
        except Exception:               # a call that will fail in validation costs nothing; the error is raised by its owner
            nb = 1
        tr = kw.get("tr", _D)
        if tr == _D:
            tr = rayleigh_optical_thickness(kw["wa_simu"], kw["psurf"]) if kw.get("psurf", _D) != _D and kw.get("wa_simu", _D) != _D else 0.1
        ta = kw.get("aot_ref", 0.0)
        ta = 0.0 if ta == _D else ta
        norders = 3 if ta == 0.0 else 40          # Fourier orders: 3 for a molecular atmosphere (IBORM = 2), tens with aerosols
        costs[i] = nb * float(bin_cost(tr + ta, 0.5 if nb > 1 else 0.0)) * norders
    return costs


def _spectrum_prefetch(kwargs_list, aer_phases, idx, device, aer_st, device_gas_tables=False, batch_surfaces=False):
    """The shared host work of a spectrum chunk `idx`, queued ahead of its per-wavelength preparation: the size-distribution
    integrals (aerosols.prefetch_size_integrals), the gas tables interpolated to the layers in one pass, and SOS_AEROSOLS at the
    simulation wavelength of each call.  Returns {index: aerosols at the simulation wavelength} for _prepare(aer_at_wa=...).
    device_gas_tables: the calls whose profiles _prepare can defer as far as the keywords alone tell (_defers_by_keywords) get
    their layer tables from the device, so the one-pass host interpolation leaves them out; a call _prepare then does not defer
    after all interpolates its own tables there.
    batch_surfaces: the sea and land surface matrices of the chunk's calls are queued first, one sosgpu_surface_batch per angle
    set (_prefetch_surfaces); they run on the device while the host does the rest of this function."""
    import torch
    from . import aerosols as _aer
    from . import absorption as _abs
    valid = {i: v for i, v in ((i, _validated(kwargs_list[i])) for i in idx) if v is not None}
    if batch_surfaces:
        _prefetch_surfaces(list(valid.values()), device)
    # the size-distribution integrals of the chunk's wavelengths, queued ahead (aerosols.prefetch_size_integrals)
    acalls = {i: c for i, c in ((i, _aerosol_call(v, aer_phases[i])) for i, v in valid.items()) if c is not None}
    reqs = []
    for c in acalls.values():
        reqs += _size_integral_requests(c, device)
    if reqs:
        with torch.cuda.stream(aer_st):
            _aer.prefetch_size_integrals(reqs)
    # ... and the gas tables of the chunk's wavelengths, interpolated to the layers in one pass
    greqs = [(r, v) for r, v in ((_gas_table_request(v), v) for v in valid.values()) if r is not None]
    if greqs:
        on_device = [r for r, v in greqs if device_gas_tables and _gas_tables_on_device(v)]
        _abs.prefetch_gas_tables([r for r, _ in greqs], device_tables=on_device)
    # ... and SOS_AEROSOLS at the simulation wavelength of each, the Legendre expansions formed together (the gas tables
    # above were made while the size integrals ran)
    aer_wa = {}
    by_angles = collections.OrderedDict()
    for i, (pp, nbm, nbo) in acalls.items():
        by_angles.setdefault((nbm, nbo), []).append((i, pp))
    for (nbm, nbo), members in by_angles.items():
        with torch.cuda.stream(aer_st):
            res = _aer.aerosols_many([(pp, pp["wa_simu"], 0.1) for _, pp in members], nbm, nbo, device=device)
        for (i, _), r in zip(members, res):
            if r is not None:
                aer_wa[i] = r
    return aer_wa


def _first_failed_index(index, device):
    """Ranks agree on a failure (one integer, MAX): the largest wavelength index any rank failed at (index -1: this rank did not
    fail; a band call passes 0 for a failure), or -1."""
    import torch
    import torch.distributed as dist
    on_gpu = dist.get_backend() == "nccl"
    t = torch.tensor([int(index)], dtype=torch.int64, device=torch.device("cuda", device) if on_gpu else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return int(t.item())


class _Chunk:
    """What the stages of one chunk of _spectrum_pass hand to each other: `plans` (every plan prepared, closed by the driver),
    `solved` [(plans, rec [K][nw][S][3][W], scal [K][nw][10+N], table)] device tensors per launch, `salb_bands` [(plans, their
    band spherical albedos [len(plans)], a device tensor)], `ckd_checks` [(status tensor of a part's device gas tables, the
    plans it speaks of)], `absorb` (absorption=True: parallel to `solved`, the device blocks [K][len(plans)][4] of
    sosgpu_level_absorption) and `where`, the wavelength being worked on (named by a failure)."""


def _part_bounds(n, parts, min_part):
    """The (s0, s1) bounds of the parts a chunk of n wavelengths goes to the solver in: at most `parts` equal steps, as long
    as n holds min_part wavelengths for each."""
    nsub = max(1, min(int(parts), n // max(1, int(min_part))))
    step = max(1, -(-n // nsub))
    return [(s0, min(s0 + step, n)) for s0 in range(0, n, step)]


def _stage_prepare(fn, ch, kwargs_list, aer_phases, device, idx, s0, s1, side, aer_st, aer_wa, alts, true_kw, batch_profiles,
                   device_tables, batch_operators, debug, batch_contexts=False):
    """The calls idx[s0:s1] of a chunk prepared on the side streams (_prepare; output_levels of the calls that have their
    bins).  Returns the plans of the part.  batch_contexts: the calls that can wait for it leave their context to
    _stage_contexts (the keyword reaches _prepare only then, so that the calls are as they were without it)."""
    import torch
    part = []
    for k, i in enumerate(idx[s0:s1], s0):
        ch.where = i
        with torch.cuda.stream(side[k % len(side)]):
            pl = _prepare(kwargs_list[i], aer_phases[i], device, shard_bins=False, aer_stream=aer_st,
                          aer_at_wa=aer_wa.get(i), defer_profiles=batch_profiles, device_gas_tables=device_tables,
                          defer_operators=batch_operators, **(dict(defer_context=True) if batch_contexts else {}), **true_kw)
            pl.writes_files = True
            pl.index = i
            ch.plans.append(pl)
            if alts is not None and pl.bins is not None:
                pl.levels = pl.ctx.output_levels(pl.bins, alts)
        if debug:
            torch.cuda.synchronize(torch.device("cuda", device))
            print("[%s] prepared" % fn, i, flush=True)
        part.append(pl)
    return part


def _stage_contexts(ch, part, fn="sos_spectrum", debug=False):
    """The contexts of the part's calls that _prepare left pending (defer_context: the calls that defer both their profiles and
    their operators): ONE solver.create_contexts call on the main stream -- one staged copy, one launch, no host wait -- where
    every such call made a sosgpu_create that waited for its copy.
    Ordering: the fill of a context's block is queued on the main stream, so whatever reads the block must come behind it on
    that stream.  Between _stage_prepare and _stage_operators nothing queued on a side stream does: what _prepare queues there
    for a pending call is the upload of its surface matrices and its aerosol work, neither of which touches the context (a
    pending context has no handle to pass); _stage_profiles and the output levels behind it run on the main stream, after this
    stage; _stage_operators, the first reader of the small tables, runs on the main stream after the main stream has waited for
    the side streams.  The blocks come from the pool, which holds only blocks whose last work has been waited for.
    debug (SOS_SPECTRUM_DEBUG): the main stream is waited for and the calls whose contexts were made are printed."""
    from . import capi, solver
    pending = [pl for pl in part if pl.ctx._pending is not None]
    if not pending:
        return
    ch.where = pending[0].index
    _seg(None)
    try:
        solver.create_contexts([pl.ctx for pl in pending])
    except Exception as e:
        for pl in pending:           # a refused call is named: the one whose spec the library's query refuses on its own
            if not capi.lib().sosgpu_create_spectrum_work_bytes(pl.ctx._pending, 1):
                ch.where = pl.index
                break
        raise SosProcError("SOS_PREPA_OS: %s" % e, ier=getattr(e, "ier", -1))
    _seg("stage: contexts")
    if debug:
        import torch
        torch.cuda.current_stream(pending[0].ctx.device).synchronize()
        print("[%s] contexts of wavelengths" % fn, [pl.index for pl in pending], flush=True)


def _stage_profiles(ch, part, alts, level_keys, true_kw, dev):
    """The profiles of the part's qualifying wavelengths: three launches for all their bins (the operators the side streams
    are still building are not needed for them), one more for the output slots.  The aerosol layers among them are made by a
    call of their own (solver.make_layer_profiles_spectrum: one launch), with output slots of their own -- one call per row
    length (solver.layer_lp: layers below 32, below 64 levels, the others), which is one where the layers of a part are alike."""
    import functools
    from . import solver
    waiting = [pl for pl in part if pl.bins is None]
    _stage_profiles_of(ch, [pl for pl in waiting if not pl.profile_request.get("layer")], solver.make_profiles_spectrum, alts,
                       level_keys, true_kw, dev)
    for lp in sorted({pl.profile_request["lp"] for pl in waiting if pl.profile_request.get("layer")}):
        _stage_profiles_of(ch, [pl for pl in waiting if pl.profile_request.get("layer") and pl.profile_request["lp"] == lp],
                           functools.partial(solver.make_layer_profiles_spectrum, lp=lp), alts, level_keys, true_kw, dev)


def _stage_profiles_of(ch, deferred, make, alts, level_keys, true_kw, dev):
    """_stage_profiles for the calls one table-form profile call `make` covers."""
    if not deferred:
        return
    ch.where = deferred[0].index
    info = {}
    try:
        made = make([pl.profile_request for pl in deferred], dev, part=info, **true_kw)
    except Exception as e:
        if info.get("bad") is not None:
            ch.where = deferred[info["bad"]].index
        raise SosProcError("SOS_PROFILE: %s" % e, ier=-1)
    if info.get("ckd_status") is not None:
        ch.ckd_checks.append((info["ckd_status"], [deferred[g] for g in info["ckd_index"]]))
    lv = None if alts is None else deferred[0].ctx.output_levels(info["bins"], alts)
    for g, pl in enumerate(deferred):
        # (views of the part's blocks: the plans keep them alive until the chunk's streams are synchronised)
        pl.bins, pl.tabs_flux, pl.profile_part = made[g], info["tabs"][g], info
        if lv is not None:
            b0, b1 = int(info["seg"][g]), int(info["seg"][g + 1])
            pl.levels = dict(nz=lv["nz"], **{k: lv[k][:, b0:b1] for k in level_keys})


def _stage_operators(ch, part):
    """The operators of the part's unbuilt contexts, grouped and single alike (after the driver's wait for the side streams:
    the surface matrices come from them)."""
    from . import solver
    unbuilt = [pl for pl in part if not pl.ctx._built]
    if unbuilt:
        ch.where = unbuilt[0].index
        solver.build_operators([pl.ctx for pl in unbuilt])


def _stage_transmissions(ch, part, salb, dev):
    """trans: the diffuse transmissions of every bin of the part: one call per direction count, whatever the calls are (it
    reads the contexts' order-0 operators, queued by _stage_operators or by the side streams waited for); salb: next to it
    the spherical albedo of the same bins."""
    import torch
    from . import solver
    by_n = collections.OrderedDict()
    for pl in part:
        if pl.bins["nb"]:
            by_n.setdefault(pl.n, []).append(pl)
    for gp in by_n.values():
        ch.where = gp[0].index
        tbins, tcob = solver.concat_profiles([pl.bins for pl in gp])
        tdifmus, tdifmug = solver.diffuse_transmissions_many([pl.ctx for pl in gp], tbins, tcob)
        b0 = 0
        for pl in gp:
            b1 = b0 + pl.bins["nb"]
            pl.trans_rows = tdifmug[b0:b1]
            sc = pl.bins["scal"]                 # TDIFMUS into column 0, as _prepare does for -SOS.Trans
            if not isinstance(sc, torch.Tensor):
                pl.host_scal = True              # (a host profile: the call stays with the singles)
                sc = pl.bins["scal"] = solver._dev_f64(np.asarray(sc), dev)
            sc[:, 0] = tdifmus[b0:b1]
            b0 = b1
        if salb:
            # the spherical albedo of the same bins seen from the ground, and its aik-weighted sum per call
            s_bin, _ = solver.spherical_albedo_many([pl.ctx for pl in gp], tbins, tcob)
            seg = np.concatenate([[0], np.cumsum([pl.bins["nb"] for pl in gp])]).astype(np.int32)
            aik = solver._dev_f64(np.concatenate([np.asarray(pl.aik, dtype=np.float64) for pl in gp]), dev)
            ch.salb_bands.append((gp, solver.albedo_band(seg, aik, s_bin)))


def _group_key(pl):
    """What the calls one launch covers agree in (the last entry is False throughout with output slots: their calls have
    zout = -1)."""
    b = pl.bins
    return (pl.n, pl.ctx.smax, pl.ctx.os_nb, bool(pl.ctx._rsurf is not None), b["lp"], b["jout"] is not None)


def _part_groups(part):
    """The groups of wavelengths one launch can cover: (groups, singles), the lists of two or more plans of equal _group_key
    in first-appearance order of the key, and the calls solved alone -- those with their own transmissions, without bins or
    with host scalars, in part order, then the one-member groups in key order."""
    import torch
    groups = collections.OrderedDict()
    single = []
    for pl in part:
        b = pl.bins
        if pl.tdifmug is not None or b["nb"] == 0 or not isinstance(b.get("scal"), torch.Tensor) or pl.host_scal:
            single.append(pl)
            continue
        groups.setdefault(_group_key(pl), []).append(pl)
    single += [gp[0] for gp in groups.values() if len(gp) == 1]
    return [gp for gp in groups.values() if len(gp) > 1], single


def _stage_solves(fn, ch, groups, single, solve_group, solve_single, alts, level_keys, dev, debug):
    """The solves of a part, queued on the main stream: one per group, then one per single call; each adds its entry to
    ch.solved."""
    import torch
    from . import solver
    for gp in groups:
        ch.where = gp[0].index
        table = solver.ContextTable([pl.ctx for pl in gp])
        bins, cob, seg = solver.concat_bins([pl.bins for pl in gp])
        aik = solver._upload(torch.from_numpy(np.concatenate([np.asarray(pl.aik, dtype=np.float64) for pl in gp])), dev)
        if debug:
            print("[%s] group" % fn, _group_key(gp[0]), "wavelengths", [pl.index for pl in gp], "bins", bins["nb"], flush=True)
        rec, scal = solve_group(table, gp, bins, cob, seg, aik)
        if debug:
            torch.cuda.synchronize(dev)
            print("[%s]   done" % fn, flush=True)
        ch.solved.append((gp, rec, scal, table))
    for pl in single:
        ch.where = pl.index
        if alts is not None and pl.levels["jout"] is not None and not pl.levels["jout"].is_contiguous():
            pl.levels = dict(pl.levels, **{k: pl.levels[k].contiguous() for k in level_keys})
        rec, scal = solve_single(pl)
        ch.solved.append(([pl], rec, scal, None))


def _stage_flux_launch(ch, nz):
    """fluxes: the flux pairs of every (wavelength, altitude) of the chunk: one launch behind the aggregates, in the order of
    _stage_todo's list; the result comes down with the recompositions'.  absorption: the blocks [K][calls][4] of ch.absorb, put
    into that order, ride behind the pairs as columns 2..5."""
    import torch
    from . import solver
    flux_dev = solver.level_flux_many([(pl.ctx, rec[k][g]) for gp, rec, _, _ in ch.solved
                                       for g, pl in enumerate(gp) for k in range(nz)])
    if ch.absorb:
        flux_dev = torch.cat([flux_dev, torch.cat([a.transpose(0, 1).reshape(-1, 4) for a in ch.absorb])], dim=1)
    return flux_dev


def _split_scalars(scal_all, shapes, n_alb, n_status):
    """The host array of _download_scalars taken apart by its layout: shapes, the (nz, len(gp), sw) of every solved entry;
    n_alb, the length of every salb_bands entry; n_status, that of every ckd_checks entry.  Returns (the reshaped scalar
    blocks, one array per albedo group, one per status group), views of scal_all; ValueError if the sizes do not add up."""
    from . import solver
    cuts = list(shapes) + [(n,) for n in n_alb] + [(n,) for n in n_status]
    if sum(math.prod(c) for c in cuts) != scal_all.size:
        raise ValueError("the packed scalars hold %d values, their sections %s add up to %d"
                         % (scal_all.size, cuts, sum(math.prod(c) for c in cuts)))
    out = solver._flat_blocks(scal_all, cuts)
    a, b = len(shapes), len(shapes) + len(n_alb)
    return out[:a], out[a:b], out[b:]


def _download_scalars(ch, nz):
    """The chunk's one copy of all band scalars (waits for the solves), and the only statement of its layout: the scalar
    blocks of ch.solved, in order; then the band spherical albedos of ch.salb_bands; then the status words of the device gas
    tables of ch.ckd_checks (as float64).  Returns what _split_scalars makes of it."""
    import torch
    scal_all = torch.cat([s.reshape(-1) for _, _, s, _ in ch.solved] + [s for _, s in ch.salb_bands] +
                         [s.to(torch.float64) for s, _ in ch.ckd_checks]).cpu().numpy()
    return _split_scalars(scal_all, [(nz, len(gp), s.shape[2]) for gp, _, s, _ in ch.solved],
                          [len(gp) for gp, _ in ch.salb_bands], [len(pls) for _, pls in ch.ckd_checks])


def _check_ckd_status(ch, status):
    """The status words of the chunk's device gas tables: a wavelength COEFF_ABS_CKD failed for raises sos_proc's error."""
    from . import absorption as _abs
    for (_, pls), codes in zip(ch.ckd_checks, status):
        for pl, code in zip(pls, codes):
            if code != 0:                           # COEFF_ABS_CKD failed for this wavelength: sos_proc's error for it
                ch.where = pl.index
                raise SosProcError(_abs.CKD_STATUS_MESSAGES.get(int(code), "COEFF_ABS_CKD failed"), ier=-1)


def _check_bins(ch, pl, fins, g):
    """The malformed-bin check of plan pl, segment g of the per-slot dictionaries fins (min_orders < 0: a bin failed)."""
    if any(f["min_orders"][g] < 0 for f in fins):
        ch.where = pl.index
        raise SosProcError("SOS_OS: wavelength %d (%r microns) holds a malformed bin (NT outside 1..CTE_OS_NT, "
                           "IBORM or an output level out of range)" % (pl.index, pl.p["wa_simu"]), ier=-1)


def _stage_irradiance_rows(ch, nz, blocks, status, alts, flux_rows, flux_row, ncol, absorb_rows):
    """irr: the rows of the chunk's calls from the downloaded blocks [K][calls][14] of sosgpu_level_irradiance -- the CKD status
    check and the malformed-bin check of _stage_todo, then per (call, altitude) the host statements of the levels pass:
    flux_row (_level_flux_row / _level_flux_split_row) on the pair (columns 4, 5) and on dist.finish_irradiance of the
    block's band scalars, _level_absorption_row on columns 0..3."""
    from . import dist as _dist
    _check_ckd_status(ch, status)
    for (gp, _, _, _), blk in zip(ch.solved, blocks):
        fins = [_dist.finish_irradiance(blk[k]) for k in range(nz)]
        for g, pl in enumerate(gp):
            _check_bins(ch, pl, fins, g)
            flux_rows[pl.index] = np.empty((nz, ncol))
            if absorb_rows is not None:
                absorb_rows[pl.index] = np.empty((nz, len(LEVEL_ABSORPTION_NAMES)))
            for k in range(nz):
                flux_rows[pl.index][k] = flux_row(pl, alts[k], fins[k], g, blk[k][g][4:6])
                if absorb_rows is not None:
                    absorb_rows[pl.index][k] = _level_absorption_row(alts[k], blk[k][g][0:4])


def _gather_rows(mine, world, *rows):
    """Every rank receives the rows of the calls the other ranks computed (all_gather_object, as _gather_results lets the flux
    rows travel): rows, the per-call lists of the pass, are filled in place."""
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, [(i, tuple(x[i] for x in rows)) for i in mine])
    for pr in parts:
        for i, vals in pr:
            for x, v in zip(rows, vals):
                if x[i] is None:
                    x[i] = v


def _stage_todo(ch, nz, blocks, albs, status, trans_out, salb):
    """The sections of the download read: the CKD status check first, the spherical albedos, then the jobs of the chunk's
    recompositions [(plan, slot, record, finish_scalars, segment)] with the malformed-bin check, and (trans_out not None) the
    trans_entry of every call."""
    from . import dist as _dist
    _check_ckd_status(ch, status)
    s_alb = {}
    for (gp, _), vals in zip(ch.salb_bands, albs):
        s_alb.update((pl.index, float(v)) for pl, v in zip(gp, vals))
    todo = []
    for (gp, rec, _, _), blk in zip(ch.solved, blocks):
        fins = [_dist.finish_scalars(blk[k]) for k in range(nz)]
        recs = [rec[k] for k in range(nz)]
        for g, pl in enumerate(gp):
            _check_bins(ch, pl, fins, g)
            todo += [(pl, k, recs[k][g], fins[k], g) for k in range(nz)]
            if trans_out is not None:               # (the same values in every slot: they ignore the altitude)
                trans_out[pl.index] = trans_entry(pl.p["tetas"], pl.mu, float(fins[0]["ttot_tronc"][g]),
                                                  float(fins[0]["ttot_vrai"][g]), float(fins[0]["tdifmus"][g]),
                                                  np.array(fins[0]["tdifmug"][g], dtype=np.float64))
                if salb:                            # (a call without bins took no part in the stage)
                    trans_out[pl.index]["s_alb"] = s_alb.get(pl.index, 0.0)
    return todo


def _stage_flux_rows(todo, flux_dev, flux_rows, flux_row, ncol, alts, absorb_rows=None):
    """fluxes: the flux rows [K][ncol] of the chunk's calls from the downloaded pairs of _stage_flux_launch; absorb_rows: the
    rows [K][5] of LEVEL_ABSORPTION_NAMES from the columns behind the pairs."""
    e = flux_dev.cpu().numpy()                      # (complete: queued ahead of the recompositions just downloaded)
    for j, (pl, k, r, f, g) in enumerate(todo):
        if flux_rows[pl.index] is None:
            flux_rows[pl.index] = np.empty((len(alts), ncol))
        flux_rows[pl.index][k] = flux_row(pl, alts[k], f, g, e[j])
        if absorb_rows is not None:
            if absorb_rows[pl.index] is None:
                absorb_rows[pl.index] = np.empty((len(alts), len(LEVEL_ABSORPTION_NAMES)))
            absorb_rows[pl.index][k] = _level_absorption_row(alts[k], e[j][2:6])


def _channel_terms(chan, nz, indices):
    """The arguments (ncalls, first, job, wgt) of solver.channel_accumulate for a chunk; indices: the call index of every
    entry of the todo list, the nz slots of a call side by side, so that call indices[j nz] is job j.  A channel names its
    calls of the chunk in ascending call index, whatever the job order is; first[c]:first[c + 1] are the terms of channel c."""
    job_of = {indices[j * nz]: j for j in range(len(indices) // nz)}
    calls = sorted(job_of)
    first, job, wgt = [0], [], []
    for c in range(chan.shape[0]):
        for i in calls:
            if chan[c, i] != 0.0:
                job.append(job_of[i])
                wgt.append(chan[c, i])
        first.append(len(job))
    return len(calls), first, job, wgt


def _stage_channels(fn, todo, flat, shapes, chan, nz, acc, ang_rows, call_scal, flux_rows, dev):
    """chan: the chunk's blocks stay on the device: one launch adds them onto the accumulator.  todo holds the K slots of a
    call side by side, in group order: block (j, k) of call todo[j K].  Returns (acc, ang_rows), made by the first chunk."""
    import torch
    from . import solver
    if len(set(shapes)) != 1:
        raise ValueError("%s: the calls do not share one block shape [nphi][7][W]: %s" % (fn, sorted(set(shapes))))
    nphi, _, w = shapes[0]
    if acc is None:
        acc = torch.zeros((chan.shape[0], nz, nphi, 3, w), dtype=torch.float64, device=dev)
        ang_rows = flat[:nphi * 7 * w].view(nphi, 7, w)[:, 3, :].clone()
    ncalls, first, job, wgt = _channel_terms(chan, nz, [t[0].index for t in todo])
    solver.channel_accumulate(flat, ncalls, nz, nphi, w, first, job, wgt, acc)
    for pl, k, r, f, g in todo:
        row = _finish_scalars(pl, f, g)
        if flux_rows is not None:
            row = row + tuple(flux_rows[pl.index][k])
        call_scal.setdefault(pl.index, [None] * nz)[k] = row
    return acc, ang_rows


def _stage_tuples(ch, todo, flat, shapes, results, nrows, nz):
    """The 23-tuples of the chunk's (wavelength, altitude) jobs from the downloaded recompositions, into results[index][k]."""
    from . import solver
    blocks = _zero_pages((len(todo), 2, 7, 361, 81))    # the result tables of the chunk's wavelengths (views of it)
    for j, ((pl, k, r, f, g), blk) in enumerate(zip(todo, solver._flat_blocks(flat, shapes))):
        ch.where = pl.index
        if results[pl.index] is None:
            results[pl.index] = [None] * nz
        results[pl.index][k] = _finish(pl, blk, r, f, g, blocks[j])
        nrows[pl.index] = len(pl.rows)


def _spectrum_pass(fn, kwargs_list, aer_phases, device, gather, chunk, timings, prep_streams, parts, alts=None, fluxes=False,
                   split=False, chan=None, trans=False, salb=False, absorption=False, irr=False):
    """The one pass behind sos_spectrum (alts None) and sos_spectrum_levels (alts: the K output altitudes), whose docstrings
    describe it.  After the solves both modes share one layout, rec[K][nw][S][3][W] / scal[K][nw][10+N] device tensors per
    launch with K = 1 for sos_spectrum (views of what its solves return); what differs is decided here, ahead of the loop.
    The phases of a chunk are the functions above, which hand the _Chunk to each other; the clock is read between them.
    split (with fluxes): the bins carry the untruncated depth rows, the levels `tauvrai`, and the flux rows two more columns.
    absorption (with fluxes): every solve is followed by one sosgpu_level_absorption launch; the blocks come down with the flux
    pairs and the pass also returns one array [K][5] of LEVEL_ABSORPTION_NAMES per call, behind the flux rows.
    chan (sos_spectrum_channels: the weights [C][calls] of the sensor channels, None: the pass as it was): the recomposition
    blocks of a chunk stay on the device and are added, weight by weight, onto one accumulator [C][K][nphi][3][W] that lives
    for the pass (solver.channel_accumulate, one call per chunk); no table is built and no 23-tuple formed per wavelength.
    Returns what _channel_results makes of the accumulator and of the per-call scalars.
    trans (transmissions=True of the two entry points): after a part's operators are queued, ONE
    solver.diffuse_transmissions_many call per group of equal direction count gives the diffuse transmissions of every bin of
    the part; they ride the groups' and the singles' aggregates, and the pass also returns one trans_entry per call.
    salb (spherical_albedo=True, only with trans): next to it ONE solver.spherical_albedo_many call per such group and one
    solver.albedo_band launch for the group's calls; the band values come down with the chunk's band scalars and become the
    key s_alb of the entries.
    irr (sos_spectrum_irradiances: alts and fluxes given, no chan, no trans): the irradiance rows alone.  The contexts and bins
    hold the Fourier order 0 alone (_prepare(order0=True)); a solved group is ONE sosgpu_os_solve_multi_levels launch and ONE
    sosgpu_level_irradiance launch behind it, whose block [K][calls][14] takes the place of the scalar blocks in the chunk's one
    download.  No aggregate, no flux launch, no recomposition, no table, no 23-tuple: the rows are formed from the block by
    _stage_irradiance_rows, and the pass returns the flux rows (with absorption: the pair of flux and absorption rows)."""
    import time
    import torch
    from . import capi, solver
    from . import dist as _dist
    from . import aerosols as _aer
    from . import absorption as _abs
    nwl = len(kwargs_list)
    if aer_phases is None:
        aer_phases = [None] * nwl
    if len(aer_phases) != nwl:
        raise ValueError("aer_phases must be parallel to kwargs_list")
    if nwl == 0:
        return tuple([] for _ in range(1 + bool(fluxes) + bool(absorption) + bool(trans))) if fluxes or trans else []
    capi.lib()
    dev = torch.device("cuda", device)
    # the per-bin diffuse transmissions of a plan: its own loop's (a -SOS.Trans call), or its rows of the part's
    # diffuse_transmissions_many (trans); the keyword is passed only with trans, so that the calls are as they were without it
    def single_trans(pl):
        return pl.tdifmug if pl.tdifmug is not None else pl.trans_rows

    def group_trans(gp):
        return dict(tdifmug=torch.cat([pl.trans_rows for pl in gp])) if trans else {}

    # solve_spectrum / solve_spectrum_levels are looked up when called: the tests count launches by replacing them
    if alts is None:
        nz, per_chunk = 1, max(1, int(chunk))

        def solve_group(table, gp, bins, cob, seg, aik):
            rec, scal = solver.solve_spectrum(table, bins, cob, seg, aik, order=None, **group_trans(gp))
            return rec[None], scal[None]

        def solve_single(pl):
            out = pl.ctx.solve(pl.bins, pl.ctx.alloc_outputs(pl.bins["nb"], zero=False))
            rec, scal = pl.ctx.aggregate(out, pl.aik, scal=pl.bins.get("scal"), tdifmug=single_trans(pl))
            return rec[None], scal[None]
    else:
        nz, per_chunk = len(alts), max(1, int(chunk) // len(alts))      # the record-memory rule of sos_spectrum_levels

        # absorption: the solves keep their per-bin records, and ONE sosgpu_level_absorption launch per solve, behind its
        # aggregates, adds the block [K][calls][4] to ch.absorb (parallel to ch.solved); without it the calls are as they were
        def solve_group(table, gp, bins, cob, seg, aik):
            levels = solver.concat_levels([pl.levels for pl in gp])
            if not absorption:
                return solver.solve_spectrum_levels(table, bins, cob, seg, aik, levels, order=None, **group_trans(gp))
            cx = table.ctxs[0]
            out = cx.alloc_outputs(bins["nb"], zero=False)
            out["rec"] = torch.empty((nz, bins["nb"], cx.smax + 1, 3, cx.w), dtype=torch.float64, device=dev)
            res = solver.solve_spectrum_levels(table, bins, cob, seg, aik, levels, out=out, order=None, **group_trans(gp))
            zbins = dict(bins, zprof=torch.cat([solver.level_altitudes(pl.bins, bins["lp"]) for pl in gp]))
            ch.absorb.append(solver.level_absorption_spectrum(table, zbins, cob, seg, aik, levels, out))
            return res

        def solve_single(pl):
            out = pl.ctx.solve_levels(pl.bins, pl.levels) if pl.bins["nb"] else None
            res = pl.ctx.aggregate_levels(out, pl.levels, pl.aik, scal=pl.bins.get("scal"), tdifmug=single_trans(pl))
            if absorption:
                ch.absorb.append(pl.ctx.level_absorption(pl.bins, pl.levels, out, pl.aik))
            return res

        if irr:
            # irradiances alone: the order-0 solve, then ONE sosgpu_level_irradiance launch; its block stands where the scalar
            # blocks stand in ch.solved, and there are no aggregated records
            def solve_group(table, gp, bins, cob, seg, aik):
                levels = solver.concat_levels([pl.levels for pl in gp])
                out = solver.solve_spectrum_order0(table, bins, cob, levels)
                zbins = dict(bins, zprof=torch.cat([solver.level_altitudes(pl.bins, bins["lp"]) for pl in gp]))
                return None, solver.level_irradiance_spectrum(table, zbins, cob, seg, aik, levels, out)

            def solve_single(pl):
                out = pl.ctx.solve_levels(pl.bins, pl.levels) if pl.bins["nb"] else None
                return None, pl.ctx.level_irradiance(pl.bins, pl.levels, out, pl.aik)
    true_kw = dict(true_depth=True) if split else {}    # (split=False: the calls as they were)
    prep_kw = dict(true_kw, order0=True) if irr else true_kw
    flux_row, flux_names = (_level_flux_split_row, LEVEL_FLUX_SPLIT_NAMES) if split else (_level_flux_row, LEVEL_FLUX_NAMES)
    level_keys = ("jout", "zz", "tauout") + (("tauvrai",) if split else ())
    rank, world = _dist_rank_world()
    if world > 1:
        shards = _dist.balanced_shards(spectrum_costs(kwargs_list), world)
        mine = [int(i) for i in shards[rank]]
    else:
        shards = [range(nwl)]
        mine = list(range(nwl))
    if chan is not None:
        mine = sorted(mine)                             # a rank adds its calls in ascending call index
        lead = rank == min(r for r in range(world) if len(shards[r]))    # the rank whose ANGDIFF rows the all-reduce carries
        acc = ang_rows = None                           # the accumulator and the ANGDIFF rows [nphi][W] of one block
        call_scal = {}                                  # call -> [K][5 (+ flux columns)]: elements 18..22 (and the flux row)
    results = [None] * nwl                              # K 23-tuples per wavelength
    flux_rows = [None] * nwl if fluxes else None        # fluxes: the [K][5] flux rows per wavelength
    absorb_rows = [None] * nwl if absorption else None  # absorption: the [K][5] actinic / absorbed-power rows per wavelength
    trans_out = [None] * nwl if trans else None         # trans: the trans_entry of every wavelength
    debug = bool(os.environ.get("SOS_SPECTRUM_DEBUG"))
    nrows = {}
    tm = dict(prepare=0.0, solve_launch=0.0, wait=0.0, trphi=0.0, finish=0.0, fluxes=0.0)
    if chan is not None:
        tm["channels"] = 0.0
    main_st = torch.cuda.current_stream(dev)
    side = [torch.cuda.Stream(device=dev) for _ in range(max(1, int(prep_streams)))]
    aer_st = torch.cuda.Stream(device=dev)
    if len(mine) >= 64 and "GPU_MAX_HW_QUEUES" not in os.environ and not getattr(_spectrum_pass, "_warned_queues", False):
        import warnings
        _spectrum_pass._warned_queues = True
        warnings.warn("GPU_MAX_HW_QUEUES is not set: the HIP runtime maps the %d preparation streams of %s onto 4 hardware "
                      "queues and the device side of the preparation becomes the limit (about 2/3 of the throughput); export "
                      "GPU_MAX_HW_QUEUES=16 before the first GPU call of the process (16 // processes when several processes share "
                      "the GPU)" % (len(side), fn), RuntimeWarning, stacklevel=3)
    # SOS_SPECTRUM_PROFILES_PER_CALL=1: every wavelength makes its own profile launches, as sos_proc does (A/B timing)
    batch_profiles = not os.environ.get("SOS_SPECTRUM_PROFILES_PER_CALL")
    # the layer tables of the deferred gas wavelengths (COEFF_ABS_CKD) are interpolated on the device, one launch per part on the
    # resident coefficient files; SOS_SPECTRUM_HOST_GAS_TABLES=1: on the host, uploaded with the requests (A/B timing).  A band
    # dealt over several ranks keeps the host tables: bin_costs needs them
    device_tables = batch_profiles and not os.environ.get("SOS_SPECTRUM_HOST_GAS_TABLES")
    # the operator tables of a part's contexts (surface packing + SOS_NOYAUX kernels) are filled by one call on the main stream,
    # at most five launches for the part; SOS_SPECTRUM_OPERATORS_PER_CALL=1: four or five launches per wavelength on its side
    # stream, as sos_proc makes them (A/B timing)
    batch_operators = not os.environ.get("SOS_SPECTRUM_OPERATORS_PER_CALL")
    # the sea and land surface matrices of a chunk's calls come from one asynchronous sosgpu_surface_batch per angle set, queued by
    # the prefetch; SOS_SPECTRUM_SURFACE_PER_CALL=1: every call that misses the cache makes its own synchronous call (A/B timing)
    batch_surfaces = not os.environ.get("SOS_SPECTRUM_SURFACE_PER_CALL")
    # the contexts of a part's calls that defer both profiles and operators are made by one asynchronous sosgpu_create_spectrum on
    # the main stream (_stage_contexts); SOS_SPECTRUM_CONTEXTS_PER_CALL=1: every call makes its own sosgpu_create, which waits for
    # its copy (A/B timing, and the checker of the batch)
    batch_contexts = batch_profiles and batch_operators and not os.environ.get("SOS_SPECTRUM_CONTEXTS_PER_CALL")
    ch, err = _Chunk(), None
    ch.where = -1                                       # the wavelength being worked on (named by a failure)
    # The cyclic garbage collector is paused for the pass: a spectrum allocates tens of container objects per wavelength next to
    # a growing list of result tuples, and the collections this triggers re-walk the results again and again (SOS_SPECTRUM_KEEP_GC=1
    # leaves the collector alone).  Nothing here relies on it: contexts are closed explicitly, tensors are freed by reference count.
    import gc
    pause_gc = gc.isenabled() and not os.environ.get("SOS_SPECTRUM_KEEP_GC")
    if pause_gc:
        gc.disable()
    try:
        for c0 in range(0, len(mine), per_chunk):
            idx = mine[c0:c0 + per_chunk]
            ch.plans, ch.solved, ch.salb_bands, ch.ckd_checks, ch.absorb = [], [], [], [], []
            try:
                t0 = time.perf_counter()
                ch.where = idx[0]
                # the preparation of wavelength k queues its device work (source operators, absorption and level profiles of its
                # bins: latency-bound kernels of 0.1-2 ms on a few wavefronts) on side stream k mod n: the wavelengths overlap on the
                # device, and the launches below wait for all of them
                for st in side + [aer_st]:
                    st.wait_stream(main_st)
                aer_wa = _spectrum_prefetch(kwargs_list, aer_phases, idx, device, aer_st, device_tables, batch_surfaces)
                # The chunk goes to the solver in a few parts: the solves of a part run on the device while the host prepares the
                # next one, so that only the last part's solve is waited for below.
                # (at least 32 wavelengths per part -- a launch per kernel variant each; SOS_SPECTRUM_MIN_PART: the tests' override)
                for s0, s1 in _part_bounds(len(idx), parts, int(os.environ.get("SOS_SPECTRUM_MIN_PART", "32"))):
                    part = _stage_prepare(fn, ch, kwargs_list, aer_phases, device, idx, s0, s1, side, aer_st, aer_wa, alts,
                                          prep_kw, batch_profiles, device_tables, batch_operators, debug, batch_contexts)
                    _stage_contexts(ch, part, fn, debug)
                    _stage_profiles(ch, part, alts, level_keys, true_kw, dev)
                    for st in side:
                        main_st.wait_stream(st)
                    _stage_operators(ch, part)
                    if trans:
                        _stage_transmissions(ch, part, salb, dev)
                    t1 = time.perf_counter()
                    tm["prepare"] += t1 - t0
                    groups, single = _part_groups(part)
                    _stage_solves(fn, ch, groups, single, solve_group, solve_single, alts, level_keys, dev, debug)
                    t0 = time.perf_counter()
                    tm["solve_launch"] += t0 - t1
                if irr:                             # the blocks come down once; the rows are host statements on them
                    t2 = time.perf_counter()
                    blocks, _, status = _download_scalars(ch, nz)
                    t3 = time.perf_counter()
                    tm["wait"] += t3 - t2
                    _stage_irradiance_rows(ch, nz, blocks, status, alts, flux_rows, flux_row, len(flux_names), absorb_rows)
                    tm["fluxes"] += time.perf_counter() - t3
                    continue
                flux_dev = None
                if fluxes:
                    tf = time.perf_counter()
                    flux_dev = _stage_flux_launch(ch, nz)
                    tm["fluxes"] += time.perf_counter() - tf
                t2 = time.perf_counter()
                blocks, albs, status = _download_scalars(ch, nz)
                t3 = time.perf_counter()
                tm["wait"] += t3 - t2
                todo = _stage_todo(ch, nz, blocks, albs, status, trans_out, salb)
                # then every azimuth recomposition back to back: one launch for every (wavelength, altitude) of the chunk, its
                # flat result downloaded as it is
                flat, shapes = _trphi_launch_many([(pl, r, int(f["n_orders"][g]), float(f["ttot_tronc"][g]), float(f["tauout"][g]))
                                                   for pl, _, r, f, g in todo])
                if chan is None:
                    flat = flat.cpu().numpy()
                t4 = time.perf_counter()
                tm["trphi"] += t4 - t3
                if fluxes:
                    _stage_flux_rows(todo, flux_dev, flux_rows, flux_row, len(flux_names), alts, absorb_rows)
                    t5 = time.perf_counter()
                    tm["fluxes"] += t5 - t4
                    t4 = t5
                if chan is not None:
                    ch.where = idx[0]
                    acc, ang_rows = _stage_channels(fn, todo, flat, shapes, chan, nz, acc, ang_rows, call_scal, flux_rows, dev)
                    tm["channels"] += time.perf_counter() - t4
                    continue
                _stage_tuples(ch, todo, flat, shapes, results, nrows, nz)
                tm["finish"] += time.perf_counter() - t4
            finally:
                _aer.drop_prefetched_size_integrals()
                _abs.drop_prefetched_gas_tables()
                for st in side + [aer_st]:
                    st.synchronize()
                main_st.synchronize()                             # the table launches read every context's operators
                _drop_prefetched_surfaces()
                for pl in ch.plans:
                    pl.ctx.close()
    except Exception as e:                         # noqa: BLE001 -- re-raised below, after the ranks have agreed
        err = e
    finally:
        if pause_gc:
            gc.enable()
    if world > 1:
        # a call failing on one rank must not leave the others waiting in the gather: the ranks agree first (one integer)
        bad = _first_failed_index(max(ch.where, 0) if err is not None else -1, device)
        if bad >= 0:
            if err is not None:
                raise SosProcError("%s: wavelength %d failed: %s" % (fn, ch.where, err), ier=getattr(err, "ier", 1)) from err
            raise SosProcError("%s: wavelength %d failed on another rank" % (fn, bad), ier=-1)
    if err is not None:
        raise err
    if timings is not None:
        timings.update(tm)
    if chan is not None:
        return _channel_results(kwargs_list[0], chan, mine, acc, ang_rows, call_scal, alts, len(flux_names) if fluxes else 0,
                                dev, world, lead)
    if irr:
        rows = (flux_rows,) + ((absorb_rows,) if absorption else ())
        if world > 1 and gather:
            _gather_rows(mine, world, *rows)
        return rows if absorption else flux_rows
    if alts is None:
        results = [None if r is None else r[0] for r in results]
    if world > 1 and gather:
        _gather_results(results, mine, nrows, world, None if alts is None else nz, flux_rows, trans_out, absorb_rows)
    ret = (results,) + ((flux_rows,) if fluxes else ()) + ((absorb_rows,) if absorption else ()) + ((trans_out,) if trans else ())
    return ret if len(ret) > 1 else results


def _channel_results(kw, chan, mine, acc, ang_rows, call_scal, alts, nflux, dev, world, lead):
    """The tail of a channel pass: the host sums of the per-call scalars (ascending call index, a = a + w * x), under
    torch.distributed ONE all-reduce (SUM) of the accumulator -- the ANGDIFF rows of the lead rank ride behind it, the other
    ranks add zeros there -- and one of the packed scalar sums, then one sosgpu_channel_finish launch, one download and the
    tables per (channel, altitude).  kw: any call of the list (the geometry is common).  Returns the tuples [C] (alts None)
    or [C][K], with nflux > 0 the pair (tuples, flux rows [C] of [K][nflux])."""
    import torch
    from . import solver
    p = dict(kw)
    validate_parameters(p)
    mu, _, _, ind_ang = angles(_angle_counts(p)[0], p["tetas"], p["ficangles_user_lum"])
    n = len(mu)
    w = 2 * n + 1
    _, rows, phi_fin = _trphi_azimuths(p["itrphi"], p["phios"], p["pas_phi"])
    nphi, nz, n_chan = len(rows), 1 if alts is None else len(alts), chan.shape[0]
    sums = np.zeros((n_chan, nz, 5 + nflux))
    vals = {i: np.array(call_scal[i], dtype=np.float64) for i in mine}
    own = np.array(mine, dtype=np.int64)                # (ascending)
    for c in range(n_chan):
        a = sums[c]
        for i in own[chan[c, own] != 0.0]:
            a = a + chan[c, i] * vals[int(i)]
        sums[c] = a
    if acc is None:                                     # a rank without a call
        acc = torch.zeros((n_chan, nz, nphi, 3, w), dtype=torch.float64, device=dev)
        ang_rows = torch.zeros((nphi, w), dtype=torch.float64, device=dev)
    if tuple(acc.shape) != (n_chan, nz, nphi, 3, w):
        raise ValueError("the blocks of the pass are %s, the common geometry says %s" % (tuple(acc.shape[2:]), (nphi, 3, w)))
    if world > 1:
        import torch.distributed as dist
        on_gpu = dist.get_backend() == "nccl"
        buf = torch.cat([acc.reshape(-1), ang_rows.reshape(-1) if lead else torch.zeros_like(ang_rows).reshape(-1)])
        st = torch.from_numpy(sums.reshape(-1).copy())
        if on_gpu:
            st = st.to(dev)
        else:
            buf = buf.cpu()
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        dist.all_reduce(st, op=dist.ReduceOp.SUM)
        buf = buf.to(dev)
        acc, ang_rows = buf[:acc.numel()].view(acc.shape), buf[acc.numel():].view(nphi, w)
        sums = st.cpu().numpy().reshape(sums.shape)
    block = torch.zeros((nphi, 7, w), dtype=torch.float64, device=dev)
    block[:, 3, :] = ang_rows
    out = solver.channel_finish(acc.contiguous(), block).cpu().numpy()
    ind_angout = np.zeros(81, dtype=np.int32)
    ind_angout[:n] = ind_ang
    tuples = []
    for c in range(n_chan):
        per = []
        for k in range(nz):
            ph, th, up, dn = _trphi_pack(n, mu, out[c, k], rows, phi_fin.copy())
            per.append((n, ind_angout.copy(), ph, th,
                        up["sca"], up["i"], up["q"], up["u"], up["ang"], up["rate"], up["lpol"],
                        dn["sca"], dn["i"], dn["q"], dn["u"], dn["ang"], dn["rate"], dn["lpol"]) +
                       tuple(float(x) for x in sums[c, k, :5]))
        tuples.append(per[0] if alts is None else per)
    if not nflux:
        return tuples
    return tuples, [sums[c, :, 5:].copy() for c in range(n_chan)]


_CHANNEL_SHARED = ("nbmu_gauss_lum", "tetas", "ficangles_user_lum", "itrphi", "phios", "pas_phi", "ipolar")


def _channel_arguments(fn, kwargs_list, weights, normalize, altitudes, fluxes, split, absorption=False):
    """The argument rules of sos_spectrum_channels, checked before any device work (ValueError naming the first offending
    channel or call).  Returns (the weights [C][calls] as they are applied, the altitudes as floats or None)."""
    nwl = len(kwargs_list)
    try:
        wts = np.array(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: weights must be a [C][%d] array of numbers" % (fn, nwl))
    if wts.ndim != 2 or wts.shape[0] < 1 or wts.shape[1] != nwl:
        raise ValueError("%s: weights must be [C][%d] (one row per channel, one column per call), got %s"
                         % (fn, nwl, tuple(wts.shape)))
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError("%s: normalize must be True or False, got %r" % (fn, normalize))
    bad = np.argwhere(~np.isfinite(wts))
    if len(bad):
        raise ValueError("%s: the weight of channel %d for call %d is not finite" % (fn, bad[0][0], bad[0][1]))
    for c in range(wts.shape[0]):
        if not np.any(wts[c] != 0.0):
            raise ValueError("%s: channel %d has no non-zero weight" % (fn, c))
    if normalize:
        for c in range(wts.shape[0]):
            total = np.cumsum(wts[c])[-1]               # the left-to-right sum
            if total == 0.0 or not np.isfinite(total):
                raise ValueError("%s: the weights of channel %d sum to %r: they cannot be normalised" % (fn, c, float(total)))
            wts[c] = wts[c] / total
    defaults = {k: v for _, k, v in PARAMS}
    shared = _CHANNEL_SHARED + (("zout",) if altitudes is None else ())
    names = {k: d for d, k, _ in PARAMS}
    for i, kw in enumerate(kwargs_list):
        for k in shared:
            if kw.get(k, defaults[k]) != kwargs_list[0].get(k, defaults[k]):
                raise ValueError("%s: call %d differs from call 0 in %s (%r against %r): the calls of a channel share their "
                                 "directions, azimuths and output altitude" % (fn, i, names[k], kw.get(k, defaults[k]),
                                                                               kwargs_list[0].get(k, defaults[k])))
    for i, kw in enumerate(kwargs_list):
        if str(kw.get("resroot", "")).strip():
            raise ValueError("%s writes no result files: -SOS_Main.ResRoot of call %d must be empty (use sos_spectrum)" % (fn, i))
    if altitudes is None:
        if fluxes or split:
            raise ValueError("%s: fluxes and split belong to the altitudes of a levels call: give `altitudes`" % fn)
        if absorption is not False:
            raise ValueError("%s: absorption=True is not available for sensor channels (and belongs to a levels call), got %r"
                             % (fn, absorption))
        return wts, None
    return wts, _levels_arguments(fn, altitudes, kwargs_list, fluxes, split, absorption)


def sos_spectrum_channels(kwargs_list, weights, normalize=True, altitudes=None, fluxes=False, split=False, aer_phases=None,
                          device=0, chunk=256, timings=None, prep_streams=16, parts=4, absorption=False):
    """The radiances of C sensor channels from a spectrum of sos_proc calls: the spectrum of sos_spectrum (or, with
    `altitudes`, of sos_spectrum_levels) weighted by each channel's spectral response and summed over the calls ON THE DEVICE,
    so that no per-wavelength block is downloaded, no per-wavelength table built and no per-wavelength 23-tuple formed.

      chan = sos_spectrum_channels(kwargs_list, weights)                         # C 23-tuples in the OUTPUT_NAMES layout
      chan = sos_spectrum_channels(kwargs_list, weights, altitudes=[-1, 0., 3.]) # chan[c][k]: channel c at altitude k
      chan, flux = sos_spectrum_channels(kwargs_list, weights, altitudes=[...], fluxes=True)   # flux[c]: [K][5] ([K][7]: split)

    weights: [C][len(kwargs_list)] numbers; weights[c][i] multiplies call i in channel c (the response times the solar
    irradiance, say).  A zero entry means the call is not in the channel: it becomes no term.  normalize=True divides each row
    by its left-to-right sum (np.cumsum(row)[-1]) first; normalize=False applies the weights as given.

    The pass is that of sos_spectrum / sos_spectrum_levels up to the azimuth recompositions of a chunk (one
    sosgpu_trphi_spectrum launch).  Behind it ONE sosgpu_channel_accumulate launch per chunk adds the chunk's blocks onto an
    accumulator [C][K][nphi][3][W] that lives for the pass: acc = acc + w * x for the I, Q, U rows, one multiply and one add
    per term, a channel's calls in ASCENDING CALL INDEX whatever `chunk` and `parts` are -- the sums equal, bit for bit, a host
    loop of that form over the tuples of sos_spectrum.  After the last chunk one sosgpu_channel_finish launch applies the
    reference's output thresholds (SOS_TRPHI.F:1212-1218) and SOS_POLAR to the sums, one download brings
    [C][K][nphi][7][W] to the host and the tables are packed per (channel, altitude).

    Returned tuples: elements 0..3 (directions, azimuths) are the calls' common geometry; the tables i, q, u (up and down) are
    the thresholded sums; sca_ang is any call's; pol_ang, pol_rate and l_pol are SOS_POLAR OF THE SUMS (not sums of the calls'
    values); elements 18..21 (flux_dir_down, flux_diff_down, flux_tot_down, flux_diff_up) and 22 (coef_tronca) are the weighted
    sums of the per-call values, formed on the host in ascending call index with the same a = a + w * x.  With fluxes=True the
    per-call flux rows of sos_spectrum_levels are summed in the same way.

    Checked before any device work, ValueError naming the first offending channel or call: the shape of `weights`, non-finite
    entries, a row without a non-zero entry, a row that sums to 0 under normalize=True, calls that differ in what shapes a
    block (-ANG.Rad.NbGauss, -ANG.Thetas, -ANG.Rad.UserAngFile, -SOS.View, -SOS.View.Phi, -SOS.View.Dphi, -SOS.Ipolar, and
    -SOS.OutputAlt when `altitudes` is None), a non-empty -SOS_Main.ResRoot (no per-wavelength files are written), and the
    rules of sos_spectrum_levels for altitudes, fluxes and split (fluxes and split need `altitudes`).  A call that fails raises
    what sos_spectrum raises for it.  absorption=True (the keyword of sos_spectrum_levels) is refused with a ValueError: the
    absorbed power is formed per CKD bin and returned per call, not per channel.
    aer_phases, device, chunk, timings, prep_streams, parts: as sos_spectrum; `timings` gains the host phase "channels" (the
    accumulate call and the per-call scalars) and its "finish" stays 0.

    With torch.distributed initialised the wavelengths are dealt to the ranks as in sos_spectrum; every rank accumulates its
    own calls; after the pass's failure agreement ONE all-reduce (SUM) of the accumulator and one of the packed scalar sums
    follow, then every rank finishes and returns the same objects.  The order of the sum across ranks differs from one
    process's, so the result equals a single process's to rounding, not to the bit."""
    wts, alts = _channel_arguments("sos_spectrum_channels", kwargs_list, weights, normalize, altitudes, fluxes, split, absorption)
    return _spectrum_pass("sos_spectrum_channels", kwargs_list, aer_phases, device, True, chunk, timings, prep_streams, parts,
                          alts, bool(fluxes), bool(split), chan=wts)


def _transmissions_argument(fn, kwargs_list, transmissions):
    """The rule of transmissions=True, checked before any library call: a bool, and no call may ask for the -SOS.Trans file
    (that option keeps its own path: one order-0 context per direction)."""
    if not isinstance(transmissions, (bool, np.bool_)):
        raise ValueError("%s: transmissions must be True or False, got %r" % (fn, transmissions))
    if transmissions:
        for i, kw in enumerate(kwargs_list):
            if str(kw.get("fictrans", "NO_OUTPUT")).strip() != "NO_OUTPUT":
                raise ValueError("%s: transmissions=True returns the diffuse transmissions as arrays; call %d asks for the "
                                 "-SOS.Trans file %r (leave it at NO_OUTPUT, or drop the keyword)" % (fn, i, kw["fictrans"]))
    return bool(transmissions)


def _spherical_albedo_argument(fn, spherical_albedo, trans):
    """The rule of spherical_albedo=True, checked before any library call: a bool, and only next to transmissions=True (the
    value is a key of the entries that keyword returns)."""
    if not isinstance(spherical_albedo, (bool, np.bool_)):
        raise ValueError("%s: spherical_albedo must be True or False, got %r" % (fn, spherical_albedo))
    if spherical_albedo and not trans:
        raise ValueError("%s: spherical_albedo=True requires transmissions=True (s_alb is a key of the trans entries)" % fn)
    return bool(spherical_albedo)


def sos_spectrum(kwargs_list, aer_phases=None, device=0, gather=True, chunk=256, timings=None, prep_streams=16, parts=4,
                 transmissions=False, spherical_albedo=False):
    """A spectrum of sos_proc calls -- one per wavelength, as the reference issues them one after the other
    (binding/run_sos.py:640-695; the bin loop of each is SOS_PROC.F:3459-3594) -- as ONE pass over the GPU:

      1. the host preparation of every wavelength (parameter checks, angles, aerosol model, gas tables, surface, context), then
         the profiles of ALL CKD bins of a part of the chunk in three launches (sosgpu_profile_spectrum through
         solver.make_profiles_spectrum: no-gas profiles, SOS_ABSPROFILE, SOS_PROFILE, every wavefront taking its wavelength's
         parameters from a device table), nothing waited for.  The gas coefficients of these wavelengths (COEFF_ABS_CKD for
         every gas, term and layer) are interpolated in one more launch ahead of them, on device-resident copies of the parsed
         CKD files (sosgpu_ckd_layer_tables); its per-wavelength status comes back with the band scalars of step 3, and a
         wavelength it flags raises the SosProcError sos_proc raises for that call (SOS_SPECTRUM_HOST_GAS_TABLES=1 in the
         environment: the tables are interpolated on the host and uploaded, for A/B timing).
         The sea and land surface matrices (-SURF.Type 1, 3, 4, 5, 7 without -SURF.File) of the chunk's calls that the surface
         cache does not hold are queued ahead of all this, one sosgpu_surface_batch per angle set
         (surface.surface_matrices_many), with one host wait per chunk for their status words; a call whose Roujean function
         goes negative raises sos_proc's error for it (SOS_SPECTRUM_SURFACE_PER_CALL=1 in the environment: one synchronous
         sosgpu_glitter / sosgpu_land_surface call per wavelength that misses the cache, for A/B timing).
         Calls with -SOS.Trans, -SOS.AbsModeCKD 2 or an aerosol layer
         (-AP.AerProfile.Type 2), and a call whose profile the library refuses (its error is then sos_proc's), make their own
         profile launches (sosgpu_absprofile + sosgpu_profile) as sos_proc does;
      2. ALL bins of ALL wavelengths in one launch of the fused solver per group of wavelengths sharing a kernel variant
         (direction count, highest Fourier order, surface-matrix flag, level capacity, output level): a device table of the
         wavelength contexts, every bin carrying the index of its own (sosgpu_ctx_table + sosgpu_os_solve_multi), and one
         segmented SOS_AGGREGATE;
      3. one device-to-host copy of the band scalars, the azimuth recompositions of every wavelength of the chunk in ONE launch
         (sosgpu_trphi_spectrum through solver.trphi_many; SOS_SPECTRUM_TRPHI_PER_CALL=1 in the environment: one sosgpu_trphi
         launch per wavelength, for A/B timing), one copy of their results, and the 23-tuples on the host.

    Outputs are those of `[sos_proc(**kw) for kw in kwargs_list]`, bit for bit (the table form of the kernels computes the same
    instruction sequence per bin; bands up to 128 bins are aggregated in the reference's serial bin order in both).
    Wavelengths are processed `chunk` at a time (their source operators are resident together: 32 MB each at N = 41).
    Calls that need the diffuse transmissions of -SOS.Trans run through the per-wavelength path.

    With torch.distributed initialised (one process per GPU) the WAVELENGTHS are dealt to the ranks by cost
    (spectrum_costs, dist.balanced_shards) -- no bin of a band leaves its rank, so there is no all-reduce, only the gather of
    the results ("partition by wavelength first"): gather=True returns the full list on every rank
    (all_gather_object of the compacted tuples), gather=False returns None in the slots of other ranks.  Result files of a
    call (-SOS_Main.ResRoot) are written by the rank that owns it.  Before the gather the ranks agree on failures (one integer
    all-reduce): a call failing on one rank makes EVERY rank raise SosProcError naming that wavelength; on one rank the call's
    own exception is raised.
    aer_phases: optional list parallel to kwargs_list of `aer_phase` dictionaries (see sos_proc) or None.
    timings: optional dict, filled with host-side phase times in seconds (prepare, solve_launch, wait, trphi, finish).
    parts: a chunk is handed to the solver in this many parts (the solves of one part overlap the host preparation of the next).
    prep_streams: HIP streams the per-wavelength preparation kernels are spread over (export GPU_MAX_HW_QUEUES=16 to give them
    hardware queues of their own, solver.solve_many): source operators, surface and aerosol steps of the wavelengths overlap
    there.  The profile kernels (level placement of the no-gas profile and of every bin: bisections, a serial chain of about
    3 ms on one wavefront per bin) are not among them any more: they run once per part for all its bins, on the stream of the
    solves.  SOS_SPECTRUM_PROFILES_PER_CALL=1 (environment, for A/B timing) sends every call through the per-wavelength
    profile launches on its side stream again.  The source operators are not among them either: the contexts are created unbuilt
    and solver.build_operators fills the operator tables of a part in at most five launches on the stream of the solves
    (sosgpu_noyaux_spectrum), after the side streams -- which produce the surface matrices -- have been waited for; a -SOS.Trans
    call builds its own, and SOS_SPECTRUM_OPERATORS_PER_CALL=1 gives every call its four or five launches on its side stream.
    The contexts of the calls that defer both their profiles and their operators are created for a whole part by one
    asynchronous call on the stream of the solves (solver.create_contexts, sosgpu_create_spectrum: one staged copy, one launch,
    no host wait); every other call makes its own sosgpu_create, and SOS_SPECTRUM_CONTEXTS_PER_CALL=1 makes all of them do.

    transmissions=True (a bool; every call with -SOS.Trans at NO_OUTPUT: ValueError naming the call otherwise, before any
    library call): returns (tuples, trans) with trans[i] the trans_entry of call i -- the diffuse transmittances TOA -> surface
    and surface -> TOA for every direction that the -SOS.Trans file prints, as arrays in full precision.  The transmissions of
    ALL bins of a part come from ONE order-0 solve per direction count (solver.diffuse_transmissions_many,
    sosgpu_trans_spectrum: no context per direction), whatever mix of grouped, single, no-gas, -SOS.AbsModeCKD 2 and aerosol-layer
    calls the part holds, and ride the aggregates that run anyway; the 23-tuples keep their bits.  With gather=True the
    entries travel with the compacted tuples.  With the default the return value, the launches and the bits are unchanged.

    spherical_albedo=True (a bool, and only with transmissions=True: ValueError otherwise, before any library call): every
    trans[i] has one more key, s_alb, the spherical albedo S of the atmosphere seen from the ground -- the third quantity of
        rho_toa = rho_path + T_down * T_up * rho_s / (1 - S * rho_s).
    Per CKD bin S = 2 sum_j ga_j mu_j A_j, A_j being the up-going flux of an order-0 solve over a black ground with the
    vertically MIRRORED profile and incidence mu_j (solver.spherical_albedo_many, sosgpu_albedo_spectrum): one more solve of
    the transmission stage's shape per part and direction count, minus the weight-0 directions, whatever path a call takes
    otherwise; one sosgpu_albedo_band launch per such group forms the band value sum aik * S_b, which comes down with the band
    scalars (no host wait is added).  S belongs to the truncated, equivalent atmosphere the solver sees, as tdifmug does; for
    a band of several CKD bins s_alb is the aik-weighted mean, and the coupling formula is exact per bin only.  With S the
    ground flux over a Lambert ground of albedo a obeys E_down(a) (1 - a S) = E_down(0); a Lambert coupling of the RADIANCE
    through t_dif_up is not claimed.  Not covered: the -SOS.Trans file path of sos_proc, and bands sharded over ranks.  Every
    other key, every tuple and, without the keyword, the keys themselves keep their bits."""
    trans = _transmissions_argument("sos_spectrum", kwargs_list, transmissions)
    salb = _spherical_albedo_argument("sos_spectrum", spherical_albedo, trans)
    return _spectrum_pass("sos_spectrum", kwargs_list, aer_phases, device, gather, chunk, timings, prep_streams, parts,
                          trans=trans, salb=salb)


def sos_spectrum_levels(altitudes, kwargs_list, aer_phases=None, device=0, gather=True, chunk=256, timings=None, prep_streams=16,
                        parts=4, fluxes=False, split=False, transmissions=False, spherical_albedo=False, absorption=False):
    """sos_spectrum for several output altitudes (-SOS.OutputAlt, km; -1 = the standard TOA / ground output): every wavelength is
    prepared once, ALL bins of a group of wavelengths go through ONE launch of the fused solver per kernel variant with K output
    slots each (sosgpu_os_solve_multi_levels), then K segmented aggregates (each altitude with its own TAUOUT) and K azimuth
    recompositions per wavelength.  Returns one list of K 23-tuples per call: result[i][k] equals
    sos_proc(**{**kwargs_list[i], "zout": altitudes[k]}) bit for bit, hence also sos_proc_levels(altitudes, **kwargs_list[i])[k].

    Argument rules of sos_proc_levels, checked for the whole list before any device work: 1 <= K <= 16 altitudes, duplicates
    allowed, each passing the -SOS.OutputAlt rule (SosProcError 2611); every call with zout = -1 and an empty -SOS_Main.ResRoot
    (ValueError otherwise).  An empty list returns [].
    Calls with -SOS.Trans (diffuse transmissions) and groups of one wavelength run through the per-wavelength path
    (SosContext.solve_levels + aggregate_levels; their scalars join the launches' one copy).
    Record memory: the records of a launch grow K-fold (at N = 41, 6 400 bins hold about 1 GB per altitude), so a chunk holds
    max(1, chunk // K) wavelengths -- a part's records then stay near what sos_spectrum holds with the same `chunk`.
    aer_phases, device, gather, timings, prep_streams, parts: as sos_spectrum.  With torch.distributed the wavelengths are dealt
    to the ranks by cost (spectrum_costs), without an all-reduce; the ranks then agree on failures (one integer all-reduce),
    so that a call failing on one rank makes EVERY rank raise SosProcError naming that wavelength instead of leaving the
    others waiting in the gather (all_gather_object of the compacted tuples, K per wavelength).  gather=False leaves None in
    the slots of other ranks.

    fluxes=True (a bool, ValueError otherwise, before any device work): returns (spec, flux) with spec the list above and
    flux[i] the numpy array [K][5] of call i, the irradiances at each altitude as sos_proc_levels(..., fluxes=True) describes
    them (columns LEVEL_FLUX_NAMES).  The flux pairs
    of ALL (wavelength, altitude) jobs of a chunk are computed by one launch (sosgpu_level_flux_spectrum through
    solver.level_flux_many) queued behind the chunk's aggregates, and come down after the recompositions without a wait of
    their own; `timings` gains the host phase "fluxes".  With gather=True the rows travel with the compacted tuples, so
    every rank returns the same arrays; gather=False leaves None in the slots of other ranks.  With the default the return
    value, the launches and the bits are unchanged.

    split=True (a bool, and only with fluxes=True: ValueError otherwise, before any device work): flux[i] is [K][7], columns
    LEVEL_FLUX_SPLIT_NAMES, the true direct / diffuse split of the down-going flux at each altitude as
    sos_proc_levels(..., fluxes=True, split=True) describes it, with its convention (the reference's linear interpolation of
    the untruncated depth between the two levels that bracket z); the rows equal that call's bit for bit.  The profile
    launches of a part export the untruncated depth rows (sosgpu_profile_spectrum_true), one sosgpu_output_depths launch per
    part or wavelength gives the depths at the altitudes, and ONE sosgpu_level_transmission launch per solved group (or single
    wavelength) -- not one per altitude -- puts their band transmissions into the scalar blocks that are downloaded anyway.

    absorption=True (a bool, and only with fluxes=True: ValueError otherwise, before any device work): returns (spec, flux,
    absorb) with absorb[i] the numpy array [K][5] of call i, columns LEVEL_ABSORPTION_NAMES: the actinic flux (direct, diffuse
    down, diffuse up, total) and the radiative power absorbed per kilometre at each altitude, as
    sos_proc_levels(..., fluxes=True, absorption=True) describes them, with its conventions; absorb[i][k] equals that call's
    row k bit for bit, whatever `chunk` is.  ONE sosgpu_level_absorption launch per solved group (or single wavelength) -- not
    one per altitude -- queued behind its aggregates forms the per-bin products and their aik-weighted sums; the blocks come
    down with the flux pairs.  With gather=True the rows travel with the compacted tuples.  Under torch.distributed the
    wavelengths are dealt whole, so the keyword is available there.  With the default the return value, the launches and the
    bits are unchanged.

    transmissions=True: as sos_spectrum describes it; trans (one trans_entry per call: the values do not depend on the output
    altitude) is appended behind spec, behind flux with fluxes=True and behind absorb with absorption=True.
    spherical_albedo=True (only with transmissions=True): the key s_alb of every entry, as sos_spectrum describes it; it does
    not depend on the output altitudes either."""
    trans = _transmissions_argument("sos_spectrum_levels", kwargs_list, transmissions)
    salb = _spherical_albedo_argument("sos_spectrum_levels", spherical_albedo, trans)
    alts = _levels_arguments("sos_spectrum_levels", altitudes, kwargs_list, fluxes, split, absorption)
    return _spectrum_pass("sos_spectrum_levels", kwargs_list, aer_phases, device, gather, chunk, timings, prep_streams, parts,
                          alts, bool(fluxes), bool(split), trans=trans, salb=salb, absorption=bool(absorption))


def _altitude_groups(k, size):
    """The (k0, k1) bounds of the groups K altitudes go to the solver in: `size` output slots per solve, the last group the
    remainder."""
    return [(k0, min(k0 + size, k)) for k0 in range(0, k, size)]


def _irradiance_weights(fn, weights, normalize, nwl, k):
    """The rule of `weights` of sos_spectrum_irradiances, checked before any device work: None, or finite numbers [R][nwl]
    (one weight per sum and call, the same at every altitude) or [R][K][nwl]; normalize (a bool) divides every weight row --
    the nwl weights of a sum, or of a sum at one altitude -- by its left-to-right sum, as sos_spectrum_channels does.  Returns
    the weights [R][K][nwl] as they are applied, or None."""
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError("%s: normalize must be True or False, got %r" % (fn, normalize))
    if weights is None:
        return None
    shapes = "[R][%d] or [R][%d][%d] (sums, altitudes, calls)" % (nwl, k, nwl)
    try:
        wts = np.array(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: weights must be an array of numbers %s" % (fn, shapes))
    if wts.ndim == 2 and wts.shape[0] >= 1 and wts.shape[1] == nwl:
        wts = np.repeat(wts[:, None, :], k, axis=1)
    elif not (wts.ndim == 3 and wts.shape[0] >= 1 and wts.shape[1:] == (k, nwl)):
        raise ValueError("%s: weights must be %s, got %s" % (fn, shapes, tuple(wts.shape)))
    bad = np.argwhere(~np.isfinite(wts))
    if len(bad):
        raise ValueError("%s: the weight of sum %d at altitude %d for call %d is not finite" % ((fn,) + tuple(bad[0])))
    if normalize:
        for r in range(wts.shape[0]):
            for j in range(k):
                total = np.cumsum(wts[r, j])[-1] if nwl else 0.0      # the left-to-right sum
                if total == 0.0 or not np.isfinite(total):
                    raise ValueError("%s: the weights of sum %d at altitude %d sum to %r: they cannot be normalised"
                                     % (fn, r, j, float(total)))
                wts[r, j] = wts[r, j] / total
    return wts


def _weighted_rows(wts, rows):
    """The weighted sums [R][K][ncol] of the per-call rows (a list of arrays [K][ncol]) with the weights [R][K][nwl] of
    _irradiance_weights: per sum and altitude a = a + w * x over the calls in ascending call index, one multiply and one add
    per column; a call of weight 0 is skipped (it adds nothing, not even a NaN row); a NaN row of non-zero weight stays NaN."""
    nr, k, nwl = wts.shape
    ncol = rows[0].shape[1] if nwl else 0
    out = np.zeros((nr, k, ncol))
    for r in range(nr):
        a = out[r]
        for i in range(nwl):
            w = wts[r, :, i]
            on = w != 0.0
            if on.any():
                a[on] = a[on] + w[on, None] * np.asarray(rows[i], dtype=np.float64)[on]
    return out


def sos_spectrum_irradiances(altitudes, kwargs_list, aer_phases=None, device=0, gather=True, chunk=256, timings=None,
                             prep_streams=16, parts=4, split=False, absorption=False, weights=None, normalize=False):
    """The irradiances of a spectrum at any number of altitudes, WITHOUT the radiances: the flux rows -- and with split=True /
    absorption=True the split and the actinic-flux / absorbed-power rows -- of
    sos_spectrum_levels(altitudes, kwargs_list, fluxes=True, ...), from Fourier order-0 solves alone.  Every column of these rows
    is an angular moment of the order-0 field at the altitude or a band scalar, and the Fourier orders do not couple in the
    solver; so the contexts are created with iborm_max = 0 (order-0 source operators, record 0 of the surface matrices), every
    bin gets iborm = 0, and a solved group is ONE sosgpu_os_solve_multi_levels launch followed by ONE sosgpu_level_irradiance
    launch that forms every moment per bin and sums it with aik next to the band scalars: no aggregate, no flux launch, no
    azimuth recomposition, no table and no 23-tuple.  The blocks [K][calls][14] come down once per chunk and the rows are the
    host statements of the levels pass on them.

      flux = sos_spectrum_irradiances(altitudes, kwargs_list)                 flux[i]: numpy [K][5], LEVEL_FLUX_NAMES
      flux, absorb = sos_spectrum_irradiances(..., split=True, absorption=True)   [K][7] LEVEL_FLUX_SPLIT_NAMES, [K][5]
                                                                              LEVEL_ABSORPTION_NAMES
    Against sos_spectrum_levels: a call of one bin (no gas, -SOS.AbsModeCKD 2) gives the same bits in every column; in a CKD
    band the two diffuse-flux columns are the aik-weighted sum of the bins' moments where the levels pass takes the moment of
    the summed record -- at most (bins + 2 N) roundings of non-negative terms apart, 1e-12 relative -- and the columns formed
    from them follow; every other column keeps its bits.

    altitudes: any number >= 1 (-1 = the standard output, whose absorption row is NaN), each passing the -SOS.OutputAlt rule.
    More than 16 go to the solver in groups of 16 output slots: one more pass over the same call list per group (every call is
    prepared again; an order-0 solve is cheap next to it), the rows concatenated in the order of `altitudes`.
    kwargs_list: the rules of sos_spectrum_levels -- no result files, zout = -1 -- and -SOS.Trans at NO_OUTPUT (ValueError
    otherwise).  Calls that keep their per-wavelength preparation there (-SOS.AbsModeCKD 2, an aerosol layer) keep it here.
    A failing call raises SosProcError naming its index.  aer_phases, device, gather, chunk, timings, prep_streams, parts: as
    sos_spectrum_levels (timings: the phases of the last altitude group).

    weights (None, or finite numbers [R][calls] or [R][K][calls]): returns the R weighted sums over the calls instead of the
    rows -- a numpy array [R][K][5 | 7], with absorption=True the pair of it and [R][K][5] -- formed on the host as
    a = a + w * x over the rows in ascending call index, a call of weight 0 skipped; actinic_tot and the NaN row of altitude -1
    are summed like any other.  With w = cross section x quantum yield x solar irradiance x band width the actinic_tot column
    is a photolysis frequency J(z), with w = solar irradiance x band width the absorbed_per_km column a broadband heating rate.
    normalize=True divides each weight row by its sum first, as sos_spectrum_channels does.  Under torch.distributed the
    wavelengths are dealt as in sos_spectrum_levels, the rows gathered on every rank (with weights whatever `gather` says),
    and every rank forms the sums in ascending call index: the bits of one process.

    ValueError, before any device work: split, absorption or normalize not a bool, weights of another shape or not finite, an
    empty altitude list."""
    from . import capi
    fn = "sos_spectrum_irradiances"
    try:
        alts_all = [float(z) for z in altitudes]
    except (TypeError, ValueError):
        raise ValueError("%s: altitudes must be a list of numbers" % fn)
    if not alts_all:
        raise ValueError("%s: at least one altitude" % fn)
    groups = _altitude_groups(len(alts_all), capi.MAX_OUTPUT_LEVELS)
    for k0, k1 in groups:                           # (the flag rules, the call rules and the -SOS.OutputAlt rule, per group)
        _levels_arguments(fn, alts_all[k0:k1], kwargs_list, True, split, absorption)
    for i, kw in enumerate(kwargs_list):
        if str(kw.get("fictrans", "NO_OUTPUT")).strip() != "NO_OUTPUT":
            raise ValueError("%s: call %d asks for the -SOS.Trans file %r: the pass solves the Fourier order 0 of the call's own "
                             "incidence alone (leave it at NO_OUTPUT)" % (fn, i, kw["fictrans"]))
    wts = _irradiance_weights(fn, weights, normalize, len(kwargs_list), len(alts_all))
    split, absorption = bool(split), bool(absorption)
    nwl = len(kwargs_list)
    flux, absorb = [[] for _ in range(nwl)], [[] for _ in range(nwl)]
    for k0, k1 in groups if nwl else []:
        res = _spectrum_pass(fn, kwargs_list, aer_phases, device, gather or wts is not None, chunk, timings, prep_streams, parts,
                             alts_all[k0:k1], True, split, absorption=absorption, irr=True)
        for rows, got in zip((flux, absorb), res if absorption else (res,)):
            for i in range(nwl):
                rows[i].append(got[i])
    join = lambda rows: [None if any(x is None for x in r) else np.concatenate(r) for r in rows]
    flux, absorb = join(flux), join(absorb) if absorption else None
    if wts is not None:
        flux = _weighted_rows(wts, flux)
        absorb = _weighted_rows(wts, absorb) if absorption else None
    return (flux, absorb) if absorption else flux


def trans_quantities(tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug):
    """The three quantities of the -SOS.Trans file (SOS_PROC.F:3785-3822) from the aggregated values: the direct transmission
    for the true optical depth, and the diffuse transmissions TOA -> surface and surface -> TOA (one per direction) brought
    back to the true atmosphere by + exp(-tau_tr/mu) - exp(-tau/mu).  Returns (t_dir_down, t_dif_down, t_dif_up[N])."""
    cs = math.cos(math.pi * tetas / 180.0)
    t_dir_down = math.exp(-ttot_vrai / cs)
    t_dif_down = tdifmus + math.exp(-ttot_tronc / cs) - math.exp(-ttot_vrai / cs)
    t_dif_up = np.empty(len(mu))
    for j in range(len(mu)):
        t_dif_up[j] = tdifmug[j] + math.exp(-ttot_tronc / mu[j]) - math.exp(-ttot_vrai / mu[j])
    return t_dir_down, t_dif_down, t_dif_up


def trans_entry(tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug):
    """trans[i] of sos_spectrum(..., transmissions=True): the angles, the aggregated values write_trans_file receives and the
    three quantities it prints (trans_quantities), in full precision."""
    t_dir_down, t_dif_down, t_dif_up = trans_quantities(tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug)
    return dict(thetas=float(tetas), thetav=np.array([math.degrees(math.acos(m)) for m in mu]),
                ttot_tronc=ttot_tronc, ttot_vrai=ttot_vrai, tdifmus=tdifmus, tdifmug=tdifmug,
                t_dir_down=t_dir_down, t_dif_down=t_dif_down, t_dif_up=t_dif_up)


def write_trans_file(path, tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug):
    """-SOS.Trans file (SOS_PROC.F:3785-3822, formats 1005, 1006, 1010, 2010): the quantities of trans_quantities."""
    t_dir_down, t_dif_down, t_dif_up = trans_quantities(tetas, mu, ttot_tronc, ttot_vrai, tdifmus, tdifmug)
    with open(path, "w") as f:
        f.write("Solar Zenith Angle : %7.3f\n" % tetas)
        f.write("Direct transmission TOA -> surface : %8.4f\n" % t_dir_down)
        f.write("  \n")
        f.write(" Diffuse transmittance : TOA -> surface\n")
        f.write("    thetas = %6.3f   td(thetas) = %7.4f\n" % (tetas, t_dif_down))
        f.write("  \n")
        f.write(" Diffuse transmittance : surface -> TOA\n")
        for j in range(len(mu)):
            f.write("    thetav = %6.3f   td(thetav) = %7.4f\n" % (math.degrees(math.acos(mu[j])), t_dif_up[j]))


def write_flux_file(path, tetas, tdir_vrai, flux_diff_down, flux_down, eplus, zalt, tr, hr, ta, ha, tauabs):
    """-SOS.Flux file (SOS_PROC.F:3840-3874, formats 1005, 2016-2020)."""
    with open(path, "w") as f:
        f.write("Solar Zenith Angle : %7.3f\n" % tetas)
        f.write("  \n")
        f.write(" Downward fluxes at BOA (normalized by TOA solar flux)\n")
        f.write("   - Downward direct flux at BOA : %9.5f\n" % tdir_vrai)
        f.write("   - Downward diffuse flux at BOA: %9.5f\n" % flux_diff_down)
        f.write("   ==> Downward total flux at BOA: %9.5f\n" % flux_down)
        f.write("  \n")
        f.write(" Upward diffuse flux at TOA (normalized by TOA solar flux): %s\n" % repr(eplus))
        f.write("\n\n")
        f.write(" According to the following profile\n")
        f.write(" Z(km)    MOT     AOT     GOT     TOTAL\n")
        nl = len(zalt)
        for i in range(nl - 1, -1, -1):                       # I = CTE_ABS_NBLEV .. 1; TAUABS(CTE_ABS_NBLEV+1-I)
            z = zalt[i]
            trz, taz, tgz = tr * math.exp(-z / hr), ta * math.exp(-z / ha), tauabs[nl - 1 - i]
            f.write("%7.2f  %7.4f %7.4f %7.4f %7.4f\n" % (z, trz, taz, tgz, trz + taz + tgz))


def write_result_bin(path, rec):
    """Write aggregated Fourier records [F][3][W] (I,Q,U) as the reference's SOS_Result.bin: Fortran sequential
    unformatted, one record per order holding Q(-N:N), U(-N:N), I(-N:N) (SOS_OS.F:1572-1574)."""
    rec = np.asarray(rec, dtype="<f8")
    with open(path, "wb") as f:
        for s in range(rec.shape[0]):
            payload = np.concatenate([rec[s, 1], rec[s, 2], rec[s, 0]]).tobytes()
            m = np.array([len(payload)], "<i4").tobytes()
            f.write(m + payload + m)


# ---------------------------------------------------------------------------------------------------------
# SOS_Up.txt / SOS_Down.txt as the reference's command-line program writes them (SOS_ABS_MAIN.F:2250-2444)
# ---------------------------------------------------------------------------------------------------------
_SEP102 = "#" + "-" * 101
# (text, width of the `(Aw)` edit descriptor it is written with): the Fortran source is UTF-8, so the degree sign counts
# two bytes and the two "180 deg / 0 deg" lines lose their last character -- part of the file format as shipped
_HDR_COLS = [("#   VZA     :  Viewing Zenith Angle (in degrees)", 48), ("#   SCA_ANG :  Scattering angle (in degrees)", 44),
             ("#   I       :  Stokes parameter I at output altitude z (in sr-1)", 64),
             ("#              normalised to the extraterrestrial solar irradiance (PI * L(z) / Esun)", 85),
             ("#   Q       :  Stokes parameter Q at output altitude z (in sr-1)", 64),
             ("#              normalised to the extraterrestrial solar irradiance", 66),
             ("#   U       :  Stokes parameter U at output altitude z (in sr-1)", 64),
             ("#              normalised to the extraterrestrial solar irradiance ", 66),
             ("#   POL_ANG :  Polarization angle (in degrees).  Note: if undefined the value is -999.00", 88),
             ("#   POL_RATE:  Degree of polarization (in %)", 44),
             ("#   IPOL    :  Polarized intensity at level z (in sr-1)", 55),
             ("#              normalised to the extraterrestrial solar irradiance (PI * Lpol(z) / Esun)", 88)]
_SAT_180 = ("#        180° <-> Satellite and Sun in the same half-plane", 58)
_SAT_0 = ("#          0° <-> Satellite and Sun in opposite half-planes with respect to the zenith direction", 96)


def _fmt_a(text, width):
    """Fortran `(Aw)` of a character constant: the first w BYTES of the UTF-8 source text when it is longer, right-justified in w
    columns when shorter; list-directed trailing blanks are kept by the runtime, not added here (flang trims none)."""
    b = text.encode("utf-8")
    return (b" " * (width - len(b)) + b) if len(b) < width else b[:width]


def main_output_header(itrphi, updown, zalt, phios=0.0):
    """SOS_OUTPUT_HEADER (fixed azimuth, SOS_TRPHI.F:1570-1680) / SOS_OUTPUT_HEADER_POLAR_DIAG (:1705-1796) as bytes."""
    up = updown == 1
    lines = []
    if itrphi == 1:
        lines.append(_fmt_a("# UPWARD RADIANCE FIELD VERSUS THE VIEWING ZENITH ANGLE", 55) if up else
                     _fmt_a("# DOWNWARD RADIANCE FIELD VERSUS THE VIEWING ZENITH ANGLE", 57))
        lines += [_fmt_a("# (RELATIVE AZIMUTH AND ALTITUDE ARE FIXED)", 43), _fmt_a(_SEP102, 102),
                  _fmt_a("# Relative azimuth (degrees) :", 30), b"#", _fmt_a("#      Relative azimuth convention :", 36)]
        if up:
            lines += [_fmt_a(*_SAT_180), _fmt_a(*_SAT_0)]
        else:
            lines += [_fmt_a("#        180° <-> Viewing direction and Sun in the same half-plane", 66),
                      _fmt_a("#          0° <-> Viewing direction and Sun in opposite half-planes with respect to the zenith "
                             "direction", 104)]
        lines += [b"#", _fmt_a("#      Simulated relative azimuth (degrees) :", 45),
                  _fmt_a("#          for VZA < 0 (sign convention):", 41) + b" " + ("%7.3f" % (phios + 180.0)).encode(),
                  _fmt_a("#          for VZA > 0 (sign convention):", 41) + b" " + ("%7.3f" % phios).encode(), b"#"]
    else:
        lines.append(_fmt_a("#UPWARD RADIANCE FIELD VERSUS THE AZIMUTH ANGLE AND VIEWING ZENITH ANGLE", 72) if up else
                     _fmt_a("#DOWNWARD RADIANCE FIELD VERSUS THE AZIMUTH ANGLE AND VIEWING ZENITH ANGLE", 74))
        lines += [_fmt_a("#(ALTITUDE FIXED)", 17), _fmt_a(_SEP102, 102), _fmt_a("# Relative azimuth convention :", 31),
                  _fmt_a(*_SAT_180), _fmt_a(*_SAT_0), b"#"]
    lines += [_fmt_a("# Value of the selected altitude for the output (km) :", 54) + b" " + ("%7.3f" % zalt).encode(), b"#",
              _fmt_a("# Columns parameters :", 22)]
    if itrphi != 1:
        lines.append(_fmt_a("#   PHI     :  Relative azimuth Angle (in degrees)", 50))
    lines += [_fmt_a(t, w) for t, w in _HDR_COLS]
    lines.append(_fmt_a(_SEP102, 102))
    if itrphi == 1:
        lines += [_fmt_a("#   VZA     SCA_ANG       I              Q              U         POL_ANG  POL_RATE    IPOL", 91),
                  _fmt_a("#(degrees) (degrees)    (sr-1)         (sr-1)         (sr-1)      (degrees)  (%)      (sr-1)", 92)]
    else:
        lines += [_fmt_a("#   PHI      VZA     SCA_ANG        I              Q              U       POL_ANG  POL_RATE    IPOL", 99),
                  _fmt_a("#(degrees) (degrees) (degrees)    (sr-1)         (sr-1)         (sr-1)    (degrees)  (%)      (sr-1)", 100)]
    return b"".join(ln + b"\n" for ln in lines)


def _f7_2(x):
    s = "%7.2f" % x
    return s if len(s) == 7 else "*" * 7                       # Fw.d overflow


def write_main_output(path_up, path_down, outputs, itrphi, phios, pas_phi, zout, user_up=None, user_down=None):
    """The two ASCII result files of the reference's command-line program, byte for byte: headers of SOS_OUTPUT_HEADER*,
    then format 55 `2(2X,F7.2),2X,3(E13.6,2X),2(F7.2,2X),E13.6` (fixed azimuth: the phi + 180 half plane with negated zenith
    angles in reversed order, then the phi half plane, SOS_ABS_MAIN.F:2304-2405) or format 56
    `3(2X,F7.2),1X,3(E13.6,2X),2(1X,F7.2),E13.6` (polar diagram, :2450-2496).  outputs: the 23-tuple of sos_proc.
    user_up / user_down: optional paths of the -SOS.ResFileUp.UserAng / -SOS.ResFileDown.UserAng files (user angles only,
    IND_ANGOUT = 1).  One quirk of the reference is kept: in the polar diagram the SCA_ANG column of the UPWARD file is read
    from row IPHI (the azimuth in degrees) of the table instead of the azimuth's row IP (SOS_ABS_MAIN.F:2466) -- with
    -SOS.View.Dphi > 1 it holds another azimuth's angle, or 0."""
    (nblum, ind_ang, phi, vza, sca_up, i_up, q_up, u_up, ang_up, rate_up, lpol_up,
     sca_dn, i_dn, q_dn, u_dn, ang_dn, rate_dn, lpol_dn) = outputs[:18]
    zal_up, zal_dn = (CTE_TOA_ALT, 0.0) if zout == -1 else (zout, zout)
    up = [main_output_header(itrphi, 1, zal_up, phios)]
    dn = [main_output_header(itrphi, 2, zal_dn, phios)]
    uu, ud = list(up), list(dn)

    def rec55(th, sca, xi, xq, xu, xan, tpol, lpol):
        return ("  %s  %s  %s  %s  %s  %s  %s  %s\n" % (_f7_2(th), _f7_2(sca), fortran_e(xi, 13, 6), fortran_e(xq, 13, 6),
                                                      fortran_e(xu, 13, 6), _f7_2(xan), _f7_2(tpol), fortran_e(lpol, 13, 6))).encode()

    def rec56(ph, th, sca, xi, xq, xu, xan, tpol, lpol):
        return ("  %s  %s  %s %s  %s  %s   %s %s%s\n" % (_f7_2(ph), _f7_2(th), _f7_2(sca), fortran_e(xi, 13, 6), fortran_e(xq, 13, 6),
                                                        fortran_e(xu, 13, 6), _f7_2(xan), _f7_2(tpol), fortran_e(lpol, 13, 6))).encode()

    if itrphi == 1:
        for row, order, sign in ((0, range(nblum - 1, -1, -1), -1.0), (1, range(nblum), 1.0)):
            for j in order:
                a = rec55(sign * vza[j], sca_up[row, j], i_up[row, j], q_up[row, j], u_up[row, j], ang_up[row, j], rate_up[row, j],
                          lpol_up[row, j])
                b = rec55(sign * vza[j], sca_dn[row, j], i_dn[row, j], q_dn[row, j], u_dn[row, j], ang_dn[row, j], rate_dn[row, j],
                          lpol_dn[row, j])
                up.append(a); dn.append(b)
                if ind_ang[j] == 1:
                    uu.append(a); ud.append(b)
    else:
        for ip, iphi in enumerate(range(0, 361, int(pas_phi))):
            for j in range(nblum):
                rest = (i_up[ip, j], q_up[ip, j], u_up[ip, j], ang_up[ip, j], rate_up[ip, j], lpol_up[ip, j])
                up.append(rec56(phi[ip], vza[j], sca_up[iphi, j], *rest))          # row IPHI: the reference's own indexing
                b = rec56(phi[ip], vza[j], sca_dn[ip, j], i_dn[ip, j], q_dn[ip, j], u_dn[ip, j], ang_dn[ip, j], rate_dn[ip, j],
                          lpol_dn[ip, j])
                dn.append(b)
                if ind_ang[j] == 1:
                    uu.append(rec56(phi[ip], vza[j], sca_up[ip, j], *rest))
                    ud.append(b)
    for path, parts in ((path_up, up), (path_down, dn), (user_up, uu), (user_down, ud)):
        if path:
            with open(path, "wb") as f:
                f.write(b"".join(parts))


_HDR_SEP = "#" + "-" * 101 + "\n"
_HDR_COLUMNS = [           # (name, description lines) of the SOS_Up.txt / SOS_Down.txt columns (binding/run_sos.py:255-270)
    ("VZA", ["Viewing Zenith Angle (in degrees)"]),
    ("SCA_ANG", ["Scattering angle (in degrees)"]),
    ("I", ["Stokes parameter I at output altitude z (in sr-1)",
           "normalised to the extraterrestrial solar irradiance (PI * L(z) / Esun)",
           "normalised to the extraterrestrial solar irradiance"]),
    ("Q", ["Stokes parameter Q at output altitude z (in sr-1)", "normalised to the extraterrestrial solar irradiance "]),
    ("U", ["Stokes parameter U at output altitude z (in sr-1)", "normalised to the extraterrestrial solar irradiance "]),
    ("POL_ANG", ["Polarization angle (in degrees). Note: if undefined the value is -999.00"]),
    ("POL_RATE", ["Degree of polarization (in %)"]),
    ("IPOL", ["Polarized intensity at level z (in sr-1)",
              "normalised to the extraterrestrial solar irradiance (PI * Lpol(z) / Esun)"]),
]


def gen_hdr_sos_output(sos_view, updown, zalt):
    """Header of SOS_Up.txt (updown = 1) / SOS_Down.txt (2), the text of binding/run_sos.py:219-278.  One deliberate
    difference: the reference tests `sosView == 1 & updown == 2` (operator precedence makes it always false); here the
    down-looking, fixed-azimuth file gets the 'Viewing direction' wording the reference meant it to have."""
    plane = sos_view == 1
    lines = ["#%s RADIANCE FIELD VERSUS %sVIEWING ZENITH ANGLE\n" % ("UPWARD" if updown == 1 else "DOWNWARD",
                                                                      "THE AZIMUTH ANGLE AND " if plane else ""),
             "# (RELATIVE AZIMUTH AND ALTITUDE ARE FIXED)\n" if plane else "# (ALTITUDE IS FIXED)", _HDR_SEP]
    if plane:
        lines.append("# Relative azimuth (degrees) :\n#\n")
    who = "Viewing direction" if (plane and updown == 2) else "Satellite"
    lines += ["#      Relative azimuth convention :\n",
              "#        180 deg <-> %s and Sun in the same half-plane\n" % who,
              "#          0 deg <-> %s and Sun in opposite half-planes with respect to the zenith direction\n#\n" % who,
              "# Value of the selected altitude for the output (km) : %s\n#\n" % zalt, "# Columns parameters :\n"]
    cols = ([("PHI", ["Relative azimuth Angle (in degrees)"])] if not plane else []) + _HDR_COLUMNS
    for name, desc in cols:
        lines.append("#   %-8s:  %s\n" % (name, desc[0]))
        lines += ["#              %s\n" % d for d in desc[1:]]
    lines.append(_HDR_SEP)
    lines.append("#   %sVZA     SCA_ANG        I              Q              U       POL_ANG  POL_RATE    IPOL\n"
                 % ("" if plane else "PHI      "))
    lines.append("#%s(degrees) (degrees)  (no unit)      (no unit)      (no unit)   (degrees) (pcts)  (no unit)\n"
                 % ("" if plane else "(degrees) "))
    return "".join(lines)


def gen_sos_output(rep_out, sos_view, updown, zalt, nblum, pas_phi, phi, vza, sca_ang, i_out, q_out, u_out,
                   pol_ang_out, pol_rate_out, l_pol_out):
    """run_sos.py:280-317: SOS_Up.txt / SOS_Down.txt (header + data block).  Fixed-azimuth view: the phi + 180 half plane
    first (negated zenith angles, reversed order), then the phi half plane."""
    name = "SOS_Up.txt" if updown == 1 else "SOS_Down.txt"
    with open(os.path.join(rep_out, name), "w") as fic:
        fic.write(gen_hdr_sos_output(sos_view, updown, zalt))
        if sos_view == 1:
            for it in range(nblum - 1, -1, -1):
                fic.write("  %7.2f %7.2f  %13.6e  %13.6e  %13.6e  %7.2f %7.2f %13.6e\n" % (
                    -vza[it], sca_ang[0, it], i_out[0, it], q_out[0, it], u_out[0, it], pol_ang_out[0, it],
                    pol_rate_out[0, it], l_pol_out[0, it]))
            for it in range(nblum):
                fic.write("  %7.2f %7.2f  %13.6e  %13.6e  %13.6e  %7.2f %7.2f %13.6e\n" % (
                    vza[it], sca_ang[1, it], i_out[1, it], q_out[1, it], u_out[1, it], pol_ang_out[1, it],
                    pol_rate_out[1, it], l_pol_out[1, it]))
        else:
            nbphi = math.ceil(360. / pas_phi)
            for ip in range(nbphi):
                for it in range(nblum):
                    fic.write(" %7.2f %7.2f %7.2f  %13.6e  %13.6e  %13.6e  %7.2f %7.2f %13.6e\n" % (
                        phi[ip], vza[it], sca_ang[ip, it], i_out[ip, it], q_out[ip, it], u_out[ip, it],
                        pol_ang_out[ip, it], pol_rate_out[ip, it], l_pol_out[ip, it]))
