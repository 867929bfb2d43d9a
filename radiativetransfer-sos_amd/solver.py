"""Host-side driver of the MI355X hot path: one `SosContext` per wavelength, batches of CKD bins solved
by the fused HIP kernel, aggregation on device.  torch is used for device memory and streams only; all
arithmetic happens in libsosgpu.so (capi.py), and there is no CPU fallback.

Mirrors the reference per-wavelength sequence of SOS_PROC (src/SOS_PROC.F:3423-3594):
  SOS_PREPA_OS -> [per bin: SOS (truncation rescale) -> SOS_OS -> SOS_AGGREGATE].
"""
import collections
import ctypes as C
import math
import threading

import numpy as np
import torch

from . import capi
from .synth import MDF_DEFAULT


class SosBinError(RuntimeError):
    """A bin of the batch is malformed / needs more than CTE_OS_NT levels: the reference's IER = -1
    (SOS_OS.F:1627-1648, SOS_PROFIL.F)."""
    ier = -1


def _dev_f64(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float64).contiguous()
    a = np.ascontiguousarray(x, dtype=np.float64)
    if not a.flags.writeable:                      # (cached read-only tables: torch wants a writable buffer to wrap)
        a = a.copy()
    return _upload(torch.from_numpy(a), device)


def _upload(t, device):
    """Host tensor -> device on the current stream without a host wait: through a pinned staging block of torch's host
    allocator (returned to it when the copy has passed).  A pageable `.to(device)` waits for the stream -- behind whatever
    preparation kernels sos_spectrum has queued there."""
    if t.numel() == 0 or t.numel() * t.element_size() > (4 << 20) or torch.device(device).type != "cuda":
        return t.to(device)                        # (large tables: uploaded once per batch, not worth a pinned block)
    return t.pin_memory().to(device, non_blocking=True)


def _dev_i32(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.int32).contiguous()
    return _upload(torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)), device)


_CONST_DEV = collections.OrderedDict()
_CONST_LOCK = threading.Lock()


def _const_dev_f64(x, device):
    """Device copy of a SMALL host array that repeats from call to call (altitude grid of the gas profiles, azimuth list of a
    view): kept per (content, device) -- a pageable upload is a host-synchronous 30 us, a spectrum makes thousands of them."""
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.nbytes > 8192:
        return _dev_f64(a, device)
    key = (a.tobytes(), str(device))
    with _CONST_LOCK:
        hit = _CONST_DEV.get(key)
        if hit is not None:
            _CONST_DEV.move_to_end(key)
            return hit
    t = torch.from_numpy(a.copy()).to(device)              # (synchronous copy: complete, usable from any stream)
    with _CONST_LOCK:
        _CONST_DEV[key] = t
        while len(_CONST_DEV) > 64:
            _CONST_DEV.popitem(last=False)
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _work_area(need, device):
    """The work area of a table-form call (include/sosgpu.h, "Work areas"): `need` bytes, as the call's _work_bytes query gave
    them, from torch's allocator -- which keeps an area dropped at return for the stream it was used on.  Never empty (an empty
    tensor has a NULL pointer): with need = 0 the call refuses, or queues nothing, with a code of its own.  The call takes
    _ptr(area) and need."""
    return torch.empty(max(int(need), 8), dtype=torch.uint8, device=device)


def _ckd_table_ptr(tables, dev):
    """table_ptr of pack_ckd_requests on a GPU: absorption.ckd_device_tables of each interval file, made once and kept in
    `tables` (id(prep) -> (prep, addresses, tensors)) for as long as the launch needs them."""
    from . import absorption as _abs

    def table_ptr(prep, k):
        hit = tables.get(id(prep))
        if hit is None:
            hit = tables[id(prep)] = (prep,) + _abs.ckd_device_tables(prep, dev)
        return hit[1][k]
    return table_ptr


def nogas_profile(tr, hr, ta, ha, device=0):
    """Queue the no-gas profile of a wavelength (SOS_PROFIL.F:349-489) on the current stream ahead of make_profiles
    (sosgpu_profile_nogas): its level placement is a ~1 ms serial chain on one wavefront that only needs the two optical
    thicknesses and scale heights, so it can run while the host is still preparing the wavelength.  Returns the device block
    to pass to SosContext.make_profiles(nogas=...)."""
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    ng = torch.empty(4 * capi.NOGAS_LEVELS, dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    capi.check(capi.lib().sosgpu_profile_nogas(dev.index or 0, float(tr), float(hr), float(ta), float(ha), _ptr(ng), st),
               "sosgpu_profile_nogas")
    return ng


SEG = None          # run_sos._seg when SOS_PREPARE_SEGMENTS is set (host-time diagnostic), else None


def output_levels_host(zprof, altitudes):
    """Output levels of several altitudes for host profiles (upload_bins with zprof: the aerosol-layer profile): the rule
    upload_bins applies to one zout (SOS_OS.F:1514-1520, first level J with ZOUT >= ZPROF(J), linear weight ZZ), once per
    altitude.  zprof[nb][L]; returns jout[K][nb] (int32) and zz[K][nb]; -1 gives the standard output (0, 0)."""
    zprof = np.atleast_2d(np.asarray(zprof, dtype=np.float64))
    nb = zprof.shape[0]
    alts = [float(z) for z in altitudes]
    jout = np.zeros((len(alts), nb), dtype=np.int32)
    zz = np.zeros((len(alts), nb))
    for k, zout in enumerate(alts):
        if zout == -1.0:
            continue
        for b in range(nb):
            j = 1
            while zout < zprof[b, j]:
                j += 1
            jout[k, b] = j
            zz[k, b] = (zout - zprof[b, j - 1]) / (zprof[b, j] - zprof[b, j - 1])
    return jout, zz


def host_output_levels(bins, altitudes):
    """The `levels` of SosContext.output_levels for bins of upload_bins (host level altitudes zprof_host, or none: standard
    output only), on the device of bins["prof"]: output_levels_host, TAUOUT from the uploaded H as run_sos computes it for
    one altitude (SOS.F:567-581).  Bins uploaded with hvrai (the untruncated H) also get `tauvrai`, by the same statements."""
    alts = [float(z) for z in altitudes]
    nz, nb, d = len(alts), bins["nb"], bins["prof"].device
    if bins.get("zprof_host") is None and any(z != -1.0 for z in alts):
        raise ValueError("output altitudes need the bins' level altitudes (make_profiles, or upload_bins with zprof)")
    zp = bins.get("zprof_host")
    jh, zh = output_levels_host(zp, alts) if zp is not None else (np.zeros((nz, nb), np.int32), np.zeros((nz, nb)))
    h = bins["prof"][:, 0, :].cpu().numpy()
    th = np.zeros((nz, nb))
    for k in range(nz):
        for b in range(nb):
            j, zzv = int(jh[k, b]), float(zh[k, b])
            th[k, b] = h[b, 0] if alts[k] == -1.0 else (1 - zzv) * h[b, j - 1] + zzv * h[b, j]
    levels = dict(nz=nz, jout=_dev_i32(jh, d), zz=_dev_f64(zh, d), tauout=_dev_f64(th, d))
    if bins.get("hvrai") is not None:
        hv = bins["hvrai"].cpu().numpy()
        tv = np.zeros((nz, nb))
        for k in range(nz):
            for b in range(nb):
                j, zzv = int(jh[k, b]), float(zh[k, b])
                tv[k, b] = hv[b, 0] if alts[k] == -1.0 else (1 - zzv) * hv[b, j - 1] + zzv * hv[b, j]
        levels["tauvrai"] = _dev_f64(tv, d)
    return levels


class SosContext:
    """Everything SOS_OS needs that does not depend on the CKD bin (angles, phase-matrix expansion,
    surface), resident on one GPU, with the Fourier kernels of every order precomputed
    (sosgpu_noyaux, replaces SOS_NOYAUX SOS_OS.F:1857).
    build=False: the constructor stops after sosgpu_create -- the surface matrices are kept, nothing is queued -- and
    build_operators() fills the operator tables of many such contexts in one call; solving before that is an error.
    create=False (with build=False): the constructor does everything but sosgpu_create -- the context is PENDING, its handle
    null and its arguments kept -- and create_contexts() makes the contexts of many such objects in one sosgpu_create_spectrum
    call; a method that needs the handle before that raises, close() does nothing."""

    def __init__(self, mu, ga, n0, alpha, beta, gamma, zeta, *, iborm_max=None, ro=0.0, imat_surf=0,
                 ifresnel=0, ind_surf=1.34, ron=MDF_DEFAULT, ipolar=1, igmax=100, rsurf=None, device=0, build=True, create=True):
        if not create and build:
            raise ValueError("create=False needs build=False: the operators are built on a created context")
        if not torch.cuda.is_available():
            raise RuntimeError("SosContext needs a GPU (gfx950); there is no CPU fallback in the product path")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.n = int(len(mu))
        self.w = 2 * self.n + 1
        self.os_nb = int(len(beta) - 1)
        self.smax = self.os_nb if iborm_max is None else int(iborm_max)
        self.n0 = int(n0)
        self.mu = np.ascontiguousarray(mu, dtype=np.float64)
        self.ga = np.ascontiguousarray(ga, dtype=np.float64)
        coefs = [np.ascontiguousarray(x, dtype=np.float64) for x in (alpha, beta, gamma, zeta)]
        self._coefs = coefs
        self._opts = dict(ind_surf=float(ind_surf), ron=float(ron), ipolar=int(ipolar), igmax=int(igmax))
        for x in coefs:
            if len(x) != self.os_nb + 1:
                raise ValueError("alpha/beta/gamma/zeta must all have os_nb+1 entries")
        wv = capi.Wave(n=self.n, os_nb=self.os_nb, n0=self.n0, imat_surf=int(imat_surf), ifresnel=int(ifresnel),
                       ipolar=int(ipolar), igmax=int(igmax), reserved=0, ro=float(ro), ind_surf=float(ind_surf),
                       ron=float(ron))
        self._handle = C.c_void_p()
        self._pending = None
        L = capi.lib()
        dp = lambda a: a.ctypes.data_as(C.c_void_p)
        SEG and SEG("context: python")
        if create:
            capi.check(L.sosgpu_create(C.byref(self._handle), self.device.index or 0, C.byref(wv), dp(self.mu), dp(self.ga),
                                       dp(coefs[0]), dp(coefs[1]), dp(coefs[2]), dp(coefs[3]), self.smax),
                       "sosgpu_create")
            SEG and SEG("context: sosgpu_create")
        else:
            # (the arrays the spec points to are the object's own: they live as long as it does)
            self._pending = capi.CtxSpec(wv=wv, mu=self.mu.ctypes.data, ga=self.ga.ctypes.data, alpha=coefs[0].ctypes.data,
                                         beta=coefs[1].ctypes.data, gamma=coefs[2].ctypes.data, zeta=coefs[3].ctypes.data,
                                         iborm_max=self.smax, reserved=0)
        self._rsurf = None
        self._built = False
        if int(imat_surf) == 1:
            if rsurf is None:
                raise ValueError("imat_surf=1 needs rsurf[smax+1][9][N][N] (float32)")
            if isinstance(rsurf, torch.Tensor):
                r = rsurf.to(device=self.device, dtype=torch.float32).contiguous()
            else:
                r = torch.from_numpy(np.ascontiguousarray(rsurf, dtype=np.float32)).to(self.device)
            if tuple(r.shape) != (self.smax + 1, 9, self.n, self.n):
                raise ValueError("rsurf shape %s != %s" % (tuple(r.shape), (self.smax + 1, 9, self.n, self.n)))
            self._rsurf = r               # kept alive: the packing (below, or build_operators') is only queued
            if build:
                capi.check(L.sosgpu_set_surface_matrices_async(self._h, _ptr(r), self._stream()),
                           "sosgpu_set_surface_matrices_async")
                SEG and SEG("context: surface matrices")
        if build:
            self.noyaux()
            SEG and SEG("context: sosgpu_noyaux")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def _h(self):
        """The library's handle of the context: every call that takes one reads it here."""
        if self._pending is not None:
            raise RuntimeError("this context was created with create=False: call solver.create_contexts first")
        return self._handle

    def noyaux(self):
        capi.check(capi.lib().sosgpu_noyaux(self._h, self._stream()), "sosgpu_noyaux")
        self._built = True

    def _need_operators(self):
        if not self._built:
            raise RuntimeError("this context was created with build=False: call solver.build_operators first")

    def noyaux_fetch(self, is_):
        """Kernels of Fourier order is_ in the reference layout (parity accessor)."""
        w = self.w
        out = np.zeros(6 * w * w + 3 * w)
        torch.cuda.synchronize(self.device)
        capi.check(capi.lib().sosgpu_noyaux_fetch(self._h, int(is_), out.ctypes.data_as(C.c_void_p)), "sosgpu_noyaux_fetch")
        names = ["BP", "GR", "GT", "ARR", "ART", "ATT"]
        d = {k: out[i * w * w:(i + 1) * w * w].reshape(w, w) for i, k in enumerate(names)}
        for i, k in enumerate(["XPL", "XRL", "XTL"]):
            d[k] = out[6 * w * w + i * w:6 * w * w + (i + 1) * w]
        return d

    def debug_tables(self):
        """The context's per-wavelength tables and their layout numbers on the host (sosgpu_debug_tables; read-only):
        dict of the TablesInfo fields plus prt, mp_aer, mp_vt, mp_uf, sv, rowmap and -- with surface matrices -- mp_gnd, rdir."""
        L = capi.lib()
        info = capi.TablesInfo()
        capi.check(L.sosgpu_debug_tables(self._h, C.byref(info), *([None] * 8)), "sosgpu_debug_tables")
        t = {k: getattr(info, k) for k, _ in capi.TablesInfo._fields_}
        s1, per = t["smax"] + 1, t["rtph"] * t["ks2h"] * 128
        a = dict(prt=np.zeros((s1, 3, t["os_nb"] + 1, t["w"])), mp_aer=np.zeros((s1, 2, per)),
                 mp_vt=np.zeros((3, t["ks2h"] * 128)), mp_uf=np.zeros((3, t["rtph"] * 64)), sv=np.zeros((s1, 4, t["kp"])),
                 mp_gnd=np.zeros((s1, per)) if self._rsurf is not None else None,
                 rdir=np.zeros((s1, 3, t["n"])) if self._rsurf is not None else None,
                 rowmap=np.zeros(t["kh"], dtype=np.int32))
        ptr = [None if a[k] is None else a[k].ctypes.data_as(C.c_void_p)
               for k in ("prt", "mp_aer", "mp_vt", "mp_uf", "sv", "mp_gnd", "rdir", "rowmap")]
        capi.check(L.sosgpu_debug_tables(self._h, C.byref(info), *ptr), "sosgpu_debug_tables")
        t.update({k: v for k, v in a.items() if v is not None})
        return t

    def upload_bins(self, h, xdel, ydel, nt=None, iborm=None, zout=-1.0, zprof=None, order=None, hvrai=None):
        """Pack per-bin profiles (after the SOS.F rescale) into the device layout of sosgpu_os_solve.
        h/xdel/ydel: [nb][L] arrays (ragged bins: pass nt[nb] and pad).
        order="cost": bins are permuted by decreasing total optical depth before upload (the returned dict holds
        `perm`, with result[i] belonging to input bin perm[i]).  Bins of similar cost then run side by side, drift
        less across Fourier orders and keep re-reading the same source operators from L2 (scheduling only: every
        bin's result is unchanged).
        hvrai: optional [nb][L], the cumulative optical depth BEFORE the truncation rescale (the untruncated depth): uploaded
        as bins["hvrai"][nb][lp], from which output_levels forms the true depth down to each altitude (`tauvrai`)."""
        h = np.atleast_2d(np.asarray(h, dtype=np.float64))
        xdel = np.atleast_2d(np.asarray(xdel, dtype=np.float64))
        ydel = np.atleast_2d(np.asarray(ydel, dtype=np.float64))
        nb, lmax = h.shape
        nt = np.full(nb, lmax - 1, dtype=np.int32) if nt is None else np.asarray(nt, dtype=np.int32)
        perm = None
        if order == "cost":
            perm = np.argsort(-h[np.arange(nb), nt], kind="stable")
            h, xdel, ydel, nt = h[perm], xdel[perm], ydel[perm], nt[perm]
            if hvrai is not None:
                hvrai = np.atleast_2d(np.asarray(hvrai, dtype=np.float64))[perm]
            if iborm is not None and np.ndim(iborm):
                iborm = np.asarray(iborm)[perm]
            if zprof is not None:
                zprof = np.atleast_2d(np.asarray(zprof, dtype=np.float64))[perm]
        lp = int(-(-lmax // 16) * 16)
        prof = np.zeros((nb, 3, lp))
        prof[:, 0, :lmax], prof[:, 1, :lmax], prof[:, 2, :lmax] = h, xdel, ydel
        if iborm is None:
            # SOS.F:549-550: IBORM = 2 for a purely molecular bin, OS_NB otherwise
            iborm = np.where(np.any(xdel != 0.0, axis=1), self.smax, min(2, self.smax)).astype(np.int32)
        iborm = np.broadcast_to(np.asarray(iborm, dtype=np.int32), (nb,)).copy()
        jout = zz = None
        if zout != -1.0:
            jout, zz = (x[0] for x in output_levels_host(zprof, [zout]))
        d = self.device
        out = dict(nb=nb, lp=lp, perm=perm, nt=_dev_i32(nt, d), iborm=_dev_i32(iborm, d), prof=_dev_f64(prof, d),
                   jout=None if jout is None else _dev_i32(jout, d), zz=None if zz is None else _dev_f64(zz, d),
                   zprof_host=None if zprof is None else np.atleast_2d(np.asarray(zprof, dtype=np.float64)))
        if hvrai is not None:
            hv = np.atleast_2d(np.asarray(hvrai, dtype=np.float64))
            if hv.shape != h.shape:
                raise ValueError("hvrai must have the shape of h")
            hp = np.zeros((nb, lp))
            hp[:, :lmax] = hv
            out["hvrai"] = _dev_f64(hp, d)
        return out

    def absorption_profiles(self, ik, xk, ro):
        """SOS_ABSPROFILE (SOS_ABSPROFILE.F:325-371) of every CKD bin on the device (sosgpu_absprofile): ik[nb][8] 1-based
        exponential term per gas, xk[8][nterm][nlev-1] / ro[8][nlev-1] from absorption.layer_tables.  Returns the device
        tensor tabs[nb][nlev] that make_profiles takes."""
        d = self.device
        if isinstance(ik, torch.Tensor) or isinstance(xk, torch.Tensor) or isinstance(ro, torch.Tensor):
            ik_t = _dev_i32(ik, d)
            xk_t, ro_t = _dev_f64(xk, d), _dev_f64(ro, d)
        else:
            # one upload for the three tables (8-byte units; a bin's eight int32 indices are four of them)
            ik_h = np.ascontiguousarray(ik, dtype=np.int32)
            xk_h, ro_h = np.ascontiguousarray(xk, dtype=np.float64), np.ascontiguousarray(ro, dtype=np.float64)
            if ik_h.ndim != 2 or ik_h.shape[1] != 8:
                raise ValueError("ik must be [nb][8], xk [8][nterm][nlev-1], ro [8][nlev-1]")
            buf = _upload(torch.from_numpy(np.concatenate([xk_h.ravel(), ro_h.ravel(), ik_h.ravel().view(np.float64)])), d)
            xk_t = buf[:xk_h.size].view(xk_h.shape)
            ro_t = buf[xk_h.size:xk_h.size + ro_h.size].view(ro_h.shape)
            ik_t = buf[xk_h.size + ro_h.size:].view(torch.int32).view(ik_h.shape)
        nb, nterm, nlev = int(ik_t.shape[0]), int(xk_t.shape[1]), int(xk_t.shape[2]) + 1
        if tuple(ik_t.shape) != (nb, 8) or xk_t.shape[0] != 8 or tuple(ro_t.shape) != (8, nlev - 1):
            raise ValueError("ik must be [nb][8], xk [8][nterm][nlev-1], ro [8][nlev-1]")
        tabs = torch.empty((nb, nlev), dtype=torch.float64, device=d)
        capi.check(capi.lib().sosgpu_absprofile(d.index or 0, nb, nlev, nterm, _ptr(ik_t), _ptr(xk_t), _ptr(ro_t), _ptr(tabs),
                                                self._stream()), "sosgpu_absprofile")
        return tabs

    def make_profiles(self, nb, tr, hr, ta, ha, altabs=None, tabs=None, *, a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0,
                      lp=608, absprofil=1, nogas=None, true_depth=False):
        """SOS_PROFILE (IPROFIL=1) + SOS_DISC + the SOS.F rescale for nb CKD bins ON THE DEVICE (sosgpu_profile):
        tabs[nb][nblev] is each bin's cumulative gas absorption optical depth on the descending altitude grid
        altabs[nblev] (None: no gas).  Returns the same dict upload_bins returns (ready for solve()), plus `zprof` and
        the per-bin scalars `scal` [nb][4] = {0, TTOT_TRONC, TTOT_VRAI, TAUOUT} that aggregate() takes.
        Bins whose profile needs more than CTE_OS_NT levels come back with nt = -1 (the reference's IER = -1).
        nogas: the block nogas_profile(tr, hr, ta, ha) queued earlier on this stream (head start), or None.
        true_depth=True (sosgpu_profile_true): the dict also holds `hvrai` [nb][lp], the cumulative optical depth of every
        level before the truncation rescale -- the untruncated depth, hvrai[b][nt] = TTOT_VRAI -- from which output_levels
        forms `tauvrai`; everything else keeps its bits."""
        d = self.device
        t_alt = t_tab = None
        nblev = 0
        if tabs is not None:
            t_tab = tabs if isinstance(tabs, torch.Tensor) else np.atleast_2d(np.asarray(tabs, dtype=np.float64))
            t_tab = _dev_f64(t_tab, d)
            t_alt = _const_dev_f64(altabs, d)
            nblev = int(t_alt.numel())
            if t_tab.shape != (nb, nblev):
                raise ValueError("tabs must be [nb][len(altabs)]")
        # (two cleared blocks instead of seven: a band has 1-125 bins, each fill is a launch)
        fb = torch.zeros(nb * (4 * lp + 5) + (nb * lp if true_depth else 0), dtype=torch.float64, device=d)
        ib = torch.zeros(3 * nb, dtype=torch.int32, device=d)
        prof = fb[:nb * 3 * lp].view(nb, 3, lp)
        zprof = fb[nb * 3 * lp:nb * 4 * lp].view(nb, lp)
        scal = fb[nb * 4 * lp:nb * (4 * lp + 4)].view(nb, 4)
        nt, iborm = ib[:nb], ib[nb:2 * nb]
        jout = zz = None
        if zout != -1.0:
            jout = ib[2 * nb:]
            zz = fb[nb * (4 * lp + 4):nb * (4 * lp + 5)]
        args = (self._h, nb, tr, hr, ta, ha, int(absprofil), nblev, _ptr(t_alt), _ptr(t_tab), a_tronc, piz, piztr, zout, lp,
                _ptr(prof), _ptr(nt), _ptr(iborm), _ptr(zprof), _ptr(jout), _ptr(zz), _ptr(scal), _ptr(nogas))
        bins = dict(nb=nb, lp=lp, perm=None, nt=nt, iborm=iborm, prof=prof, jout=jout, zz=zz, zprof=zprof, scal=scal)
        if true_depth:
            bins["hvrai"] = fb[nb * (4 * lp + 5):].view(nb, lp)
            capi.check(capi.lib().sosgpu_profile_true(*args, _ptr(bins["hvrai"]), self._stream()), "sosgpu_profile_true")
        else:
            capi.check(capi.lib().sosgpu_profile(*args, self._stream()), "sosgpu_profile")
        return bins

    def make_layer_profile(self, tr, hr, ta, zmin, zmax, *, a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, lp=608,
                           true_depth=False):
        """SOS_PROFILE for IPROFIL = 2 (an aerosol layer between zmin and zmax km, no gas) + the SOS.F rescale ON THE DEVICE
        (sosgpu_profile_layer): the dict make_profiles returns for one bin -- device `zprof` and `scal`, `hvrai` with
        true_depth=True.  The refusals of the level grid (geometry.layer_grid) come back as the library's error before
        anything is queued; a profile that does not fit lp has nt = -1."""
        d = self.device
        # (one cleared block: the doubles, then nt, iborm and jout as int32 in its last two doubles)
        nd = 4 * lp + 5 + (lp if true_depth else 0)
        fb = torch.zeros(nd + 2, dtype=torch.float64, device=d)
        ib = fb[nd:].view(torch.int32)
        prof, zprof, scal = fb[:3 * lp].view(1, 3, lp), fb[3 * lp:4 * lp].view(1, lp), fb[4 * lp:4 * lp + 4].view(1, 4)
        nt, iborm = ib[0:1], ib[1:2]
        jout = zz = None
        if zout != -1.0:
            jout, zz = ib[2:3], fb[4 * lp + 4:4 * lp + 5]
        bins = dict(nb=1, lp=lp, perm=None, nt=nt, iborm=iborm, prof=prof, jout=jout, zz=zz, zprof=zprof, scal=scal)
        if true_depth:
            bins["hvrai"] = fb[4 * lp + 5:nd].view(1, lp)
        capi.check(capi.lib().sosgpu_profile_layer(self._h, float(tr), float(hr), float(ta), float(zmin), float(zmax),
                                                   float(a_tronc), float(piz), float(piztr), float(zout), lp, _ptr(prof), _ptr(nt),
                                                   _ptr(iborm), _ptr(zprof), _ptr(jout), _ptr(zz), _ptr(scal),
                                                   _ptr(bins.get("hvrai")), self._stream()), "sosgpu_profile_layer")
        return bins

    def solve_band(self, bins, aik, seg=None, group=None, tdifmug=None, reduce=True):
        """The whole per-wavelength bin loop of SOS_PROC (SOS_PROC.F:3459-3594) for bins already on the device
        (upload_bins / make_profiles): fused SOS_OS of every bin, AIK-weighted SOS_AGGREGATE, and -- when
        torch.distributed is initialised with more than one rank -- the one all-reduce that joins the ranks' bin
        slices.  aik[nb]: this rank's normalised weights (in the order of `bins`; apply bins["perm"] first when the
        upload was cost-sorted).  A rank may hold no bin at all (nb = 0): it contributes the neutral element.
        reduce=False: this rank holds the whole band (a replica, not a shard) -- no collective.
        Raises SosBinError (the reference's IER = -1) on every rank when any bin of the band is malformed.
        Returns (rec[nseg][smax+1][3][W] device tensor, scalars dict of dist.finish_scalars)."""
        from . import dist as _dist
        out = self.solve(bins) if bins["nb"] else None
        rec, scal = self.aggregate(out, aik, seg=seg, scal=bins.get("scal"), tdifmug=tdifmug)
        if reduce:
            buf = _dist.all_reduce_partial(_dist.pack_partial(rec, scal), scal.shape[1], group=group)
            rec, scal = _dist.unpack_partial(buf, rec.shape)
        fin = _dist.finish_scalars(scal)
        if (fin["min_orders"] < 0).any():
            raise SosBinError("SOS_OS: %d band(s) hold a malformed bin (NT outside 1..CTE_OS_NT or IBORM out of range)"
                              % int((fin["min_orders"] < 0).sum()))
        return rec, fin

    def output_levels(self, bins, altitudes):
        """Output levels of K altitudes (1 <= K <= capi.MAX_OUTPUT_LEVELS, -1 = the standard output) for every bin: the level
        pair, weight and TAUOUT a single-altitude profile gives for each.  Bins of make_profiles: sosgpu_output_levels on the
        device; bins of upload_bins with zprof (the aerosol-layer profile): output_levels_host, TAUOUT from the uploaded H
        as run_sos computes it for one altitude (SOS.F:567-581).  Returns dict(nz, jout[K][nb], zz[K][nb], tauout[K][nb])
        of device tensors, the `levels` solve_levels takes (no tensors for an empty batch: a rank without bins).
        Bins that carry `hvrai` (make_profiles(true_depth=True), upload_bins(hvrai=...)) also get `tauvrai`[K][nb], the
        UNTRUNCATED optical depth down to each altitude: the same level pair and weight applied to hvrai
        (sosgpu_output_depths), i.e. the reference's linear interpolation between the two levels that bracket z."""
        alts = [float(z) for z in altitudes]
        nz, nb, d = len(alts), bins["nb"], self.device
        if not 1 <= nz <= capi.MAX_OUTPUT_LEVELS:
            raise ValueError("1 to %d output altitudes per solve" % capi.MAX_OUTPUT_LEVELS)
        if nb == 0:
            return dict(nz=nz, jout=None, zz=None, tauout=None)
        if isinstance(bins.get("zprof"), torch.Tensor):
            jout = torch.empty((nz, nb), dtype=torch.int32, device=d)
            zz = torch.empty((nz, nb), dtype=torch.float64, device=d)
            tauout = torch.empty((nz, nb), dtype=torch.float64, device=d)
            capi.check(capi.lib().sosgpu_output_levels(self._h, nb, bins["lp"], _ptr(bins["prof"]), _ptr(bins["zprof"]),
                                                       _ptr(bins["nt"]), nz, (C.c_double * nz)(*alts), _ptr(jout), _ptr(zz),
                                                       _ptr(tauout), self._stream()), "sosgpu_output_levels")
            levels = dict(nz=nz, jout=jout, zz=zz, tauout=tauout)
            if bins.get("hvrai") is not None:
                levels["tauvrai"] = torch.empty((nz, nb), dtype=torch.float64, device=d)
                capi.check(capi.lib().sosgpu_output_depths(d.index or 0, nb, bins["lp"], _ptr(bins["hvrai"]), bins["lp"],
                                                           _ptr(bins["zprof"]), _ptr(bins["nt"]), nz, (C.c_double * nz)(*alts),
                                                           _ptr(levels["tauvrai"]), self._stream()), "sosgpu_output_depths")
            return levels
        return host_output_levels(bins, alts)

    def solve_levels(self, bins, levels, out=None):
        """One solve for the K output levels of output_levels (sosgpu_os_solve_levels).  Returns dict(rec[K][nb][smax+1][3][W],
        norders, iglast, flux): rec[k] equals the rec of solve() with that altitude's jout / zz, bit for bit."""
        self._need_operators()
        nz, nb = levels["nz"], bins["nb"]
        if out is None:
            out = self.alloc_outputs(nb)
            out["rec"] = torch.zeros((nz, nb, self.smax + 1, 3, self.w), dtype=torch.float64, device=self.device)
        capi.check(capi.lib().sosgpu_os_solve_levels(self._h, nb, bins["lp"], _ptr(bins["nt"]), _ptr(bins["iborm"]),
                                                     _ptr(bins["prof"]), nz, _ptr(levels["jout"]), _ptr(levels["zz"]),
                                                     _ptr(out["rec"]), _ptr(out["norders"]), _ptr(out["iglast"]),
                                                     _ptr(out["flux"]), self._stream()), "sosgpu_os_solve_levels")
        return out

    def solve_band_levels(self, bins, levels, aik, tdifmug=None, reduce=True, group=None, absorption=None):
        """solve_band for K output altitudes: ONE solve (solve_levels), then every altitude's records aggregated with its
        own TAUOUT, and -- sharded over ranks -- one all-reduce covering the K record sets.  levels: output_levels of these
        bins (a rank without bins contributes K neutral elements).  Returns (rec[K][smax+1][3][W], finish_scalars dict with
        one entry per altitude); raises SosBinError as solve_band does.
        absorption: None, or a list that receives the device tensor [K][4] of level_absorption, queued behind the aggregates
        (a band that is whole on this rank: the per-bin products do not pass through the all-reduce)."""
        from . import dist as _dist
        out = self.solve_levels(bins, levels) if bins["nb"] else None
        rec, scal = self.aggregate_levels(out, levels, aik, scal=bins.get("scal"), tdifmug=tdifmug)
        if absorption is not None:
            absorption.append(self.level_absorption(bins, levels, out, aik)[:, 0])
        rec, scal = rec[:, 0], scal[:, 0]                   # one segment: the band
        if reduce:
            buf = _dist.all_reduce_partial(_dist.pack_partial(rec, scal), scal.shape[1], group=group)
            rec, scal = _dist.unpack_partial(buf, rec.shape)
        fin = _dist.finish_scalars(scal)
        if (fin["min_orders"] < 0).any():
            raise SosBinError("SOS_OS: a bin of the band is malformed (NT outside 1..CTE_OS_NT, IBORM or an output level out "
                              "of range)")
        return rec, fin

    def diffuse_transmissions(self, bins):
        """Diffuse transmissions of the `-SOS.Trans` option (SOS.F:600-635): for the solar direction and for every
        direction J as incidence, SOS_OS restricted to Fourier order 0 over a black, non-reflecting ground
        (RHO = 0, IMAT_SURF = IFRESNEL = 0, IBORM = 0, ZOUT = -1); its EMOINS is TDIFMUS (N0 = solar index) resp.
        TDIFMUG(J) (N0 = J).  One order-0 context per incidence direction (they differ in the single-scattering
        vectors only), all bins per launch.  Returns (tdifmus[nb], tdifmug[nb][N]) as device tensors; values are for
        the equivalent (truncated) atmosphere, as SOS_OS delivers them."""
        nb = bins["nb"]
        zeros = torch.zeros(nb, dtype=torch.int32, device=self.device)
        sub = dict(bins, iborm=zeros, jout=None, zz=None)
        tdifmug = torch.empty((nb, self.n), dtype=torch.float64, device=self.device)
        tdifmus = None
        for j in range(1, self.n + 1):
            cx = SosContext(self.mu, self.ga, j, *self._coefs, iborm_max=0, ro=0.0, imat_surf=0, ifresnel=0,
                            device=self.device, **self._opts)
            try:
                out = cx.solve(sub)
                tdifmug[:, j - 1] = out["flux"][:, 0]
                if j == self.n0:
                    tdifmus = out["flux"][:, 0].clone()
                torch.cuda.synchronize(self.device)
            finally:
                cx.close()
        return tdifmus, tdifmug

    def alloc_outputs(self, nb, zero=True):
        """Output buffers of solve().  zero=True: rec is zero-initialised (the kernel only writes the orders a bin runs,
        sosgpu.h); zero=False: plain allocations -- for callers that read the records through norders only (aggregate does),
        it saves four fill kernels per call (they matter when many small launches share the GPU, solve_many)."""
        d = self.device
        mk = torch.zeros if zero else torch.empty
        return dict(rec=mk((nb, self.smax + 1, 3, self.w), dtype=torch.float64, device=d),
                    norders=mk(nb, dtype=torch.int32, device=d),
                    iglast=mk((nb, self.smax + 1), dtype=torch.int32, device=d),
                    flux=mk((nb, 2), dtype=torch.float64, device=d))

    def solve(self, bins, out=None):
        """Run the fused SOS_OS kernel on a batch of bins already resident in HBM (upload_bins)."""
        self._need_operators()
        if out is None:
            out = self.alloc_outputs(bins["nb"])
        capi.check(capi.lib().sosgpu_os_solve(self._h, bins["nb"], bins["lp"], _ptr(bins["nt"]), _ptr(bins["iborm"]),
                                              _ptr(bins["prof"]), _ptr(bins["jout"]), _ptr(bins["zz"]),
                                              _ptr(out["rec"]), _ptr(out["norders"]), _ptr(out["iglast"]),
                                              _ptr(out["flux"]), self._stream()), "sosgpu_os_solve")
        return out

    def last_solve_ms(self):
        ms = C.c_float(0)
        capi.check(capi.lib().sosgpu_last_solve_ms(self._h, C.byref(ms)), "sosgpu_last_solve_ms")
        return ms.value

    def solve_flops(self, bins, out):
        """(reference-algorithm flops, flops of the parity / rank-4 form executed) of the last solve; see
        sosgpu_os_flops in include/sosgpu.h."""
        fl = (C.c_double * 2)(0.0, 0.0)
        torch.cuda.synchronize(self.device)
        capi.check(capi.lib().sosgpu_os_flops(self._h, bins["nb"], _ptr(bins["nt"]), _ptr(out["norders"]),
                                              _ptr(out["iglast"]), fl), "sosgpu_os_flops")
        return fl[0], fl[1]

    def aggregate(self, out, aik, seg=None, scal=None, tdifmug=None):
        """SOS_AGGREGATE over segments of bins (default: all bins = one wavelength).  out = None or an empty batch
        gives the neutral element (a rank without bins).  tdifmug: optional per-bin [nb][N] diffuse transmissions.
        Returns (rec[nseg][smax+1][3][W], scal[nseg][10+N]) on device; see include/sosgpu.h for scal."""
        nb = 0 if out is None else out["rec"].shape[0]
        d = self.device
        sw = capi.SCAL_BASE + self.n
        if nb == 0:
            o_rec = torch.empty((1, self.smax + 1, 3, self.w), dtype=torch.float64, device=d)
            o_scal = torch.empty((1, sw), dtype=torch.float64, device=d)
            capi.check(capi.lib().sosgpu_aggregate(self._h, 0, 1, None, None, None, None, None, None, None,
                                                   _ptr(o_rec), _ptr(o_scal), self._stream()), "sosgpu_aggregate")
            return o_rec, o_scal
        if seg is None:
            # the default segment table [0, nb] is kept on the device: a host-to-device copy here would block the host until the
            # solve queued before it on this stream has finished, and with it every overlap of wavelengths on other streams
            cache = self.__dict__.setdefault("_seg_cache", {})
            seg_t = cache.get(nb)
            if seg_t is None:
                seg_t = cache[nb] = _dev_i32(np.array([0, nb], dtype=np.int32), d)
        else:
            seg_t = _dev_i32(seg, d)
        nseg = seg_t.numel() - 1
        aik_t = _dev_f64(aik, d)
        scal_t = torch.zeros((nb, 4), dtype=torch.float64, device=d) if scal is None else _dev_f64(scal, d)
        tdg = None if tdifmug is None else _dev_f64(tdifmug, d)
        if tdg is not None and tuple(tdg.shape) != (nb, self.n):
            raise ValueError("tdifmug must be [nb][N]")
        o_rec = torch.empty((nseg, self.smax + 1, 3, self.w), dtype=torch.float64, device=d)
        o_scal = torch.empty((nseg, sw), dtype=torch.float64, device=d)
        capi.check(capi.lib().sosgpu_aggregate(self._h, nb, nseg, _ptr(seg_t), _ptr(aik_t), _ptr(out["rec"]),
                                               _ptr(out["norders"]), _ptr(out["flux"]), _ptr(scal_t), _ptr(tdg),
                                               _ptr(o_rec), _ptr(o_scal), self._stream()), "sosgpu_aggregate")
        return o_rec, o_scal

    def aggregate_levels(self, out, levels, aik, seg=None, scal=None, tdifmug=None):
        """aggregate for the K output slots of solve_levels / solve_spectrum_levels: slot k's records out["rec"][k] with that
        altitude's TAUOUT (levels["tauout"][k]) in column 3 of a copy of the per-bin scalars `scal` (zeros when there are
        none); out = None gives the neutral element K times (a rank without bins).  Returns (rec[K][nseg][smax+1][3][W],
        scal[K][nseg][10+N]) on device; no synchronisation.
        levels with `tauvrai` (output_levels of bins that carry hvrai): one more launch behind the K aggregates
        (sosgpu_level_transmission) puts sum aik exp(-tauvrai[k]) of every slot and segment into element 9 of its scalar
        block, where it rides the all-reduce and the download of its neighbours (dist.finish_scalars: tauvrai_out)."""
        true_depth = out is not None and levels.get("tauvrai") is not None
        if out is None:
            parts = [self.aggregate(None, aik) for _ in range(levels["nz"])]
        else:
            nb, d = out["rec"].shape[1], self.device
            if true_depth:                                  # (the launch below takes the tensors the aggregates take)
                aik = _dev_f64(aik, d)
                seg = None if seg is None else _dev_i32(seg, d)
            base = None if scal is None else _dev_f64(scal, d)
            parts = []
            for k in range(levels["nz"]):
                sc = torch.zeros((nb, 4), dtype=torch.float64, device=d) if base is None else base.clone()
                sc[:, 3] = levels["tauout"][k]
                parts.append(self.aggregate(dict(rec=out["rec"][k], norders=out["norders"], flux=out["flux"]), aik, seg=seg,
                                            scal=sc, tdifmug=tdifmug))
        o_rec, o_scal = torch.stack([r for r, _ in parts]), torch.stack([s for _, s in parts])
        if true_depth:
            seg_t = self._seg_cache[nb] if seg is None else seg
            nz, nseg, sw = o_scal.shape
            capi.check(capi.lib().sosgpu_level_transmission(d.index or 0, nb, nseg, _ptr(seg_t), _ptr(aik), _ptr(out["norders"]),
                                                            nz, _ptr(levels["tauvrai"]), _ptr(o_scal), nseg * sw, sw,
                                                            self._stream()), "sosgpu_level_transmission")
        return o_rec, o_scal

    def trphi(self, rec, nf, tau, tauout, phis_rad, igli=0, wind=0.0, land=None):
        """SOS_TRPHI + SOS_POLAR for a list of azimuths (radians).  rec: device tensor [>=nf][3][W]
        (aggregated records).  Returns a device tensor [nphi][7][W]: XIT, XQT, XUT, ANGDIFF, polarisation
        angle, polarisation rate, polarised radiance."""
        d = self.device
        phis = _const_dev_f64(np.atleast_1d(np.asarray(phis_rad, dtype=np.float64)), d)
        rec = rec.to(device=d, dtype=torch.float64).contiguous()
        out = torch.empty((phis.numel(), 7, self.w), dtype=torch.float64, device=d)
        lp = None if land is None else C.byref(land)          # capi.Land: direct term of the land model (-SURF.Type 3..7)
        capi.check(capi.lib().sosgpu_trphi(self._h, int(nf), _ptr(rec), float(tau), float(tauout), phis.numel(),
                                           _ptr(phis), int(igli), float(wind), lp, _ptr(out), self._stream()), "sosgpu_trphi")
        return out

    def level_flux(self, rec):
        """Diffuse fluxes at the output altitude of an aggregated record (sosgpu_level_flux): rec is a device tensor
        [>=1][3][W] (one output slot of aggregate / aggregate_levels); only its order-0 intensity row is read.  Returns a device
        tensor [2]: E-(z), E+(z) (for the standard output: E- at the ground, E+ at the top of the atmosphere).  Nothing is
        waited for."""
        row = _flux_row(rec, self.device, self.w)
        out = torch.empty(2, dtype=torch.float64, device=self.device)
        capi.check(capi.lib().sosgpu_level_flux(self._h, _ptr(row), _ptr(out), self._stream()), "sosgpu_level_flux")
        return out

    def level_absorption(self, bins, levels, out, aik, seg=None):
        """Actinic flux and absorbed power per km of a band at the K output slots of solve_levels (sosgpu_level_absorption, one
        launch behind the solve): bins / levels as solve_levels took them, out its result (the per-bin records and norders),
        aik[nb] and seg as aggregate takes them.  The level altitudes are bins["zprof"] (make_profiles), or the zprof_host of
        upload_bins (the aerosol-layer profile), uploaded here.  Returns a device tensor [K][nseg][4]: the aik-weighted sums of
        a_dir, a_dn, a_up (the direct, down-going and up-going parts of the actinic flux) and q (absorbed power per km), all in
        the unit of the flux columns; zeros in a standard-output slot (altitude -1).  Nothing is waited for."""
        return _level_absorption(self, None, None, bins, levels, out, aik, seg)

    def level_irradiance(self, bins, levels, out, aik, seg=None):
        """Every irradiance quantity of a band at the K output slots of solve_levels (sosgpu_level_irradiance, ONE launch behind
        the solve, no aggregate): bins / levels as solve_levels took them (bins["scal"]: the per-bin scalars, zeros when there
        are none; levels["tauvrai"], where the bins carry hvrai, fills the last column), out its result (the per-bin records,
        norders and flux pairs), aik[nb] and seg as aggregate takes them.  Only the order-0 row of every record is read: the
        context may have been created with iborm_max = 0.  Returns a device tensor [K][nseg][capi.IRRADIANCE_COLS], columns as
        include/sosgpu.h lists them: level_absorption's four, sum aik {E-, E+}, the band scalars of aggregate's block and
        of sosgpu_level_transmission.  Nothing is waited for."""
        return _level_irradiance(self, None, None, bins, levels, out, aik, seg)

    def close(self):
        h = getattr(self, "_handle", None)                 # (a pending context has no handle: nothing to do)
        if h is not None and h.value:
            capi.lib().sosgpu_destroy(h)                  # waits for the streams this context's work was queued on
            self._handle = C.c_void_p()
            self._rsurf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trphi_many(items):
    """SosContext.trphi for many jobs in ONE sosgpu_trphi_spectrum call (one launch) on the current stream.  items: a list of
    (ctx, rec, nf, tau, tauout, phis_rad, igli, wind, land), each as SosContext.trphi takes them; the contexts live on one device.
    Returns (flat, views): one flat device tensor holding the results back to back and its per-item views [nphi][7][W] -- the
    bits SosContext.trphi gives for each item.  Every distinct azimuth list is uploaded once (and kept, _const_dev_f64).
    Nothing is waited for."""
    if not items:
        return None, []
    L = capi.lib()
    d = items[0][0].device
    lists, offs, total = {}, [], 0                  # distinct azimuth lists -> offset in the call's azimuth array
    for it in items:
        a = np.atleast_1d(np.asarray(it[5], dtype=np.float64))
        key = a.tobytes()
        if key not in lists:
            lists[key] = (total, a)
            total += a.size
        offs.append((lists[key][0], a.size))
    if len(lists) == 1:
        phis = _const_dev_f64(next(iter(lists.values()))[1], d)
    else:
        phis = torch.cat([_const_dev_f64(a, d) for _, a in lists.values()])
    n = len(items)
    jobs = (capi.TrphiJob * n)()
    recs, shapes, count = [], [], 0
    for j, ((cx, rec, nf, tau, tauout, _, igli, wind, land), (off, nphi)) in zip(jobs, zip(items, offs)):
        rec = rec.to(device=d, dtype=torch.float64).contiguous()
        recs.append(rec)
        j.cx, j.d_rec, j.nf, j.igli, j.phi_off, j.nphi = cx._h.value, rec.data_ptr(), int(nf), int(igli), off, nphi
        j.tau, j.tauout, j.wind = float(tau), float(tauout), float(wind)
        if land is not None:
            j.land = C.pointer(land)
        shapes.append((nphi, 7, cx.w))
        count += nphi * 7 * cx.w
    flat = torch.empty(count, dtype=torch.float64, device=d)
    need = int(L.sosgpu_trphi_spectrum_work_bytes(n))
    work = _work_area(need, d)
    capi.check(L.sosgpu_trphi_spectrum(jobs, n, _ptr(phis), int(phis.numel()), _ptr(flat), _ptr(work), need,
                                       items[0][0]._stream()), "sosgpu_trphi_spectrum")
    return flat, _flat_blocks(flat, shapes)


def _flat_blocks(flat, shapes):
    """A flat array (numpy array or tensor) of blocks lying back to back, cut into one view per shape, in order."""
    blocks, pos = [], 0
    for shp in shapes:
        m = math.prod(shp)
        blocks.append(flat[pos:pos + m].reshape(shp))
        pos += m
    return blocks


def _flux_row(rec, device, w):
    """The order-0 intensity row rec[0][0][W] of a record tensor, contiguous on `device` (a view wherever the record allows)."""
    row = rec[0, 0]
    if row.shape != (w,):
        raise ValueError("a record is [orders][3][W] with W = %d, got %s" % (w, tuple(rec.shape)))
    return row.to(device=device, dtype=torch.float64).contiguous()


def level_flux_many(items):
    """SosContext.level_flux for many jobs in ONE sosgpu_level_flux_spectrum call (one launch) on the current stream.  items: a
    list of (ctx, rec), each as SosContext.level_flux takes them; the contexts live on one device; jobs may share a context or a
    record.  Returns a device tensor [njobs][2] (E-, E+ per job) -- the bits SosContext.level_flux gives for each item.  Nothing
    is waited for."""
    n = len(items)
    if n == 0:
        return None
    L = capi.lib()
    d = items[0][0].device
    jobs = (capi.FluxJob * n)()
    rows = []
    for j, (cx, rec) in zip(jobs, items):
        row = _flux_row(rec, d, cx.w)
        rows.append(row)
        j.cx, j.d_rec = cx._h.value, row.data_ptr()
    out = torch.empty((n, 2), dtype=torch.float64, device=d)
    need = int(L.sosgpu_level_flux_spectrum_work_bytes(n))
    work = _work_area(need, d)
    capi.check(L.sosgpu_level_flux_spectrum(jobs, n, _ptr(out), _ptr(work), need, items[0][0]._stream()),
               "sosgpu_level_flux_spectrum")
    return out


def channel_accumulate(flat, njobs, K, nphi, W, first, job, wgt, acc):
    """The terms of C sensor channels onto the accumulator of a spectrum, in ONE sosgpu_channel_accumulate call (one launch) on
    the current stream: acc[c][k][iphi][q][t] += sum_m wgt[m] * block(job[m], k)[iphi][q][t] for q = 0, 1, 2 over the terms
    m = first[c] .. first[c+1]-1, in term order, each step a = a + w * x (one multiply, one add).  flat: device tensor of
    njobs * K blocks [nphi][7][W] back to back (job j, slot k at (j K + k) nphi 7 W) -- what trphi_many returns for the jobs of a
    part of a levels pass; first [C+1], job and wgt [first[C]]: host arrays; acc: contiguous float64 device tensor
    [C][K][nphi][3][W], updated in place.  Nothing is waited for."""
    first = np.ascontiguousarray(first, dtype=np.int32)
    job = np.ascontiguousarray(job, dtype=np.int32)
    wgt = np.ascontiguousarray(wgt, dtype=np.float64)
    nchan = first.size - 1
    if nchan < 1 or job.shape != wgt.shape or job.ndim != 1 or job.size != int(first[-1]):
        raise ValueError("first is [C+1] with first[C] = len(job) = len(wgt)")
    if flat.dtype != torch.float64 or not flat.is_contiguous() or flat.numel() < njobs * K * nphi * 7 * W:
        raise ValueError("flat holds njobs * K contiguous float64 blocks [nphi][7][W]")
    if acc.dtype != torch.float64 or not acc.is_contiguous() or acc.device != flat.device or acc.numel() != nchan * K * nphi * 3 * W:
        raise ValueError("acc is a contiguous float64 tensor [C][K][nphi][3][W] on the device of the blocks")
    L = capi.lib()
    d = flat.device
    need = int(L.sosgpu_channel_accumulate_work_bytes(nchan, job.size))
    work = _work_area(need, d)
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(L.sosgpu_channel_accumulate(d.index or 0, _ptr(flat), int(njobs), int(K), int(nphi), int(W), nchan, ip(first),
                                           ip(job), ip(wgt), _ptr(acc), _ptr(work), need,
                                           C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "sosgpu_channel_accumulate")
    return acc


def channel_finish(acc, angdiff_block):
    """The channel radiances from the accumulator of channel_accumulate, in ONE sosgpu_channel_finish call (one launch) on the
    current stream: acc [C][K][nphi][3][W] -> a new device tensor [C][K][nphi][7][W] in SosContext.trphi's row order (the sums
    behind the reference's output thresholds, ANGDIFF from angdiff_block -- any block [nphi][7][W] of the spectrum --, SOS_POLAR
    of the sums, direction 0 zero).  Nothing is waited for."""
    if acc.dim() != 5 or acc.shape[3] != 3 or acc.dtype != torch.float64 or not acc.is_contiguous():
        raise ValueError("acc is a contiguous float64 tensor [C][K][nphi][3][W]")
    nchan, K, nphi, _, W = acc.shape
    d = acc.device
    blk = angdiff_block.to(device=d, dtype=torch.float64).contiguous()
    if blk.numel() != nphi * 7 * W:
        raise ValueError("angdiff_block is one block [nphi][7][W] of the spectrum")
    out = torch.empty((nchan, K, nphi, 7, W), dtype=torch.float64, device=d)
    capi.check(capi.lib().sosgpu_channel_finish(d.index or 0, _ptr(acc), _ptr(blk), nchan, K, nphi, W, _ptr(out),
                                                C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "sosgpu_channel_finish")
    return out


def create_contexts(ctxs):
    """The library contexts of the objects made with create=False, in ONE sosgpu_create_spectrum call on the current stream:
    one staged copy of all their small tables and one launch; the same contexts, bit for bit, sosgpu_create makes.  The
    objects live on one device and may differ in every size.  One that has its handle already is an error (ValueError, before
    the call); an empty list does nothing.  Nothing is waited for: the tables are in place once the current stream has passed
    the call, so work that reads them on another stream must be ordered behind it.  Returns the number of contexts made."""
    ctxs = list(ctxs)
    for cx in ctxs:
        if cx._pending is None:
            raise ValueError("create_contexts: a context of the list has its handle already (or was closed)")
        if cx.device != ctxs[0].device:
            raise ValueError("create_contexts: the contexts must live on one device")
    if len({id(cx) for cx in ctxs}) != len(ctxs):
        raise ValueError("create_contexts: a context appears twice in the list")
    if not ctxs:
        return 0
    L = capi.lib()
    n = len(ctxs)
    first = ctxs[0]
    specs =(capi.CtxSpec * n)(*[cx._pending for cx in ctxs])
    need = int(L.sosgpu_create_spectrum_work_bytes(specs, n))
    work = _work_area(need, first.device)
    hs = (C.c_void_p * n)()
    capi.check(L.sosgpu_create_spectrum(hs, first.device.index or 0, specs, n, _ptr(work), need, first._stream()),
               "sosgpu_create_spectrum")
    for cx, h in zip(ctxs, hs):
        cx._handle = C.c_void_p(h)
        cx._pending = None
    return n


def build_operators(ctxs):
    """The operator tables of the contexts created with build=False, in ONE sosgpu_noyaux_spectrum call on the current stream:
    at most five launches for all of them (the table forms of the kernels of sosgpu_set_surface_matrices_async and
    sosgpu_noyaux; the same bits).  The contexts live on one device and may differ in every size; their surface matrices must
    be complete on, or ordered before, the current stream.  Contexts that are built already are left alone.  Nothing is
    waited for."""
    todo = [cx for cx in ctxs if not cx._built]
    if not todo:
        return 0
    L = capi.lib()
    n = len(todo)
    first = todo[0]
    need = int(L.sosgpu_noyaux_spectrum_work_bytes(n))
    work = _work_area(need, first.device)
    hs = (C.c_void_p * n)(*[cx._h for cx in todo])
    rs = None
    if any(cx._rsurf is not None for cx in todo):
        rs = (C.c_void_p * n)(*[None if cx._rsurf is None else cx._rsurf.data_ptr() for cx in todo])
    capi.check(L.sosgpu_noyaux_spectrum(hs, n, rs, _ptr(work), need, first._stream()), "sosgpu_noyaux_spectrum")
    for cx in todo:
        cx._built = True
    return n


def _many_contexts(fn, ctxs, bins, ctx_of_bin):
    """The common opening of diffuse_transmissions_many and spherical_albedo_many (`fn`, named by the errors): the context list
    with its operators asked for, the ctx_of_bin rule and the handle array.  Returns (ctxs, first, device, N, nb, ctx_of_bin on
    the device or None, the library, the handles)."""
    ctxs = list(ctxs)
    if not ctxs:
        raise ValueError("%s needs at least one context" % fn)
    for cx in ctxs:
        cx._need_operators()
    first = ctxs[0]
    d, n, nb = first.device, first.n, int(bins["nb"])
    if ctx_of_bin is None and len(ctxs) > 1:
        raise ValueError("ctx_of_bin is required with more than one context")
    cob = None if ctx_of_bin is None else _dev_i32(ctx_of_bin, d)
    return ctxs, first, d, n, nb, cob, capi.lib(), (C.c_void_p * len(ctxs))(*[cx._h for cx in ctxs])


def diffuse_transmissions_many(ctxs, bins, ctx_of_bin=None):
    """SosContext.diffuse_transmissions for the bins of MANY contexts in one call (sosgpu_trans_spectrum): every (bin,
    direction) pair is an item of ONE order-0 solve, every (context, direction) pair an entry of a device table that shares
    the context's order-0 operators -- no context per direction, nothing waited for.  ctxs: built contexts of one device that
    agree in N (OS_NB, polarisation, surface may differ); bins: their concatenated bins (concat_bins, or the bins of the one
    context); ctx_of_bin[nb]: int32 index into ctxs of every bin (None with one context).  Returns (tdifmus[nb],
    tdifmug[nb][N]) device tensors with the bits of the per-direction loop; tdifmus[b] is column n0 - 1 of the bin's context.
    The work area comes from torch's allocator and is dropped at return (the allocator keeps it for the stream)."""
    ctxs, first, d, n, nb, cob, L, hs = _many_contexts("diffuse_transmissions_many", ctxs, bins, ctx_of_bin)
    tdifmug = torch.empty((nb, n), dtype=torch.float64, device=d)
    need = int(L.sosgpu_trans_spectrum_work_bytes(hs, len(ctxs), nb, bins["lp"]))
    work = _work_area(need, d)
    capi.check(L.sosgpu_trans_spectrum(hs, len(ctxs), _ptr(cob), nb, bins["lp"], _ptr(bins["nt"]), _ptr(bins["prof"]),
                                       _ptr(tdifmug), _ptr(work), need, first._stream()), "sosgpu_trans_spectrum")
    if len({cx.n0 for cx in ctxs}) == 1:
        return tdifmug[:, first.n0 - 1].clone(), tdifmug
    n0 = _dev_i32(np.array([cx.n0 - 1 for cx in ctxs], dtype=np.int32), d).long()
    return tdifmug.gather(1, n0[cob.long()][:, None])[:, 0].contiguous(), tdifmug


def spherical_albedo_many(ctxs, bins, ctx_of_bin=None, from_below=True):
    """The spherical albedo of the atmosphere for the bins of MANY contexts in one call (sosgpu_albedo_spectrum): per bin
    S = 2 sum_j ga_j mu_j A_j, with A_j the up-going flux of an order-0 solve over a black ground with incidence mu_j -- the
    items, child table and solve of diffuse_transmissions_many, which keeps the other flux.  from_below=True lights the
    atmosphere from the ground (every item's profile mirrored in the vertical about its own NT): the S of
    rho_toa = rho_path + T_down T_up rho_s / (1 - S rho_s), for which the ground flux over a Lambert ground of albedo a obeys
    E_down(a) (1 - a S) = E_down(0).  from_below=False: the spherical albedo seen from space over a black ground (the
    planetary quantity).  S belongs to the truncated, equivalent atmosphere the solver sees, as tdifmug does.
    ctxs, bins, ctx_of_bin: as diffuse_transmissions_many takes them.  Returns (salb[nb], plane[nb][N]) device tensors;
    plane[b][j] is the plane albedo A_j, 0 in the columns of weight-0 directions (the inserted solar angle, user angles), which
    are not solved; a malformed bin gives zeros.  Nothing is waited for."""
    ctxs, first, d, n, nb, cob, L, hs = _many_contexts("spherical_albedo_many", ctxs, bins, ctx_of_bin)
    salb = torch.empty(nb, dtype=torch.float64, device=d)
    plane = torch.empty((nb, n), dtype=torch.float64, device=d)
    need = int(L.sosgpu_albedo_spectrum_work_bytes(hs, len(ctxs), nb, bins["lp"]))
    work = _work_area(need, d)
    capi.check(L.sosgpu_albedo_spectrum(hs, len(ctxs), _ptr(cob), nb, bins["lp"], _ptr(bins["nt"]), _ptr(bins["prof"]),
                                        1 if from_below else 0, _ptr(plane), _ptr(salb), _ptr(work), need, first._stream()),
               "sosgpu_albedo_spectrum")
    return salb, plane


def albedo_band(seg, aik, salb):
    """sum aik * salb over the bins of every segment (sosgpu_albedo_band): seg int32 [nseg + 1] (host or device), aik and salb
    [nb] device tensors.  Returns the device tensor [nseg]; one launch on the current stream, nothing waited for."""
    d = salb.device
    seg_t = _dev_i32(seg, d)
    nseg = int(seg_t.numel()) - 1
    out = torch.empty(max(nseg, 0), dtype=torch.float64, device=d)
    if nseg < 1:
        return out
    capi.check(capi.lib().sosgpu_albedo_band(nseg, _ptr(seg_t), _ptr(aik), _ptr(salb), _ptr(out), d.index or 0,
                                             C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "sosgpu_albedo_band")
    return out


def level_altitudes(bins, lp=None):
    """The level altitudes of a bin dict as the device tensor [nb][lp] sosgpu_level_absorption takes: bins["zprof"]
    (make_profiles) as it is, or the zprof_host of upload_bins (the aerosol-layer profile), uploaded with zeros past its levels;
    lp: a larger level capacity to pad to (concat_bins).  ValueError for bins without altitudes."""
    d = bins["prof"].device
    lp = bins["lp"] if lp is None else lp
    z = bins.get("zprof")
    if not isinstance(z, torch.Tensor):
        zh = bins.get("zprof_host")
        if zh is None:
            raise ValueError("the absorbed power needs the bins' level altitudes (make_profiles, or upload_bins with zprof)")
        zp = np.zeros((bins["nb"], lp))
        zp[:, :zh.shape[1]] = zh
        return _dev_f64(zp, d)
    z = z.to(device=d, dtype=torch.float64)
    if z.shape[1] < lp:
        z = torch.nn.functional.pad(z, (0, lp - z.shape[1]))
    return z.contiguous()


def _level_absorption(cx, table, ctx_of_bin, bins, levels, out, aik, seg):
    """The one caller of sosgpu_level_absorption: SosContext.level_absorption (table None) and level_absorption_spectrum."""
    d = cx.device
    nz, nb = levels["nz"], bins["nb"]
    if seg is None:
        seg = np.array([0, nb], dtype=np.int32)
    seg_t = _dev_i32(seg, d)
    nseg = int(seg_t.numel()) - 1
    res = torch.zeros((nz, max(nseg, 0), 4), dtype=torch.float64, device=d)
    if nb == 0 or nseg < 1:
        return res
    zprof = level_altitudes(bins)
    aik_t = _dev_f64(aik, d)
    lv = [levels[k].contiguous() for k in ("jout", "zz", "tauout")]     # (views of a part's block: [K][nb] of their own here)
    if tuple(zprof.shape) != (nb, bins["lp"]) or aik_t.numel() != nb or tuple(out["rec"].shape[:2]) != (nz, nb):
        raise ValueError("level_absorption: zprof [nb][lp], aik [nb] and the records [K][nb] of solve_levels are needed")
    capi.check(capi.lib().sosgpu_level_absorption(cx._h, None if table is None else _ptr(table.table), _ptr(ctx_of_bin), nb,
                                                  bins["lp"], _ptr(bins["nt"]), _ptr(bins["prof"]), _ptr(zprof), nz,
                                                  _ptr(lv[0]), _ptr(lv[1]), _ptr(lv[2]), _ptr(out["rec"]), _ptr(out["norders"]),
                                                  nseg, _ptr(seg_t), _ptr(aik_t), _ptr(res), cx._stream()),
               "sosgpu_level_absorption")
    return res


def level_absorption_spectrum(table, bins, ctx_of_bin, seg, aik, levels, out):
    """SosContext.level_absorption for the bins of many wavelengths in ONE launch, behind solve_spectrum_levels: table, bins,
    ctx_of_bin, seg, aik and levels as that call took them (bins with the level altitudes `zprof` [nb][lp]: concat_bins does
    not carry them, see level_altitudes), out its per-bin result (rec [K][nb][smax+1][3][W], norders).  Bin b is read with mu,
    ga and n0 of table.ctxs[ctx_of_bin[b]].  Returns a device tensor [K][nwavelengths][4]; nothing is waited for."""
    return _level_absorption(table.ctxs[0], table, ctx_of_bin, bins, levels, out, aik, seg)


def _level_irradiance(cx, table, ctx_of_bin, bins, levels, out, aik, seg):
    """The one caller of sosgpu_level_irradiance: SosContext.level_irradiance (table None) and level_irradiance_spectrum."""
    d = cx.device
    nz, nb = levels["nz"], bins["nb"]
    if seg is None:
        seg = np.array([0, nb], dtype=np.int32)
    seg_t = _dev_i32(seg, d)
    nseg = int(seg_t.numel()) - 1
    res = torch.zeros((nz, max(nseg, 0), capi.IRRADIANCE_COLS), dtype=torch.float64, device=d)
    if nb == 0 or nseg < 1:
        return res
    zprof = level_altitudes(bins)
    aik_t = _dev_f64(aik, d)
    scal = torch.zeros((nb, 4), dtype=torch.float64, device=d) if bins.get("scal") is None else _dev_f64(bins["scal"], d)
    lv = [levels[k].contiguous() for k in ("jout", "zz", "tauout")]     # (views of a part's block: [K][nb] of their own here)
    tv = None if levels.get("tauvrai") is None else levels["tauvrai"].contiguous()
    if tuple(zprof.shape) != (nb, bins["lp"]) or aik_t.numel() != nb or tuple(out["rec"].shape[:2]) != (nz, nb) or \
            tuple(scal.shape) != (nb, 4) or tuple(out["flux"].shape) != (nb, 2):
        raise ValueError("level_irradiance: zprof [nb][lp], aik [nb], scal [nb][4] and the records [K][nb] and flux [nb][2] of "
                         "solve_levels are needed")
    capi.check(capi.lib().sosgpu_level_irradiance(cx._h, None if table is None else _ptr(table.table), _ptr(ctx_of_bin), nb,
                                                  bins["lp"], _ptr(bins["nt"]), _ptr(bins["prof"]), _ptr(zprof), nz,
                                                  _ptr(lv[0]), _ptr(lv[1]), _ptr(lv[2]), _ptr(out["rec"]), _ptr(out["norders"]),
                                                  _ptr(out["flux"]), _ptr(scal), _ptr(tv), nseg, _ptr(seg_t), _ptr(aik_t),
                                                  _ptr(res), cx._stream()), "sosgpu_level_irradiance")
    return res


def level_irradiance_spectrum(table, bins, ctx_of_bin, seg, aik, levels, out):
    """SosContext.level_irradiance for the bins of many wavelengths in ONE launch, behind the sosgpu_os_solve_multi_levels call
    of solve_spectrum_order0: table, bins (with `scal`, and the level altitudes `zprof` [nb][lp], see level_altitudes),
    ctx_of_bin, seg, aik and levels as that call took them, out its per-bin result.  Bin b is read with mu, ga and n0 of
    table.ctxs[ctx_of_bin[b]].  Returns a device tensor [K][nwavelengths][capi.IRRADIANCE_COLS]; nothing is waited for."""
    return _level_irradiance(table.ctxs[0], table, ctx_of_bin, bins, levels, out, aik, seg)


def solve_spectrum_order0(table, bins, ctx_of_bin, levels, out=None):
    """The solve alone of solve_spectrum_levels, for level_irradiance_spectrum: ONE sosgpu_os_solve_multi_levels launch over the
    bins of many wavelengths in the order given, no aggregate behind it.  The contexts of an irradiance pass hold the order-0
    operators alone (iborm_max = 0) and every bin has iborm = 0, so the records are [K][nb][1][3][W]; the Fourier orders do not
    couple, so their order-0 rows and the flux pairs are those of a solve of every order.  Returns the per-bin result dict
    (rec, norders, iglast, flux); no synchronisation."""
    cx = table.ctxs[0]
    nz, nb = levels["nz"], bins["nb"]
    if out is None:
        out = cx.alloc_outputs(nb, zero=False)
        out["rec"] = torch.empty((nz, nb, cx.smax + 1, 3, cx.w), dtype=torch.float64, device=cx.device)
    capi.check(capi.lib().sosgpu_os_solve_multi_levels(cx._h, _ptr(table.table), _ptr(ctx_of_bin), None, nb, bins["lp"],
                                                       _ptr(bins["nt"]), _ptr(bins["iborm"]), _ptr(bins["prof"]), nz,
                                                       _ptr(levels["jout"]), _ptr(levels["zz"]), _ptr(out["rec"]),
                                                       _ptr(out["norders"]), _ptr(out["iglast"]), _ptr(out["flux"]),
                                                       cx._stream()), "sosgpu_os_solve_multi_levels")
    return out


def release_scratch():
    """Return the scratch buffers the library keeps from destroyed contexts (streamed solver; at most 8 GiB) to the device,
    and free the pinned staging blocks of the table-form calls whose copies have passed (sosgpu_trim)."""
    capi.check(capi.lib().sosgpu_trim(), "sosgpu_trim")


class ContextTable:
    """Device-resident table of wavelength contexts (sosgpu_ctx_table) for solve_spectrum: ONE kernel launch then covers the
    bins of all these wavelengths.  The contexts must agree in N, iborm_max and IMAT_SURF; the table stays valid while they
    live (rebuild it after closing one or changing its surface matrices)."""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        if not self.ctxs:
            raise ValueError("ContextTable needs at least one context")
        self.device = self.ctxs[0].device
        for cx in self.ctxs:
            cx._need_operators()              # (the table copies the ground-operator pointers the build registers)
        L = capi.lib()
        n = len(self.ctxs)
        self.table = torch.empty(n * int(L.sosgpu_ctx_table_entry_bytes()), dtype=torch.uint8, device=self.device)
        hs = (C.c_void_p * n)(*[cx._h for cx in self.ctxs])
        capi.check(L.sosgpu_ctx_table(hs, n, _ptr(self.table), self.ctxs[0]._stream()), "sosgpu_ctx_table")


def concat_bins(bins_list):
    """Concatenate per-wavelength bin dicts (upload_bins / make_profiles) for solve_spectrum: the level axis is padded to the
    largest lp.  Returns (bins, ctx_of_bin int32 device tensor, seg int32 device tensor of len(bins_list) + 1)."""
    d = bins_list[0]["prof"].device
    lp = max(b["lp"] for b in bins_list)
    zo = [b["jout"] is not None for b in bins_list]
    if any(zo) != all(zo):
        raise ValueError("either every wavelength or none has an output level (zout)")
    prof = []
    for b in bins_list:
        p = b["prof"]
        if b["lp"] < lp:
            p = torch.nn.functional.pad(p, (0, lp - b["lp"]))
        prof.append(p)
    cat = lambda k: torch.cat([b[k] for b in bins_list])
    counts = [b["nb"] for b in bins_list]
    out = dict(nb=int(sum(counts)), lp=lp, perm=None, nt=cat("nt"), iborm=cat("iborm"), prof=torch.cat(prof).contiguous(),
               jout=cat("jout") if all(zo) else None, zz=cat("zz") if all(zo) else None)
    if all(b.get("scal") is not None for b in bins_list):
        out["scal"] = cat("scal")
    if all(b.get("hvrai") is not None for b in bins_list):
        out["hvrai"] = torch.cat([torch.nn.functional.pad(b["hvrai"], (0, lp - b["lp"])) if b["lp"] < lp else b["hvrai"]
                                  for b in bins_list]).contiguous()
    cob = _dev_i32(np.repeat(np.arange(len(bins_list), dtype=np.int32), counts), d)
    seg = _dev_i32(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), d)
    return out, cob, seg


def concat_profiles(bins_list):
    """The level profiles alone of per-wavelength bin dicts, concatenated as concat_bins does it (level axis padded to the
    largest lp) -- what diffuse_transmissions_many reads, whatever output levels the dicts carry.  Returns (dict(nb, lp, nt,
    prof), ctx_of_bin int32 device tensor); one dict is passed through as it is, with ctx_of_bin None."""
    if len(bins_list) == 1:
        return bins_list[0], None
    d = bins_list[0]["prof"].device
    lp = max(b["lp"] for b in bins_list)
    prof = [b["prof"] if b["lp"] == lp else torch.nn.functional.pad(b["prof"], (0, lp - b["lp"])) for b in bins_list]
    counts = [b["nb"] for b in bins_list]
    cob = _dev_i32(np.repeat(np.arange(len(bins_list), dtype=np.int32), counts), d)
    return dict(nb=int(sum(counts)), lp=lp, nt=torch.cat([b["nt"] for b in bins_list]), prof=torch.cat(prof).contiguous()), cob


def solve_spectrum(table, bins, ctx_of_bin, seg, aik, out=None, order="cost", tdifmug=None):
    """The bin loops of MANY wavelengths (one SOS_PROC call each in the reference, binding/run_sos.py:640) as ONE launch of the
    fused solver plus one segmented SOS_AGGREGATE: bin b runs with the operators of table.ctxs[ctx_of_bin[b]], segment g of
    `seg` is wavelength g.  bins / ctx_of_bin / seg from concat_bins; aik[nb] device tensor in the same order.
    tdifmug: optional per-bin [nb][N] diffuse transmissions (diffuse_transmissions_many), aggregated per segment.
    Returns (rec[nwavelengths][smax+1][3][W], scal[nwavelengths][10+N]) like SosContext.aggregate; no synchronisation."""
    cx = table.ctxs[0]
    if out is None:
        out = cx.alloc_outputs(bins["nb"], zero=False)
    # order="cost": the workgroups take the bins by decreasing total optical depth (levels x scattering orders go with it), so
    # that the long bins start first and the launch does not end on them; the bins stay where they are.  None: as given.
    # (Measured, scripts/spectrum_stream_bench.py / spectrum_bench.py: +4 % on real level grids, 160 x 25 bins; -5 % for the
    #  LDS-resident kernel at NT = 30, where neighbouring bins of one wavelength share their operators in L2 -- not applied there.)
    ord_t = _spectrum_order(cx, bins, order)
    capi.check(capi.lib().sosgpu_os_solve_multi(cx._h, _ptr(table.table), _ptr(ctx_of_bin), _ptr(ord_t), bins["nb"], bins["lp"],
                                                _ptr(bins["nt"]), _ptr(bins["iborm"]), _ptr(bins["prof"]),
                                                _ptr(bins["jout"]), _ptr(bins["zz"]), _ptr(out["rec"]), _ptr(out["norders"]),
                                                _ptr(out["iglast"]), _ptr(out["flux"]), cx._stream()), "sosgpu_os_solve_multi")
    return cx.aggregate(out, aik, seg=seg, scal=bins.get("scal"), tdifmug=tdifmug)


CKD_WL_DTYPE = np.dtype(capi.CkdWl)          # sosgpu_ckd_wl as a numpy record


def pack_ckd_requests(preps, table_ptr, xk_off=None, base=0):
    """Host side of ckd_layer_tables (pure numpy): the per-wavelength table, the slot pointers and the packed axes / layer
    states of a list of absorption.prepa_absprofile dicts.
      table_ptr(prep, gas)  device address (int) of the interval's coefficient block of that gas, [5][NP][NT] (H2O
                            [5][NC][NP][NT]) doubles -- absorption.ckd_device_tables on a GPU, anything in a test
      xk_off                where each wavelength's xk[8][5][nlay] starts in the output block, in doubles (default: one after
                            the other);  base: where `axes` will start in the device buffer it is uploaded into, in doubles
    Returns a dict: wl (structured array [nwl], CKD_WL_DTYPE = sosgpu_ckd_wl), slots (uint64 [nwl * 40]: slot gas * 5 + term of
    each wavelength, 0 = NULL for a term >= NEXP of the gas and for a table that is all zero), axes (float64: every distinct
    axis and layer state once -- a spectrum shares one atmosphere and a file's intervals share their axes), nlay, nterm,
    out_doubles (end of the last xk block)."""
    from . import absorption as _abs
    nterm, nlay = _abs.CKD_NAI_MAX, _abs.NLEVEL - 1
    wl = np.zeros(len(preps), dtype=CKD_WL_DTYPE)
    slots = np.zeros((len(preps), 8, nterm), dtype=np.uint64)
    parts, where, n = [], {}, 0

    def place(a):
        nonlocal n
        hit = where.get(id(a))
        if hit is None:
            hit = where[id(a)] = (n, a)                       # (the array is held: its id stays its own)
            parts.append(np.ascontiguousarray(a, dtype=np.float64).ravel())
            n += parts[-1].size
        return base + hit[0]

    states = {}
    out = 0
    for w, prep in enumerate(preps):
        e = wl[w]
        e["nterm"], e["nt"], e["np"], e["nc"] = nterm, len(prep["tab_temp"]), len(prep["tab_pres"]), len(prep["tab_conc"])
        e["pres_off"], e["temp_off"], e["conc_off"] = place(prep["tab_pres"]), place(prep["tab_temp"]), place(prep["tab_conc"])
        st = states.get(id(prep["userprofil"]))
        if st is None:
            st = states[id(prep["userprofil"])] = (prep["userprofil"],) + tuple(_abs.layer_state(prep))
        e["prs_off"], e["tmp_off"], e["cl_off"] = place(st[1]), place(st[2]), place(st[3])
        e["xk_off"] = out if xk_off is None else int(xk_off[w])
        out = max(out, int(e["xk_off"]) + 8 * nterm * nlay)
        absorbing = _abs.ckd_absorbing(prep)
        for k in range(8):
            if absorbing[k].any():
                block = int(table_ptr(prep, k))
                per = prep["ki"][k][0].size * 8                # bytes of one term's table
                for term in np.flatnonzero(absorbing[k]):
                    slots[w, k, term] = block + int(term) * per
    axes = np.concatenate(parts) if parts else np.zeros(0)
    return dict(wl=wl, slots=slots.reshape(-1), axes=axes, nlay=nlay, nterm=nterm, out_doubles=out)


def _ckd_launch(L, dev, pk, axes_t, axes_doubles, out_t, out_doubles, st, where):
    """Queue sosgpu_ckd_layer_tables for the packed requests pk on stream handle st; returns (status tensor, work area)."""
    nwl, nslots = len(pk["wl"]), int(pk["slots"].size)
    need = int(L.sosgpu_ckd_layer_tables_work_bytes(nwl, nslots))
    work = _work_area(need, dev)
    status = torch.empty(nwl, dtype=torch.int32, device=dev)
    bad = C.c_int(-1)
    rc = L.sosgpu_ckd_layer_tables(dev.index or 0, nwl, pk["wl"].ctypes.data_as(C.c_void_p), nslots,
                                   pk["slots"].ctypes.data_as(C.c_void_p), _ptr(axes_t), axes_doubles, pk["nlay"], _ptr(work),
                                   need, _ptr(out_t), out_doubles, _ptr(status), C.byref(bad), st)
    if rc != 0 and bad.value >= 0 and where is not None:
        where["bad"] = int(bad.value)
    capi.check(rc, "sosgpu_ckd_layer_tables")
    return status, work


def ckd_layer_tables(preps, device=0, stream=None):
    """COEFF_ABS_CKD of many wavelengths in ONE launch on device-resident coefficient tables (sosgpu_ckd_layer_tables): what
    absorption.layer_tables computes for each prep (absorption.prepa_absprofile), bit for bit, without the host interpolation
    and without an upload of the tables.  One upload (axes and layer states), queued on `stream` (a torch stream; None: the
    current one), nothing waited for.  Returns (xk, ro, status): xk[g] device tensors [8][5][49] (views of one block), ro[g]
    host arrays [8][49] as layer_tables returns them, status an int32 device tensor [len(preps)] -- 0 ok, else the key of
    absorption.CKD_STATUS_MESSAGES for the error the host routine raises for that wavelength (its xk is then not usable)."""
    from . import absorption as _abs
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    tables = {}
    pk = pack_ckd_requests(preps, _ckd_table_ptr(tables, dev))
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        axes = _upload(torch.from_numpy(pk["axes"]), dev)
        out = torch.empty(pk["out_doubles"], dtype=torch.float64, device=dev)
        status, work = _ckd_launch(capi.lib(), dev, pk, axes, pk["axes"].size, out, pk["out_doubles"], st, None)
    per = 8 * pk["nterm"] * pk["nlay"]
    xk = [out[int(o):int(o) + per].view(8, pk["nterm"], pk["nlay"]) for o in pk["wl"]["xk_off"]]
    status._keep = (axes, work, [t[2] for t in tables.values()])      # alive until the caller lets go of the result
    return xk, [_abs.layer_ro(p) for p in preps], status


PROFILE_WL_DTYPE = np.dtype(capi.ProfileWl)  # sosgpu_profile_wl as a numpy record


def pack_profile_requests(requests, table_ptr=None):
    """Host side of make_profiles_spectrum (pure numpy): the per-wavelength table, the packed gas buffer and the per-bin
    wavelength index of a list of profile requests.  A request is a dict with the arguments of SosContext.absorption_profiles
    and make_profiles of one wavelength -- ik[nb][8], xk[8][nterm][nlev-1], ro[8][nlev-1], altabs[nlev] (ik None: no gas,
    one bin), tr, hr, ta, ha, a_tronc, piz, piztr, zout, absprofil -- and `smax`, the highest Fourier order of its context.
    Returns a dict:
      wl          structured array [nwl] (PROFILE_WL_DTYPE = sosgpu_profile_wl); xk_off / ro_off / alt_off count doubles in buf
      buf         ONE float64 array for one upload: the gas tables of every wavelength (xk, ro, altabs, in request order), then
                  ik[nb][8] (int32, rows of no-gas bins zero) at ik_off, then wl_of_bin[nb] (int32) at wob_off
      gas_doubles, ik_off, wob_off   (in doubles);  nb, nblev (0 without any gas), seg[nwl + 1] (first bin of each request)
    A gas request may carry `prep` (absorption.prepa_absprofile's dict) in place of `xk`: its xk[8][5][nlev-1] is then made on
    the device (sosgpu_ckd_layer_tables, queued ahead of the profile kernels) in a block BEHIND buf -- the device buffer is
    buf.size + device_doubles long and the request's xk_off points there.  The dict then also holds `ckd`, the
    pack_ckd_requests of these requests (its axes appended to buf, its xk_off those of wl), and `ckd_index`, their indices in
    requests; table_ptr: see pack_ckd_requests."""
    nwl = len(requests)
    dev_w, dev_off = [], 0
    wl = np.zeros(nwl, dtype=PROFILE_WL_DTYPE)
    gas, iks, counts = [], [], []
    nblev, off = 0, 0
    for w, r in enumerate(requests):
        e = wl[w]
        for k in ("tr", "hr", "ta", "ha", "a_tronc", "piz", "piztr", "zout"):
            e[k] = float(r[k])
        e["smax"] = int(r["smax"])
        if r.get("ik") is None:
            e["nterm"], e["nbins"], e["absprofil"] = 0, 1, 7
            iks.append(np.zeros((1, 8), dtype=np.int32))
            counts.append(1)
            continue
        ik = np.ascontiguousarray(r["ik"], dtype=np.int32)
        ro = np.ascontiguousarray(r["ro"], dtype=np.float64)
        alt = np.ascontiguousarray(r["altabs"], dtype=np.float64).ravel()
        nlev = int(alt.size)
        if r.get("xk") is None and r.get("prep") is not None:
            if ik.ndim != 2 or ik.shape[1] != 8 or ik.shape[0] < 1 or nlev != 50 or ro.shape != (8, nlev - 1):
                raise ValueError("request %d: ik must be [nb][8], ro [8][49], altabs [50] with the tables made on the device" % w)
            if nblev and nlev != nblev:
                raise ValueError("request %d: every wavelength of a launch must have the same number of absorption levels" % w)
            nblev = nlev
            e["nterm"], e["nbins"], e["absprofil"] = 5, ik.shape[0], int(r["absprofil"])
            e["xk_off"], e["ro_off"], e["alt_off"] = dev_off, off, off + ro.size        # (xk_off: moved behind buf below)
            dev_off += 8 * 5 * (nlev - 1)
            off += ro.size + nlev
            gas += [ro.ravel(), alt]
            dev_w.append(w)
            iks.append(ik)
            counts.append(ik.shape[0])
            continue
        xk = np.ascontiguousarray(r["xk"], dtype=np.float64)
        if ik.ndim != 2 or ik.shape[1] != 8 or ik.shape[0] < 1 or xk.ndim != 3 or xk.shape[0] != 8 or xk.shape[1] < 1 or \
                xk.shape[2] != nlev - 1 or ro.shape != (8, nlev - 1):
            raise ValueError("request %d: ik must be [nb][8], xk [8][nterm][nlev-1], ro [8][nlev-1], altabs [nlev]" % w)
        if nblev and nlev != nblev:
            raise ValueError("request %d: every wavelength of a launch must have the same number of absorption levels" % w)
        nblev = nlev
        e["nterm"], e["nbins"], e["absprofil"] = xk.shape[1], ik.shape[0], int(r["absprofil"])
        e["xk_off"], e["ro_off"], e["alt_off"] = off, off + xk.size, off + xk.size + ro.size
        off += xk.size + ro.size + nlev
        gas += [xk.ravel(), ro.ravel(), alt]
        iks.append(ik)
        counts.append(ik.shape[0])
    nb = int(sum(counts))
    wob = np.repeat(np.arange(nwl, dtype=np.int32), counts)
    if nb % 2:
        wob = np.concatenate([wob, np.zeros(1, dtype=np.int32)])          # (8-byte units)
    tail = [np.concatenate(iks).ravel().view(np.float64), wob.view(np.float64)]
    out = dict(wl=wl, gas_doubles=off, ik_off=off, wob_off=off + 4 * nb, nb=nb, nblev=nblev,
               seg=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), ckd=None, ckd_index=dev_w, device_doubles=dev_off)
    if dev_w:
        if table_ptr is None:
            raise ValueError("requests with `prep` need table_ptr (the device addresses of the coefficient tables)")
        axes_off = off + sum(t.size for t in tail)
        ckd = pack_ckd_requests([requests[w]["prep"] for w in dev_w], table_ptr, xk_off=wl["xk_off"][dev_w], base=axes_off)
        total = axes_off + ckd["axes"].size
        wl["xk_off"][dev_w] += total
        ckd["wl"]["xk_off"] += total
        ckd["out_doubles"] = total + dev_off
        tail.append(ckd["axes"])
        out["ckd"] = ckd
    out["buf"] = np.concatenate(gas + tail)
    return out


def make_profiles_spectrum(requests, device=0, stream=None, lp=608, part=None, true_depth=False):
    """The profile stage of MANY wavelengths in three launches (sosgpu_profile_spectrum: no-gas profiles, SOS_ABSPROFILE and
    SOS_PROFILE of every bin of every wavelength, each wavefront taking its wavelength's parameters from a device table)
    instead of three per wavelength.  requests: see pack_profile_requests.  One upload (its buf), one cleared output allocation
    for all bins (the two blocks of SosContext.make_profiles), queued on `stream` (a torch stream; None: the current one),
    nothing waited for.  Returns one `bins` dict per request, as make_profiles returns it for that wavelength alone -- the same
    keys, dtypes and, bit for bit, values; the tensors are views of the shared blocks.
    part: optional dict, filled with `bins` (all bins as one dict, for output_levels), `tabs` (per request: TAUABS[nb][nlev]
    view, or None without gas), `seg`, and -- when the library refuses a wavelength -- `bad`, its index in requests.
    A gas request with `prep` in place of `xk` (pack_profile_requests) gets its coefficient tables from ONE launch of
    sosgpu_ckd_layer_tables over all such requests, on the device-resident CKD files, queued on the same stream ahead of the
    profile kernels and writing straight to the request's xk block: no host interpolation, no upload of xk.  `part` then also
    holds `ckd_status` (int32 device tensor, one entry per such request: absorption.CKD_STATUS_MESSAGES) and `ckd_index` (their
    indices in requests); without such requests `ckd_status` is None.
    true_depth=True (sosgpu_profile_spectrum_true): every dict, and part["bins"], also holds `hvrai` (the untruncated depth
    rows, as SosContext.make_profiles(true_depth=True) returns them), inside the same cleared block."""
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    tables = {}
    pk = pack_profile_requests(requests, _ckd_table_ptr(tables, dev))
    nwl, nb, nblev, seg = len(requests), pk["nb"], pk["nblev"], pk["seg"]
    L = capi.lib()
    need = int(L.sosgpu_profile_spectrum_work_bytes(nwl))          # (no-gas blocks, then the table: whole doubles)
    if part is None:
        part = {}
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ckd, status, work = pk["ckd"], None, None
        if ckd is None:
            up = _upload(torch.from_numpy(pk["buf"]), dev)
        else:
            # (the xk blocks the device fills stand behind the uploaded part of the one gas buffer)
            up = torch.empty(pk["buf"].size + pk["device_doubles"], dtype=torch.float64, device=dev)
            up[:pk["buf"].size].copy_(torch.from_numpy(pk["buf"]).pin_memory(), non_blocking=True)
            refused = {}
            try:
                status, work = _ckd_launch(L, dev, ckd, up, ckd["out_doubles"], up, ckd["out_doubles"], st, refused)
            finally:
                if "bad" in refused:
                    part["bad"] = int(pk["ckd_index"][refused["bad"]])
        # (two cleared blocks for the whole part; the work area of the launch rides at the end of the first)
        o_z, o_s, o_zz, o_t = nb * 3 * lp, nb * 4 * lp, nb * (4 * lp + 4), nb * (4 * lp + 5)
        o_ng = o_t + nb * nblev
        o_hv = o_ng + need // 8
        fb = torch.zeros(o_hv + (nb * lp if true_depth else 0), dtype=torch.float64, device=dev)
        hvrai = fb[o_hv:].view(nb, lp) if true_depth else None
        ib = torch.zeros(3 * nb, dtype=torch.int32, device=dev)
        prof, zprof, scal = fb[:o_z].view(nb, 3, lp), fb[o_z:o_s].view(nb, lp), fb[o_s:o_zz].view(nb, 4)
        zz, tabs = fb[o_zz:o_t], (fb[o_t:o_ng].view(nb, nblev) if nblev else None)
        nt, iborm, jout = ib[:nb], ib[nb:2 * nb], ib[2 * nb:]
        any_out = bool((pk["wl"]["zout"] != -1.0).any())
        ik_t = up[pk["ik_off"]:pk["wob_off"]].view(torch.int32) if nblev else None
        bad = C.c_int(-1)
        args = (dev.index or 0, nwl, pk["wl"].ctypes.data_as(C.c_void_p), nb, _ptr(up[pk["wob_off"]:]),
                _ptr(ik_t), _ptr(up) if nblev else None, pk["gas_doubles"] if ckd is None else up.numel(), nblev, lp,
                _ptr(fb[o_ng:o_hv]), need, _ptr(tabs), _ptr(prof), _ptr(nt), _ptr(iborm),
                _ptr(zprof), _ptr(jout) if any_out else None, _ptr(zz) if any_out else None, _ptr(scal), C.byref(bad))
        rc = L.sosgpu_profile_spectrum_true(*args, _ptr(hvrai), st) if true_depth else L.sosgpu_profile_spectrum(*args, st)
    if rc != 0 and bad.value >= 0:
        part["bad"] = int(bad.value)
    capi.check(rc, "sosgpu_profile_spectrum_true" if true_depth else "sosgpu_profile_spectrum")
    out, tabs_l = [], []
    for w in range(nwl):
        b0, b1 = int(seg[w]), int(seg[w + 1])
        lev = float(pk["wl"]["zout"][w]) != -1.0
        out.append(dict(nb=b1 - b0, lp=lp, perm=None, nt=nt[b0:b1], iborm=iborm[b0:b1], prof=prof[b0:b1],
                        jout=jout[b0:b1] if lev else None, zz=zz[b0:b1] if lev else None, zprof=zprof[b0:b1], scal=scal[b0:b1]))
        if true_depth:
            out[-1]["hvrai"] = hvrai[b0:b1]
        tabs_l.append(tabs[b0:b1] if pk["wl"]["nterm"][w] else None)
    part.update(bins=dict(nb=nb, lp=lp, perm=None, nt=nt, iborm=iborm, prof=prof, jout=None, zz=None, zprof=zprof, scal=scal),
                tabs=tabs_l, seg=seg, upload=up, ckd_status=status, ckd_index=pk["ckd_index"],
                ckd_keep=(work, [t[2] for t in tables.values()]))
    if true_depth:
        part["bins"]["hvrai"] = hvrai
    return out


def layer_lp(nt):
    """Row length for an aerosol-layer profile of nt levels: 32, 64 or 608 -- the level class (lp <= 32, <= 64, above) of the
    row upload_bins gives the host profile (16 ceil((nt + 1) / 16)), which is what selects the solver kernel.  A thin layer
    (tr + ta < 0.32) so keeps the LDS-resident kernels, and the device profile the solve of the host profile."""
    return 32 if nt < 32 else 64 if nt < 64 else 608


def pack_layer_requests(requests, lp=608, true_depth=False):
    """Host side of make_layer_profiles_spectrum (pure numpy): the table and the layout of the one device block of a list of
    aerosol-layer requests.  A request is a dict with the arguments of SosContext.make_layer_profile of one wavelength -- tr, hr,
    ta, zmin, zmax, a_tronc, piz, piztr, zout -- and `smax`, the highest Fourier order of its context.  Returns a dict:
      wl        structured array [nwl] (capi.LAYER_WL_DTYPE = sosgpu_layer_wl): the one buffer that is uploaded
      nb, seg   a wavelength is one bin: nb = nwl, seg = 0..nwl
      off       where the sections of the cleared block start, in doubles: prof[nb][3][lp], zprof[nb][lp], scal[nb][4], zz[nb],
                hvrai[nb][lp] (true_depth, else empty), work (the call's work area, work_doubles long), ints (nt, iborm and
                jout[nb] as int32)
      doubles   length of the block."""
    nwl = len(requests)
    wl = np.zeros(nwl, dtype=capi.LAYER_WL_DTYPE)
    for w, r in enumerate(requests):
        for k in ("tr", "hr", "ta", "zmin", "zmax", "a_tronc", "piz", "piztr", "zout"):
            wl[k][w] = float(r[k])
        wl["smax"][w] = int(r["smax"])
    nb = nwl
    work_doubles = -(-nwl * capi.LAYER_ENTRY_BYTES // 8)
    off, at = {}, 0
    for name, n in (("prof", nb * 3 * lp), ("zprof", nb * lp), ("scal", nb * 4), ("zz", nb),
                    ("hvrai", nb * lp if true_depth else 0), ("work", work_doubles), ("ints", -(-3 * nb // 2))):
        off[name] = at
        at += n
    return dict(wl=wl, nb=nb, seg=np.arange(nwl + 1, dtype=np.int64), off=off, work_doubles=work_doubles, doubles=at)


def make_layer_profiles_spectrum(requests, device=0, stream=None, lp=608, part=None, true_depth=False):
    """The aerosol-layer profiles (IPROFIL = 2) of MANY wavelengths in one launch (sosgpu_profile_layer_spectrum), shaped like
    make_profiles_spectrum.  requests: see pack_layer_requests.  One upload (the table, by the library), one cleared allocation
    for all bins and the work area, queued on `stream` (a torch stream; None: the current one), nothing waited for.  Returns one
    `bins` dict per request, as SosContext.make_layer_profile returns it for that wavelength alone -- the same keys, dtypes and,
    bit for bit, values; the tensors are views of the shared block.
    part: optional dict, filled with `bins` (all bins as one dict, for output_levels), `tabs` (None per request), `seg`, and --
    when the library refuses a wavelength -- `bad`, its index in requests."""
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    pk = pack_layer_requests(requests, lp, true_depth)
    nwl, nb, off = len(requests), pk["nb"], pk["off"]
    L = capi.lib()
    need = int(L.sosgpu_profile_layer_spectrum_work_bytes(nwl))
    if need > 8 * pk["work_doubles"]:
        raise RuntimeError("sosgpu_profile_layer_spectrum_work_bytes: the table entry is not capi.LAYER_ENTRY_BYTES long")
    if part is None:
        part = {}
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        fb = torch.zeros(pk["doubles"], dtype=torch.float64, device=dev)
        prof, zprof = fb[:off["zprof"]].view(nb, 3, lp), fb[off["zprof"]:off["scal"]].view(nb, lp)
        scal, zz = fb[off["scal"]:off["zz"]].view(nb, 4), fb[off["zz"]:off["hvrai"]]
        hvrai = fb[off["hvrai"]:off["work"]].view(nb, lp) if true_depth else None
        work = fb[off["work"]:off["ints"]]
        ib = fb[off["ints"]:].view(torch.int32)
        nt, iborm, jout = ib[:nb], ib[nb:2 * nb], ib[2 * nb:3 * nb]
        any_out = bool((pk["wl"]["zout"] != -1.0).any())
        bad = C.c_int(-1)
        rc = L.sosgpu_profile_layer_spectrum(dev.index or 0, nwl, pk["wl"].ctypes.data_as(C.c_void_p), lp, _ptr(work), need,
                                             _ptr(prof), _ptr(nt), _ptr(iborm), _ptr(zprof), _ptr(jout) if any_out else None,
                                             _ptr(zz) if any_out else None, _ptr(scal), _ptr(hvrai), C.byref(bad), st)
    if rc != 0 and bad.value >= 0:
        part["bad"] = int(bad.value)
    capi.check(rc, "sosgpu_profile_layer_spectrum")
    out = []
    for w in range(nwl):
        lev = float(pk["wl"]["zout"][w]) != -1.0
        out.append(dict(nb=1, lp=lp, perm=None, nt=nt[w:w + 1], iborm=iborm[w:w + 1], prof=prof[w:w + 1],
                        jout=jout[w:w + 1] if lev else None, zz=zz[w:w + 1] if lev else None, zprof=zprof[w:w + 1],
                        scal=scal[w:w + 1]))
        if true_depth:
            out[-1]["hvrai"] = hvrai[w:w + 1]
    part.update(bins=dict(nb=nb, lp=lp, perm=None, nt=nt, iborm=iborm, prof=prof, jout=None, zz=None, zprof=zprof, scal=scal),
                tabs=[None] * nwl, seg=pk["seg"], ckd_status=None, ckd_index=[])
    if true_depth:
        part["bins"]["hvrai"] = hvrai
    return out


def concat_levels(levels_list):
    """Concatenate the output slots of per-wavelength bin dicts (SosContext.output_levels of each, all with the same altitude
    count K) in the bin order of concat_bins(bins_list): jout / zz / tauout [K][nb_total].  The levels stay valid on the padded
    level axis of concat_bins (the padding appends levels past every bin's NT; jout <= NT).  Returns the `levels` of
    solve_spectrum_levels."""
    nz = levels_list[0]["nz"]
    if any(lv["nz"] != nz for lv in levels_list):
        raise ValueError("every wavelength must have the same number of output altitudes")
    parts = [lv for lv in levels_list if lv["jout"] is not None]          # (a batch without bins has no tensors)
    if not parts:
        return dict(nz=nz, jout=None, zz=None, tauout=None)
    cat = lambda k: torch.cat([lv[k] for lv in parts], dim=1).contiguous()
    levels = dict(nz=nz, jout=cat("jout"), zz=cat("zz"), tauout=cat("tauout"))
    if all(lv.get("tauvrai") is not None for lv in parts):
        levels["tauvrai"] = cat("tauvrai")
    return levels


def _spectrum_order(cx, bins, order):
    """The workgroup order of a table launch (solve_spectrum): a device int32 permutation, or None."""
    if isinstance(order, str) and order == "cost" and bins["lp"] <= 64:
        order = None
    if isinstance(order, str) and order == "cost":
        htot = bins["prof"][:, 0, :].gather(1, bins["nt"].long().clamp(min=0, max=bins["lp"] - 1)[:, None])[:, 0]
        return torch.argsort(htot, descending=True, stable=True).to(torch.int32)
    if order is not None:
        return _dev_i32(order, cx.device)
    return None


def solve_spectrum_levels(table, bins, ctx_of_bin, seg, aik, levels, out=None, order="cost", tdifmug=None):
    """solve_spectrum for K output altitudes: ONE launch of the fused solver over the bins of many wavelengths, every bin with
    K output slots (sosgpu_os_solve_multi_levels), then one segmented SOS_AGGREGATE per altitude with that altitude's TAUOUT in
    scal[:, 3] (SosContext.aggregate_levels).  bins / ctx_of_bin / seg from concat_bins, levels from concat_levels,
    aik[nb] device tensor in the same order; order as in solve_spectrum.  Returns (rec[K][nwavelengths][smax+1][3][W],
    scal[K][nwavelengths][10+N]) device tensors; no synchronisation.  Slot k of wavelength g equals solve_spectrum's record of
    g with that altitude's profile, bit for bit.  tdifmug: optional per-bin [nb][N] diffuse transmissions, aggregated per
    segment into every altitude's scalar block."""
    cx = table.ctxs[0]
    nz, nb = levels["nz"], bins["nb"]
    if out is None:
        out = cx.alloc_outputs(nb, zero=False)
        out["rec"] = torch.empty((nz, nb, cx.smax + 1, 3, cx.w), dtype=torch.float64, device=cx.device)
    ord_t = _spectrum_order(cx, bins, order)
    capi.check(capi.lib().sosgpu_os_solve_multi_levels(cx._h, _ptr(table.table), _ptr(ctx_of_bin), _ptr(ord_t), nb, bins["lp"],
                                                       _ptr(bins["nt"]), _ptr(bins["iborm"]), _ptr(bins["prof"]), nz,
                                                       _ptr(levels["jout"]), _ptr(levels["zz"]), _ptr(out["rec"]),
                                                       _ptr(out["norders"]), _ptr(out["iglast"]), _ptr(out["flux"]),
                                                       cx._stream()), "sosgpu_os_solve_multi_levels")
    return cx.aggregate_levels(out, levels, aik, seg=seg, scal=bins.get("scal"), tdifmug=tdifmug)


def solve_many(items, n_streams=16):
    """Hyperspectral shape of the work (BASELINE config 5): MANY wavelengths with FEW CKD bins each.  One wavelength = one
    SosContext (its own source operators); its few bins occupy a fraction of the chip (one workgroup per bin, 512 resident),
    so the wavelengths are issued round-robin on `n_streams` HIP streams and overlap on the device.
    items: list of (ctx, bins, aik) with bins from ctx.upload_bins / make_profiles and aik a DEVICE tensor (a host array would
    be copied after the solve on the same stream, which blocks the host and serialises everything).
    Returns [(rec, scal)] of ctx.aggregate per wavelength, in order; the caller synchronises (torch.cuda.synchronize()).
    The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4): export GPU_MAX_HW_QUEUES=16 before
    the first GPU call -- measured on 128 wavelengths x 32 bins: 18.6 k bins/s on one stream, 47.9 k (4 queues), 76.4 k (8),
    125 k (16) (scripts/spectrum_bench.py, profiles/r02_spectrum.txt)."""
    if not items:
        return []
    dev = items[0][0].device
    cur = torch.cuda.current_stream(dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(1, min(n_streams, len(items))))]
    for st in streams:
        st.wait_stream(cur)
    res = []
    for i, (cx, bins, aik) in enumerate(items):
        with torch.cuda.stream(streams[i % len(streams)]):
            out = cx.solve(bins, cx.alloc_outputs(bins["nb"], zero=False))
            res.append(cx.aggregate(out, aik, scal=bins.get("scal")))
    for st in streams:
        cur.wait_stream(st)
    return res
