"""Cells of the aerosol-layer profile tests (test_layer_profile.py, test_layer_profile_gpu.py): single profiles of 8 to 600
levels with their level counts, the refusals, and the host chain the device is held to bit for bit --
geometry.profile_layer, synth.rescale_profile, solver.output_levels_host and the TAUOUT statements of run_sos._layer_profile."""
import numpy as np

# (tr, hr, ta, zmin, zmax) -> NT, (nbsc_c1, nbsc_c2, nbsc_c3)
CELLS = [
    ((0.02, 8.0, 0.02, 0.0, 1.0), 8, (3, 4, 0)),            # smallest; c1 at its floor
    ((0.04, 8.0, 0.03, 0.0, 2.0), 14, (5, 8, 0)),           # layer on the ground, no third zone
    ((0.02, 8.0, 0.05, 3.0, 3.5), 14, (3, 6, 3)),           # both floors raised from 2 and 1
    ((0.0973, 8.0, 0.3, 0.0, 2.0), 79, (14, 64, 0)),
    ((0.0973, 8.0, 0.3, 1.0, 3.0), 79, (12, 62, 3)),        # the golden case's shape
    ((0.0973, 8.0, 0.2, 10.0, 12.0), 59, (4, 40, 13)),      # large third zone
    ((0.0973, 8.0, 0.5, 0.02, 1.0), 119, (16, 98, 3)),      # zmin - dzt = 0.01
    ((0.05, 6.5, 0.4, 2.0, 5.0), 90, (4, 81, 3)),
    ((0.1, 8.0, 0.2155, 1.0, 3.0), 63, None),               # either side of the 64-lane stride
    ((0.1, 8.0, 0.2205, 1.0, 3.0), 64, None),
    ((0.1, 8.0, 0.2255, 1.0, 3.0), 65, None),
    ((0.3, 8.0, 3.2, 1.0, 4.0), 600, (31, 562, 5)),         # NT capped at CTE_OS_NT
    ((0.2, 8.0, 2.8, 0.5, 2.5), 600, (29, 566, 3)),
]
PARAMS = [c[0] for c in CELLS]
TAIL_CELLS = [PARAMS[0], PARAMS[2], PARAMS[4], PARAMS[11]]                 # NT = 8, 14, 79, 600

E_ARG, E_UNSUPPORTED = -1, -3                                              # SOSGPU_E_ARG, SOSGPU_E_UNSUPPORTED
REFUSALS = [
    ((0.1, 8.0, 2e-5, 1.0, 3.0), E_UNSUPPORTED, "ERROR 1020"),             # ta / nbsc_c2 = 6.7e-6
    ((0.03, 8.0, 0.012, 1.0, 2.0), E_UNSUPPORTED, "ERROR 1020"),           # nbsc_c2 = 0
    ((0.1, 8.0, 0.3, 2.0, 1.0), E_ARG, "Zmin"),                            # zmax <= zmin
    ((0.1, 8.0, 0.3, 2.0, 2.0), E_ARG, "Zmin"),
    ((0.1, 8.0, 0.3, -0.5, 2.0), E_ARG, "Zmin"),                           # zmin < 0
]

PIZ = 0.9                                                                  # single-scattering albedo of the truncation cases
LP = 608


def tail_zouts(cell):
    """The output altitudes of the tail cases: standard output, ground, the layer's edges and middle, inside the 10 m
    transition above the layer, far above it."""
    zmin, zmax = cell[3], cell[4]
    return [-1.0, 0.0, zmin, zmax, 0.5 * (zmin + zmax), zmax + 0.005, 50.0]


def host_chain(pkg, cell, a_tronc=0.0, piz=1.0, piztr=1.0, zout=-1.0, smax=8, lp=LP):
    """What run_sos._layer_profile makes on the host (SOS_LAYER_PROFILE_HOST=1) for one layer, in the layout of the device
    outputs: nt, iborm, prof[3][lp], zprof[lp], hvrai[lp], jout, zz, scal[4]."""
    h, xdel, ydel, zprof = pkg.geometry.profile_layer(*cell)
    nt = len(h) - 1
    hv = np.array(h, dtype=np.float64)
    ttot_vrai = h[-1]
    h, xdel, ydel, ib = pkg.synth.rescale_profile(h, xdel, ydel, a_tronc, piz, piztr, smax)
    jout, zz = 0, 0.0
    if zout == -1.0:
        tauout = h[0]
    else:
        jh, zh = pkg.solver.output_levels_host(zprof[None], [zout])
        jout, zz = int(jh[0, 0]), float(zh[0, 0])
        tauout = (1 - zz) * h[jout - 1] + zz * h[jout]
    prof = np.zeros((3, lp))
    prof[0, :nt + 1], prof[1, :nt + 1], prof[2, :nt + 1] = h, xdel, ydel
    zp, hvp = np.zeros(lp), np.zeros(lp)
    zp[:nt + 1], hvp[:nt + 1] = zprof, hv
    return dict(nt=nt, iborm=min(ib, smax), prof=prof, zprof=zp, hvrai=hvp, jout=jout, zz=zz,
                scal=np.array([0.0, h[-1], ttot_vrai, tauout]))
