"""A spectrum at K output altitudes: K sos_spectrum calls (one -SOS.OutputAlt each) against ONE run_sos.sos_spectrum_levels, for
K = 1, 2, 4, 8.  Workload: the hyperspectral run of scripts/hyperspectral_bench.py (all eight gases with synthetic CKD tables,
log-normal aerosol, Roujean + Maignan surface, polar view), every k-th interval (--every).  Reports wall time, wavelength x
altitudes per second and the host phases (timings) of both forms, and checks the outputs equal bit for bit.
Usage: python scripts/spectrum_levels_bench.py [--every 10]   (profiles/spectrum_levels_bench.txt holds a run on the MI355X)"""
import argparse
import importlib
import os
import sys
import tempfile
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")          # hardware queues for the side streams of sos_spectrum (runtime default: 4)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_ckd
from hyperspectral_bench import spectrum_kwargs

ALTS = [-1.0, 3.0, 0.5, 12.0, 1.0, 8.0, 2.0, 20.0]
PHASES = ("prepare", "solve_launch", "wait", "trphi", "finish")


def _fmt(tm):
    return " ".join("%s %.2f" % (k, tm.get(k, 0.0)) for k in PHASES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=10, help="take every k-th interval of the spectrum")
    ap.add_argument("--chunk", type=int, default=256)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    kws = spectrum_kwargs(rs, a.every)
    nwl = len(kws)
    nb = sum(pkg.absorption.band_bin_count(kw["wa_simu"], 10.0) for kw in kws)
    print("spectrum_levels_bench: %d wavelengths, %d CKD bins, chunk %d" % (nwl, nb, a.chunk), flush=True)
    rs.sos_spectrum(kws[:8])                                # warm-up: library load, surface matrices, caches
    rs.sos_spectrum_levels(ALTS[:2], kws[:8])
    torch.cuda.synchronize()
    print("%2s %12s %12s %8s %14s %14s" % ("K", "K x spectrum", "levels", "speedup", "K x spec wl*alt/s", "levels wl*alt/s"))
    for K in (1, 2, 4, 8):
        alts = ALTS[:K]
        tms = [{} for _ in alts]
        t0 = time.perf_counter()
        ref = [rs.sos_spectrum([dict(kw, zout=z) for kw in kws], timings=tms[k], chunk=a.chunk) for k, z in enumerate(alts)]
        t_ref = time.perf_counter() - t0
        tl = {}
        t0 = time.perf_counter()
        got = rs.sos_spectrum_levels(alts, kws, timings=tl, chunk=a.chunk)
        t_lv = time.perf_counter() - t0
        same = all(np.array_equal(np.asarray(x), np.asarray(y))
                   for k in range(K) for i in range(nwl) for x, y in zip(ref[k][i], got[i][k]))
        print("%2d %10.2f s %10.2f s %7.2fx %14.1f %14.1f   bit-identical %s" % (
            K, t_ref, t_lv, t_ref / t_lv, nwl * K / t_ref, nwl * K / t_lv, same), flush=True)
        tsum = {p: sum(t.get(p, 0.0) for t in tms) for p in PHASES}
        print("     K x sos_spectrum phases (s): %s" % _fmt(tsum))
        print("     sos_spectrum_levels phases (s): %s" % _fmt(tl), flush=True)
    print("speedup = (K sos_spectrum calls) / (one sos_spectrum_levels); wl*alt/s = wavelengths x altitudes per second")


if __name__ == "__main__":
    main()
