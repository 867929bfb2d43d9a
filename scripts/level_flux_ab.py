"""A/B of the per-altitude fluxes of run_sos.sos_spectrum_levels in ONE process and one build: fluxes=True (one
sosgpu_level_flux_spectrum launch per chunk, the flux rows downloaded behind the recompositions) against fluxes=False, on the
spectrum of scripts/spectrum_levels_bench.py (every --every-th interval of the hyperspectral run) at the first K altitudes of
that script.  The legs alternate inside the process: off 1, on 1, off 2, ...  Prints every pass with its host phases, then the
sorted rates, the median and the spread (max - min) of each leg, and the medians of the fluxes and trphi phases per job.
GPU_MAX_HW_QUEUES is taken from the environment (the runs of profiles/level_flux.txt: 4).
--one-leg on|off: a warm-up pass and a single pass of one leg (for a kernel trace)."""
import argparse, importlib, os, statistics, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_ckd
from spectrum_levels_bench import ALTS, spectrum_kwargs     # (sets GPU_MAX_HW_QUEUES=16 unless the environment has a value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--altitudes", type=int, default=4)
    ap.add_argument("--one-leg", choices=["on", "off"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    kws = spectrum_kwargs(rs, a.every)
    alts = ALTS[:a.altitudes]
    njobs = len(kws) * len(alts)
    print("spectrum: %d wavelengths, altitudes %s, chunk %d (%d wavelengths per chunk), GPU_MAX_HW_QUEUES=%s" % (
        len(kws), alts, a.chunk, max(1, a.chunk // len(alts)), os.environ.get("GPU_MAX_HW_QUEUES")), flush=True)

    def leg(name):
        tm = {}
        t0 = time.perf_counter()
        out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=name == "on")
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    if a.one_leg:
        leg(a.one_leg)                                       # warm-up pass: tables parsed, caches filled
        print("[%s] %.1f wavelengths x altitudes/s" % (a.one_leg, leg(a.one_leg)[0]), flush=True)
        return
    ref = leg("off")[2]
    got, flux = leg("on")[2]
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for r, g in zip(ref, got) for s1, s2 in zip(r, g) for x, y in zip(s1, s2))
    # row 0 is the standard output: its total and up-going columns restate elements 20 and 21 of that altitude's tuple
    worst = max(max(abs(f[0, 2] / t[0][20] - 1), abs(f[0, 3] / t[0][21] - 1)) for f, t in zip(flux, got)) if alts[0] == -1.0 else -1.0
    print("warm-up passes done; 23-tuples of the two legs identical, bit for bit: %s; standard-output row against elements 20 / 21, "
          "worst relative difference %.2e" % (same, worst), flush=True)
    del ref, got, flux
    rates = {"off": [], "on": []}
    phases = {"off": [], "on": []}
    for k in range(a.runs):
        for name in ("off", "on"):
            r, tm, _ = leg(name)
            rates[name].append(r)
            phases[name].append(tm)
            print("[fluxes %-3s %d] %7.1f wavelengths x altitudes/s   host phases per wavelength x altitude (ms): %s" % (
                name, k + 1, r, ", ".join("%s %.4f" % (q, 1e3 * v / njobs) for q, v in tm.items())), flush=True)
    for name, v in rates.items():
        print("wavelengths x altitudes/s  fluxes %-3s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)), flush=True)
    for name, v in phases.items():
        print("median host phase per wavelength x altitude (ms)  fluxes %-3s: fluxes %.4f, trphi %.4f" % (
            name, 1e3 * statistics.median(t["fluxes"] for t in v) / njobs, 1e3 * statistics.median(t["trphi"] for t in v) / njobs),
            flush=True)


if __name__ == "__main__":
    main()
