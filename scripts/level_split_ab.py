"""A/B of the true direct / diffuse split of run_sos.sos_spectrum_levels in ONE process and one build: fluxes=True, split=True
(the profile launches export the untruncated depth rows, one sosgpu_output_depths launch per part, one
sosgpu_level_transmission launch per solved group) against fluxes=True alone, on the spectrum of
scripts/spectrum_levels_bench.py (every --every-th interval of the hyperspectral run) at the first K altitudes of that script.
The legs alternate inside the process: flux 1, split 1, flux 2, ...  Prints every pass with its host phases, then the sorted
rates, the median and the spread (max - min) of each leg, and what the split costs per (wavelength, altitude) job, from the
medians.  The `flux` leg is the `on` leg of scripts/level_flux_ab.py (same spectrum, altitudes and chunk), whose output also
gives what fluxes=True itself costs over fluxes=False.  GPU_MAX_HW_QUEUES is taken from the environment.
--one-leg flux|split: a warm-up pass and a single pass of one leg (for a kernel trace)."""
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
    ap.add_argument("--one-leg", choices=["flux", "split"], help="a single pass of one leg (for a kernel trace)")
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
        out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=True, split=name == "split")
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    if a.one_leg:
        leg(a.one_leg)                                       # warm-up pass: tables parsed, caches filled
        print("[%s] %.1f wavelengths x altitudes/s" % (a.one_leg, leg(a.one_leg)[0]), flush=True)
        return
    ref, rflux = leg("flux")[2]
    got, flux = leg("split")[2]
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for r, g in zip(ref, got) for s1, s2 in zip(r, g) for x, y in zip(s1, s2))
    same = same and all(np.array_equal(f[:, :5], r) for f, r in zip(flux, rflux))
    # columns 5 + 6 restate column 2; row 0 is the standard output, whose column 5 restates element 18 of that altitude's tuple
    worst = max(float(np.max(np.abs(f[:, 5] + f[:, 6] - f[:, 2]) / f[:, 2])) for f in flux)
    e18 = all(f[0, 5] == t[0][18] for f, t in zip(flux, got)) if alts[0] == -1.0 else None
    below = sum(int((f[:, 5] < f[:, 0]).sum()) for f in flux)
    print("warm-up passes done; tuples and first five columns of the two legs identical, bit for bit: %s; columns 5 + 6 against "
          "column 2, worst relative difference %.2e; standard-output row equal to element 18: %s; rows with the true direct beam "
          "below the truncated one: %d of %d" % (same, worst, e18, below, njobs), flush=True)
    del ref, got, flux, rflux
    rates = {"flux": [], "split": []}
    phases = {"flux": [], "split": []}
    for k in range(a.runs):
        for name in ("flux", "split"):
            r, tm, _ = leg(name)
            rates[name].append(r)
            phases[name].append(tm)
            print("[%-5s %d] %7.1f wavelengths x altitudes/s   host phases per wavelength x altitude (ms): %s" % (
                name, k + 1, r, ", ".join("%s %.4f" % (q, 1e3 * v / njobs) for q, v in tm.items())), flush=True)
    for name, v in rates.items():
        print("wavelengths x altitudes/s  %-5s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)), flush=True)
    med = {name: statistics.median(v) for name, v in rates.items()}
    print("cost of the split per wavelength x altitude, from the medians: %.4f ms (%.4f -> %.4f ms per job)" % (
        1e3 / med["split"] - 1e3 / med["flux"], 1e3 / med["flux"], 1e3 / med["split"]), flush=True)
    for name, v in phases.items():
        print("median host phase per wavelength x altitude (ms)  %-5s: %s" % (
            name, ", ".join("%s %.4f" % (q, 1e3 * statistics.median(t[q] for t in v) / njobs) for q in v[0])), flush=True)


if __name__ == "__main__":
    main()
