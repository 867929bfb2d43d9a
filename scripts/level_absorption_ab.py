"""A/B of the actinic flux / absorbed power of run_sos.sos_spectrum_levels in ONE process and one build: fluxes=True,
absorption=True (the solves keep their per-bin records, one sosgpu_level_absorption launch per solved group, its block comes
down with the flux pairs) against fluxes=True alone, on the spectrum of scripts/spectrum_levels_bench.py (every --every-th
interval of the hyperspectral run) at the first K altitudes of that script.  The legs alternate inside the process: flux 1,
absorb 1, flux 2, ...  Prints every pass with its host phases, then the sorted rates, the median and the spread (max - min) of
each leg, and what the keyword costs per (wavelength, altitude) job, from the medians; the same lines go to --out (default
profiles/level_absorption_ab.txt).  The `flux` leg is the `on` leg of scripts/level_flux_ab.py (same spectrum, altitudes and
chunk).  GPU_MAX_HW_QUEUES is taken from the environment.  The feature is opt-in: no rate decides anything.
--one-leg flux|absorb: a warm-up pass and a single pass of one leg (for a kernel trace)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_absorption_ab.txt"))
    ap.add_argument("--one-leg", choices=["flux", "absorb"], help="a single pass of one leg (for a kernel trace)")
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
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("spectrum: %d wavelengths, altitudes %s, chunk %d (%d wavelengths per chunk), GPU_MAX_HW_QUEUES=%s" % (
        len(kws), alts, a.chunk, max(1, a.chunk // len(alts)), os.environ.get("GPU_MAX_HW_QUEUES")))

    def leg(name):
        tm = {}
        t0 = time.perf_counter()
        out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=True, absorption=name == "absorb")
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    if a.one_leg:
        leg(a.one_leg)                                       # warm-up pass: tables parsed, caches filled
        print("[%s] %.1f wavelengths x altitudes/s" % (a.one_leg, leg(a.one_leg)[0]), flush=True)
        return
    ref, rflux = leg("flux")[2]
    got, flux, absorb = leg("absorb")[2]
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for r, g in zip(ref, got) for s1, s2 in zip(r, g) for x, y in zip(s1, s2))
    same = same and all(np.array_equal(f, r) for f, r in zip(flux, rflux))
    rows = np.array([ab[k] for ab in absorb for k, z in enumerate(alts) if z != -1.0])
    nan_rows = all(np.isnan(ab[k]).all() for ab in absorb for k, z in enumerate(alts) if z == -1.0)
    say("warm-up passes done; tuples and flux rows of the two legs identical, bit for bit: %s; standard-output rows NaN: %s; "
        "absorbed_per_km over the %d interior rows: min %.3e median %.3e max %.3e; actinic_tot: min %.4f max %.4f" % (
            same, nan_rows, len(rows), rows[:, 4].min(), float(np.median(rows[:, 4])), rows[:, 4].max(), rows[:, 3].min(),
            rows[:, 3].max()))
    del ref, got, flux, rflux, absorb
    rates = {"flux": [], "absorb": []}
    phases = {"flux": [], "absorb": []}
    for k in range(a.runs):
        for name in ("flux", "absorb"):
            r, tm, _ = leg(name)
            rates[name].append(r)
            phases[name].append(tm)
            say("[%-6s %d] %7.1f wavelengths x altitudes/s   host phases per wavelength x altitude (ms): %s" % (
                name, k + 1, r, ", ".join("%s %.4f" % (q, 1e3 * v / njobs) for q, v in tm.items())))
    for name, v in rates.items():
        say("wavelengths x altitudes/s  %-6s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)))
    med = {name: statistics.median(v) for name, v in rates.items()}
    say("cost of absorption=True per wavelength x altitude, from the medians: %.4f ms (%.4f -> %.4f ms per job)" % (
        1e3 / med["absorb"] - 1e3 / med["flux"], 1e3 / med["flux"], 1e3 / med["absorb"]))
    for name, v in phases.items():
        say("median host phase per wavelength x altitude (ms)  %-6s: %s" % (
            name, ", ".join("%s %.4f" % (q, 1e3 * statistics.median(t[q] for t in v) / njobs) for q in v[0])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
