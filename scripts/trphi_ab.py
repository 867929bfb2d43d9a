"""A/B of the azimuth recomposition of run_sos.sos_spectrum / sos_spectrum_levels in ONE process and one build: the batched
default (sosgpu_trphi_spectrum, one launch per chunk) against SOS_SPECTRUM_TRPHI_PER_CALL=1 (one sosgpu_trphi launch per
wavelength and altitude), on the spectrum of scripts/hyperspectral_bench.py (BASELINE config 5).  --altitudes 0: sos_spectrum;
K > 0: sos_spectrum_levels at the first K altitudes of scripts/spectrum_levels_bench.py.  The switch is read by every pass, so
the legs alternate inside the process: batched 1, per call 1, batched 2, ...  Prints every pass with its host phases, then the
sorted rates, the median and the spread (max - min) of each leg, and the medians of the trphi and finish phases."""
import argparse, importlib, os, statistics, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_ckd
import hyperspectral_bench as hb                              # (sets GPU_MAX_HW_QUEUES=16 unless the environment has a value)
from spectrum_levels_bench import ALTS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--altitudes", type=int, default=0, help="0: sos_spectrum; K: sos_spectrum_levels at K altitudes")
    ap.add_argument("--one-leg", choices=["batched", "per_call"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    hb.link_aerosol_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    kws = hb.spectrum_kwargs(rs, a.every)
    alts = ALTS[:a.altitudes]
    njobs = len(kws) * max(1, len(alts))
    print("spectrum: %d wavelengths, altitudes %s, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), alts or "(sos_spectrum)", a.chunk, os.environ.get("GPU_MAX_HW_QUEUES")), flush=True)

    def leg(name):
        if name == "per_call":
            os.environ["SOS_SPECTRUM_TRPHI_PER_CALL"] = "1"
        else:
            os.environ.pop("SOS_SPECTRUM_TRPHI_PER_CALL", None)
        tm = {}
        t0 = time.perf_counter()
        if alts:
            out = [t for r in rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk) for t in r]
        else:
            out = rs.sos_spectrum(kws, timings=tm, chunk=a.chunk)
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    if a.one_leg:
        leg(a.one_leg)                                       # warm-up pass: tables parsed, caches filled
        print("[%s] %.1f wavelengths x altitudes/s" % (a.one_leg, leg(a.one_leg)[0]), flush=True)
        return
    ref = leg("batched")[2]
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for s1, s2 in zip(ref, leg("per_call")[2]) for x, y in zip(s1, s2))
    print("warm-up passes done; outputs of the two legs identical, bit for bit: %s" % same, flush=True)
    del ref
    rates = {"batched": [], "per_call": []}
    phases = {"batched": [], "per_call": []}
    for k in range(a.runs):
        for name in ("batched", "per_call"):
            r, tm, _ = leg(name)
            rates[name].append(r)
            phases[name].append(tm)
            print("[%s %d] %7.1f wavelengths x altitudes/s   host phases per wavelength x altitude (ms): %s" % (
                name, k + 1, r, ", ".join("%s %.4f" % (q, 1e3 * v / njobs) for q, v in tm.items())), flush=True)
    for name, v in rates.items():
        print("wavelengths x altitudes/s  %-8s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)), flush=True)
    for name, v in phases.items():
        print("median host phase per wavelength x altitude (ms)  %-8s: trphi %.4f, finish %.4f" % (
            name, 1e3 * statistics.median(t["trphi"] for t in v) / njobs, 1e3 * statistics.median(t["finish"] for t in v) / njobs),
            flush=True)


if __name__ == "__main__":
    main()
