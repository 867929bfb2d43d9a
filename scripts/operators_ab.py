"""A/B of the operator stage of run_sos.sos_spectrum in ONE process and one build: the batched default
(sosgpu_noyaux_spectrum, at most five launches per part) against SOS_SPECTRUM_OPERATORS_PER_CALL=1 (four or five launches per
wavelength on its side stream), on the spectrum of scripts/hyperspectral_bench.py (BASELINE config 5).  The switch is read by
every pass, so the legs alternate inside the process: batched 1, per call 1, batched 2, ...  Prints every pass, then the sorted
rates, the median and the spread (max - min) of each leg.  The number of hardware queues is the process's GPU_MAX_HW_QUEUES
(unlike hyperspectral_bench.py this script does not set it)."""
import argparse, importlib, os, statistics, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
queues = os.environ.get("GPU_MAX_HW_QUEUES")
import synth_ckd
import hyperspectral_bench as hb
if queues is None:
    os.environ.pop("GPU_MAX_HW_QUEUES", None)              # (hyperspectral_bench sets 16 on import)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--aer-model", choices=sorted(hb.AER_MODELS), default="lnd")
    ap.add_argument("--surface", choices=["maignan", "lambert"], default="maignan",
                    help="maignan: the keywords of hyperspectral_bench (surface matrices, five launches); lambert: -SURF.Type 0")
    ap.add_argument("--one-leg", choices=["batched", "per_call"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    hb.link_aerosol_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    if a.surface == "lambert":
        hb.USER.update({"-SURF.Type": 0, "-SURF.Alb": 0.1})
    kws = hb.spectrum_kwargs(rs, a.every, a.aer_model)
    print("spectrum: %d wavelengths, surface %s, aerosol model %s, GPU_MAX_HW_QUEUES=%s" % (len(kws), a.surface, a.aer_model, queues), flush=True)

    def leg(name):
        if name == "per_call":
            os.environ["SOS_SPECTRUM_OPERATORS_PER_CALL"] = "1"
        else:
            os.environ.pop("SOS_SPECTRUM_OPERATORS_PER_CALL", None)
        tm = {}
        t0 = time.perf_counter()
        out = rs.sos_spectrum(kws, timings=tm, chunk=a.chunk)
        dt = time.perf_counter() - t0
        return len(kws) / dt, tm, out

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    if a.one_leg:
        leg(a.one_leg)                                       # warm-up pass: tables parsed, caches filled
        print("[%s] %.1f wavelengths/s" % (a.one_leg, leg(a.one_leg)[0]), flush=True)
        return
    ref = leg("batched")[2]
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for s1, s2 in zip(ref, leg("per_call")[2]) for x, y in zip(s1, s2))
    print("warm-up passes done; outputs of the two legs identical, bit for bit: %s" % same, flush=True)
    rates = {"batched": [], "per_call": []}
    for k in range(a.runs):
        for name in ("batched", "per_call"):
            r, tm, _ = leg(name)
            rates[name].append(r)
            print("[%s %d] %7.1f wavelengths/s   host phases per wavelength (ms): %s" % (
                name, k + 1, r, ", ".join("%s %.3f" % (q, 1e3 * v / len(kws)) for q, v in tm.items())), flush=True)
    for name, v in rates.items():
        print("wavelengths/s  %-8s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)), flush=True)


if __name__ == "__main__":
    main()
