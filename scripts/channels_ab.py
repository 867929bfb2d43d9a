"""A/B of sensor channels on the spectrum of scripts/hyperspectral_bench.py (BASELINE config 5) in ONE process and one build:
run_sos.sos_spectrum_channels (the response-weighted sums formed on the device, sosgpu_channel_accumulate per chunk) against
run_sos.sos_spectrum followed by the host convolution of its tuples -- or, with --altitudes K, sos_spectrum_levels at the first
K altitudes of scripts/spectrum_levels_bench.py.  16 box-car channels of equal width (156 wavelengths each on the full
spectrum).  The host convolution is the cheapest a user could write: a = a + w * x on the rows and columns of the six I, Q, U
tables that are in use, nothing else.  The legs alternate after a warm-up of both: channels 1, spectrum 1, channels 2, ...
Prints every pass with its host phases, then the sorted rates, the median and the spread (max - min) of each leg, the medians
of the trphi / finish / channels phases, and the peak resident set after each leg's warm-up (resource.getrusage; the channel
leg is warmed first, the counter only grows)."""
import argparse, importlib, os, resource, statistics, sys, tempfile, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_ckd
import hyperspectral_bench as hb
from spectrum_levels_bench import ALTS

NCHAN = 16
SUMMED = (5, 6, 7, 12, 13, 14)                               # i, q, u up and down in OUTPUT_NAMES


def boxcars(n):
    """[NCHAN][n]: channel c covers the calls c * width .. (c + 1) * width - 1, width = n // NCHAN; calls past the last are in none."""
    width = n // NCHAN
    w = np.zeros((NCHAN, n))
    for c in range(NCHAN):
        w[c, c * width:(c + 1) * width] = 1.0
    return w


def host_convolution(tuples, w, nrow):
    """What the user of sos_spectrum does next: per channel the weighted sum of the used part of the six I, Q, U tables."""
    wn = np.array([row / np.cumsum(row)[-1] for row in w])
    n = int(tuples[0][0])
    out = []
    for c in range(len(w)):
        acc = [np.zeros((nrow, n)) for _ in SUMMED]
        for i in np.flatnonzero(wn[c]):
            for a, e in enumerate(SUMMED):
                acc[a] = acc[a] + wn[c, i] * tuples[i][e][:nrow, :n]
        out.append(acc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--altitudes", type=int, default=0, help="0: sos_spectrum; K: sos_spectrum_levels at K altitudes")
    ap.add_argument("--one-leg", choices=["channels", "spectrum"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    hb.link_aerosol_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    kws = hb.spectrum_kwargs(rs, a.every)
    kws = kws[:NCHAN * (len(kws) // NCHAN)]
    alts = ALTS[:a.altitudes]
    w = boxcars(len(kws))
    nrow = len(range(0, 361, int(kws[0]["pas_phi"])))
    print("spectrum: %d wavelengths, %d box-car channels of %d, altitudes %s, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), NCHAN, len(kws) // NCHAN, alts or "(sos_spectrum)", a.chunk, os.environ.get("GPU_MAX_HW_QUEUES")), flush=True)

    def leg(name):
        tm = {}
        t0 = time.perf_counter()
        if name == "channels":
            out = rs.sos_spectrum_channels(kws, w, altitudes=alts or None, timings=tm, chunk=a.chunk)
            out = [[[t[e][:nrow, :int(t[0])] for e in SUMMED] for t in (c if alts else [c])] for c in out]
        elif alts:
            spec = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk)
            per = [host_convolution([s[k] for s in spec], w, nrow) for k in range(len(alts))]
            out = [[per[k][c] for k in range(len(alts))] for c in range(NCHAN)]
        else:
            out = [[c] for c in host_convolution(rs.sos_spectrum(kws, timings=tm, chunk=a.chunk), w, nrow)]
        dt = time.perf_counter() - t0
        return len(kws) / dt, tm, out

    def rss():
        return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    if a.one_leg:
        leg(a.one_leg)                                       # warm-up pass: tables parsed, caches filled
        print("[%s] %.1f wavelengths/s" % (a.one_leg, leg(a.one_leg)[0]), flush=True)
        return
    got = leg("channels")[2]
    rss_channels = rss()
    ref = leg("spectrum")[2]
    rss_spectrum = rss()
    # the device applies the reference's output thresholds to the sums; on this spectrum no sum comes near them
    same = all(np.array_equal(x, y) for c1, c2 in zip(got, ref) for k1, k2 in zip(c1, c2) for x, y in zip(k1, k2))
    print("warm-up passes done; I, Q, U of the two legs identical, bit for bit: %s" % same, flush=True)
    print("peak resident set after the warm-up of the channel leg %.0f MB, after that of the spectrum leg %.0f MB" % (
        rss_channels, rss_spectrum), flush=True)
    del got, ref
    rates = {"channels": [], "spectrum": []}
    phases = {"channels": [], "spectrum": []}
    for k in range(a.runs):
        for name in ("channels", "spectrum"):
            r, tm, _ = leg(name)
            rates[name].append(r)
            phases[name].append(tm)
            print("[%s %d] %7.1f wavelengths/s   host phases per wavelength (ms): %s" % (
                name, k + 1, r, ", ".join("%s %.4f" % (q, 1e3 * v / len(kws)) for q, v in tm.items())), flush=True)
    for name, v in rates.items():
        print("wavelengths/s  %-8s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)), flush=True)
    for name, v in phases.items():
        print("median host phase per wavelength (ms)  %-8s: trphi %.4f, finish %.4f, channels %.4f" % (
            name, 1e3 * statistics.median(t["trphi"] for t in v) / len(kws), 1e3 * statistics.median(t["finish"] for t in v) / len(kws),
            1e3 * statistics.median(t.get("channels", 0.0) for t in v) / len(kws)), flush=True)
    print("peak resident set at the end %.0f MB" % rss(), flush=True)


if __name__ == "__main__":
    main()
