"""A/B of sensor channels on the spectrum of scripts/hyperspectral_bench.py (BASELINE config 5) in ONE process and one build:
run_sos.sos_spectrum_channels (the response-weighted sums formed on the device, sosgpu_channel_accumulate per chunk) against
run_sos.sos_spectrum followed by the host convolution of its tuples -- or, with --altitudes K, sos_spectrum_levels at the first
K altitudes of scripts/spectrum_levels_bench.py.  16 box-car channels of equal width (156 wavelengths each on the full
spectrum).  The host convolution is the cheapest a user could write: a = a + w * x on the rows and columns of the six I, Q, U
tables that are in use, nothing else.  The legs alternate after a warm-up of both: channels 1, spectrum 1, channels 2, ...
Prints every pass with its host phases, then the sorted rates, the median and the spread (max - min) of each leg, the medians
of the trphi / finish / channels phases, and the peak resident set after each leg's warm-up (resource.getrusage; the channel
leg is warmed first, the counter only grows)."""
import resource, time
import ab_harness as ab
QUEUES = ab.queues("4")
import numpy as np
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
    ap = ab.parser()
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--altitudes", type=int, default=0, help="0: sos_spectrum; K: sos_spectrum_levels at K altitudes")
    ap.add_argument("--one-leg", choices=["channels", "spectrum"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    rs = ab.package().run_sos
    ab.synthetic_tables(link_aerosols=True)
    kws = hb.spectrum_kwargs(rs, a.every)
    kws = kws[:NCHAN * (len(kws) // NCHAN)]
    alts = ALTS[:a.altitudes]
    w = boxcars(len(kws))
    nrow = len(range(0, 361, int(kws[0]["pas_phi"])))
    rep = ab.Report(a.out)
    say = rep.say
    say("spectrum: %d wavelengths, %d box-car channels of %d, altitudes %s, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), NCHAN, len(kws) // NCHAN, alts or "(sos_spectrum)", a.chunk, QUEUES))

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

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, "wavelengths/s")
    got = leg("channels")[2]
    rss_channels = rss()
    ref = leg("spectrum")[2]
    rss_spectrum = rss()
    # the device applies the reference's output thresholds to the sums; on this spectrum no sum comes near them
    say("warm-up passes done; I, Q, U of the two legs identical, bit for bit: %s" % ab.tuples_identical(got, ref))
    say("peak resident set after the warm-up of the channel leg %.0f MB, after that of the spectrum leg %.0f MB" % (
        rss_channels, rss_spectrum))
    del got, ref
    _, phases = ab.alternate({name: (lambda name=name: leg(name)[:2]) for name in ("channels", "spectrum")}, a.runs,
                             "wavelengths/s", say, per_pass=ab.host_phases(len(kws), "wavelength"))
    ab.phase_medians(phases, len(kws), "wavelength", say, keys=("trphi", "finish", "channels"))
    say("peak resident set at the end %.0f MB" % rss())
    rep.close()


if __name__ == "__main__":
    main()
