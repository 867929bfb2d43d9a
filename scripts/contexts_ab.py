"""A/B of the contexts of a spectrum part in ONE process and one build: one sosgpu_create per wavelength, each waiting for its
copy (SOS_SPECTRUM_CONTEXTS_PER_CALL=1), against the default (one asynchronous sosgpu_create_spectrum per part: one staged
copy, one k_ctx_fill launch, no host wait).  The workload is that of profiles/prepare_stages_ab.txt: BASELINE config 5 of
scripts/hyperspectral_bench.py (2496 wavelengths with --every 1), chunk 256, SOS_PREPARE_SEGMENTS=1.  The legs alternate inside
the process: per call 1, batch 1, per call 2, ...  Prints every pass -- wavelengths/s, host ms per wavelength (prepare +
solve_launch + finish of the pass's host phases, as bench.py --workload hyperspectral forms it), the `context:` segments of
_prepare and the time of the context stage -- then per leg the medians and the spread (max - min), and what the rule of the
issue says of them; the same lines go to --out (default profiles/contexts_ab.txt).  Before the passes: the tuples of the two
legs compared bit for bit.  GPU_MAX_HW_QUEUES is taken from the environment, 4 (the runtime's default) without one.  No number
is promised: the per-call leg of the same process is the reference, never the batch leg alone."""
import os, time
os.environ.setdefault("SOS_PREPARE_SEGMENTS", "1")
from statistics import median
import ab_harness as ab
QUEUES = ab.queues("4")
from hyperspectral_bench import spectrum_kwargs

UNIT, JOB = "wavelengths/s", "wavelength"
SWITCH = "SOS_SPECTRUM_CONTEXTS_PER_CALL"
HOST = ("prepare", "solve_launch", "finish")
SEGMENTS = ("context: python", "context: sosgpu_create", "context", "stage: contexts")


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "contexts_ab.txt"))
    ap.add_argument("--every", type=int, default=1)
    ap.set_defaults(runs=3)
    a = ap.parse_args()
    pkg = ab.package()
    rs, L = pkg.run_sos, pkg.capi.lib()
    ab.synthetic_tables(link_aerosols=True)
    kws = spectrum_kwargs(rs, a.every)
    n = len(kws)
    rep = ab.Report(a.out)
    say = rep.say
    say("spectrum: %d wavelengths of BASELINE config 5, chunk %d, GPU_MAX_HW_QUEUES=%s, SOS_PREPARE_SEGMENTS=1" % (n, a.chunk, QUEUES))
    count = {}
    for name in ("sosgpu_create", "sosgpu_create_spectrum"):           # counted at the library
        def counted(*args, _f=getattr(L, name), _n=name):
            count[_n] = count.get(_n, 0) + 1
            return _f(*args)
        setattr(L, name, counted)

    def leg(per_call):
        tm = {}
        count.clear()
        rs.PREPARE_SEGMENTS.clear()
        with ab.switch(SWITCH, per_call):
            t0 = time.perf_counter()
            out = rs.sos_spectrum(kws, timings=tm, chunk=a.chunk)
            dt = time.perf_counter() - t0
        x = {"host": sum(tm.get(k, 0.0) for k in HOST)}
        x.update({k: tm.get(k, 0.0) for k in HOST})
        x.update({k: rs.PREPARE_SEGMENTS.get(k, 0.0) for k in SEGMENTS})
        x["calls"] = (count.get("sosgpu_create", 0), count.get("sosgpu_create_spectrum", 0))
        return n / dt, x, out

    ab.warm_up(rs, kws[0])
    per_call, batch = leg(True)[2], leg(False)[2]       # (the first pass also parses every table file)
    same = ab.tuples_identical(per_call, batch)
    say("warm-up passes done; tuples of the two legs identical, bit for bit: %s" % same)
    del per_call, batch

    def fmt(x):
        return "host %.4f ms per wavelength (%s); segments (ms): %s; sosgpu_create %d, sosgpu_create_spectrum %d" % (
            1e3 * x["host"] / n, " + ".join("%s %.4f" % (k, 1e3 * x[k] / n) for k in HOST),
            ", ".join("%s %.4f" % (k, 1e3 * x[k] / n) for k in SEGMENTS), x["calls"][0], x["calls"][1])

    rates, extras = ab.alternate({"per call": lambda: leg(True)[:2], "batch": lambda: leg(False)[:2]}, a.runs, UNIT, say,
                                 per_pass=fmt)
    ab.phase_medians(extras, n, JOB, say, keys=("host",) + HOST + SEGMENTS)
    host = {k: sorted(1e3 * x["host"] / n for x in v) for k, v in extras.items()}
    for k, v in host.items():
        say("host ms per wavelength  %-8s: %s   median %.4f, max - min %.4f" % (k, " ".join("%.4f" % q for q in v), median(v),
                                                                                   v[-1] - v[0]))
    ref, new, spread = median(host["per call"]), median(host["batch"]), host["per call"][-1] - host["per call"][0]
    say("batch median %.4f against per-call median %.4f: %+.4f ms per wavelength; the per-call leg's own spread is %.4f -- %s" % (
        new, ref, new - ref, spread, "a saving beyond the spread" if ref - new > spread else "NOT resolved"))
    say("tuples of the two legs identical, bit for bit: %s" % same)
    rep.close()


if __name__ == "__main__":
    main()
