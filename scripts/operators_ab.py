"""A/B of the operator stage of run_sos.sos_spectrum in ONE process and one build: the batched default
(sosgpu_noyaux_spectrum, at most five launches per part) against SOS_SPECTRUM_OPERATORS_PER_CALL=1 (four or five launches per
wavelength on its side stream), on the spectrum of scripts/hyperspectral_bench.py (BASELINE config 5).  The switch is read by
every pass, so the legs alternate inside the process: batched 1, per call 1, batched 2, ...  Prints every pass, then the sorted
rates, the median and the spread (max - min) of each leg.  The number of hardware queues is the process's GPU_MAX_HW_QUEUES
(unlike hyperspectral_bench.py this script does not set it: ab_harness.queues(None))."""
import time
import ab_harness as ab
QUEUES = ab.queues(None)                                     # (not the 16 that hyperspectral_bench sets on import either)
import hyperspectral_bench as hb


def main():
    ap = ab.parser()
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--aer-model", choices=sorted(hb.AER_MODELS), default="lnd")
    ap.add_argument("--surface", choices=["maignan", "lambert"], default="maignan",
                    help="maignan: the keywords of hyperspectral_bench (surface matrices, five launches); lambert: -SURF.Type 0")
    ap.add_argument("--one-leg", choices=["batched", "per_call"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    rs = ab.package().run_sos
    ab.synthetic_tables(link_aerosols=True)
    if a.surface == "lambert":
        hb.USER.update({"-SURF.Type": 0, "-SURF.Alb": 0.1})
    kws = hb.spectrum_kwargs(rs, a.every, a.aer_model)
    rep = ab.Report(a.out)
    say = rep.say
    say("spectrum: %d wavelengths, surface %s, aerosol model %s, GPU_MAX_HW_QUEUES=%s" % (len(kws), a.surface, a.aer_model, QUEUES))

    def leg(name):
        with ab.switch("SOS_SPECTRUM_OPERATORS_PER_CALL", name == "per_call"):
            tm = {}
            t0 = time.perf_counter()
            out = rs.sos_spectrum(kws, timings=tm, chunk=a.chunk)
            dt = time.perf_counter() - t0
        return len(kws) / dt, tm, out

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, "wavelengths/s")
    ref = leg("batched")[2]
    say("warm-up passes done; outputs of the two legs identical, bit for bit: %s" % ab.tuples_identical(ref, leg("per_call")[2]))
    ab.alternate({name: (lambda name=name: leg(name)[:2]) for name in ("batched", "per_call")}, a.runs, "wavelengths/s", say,
                 per_pass=ab.host_phases(len(kws), "wavelength"))
    rep.close()


if __name__ == "__main__":
    main()
