"""A/B of the azimuth recomposition of run_sos.sos_spectrum / sos_spectrum_levels in ONE process and one build: the batched
default (sosgpu_trphi_spectrum, one launch per chunk) against SOS_SPECTRUM_TRPHI_PER_CALL=1 (one sosgpu_trphi launch per
wavelength and altitude), on the spectrum of scripts/hyperspectral_bench.py (BASELINE config 5).  --altitudes 0: sos_spectrum;
K > 0: sos_spectrum_levels at the first K altitudes of scripts/spectrum_levels_bench.py.  The switch is read by every pass, so
the legs alternate inside the process: batched 1, per call 1, batched 2, ...  Prints every pass with its host phases, then the
sorted rates, the median and the spread (max - min) of each leg, and the medians of the trphi and finish phases."""
import time
import ab_harness as ab
QUEUES = ab.queues("16")                                     # (what hyperspectral_bench sets on import)
import hyperspectral_bench as hb
from spectrum_levels_bench import ALTS

UNIT, JOB = "wavelengths x altitudes/s", "wavelength x altitude"


def main():
    ap = ab.parser()
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--altitudes", type=int, default=0, help="0: sos_spectrum; K: sos_spectrum_levels at K altitudes")
    ap.add_argument("--one-leg", choices=["batched", "per_call"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    rs = ab.package().run_sos
    ab.synthetic_tables(link_aerosols=True)
    kws = hb.spectrum_kwargs(rs, a.every)
    alts = ALTS[:a.altitudes]
    njobs = len(kws) * max(1, len(alts))
    rep = ab.Report(a.out)
    say = rep.say
    say("spectrum: %d wavelengths, altitudes %s, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), alts or "(sos_spectrum)", a.chunk, QUEUES))

    def leg(name):
        with ab.switch("SOS_SPECTRUM_TRPHI_PER_CALL", name == "per_call"):
            tm = {}
            t0 = time.perf_counter()
            if alts:
                out = [t for r in rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk) for t in r]
            else:
                out = rs.sos_spectrum(kws, timings=tm, chunk=a.chunk)
            dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, UNIT)
    ref = leg("batched")[2]
    say("warm-up passes done; outputs of the two legs identical, bit for bit: %s" % ab.tuples_identical(ref, leg("per_call")[2]))
    del ref
    _, phases = ab.alternate({name: (lambda name=name: leg(name)[:2]) for name in ("batched", "per_call")}, a.runs, UNIT, say,
                             per_pass=ab.host_phases(njobs, JOB))
    ab.phase_medians(phases, njobs, JOB, say, keys=("trphi", "finish"))
    rep.close()


if __name__ == "__main__":
    main()
