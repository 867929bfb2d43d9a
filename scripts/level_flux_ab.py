"""A/B of the per-altitude fluxes of run_sos.sos_spectrum_levels in ONE process and one build: fluxes=True (one
sosgpu_level_flux_spectrum launch per chunk, the flux rows downloaded behind the recompositions) against fluxes=False, on the
spectrum of scripts/spectrum_levels_bench.py (every --every-th interval of the hyperspectral run) at the first K altitudes of
that script.  The legs alternate inside the process: off 1, on 1, off 2, ...  Prints every pass with its host phases, then the
sorted rates, the median and the spread (max - min) of each leg, and the medians of the fluxes and trphi phases per job.
GPU_MAX_HW_QUEUES is taken from the environment, 16 without one (the runs of profiles/level_flux.txt: 4).
--one-leg on|off: a warm-up pass and a single pass of one leg (for a kernel trace)."""
import time
import ab_harness as ab
QUEUES = ab.queues("16")                                     # (what spectrum_levels_bench sets on import)
from spectrum_levels_bench import ALTS, spectrum_kwargs

UNIT, JOB = "wavelengths x altitudes/s", "wavelength x altitude"


def main():
    ap = ab.parser()
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--altitudes", type=int, default=4)
    ap.add_argument("--one-leg", choices=["on", "off"], help="a single pass of one leg (for a kernel trace)")
    a = ap.parse_args()
    rs = ab.package().run_sos
    ab.synthetic_tables()
    kws = spectrum_kwargs(rs, a.every)
    alts = ALTS[:a.altitudes]
    njobs = len(kws) * len(alts)
    rep = ab.Report(a.out)
    say = rep.say
    say("spectrum: %d wavelengths, altitudes %s, chunk %d (%d wavelengths per chunk), GPU_MAX_HW_QUEUES=%s" % (
        len(kws), alts, a.chunk, max(1, a.chunk // len(alts)), QUEUES))

    def leg(name):
        tm = {}
        t0 = time.perf_counter()
        out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=name == "on")
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, UNIT)
    ref = leg("off")[2]
    got, flux = leg("on")[2]
    same = ab.tuples_identical(ref, got)
    # row 0 is the standard output: its total and up-going columns restate elements 20 and 21 of that altitude's tuple
    worst = max(max(abs(f[0, 2] / t[0][20] - 1), abs(f[0, 3] / t[0][21] - 1)) for f, t in zip(flux, got)) if alts[0] == -1.0 else -1.0
    say("warm-up passes done; 23-tuples of the two legs identical, bit for bit: %s; standard-output row against elements 20 / 21, "
        "worst relative difference %.2e" % (same, worst))
    del ref, got, flux
    _, phases = ab.alternate({"fluxes " + name: (lambda name=name: leg(name)[:2]) for name in ("off", "on")}, a.runs, UNIT, say,
                             per_pass=ab.host_phases(njobs, JOB))
    ab.phase_medians(phases, njobs, JOB, say, keys=("fluxes", "trphi"))
    rep.close()


if __name__ == "__main__":
    main()
