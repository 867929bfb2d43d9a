"""A/B of the irradiance rows of a spectrum in ONE process and one build: run_sos.sos_spectrum_levels(fluxes=True, split=True,
absorption=True) -- every Fourier order solved, K aggregates, the flux, transmission and absorption launches, one azimuth
recomposition and two (7, 361, 81) tables per job -- against run_sos.sos_spectrum_irradiances(split=True, absorption=True) --
order-0 contexts and solves, ONE sosgpu_level_irradiance launch per solved group, no recomposition and no table -- on the
spectrum of scripts/level_absorption_ab.py (every --every-th interval of the hyperspectral run, the first K altitudes of
scripts/spectrum_levels_bench.py).  The legs alternate inside the process: levels 1, irradiance 1, levels 2, ...  Prints every
pass with its host phases, then the sorted rates, the median and the spread (max - min) of each leg and the cost per
(wavelength, altitude) job from the medians; the same lines go to --out (default profiles/irradiance_ab.txt).  Before the
passes: the rows of the two legs compared (equal bits, or the worst relative deviation of the diffuse-flux columns of the
bands).  GPU_MAX_HW_QUEUES is taken from the environment, 16 without one.  No rate is promised and none decides anything.
--one-leg levels|irradiance: a warm-up pass and a single pass of one leg (for a kernel trace)."""
import os, time
import ab_harness as ab
QUEUES = ab.queues("16")                                     # (what spectrum_levels_bench sets on import)
import numpy as np
from spectrum_levels_bench import ALTS, spectrum_kwargs

UNIT, JOB = "wavelengths x altitudes/s", "wavelength x altitude"


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "irradiance_ab.txt"))
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--altitudes", type=int, default=4)
    ap.add_argument("--one-leg", choices=["levels", "irradiance"], help="a single pass of one leg (for a kernel trace)")
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
        if name == "levels":
            out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=True, split=True, absorption=True)[1:]
        else:
            out = rs.sos_spectrum_irradiances(alts, kws, timings=tm, chunk=a.chunk, split=True, absorption=True)
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, UNIT)
    (rflux, rabsorb), (flux, absorb) = leg("levels")[2], leg("irradiance")[2]
    same_absorb = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(absorb, rabsorb))
    exact = sum(bool(np.array_equal(x, y)) for x, y in zip(flux, rflux))
    worst = max(float(np.abs(x / y - 1).max()) for x, y in zip(flux, rflux))
    say("warm-up passes done; absorption rows of the two legs identical, bit for bit: %s; flux rows identical in %d of %d calls, "
        "worst relative deviation of a flux column %.3e" % (same_absorb, exact, len(flux), worst))
    del rflux, rabsorb, flux, absorb
    rates, phases = ab.alternate({name: (lambda name=name: leg(name)[:2]) for name in ("levels", "irradiance")}, a.runs, UNIT,
                                 say, per_pass=ab.host_phases(njobs, JOB))
    ab.job_cost(rates, "levels", "irradiance", "the irradiance pass (negative: a saving)", JOB, say)
    ab.phase_medians(phases, njobs, JOB, say)
    rep.close()


if __name__ == "__main__":
    main()
