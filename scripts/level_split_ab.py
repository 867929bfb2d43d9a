"""A/B of the true direct / diffuse split of run_sos.sos_spectrum_levels in ONE process and one build: fluxes=True, split=True
(the profile launches export the untruncated depth rows, one sosgpu_output_depths launch per part, one
sosgpu_level_transmission launch per solved group) against fluxes=True alone, on the spectrum of
scripts/spectrum_levels_bench.py (every --every-th interval of the hyperspectral run) at the first K altitudes of that script.
The legs alternate inside the process: flux 1, split 1, flux 2, ...  Prints every pass with its host phases, then the sorted
rates, the median and the spread (max - min) of each leg, and what the split costs per (wavelength, altitude) job, from the
medians.  The `flux` leg is the `on` leg of scripts/level_flux_ab.py (same spectrum, altitudes and chunk), whose output also
gives what fluxes=True itself costs over fluxes=False.  GPU_MAX_HW_QUEUES is taken from the environment, 16 without one.
--one-leg flux|split: a warm-up pass and a single pass of one leg (for a kernel trace)."""
import time
import ab_harness as ab
QUEUES = ab.queues("16")                                     # (what spectrum_levels_bench sets on import)
import numpy as np
from spectrum_levels_bench import ALTS, spectrum_kwargs

UNIT, JOB = "wavelengths x altitudes/s", "wavelength x altitude"


def main():
    ap = ab.parser()
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--altitudes", type=int, default=4)
    ap.add_argument("--one-leg", choices=["flux", "split"], help="a single pass of one leg (for a kernel trace)")
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
        out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=True, split=name == "split")
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, UNIT)
    ref, rflux = leg("flux")[2]
    got, flux = leg("split")[2]
    same = ab.tuples_identical(ref, got) and ab.tuples_identical([f[:, :5] for f in flux], rflux)
    # columns 5 + 6 restate column 2; row 0 is the standard output, whose column 5 restates element 18 of that altitude's tuple
    worst = max(float(np.max(np.abs(f[:, 5] + f[:, 6] - f[:, 2]) / f[:, 2])) for f in flux)
    e18 = all(f[0, 5] == t[0][18] for f, t in zip(flux, got)) if alts[0] == -1.0 else None
    below = sum(int((f[:, 5] < f[:, 0]).sum()) for f in flux)
    say("warm-up passes done; tuples and first five columns of the two legs identical, bit for bit: %s; columns 5 + 6 against "
        "column 2, worst relative difference %.2e; standard-output row equal to element 18: %s; rows with the true direct beam "
        "below the truncated one: %d of %d" % (same, worst, e18, below, njobs))
    del ref, got, flux, rflux
    rates, phases = ab.alternate({name: (lambda name=name: leg(name)[:2]) for name in ("flux", "split")}, a.runs, UNIT, say,
                                 per_pass=ab.host_phases(njobs, JOB))
    ab.job_cost(rates, "flux", "split", "the split", JOB, say)
    ab.phase_medians(phases, njobs, JOB, say)
    rep.close()


if __name__ == "__main__":
    main()
