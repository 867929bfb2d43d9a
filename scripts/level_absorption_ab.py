"""A/B of the actinic flux / absorbed power of run_sos.sos_spectrum_levels in ONE process and one build: fluxes=True,
absorption=True (the solves keep their per-bin records, one sosgpu_level_absorption launch per solved group, its block comes
down with the flux pairs) against fluxes=True alone, on the spectrum of scripts/spectrum_levels_bench.py (every --every-th
interval of the hyperspectral run) at the first K altitudes of that script.  The legs alternate inside the process: flux 1,
absorb 1, flux 2, ...  Prints every pass with its host phases, then the sorted rates, the median and the spread (max - min) of
each leg, and what the keyword costs per (wavelength, altitude) job, from the medians; the same lines go to --out (default
profiles/level_absorption_ab.txt).  The `flux` leg is the `on` leg of scripts/level_flux_ab.py (same spectrum, altitudes and
chunk).  GPU_MAX_HW_QUEUES is taken from the environment, 16 without one.  The feature is opt-in: no rate decides anything.
--one-leg flux|absorb: a warm-up pass and a single pass of one leg (for a kernel trace)."""
import os, time
import ab_harness as ab
QUEUES = ab.queues("16")                                     # (what spectrum_levels_bench sets on import)
import numpy as np
from spectrum_levels_bench import ALTS, spectrum_kwargs

UNIT, JOB = "wavelengths x altitudes/s", "wavelength x altitude"


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "level_absorption_ab.txt"))
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--altitudes", type=int, default=4)
    ap.add_argument("--one-leg", choices=["flux", "absorb"], help="a single pass of one leg (for a kernel trace)")
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
        out = rs.sos_spectrum_levels(alts, kws, timings=tm, chunk=a.chunk, fluxes=True, absorption=name == "absorb")
        dt = time.perf_counter() - t0
        return njobs / dt, tm, out

    ab.warm_up(rs, kws[0])
    if a.one_leg:
        return ab.one_pass(lambda: leg(a.one_leg), a.one_leg, UNIT)
    ref, rflux = leg("flux")[2]
    got, flux, absorb = leg("absorb")[2]
    same = ab.tuples_identical(ref, got) and ab.tuples_identical(flux, rflux)
    rows = np.array([ab[k] for ab in absorb for k, z in enumerate(alts) if z != -1.0])
    nan_rows = all(np.isnan(ab[k]).all() for ab in absorb for k, z in enumerate(alts) if z == -1.0)
    say("warm-up passes done; tuples and flux rows of the two legs identical, bit for bit: %s; standard-output rows NaN: %s; "
        "absorbed_per_km over the %d interior rows: min %.3e median %.3e max %.3e; actinic_tot: min %.4f max %.4f" % (
            same, nan_rows, len(rows), rows[:, 4].min(), float(np.median(rows[:, 4])), rows[:, 4].max(), rows[:, 3].min(),
            rows[:, 3].max()))
    del ref, got, flux, rflux, absorb
    rates, phases = ab.alternate({name: (lambda name=name: leg(name)[:2]) for name in ("flux", "absorb")}, a.runs, UNIT, say,
                                 per_pass=ab.host_phases(njobs, JOB))
    ab.job_cost(rates, "flux", "absorb", "absorption=True", JOB, say)
    ab.phase_medians(phases, njobs, JOB, say)
    rep.close()


if __name__ == "__main__":
    main()
