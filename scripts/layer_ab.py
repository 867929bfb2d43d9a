"""A/B of the aerosol-layer profile (-AP.AerProfile.Type 2) of a spectrum in ONE process and one build: the profile made on the
host and uploaded per wavelength (SOS_LAYER_PROFILE_HOST=1: geometry.profile_layer, synth.rescale_profile, upload_bins; every
wavelength then gets its own solve) against the default (one sosgpu_profile_layer_spectrum launch per part, the solves of
wavelengths with equal angle sets grouped).  The spectrum: every --every-th interval of the hyperspectral run
(scripts/hyperspectral_bench.py: its angle counts and surface), no gas, a layer between 1 and 3 km whose aerosol optical
thickness varies with the wavelength so that the level count runs from about 260 down to 40; the aerosol is a given
Henyey-Greenstein expansion, so that no Mie step stands in front of the profiles.  The legs alternate inside the process: host 1,
device 1, host 2, ...  Prints every pass with its host phases and its solve launches, then the sorted rates, the median and the
spread (max - min) of each leg; the same lines go to --out (default profiles/layer_profile_ab.txt).  Before the passes: the tuples
of the two legs compared bit for bit.  GPU_MAX_HW_QUEUES is taken from the environment, 4 (the runtime's default) without one.  No
rate is promised and none decides anything."""
import os, time
import ab_harness as ab
QUEUES = ab.queues("4")
from hyperspectral_bench import spectrum_kwargs

UNIT, JOB = "wavelengths/s", "wavelength"
SWITCH = "SOS_LAYER_PROFILE_HOST"
SOLVES = ("sosgpu_os_solve", "sosgpu_os_solve_multi")


def layer_spectrum(pkg, every):
    """(keyword sets, aerosol expansions): tr + ta runs linearly from 1.3 at the first (shortest) wavelength to 0.2 at the last."""
    rs = pkg.run_sos
    kws = spectrum_kwargs(rs, every)
    al, be, ga, ze = pkg.synth.hg_phase(rs._angle_counts(kws[0])[2], 0.7)
    aer = dict(alpha=al, beta=be, gamma=ga, zeta=ze, piz=0.95, piztr=0.95, a_tronc=0.0)
    out = []
    for k, kw in enumerate(kws):
        ttot = 1.3 - 1.1 * k / max(1, len(kws) - 1)
        tr = rs.rayleigh_optical_thickness(kw["wa_simu"], kw["psurf"])
        out.append(dict(kw, absprofil=7, iprofil=2, zmin=1.0, zmax=3.0, aot_ref=float(ttot - tr)))
    return out, [aer] * len(out)


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "layer_profile_ab.txt"))
    ap.add_argument("--every", type=int, default=10)
    ap.set_defaults(runs=3)
    a = ap.parse_args()
    pkg = ab.package()
    rs, L = pkg.run_sos, pkg.capi.lib()
    kws, aers = layer_spectrum(pkg, a.every)
    nts = [pkg.geometry.layer_grid(rs.rayleigh_optical_thickness(kw["wa_simu"], kw["psurf"]), kw["hr"], kw["aot_ref"], 1.0, 3.0)[0]
           for kw in kws]
    rep = ab.Report(a.out)
    say = rep.say
    say("spectrum: %d layer wavelengths (1-3 km), NT %d..%d, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), min(nts), max(nts), a.chunk, QUEUES))
    count = {}
    for name in SOLVES:                                      # solve launches, counted at the library
        def counted(*args, _f=getattr(L, name), _n=name):
            count[_n] = count.get(_n, 0) + 1
            return _f(*args)
        setattr(L, name, counted)

    def leg(host):
        tm = {}
        count.clear()
        with ab.switch(SWITCH, host):
            t0 = time.perf_counter()
            out = rs.sos_spectrum(kws, aer_phases=aers, timings=tm, chunk=a.chunk)
            dt = time.perf_counter() - t0
        tm = {k: tm.get(k, 0.0) for k in ("prepare", "solve_launch", "wait", "finish")}
        tm["solve launches"] = sum(count.values())
        return len(kws) / dt, tm, out

    rs.sos_proc(aer_phase=aers[0], **kws[0])                 # library load, surface matrices, caches
    host, dev = leg(True)[2], leg(False)[2]
    say("warm-up passes done; tuples of the two legs identical, bit for bit: %s" % ab.tuples_identical(host, dev))
    del host, dev

    def fmt(tm):
        return "host phases per wavelength (ms): %s; solve launches %d" % (
            ", ".join("%s %.4f" % (q, 1e3 * v / len(kws)) for q, v in tm.items() if q != "solve launches"), tm["solve launches"])

    rates, phases = ab.alternate({"host profile": lambda: leg(True)[:2], "device profile": lambda: leg(False)[:2]}, a.runs, UNIT,
                                 say, per_pass=fmt)
    ab.job_cost(rates, "host profile", "device profile", "the device profile (negative: a saving)", JOB, say)
    ab.phase_medians(phases, len(kws), JOB, say, keys=("prepare", "solve_launch", "wait", "finish"))
    rep.close()


if __name__ == "__main__":
    main()
