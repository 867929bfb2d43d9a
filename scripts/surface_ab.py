"""A/B of the surface matrices of a spectrum in ONE process and one build, on two synthetic spectra whose surface changes with
the wavelength, at the reference's default angle counts (no -ANG.*.NbGauss keyword), molecules only, no gas absorption:
  land   -SURF.Type 7 (Roujean + Maignan, C = 4, index 1.5), (k0, k1, k2) ramped over the wavelengths;
  sea    -SURF.Type 1 at one wind (7 m/s), -SURF.Ind ramped from 1.343 to 1.325.
Legs, both through run_sos.sos_spectrum:
  batch     the default path: one sosgpu_surface_batch per chunk and angle set, queued by the prefetch;
  per_call  SOS_SPECTRUM_SURFACE_PER_CALL=1: every wavelength misses the cache and makes its own synchronous
            sosgpu_glitter / sosgpu_land_surface call.
The legs alternate after a warm-up of both (batch 1, per_call 1, batch 2, ...), each pass between two device synchronisations
and with the surface cache emptied first.  Prints every pass, then the sorted rates, the median and the spread (max - min) of
each leg in wavelengths per second, and writes the same lines to --out."""
import os, time
import ab_harness as ab
QUEUES = ab.queues("4")
import numpy as np

BASE = {"-ANG.Thetas": 35.0, "-AP.HR": 8.0, "-AP.AerHS.HA": 2.0, "-AP.Psurf": 1013.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.0,
        "-AER.Waref": 0.55, "-SOS.IGmax": 100, "-SOS.View": 2, "-SOS.View.Dphi": 120, "-SURF.Alb": 0.0,
        "-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT"}


def spectra(rs, n):
    was = np.linspace(0.40, 0.90, n)
    f = np.linspace(0.0, 1.0, n)

    def kw(user):
        return rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), dict(BASE, **user)), trace=False)

    land = [kw({"-SOS_Main.Wa": float(w), "-SURF.Type": 7, "-SURF.Ind": 1.5, "-SURF.Maignan.C": 4.0,
                "-SURF.Roujean.K0": float(0.05 + 0.30 * x), "-SURF.Roujean.K1": float(0.005 + 0.03 * x),
                "-SURF.Roujean.K2": float(0.10 + 0.30 * x)}) for w, x in zip(was, f)]
    sea = [kw({"-SOS_Main.Wa": float(w), "-SURF.Type": 1, "-SURF.Glitter.Wind": 7.0, "-SURF.Ind": float(1.343 - 0.018 * x)})
           for w, x in zip(was, f)]
    return dict(land=land, sea=sea)


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "surface_ab.txt"))
    ap.add_argument("--n", type=int, default=64, help="wavelengths of each spectrum")
    a = ap.parse_args()
    import torch
    rs = ab.package().run_sos
    rep = ab.Report(a.out)
    say = rep.say

    def leg(kws, name):
        with ab.switch("SOS_SPECTRUM_SURFACE_PER_CALL", name == "per_call"):
            rs._SURF_CACHE.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tuples = rs.sos_spectrum(kws, chunk=a.chunk)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return len(kws) / dt, tuples

    say("GPU_MAX_HW_QUEUES=%s, chunk %d (both legs run in this process under that queue setting; the rates hold for it only)" % (
        QUEUES, a.chunk))
    for which, kws in spectra(rs, a.n).items():
        ab.warm_up(rs, kws[0])
        _, t_b = leg(kws, "batch")
        _, t_p = leg(kws, "per_call")
        say("%s spectrum: %d wavelengths, %d directions; warm-up passes done; the 23-tuples of the two legs identical, bit for "
            "bit: %s" % (which, len(kws), int(t_b[0][0]), ab.tuples_identical(t_b, t_p)))
        del t_b, t_p
        ab.alternate({"%s %s" % (which, name): (lambda name=name: (leg(kws, name)[0], None)) for name in ("batch", "per_call")},
                     a.runs, "wavelengths/s", say)
    rep.close()


if __name__ == "__main__":
    main()
