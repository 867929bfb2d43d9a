"""A/B of the spherical albedo of a spectrum in ONE process and one build, on the wavelengths of
scripts/hyperspectral_bench.py (BASELINE config 5; --every k takes every k-th interval, default 16: 156 wavelengths):
  trans    run_sos.sos_spectrum(..., transmissions=True): the diffuse transmissions, one order-0 solve per part and direction
           count (solver.diffuse_transmissions_many);
  albedo   the same with spherical_albedo=True: one more such solve on the mirrored profiles, minus the weight-0 directions
           (solver.spherical_albedo_many), and one band-sum launch per group (solver.albedo_band).
The legs alternate after a warm-up of both: trans 1, albedo 1, trans 2, ...  Prints every pass, then the sorted rates, the
median and the spread (max - min) of each leg in wavelengths per second, and writes the same lines to --out with the commit
and the queue count."""
import os, subprocess, time
import ab_harness as ab
QUEUES = ab.queues("4")
import numpy as np
import hyperspectral_bench as hb


def commit():
    try:
        return subprocess.check_output(["git", "-C", ab.ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "albedo_ab.txt"))
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--commit", default=None, help="the commit to state (default: git rev-parse of this tree)")
    a = ap.parse_args()
    rs = ab.package().run_sos
    ab.synthetic_tables(link_aerosols=True)
    kws = [dict(kw, fictrans="NO_OUTPUT") for kw in hb.spectrum_kwargs(rs, a.every)]
    rep = ab.Report(a.out)
    say = rep.say

    def leg(name):
        t0 = time.perf_counter()
        tuples, trans = rs.sos_spectrum(kws, chunk=a.chunk, transmissions=True, spherical_albedo=name == "albedo")
        dt = time.perf_counter() - t0
        return len(kws) / dt, tuples, trans

    ab.warm_up(rs, kws[0])
    _, t_trans, e_trans = leg("trans")
    _, t_alb, e_alb = leg("albedo")
    same = ab.tuples_identical(t_trans, t_alb) and \
        all(ab.tuples_identical(p[k], q[k]) for p, q in zip(e_trans, e_alb) for k in p)
    n = int(t_trans[0][0])
    say("commit %s (working tree of the spherical-albedo change on top of it), GPU_MAX_HW_QUEUES=%s" % (a.commit or commit(), QUEUES))
    say("spectrum: %d wavelengths (every %d-th interval), %d directions, chunk %d" % (len(kws), a.every, n, a.chunk))
    say("(both legs run in this process under that queue setting; the rates hold for it only)")
    s = np.array([e["s_alb"] for e in e_alb])
    say("warm-up passes done; the 23-tuples and the transmission entries of the two legs identical, bit for bit: %s; s_alb of the "
        "first wavelength %.6f, over the spectrum min %.6f max %.6f" % (same, s[0], s.min(), s.max()))
    del t_trans, t_alb, e_trans, e_alb
    ab.alternate({name: (lambda name=name: (leg(name)[0], None)) for name in ("trans", "albedo")}, a.runs, "wavelengths/s", say)
    rep.close()


if __name__ == "__main__":
    main()
