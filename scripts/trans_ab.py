"""A/B of the diffuse transmissions of a spectrum in ONE process and one build, on the wavelengths of
scripts/hyperspectral_bench.py (BASELINE config 5; --every k takes every k-th interval, default 16: 156 wavelengths):
  file   every call asks for the -SOS.Trans option and goes through run_sos.sos_spectrum -- the per-direction path: such a call
         leaves the batched stages and makes one order-0 context per direction (SosContext.diffuse_transmissions).  No result
         directory is given, so nothing is written: the leg pays for the transmissions, not for files;
  many   run_sos.sos_spectrum(..., transmissions=True): one order-0 solve per part and direction count
         (solver.diffuse_transmissions_many, sosgpu_trans_spectrum), the calls staying in the batched stages.
The legs alternate after a warm-up of both: many 1, file 1, many 2, ...  Prints every pass, then the sorted rates, the median
and the spread (max - min) of each leg in wavelengths per second, and writes the same lines to --out."""
import os, time
import ab_harness as ab
QUEUES = ab.queues("4")
import hyperspectral_bench as hb


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "trans_ab.txt"))
    ap.add_argument("--every", type=int, default=16)
    a = ap.parse_args()
    rs = ab.package().run_sos
    ab.synthetic_tables(link_aerosols=True)
    kws = [dict(kw, fictrans="NO_OUTPUT") for kw in hb.spectrum_kwargs(rs, a.every)]
    kws_file = [dict(kw, fictrans="SOS_Transm.txt") for kw in kws]
    rep = ab.Report(a.out)
    say = rep.say

    def leg(name):
        t0 = time.perf_counter()
        if name == "many":
            tuples, trans = rs.sos_spectrum(kws, chunk=a.chunk, transmissions=True)
        else:
            tuples, trans = rs.sos_spectrum(kws_file, chunk=a.chunk), None
        dt = time.perf_counter() - t0
        return len(kws) / dt, tuples, trans

    ab.warm_up(rs, kws[0])
    _, t_many, trans = leg("many")
    _, t_file, _ = leg("file")
    same = ab.tuples_identical(t_many, t_file)
    n = int(t_many[0][0])
    say("spectrum: %d wavelengths (every %d-th interval), %d directions, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), a.every, n, a.chunk, QUEUES))
    say("(both legs run in this process under that queue setting; the rates hold for it only)")
    say("warm-up passes done; the 23-tuples of the two legs identical, bit for bit: %s; diffuse transmittance of the first "
        "wavelength, TOA -> surface %.6f, surface -> TOA at the first direction %.6f" % (
            same, trans[0]["t_dif_down"], trans[0]["t_dif_up"][0]))
    del t_many, t_file, trans
    ab.alternate({name: (lambda name=name: (leg(name)[0], None)) for name in ("many", "file")}, a.runs, "wavelengths/s", say)
    rep.close()


if __name__ == "__main__":
    main()
