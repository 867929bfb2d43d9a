"""A/B of the diffuse transmissions of a spectrum in ONE process and one build, on the wavelengths of
scripts/hyperspectral_bench.py (BASELINE config 5; --every k takes every k-th interval, default 16: 156 wavelengths):
  file   every call asks for the -SOS.Trans option and goes through run_sos.sos_spectrum -- the per-direction path: such a call
         leaves the batched stages and makes one order-0 context per direction (SosContext.diffuse_transmissions).  No result
         directory is given, so nothing is written: the leg pays for the transmissions, not for files;
  many   run_sos.sos_spectrum(..., transmissions=True): one order-0 solve per part and direction count
         (solver.diffuse_transmissions_many, sosgpu_trans_spectrum), the calls staying in the batched stages.
The legs alternate after a warm-up of both: many 1, file 1, many 2, ...  Prints every pass, then the sorted rates, the median
and the spread (max - min) of each leg in wavelengths per second, and writes the same lines to --out."""
import argparse, importlib, os, statistics, sys, tempfile, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_ckd
import hyperspectral_bench as hb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trans_ab.txt"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    hb.link_aerosol_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    kws = [dict(kw, fictrans="NO_OUTPUT") for kw in hb.spectrum_kwargs(rs, a.every)]
    kws_file = [dict(kw, fictrans="SOS_Transm.txt") for kw in kws]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def leg(name):
        t0 = time.perf_counter()
        if name == "many":
            tuples, trans = rs.sos_spectrum(kws, chunk=a.chunk, transmissions=True)
        else:
            tuples, trans = rs.sos_spectrum(kws_file, chunk=a.chunk), None
        dt = time.perf_counter() - t0
        return len(kws) / dt, tuples, trans

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    _, t_many, trans = leg("many")
    _, t_file, _ = leg("file")
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for p, q in zip(t_many, t_file) for x, y in zip(p, q))
    n = int(t_many[0][0])
    say("spectrum: %d wavelengths (every %d-th interval), %d directions, chunk %d, GPU_MAX_HW_QUEUES=%s" % (
        len(kws), a.every, n, a.chunk, os.environ.get("GPU_MAX_HW_QUEUES")))
    say("(both legs run in this process under that queue setting; the rates hold for it only)")
    say("warm-up passes done; the 23-tuples of the two legs identical, bit for bit: %s; diffuse transmittance of the first "
        "wavelength, TOA -> surface %.6f, surface -> TOA at the first direction %.6f" % (
            same, trans[0]["t_dif_down"], trans[0]["t_dif_up"][0]))
    del t_many, t_file, trans
    rates = {"many": [], "file": []}
    for k in range(a.runs):
        for name in ("many", "file"):
            r = leg(name)[0]
            rates[name].append(r)
            say("[%s %d] %8.1f wavelengths/s" % (name, k + 1, r))
    for name, v in rates.items():
        say("wavelengths/s  %-5s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
