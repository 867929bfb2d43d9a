"""A/B of the spherical albedo of a spectrum in ONE process and one build, on the wavelengths of
scripts/hyperspectral_bench.py (BASELINE config 5; --every k takes every k-th interval, default 16: 156 wavelengths):
  trans    run_sos.sos_spectrum(..., transmissions=True): the diffuse transmissions, one order-0 solve per part and direction
           count (solver.diffuse_transmissions_many);
  albedo   the same with spherical_albedo=True: one more such solve on the mirrored profiles, minus the weight-0 directions
           (solver.spherical_albedo_many), and one band-sum launch per group (solver.albedo_band).
The legs alternate after a warm-up of both: trans 1, albedo 1, trans 2, ...  Prints every pass, then the sorted rates, the
median and the spread (max - min) of each leg in wavelengths per second, and writes the same lines to --out with the commit
and the queue count."""
import argparse, importlib, os, statistics, subprocess, sys, tempfile, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_ckd
import hyperspectral_bench as hb


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--commit", default=None, help="the commit to state (default: git rev-parse of this tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "albedo_ab.txt"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    hb.link_aerosol_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    kws = [dict(kw, fictrans="NO_OUTPUT") for kw in hb.spectrum_kwargs(rs, a.every)]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def leg(name):
        t0 = time.perf_counter()
        tuples, trans = rs.sos_spectrum(kws, chunk=a.chunk, transmissions=True, spherical_albedo=name == "albedo")
        dt = time.perf_counter() - t0
        return len(kws) / dt, tuples, trans

    rs.sos_proc(**kws[0]); torch.cuda.synchronize()
    _, t_trans, e_trans = leg("trans")
    _, t_alb, e_alb = leg("albedo")
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for p, q in zip(t_trans, t_alb) for x, y in zip(p, q)) and \
        all(np.array_equal(np.asarray(p[k]), np.asarray(q[k])) for p, q in zip(e_trans, e_alb) for k in p)
    n = int(t_trans[0][0])
    say("commit %s (working tree of the spherical-albedo change on top of it), GPU_MAX_HW_QUEUES=%s" % (
        a.commit or commit(), os.environ.get("GPU_MAX_HW_QUEUES")))
    say("spectrum: %d wavelengths (every %d-th interval), %d directions, chunk %d" % (len(kws), a.every, n, a.chunk))
    say("(both legs run in this process under that queue setting; the rates hold for it only)")
    s = np.array([e["s_alb"] for e in e_alb])
    say("warm-up passes done; the 23-tuples and the transmission entries of the two legs identical, bit for bit: %s; s_alb of the "
        "first wavelength %.6f, over the spectrum min %.6f max %.6f" % (same, s[0], s.min(), s.max()))
    del t_trans, t_alb, e_trans, e_alb
    rates = {"trans": [], "albedo": []}
    for k in range(a.runs):
        for name in ("trans", "albedo"):
            r = leg(name)[0]
            rates[name].append(r)
            say("[%s %d] %8.1f wavelengths/s" % (name, k + 1, r))
    for name, v in rates.items():
        say("wavelengths/s  %-6s: %s   median %.1f, max - min %.1f" % (
            name, " ".join("%.1f" % x for x in sorted(v)), statistics.median(v), max(v) - min(v)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
