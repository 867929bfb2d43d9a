"""Several output altitudes: K single-altitude solves against ONE K-slot solve (sosgpu_os_solve_levels), K = 1, 2, 4, 8, timed
with device events, and the records checked equal.  Cases: N = 41 at NT = 30 (LDS-resident field) and N = 25 / 41 on level grids
of reference size, NT = 120 and 300 (streamed field; order-parallel form for the small band, one workgroup per bin for the large
batch).  Usage: python scripts/levels_bench.py [reps]   (profiles/levels_bench.txt holds a run on the MI355X)"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("radiativetransfer-sos_amd")
S = pkg.synth
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ALTS = [3.0, 1.0, 8.0, 0.5, 12.0, 2.0, 20.0, 5.0]
CASES = [("N=41 NT=30 (LDS)", 40, 30, 4096), ("N=25 NT=120 (streamed)", 24, 120, 1024),
         ("N=41 NT=120 (streamed)", 40, 120, 1024), ("N=41 NT=300 (streamed)", 40, 300, 256),
         ("N=41 NT=120 band of 25 bins (order-parallel)", 40, 120, 25)]


def timed(fn):
    ms = []
    for _ in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[1:]))


print("levels_bench: K single-altitude solves vs one K-slot solve (ms, median of %d)" % REPS)
print("%-46s %2s %10s %10s %7s %9s" % ("case", "K", "K x single", "K-slot", "ratio", "vs 1 alt"))
for label, ng, nt, nb in CASES:
    mu, w, n0 = S.gauss_angles(ng, 35.0)
    os_nb = 80
    al, be, ga, ze = S.hg_phase(os_nb, 0.75)
    b = S.ckd_bins(nb, nt, seed=1234)
    h, x, y, iborm = S.rescale_profile(b["h"], b["xdel"], b["ydel"], 0.0, 0.95, 0.95, os_nb)
    cx = pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=iborm, ro=0.1)
    bins = cx.upload_bins(h, x, y, zprof=b["zprof"])
    one_ms = None
    for K in (1, 2, 4, 8):
        alts = ALTS[:K]
        lv = cx.output_levels(bins, alts)
        singles = [dict(bins, jout=lv["jout"][k].contiguous(), zz=lv["zz"][k].contiguous()) for k in range(K)]
        outs = [cx.alloc_outputs(nb) for _ in range(K)]
        lout = cx.alloc_outputs(nb)
        lout["rec"] = torch.zeros((K, nb, cx.smax + 1, 3, cx.w), dtype=torch.float64, device=cx.device)
        t_single = timed(lambda: [cx.solve(singles[k], outs[k]) for k in range(K)])
        t_levels = timed(lambda: cx.solve_levels(bins, lv, lout))
        for k in range(K):
            assert torch.equal(outs[k]["rec"], lout["rec"][k]) and torch.equal(outs[k]["norders"], lout["norders"]), (label, K, k)
        if K == 1:
            one_ms = t_single
        print("%-46s %2d %10.2f %10.2f %7.3f %9.3f" % (label, K, t_single, t_levels, t_levels / t_single, t_levels / one_ms),
              flush=True)
    cx.close()
print("ratio = K-slot / (K single solves); vs 1 alt = K-slot / one single-altitude solve; records equal bit for bit")
