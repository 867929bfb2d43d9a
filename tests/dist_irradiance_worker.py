"""Worker of tests/test_irradiance_dist.py: run_sos.sos_spectrum_irradiances under torch.distributed (two ranks on cuda:0, gloo).
The wavelengths are dealt whole to the ranks and the rows gathered, so every rank returns the rows and the weighted sums of one
process; then a spectrum with one refused call must make every rank raise SosProcError (no rank left waiting in the gather)."""
import argparse
import json
import os

import torch
import torch.distributed as dist

from dist_launch import rank_begin, rank_end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    import test_irradiance_dist as tid
    kws = tid.dist_kws(rs, os.path.join(os.path.dirname(a.out), "rank%d" % rank))
    mine = [int(i) for i in pkg.dist.balanced_shards(rs.spectrum_costs(kws), world)[rank]]
    flux, absorb = rs.sos_spectrum_irradiances(tid.ALTS, kws, split=True, absorption=True)
    torch.cuda.synchronize()
    assert all(x is not None and x.shape == (len(tid.ALTS), 7) for x in flux) and all(x is not None for x in absorb)
    pflux, pabsorb = rs.sos_spectrum_irradiances(tid.ALTS, kws, split=True, absorption=True, gather=False)
    partial_ok = ([i for i, x in enumerate(pflux) if x is not None] == mine and
                  all(tid.rows_digest([pflux[i]], [pabsorb[i]]) == tid.rows_digest([flux[i]], [absorb[i]]) for i in mine))
    sums = rs.sos_spectrum_irradiances(tid.ALTS, kws, split=True, absorption=True, weights=tid.weights(len(kws)), gather=False)
    # call 3 refused (-SURF.Type 6 without its surface index): every rank raises, whichever owns it
    bad = list(kws)
    bad[3] = dict(kws[3], isurf=6)
    raised, msg = False, ""
    try:
        rs.sos_spectrum_irradiances(tid.ALTS, bad, split=True, absorption=True)
    except rs.SosProcError as e:
        raised, msg = True, str(e)
    dig, sdig, own, ok, rz, ms = ([None] * world for _ in range(6))
    dist.all_gather_object(dig, tid.rows_digest(flux, absorb))
    dist.all_gather_object(sdig, tid.rows_digest([sums[0]], [sums[1]]))
    dist.all_gather_object(own, mine)
    dist.all_gather_object(ok, bool(partial_ok))
    dist.all_gather_object(rz, raised)
    dist.all_gather_object(ms, msg)
    if rank == 0:
        with open(a.out, "w") as f:
            json.dump({"world": world, "n": len(kws), "digests": dig, "sum_digests": sdig, "owners": own, "partial_ok": ok,
                       "raised": rz, "messages": ms}, f)
    rank_end()


if __name__ == "__main__":
    main()
