"""Worker of tests/test_spectrum_levels.py::test_sos_spectrum_levels_two_ranks_on_one_gpu: run_sos.sos_spectrum_levels under
torch.distributed (two ranks on cuda:0, gloo).  The wavelengths are dealt to the ranks, the K tuples of each gathered; then a
spectrum with one refused call must make every rank raise SosProcError (no rank left waiting in the gather)."""
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
    import test_spectrum_levels as tsl
    kws = tsl._kws(rs, os.path.join(os.path.dirname(a.out), "rank%d" % rank), tsl.DIST_NAMES)
    mine = [int(i) for i in pkg.dist.balanced_shards(rs.spectrum_costs(kws), world)[rank]]
    outs = rs.sos_spectrum_levels(tsl.ALTS, kws)
    torch.cuda.synchronize()
    assert all(o is not None and len(o) == len(tsl.ALTS) for o in outs)
    part = rs.sos_spectrum_levels(tsl.ALTS, kws, gather=False)
    assert [i for i, o in enumerate(part) if o is not None] == mine
    # call 3 refused (-SURF.Type 6 without its surface index): every rank raises, whichever owns it
    bad = list(kws)
    bad[3] = dict(kws[3], isurf=6)
    raised, msg = False, ""
    try:
        rs.sos_spectrum_levels(tsl.ALTS, bad)
    except rs.SosProcError as e:
        raised, msg = True, str(e)
    dig, own, rz, ms = [None] * world, [None] * world, [None] * world, [None] * world
    dist.all_gather_object(dig, tsl._digest(outs))
    dist.all_gather_object(own, mine)
    dist.all_gather_object(rz, raised)
    dist.all_gather_object(ms, msg)
    if rank == 0:
        with open(a.out, "w") as f:
            json.dump({"world": world, "n": len(kws), "digests": dig, "owners": own, "raised": rz, "messages": ms}, f)
    rank_end()


if __name__ == "__main__":
    main()
