"""Worker of tests/test_level_absorption.py::test_two_ranks_on_one_gpu_return_the_same_rows: run_sos.sos_spectrum_levels with
fluxes=True, absorption=True under torch.distributed (two ranks on cuda:0, gloo).  The wavelengths are dealt whole to the ranks;
with gather=True the rows travel with the compacted tuples, with gather=False the slots of the other rank stay None."""
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
    import test_level_absorption as tla
    kws = tla.dist_kws(rs, os.path.join(os.path.dirname(a.out), "rank%d" % rank))
    mine = [int(i) for i in pkg.dist.balanced_shards(rs.spectrum_costs(kws), world)[rank]]
    outs, flux, absorb = rs.sos_spectrum_levels(tla.DIST_ALTS, kws, fluxes=True, absorption=True)
    torch.cuda.synchronize()
    assert all(o is not None for o in outs) and all(x is not None and x.shape == (len(tla.DIST_ALTS), 5) for x in absorb)
    _, pflux, pabsorb = rs.sos_spectrum_levels(tla.DIST_ALTS, kws, fluxes=True, absorption=True, gather=False)
    partial_ok = ([i for i, x in enumerate(pabsorb) if x is not None] == mine and
                  all(tla.rows_digest([pflux[i]], [pabsorb[i]]) == tla.rows_digest([flux[i]], [absorb[i]]) for i in mine))
    dig, own, ok = [None] * world, [None] * world, [None] * world
    dist.all_gather_object(dig, tla.rows_digest(flux, absorb))
    dist.all_gather_object(own, mine)
    dist.all_gather_object(ok, bool(partial_ok))
    if rank == 0:
        with open(a.out, "w") as f:
            json.dump({"world": world, "n": len(kws), "digests": dig, "owners": own, "partial_ok": ok}, f)
    rank_end()


if __name__ == "__main__":
    main()
