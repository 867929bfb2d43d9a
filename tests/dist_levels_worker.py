"""Worker of tests/test_output_levels.py: one rank of run_sos.sos_proc_levels under torch.distributed (gloo, every rank on
cuda:0).  The CKD band's bins are sharded over the ranks and one all-reduce covers the K record sets; every rank must return,
for each altitude, exactly what sos_proc with that altitude returns under the same sharding.  Rank 0 saves its outputs."""
import argparse
import json
import os

import numpy as np
import torch.distributed as dist

from dist_launch import GOLD, rank_begin, rank_end

ALTS = [-1.0, 3.0, 0.0, 120.0, 3.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    g = np.load(os.path.join(GOLD, "sos_proc_ckd_h2o_o2_25bins_flatsea.npz"))
    user = json.loads(str(g["user_json"]))
    user.pop("-SOS.OutputAlt", None)
    user.update({"-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT", "-SOS_Main.ResRoot": ""})
    aer = {k: g["aer_" + k] for k in ("alpha", "beta", "gamma", "zeta", "a_tronc", "piztr", "piz")}
    kw = rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False)
    got = rs.sos_proc_levels(ALTS, aer_phase=aer, device=0, **kw)
    for k, z in enumerate(ALTS):
        ref = rs.sos_proc(aer_phase=aer, device=0, **dict(kw, zout=z))
        for i in range(23):
            assert np.array_equal(np.asarray(got[k][i]), np.asarray(ref[i])), (rank, z, i)
    dist.barrier()
    if rank == 0:
        res = {"alts": np.array(ALTS)}
        for k in range(len(ALTS)):
            for i in range(23):
                res["out_%d_%d" % (k, i)] = np.asarray(got[k][i])
        np.savez(a.out, **res)
    rank_end()


if __name__ == "__main__":
    main()
