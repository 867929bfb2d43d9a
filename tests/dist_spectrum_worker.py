"""Worker of tests/test_spectrum.py::test_sos_spectrum_wavelengths_over_ranks_on_one_gpu: run_sos.sos_spectrum under
torch.distributed (several ranks on cuda:0, gloo): the wavelengths are partitioned over the ranks, results gathered; then a
spectrum with one refused call must make every rank raise SosProcError (no rank left waiting in the gather)."""
import argparse
import hashlib
import json
import os

import numpy as np
import torch
import torch.distributed as dist

from dist_launch import rank_begin, rank_end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    import cases
    import spectrum_cases
    names = ["ckd_h2o_o2_25bins_flatsea", "cfg1_lambert", "ckd_o2a_5bins", "cfg2_lnd_lambert", "rand_00", "rand_13", "rand_05",
             "cfg5_ckd_maignan_25bins", "flatsea_zout", "rand_17", "land_roujean"]
    tmp = os.path.join(os.path.dirname(a.out), "rank%d" % rank)
    kws, golds, coefs, rtols = spectrum_cases.build(rs, tmp, names=names)
    mine = [int(i) for i in pkg.dist.balanced_shards(rs.spectrum_costs(kws), world)[rank]]
    outs = rs.sos_spectrum(kws)
    torch.cuda.synchronize()
    assert all(o is not None for o in outs)
    for out, g, coef, rtol in zip(outs, golds, coefs, rtols):
        cases.compare_proc_outputs(rs, out, g, coef_tronca=coef, rtol=rtol)
    h = hashlib.sha256()
    for out in outs:
        for x in out:
            h.update(np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes())
    part = rs.sos_spectrum(kws, gather=False)              # without the gather: only this rank's wavelengths are filled
    assert [i for i, o in enumerate(part) if o is not None] == mine
    # call 3 refused (-SURF.Type 6 without its surface index): every rank raises, whichever owns it
    bad = list(kws)
    bad[3] = dict(kws[3], isurf=6)
    raised, msg = False, ""
    try:
        rs.sos_spectrum(bad)
    except rs.SosProcError as e:
        raised, msg = True, str(e)
    dig, own, rz, ms = [None] * world, [None] * world, [None] * world, [None] * world
    dist.all_gather_object(dig, h.hexdigest())
    dist.all_gather_object(own, mine)
    dist.all_gather_object(rz, raised)
    dist.all_gather_object(ms, msg)
    if rank == 0:
        with open(a.out, "w") as f:
            json.dump({"world": world, "n": len(kws), "digests": dig, "owners": own, "raised": rz, "messages": ms}, f)
    rank_end()


if __name__ == "__main__":
    main()
