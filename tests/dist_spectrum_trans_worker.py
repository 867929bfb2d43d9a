"""Worker of tests/test_spectrum_transmissions_dist.py: one rank of run_sos.sos_spectrum(..., transmissions=True) and of
run_sos.sos_spectrum_levels(..., fluxes=True, transmissions=True) under torch.distributed (gloo, every rank on cuda:0): the
wavelengths are dealt to the ranks, the transmission entries travel with the gathered tuples.  Every rank saves its entries."""
import argparse
import os

import numpy as np

from dist_launch import rank_begin, rank_end

ALTS = [-1.0, 2.0]
KEYS = ("thetas", "thetav", "ttot_tronc", "ttot_vrai", "tdifmus", "tdifmug", "t_dir_down", "t_dif_down", "t_dif_up")


def flatten(trans, prefix):
    """The entries of a pass as arrays for np.savez: <prefix><call>_<key>."""
    return {"%s%d_%s" % (prefix, i, k): np.asarray(t[k]) for i, t in enumerate(trans) for k in KEYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    from test_spectrum_transmissions import spectrum_keywords
    kws = spectrum_keywords(rs, os.path.join(a.out, "rank%d" % rank))
    tuples, trans = rs.sos_spectrum(kws, transmissions=True)
    assert len(tuples) == len(trans) == len(kws) and all(t is not None for t in trans)
    part, ptrans = rs.sos_spectrum(kws, transmissions=True, gather=False)
    assert [i for i, t in enumerate(part) if t is not None] == [i for i, t in enumerate(ptrans) if t is not None]
    spec, flux, ltrans = rs.sos_spectrum_levels(ALTS, kws, fluxes=True, transmissions=True)
    assert len(spec) == len(flux) == len(ltrans) == len(kws)
    np.savez(os.path.join(a.out, "trans_rank%d.npz" % rank), owned=np.array([t is not None for t in ptrans]),
             **flatten(trans, "s"), **flatten(ltrans, "l"))
    rank_end()


if __name__ == "__main__":
    main()
