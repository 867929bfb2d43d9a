"""Worker of tests/test_spectrum_albedo_dist.py: one rank of run_sos.sos_spectrum(..., transmissions=True,
spherical_albedo=True) and of run_sos.sos_spectrum_levels with the same keywords under torch.distributed (gloo, every rank
on cuda:0): the wavelengths are dealt to the ranks, s_alb travels inside the gathered transmission entries.  Every rank saves
what it holds."""
import argparse
import os

import numpy as np

from dist_launch import rank_begin, rank_end

ALTS = [-1.0, 2.0]
NCALLS = 5          # the first calls of test_spectrum_transmissions.NAMES: grouped, 5-bin band, no-gas, 25-bin band, single


def keywords(rs, workdir):
    from test_spectrum_transmissions import spectrum_keywords
    return spectrum_keywords(rs, workdir)[:NCALLS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    kws = keywords(rs, os.path.join(a.out, "rank%d" % rank))
    tuples, trans = rs.sos_spectrum(kws, transmissions=True, spherical_albedo=True)
    assert len(tuples) == len(trans) == len(kws) and all(t is not None and "s_alb" in t for t in trans)
    _, ptrans = rs.sos_spectrum(kws, transmissions=True, spherical_albedo=True, gather=False)
    spec, ltrans = rs.sos_spectrum_levels(ALTS, kws, transmissions=True, spherical_albedo=True)
    assert len(spec) == len(ltrans) == len(kws)
    np.savez(os.path.join(a.out, "albedo_rank%d.npz" % rank), owned=np.array([t is not None for t in ptrans]),
             s_alb=np.array([t["s_alb"] for t in trans]), s_alb_levels=np.array([t["s_alb"] for t in ltrans]),
             s_alb_owned=np.array([np.nan if t is None else t["s_alb"] for t in ptrans]))
    rank_end()


if __name__ == "__main__":
    main()
