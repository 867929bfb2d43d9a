"""Worker of tests/test_spectrum_channels_dist.py: one rank of run_sos.sos_spectrum_channels -- plain, and at three altitudes
with fluxes -- under torch.distributed (gloo, every rank on cuda:0).  Every rank saves what it returns and the calls it owns."""
import argparse
import os

import numpy as np

from dist_launch import rank_begin, rank_end

ALTS = [-1.0, 0.0, 3.0]
VARIANT = "lambert"


def inputs(rs, workdir):
    """(keyword list, weights) of the run."""
    import test_spectrum_channels as cases
    kws = cases.spectrum(rs, workdir, VARIANT)
    return kws, cases.weights(len(kws))


def pack(chan, flux=None):
    """The arrays of a result: tables [C][K][14][361][81], scalars [C][K][5], flux rows [C][K][5]."""
    chan = [c if isinstance(c, list) else [c] for c in chan]
    out = dict(tables=np.array([[[t[e] for e in range(4, 18)] for t in c] for c in chan]),
               scalars=np.array([[[t[e] for e in range(18, 23)] for t in c] for c in chan]),
               geometry=np.concatenate([np.atleast_1d(np.asarray(chan[0][0][e], dtype=np.float64)) for e in range(4)]))
    if flux is not None:
        out["flux"] = np.array(flux)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    kws, w = inputs(rs, os.path.join(a.out, "rank%d" % rank))
    owned = np.array(sorted(int(i) for i in pkg.dist.balanced_shards(rs.spectrum_costs(kws), world)[rank]))
    plain = pack(rs.sos_spectrum_channels(kws, w))
    levels = pack(*rs.sos_spectrum_channels(kws, w, altitudes=ALTS, fluxes=True))
    np.savez(os.path.join(a.out, "channels_rank%d.npz" % rank), owned=owned, **{"plain_" + k: v for k, v in plain.items()},
             **{"levels_" + k: v for k, v in levels.items()})
    rank_end()


if __name__ == "__main__":
    main()
