"""Worker of tests/test_level_split_dist.py: one rank of run_sos.sos_proc_levels(..., fluxes=True, split=True) on a CKD band
(bins sharded over the ranks: the band transmission of the untruncated depth rides the one all-reduce in element 9 of the
scalar blocks) and of run_sos.sos_spectrum_levels(..., fluxes=True, split=True) on four wavelengths (dealt to the ranks, the
[K][7] rows gathered with the tuples), under torch.distributed (gloo, every rank on cuda:0).  Every rank saves its arrays."""
import argparse
import os

import numpy as np

from dist_launch import rank_begin, rank_end

ALTS = [-1.0, 0.0, 3.0]
BAND = "ckd_o2a_5bins"
SPECTRUM = ["cfg1_lambert", "cfg4_glitter_bilnd", "ckd_o2a_5bins", "layer_1_3km_lnd"]


def inputs(rs, workdir):
    """(keywords of the band, keyword list of the spectrum), zout = -1."""
    import spectrum_cases
    kws, _, _, _ = spectrum_cases.build(rs, workdir, names=[BAND] + SPECTRUM)
    kws = [dict(kw, zout=-1.0) for kw in kws]
    return kws[0], kws[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world, pkg = rank_begin()
    rs = pkg.run_sos
    band, spectrum = inputs(rs, os.path.join(a.out, "rank%d" % rank))
    tuples, flux = rs.sos_proc_levels(ALTS, fluxes=True, split=True, **band)
    assert len(tuples) == len(ALTS) and flux.shape == (len(ALTS), 7)
    spec, sflux = rs.sos_spectrum_levels(ALTS, spectrum, fluxes=True, split=True)
    assert len(spec) == len(sflux) == len(spectrum) and all(f is not None and f.shape == (len(ALTS), 7) for f in sflux)
    part, pflux = rs.sos_spectrum_levels(ALTS, spectrum, fluxes=True, split=True, gather=False)
    assert [i for i, t in enumerate(part) if t is not None] == [i for i, f in enumerate(pflux) if f is not None]
    assert all(np.array_equal(f, sflux[i]) for i, f in enumerate(pflux) if f is not None)
    np.savez(os.path.join(a.out, "split_rank%d.npz" % rank), band=flux, spectrum=np.array(sflux),
             owned=np.array([f is not None for f in pflux]))
    rank_end()


if __name__ == "__main__":
    main()
