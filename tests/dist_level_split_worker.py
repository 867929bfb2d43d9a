"""Worker of tests/test_level_split_dist.py: one rank of run_sos.sos_proc_levels(..., fluxes=True, split=True) on a CKD band
(bins sharded over the ranks: the band transmission of the untruncated depth rides the one all-reduce in element 9 of the
scalar blocks) and of run_sos.sos_spectrum_levels(..., fluxes=True, split=True) on four wavelengths (dealt to the ranks, the
[K][7] rows gathered with the tuples), under torch.distributed (gloo, every rank on cuda:0).  Every rank saves its arrays."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ["SOS_ABS_ROOT"] = os.path.join(ROOT, "tests", "golden")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rs = importlib.import_module("radiativetransfer-sos_amd").run_sos
    band, spectrum = inputs(rs, os.path.join(a.out, "rank%d" % rank))
    tuples, flux = rs.sos_proc_levels(ALTS, fluxes=True, split=True, **band)
    assert len(tuples) == len(ALTS) and flux.shape == (len(ALTS), 7)
    spec, sflux = rs.sos_spectrum_levels(ALTS, spectrum, fluxes=True, split=True)
    assert len(spec) == len(sflux) == len(spectrum) and all(f is not None and f.shape == (len(ALTS), 7) for f in sflux)
    part, pflux = rs.sos_spectrum_levels(ALTS, spectrum, fluxes=True, split=True, gather=False)
    assert [i for i, t in enumerate(part) if t is not None] == [i for i, f in enumerate(pflux) if f is not None]
    assert all(np.array_equal(f, sflux[i]) for i, f in enumerate(pflux) if f is not None)
    torch.cuda.synchronize()
    np.savez(os.path.join(a.out, "split_rank%d.npz" % rank), band=flux, spectrum=np.array(sflux),
             owned=np.array([f is not None for f in pflux]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
