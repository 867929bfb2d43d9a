"""split=True of run_sos.sos_proc_levels and sos_spectrum_levels under torch.distributed: two ranks on one GPU
(tests/dist_level_split_worker.py)."""
import os

import numpy as np
import pytest

import spectrum_cases
from dist_launch import run_ranks


@pytest.mark.gpu
def test_split_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """A band of five CKD bins sharded over two ranks and four wavelengths dealt to them: both ranks return [K][7] arrays
    equal bit for bit to each other (element 9 of the scalar blocks is summed by the band's one all-reduce; the spectrum's
    wider rows travel with the gathered tuples, and the ungathered rows equal them -- asserted in the worker), and equal to
    this process's within 1e-12 relative: the all-reduce changes the order of the bin sums, nothing else differs."""
    import dist_level_split_worker as worker
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    out = str(tmp_path)
    run_ranks("dist_level_split_worker.py", ("--out", out), timeout=600)
    r0, r1 = (np.load(os.path.join(out, "split_rank%d.npz" % r)) for r in (0, 1))
    assert r0["band"].shape == (len(worker.ALTS), 7) and r0["spectrum"].shape == (len(worker.SPECTRUM), len(worker.ALTS), 7)
    assert np.array_equal(r0["band"], r1["band"]) and np.array_equal(r0["spectrum"], r1["spectrum"])
    assert r0["owned"].any() and r1["owned"].any() and np.array_equal(r0["owned"], ~r1["owned"])
    band, spectrum = worker.inputs(rs, str(tmp_path / "single"))
    _, flux = rs.sos_proc_levels(worker.ALTS, fluxes=True, split=True, **band)
    _, sflux = rs.sos_spectrum_levels(worker.ALTS, spectrum, fluxes=True, split=True)
    assert np.isfinite(flux).all() and (flux[:, [0, 1, 2, 3, 5, 6]] > 0).all()
    assert np.all(np.abs(r0["band"] - flux) <= 1e-12 * np.abs(flux)), np.abs(r0["band"] / flux - 1).max()
    sflux = np.array(sflux)
    assert np.all(np.abs(r0["spectrum"] - sflux) <= 1e-12 * np.abs(sflux)), np.abs(r0["spectrum"] / sflux - 1).max()
