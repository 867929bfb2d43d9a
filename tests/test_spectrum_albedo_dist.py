"""spherical_albedo=True of run_sos.sos_spectrum and sos_spectrum_levels under torch.distributed: two ranks on one GPU
(tests/dist_spectrum_albedo_worker.py)."""
import os

import numpy as np
import pytest

import spectrum_cases
from dist_launch import run_ranks


@pytest.mark.gpu
def test_spherical_albedo_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """Five wavelengths dealt to two ranks: every rank holds every call's s_alb, equal to what this process computes alone, bit
    for bit (no bin of a band leaves its rank), from both entry points; with gather=False a rank holds its own calls' only."""
    import dist_spectrum_albedo_worker as worker
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    out = str(tmp_path)
    run_ranks("dist_spectrum_albedo_worker.py", ("--out", out), timeout=300)
    r0, r1 = (np.load(os.path.join(out, "albedo_rank%d.npz" % r)) for r in (0, 1))
    assert r0["owned"].any() and r1["owned"].any() and np.array_equal(r0["owned"], ~r1["owned"])
    _, trans = rs.sos_spectrum(worker.keywords(rs, tmp_path / "single"), transmissions=True, spherical_albedo=True)
    single = np.array([t["s_alb"] for t in trans])
    assert np.all(single > 0.0)
    for r in (r0, r1):
        assert np.array_equal(r["s_alb"], single) and np.array_equal(r["s_alb_levels"], single)
        assert np.array_equal(r["s_alb_owned"][r["owned"]], single[r["owned"]]) and np.all(np.isnan(r["s_alb_owned"][~r["owned"]]))
