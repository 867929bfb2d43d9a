"""transmissions=True of run_sos.sos_spectrum and sos_spectrum_levels under torch.distributed: two ranks on one GPU
(tests/dist_spectrum_trans_worker.py)."""
import os

import numpy as np
import pytest

import spectrum_cases
from dist_launch import run_ranks


@pytest.mark.gpu
def test_transmissions_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """Eight wavelengths dealt to two ranks: every rank returns, for every call, the entry this process computes alone, bit
    for bit (no bin of a band leaves its rank, so nothing changes the order of a sum), from both entry points."""
    import dist_spectrum_trans_worker as worker
    from test_spectrum_transmissions import spectrum_keywords
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    out = str(tmp_path)
    run_ranks("dist_spectrum_trans_worker.py", ("--out", out), timeout=600)
    r0, r1 = (np.load(os.path.join(out, "trans_rank%d.npz" % r)) for r in (0, 1))
    assert r0["owned"].any() and r1["owned"].any() and np.array_equal(r0["owned"], ~r1["owned"])
    kws = spectrum_keywords(rs, tmp_path / "single")
    _, trans = rs.sos_spectrum(kws, transmissions=True)
    single = worker.flatten(trans, "s")
    single.update(worker.flatten(trans, "l"))
    for r in (r0, r1):
        assert set(r.files) == set(single) | {"owned"}
        for k, v in single.items():
            assert np.array_equal(r[k], v), k
