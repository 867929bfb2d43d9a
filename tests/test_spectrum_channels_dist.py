"""run_sos.sos_spectrum_channels under torch.distributed: two ranks on one GPU (tests/dist_channels_worker.py)."""
import os

import numpy as np
import pytest

import spectrum_cases
from dist_launch import run_ranks


@pytest.mark.gpu
def test_channels_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """Seven wavelengths dealt to two ranks, both owning some: the ranks return arrays equal bit for bit to each other (one
    all-reduce of the accumulator and one of the scalar sums, then every rank finishes), and equal to this process's
    single-rank result within 1e-9 |ref| + 1e-12 max(1, max |ref|) per table -- only the order of the sum across the ranks
    differs.  Plain, and at three altitudes with fluxes."""
    import dist_channels_worker as worker
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    out = str(tmp_path)
    run_ranks("dist_channels_worker.py", ("--out", out), timeout=600)
    r0, r1 = (np.load(os.path.join(out, "channels_rank%d.npz" % r)) for r in (0, 1))
    assert len(r0["owned"]) and len(r1["owned"])
    assert sorted(list(r0["owned"]) + list(r1["owned"])) == list(range(len(r0["owned"]) + len(r1["owned"])))
    for k in r0.files:
        if k != "owned":
            assert np.array_equal(r0[k], r1[k]), k
    kws, w = worker.inputs(rs, str(tmp_path / "single"))
    single = dict(("plain_" + k, v) for k, v in worker.pack(rs.sos_spectrum_channels(kws, w)).items())
    single.update(("levels_" + k, v) for k, v in
                  worker.pack(*rs.sos_spectrum_channels(kws, w, altitudes=worker.ALTS, fluxes=True)).items())
    assert sorted(single) == sorted(k for k in r0.files if k != "owned")
    for k, ref in single.items():
        got = r0[k]
        assert got.shape == ref.shape, k
        if k.endswith("tables"):                          # per table: [C][K][14] tables of (361, 81)
            flat_ref = ref.reshape(-1, 361, 81)
            flat_got = got.reshape(-1, 361, 81)
        else:
            flat_ref, flat_got = ref[None], got[None]
        for t, (g, r) in enumerate(zip(flat_got, flat_ref)):
            tol = 1e-9 * np.abs(r) + 1e-12 * max(1.0, np.abs(r).max())
            assert np.all(np.abs(g - r) <= tol), (k, t, np.abs(g - r).max())
