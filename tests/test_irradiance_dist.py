"""run_sos.sos_spectrum_irradiances on two ranks sharing one GPU (tests/dist_irradiance_worker.py through dist_launch): the
rows and the weighted sums are those of one process, bit for bit, and a call failing on one rank makes both raise."""
import json

import numpy as np
import pytest

from dist_launch import run_ranks
from test_level_absorption import dist_kws, rows_digest
from test_level_flux import GOLD

ALTS = [-1, 0.0, 3.0]


def weights(nwl):
    """R = 2: one weight per call, and one per altitude and call with a weight-0 call."""
    rng = np.random.default_rng(4)
    w = np.stack([np.repeat(rng.uniform(0.5, 2.0, (1, nwl)), len(ALTS), axis=0), rng.uniform(0.1, 2.0, (len(ALTS), nwl))])
    w[1, :, 1] = 0.0
    return w


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_return_the_rows_and_sums_of_one_process(gpu_pkg, tmp_path, monkeypatch):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    out = str(tmp_path / "res.json")
    run_ranks("dist_irradiance_worker.py", ("--out", out), timeout=600)
    r = json.load(open(out))
    kws = dist_kws(rs, tmp_path / "single")
    flux, absorb = rs.sos_spectrum_irradiances(ALTS, kws, split=True, absorption=True)
    sums = rs.sos_spectrum_irradiances(ALTS, kws, split=True, absorption=True, weights=weights(len(kws)))
    assert sums[0].shape == (2, len(ALTS), 7) and sums[1].shape == (2, len(ALTS), 5)
    assert r["world"] == 2 and r["digests"] == [rows_digest(flux, absorb)] * 2, r["digests"]
    assert r["sum_digests"] == [rows_digest([sums[0]], [sums[1]])] * 2, r["sum_digests"]
    assert sorted(i for own in r["owners"] for i in own) == list(range(len(kws))) and all(len(own) > 0 for own in r["owners"])
    assert r["partial_ok"] == [True, True]
    assert r["raised"] == [True, True] and all("wavelength 3" in m for m in r["messages"]), r["messages"]
