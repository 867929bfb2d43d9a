"""bench.py's contract: a plain run times the steps and prints the headline line, nothing else; --dump-outputs writes what the
last timed step computed (the band result, and the per-bin outputs of a fixed, seeded sample of bins in generation order)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = {"band_rec", "band_scal", "bin_rec", "bin_norders", "bin_iglast", "bin_flux"}
FULL_ONLY = {"roofline", "per_rank", "batch_4096", "realistic_mix", "small_band", "variants", "hyperspectral", "cpu_baseline"}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_sample_in_generation_order(pkg, tmp_path):
    import torch
    nb, s, w = 300, 4, 5
    gen_rec = np.random.default_rng(2).normal(size=(nb, s, 3, w))
    perm = np.random.default_rng(1).permutation(nb)            # device position i holds generation bin perm[i] (upload_bins)
    out = dict(rec=torch.from_numpy(gen_rec[perm]), norders=torch.from_numpy(perm.astype(np.int32)),
               iglast=torch.from_numpy(np.repeat(perm[:, None], s, axis=1).astype(np.int32)),
               flux=torch.from_numpy(np.stack([perm, -perm], axis=1).astype(np.float64)))
    band_rec = torch.from_numpy(np.random.default_rng(3).normal(size=(1, s, 3, w)))
    band_scal = torch.from_numpy(np.arange(12, dtype=np.float64)[None])
    buf = pkg.dist.pack_partial(band_rec, band_scal)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), pkg, torch, buf, out, perm)
    got, again = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(got) == DUMPED and all(a.dtype == np.float64 for a in got.values())
    assert all(np.array_equal(got[k], again[k]) for k in DUMPED)             # the sample is fixed
    idx = got["bin_norders"].astype(np.int64)                                   # generation indices of the sampled bins
    assert len(idx) == bench.DUMP_BINS and np.all(np.diff(idx) > 0)
    assert np.array_equal(got["bin_rec"], gen_rec[idx])
    assert np.array_equal(got["bin_iglast"][:, 0], idx) and np.array_equal(got["bin_flux"][:, 1], -idx)
    assert np.array_equal(got["band_rec"], band_rec.numpy()) and np.array_equal(got["band_scal"], band_scal.numpy())
    bench.dump_outputs(str(tmp_path / "c"), pkg, torch, buf, out, None)      # no permutation: device order is generation order
    assert np.array_equal(_load(tmp_path / "c")["bin_rec"], gen_rec[perm][idx])


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(gpu_pkg, tmp_path):
    d = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bins", "1024", "--dump-outputs", d], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == "CKD spectral bins/sec (full Stokes I,Q,U, TOA+surface)" and line["unit"] == "bins/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1024 * 1e3 / line["ms_per_step"], rel=1e-9)
    assert not FULL_ONLY & set(line)
    got = _load(d)
    assert set(got) == DUMPED and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(np.all(np.isfinite(a)) for a in got.values())
    nord = got["bin_norders"]
    assert len(nord) == bench.DUMP_BINS and np.all(nord >= 1)
    # the band is the AIK-weighted sum of every bin: its order count is the largest of the batch's
    assert int(got["band_scal"][0, 7]) >= nord.max()
