"""spherical_albedo=True of run_sos.sos_spectrum and sos_spectrum_levels under torch.distributed: two ranks on one GPU
(tests/dist_spectrum_albedo_worker.py)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import spectrum_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_spherical_albedo_two_ranks_on_one_gpu(gpu_pkg, tmp_path, monkeypatch):
    """Five wavelengths dealt to two ranks: every rank holds every call's s_alb, equal to what this process computes alone, bit
    for bit (no bin of a band leaves its rank), from both entry points; with gather=False a rank holds its own calls' only."""
    import dist_spectrum_albedo_worker as worker
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dist_spectrum_albedo_worker.py"), "--out", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    r0, r1 = (np.load(os.path.join(out, "albedo_rank%d.npz" % r)) for r in (0, 1))
    assert r0["owned"].any() and r1["owned"].any() and np.array_equal(r0["owned"], ~r1["owned"])
    _, trans = rs.sos_spectrum(worker.keywords(rs, tmp_path / "single"), transmissions=True, spherical_albedo=True)
    single = np.array([t["s_alb"] for t in trans])
    assert np.all(single > 0.0)
    for r in (r0, r1):
        assert np.array_equal(r["s_alb"], single) and np.array_equal(r["s_alb_levels"], single)
        assert np.array_equal(r["s_alb_owned"][r["owned"]], single[r["owned"]]) and np.all(np.isnan(r["s_alb_owned"][~r["owned"]]))
