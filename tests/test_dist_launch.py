"""tests/dist_launch.py, the pure half: the command line of the ranks and the environment they get (no GPU, no process)."""
import os
import sys

import pytest
from torch.distributed import run as launcher

import dist_launch

LAUNCHER = dict(WORLD_SIZE="8", RANK="3", LOCAL_RANK="3", MASTER_PORT="29500", MASTER_ADDR="10.0.0.1")


@pytest.mark.parametrize("world,args", [(2, ("--out", "/tmp/x")), (4, ("--case", "ckd_o2a_5bins", "--bins", 7))])
def test_rank_command(world, args):
    cmd = dist_launch.rank_command("dist_proc_worker.py", args, world=world, port=12345)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_proc_worker.py")
    assert cmd == [sys.executable, "-m", launcher.__name__, "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                   "--master-port", "12345", worker] + [str(x) for x in args]
    assert os.path.isfile(worker) and all(isinstance(x, str) for x in cmd)


def test_rank_command_defaults():
    """Two ranks, no worker arguments, a port of its own choice."""
    cmd = dist_launch.rank_command("dist_gpu_worker.py")
    assert cmd[5] == "2" and cmd[-1].endswith(os.path.join("tests", "dist_gpu_worker.py"))
    assert cmd[-3] == "--master-port" and 0 < int(cmd[-2]) < 65536


def test_rank_env_drops_the_launcher_variables():
    base = dict(LAUNCHER, PATH="/usr/bin", HSA_ENABLE_IPC_MODE_LEGACY="1")
    env = dist_launch.rank_env(base=base)
    assert env == {"PATH": "/usr/bin", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    assert base["RANK"] == "3" and base["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"            # a copy: the base is left alone
    env = dist_launch.rank_env({"SOS_ABS_ROOT": "/data", "MASTER_PORT": "1234"}, base=base)
    assert env == {"PATH": "/usr/bin", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "SOS_ABS_ROOT": "/data", "MASTER_PORT": "1234"}


def test_rank_env_reads_the_environment_of_the_call(monkeypatch):
    """The default base is the process's environment when the ranks start, not when the module was imported."""
    monkeypatch.setenv("SOS_ABS_ROOT", "/somewhere")
    monkeypatch.setenv("RANK", "1")
    env = dist_launch.rank_env()
    assert env["SOS_ABS_ROOT"] == "/somewhere" and "RANK" not in env and env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
