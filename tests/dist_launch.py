"""The multi-rank plumbing of the suite, stated once.  For the tests: the torch.distributed.run command line of a worker
(tests/dist_*_worker.py), the environment its ranks get, and the run with the tails of its output in the assert.  For the
workers: the set-up of a rank (device, process group, package) and its ending."""
import importlib
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
GOLD = os.path.join(TESTS, "golden")
LAUNCHER_VARIABLES = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")     # must not leak into the ranks


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_command(worker, args=(), world=2, port=None):
    """The argv that starts `world` ranks of tests/<worker> on this host; port None: a free one."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
            "--master-port", str(free_port() if port is None else port), os.path.join(TESTS, worker)] + [str(x) for x in args]


def rank_env(extra=None, base=os.environ):
    """A copy of `base` without the launcher's variables, HSA_ENABLE_IPC_MODE_LEGACY=0 (several ranks share one device), then
    `extra`."""
    env = {k: v for k, v in base.items() if k not in LAUNCHER_VARIABLES}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env.update(extra or {})
    return env


def run_ranks(worker, args=(), world=2, timeout=600, env=None):
    """Runs the ranks to their end; a rank that fails shows the tails of what they wrote.  env None: rank_env()."""
    p = subprocess.run(rank_command(worker, args, world), capture_output=True, text=True, timeout=timeout,
                       env=rank_env() if env is None else env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    return p


def rank_begin(abs_root=GOLD, backend="gloo"):
    """First lines of a worker: (rank, world, package).  gloo: every rank on cuda:0; nccl: one device per rank.  abs_root: the
    SOS_ABS_ROOT of the rank (None: left as it is)."""
    import torch
    import torch.distributed as dist
    for p in (TESTS, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if abs_root is not None:
        os.environ["SOS_ABS_ROOT"] = abs_root
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) if backend == "nccl" else 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, importlib.import_module("radiativetransfer-sos_amd")


def rank_end():
    """Last lines of a worker: no rank leaves while another still computes or writes."""
    import torch
    import torch.distributed as dist
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
