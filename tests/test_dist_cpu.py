"""World-size-2 gloo test of the sharded bin aggregation (the N>1 path of bench.py without GPUs):
each rank forms the AIK-weighted partial sums of its shard, one all-reduce combines them, and the
result equals the serial SOS_AGGREGATE of the whole bin list within fp64 summation noise."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dist_launch import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q, nb=13, balanced=False):
    sys.path.insert(0, ROOT)
    import importlib
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(11)
    S1, W = 6, 9
    rec = rng.normal(size=(nb, S1, 3, W))
    nf = rng.integers(1, S1 + 1, nb)
    for b in range(nb):
        rec[b, nf[b]:] = 0.0
    aik = rng.dirichlet(np.ones(nb))
    flux = rng.uniform(size=(nb, 2))
    scal = rng.uniform(size=(nb, 4))
    if balanced:      # the drop-in's partition: bins dealt by cost, original order kept within a rank, possibly empty
        sl = pkg.dist.balanced_shards(rng.uniform(1.0, 10.0, nb), world)[rank]
    else:
        sl = np.arange(*pkg.dist.shard_range(nb, rank, world))
    # local partial sums in the layout sosgpu_aggregate produces (include/sosgpu.h); an empty shard gives the neutral element
    prec = torch.from_numpy((aik[sl, None, None, None] * rec[sl]).sum(0, keepdims=True))
    a = aik[sl]
    tdg = rng.uniform(size=(nb, 4))                       # TDIFMUG(1..N), N = 4
    nmax, nmin = (float(nf[sl].max()), -float(nf[sl].min())) if len(sl) else (0.0, -2147483647.0)
    pscal = torch.tensor([[(a * scal[sl, 0]).sum(), (a * flux[sl, 0]).sum(), (a * flux[sl, 1]).sum(),
                           (a * np.exp(-scal[sl, 1])).sum(), (a * np.exp(-scal[sl, 2])).sum(),
                           (a * np.exp(-scal[sl, 3])).sum(), a.sum(), nmax, nmin,
                           0.0] + list((a[:, None] * tdg[sl]).sum(0))], dtype=torch.float64)
    buf = pkg.dist.pack_partial(prec, pscal)
    buf = pkg.dist.all_reduce_partial(buf, pscal.shape[1])
    r, s = pkg.dist.unpack_partial(buf, prec.shape)
    fin = pkg.dist.finish_scalars(s)
    if rank == 0:
        q.put((r.numpy(), {k: v for k, v in fin.items()}, rec, nf, aik, flux, scal, tdg))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,nb,balanced", [(2, 13, False), (2, 13, True), (3, 13, True), (3, 2, True)])
def test_sharded_aggregate_matches_serial(oracle, world, nb, balanced):
    """Contiguous (bench.py's weak-scaling bands) and cost-balanced (the drop-in's) partitions, 2 and 3 ranks, and 2 bins over
    3 ranks (one rank holds none and contributes the neutral element): the all-reduced band equals the serial SOS_AGGREGATE."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, nb, balanced)) for r in range(world)]
    for p in procs:
        p.start()
    got_rec, fin, rec, nf, aik, flux, scal, tdg = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sb = np.zeros((len(aik), 7))
    sb[:, 0], sb[:, 1], sb[:, 2] = scal[:, 0], flux[:, 0], flux[:, 1]
    sb[:, 3:6] = scal[:, 1:4]
    exp_rec, exp_scal = oracle.aggregate(rec, nf.astype(np.int32), aik, sb)
    assert np.allclose(got_rec[0][:exp_rec.shape[0]], exp_rec, rtol=1e-13, atol=1e-14)
    assert np.allclose([fin["tdifmus"][0], fin["emoins"][0], fin["eplus"][0]], exp_scal[:3], rtol=1e-12)
    assert np.allclose([fin["ttot_tronc"][0], fin["ttot_vrai"][0], fin["tauout"][0]], exp_scal[3:6], rtol=1e-11)
    assert fin["n_orders"][0] == nf.max() and fin["min_orders"][0] == nf.min()
    assert np.allclose(fin["tdifmug"][0], (aik[:, None] * tdg).sum(0), rtol=1e-13)      # SOS_AGGREGATE.F:455-458
    assert abs(fin["sum_aik"][0] - 1.0) < 1e-12


def test_shard_range_partitions():
    import importlib
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    for nb in (1, 7, 32, 4097):
        for world in (1, 2, 3, 8):
            spans = [pkg.dist.shard_range(nb, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == nb
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_bench_self_launch_two_ranks():
    """`python bench.py --gpus 2` with no launcher environment must start two ranks by itself (child torchrun) and report
    n_gpus = 2; --dry-run keeps it on the CPU (gloo, fabricated partials, the real pack / all-reduce / finish code)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--bins", "5"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["dry_run"] is True and res["reduce_ok"] is True


def test_bench_rejects_mismatched_world():
    import subprocess
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_cost_balanced_partition_on_the_realistic_mix(pkg, oracle):
    """Strong scaling of ONE band: the bins of the realistic mix (gas columns k log-uniform 1e-3..30) differ 3x in
    cost (NT 117...420, 69...115 scattering steps).  dist.bin_cost knows only the optical depths; the TRUE cost of every bin,
    NT x scattering steps, comes from the oracle (SOS_PROFILE + SOS_OS restatements, N = 8 to keep it short).  Dealt by
    balanced_shards the per-rank sums of the true cost differ by < 5 %; contiguous slices of the band in the reference's bin
    order (strongest absorber first, SOS_PROC.F:3459-3466) by far more."""
    sys.path.insert(0, ROOT)
    import bench
    S, D = pkg.synth, pkg.dist
    nb = 128
    alt, tabs = bench.realistic_columns(nb)
    mu, w, n0 = S.gauss_angles(8, 35.0)
    os_nb = 24
    al, be, ga, ze = S.hg_phase(os_nb, 0.75)
    true = np.zeros(nb)
    for b in range(nb):
        pr = oracle.sos_profile(0.0948, 8.0, 0.3, 2.0, alt, tabs[b], 1)
        h, x, y, ib = oracle.profile_rescale(pr["h"], pr["xdel"], pr["ydel"], 0.0, 0.95, 0.95, os_nb)
        r = oracle.sos_os(mu, w, os_nb, h, x, y, al, be, ga, ze, n0=n0, ro=0.1, iborm=ib, zprof=pr["zprof"])
        true[b] = pr["nt"] * float(r["ig_counts"].sum())
    assert true.max() > 2.5 * true.min()
    est = D.bin_cost(0.0948 + 0.3, tabs[:, -1])
    assert np.corrcoef(true, est)[0, 1] > 0.95
    order = np.argsort(-tabs[:, -1])                       # the band as the reference enumerates it: strongest absorber first
    for world in (2, 3, 4, 8):
        loads = np.array([true[s].sum() for s in D.balanced_shards(est, world)])
        spread = (loads.max() - loads.min()) / loads.mean()
        cont = np.array([true[order][slice(*D.shard_range(nb, r, world))].sum() for r in range(world)])
        spread_c = (cont.max() - cont.min()) / cont.mean()
        assert spread < 0.05, (world, spread)
        assert spread_c > 4 * spread, (world, spread, spread_c)
