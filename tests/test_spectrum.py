"""run_sos.sos_spectrum: a list of sos_proc calls (one per wavelength, binding/run_sos.py:640-695) as one pass over the GPU --
all bins of all wavelengths in one launch per kernel variant (BASELINE config 5's shape), and, under torch.distributed, the
wavelengths dealt to the ranks (gather only, no all-reduce)."""
import json
import os
import sys

import numpy as np
import pytest

import cases
import spectrum_cases
from dist_launch import free_port, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = spectrum_cases.GOLD


def test_spectrum_costs_and_balanced_shards(pkg, monkeypatch, tmp_path):
    """Host side of the wavelength partition: costs from the keywords alone (bins of the interval x level / order estimate),
    longest-processing-time dealing, every wavelength owned exactly once, identical on every rank (deterministic)."""
    rs, D = pkg.run_sos, pkg.dist
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=["cfg1_lambert", "ckd_o2a_5bins",
                                                             "ckd_h2o_o2_25bins_flatsea", "cfg2_lnd_lambert"])
    c = rs.spectrum_costs(kws)
    assert c.shape == (4,) and np.all(c > 0)
    assert c[2] > c[1] > c[0]                              # 25 bins > 5 bins > 1 molecular bin
    assert c[3] > c[0]                                     # aerosols: tens of Fourier orders instead of 3
    rng = np.random.default_rng(3)
    costs = rng.uniform(1.0, 100.0, 500)
    for world in (1, 2, 3, 8):
        sh = D.balanced_shards(costs, world)
        assert len(sh) == world
        allidx = np.concatenate(sh)
        assert sorted(allidx.tolist()) == list(range(500))
        assert all(np.all(np.diff(s) > 0) for s in sh if len(s) > 1)       # original order kept within a rank
        loads = np.array([costs[s].sum() for s in sh])
        assert (loads.max() - loads.min()) / loads.mean() < 0.02
    sh = D.balanced_shards([5.0, 1.0], 3)                  # fewer items than ranks: an empty shard
    assert [len(s) for s in sh] == [1, 1, 0]


def test_compact_and_expand_outputs_round_trip(pkg):
    rs = pkg.run_sos
    rng = np.random.default_rng(0)
    n, nrow = 13, 2
    tabs = []
    for _ in range(14):
        t = np.zeros((361, 81))
        t[:nrow, :n] = rng.normal(size=(nrow, n))
        tabs.append(t)
    tup = (n, np.arange(81, dtype=np.int32), rng.normal(size=361), rng.normal(size=81)) + tuple(tabs) + (0.1, 0.2, 0.3, 0.4, 0.5)
    c = rs._compact_outputs(tup, nrow)
    assert c[5].shape == (nrow, n)
    back = rs._expand_outputs(c)
    assert len(back) == 23
    for a, b in zip(tup, back):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import importlib
    import torch.distributed as dist
    pkg = importlib.import_module("radiativetransfer-sos_amd")
    rs = pkg.run_sos
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nwl = 7
    costs = np.array([3.0, 50.0, 1.0, 20.0, 20.0, 2.0, 9.0])
    mine = [int(i) for i in pkg.dist.balanced_shards(costs, world)[rank]]
    results, nrows = [None] * nwl, {}
    for i in mine:                          # fabricated 23-tuples: a function of the wavelength index only
        rng = np.random.default_rng(100 + i)
        n, nrow = 5 + i, 2 + i
        tabs = []
        for _ in range(14):
            t = np.zeros((361, 81))
            t[:nrow, :n] = rng.normal(size=(nrow, n))
            tabs.append(t)
        results[i] = (n, np.arange(81, dtype=np.int32), rng.normal(size=361), rng.normal(size=81)) + tuple(tabs) + (0.1 * i,) * 5
        nrows[i] = nrow
    nz = 3                                  # ... and lists of nz tuples per wavelength (output altitudes): slot k scaled by k + 1
    levels = [None if r is None else [tuple(x * (k + 1) if i == 5 else x for i, x in enumerate(r)) for k in range(nz)]
              for r in results]
    rs._gather_results(results, mine, nrows, world)
    rs._gather_results(levels, mine, nrows, world, nz)
    sums = [float(np.asarray(r[5]).sum()) + float(r[22]) for r in results]
    for r, lv in zip(results, levels):
        assert len(lv) == nz
        for k, t in enumerate(lv):
            assert len(t) == 23 and all(np.array_equal(np.asarray(x) * (k + 1) if i == 5 else np.asarray(x), np.asarray(y))
                                        for i, (x, y) in enumerate(zip(r, t)))
    q.put((rank, mine, sums))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_wavelength_partition_gather_gloo(world):
    """The N > 1 path of sos_spectrum without GPUs: every rank computes its own wavelengths (fabricated tuples), one
    all_gather_object of the compacted tuples, and every rank ends with the complete, identical list -- for one tuple per
    wavelength and for lists of K tuples per wavelength (sos_spectrum_levels)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    owned = sorted(i for _, mine, _ in got for i in mine)
    assert owned == list(range(7))
    sums = [s for _, _, s in got]
    assert all(s == sums[0] for s in sums) and all(np.isfinite(sums[0]))


@pytest.mark.gpu
def test_sos_spectrum_equals_sequential_sos_proc_bitwise(gpu_pkg, tmp_path, monkeypatch):
    """56 calls (the 20 random keyword sets twice + 16 fixed goldens: CKD bands of 5 and 25 bins, aerosol models through the
    reference's Aerosols.txt, every surface type, both views, output levels) through sos_spectrum: every output equals the
    compiled reference's at the golden's tolerance, and equals the sequential sos_proc of the same keywords BIT FOR BIT."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, golds, coefs, rtols = spectrum_cases.build(rs, tmp_path)
    assert len(kws) >= 40
    tm = {}
    outs = rs.sos_spectrum(kws, timings=tm)
    assert len(outs) == len(kws) and all(o is not None for o in outs)
    for out, g, coef, rtol in zip(outs, golds, coefs, rtols):
        cases.compare_proc_outputs(rs, out, g, coef_tronca=coef, rtol=rtol)
    for k, kw in enumerate(kws):
        seq = rs.sos_proc(**kw)
        for a, b in zip(seq, outs[k]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (k, kw["wa_simu"])
    assert set(tm) >= {"prepare", "solve_launch", "wait", "trphi", "finish"}
    # a small chunk size splits the launches; results do not change
    outs2 = rs.sos_spectrum(kws[:12], chunk=5)
    for a, b in zip(outs[:12], outs2):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    # ... and so does handing a chunk to the solver in parts (the solves of a part overlap the preparation of the next)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "4")
    outs3 = rs.sos_spectrum(kws, parts=3, prep_streams=5)
    for a, b in zip(outs, outs3):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.gpu
def test_sos_spectrum_writes_the_result_files_of_every_call(gpu_pkg, tmp_path, monkeypatch):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    names = ["ckd_o2a_5bins", "cfg2_lnd_lambert", "rand_03"]
    kws, golds, _, _ = spectrum_cases.build(rs, tmp_path, names=names, resroot=True)
    rs.sos_spectrum(kws)
    for kw, g in zip(kws, golds):
        d = os.path.join(kw["resroot"], "SOS")
        assert os.path.exists(os.path.join(d, "SOS_Result.bin")) and os.path.exists(os.path.join(d, "SOS_UsedAngles.txt"))
    # the -SOS.Trans file of the O2-A golden (diffuse transmissions: per-wavelength path inside sos_spectrum)
    assert os.path.exists(os.path.join(kws[0]["resroot"], "SOS", str(kws[0]["fictrans"]).strip())) or \
        str(kws[0]["fictrans"]).strip() == "NO_OUTPUT"


@pytest.mark.gpu
def test_sos_spectrum_raises_the_failing_call(gpu_pkg, tmp_path, monkeypatch):
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, _, _, _ = spectrum_cases.build(rs, tmp_path, names=["cfg1_lambert", "cfg2_lnd_lambert"])
    bad = dict(kws[0]); bad["isurf"] = 6
    with pytest.raises(rs.SosProcError):
        rs.sos_spectrum([kws[1], bad])
    out = rs.sos_spectrum([])                              # an empty spectrum is an empty list
    assert out == []


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sos_spectrum_wavelengths_over_ranks_on_one_gpu(tmp_path, world):
    """tests/dist_launch.py starts `world` ranks sharing cuda:0 (gloo): the wavelengths are dealt to the ranks by cost, each
    rank runs its own through sos_spectrum's launches, one all_gather_object -- every rank ends with the full list, equal to
    the goldens and identical across ranks; a spectrum with one refused call makes every rank raise SosProcError naming it --
    no rank is left waiting in the gather."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = str(tmp_path / "res.json")
    run_ranks("dist_spectrum_worker.py", ("--out", out), world=world, timeout=900)
    r = json.load(open(out))
    assert r["world"] == world and len(set(r["digests"])) == 1, r["digests"]
    assert sorted(i for own in r["owners"] for i in own) == list(range(r["n"]))
    assert all(len(own) > 0 for own in r["owners"])
    assert r["raised"] == [True] * world and all("wavelength 3" in m for m in r["messages"]), r["messages"]


@pytest.mark.gpu
def test_spectrum_pool_of_host_processes_equals_sos_spectrum(gpu_pkg, tmp_path, monkeypatch):
    """spectrum_pool.SpectrumPool: two worker processes on the same GPU take the wavelengths of a spectrum by cost; the 23-tuples
    that come back equal run_sos.sos_spectrum's in this process bit for bit, a second run on the same pool too, and a refused
    call raises SosProcError in the caller."""
    rs, sp = gpu_pkg.run_sos, gpu_pkg.spectrum_pool
    monkeypatch.setenv("SOS_ABS_ROOT", GOLD)
    kws, golds, coefs, rtols = spectrum_cases.build(rs, tmp_path)
    kws = kws[:30]
    ref = rs.sos_spectrum(kws)
    with sp.SpectrumPool(processes=2) as pool:
        for _ in range(2):
            outs = pool.run(kws)
            assert len(outs) == len(kws)
            for a, b in zip(ref, outs):
                for x, y in zip(a, b):
                    assert np.array_equal(np.asarray(x), np.asarray(y))
        bad = dict(kws[3])
        bad["tetas"] = 95.0
        with pytest.raises(rs.SosProcError):
            pool.run(kws[:3] + [bad] + kws[4:8])
        outs = pool.run(kws[:5])                             # the pool survives a refused spectrum
        for a, b in zip(ref[:5], outs):
            for x, y in zip(a, b):
                assert np.array_equal(np.asarray(x), np.asarray(y))
