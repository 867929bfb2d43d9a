"""Sensor channels of a spectrum on the device (csrc/channels.hip: k_channel_accumulate, k_channel_finish; the entry points
sosgpu_channel_accumulate / sosgpu_channel_finish; solver.channel_accumulate / channel_finish).  The blocks are seeded
synthetic arrays, no solver is involved.  The reference of the sums is the host loop a = a + w * x in term order, compared
with np.array_equal; the finished rows 0..2 against the host thresholds bit for bit, rows 4..6 against oracle.polar of the
device's own rows 0..2 at the tolerances of test_surface_trphi.test_trphi_gpu_vs_oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer-sos_amd", "csrc")
E_ARG = -1
GUARD = 1024
SENTINEL = -7.25e300                              # fills the guards: a finite value no sum produces


def _ip(a):
    return a.ctypes.data_as(C.c_void_p)


def _stage_blocks(pkg):
    total, idle = C.c_int(-1), C.c_int(-1)
    assert pkg.capi.lib().sosgpu_debug_stage_blocks(0, C.byref(total), C.byref(idle)) == 0
    return total.value, idle.value


# ---------------------------------------------------------------------------------------------------------------- CPU tests


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    assert re.search(r"\bsize_t\s+sosgpu_channel_accumulate_work_bytes\s*\(int nchan, int nterms\);", hdr)
    assert re.search(r"\bint\s+sosgpu_channel_accumulate\s*\(int device, const double \*d_blocks, int njobs, int nslots, int nphi, "
                     r"int w, int nchan,\s*const int32_t \*first, const int32_t \*job, const double \*wgt, double \*d_acc, "
                     r"void \*d_work,\s*size_t work_bytes, void \*stream\);", hdr)
    assert re.search(r"\bint\s+sosgpu_channel_finish\s*\(int device, const double \*d_acc, const double \*d_angdiff_block, int nchan, "
                     r"int nslots, int nphi,\s*int w, double \*d_out, void \*stream\);", hdr)
    L = pkg.capi.lib()
    for sym, nargs in (("sosgpu_channel_accumulate", 14), ("sosgpu_channel_accumulate_work_bytes", 2),
                       ("sosgpu_channel_finish", 9)):
        assert sym in pkg.capi.EXPORTS
        assert len(getattr(L, sym).argtypes) == nargs, sym
    assert callable(pkg.solver.channel_accumulate) and callable(pkg.solver.channel_finish)
    assert callable(pkg.run_sos.sos_spectrum_channels)


def test_work_bytes(pkg):
    f = pkg.capi.lib().sosgpu_channel_accumulate_work_bytes
    assert f(0, 5) == 0 and f(3, -1) == 0
    for nchan, nterms in ((1, 0), (1, 1), (3, 7), (16, 2496), (65535, 1)):
        n = f(nchan, nterms)
        assert n % 8 == 0 and 0 <= n - (12 * nterms + 4 * (nchan + 1)) < 8, (nchan, nterms, n)


def _good_call():
    """Arguments of a valid sosgpu_channel_accumulate call of 2 channels and 3 terms on 4 jobs; the device pointers are never
    dereferenced: the calls made with them are refused before anything is queued."""
    p = C.c_void_p(4096)
    return dict(device=0, d_blocks=p, njobs=4, nslots=2, nphi=2, w=5, nchan=2, first=np.array([0, 2, 3], dtype=np.int32),
                job=np.array([0, 3, 1], dtype=np.int32), wgt=np.array([0.5, -0.25, 1.0]), d_acc=p, d_work=p, work_bytes=48,
                stream=None)


def _accumulate(pkg, a):
    host = lambda x: None if x is None else _ip(x)
    return pkg.capi.lib().sosgpu_channel_accumulate(a["device"], a["d_blocks"], a["njobs"], a["nslots"], a["nphi"], a["w"],
                                                    a["nchan"], host(a["first"]), host(a["job"]), host(a["wgt"]), a["d_acc"],
                                                    a["d_work"], a["work_bytes"], a["stream"])


ACC_REFUSALS = {
    "njobs 0": dict(njobs=0), "nslots 0": dict(nslots=0), "nphi 0": dict(nphi=0), "w 0": dict(w=0), "nchan 0": dict(nchan=0),
    "nslots 65536": dict(nslots=65536),
    "first from 1": dict(first=np.array([1, 2, 3], dtype=np.int32)),
    "first decreasing": dict(first=np.array([0, 3, 2], dtype=np.int32)),
    "job -1": dict(job=np.array([0, -1, 1], dtype=np.int32)),
    "job njobs": dict(job=np.array([0, 3, 4], dtype=np.int32)),
    "weight nan": dict(wgt=np.array([0.5, np.nan, 1.0])),
    "weight inf": dict(wgt=np.array([0.5, -0.25, np.inf])),
    "null blocks": dict(d_blocks=None), "null first": dict(first=None), "null job": dict(job=None), "null wgt": dict(wgt=None),
    "null acc": dict(d_acc=None), "null work": dict(d_work=None),
    "work misaligned": dict(d_work=C.c_void_p(4100)),
    "work too small": dict(work_bytes=47),
}


def test_accumulate_refusals_take_no_staging_block(pkg):
    """Every refusal of sosgpu_channel_accumulate returns SOSGPU_E_ARG before a device is looked for, and the count of staging
    blocks (sosgpu_debug_stage_blocks) is what it was; a call without a term is accepted with nothing queued."""
    assert pkg.capi.lib().sosgpu_channel_accumulate_work_bytes(2, 3) == 48
    before = _stage_blocks(pkg)
    for what, change in ACC_REFUSALS.items():
        assert _accumulate(pkg, dict(_good_call(), **change)) == E_ARG, what
        assert _stage_blocks(pkg) == before, what
    empty = dict(_good_call(), first=np.zeros(3, dtype=np.int32), work_bytes=16)
    assert _accumulate(pkg, empty) == 0
    assert _stage_blocks(pkg) == before


def test_finish_refusals(pkg):
    L = pkg.capi.lib()
    p = C.c_void_p(4096)
    good = [0, p, p, 2, 2, 2, 5, p, None]
    before = _stage_blocks(pkg)
    for pos, bad in ((1, None), (2, None), (7, None), (3, 0), (4, 0), (5, 0), (6, 4), (6, 1), (3, 65536), (4, 65536)):
        a = list(good)
        a[pos] = bad
        assert L.sosgpu_channel_finish(*a) == E_ARG, (pos, bad)
        assert _stage_blocks(pkg) == before


def test_kernels_cross_compile_for_gfx950(tmp_path):
    """csrc/channels.hip compiles for gfx950 without a device; in the assembly of k_channel_accumulate the term table comes in
    by scalar loads, the sum is a multiply and an add (no fused multiply-add), and the accumulator element is loaded once and
    stored once (two vector loads in all: the element and the term's block element)."""
    out = str(tmp_path / "channels.s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-S",
                           os.path.join(CSRC, "channels.hip"), "-o", out], cwd=CSRC, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    bodies = {}
    for name in ("k_channel_accumulate", "k_channel_finish"):
        m = re.search(r"^(_Z\d+%s\w*):[^\n]*\n(.*?)s_endpgm" % name, asm, re.S | re.M)
        assert m, name
        bodies[name] = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
    acc = [ln for ln in bodies["k_channel_accumulate"] if ln]
    count = lambda pat: sum(1 for ln in acc if re.match(pat, ln))
    assert count(r"v_fma_f64|v_fmac_f64") == 0
    assert count(r"v_mul_f64") == 1 and count(r"v_add_f64") == 1
    assert count(r"global_load_dwordx2") == 2 and count(r"global_store_dwordx2") == 1
    assert count(r"global_load|flat_load|buffer_load") == 2
    assert count(r"s_load_dword") >= 4                      # kernel arguments, first[c] | first[c + 1], job[m], wgt[m]
    assert any(re.match(r"global_store_dwordx2", ln) for ln in bodies["k_channel_finish"])


# ---------------------------------------------------------------------------------------------------------------- GPU tests


def host_accumulate(acc, blocks, first, job, wgt):
    """acc[c] = acc[c] + wgt[m] * blocks[job[m]][:, :, :3] for the terms of every channel in term order: one rounded product
    and one rounded sum per step (numpy forms them as two operations)."""
    acc = acc.copy()
    for c in range(len(first) - 1):
        a = acc[c]
        for m in range(first[c], first[c + 1]):
            a = a + wgt[m] * blocks[job[m], :, :, :3, :]
        acc[c] = a
    return acc


def make_blocks(rng, njobs, K, nphi, W):
    """[njobs][K][nphi][7][W] of mixed sign and magnitude; rows 3..6 hold NaN: a kernel that reads them shows it."""
    b = rng.standard_normal((njobs, K, nphi, 7, W)) * 10.0 ** rng.integers(-6, 3, size=(njobs, K, nphi, 7, 1))
    b[:, :, :, 3:, :] = np.nan
    return b


def make_terms(rng, nchan, njobs):
    """C = 1: one channel with every job in ascending order.  C = 3: channel 0 names every job in shuffled order, some weights
    negative; channel 1 has no term; channel 2 shares every other job (and the last) with channel 0, one weight negative."""
    if nchan == 1:
        return np.array([0, njobs], dtype=np.int32), np.arange(njobs, dtype=np.int32), rng.uniform(0.1, 2.0, njobs)
    assert nchan == 3
    j0 = rng.permutation(njobs).astype(np.int32)
    w0 = rng.uniform(0.1, 2.0, njobs) * np.where(rng.random(njobs) < 0.3, -1.0, 1.0)
    w0[0] = -abs(w0[0])
    j2 = np.unique(np.concatenate([np.arange(0, njobs, 2), [njobs - 1]])).astype(np.int32)[::-1].copy()
    w2 = rng.uniform(0.1, 2.0, j2.size)
    w2[-1] = -w2[-1]
    first = np.array([0, njobs, njobs, njobs + j2.size], dtype=np.int32)
    return first, np.concatenate([j0, j2]), np.concatenate([w0, w2])


class Device:
    """Blocks and accumulator on the device, each followed by a guard; acc starts from seeded non-zero values."""

    def __init__(self, rng, blocks, nchan):
        import torch
        self.njobs, self.K, self.nphi, _, self.W = blocks.shape
        self.nchan = nchan
        self.acc0 = rng.standard_normal((nchan, self.K, self.nphi, 3, self.W))
        guard = np.full(GUARD, SENTINEL)
        self.d_blocks = torch.from_numpy(np.concatenate([blocks.reshape(-1), guard])).cuda()
        self.d_acc = torch.from_numpy(np.concatenate([self.acc0.reshape(-1), guard])).cuda()
        self.nb, self.na = blocks.size, self.acc0.size
        self.blocks_bits = self.d_blocks.clone()

    def reset(self):
        import torch
        self.d_acc[:self.na] = torch.from_numpy(self.acc0.reshape(-1)).cuda()

    def acc(self):
        return self.d_acc[:self.na].view(self.nchan, self.K, self.nphi, 3, self.W)

    def accumulate(self, pkg, first, job, wgt):
        pkg.solver.channel_accumulate(self.d_blocks[:self.nb], self.njobs, self.K, self.nphi, self.W, first, job, wgt, self.acc())

    def check_guards(self):
        import torch
        assert bool((self.d_acc[self.na:] == SENTINEL).all()), "guard behind acc"
        a, b = self.d_blocks.view(torch.int64), self.blocks_bits.view(torch.int64)
        assert torch.equal(a, b), "blocks or their guard were written"


JOB_COUNTS = (1, 31, 32, 33, 65)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("nphi", [1, 2, 7])
@pytest.mark.parametrize("W", [5, 171])
def test_accumulate_equals_the_host_loop_bitwise(gpu_pkg, W, nphi, K):
    """1, 31, 32, 33 and 65 jobs, C = 1 (every job ascending) and C = 3 (shuffled term order with negative weights, a channel
    without a term, a channel sharing jobs): the accumulator equals the host loop bit for bit; the part of the channel without a
    term keeps its previous bits; rows 3..6 of the blocks are NaN; the guards behind acc and behind the blocks are untouched.
    A second round (recycled staging blocks) gives the same bits on as many blocks."""
    import torch
    rng = np.random.default_rng(1000 * W + 10 * nphi + K)
    for njobs in JOB_COUNTS:
        blocks = make_blocks(rng, njobs, K, nphi, W)
        for nchan in (1, 3):
            first, job, wgt = make_terms(rng, nchan, njobs)
            dev = Device(rng, blocks, nchan)
            ref = host_accumulate(dev.acc0, blocks, first, job, wgt)
            assert not np.isnan(ref).any()
            dev.accumulate(gpu_pkg, first, job, wgt)
            got = dev.acc().cpu().numpy()
            assert np.array_equal(got, ref), (njobs, nchan, int((got != ref).sum()))
            if nchan == 3:
                assert np.array_equal(got[1].view(np.int64), dev.acc0[1].view(np.int64))
                if njobs > 1:                               # (the shuffle is seeded: it is not the ascending order)
                    assert (wgt < 0).any() and not np.array_equal(job[:njobs], np.sort(job[:njobs]))
            dev.check_guards()
            held = _stage_blocks(gpu_pkg)[0]
            dev.reset()
            dev.accumulate(gpu_pkg, first, job, wgt)
            assert torch.equal(dev.acc().cpu(), torch.from_numpy(ref)), (njobs, nchan, "second round")
            assert _stage_blocks(gpu_pkg)[0] == held >= 1
            dev.check_guards()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [5, 171])
def test_split_calls_give_the_bits_of_one_call(gpu_pkg, W):
    """The terms of three channels on 33 jobs (K = 3, nphi = 2) in one call, and cut at every position of the term list into
    two successive calls on the same accumulator: equal bits, and equal to the host loop."""
    import torch
    rng = np.random.default_rng(77 + W)
    njobs, K, nphi = 33, 3, 2
    blocks = make_blocks(rng, njobs, K, nphi, W)
    first, job, wgt = make_terms(rng, 3, njobs)
    dev = Device(rng, blocks, 3)
    dev.accumulate(gpu_pkg, first, job, wgt)
    one = dev.acc().clone()
    assert np.array_equal(one.cpu().numpy(), host_accumulate(dev.acc0, blocks, first, job, wgt))
    nterms = int(first[-1])
    bad = []
    for s in range(nterms + 1):
        dev.reset()
        f1 = np.minimum(first, s).astype(np.int32)
        f2 = (np.maximum(first, s) - s).astype(np.int32)
        dev.accumulate(gpu_pkg, f1, job[:s], wgt[:s])
        dev.accumulate(gpu_pkg, f2, job[s:], wgt[s:])
        if not torch.equal(dev.acc(), one):
            bad.append(s)
    assert not bad, bad
    dev.check_guards()


@pytest.mark.gpu
def test_a_refusal_on_a_warm_library_takes_no_block(gpu_pkg):
    """After a valid call (the library holds a staging block) a refused one leaves total and idle as they were and the
    accumulator untouched."""
    import torch
    rng = np.random.default_rng(5)
    blocks = make_blocks(rng, 4, 1, 1, 5)
    first, job, wgt = make_terms(rng, 1, 4)
    dev = Device(rng, blocks, 1)
    dev.accumulate(gpu_pkg, first, job, wgt)
    torch.cuda.synchronize()
    before, bits = _stage_blocks(gpu_pkg), dev.d_acc.clone()
    assert before[0] >= 1
    with pytest.raises(gpu_pkg.capi.SosgpuError):
        dev.accumulate(gpu_pkg, first, np.array([0, 1, 2, 4], dtype=np.int32), wgt)
    with pytest.raises(gpu_pkg.capi.SosgpuError):
        dev.accumulate(gpu_pkg, first, job, np.array([1.0, np.inf, 1.0, 1.0]))
    torch.cuda.synchronize()
    assert _stage_blocks(gpu_pkg) == before
    assert torch.equal(dev.d_acc.view(torch.int64), bits.view(torch.int64))


def host_thresholds(acc):
    """SOS_TRPHI.F:1212-1218 on [..][3][W] sums."""
    out = acc.copy()
    i, q, u = out[..., 0, :], out[..., 1, :], out[..., 2, :]
    i[i <= 1e-99] = 0.0
    q[np.abs(q) < 1e-15] = 0.0
    u[np.abs(u) < 1e-15] = 0.0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W", [5, 171])
def test_finish(gpu_pkg, oracle, W):
    """C = 2, K = 2, nphi = 2: rows 0..2 equal the host thresholds bit for bit, with accumulators planted so that each fires
    (I = 1e-100; |Q| = 5e-16 beside a U above the threshold, of both signs; Q = U = 0; I = 0 beside a polarised Q, U); row 3 is
    the block handed in (whose other rows are NaN); rows 4..6 agree with oracle.polar of the device's rows 0..2 at
    test_trphi_gpu_vs_oracle's tolerances, the -999 of an undefined angle and of an undefined rate among them; direction 0 is
    zero in every row; the accumulator is left as it was."""
    import torch
    rng = np.random.default_rng(31 + W)
    nchan, K, nphi, N = 2, 2, 2, (W - 1) // 2
    acc = rng.standard_normal((nchan, K, nphi, 3, W)) * 10.0 ** rng.integers(-4, 2, size=(nchan, K, nphi, 3, 1))
    acc[..., 0, :] = np.abs(acc[..., 0, :])
    acc[0, 0, 0, :, 0] = (1e-100, 0.3, -0.2)              # I under its threshold: 0, rate undefined
    acc[0, 0, 0, :, 1] = (2.0, 5e-16, 0.25)               # Q under its threshold, U > 0: angle 45
    acc[0, 1, 1, :, 1] = (2.0, -5e-16, -0.25)             # ... U < 0: angle -45
    acc[1, 0, 1, :, W - 1] = (1.5, 0.0, 0.0)              # unpolarised: angle undefined
    acc[1, 1, 0, :, W - 2] = (0.0, 0.1, 0.1)              # no intensity: rate undefined
    acc[1, 1, 1, :, 0] = (1.0, -0.3, 0.3)                 # second quadrant
    acc[1, 1, 1, :, 1] = (1.0, -0.3, -0.3)                # third quadrant
    block = np.full((nphi, 7, W), np.nan)
    block[:, 3, :] = rng.uniform(0.0, 180.0, (nphi, W))
    block[:, 3, N] = 0.0
    d_acc = torch.from_numpy(acc).cuda()
    out_t = gpu_pkg.solver.channel_finish(d_acc, torch.from_numpy(block).cuda())
    out = out_t.cpu().numpy()
    assert out.shape == (nchan, K, nphi, 7, W) and not np.isnan(out).any()
    assert torch.equal(d_acc.cpu(), torch.from_numpy(acc))
    ref = host_thresholds(acc)
    ref[..., N] = 0.0
    assert np.array_equal(out[..., :3, :], ref)
    assert out[0, 0, 0, 0, 0] == 0.0 and out[0, 0, 0, 1, 1] == 0.0 and out[0, 1, 1, 1, 1] == 0.0
    assert np.array_equal(out[..., 3, :], np.broadcast_to(block[:, 3, :], (nchan, K, nphi, W)))
    assert np.array_equal(out[..., N], np.zeros((nchan, K, nphi, 7)))
    seen = set()
    for c in range(nchan):
        for k in range(K):
            for p in range(nphi):
                for t in list(range(N)) + list(range(N + 1, W)):
                    xan, tpol, lpol = oracle.polar(out[c, k, p, 0, t], out[c, k, p, 1, t], out[c, k, p, 2, t])
                    where = (c, k, p, t)
                    assert abs(out[c, k, p, 4, t] - xan) <= 1e-9 * max(1.0, abs(xan)), where
                    assert abs(out[c, k, p, 5, t] - tpol) <= 1e-9 * max(1.0, abs(tpol)), where
                    assert abs(out[c, k, p, 6, t] - lpol) <= 1e-12 + 1e-9 * abs(lpol), where
                    seen.add((xan == -999.0, tpol == -999.0))
    assert seen == {(False, False), (True, False), (False, True)}
    assert out[0, 0, 0, 4, 1] == 45.0 and out[0, 1, 1, 4, 1] == -45.0 and out[1, 0, 1, 4, W - 1] == -999.0
    assert out[0, 0, 0, 5, 0] == -999.0 and out[1, 1, 0, 5, W - 2] == -999.0
    assert out[1, 1, 1, 4, 0] > 45.0 and out[1, 1, 1, 4, 1] < -45.0
