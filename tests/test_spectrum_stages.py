"""The decisions of run_sos._spectrum_pass that need no device, as the functions its stages call: the part boundaries of a
chunk, which calls share a launch, the sections of the chunk's packed scalar download, the channel terms, and the cut of a
flat array into blocks (solver._flat_blocks).  Every reference below is the inline code of the pass as it stood before the
stages were cut out, transcribed verbatim; none is the function under test.  No library, no GPU."""
import collections
import json
import os
import types

import numpy as np
import pytest
import torch

import spectrum_cases

NS = types.SimpleNamespace


# ---------------------------------------------------------------------------------------------------- part boundaries
def _parts_before(idx, parts):
    out = []
    nsub = max(1, min(int(parts), len(idx) // max(1, int(os.environ.get("SOS_SPECTRUM_MIN_PART", "32")))))
    step = max(1, -(-len(idx) // nsub))
    for s0 in range(0, len(idx), step):
        out.append(idx[s0:s0 + step])
    return out


@pytest.mark.parametrize("min_part", [1, 2, 32])
@pytest.mark.parametrize("parts", [1, 4])
def test_part_bounds_tile_the_chunk_as_before(pkg, monkeypatch, parts, min_part):
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", str(min_part))
    for n in range(1, 71):
        idx = list(range(100, 100 + n))
        pairs = pkg.run_sos._part_bounds(n, parts, min_part)
        assert [idx[s0:s1] for s0, s1 in pairs] == _parts_before(idx, parts)
        assert pairs[0][0] == 0 and pairs[-1][1] == n and all(s0 < s1 for s0, s1 in pairs)
        assert [p[1] for p in pairs[:-1]] == [p[0] for p in pairs[1:]]          # they tile range(n)
        assert len(pairs) <= parts


# ---------------------------------------------------------------------------------------------------- grouping
def _groups_before(part):
    groups = collections.OrderedDict()
    single = []
    launches = []
    for pl in part:
        b = pl.bins
        if pl.tdifmug is not None or b["nb"] == 0 or not isinstance(b.get("scal"), torch.Tensor) or pl.host_scal:
            single.append(pl)
            continue
        # (the last entry is False throughout with output slots: their calls have zout = -1)
        key = (pl.n, pl.ctx.smax, pl.ctx.os_nb, bool(pl.ctx._rsurf is not None), b["lp"], b["jout"] is not None)
        groups.setdefault(key, []).append(pl)
    for key, gp in groups.items():
        if len(gp) == 1:
            single.append(gp[0])
            continue
        launches.append(gp)
    return launches, single


def _plan(index, n=13, smax=40, os_nb=80, rsurf=None, nb=5, lp=30, jout=None, scal="tensor", tdifmug=None, host_scal=False):
    scal = torch.zeros((nb, 4), dtype=torch.float64) if scal == "tensor" else np.zeros((nb, 4))
    return NS(index=index, n=n, ctx=NS(smax=smax, os_nb=os_nb, _rsurf=rsurf), tdifmug=tdifmug, host_scal=host_scal,
              bins=dict(nb=nb, lp=lp, jout=jout, scal=scal))


def test_grouping_keeps_the_order_of_the_launches(pkg):
    """Two keys of two plans, a one-member key and one plan for each of the four reasons to solve a call alone: nine plans
    (each reason needs a plan of its own), pinned whole and as its two parts of eight."""
    part = [_plan(0, lp=31),                                    # a one-member key, met first
            _plan(1),                                           # key A
            _plan(2, tdifmug=torch.zeros((5, 13))),             # its own transmissions
            _plan(3, rsurf=torch.zeros(1)),                     # key B
            _plan(4, nb=0),                                     # no bins
            _plan(5),                                           # key A
            _plan(6, scal="numpy"),                             # host scalars
            _plan(7, rsurf=torch.zeros(1)),                     # key B
            _plan(8, host_scal=True)]                           # a host profile whose scalars were uploaded
    groups, single = pkg.run_sos._part_groups(part)
    assert [[pl.index for pl in gp] for gp in groups] == [[1, 5], [3, 7]]
    assert [pl.index for pl in single] == [2, 4, 6, 8, 0]
    groups, single = pkg.run_sos._part_groups(part[:8])
    assert [[pl.index for pl in gp] for gp in groups] == [[1, 5], [3, 7]]
    assert [pl.index for pl in single] == [2, 4, 6, 0]
    groups, single = pkg.run_sos._part_groups(part[1:])
    assert [[pl.index for pl in gp] for gp in groups] == [[1, 5], [3, 7]]
    assert [pl.index for pl in single] == [2, 4, 6, 8]
    for members in (part[:8], part[1:], part, part[::-1], part[:1], []):
        want, got = _groups_before(members), pkg.run_sos._part_groups(members)
        assert [[id(pl) for pl in gp] for gp in got[0]] == [[id(pl) for pl in gp] for gp in want[0]]
        assert [id(pl) for pl in got[1]] == [id(pl) for pl in want[1]]
    # every entry of the key separates: two plans that differ in one of them do not share a launch
    for other in (dict(n=14), dict(smax=41), dict(os_nb=81), dict(rsurf=torch.zeros(1)), dict(lp=29), dict(jout=torch.zeros(1))):
        groups, single = pkg.run_sos._part_groups([_plan(0), _plan(1, **other)])
        assert groups == [] and [pl.index for pl in single] == [0, 1], other


# ---------------------------------------------------------------------------------------------------- packed download
def _sections_before(scal_all, nz, solved, salb_bands, ckd_checks):
    status = []
    pos = scal_all.size - sum(len(pls) for _, pls in ckd_checks)
    for _, pls in ckd_checks:
        status.append(scal_all[pos:pos + len(pls)])
        pos += len(pls)
    albs, pos = [], sum(s.numel() for _, _, s, _ in solved)
    for gp, _ in salb_bands:
        albs.append(scal_all[pos:pos + len(gp)])
        pos += len(gp)
    blocks, pos = [], 0
    for gp, rec, scal, _ in solved:
        sw = scal.shape[2]
        blk = scal_all[pos:pos + nz * len(gp) * sw].reshape(nz, len(gp), sw)
        pos += nz * len(gp) * sw
        blocks.append(blk)
    return blocks, albs, status


def _chunk(nz, with_albedo, with_status):
    """A chunk whose download is arange(total): two solved entries (3 calls of 23 scalars, 1 call of 17), two albedo groups
    and two status groups, each rider list empty on request.  CPU tensors; the status words are int32 as the device's are."""
    pos = [0]

    def take(shape, dtype=torch.float64):
        m = int(np.prod(shape))
        t = torch.arange(pos[0], pos[0] + m, dtype=dtype).reshape(shape)
        pos[0] += m
        return t

    solved = [(["a", "b", "c"], None, take((nz, 3, 23)), None), (["d"], None, take((nz, 1, 17)), None)]
    salb = [(["a", "b"], take((2,))), (["c"], take((1,)))] if with_albedo else []
    ckd = [(take((1,), torch.int32), ["b"]), (take((3,), torch.int32), ["a", "c", "d"])] if with_status else []
    return NS(solved=solved, salb_bands=salb, ckd_checks=ckd, plans=[], where=-1), pos[0]


@pytest.mark.parametrize("with_status", [True, False])
@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("nz", [1, 3])
def test_download_sections_are_the_slices_read_before(pkg, nz, with_albedo, with_status):
    rs = pkg.run_sos
    ch, total = _chunk(nz, with_albedo, with_status)
    scal_all = np.arange(total, dtype=np.float64)
    want = _sections_before(scal_all, nz, ch.solved, ch.salb_bands, ch.ckd_checks)
    shapes = [(nz, 3, 23), (nz, 1, 17)]
    for got in (rs._download_scalars(ch, nz),
                rs._split_scalars(scal_all, shapes, [2, 1] if with_albedo else [], [1, 3] if with_status else [])):
        assert [len(x) for x in got] == [len(x) for x in want] == [2, 2 * with_albedo, 2 * with_status]
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                assert x.shape == y.shape and x.dtype == np.float64 and np.array_equal(x, y)
        # the stated order: blocks, albedos, status words, back to back -- one arange
        assert np.array_equal(np.concatenate([x.reshape(-1) for sec in got for x in sec]), scal_all)
    assert [b.shape for b in got[0]] == shapes
    assert all(np.shares_memory(x, scal_all) for sec in got for x in sec)      # (cut from scal_all itself: views)


@pytest.mark.parametrize("off", [-1, 1])
def test_download_sizes_that_do_not_add_up_are_refused(pkg, off):
    rs = pkg.run_sos
    scal_all = np.arange(3 * 23 + 17 + 3 + 4 + off, dtype=np.float64)
    with pytest.raises(ValueError, match="packed scalars"):
        rs._split_scalars(scal_all, [(1, 3, 23), (1, 1, 17)], [2, 1], [1, 3])
    with pytest.raises(ValueError, match="packed scalars"):
        rs._split_scalars(np.arange(5.0), [], [], [4])


# ---------------------------------------------------------------------------------------------------- channel terms
def _terms_before(chan, nz, todo):
    n_chan = chan.shape[0]
    job_of = {todo[j * nz][0].index: j for j in range(len(todo) // nz)}
    calls = sorted(job_of)
    first, job, wgt = [0], [], []
    for c in range(n_chan):
        for i in calls:
            if chan[c, i] != 0.0:
                job.append(job_of[i])
                wgt.append(chan[c, i])
        first.append(len(job))
    return len(calls), first, job, wgt


@pytest.mark.parametrize("nz", [1, 2])
def test_channel_terms_name_the_calls_in_ascending_index(pkg, nz):
    order = [7, 2, 9, 4, 3]                                     # the calls of the chunk in job order (group order)
    chan = np.zeros((3, 12))
    chan[0, [2, 3, 4, 7, 9]] = [0.5, 0.25, 0.125, 0.0625, 0.03125]
    chan[1, [9, 7, 4]] = [0.3, 0.0, 0.7]                        # one zero weight, two calls not named
    chan[2, [3]] = [1.0]
    chan[:, [0, 11]] = 0.9                                      # calls of other chunks
    todo = [(NS(index=i), k, None, None, 0) for i in order for k in range(nz)]
    ncalls, first, job, wgt = pkg.run_sos._channel_terms(chan, nz, [t[0].index for t in todo])
    assert (ncalls, first, job, wgt) == _terms_before(chan, nz, todo)
    assert ncalls == 5 and first == [0, 5, 7, 8]
    assert job == [1, 4, 3, 0, 2, 3, 2, 4] and wgt == [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.7, 0.3, 1.0]
    for c in range(3):
        calls = [order[j] for j in job[first[c]:first[c + 1]]]
        assert calls == sorted(calls) and len(set(calls)) == len(calls)


# ---------------------------------------------------------------------------------------------------- flat blocks
SHAPES = [(2, 7, 27), (1, 7, 27), (3, 7, 41), (1, 1), (5,)]


def _blocks_before_band(flat, shapes):                         # run_sos._band_call
    outs, pos = [], 0
    for shp in shapes:
        outs.append(flat[pos:pos + int(np.prod(shp))].reshape(shp))
        pos += outs[-1].size
    return outs


def _blocks_before_pass(flat, shapes):                         # run_sos._spectrum_pass (three-dimensional blocks)
    outs, pos = [], 0
    for shp in shapes:
        cnt = shp[0] * shp[1] * shp[2]
        outs.append(flat[pos:pos + cnt].reshape(shp))
        pos += cnt
    return outs


def _blocks_before_trphi(flat, shapes):                        # solver.trphi_many (three-dimensional blocks, a tensor)
    views, pos = [], 0
    for shp in shapes:
        m = shp[0] * shp[1] * shp[2]
        views.append(flat[pos:pos + m].view(shp))
        pos += m
    return views


def test_flat_blocks_are_views_in_order(pkg):
    cut = pkg.solver._flat_blocks
    total = sum(int(np.prod(s)) for s in SHAPES)
    flat = np.arange(total + 3, dtype=np.float64)              # (a tail nobody claims is left alone)
    got = cut(flat, SHAPES)
    for a, b in zip(got, _blocks_before_band(flat, SHAPES)):
        assert a.shape == b.shape and np.array_equal(a, b)
    for a, b in zip(cut(flat, SHAPES[:3]), _blocks_before_pass(flat, SHAPES[:3])):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert len(got) == len(SHAPES) and all(np.shares_memory(a, flat) for a in got)
    got[2][0, 0, 0] = -1.0
    assert flat[3 * 7 * 27] == -1.0
    t = torch.arange(total, dtype=torch.float64)
    views = cut(t, SHAPES)
    for a, b in zip(cut(t, SHAPES[:3]), _blocks_before_trphi(t, SHAPES[:3])):
        assert a.shape == b.shape and torch.equal(a, b) and a.data_ptr() == b.data_ptr()
    assert [tuple(v.shape) for v in views] == SHAPES
    assert all(v.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for v in views)
    views[3][0, 0] = -2.0
    assert t[3 * 7 * 27 + 3 * 7 * 41] == -2.0
    assert cut(flat, []) == [] and cut(t, []) == []


# ---------------------------------------------------------------------------------------------------- every stage in one pass
ALTS = [-1, 2.0]
O2A = {"-SOS_Main.Wa": 0.762, "-AP.AbsProfile.Type": 2, "-AP.SpectralResol": 10.0}     # the 5-bin band of ckd_o2a_5bins


def _six_calls(rs):
    """Six calls on two fixed goldens of 12 Gauss angles (N = 13): a Lambert pair and a Roujean pair in the O2 A band, which
    group; the no-gas Lambert golden as it is; and that call with the -SOS.Trans option."""
    def call(name, **more):
        g = np.load(os.path.join(spectrum_cases.GOLD, "sos_proc_%s.npz" % name))
        user = dict(json.loads(str(g["user_json"])), **{"-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT"})
        user.update(more)
        return dict(rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False), zout=-1.0)

    return [call("nopolar_polar", **O2A), call("nopolar_polar", **dict(O2A, **{"-SURF.Alb": 0.1})),
            call("nopolar_polar"), call("nopolar_polar", **{"-SOS.Trans": "SOS_Transm.txt"}),
            call("land_roujean", **O2A), call("land_roujean", **dict(O2A, **{"-SURF.Roujean.K0": 0.3}))]


@pytest.mark.gpu
def test_every_stage_in_one_pass_equals_the_calls_one_by_one(gpu_pkg, monkeypatch):
    """sos_spectrum_levels at two altitudes with chunk=4, parts=2 and parts of two calls, with fluxes, split, transmissions and
    spherical_albedo, against sos_proc_levels call by call, bit for bit; the trans entries and s_alb against the passes that
    ask for one keyword at a time (the calls of test_spectrum_transmissions and test_spectrum_albedo, default chunk).
    transmissions=True refuses a call with the -SOS.Trans option (checked here too, the text unchanged), so that call goes
    through the pass twice: as it is with fluxes and split -- its own per-direction transmissions ride its aggregate, the
    branch of the single solves no other call takes -- and with the option at NO_OUTPUT under all four keywords."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    monkeypatch.setenv("SOS_SPECTRUM_MIN_PART", "2")
    with_file = _six_calls(rs)
    kws = [dict(kw, fictrans="NO_OUTPUT") for kw in with_file]
    assert [int(kw["absprofil"]) for kw in kws] == [2, 2, 7, 7, 2, 2] and [int(kw["isurf"]) for kw in kws] == [0, 0, 0, 0, 3, 3]
    assert [kw["fictrans"] != "NO_OUTPUT" for kw in with_file] == [False, False, False, True, False, False]
    want = [rs.sos_proc_levels(ALTS, fluxes=True, split=True, **kw) for kw in with_file]
    want_off = rs.sos_proc_levels(ALTS, fluxes=True, split=True, **kws[3])
    assert all(int(t[0]) == 13 for tuples, _ in want for t in tuples)

    def same(spec, flux, tuples, rows):
        assert flux.shape == (2, 7) and np.array_equal(flux, rows)
        for k in range(2):
            assert len(spec[k]) == len(tuples[k]) == 23
            for x, y in zip(spec[k], tuples[k]):
                assert np.array_equal(np.asarray(x), np.asarray(y))

    groups = []
    real = gpu_pkg.solver.solve_spectrum_levels

    def counted(table, bins, *a, **k):
        groups.append(int(bins["nb"]))
        return real(table, bins, *a, **k)

    monkeypatch.setattr(gpu_pkg.solver, "solve_spectrum_levels", counted)
    with pytest.raises(ValueError, match="call 3 asks for the -SOS.Trans file"):
        rs.sos_spectrum_levels(ALTS, with_file, chunk=4, parts=2, fluxes=True, split=True, transmissions=True,
                               spherical_albedo=True)
    tm = {}
    spec, flux = rs.sos_spectrum_levels(ALTS, with_file, chunk=4, parts=2, fluxes=True, split=True, timings=tm)
    assert groups == [10, 10]                                   # the two pairs, five bins a call
    for i in range(6):
        same(spec[i], flux[i], *want[i])
    del groups[:]
    spec, flux, trans = rs.sos_spectrum_levels(ALTS, kws, chunk=4, parts=2, fluxes=True, split=True, transmissions=True,
                                               spherical_albedo=True, timings=tm)
    assert groups == [10, 2, 10]                                # (the two no-gas calls are a pair now)
    assert set(tm) == {"prepare", "solve_launch", "wait", "trphi", "finish", "fluxes"}
    for i in range(6):
        same(spec[i], flux[i], *(want_off if i == 3 else want[i]))
    monkeypatch.setattr(gpu_pkg.solver, "solve_spectrum_levels", real)
    _, trans_kw = rs.sos_spectrum(kws, transmissions=True)
    _, salb_kw = rs.sos_spectrum(kws, transmissions=True, spherical_albedo=True)
    keys = ("thetas", "thetav", "ttot_tronc", "ttot_vrai", "tdifmus", "tdifmug", "t_dir_down", "t_dif_down", "t_dif_up")
    for t, a, b in zip(trans, trans_kw, salb_kw):
        assert set(t) == set(keys) | {"s_alb"} == set(b) and set(a) == set(keys)
        for k in keys:
            assert np.array_equal(np.asarray(t[k]), np.asarray(a[k])), k
        assert t["s_alb"] == b["s_alb"] and 0.0 < t["s_alb"] < 1.0
