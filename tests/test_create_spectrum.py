"""sosgpu_create_spectrum without a device: the two exports and their declarations, the work-area query as host arithmetic
(0 for every list the call would refuse, growing with the list otherwise) and the refusals of the call, which come before a
device is looked for -- so the answer here is SOSGPU_E_ARG, never SOSGPU_E_NODEVICE -- and leave every output NULL.  The
Python mirror: the keyword rule of SosContext(create=False) and the new names.  (On the device: test_create_spectrum_gpu.py.)"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_context_tables import CELLS, cell_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG = 0, -1
SENTINEL = 0xDEAD0


def spec_of(capi, name, keep, smax=None, **wave):
    """The sosgpu_ctx_spec of a cell of test_context_tables (its inputs appended to `keep`, which must outlive the spec);
    `wave`: fields of the sosgpu_wave to overwrite."""
    c, i = CELLS[name], cell_inputs(name)
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (i["mu"], i["wt"]) + tuple(i["coefs"])]
    keep.append(arrs)
    f = dict(n=len(i["mu"]), os_nb=c["os_nb"], n0=i["n0"], imat_surf=1 if c["surf"] else 0, ifresnel=c["ifresnel"],
             ipolar=c["ipolar"], igmax=100, reserved=0, ro=c["ro"], ind_surf=1.34, ron=c["ron"])
    f.update(wave)
    return capi.CtxSpec(capi.Wave(**f), *[a.ctypes.data for a in arrs], c["smax"] if smax is None else smax, 0)


def spec_array(capi, specs):
    return (capi.CtxSpec * len(specs))(*specs)


def bad_specs(capi, keep):
    """name -> a spec sosgpu_create's rules refuse (the cell n5: N = 5, OS_NB = 24)."""
    n, b = len(cell_inputs("n5")["mu"]), CELLS["n5"]["os_nb"]
    bad = {"n = 0": spec_of(capi, "n5", keep, n=0), "n = 86": spec_of(capi, "n5", keep, n=86),
           "os_nb = 1": spec_of(capi, "n5", keep, os_nb=1, smax=0), "n0 = 0": spec_of(capi, "n5", keep, n0=0),
           "n0 = n + 1": spec_of(capi, "n5", keep, n0=n + 1), "igmax = 0": spec_of(capi, "n5", keep, igmax=0),
           "iborm_max = os_nb + 1": spec_of(capi, "n5", keep, smax=b + 1)}
    for field in ("mu", "ga", "alpha", "beta", "gamma", "zeta"):
        s = spec_of(capi, "n5", keep)
        setattr(s, field, None)
        bad["NULL " + field] = s
    s = spec_of(capi, "n5", keep)
    zeros = np.zeros(n)
    keep.append(zeros)
    s.ga = zeros.ctypes.data
    bad["all weights zero"] = s
    return bad


def test_exports_and_header(pkg):
    capi = pkg.capi
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "sosgpu.h")).read()
    for sym in ("sosgpu_create_spectrum", "sosgpu_create_spectrum_work_bytes"):
        assert sym in capi.EXPORTS and hasattr(L, sym) and sym + "(" in hdr
    assert "typedef struct sosgpu_ctx_spec" in hdr
    # the structure as the header lays it out: the wave, six pointers, two int32
    assert C.sizeof(capi.CtxSpec) == C.sizeof(capi.Wave) + 6 * 8 + 8 and capi.CtxSpec.mu.offset == C.sizeof(capi.Wave)
    assert [f[0] for f in capi.CtxSpec._fields_] == ["wv", "mu", "ga", "alpha", "beta", "gamma", "zeta", "iborm_max", "reserved"]


def test_query_is_zero_for_what_the_call_refuses(pkg):
    capi = pkg.capi
    L, keep = capi.lib(), []
    good = [spec_of(capi, k, keep) for k in ("n2", "n5", "gnd_n5", "n22")]
    q = L.sosgpu_create_spectrum_work_bytes
    assert q(spec_array(capi, good), -1) == 0
    assert q(None, 3) == 0
    assert q(spec_array(capi, good), 65536) == 0
    for what, bad in bad_specs(capi, keep).items():
        assert q(spec_array(capi, [bad]), 1) == 0, what
        assert q(spec_array(capi, good[:2] + [bad] + good[2:]), 5) == 0, what


def test_query_grows_with_the_list(pkg):
    """Positive and strictly increasing in nctx; a pure function of the list (asked twice, and with a list that repeats)."""
    capi = pkg.capi
    L, keep = capi.lib(), []
    names = ["n2", "n85", "gnd_n27", "n5", "n43", "n2", "n2"]
    arr = spec_array(capi, [spec_of(capi, k, keep) for k in names])
    sizes = [L.sosgpu_create_spectrum_work_bytes(arr, n) for n in range(1, len(names) + 1)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes == [L.sosgpu_create_spectrum_work_bytes(arr, n) for n in range(1, len(names) + 1)]
    # every image starts on a multiple of 256 bytes, so the steps are such multiples
    assert all((b - a) % 256 == 0 for a, b in zip(sizes, sizes[1:])), sizes
    # the job table passes 256 entries without a change of rule
    many = spec_array(capi, [spec_of(capi, "n2", keep)] * 300)
    assert L.sosgpu_create_spectrum_work_bytes(many, 300) > L.sosgpu_create_spectrum_work_bytes(many, 256) > sizes[0]


def _call(L, specs, nctx, work, work_bytes, nout=None):
    out = (C.c_void_p * max(nout if nout is not None else nctx, 1))(*([SENTINEL] * max(nout if nout is not None else nctx, 1)))
    rc = L.sosgpu_create_spectrum(out, 0, specs, nctx, work, work_bytes, None)
    return rc, list(out)


def test_call_refuses_before_it_looks_for_a_device(pkg):
    capi = pkg.capi
    L, keep = capi.lib(), []
    good = [spec_of(capi, k, keep) for k in ("n2", "n5", "gnd_n5", "n22")]
    arr = spec_array(capi, good)
    need = L.sosgpu_create_spectrum_work_bytes(arr, 4)
    area = C.c_void_p(0x7F0000001000)            # an address that is never touched: every call below is refused on the host
    for what, bad in bad_specs(capi, keep).items():
        five = spec_array(capi, good[:2] + [bad] + good[2:])
        rc, out = _call(L, five, 5, area, 1 << 30)
        assert rc == E_ARG and out == [None] * 5, (what, rc, out)
    rc, out = _call(L, arr, 4, None, need)
    assert rc == E_ARG and out == [None] * 4                     # no work area
    rc, out = _call(L, arr, 4, C.c_void_p(area.value + 4), need + 8)
    assert rc == E_ARG and out == [None] * 4                     # a misaligned one
    rc, out = _call(L, arr, 4, area, need - 1)
    assert rc == E_ARG and out == [None] * 4                     # one byte short
    rc, out = _call(L, None, 4, area, need)
    assert rc == E_ARG and out == [None] * 4                     # no specs
    assert L.sosgpu_create_spectrum(None, 0, arr, 4, area, need, None) == E_ARG
    rc, out = _call(L, arr, -1, area, need, nout=4)
    assert rc == E_ARG and out == [SENTINEL] * 4                 # (nctx < 0: there is no output to clear)


def test_empty_list_is_accepted(pkg):
    capi = pkg.capi
    L = capi.lib()
    rc, out = _call(L, None, 0, None, 0, nout=1)
    assert rc == OK and out == [SENTINEL]
    assert L.sosgpu_create_spectrum_work_bytes(None, 0) == 0


def test_python_mirror_without_a_device(pkg):
    S = pkg.solver
    assert inspect.signature(S.SosContext.__init__).parameters["create"].default is True
    assert inspect.signature(pkg.run_sos._prepare).parameters["defer_context"].default is False
    assert S.create_contexts([]) == 0
    mu, w, n0 = pkg.synth.gauss_angles(4, 35.0)
    al, be, ga, ze = pkg.synth.hg_phase(8, 0.5)
    with pytest.raises(ValueError, match="create=False needs build=False"):
        S.SosContext(mu, w, n0, al, be, ga, ze, create=False)
    with pytest.raises(ValueError, match="create=False needs build=False"):
        S.SosContext(mu, w, n0, al, be, ga, ze, create=False, build=True)
