"""Synthetic cells for tests/test_ckd_device.py: wavelengths of sosgpu_ckd_layer_tables with axes, tables and layer states made
in the test, the checker (absorption.coeff_abs_ckd called per layer, gas and term) and the call through the C ABI."""
import ctypes as C

import numpy as np


def axes(nt, npr, nc):
    """Ascending axes of the given lengths: temperatures from 160 to 320 K (the 9-point axis is the reference's, 20 K steps),
    pressures geometric from 0.1 to 1050 hPa, concentrations geometric from 1e-6 to 0.05."""
    return (np.linspace(160.0, 320.0, nt), np.geomspace(0.1, 1050.0, npr), np.geomspace(1e-6, 0.05, nc))


def smooth_table(rng, shape, scale=1e-22):
    """A positive table varying smoothly along its last (temperature) axis, random along the others."""
    nt = shape[-1]
    base = rng.uniform(0.2, 1.0, size=shape[:-1] + (1,))
    return scale * base * (1.0 + 0.3 * np.sin(0.7 * np.arange(nt) + rng.uniform(0, 3, size=shape[:-1] + (1,))))


def edge_states(T, P, Cc, nlay):
    """nlay layer states walking every edge of the three searches, cyclically: prs on P[0] (inactive), one ulp above, on an
    interior node, on the last node, above it and inside; tmp below T[0], on every node, above the last; conc below, on a
    node, above, inside."""
    pe = [P[0], np.nextafter(P[0], np.inf), P[len(P) // 2], P[-1], P[-1] * 1.5, 0.5 * (P[0] + P[1]), 0.5 * P[0],
          0.37 * P[-1] + 0.63 * P[-2]]
    te = [T[0] - 25.0] + list(T) + [T[-1] + 60.0, 0.5 * (T[0] + T[1]), 0.3 * T[-2] + 0.7 * T[-1]]
    ce = [Cc[0] * 0.1, Cc[0], Cc[len(Cc) // 2], Cc[-1], Cc[-1] * 3.0, 0.5 * (Cc[0] + Cc[1]), 0.9 * Cc[-1]]
    import math

    def walk(lst, first):
        # (a stride coprime with the list's length: every entry is visited, the combinations change from layer to layer)
        step = next(s for s in range(3, 3 + len(lst)) if math.gcd(s, len(lst)) == 1)
        return np.array([lst[(first + step * k) % len(lst)] for k in range(nlay)], dtype=np.float64)

    return walk(pe, 1), walk(te, 0), walk(ce, 1)


def make_cell(T, P, Cc, nterm, tables, prs, tmp, conc):
    """tables: {(gas, term): array [np][nt], gas 0 [nc][np][nt]}; every other slot is NULL."""
    return dict(T=np.asarray(T, dtype=np.float64), P=np.asarray(P, dtype=np.float64), C=np.asarray(Cc, dtype=np.float64),
                nterm=int(nterm), tables=tables, prs=np.asarray(prs, dtype=np.float64), tmp=np.asarray(tmp, dtype=np.float64),
                conc=np.asarray(conc, dtype=np.float64))


def reference(A, cell):
    """(xk [8][nterm][nlay], status) from absorption.coeff_abs_ckd, layer by layer: status 1 for the SPLINT error, 2 for
    ERROR_923 (the largest over the cell, as the kernel's atomic max); entries of a failing layer are left +0.0."""
    nlay = len(cell["prs"])
    xk = np.zeros((8, cell["nterm"], nlay))
    status = 0
    with np.errstate(all="ignore"):
        for (g, term), ki in cell["tables"].items():
            for j in range(nlay):
                try:
                    xk[g, term, j] = A.coeff_abs_ckd(g + 1, ki, cell["P"], cell["T"], cell["C"], cell["prs"][j], cell["tmp"][j],
                                                     cell["conc"][j])[0]
                except A.AbsorptionError as e:
                    status = max(status, 2 if "ERROR_923" in str(e) else 1)
    return xk, status


def run(pkg, cells, xk_off=None, out_doubles=None, stream=None):
    """sosgpu_ckd_layer_tables for the cells (one wavelength each) through the C ABI.  Returns (out, status): the whole output
    block as a host array -- pre-filled with NaN -- and the status words; xk_off defaults to one block after the other."""
    import torch
    capi = pkg.capi
    L = capi.lib()
    nlay = len(cells[0]["prs"])
    dev = torch.device("cuda", 0)
    wl = (capi.CkdWl * len(cells))()
    parts, n, ptrs, keep = [], 0, [], []
    off = 0
    for w, c in enumerate(cells):
        e = wl[w]
        for name, arr in (("pres_off", c["P"]), ("temp_off", c["T"]), ("conc_off", c["C"]), ("prs_off", c["prs"]),
                          ("tmp_off", c["tmp"]), ("cl_off", c["conc"])):
            setattr(e, name, n)
            parts.append(arr)
            n += arr.size
        e.nterm, e.nt, e.np, e.nc = c["nterm"], len(c["T"]), len(c["P"]), len(c["C"])
        e.xk_off = off if xk_off is None else int(xk_off[w])
        off = max(off, e.xk_off + 8 * c["nterm"] * nlay)
        for g in range(8):
            for term in range(c["nterm"]):
                ki = c["tables"].get((g, term))
                if ki is None:
                    ptrs.append(0)
                    continue
                assert ki.shape == ((len(c["C"]),) if g == 0 else ()) + (len(c["P"]), len(c["T"]))
                t = torch.from_numpy(np.ascontiguousarray(ki, dtype=np.float64)).to(dev)
                keep.append(t)
                ptrs.append(t.data_ptr())
    nout = off if out_doubles is None else int(out_doubles)
    ax = torch.from_numpy(np.concatenate(parts)).to(dev)
    out = torch.full((nout,), float("nan"), dtype=torch.float64, device=dev)
    nw = int(L.sosgpu_ckd_layer_tables_work_bytes(len(cells), len(ptrs)))
    work = torch.empty(nw, dtype=torch.uint8, device=dev)
    status = torch.full((len(cells),), 77, dtype=torch.int32, device=dev)          # (the call clears it)
    slots = (C.c_uint64 * len(ptrs))(*ptrs)
    bad = C.c_int(-5)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(dev) if stream is None else stream
    rc = L.sosgpu_ckd_layer_tables(0, len(cells), wl, len(ptrs), slots, C.c_void_p(ax.data_ptr()), n, nlay,
                                   C.c_void_p(work.data_ptr()), nw, C.c_void_p(out.data_ptr()), nout,
                                   C.c_void_p(status.data_ptr()), C.byref(bad), C.c_void_p(st.cuda_stream))
    assert rc == 0 and bad.value == -1, (rc, bad.value)
    st.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def same_doubles(a, b):
    """Equality of doubles as the tests mean it: equal values, no NaN, and the same sign on zeros."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b) and \
        np.array_equal(np.signbit(a), np.signbit(b))
