"""Fourier order 0 contracts the I and Q columns only (csrc/solve_variant.h sos_order0_kpairs, SosDev::ks2h0).

U is exactly zero at s = 0: the kernels GT, ART and the function T^0_l that couple it to I and Q are exact zeros, so the K
positions of the U columns, 2 Nw ... 3 Nw - 1, feed the contraction products with an exact zero factor.  CPU part: the zeros in
the oracle's kernels, and the rule for the k-pair count -- ceil(2 Nw / 8) without surface matrices, all ceil(3 Nw / 8) with them.
GPU part: the same contexts solved with the trimmed count and with the full count (sosgpu_debug_ctx_order0_kpairs) give the same
records, fluxes and order counts bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cases

S = cases.S


def _angles(name):
    """Gauss counts 3, 24, 33 (2 Nw = 66, no multiple of 8) and 40, and 24 Gauss angles with two zero-weight user angles."""
    if name == "user2":
        mu, w, n0 = S.gauss_angles(24, 35.0)
        extra = np.cos(np.radians([10.0, 72.0]))
        mu_all, w_all = np.concatenate([mu, extra]), np.concatenate([w, np.zeros(2)])
        order = np.argsort(-mu_all, kind="stable")
        mus = mu[n0 - 1]
        mu, w = mu_all[order], w_all[order]
        return mu, w, int(np.where(mu == mus)[0][0]) + 1
    return S.gauss_angles(int(name), 35.0)


CONTEXTS = ["3", "24", "33", "40", "user2"]


def _ceil8(x):
    return (x + 7) // 8


@pytest.mark.parametrize("name", CONTEXTS)
def test_oracle_order0_u_kernels_are_exact_zeros(oracle, name):
    mu, w, n0 = _angles(name)
    os_nb = 24
    al, be, ga, ze = S.hg_phase(os_nb, 0.75)
    k = oracle.noyaux(0, -mu[n0 - 1], mu, os_nb, al, be, ga, ze)
    for key in ("GT", "ART", "XTL"):
        assert not np.any(k[key]), (name, key, np.abs(k[key]).max())
    assert np.any(k["ATT"]) and np.any(k["GR"])          # (the kernels that do not involve T are there)


def test_order0_kpair_rule(pkg):
    L = pkg.capi.lib()
    for nwgt in range(1, 86):
        full, iq = _ceil8(3 * nwgt), _ceil8(2 * nwgt)
        assert L.sosgpu_debug_order0_kpairs(nwgt, 0) == iq, nwgt
        assert L.sosgpu_debug_order0_kpairs(nwgt, 1) == full, nwgt
        assert iq <= full
    for name in CONTEXTS:
        mu, w, n0 = _angles(name)
        nwgt = int(np.count_nonzero(w))
        assert nwgt == (24 if name == "user2" else int(name))
        assert L.sosgpu_debug_order0_kpairs(nwgt, 0) == _ceil8(2 * nwgt)
    assert L.sosgpu_debug_order0_kpairs(0, 0) == -1 and L.sosgpu_debug_order0_kpairs(86, 0) == -1     # SOSGPU_E_ARG


def _bins(nt, os_nb):
    rows = []
    for k, atm in ((0.0, "both"), (1.0, "both"), (0.3, "mol"), (0.3, "aer")):
        h, x, y, z = S.profile(nt, k_abs=k)
        if atm == "mol":
            x = np.zeros_like(x)
        elif atm == "aer":
            y = np.zeros_like(y)
        h, x, y, _ = S.rescale_profile(h, x, y, 0.0, 0.95, 0.95, os_nb)
        rows.append((h, x, y))
    return [np.array([r[i] for r in rows]) for i in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("surface", ["lambert", "fresnel", "matrices"])
@pytest.mark.parametrize("name", CONTEXTS)
def test_trimmed_and_full_contraction_agree_bit_for_bit(gpu_pkg, name, surface):
    import torch
    mu, w, n0 = _angles(name)
    os_nb, nt = 24, 22
    al, be, ga, ze = S.hg_phase(os_nb, 0.75)
    kw = dict(ro=0.1)
    if surface == "fresnel":
        kw = dict(ro=0.05, ifresnel=1, ind_surf=1.34)
    elif surface == "matrices":
        kw = dict(ro=0.02, imat_surf=1, rsurf=cases._surf_matrices(len(mu), os_nb, 7))
    cx = gpu_pkg.SosContext(mu, w, n0, al, be, ga, ze, iborm_max=os_nb, **kw)
    L = gpu_pkg.capi.lib()
    nwgt = int(np.count_nonzero(w))
    full, iq = _ceil8(3 * nwgt), _ceil8(2 * nwgt)
    assert L.sosgpu_debug_ctx_order0_kpairs(cx._h, -1) == (full if surface == "matrices" else iq)
    h, x, y = _bins(nt, os_nb)
    bins = cx.upload_bins(h, x, y)
    a = {k: v.clone() for k, v in cx.solve(bins).items() if k in ("rec", "flux", "iglast", "norders")}
    assert L.sosgpu_debug_ctx_order0_kpairs(cx._h, 1) == full
    b = cx.solve(bins)
    torch.cuda.synchronize()
    assert L.sosgpu_debug_ctx_order0_kpairs(cx._h, 0) == (full if surface == "matrices" else iq)
    assert int(a["norders"].min()) >= 1                   # every bin ran (order 0 at least)
    for k in ("rec", "flux", "iglast", "norders"):
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), (name, surface, k)
    cx.close()
