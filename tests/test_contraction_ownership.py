"""Which wave owns which tile of the source contraction: the four-wave, two-column-tile kernels of seven or eight row tiles
(k_sos_os<4,2,2,.,.,false>, N = 33 ... 42 at up to 32 levels -- the flagship's shape) against the C oracle at the cells where a
mapping of row and column tiles to waves can go wrong.  Comparison and tolerance are those of
test_gpu_parity.test_sos_os_vs_oracle: 1e-9 relative on every record, identical Fourier-order and scattering-order counts.
(Written with the column-tile ownership of DESIGN.md section 4, which was measured and not kept; the cells hold for any
ownership, and every one of them runs the order-0 contraction over the I and Q columns only.)

  Gauss counts 32, 36, 37, 41 (N = 33, 37, 38, 42): seven row tiles with a partial last tile (4 / 3 tiles on the two row halves),
      seven full tiles (no pad rows: the molecular projection is not folded), eight tiles with a partial last tile, eight full
      tiles without pad rows
  NT = 15, 16, 31: the second column tile all padding, holding one level, both column tiles full
  aerosol + molecular, molecular only (projection alone), aerosol only
  Lambert and flat-sea Fresnel ground, one cell with surface matrices, one with an output altitude
  OS_NB = 8: orders s <= 2 (molecular operator, folded or not) and s > 2 (XDEL fused into the write-back) both run
and the headline shape, N = 41 at 30 layers and OS_NB = 80, on 4 bins."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
S = cases.S

N_OF_GAUSS = {32: 33, 36: 37, 37: 38, 41: 42, 40: 41}


def _case(ng, nt, atm, os_nb=8, kabs=(0.0, 1.0), g=0.7, **kw):
    mu, w, n0 = S.gauss_angles(ng, 35.0)
    assert len(mu) == N_OF_GAUSS[ng]
    al, be, ga, ze = S.hg_phase(os_nb, g)
    bins, iborm = [], os_nb
    for k in kabs:
        h, x, y, z = S.profile(nt, k_abs=k)
        if atm == "mol":
            x = np.zeros_like(x)
        elif atm == "aer":
            y = np.zeros_like(y)
        h, x, y, iborm = S.rescale_profile(h, x, y, 0.0, 0.95, 0.95, os_nb)
        bins.append((h, x, y, z))
    if kw.get("imat_surf"):
        kw["rsurf"] = cases._surf_matrices(len(mu), iborm, 7)
    return dict(name="ownership_g%d_nt%d_%s" % (ng, nt, atm), rmu=mu, ga=w, n0=n0, os_nb=os_nb, coefs=(al, be, ga, ze),
                bins=bins, iborm=iborm, kw=kw)


def _check(gpu_pkg, oracle, case, min_orders):
    got = cases.run_gpu(gpu_pkg, case)
    for b, g in enumerate(got):
        ref = cases.run_cpu(oracle, case, b)
        assert len(g["records"]) == len(ref["records"]), (case["name"], b, len(g["records"]), len(ref["records"]))
        assert len(ref["records"]) >= min_orders, (case["name"], b, len(ref["records"]))
        assert np.array_equal(g["ig_counts"], ref["ig_counts"]), (case["name"], b, g["ig_counts"], ref["ig_counts"])
        worst = cases.compare_records(g["records"], ref["records"], 1e-9, "%s bin %d" % (case["name"], b))
        assert abs(g["emoins"] - ref["emoins"]) <= 1e-9 * abs(ref["emoins"]) + 1e-300
        assert abs(g["eplus"] - ref["eplus"]) <= 1e-9 * abs(ref["eplus"]) + 1e-300
        print(case["name"], b, "F", len(ref["records"]), "worst rel", worst)


@pytest.mark.parametrize("atm", ["both", "mol", "aer"])
@pytest.mark.parametrize("nt", [15, 16, 31])
@pytest.mark.parametrize("ng", [32, 36, 37, 41])
def test_lambert_vs_oracle(gpu_pkg, oracle, ng, nt, atm):
    # (a molecular atmosphere has the orders 0 .. 2 only; with aerosols the orders beyond 2 must run too)
    _check(gpu_pkg, oracle, _case(ng, nt, atm, ro=0.1), 3 if atm == "mol" else 4)


@pytest.mark.parametrize("atm", ["both", "mol", "aer"])
@pytest.mark.parametrize("ng", [32, 36, 37, 41])
def test_fresnel_vs_oracle(gpu_pkg, oracle, ng, atm):
    _check(gpu_pkg, oracle, _case(ng, 16, atm, ro=0.05, ifresnel=1, ind_surf=1.34), 3 if atm == "mol" else 4)


def test_surface_matrices_vs_oracle(gpu_pkg, oracle):
    _check(gpu_pkg, oracle, _case(37, 31, "both", ro=0.02, imat_surf=1), 4)


def test_output_altitude_vs_oracle(gpu_pkg, oracle):
    _check(gpu_pkg, oracle, _case(32, 31, "both", ro=0.1, zout=3.0), 4)


def test_headline_shape_vs_oracle(gpu_pkg, oracle):
    _check(gpu_pkg, oracle, _case(40, 30, "both", os_nb=80, kabs=(0.0, 0.3, 2.0, 8.0), g=0.75, ro=0.1), 4)
