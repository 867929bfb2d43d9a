"""Land surfaces, -SURF.Type 3 (Roujean BRDF), 4 (+ Rondeaux-Herman BPDF), 5 (+ Breon BPDF), 7 (+ Maignan BPDF): SURVEY 8 row f4.
Type 6 (Nadal) is refused by the reference's own SOS_PROC, and here with the same message.

Goldens (make_golden.py proc_land) from the compiled reference: the surface file it generated (every Fourier order, REAL*4),
SOS_Result.bin and the 23 outputs; `cfg5_roujean_maignan` is BASELINE config 5's surface with an LND aerosol, so that all 41
orders of the matrices act inside the solve and the direct terms of SOS_TRPHI (Roujean + Maignan) are exercised in polar view."""
import json
import os

import numpy as np
import pytest

import cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAND_CASES = ["land_roujean", "land_rondeaux", "land_breon", "cfg5_roujean_maignan"]


def test_nadal_is_refused_like_the_reference(pkg):
    rs = pkg.run_sos
    kw = rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), {
        "-SOS_Main.Wa": 0.67, "-ANG.Thetas": 30.0, "-AP.AbsProfile.Type": 7, "-AER.AOTref": 0.0, "-SURF.Alb": 0.0, "-AP.HR": 8.0,
        "-AP.Psurf": 1013.0, "-SOS.View": 1, "-SOS.View.Phi": 0.0, "-SURF.Type": 6, "-SURF.Ind": 1.5, "-SURF.Roujean.K0": 0.2,
        "-SURF.Roujean.K1": 0.03, "-SURF.Roujean.K2": 0.25, "-SURF.Nadal.Alpha": 0.01, "-SURF.Nadal.Beta": 80.0}))
    with pytest.raises(rs.SosProcError, match="Nadal"):
        rs.sos_proc(**kw)


def _case_angles(rs, user):
    nb_lum, nb_mie = int(user["-ANG.Rad.NbGauss"]), int(user["-ANG.Aer.NbGauss"])
    mu, ga, n0, _ = rs.angles(nb_lum, user["-ANG.Thetas"])
    return mu, ga, n0, 2 * nb_mie, 2 * nb_lum


@pytest.mark.parametrize("name", LAND_CASES)
def test_land_oracle_vs_reference_file(pkg, oracle, name):
    """oracle.land (oracle/sos_land_oracle.c) against the surface file the reference wrote.  The reference sources are not
    in this repository, so this pin is what makes the restatement an oracle.  Measured on all four files: 0 differing
    elements, max error 0 (bit-identical, as oracle.glitter is on glitter_n13.npz); the bar stays that of the GPU test below."""
    g = np.load(os.path.join(GOLD, "sos_proc_%s.npz" % name))
    user = json.loads(str(g["user_json"]))
    mu, ga, n0, os_nb, os_ns = _case_angles(pkg.run_sos, user)
    o = oracle.land(user["-SURF.Type"], mu, ga, user["-SURF.Roujean.K0"], user["-SURF.Roujean.K1"], user["-SURF.Roujean.K2"],
                    user.get("-SURF.Maignan.C", 0.0), user.get("-SURF.Ind", 1.0), os_nb, os_ns, os_nb + os_ns)
    got, ref = o["rsurf"], g["rsurf"]
    assert o["ier"] == 0 and got.shape == ref.shape
    scale = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    print("%s: share of differing elements %.3e, max error / scale %.3e" % (name, np.mean(got != ref), err / scale))
    assert err <= 4e-7 * scale, err / scale
    assert np.mean(got != ref) < 2e-2
    assert np.array_equal(got == 0, ref == 0)


@pytest.mark.parametrize("name", LAND_CASES)
def test_land_direct_terms_oracle_vs_reference_radiances(pkg, oracle, name):
    """oracle.trphi_land fed with the reference's own SOS_Result.bin against the radiances the reference recomposed from it,
    at the azimuth rows of the case's view mode: the Roujean branch in all four cases, Rondeaux-Herman, Breon and Maignan in
    one each.  tau comes from host code alone: rayleigh_optical_thickness + profile_nogas, and for cfg5_roujean_maignan the
    delta-truncation rescale with the stored aerosol coefficients.  Bar: the 1e-9 record bar.  Measured worst relative error
    (floor 1e-3 of the I scale): 3.3e-16, 2.1e-16, 3.1e-16, 4.0e-16."""
    rs = pkg.run_sos
    g = np.load(os.path.join(GOLD, "sos_proc_%s.npz" % name))
    user = json.loads(str(g["user_json"]))
    mu, ga, n0, os_nb, os_ns = _case_angles(rs, user)
    n, w = len(mu), 2 * len(mu) + 1
    rb = g["result_bin"]                                   # one record per order: Q(-N:N), U(-N:N), I(-N:N)
    rec = np.stack([rb[:, 2 * w:], rb[:, :w], rb[:, w:2 * w]], axis=1)
    tr = rs.rayleigh_optical_thickness(user["-SOS_Main.Wa"], user["-AP.Psurf"])
    ta = user["-AER.AOTref"]
    h, xdel, ydel, _ = rs.profile_nogas(tr, user["-AP.HR"], ta, user["-AP.AerHS.HA"] if ta else 1.0)
    if ta:
        h, xdel, ydel, _ = rs.rescale_profile(h, xdel, ydel, float(g["aer_a_tronc"]), float(g["aer_piz"]), float(g["aer_piztr"]), os_nb)
    tau = -np.log(np.exp(-h[-1]))                          # SOS_AGGREGATE keeps the optical depths as -ln(sum aik exp(-tau))
    phis, rows, _ = rs._trphi_azimuths(user["-SOS.View"], user.get("-SOS.View.Phi"), user["-SOS.View.Dphi"])
    scale = np.abs(g["i_up"]).max()
    worst = 0.0
    for k, phi in zip(rows, phis):
        o = oracle.trphi_land(mu, rec, tau, 0.0, phi, n0=n0, ind_surf=user.get("-SURF.Ind", 1.0), isurf=user["-SURF.Type"],
                              k0=user["-SURF.Roujean.K0"], k1=user["-SURF.Roujean.K1"], k2=user["-SURF.Roujean.K2"],
                              coef_c=user.get("-SURF.Maignan.C", 0.0))["out"]
        for q, nm in enumerate(["i", "q", "u"]):
            for got, exp in ((o[q][n + 1:], g[nm + "_up"][k, :n]), (o[q][:n][::-1], g[nm + "_down"][k, :n])):
                assert np.isfinite(got).all()
                err = np.abs(got - exp)
                worst = max(worst, (err / np.maximum(np.abs(exp), 1e-3 * scale)).max())
                assert np.all(err <= 1e-9 * np.abs(exp) + 1e-12 * scale), (k, nm, err.max())
        for got, exp in ((o[3][n + 1:], g["sca_ang_up"][k, :n]), (o[3][:n][::-1], g["sca_ang_down"][k, :n])):
            assert np.allclose(np.cos(np.radians(got)), np.cos(np.radians(exp)), rtol=0, atol=1e-13)
    print("%s: tau %.12g, worst relative error %.2e" % (name, tau, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAND_CASES)
def test_land_matrices_vs_reference_file(gpu_pkg, name):
    """sosgpu_land_surface against the surface file the reference wrote: REAL*4 elements equal up to last-bit flips (device
    cos / exp differ from the host libm by an ulp before the REAL*4 rounding), same zero pattern, same truncation orders."""
    import torch
    rs, surf = gpu_pkg.run_sos, gpu_pkg.surface
    g = np.load(os.path.join(GOLD, "sos_proc_%s.npz" % name))
    user = json.loads(str(g["user_json"]))
    nb_lum, nb_mie = int(user["-ANG.Rad.NbGauss"]), int(user["-ANG.Aer.NbGauss"])
    os_nb, os_ns = 2 * nb_mie, 2 * nb_lum
    mu, ga, n0, _ = rs.angles(nb_lum, user["-ANG.Thetas"])
    land = surf.land_model(user["-SURF.Type"], user["-SURF.Roujean.K0"], user["-SURF.Roujean.K1"], user["-SURF.Roujean.K2"],
                           coef_c=user.get("-SURF.Maignan.C", 0.0))
    got = surf.land_matrices(land, mu, ga, user.get("-SURF.Ind", 1.0), os_nb, os_ns, os_nb + os_ns)
    torch.cuda.synchronize()
    got, ref = got.cpu().numpy(), g["rsurf"]
    assert got.shape == ref.shape
    scale = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert err.max() <= 4e-7 * scale, err.max() / scale
    assert np.mean(got != ref) < 2e-2                       # bit-identical but for last-bit flips (wave-order sums, device cos)
    assert np.array_equal(got == 0, ref == 0) or np.mean((got == 0) != (ref == 0)) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAND_CASES)
def test_sos_proc_land_vs_reference(gpu_pkg, name, tmp_path):
    rs = gpu_pkg.run_sos
    g = np.load(os.path.join(GOLD, "sos_proc_%s.npz" % name))
    user = json.loads(str(g["user_json"]))
    user.update({"-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT"})
    coef = None
    if user["-AER.AOTref"] != 0.0:
        f = str(tmp_path / "Aerosols_user.txt")
        rs.write_aerosols_file(f, {k: g["aer_" + k] for k in ("alpha", "beta", "gamma", "zeta", "a_tronc", "piztr", "piz")}, *g["kmat"])
        user["-AER.UserFile"] = f
        coef = 0.0
    out = rs.sos_proc(**rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False))
    # REAL*4 surface matrices with rare last-bit differences enter linearly: 1e-7 relative on the reflected part
    cases.compare_proc_outputs(rs, out, g, coef_tronca=coef, rtol=2e-7)


def test_surface_file_round_trip(pkg, tmp_path):
    rs = pkg.run_sos
    g = np.load(os.path.join(GOLD, "sos_proc_land_rondeaux.npz"))
    f = str(tmp_path / "SURF_USER")
    rs.write_surface_file(f, g["rsurf"])
    n = g["rsurf"].shape[-1]
    back = rs.read_surface_file(f, n, g["rsurf"].shape[0] - 1)
    assert back.dtype == np.float32 and np.array_equal(back, g["rsurf"])
    assert os.path.getsize(f) == g["rsurf"].shape[0] * (9 * n * n * 4 + 8)          # one unformatted record per Fourier order
    with pytest.raises(rs.SosProcError):
        rs.read_surface_file(f, n + 1, 3)                                            # made for another angle set
    with pytest.raises(rs.SosProcError):
        rs.read_surface_file(f, n, g["rsurf"].shape[0])                              # one order short


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAND_CASES)
def test_sos_proc_with_the_references_surface_file(gpu_pkg, name, tmp_path):
    """-SURF.File: the reflection matrices come from a user file (here the very file the reference wrote for the case), the
    surface computation is skipped (SOS_PROC.F:3186-3189).  With bit-identical matrices the radiances match at 1e-9."""
    rs = gpu_pkg.run_sos
    g = np.load(os.path.join(GOLD, "sos_proc_%s.npz" % name))
    user = json.loads(str(g["user_json"]))
    f = str(tmp_path / "SURF_USER")
    rs.write_surface_file(f, g["rsurf"])
    user.update({"-SOS_Main.Log": "NO_LOG_FILE", "-SOS.Flux": "NO_OUTPUT", "-SURF.File": f})
    coef = None
    if user["-AER.AOTref"] != 0.0:
        fa = str(tmp_path / "Aerosols_user.txt")
        rs.write_aerosols_file(fa, {k: g["aer_" + k] for k in ("alpha", "beta", "gamma", "zeta", "a_tronc", "piztr", "piz")}, *g["kmat"])
        user["-AER.UserFile"] = fa
        coef = 0.0
    out = rs.sos_proc(**rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False))
    cases.compare_proc_outputs(rs, out, g, coef_tronca=coef)
    user["-SURF.File"] = str(tmp_path / "missing")
    with pytest.raises(rs.SosProcError):
        rs.sos_proc(**rs.sos_proc_kwargs(rs.update_parameters(rs.default_parameters(), user), trace=False))
