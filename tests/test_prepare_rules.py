"""The refusals of run_sos._prepare: the message and `ier` of every SosProcError it raises itself for a keyword set that
validate_parameters lets through, and which refusal wins when a call has two faults (the order of validate_parameters, then
of _prepare's stages).  The messages are the literals of the code as it stood before the stages were split, so a reworded or
reordered refusal fails here.  With -AER.AOTref 0 a refusal is reached before the device is touched (the head start of the
no-gas profile swallows its own failure): those run without a GPU."""
import pytest

import spectrum_cases
from test_surface_matrix import NEGATIVE_TRIPLE

D = -999.0
ABSENT = "/nonexistent/prepare_rules"

# Refusals of _prepare that validate_parameters raises first (with its own ERROR_nnnn text), so no keyword set reaches them:
#   -SOS_Main.Wa (2100), -ANG.Thetas (2200, 2201), -AP.AerProfile.Type (2505, 2506), -AP.AerLayer.Zmin / Zmax (2509),
#   -AP.AbsProfile.Type (2510, 2511), -SURF.Alb (2401), -AER.AOTref (2301), -SOS.View.Phi (2607), -SOS.View.Dphi (2608),
#   -AP.AerProfile.Type 2 with gas (2513), -AP.SpectralResol (2514), -AP.AbsProfile.UserFile (2512), -SURF.Ind (2405),
#   -SURF.Roujean.K0/K1/K2 (2407), -SURF.Maignan.C (2411), -SURF.Glitter.Wind (2406).
# The angle errors ("user angle out of [0,90]", "number of radiance angles > CTE_OS_NBMU_MAX") are run_sos.angles' own.

# name -> (base keyword set, the fault, aer_phase, environment variable to remove, message, ier)
HOST_FAULTS = {
    "surf_type_not_integral": ("cfg1_lambert", dict(isurf=0.5), None, None, "-SURF.Type must be in 0..7", 1),
    "aer_model": ("cfg1_lambert", dict(aot_ref=-0.3), None, None, "-AER.Model must be in 0..5", 1),
    "hr": ("cfg1_lambert", dict(hr=D), None, None, "-AP.HR must be defined", 1),
    "waref": ("cfg1_lambert", dict(aot_ref=-0.3, imod_aer=0, waref_aot=D), None, None, "-AER.Waref must be defined", 1),
    "aerosol_error": ("cfg1_lambert", dict(aot_ref=0.3, imod_aer=1, imodele_wmo=2), None, "SOS_ABS_ROOT",
                      "SOS_ABS_ROOT is not defined (SOS_AEROSOLS ERROR_925)", -1),
    "user_aerosols_absent": ("cfg2_lnd_lambert", dict(ficuser_aer=ABSENT), None, None, "-AER.UserFile %s not found" % ABSENT, 1),
    "aer_phase_length": ("cfg2_lnd_lambert", dict(), "short", None, "aer_phase arrays must have OS_NB+1 = %d entries", 1),
    "ha": ("cfg1_lambert", dict(aot_ref=-0.3, ha=D), "full", None, "-AP.AerHS.HA must be defined", 1),
    "mot_or_psurf": ("cfg1_lambert", dict(psurf=D), None, None, "-AP.MOT or -AP.Psurf must be defined", 1),
    "absorption_error": ("ckd_o2a_5bins", dict(), None, "SOS_ABS_ROOT", "SOS_ABS_ROOT is not defined (SOS_PREPA_ABSPROFILE ERROR_925)", -1),
    "abs_mode_ckd": ("cfg1_lambert", dict(imode_ckd_calcul=3), None, None, "-SOS.AbsModeCKD must be 1 or 2", 1),
    "nadal": ("land_breon", dict(isurf=6), None, None, "The Nadal's BPDF model is not supported ==> Select another surface model", 1),
    "surf_file_absent": ("glitter_polar", dict(ficsurf=ABSENT), None, None,
                         "-SURF.File %s does not exist (SOS_PREPA_OS ERROR_1020)" % ABSENT, -1),
}

# two faults: the refusal that comes first in today's order wins
TWO_FAULTS = {
    # (validate_parameters refuses all three of these pairs, in its own order: surface before atmosphere)
    "hr_and_nadal": ("land_breon", dict(hr=D, isurf=6), "The Nadal's BPDF model is not supported ==> Select another surface model", 1),
    "resol_and_wind": ("glitter_polar", dict(absprofil=2, nustep=-999, wind=D),
                       "SOS_PROC : ERROR_2406 on parameters -- -SURF.Glitter.Wind must be defined", 1),
    "layer_with_gas_and_mode3": ("layer_1_3km_lnd", dict(absprofil=2, nustep=10.0, imode_ckd_calcul=3),
                                 "SOS_PROC : ERROR_2513 on parameters -- -AP.AerProfile.Type 2 requires -AP.AbsProfile.Type 7 "
                                 "(no gas absorption)", 1),
    # (pairs that reach _prepare's own stages: checks < thickness < gas tables < surface)
    "hr_and_mode3": ("cfg1_lambert", dict(hr=D, imode_ckd_calcul=3), "-AP.HR must be defined", 1),
    "psurf_and_surf_file": ("glitter_polar", dict(psurf=D, ficsurf=ABSENT), "-AP.MOT or -AP.Psurf must be defined", 1),
    "mode3_and_surf_file": ("glitter_polar", dict(imode_ckd_calcul=3, ficsurf=ABSENT), "-SOS.AbsModeCKD must be 1 or 2", 1),
}

BASES = sorted({v[0] for v in HOST_FAULTS.values()} | {v[0] for v in TWO_FAULTS.values()})


@pytest.fixture(scope="module")
def bases(pkg, tmp_path_factory):
    kws, _, _, _ = spectrum_cases.build(pkg.run_sos, tmp_path_factory.mktemp("prepare_rules"), names=BASES)
    return dict(zip(BASES, kws))


def _refused(rs, kw, aer_phase=None):
    with pytest.raises(rs.SosProcError) as e:
        pl = rs._prepare(kw, aer_phase, 0, shard_bins=False)
        pl.ctx.close()
    return str(e.value), e.value.ier


@pytest.mark.parametrize("name", sorted(HOST_FAULTS))
def test_refusal_of_one_fault(pkg, bases, monkeypatch, name):
    rs = pkg.run_sos
    base, fault, phase, unset, message, ier = HOST_FAULTS[name]
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    if unset:
        monkeypatch.delenv(unset)
    kw = dict(bases[base], **fault)
    os_nb = rs._angle_counts(kw)[2]
    if phase is not None:
        entries = os_nb + 1 if phase == "full" else os_nb
        phase = dict(alpha=[0.0] * entries, beta=[1.0] * entries, gamma=[0.0] * entries, zeta=[0.0] * entries, piz=0.9, piztr=0.9)
    if "%d" in message:
        message = message % (os_nb + 1)
    assert _refused(rs, kw, phase) == (message, ier)


@pytest.mark.parametrize("name", sorted(TWO_FAULTS))
def test_the_earlier_refusal_wins(pkg, bases, monkeypatch, name):
    rs = pkg.run_sos
    base, faults, message, ier = TWO_FAULTS[name]
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    assert _refused(rs, dict(bases[base], **faults)) == (message, ier)


def test_predictors_decline_what_prepare_refuses(pkg, bases):
    """The predictors read _prepare's rules: a keyword set whose surface, gas or aerosol rule refuses gets no request."""
    rs = pkg.run_sos
    assert rs._surface_request(dict(bases["glitter_polar"], ficsurf=ABSENT), 0) is None
    assert rs._surface_request(dict(bases["land_breon"], isurf=6), 0) is None
    assert rs._surface_request(bases["glitter_polar"], 0) is not None
    assert rs._gas_table_request(dict(bases["ckd_o2a_5bins"], nustep=-999)) is None
    assert rs._gas_table_request(bases["ckd_o2a_5bins"])[7:] == (2, "NO_USER_ABS_PROFILE_FILE")
    assert rs._aerosol_call(dict(bases["cfg1_lambert"], aot_ref=0.3, wa_simu=0.67), None) is None          # -AER.Model undefined
    assert rs._aerosol_call(dict(bases["cfg1_lambert"], aot_ref=0.3, wa_simu=0.67, imod_aer=1), None)[1:] == \
        rs._angle_counts(bases["cfg1_lambert"])[1:3]


# --- refusals that need the device ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_negative_roujean_function_is_refused(gpu_pkg, bases):
    rs = gpu_pkg.run_sos
    t = NEGATIVE_TRIPLE
    rs._SURF_CACHE.clear()
    assert _refused(rs, dict(bases["land_breon"], isurf=3, k0_roujean=t[0], k1_roujean=t[1], k2_roujean=t[2])) == \
        ("SOS_FSF_ROUJEAN: BRDF < 0 for some geometry -- unsuitable Roujean coefficients (IER = -1)", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["cfg1_lambert", "ckd_o2a_5bins"])
def test_refused_profile_is_reported_as_sos_profile(gpu_pkg, bases, monkeypatch, base):
    """A scale height the profile entry point refuses (its argument check, before any launch): the no-gas profile and the
    CKD band both report it as "SOS_PROFILE: ..." with ier -1."""
    rs = gpu_pkg.run_sos
    monkeypatch.setenv("SOS_ABS_ROOT", spectrum_cases.GOLD)
    message, ier = _refused(rs, dict(bases[base], hr=-1.0))
    assert message.startswith("SOS_PROFILE: sosgpu_profile failed: ") and ier == -1
