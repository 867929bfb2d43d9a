"""The parameter table of the reference's front end (`-Group.Key` dictionary, sos_proc keywords, defaults), the constants of
inc/SOS.h the host side restates, SosProcError and the user-parameter checks of SOS_PROC.  Imports nothing of the package."""
import numpy as np

SOS_NOT_DEFINED_VALUE_INT = -999
SOS_NOT_DEFINED_VALUE_DBLE = -999.0
SOS_DEFAULT_AER_JUNGE_RMAX = 50.
SOS_DEFAULT_FICANGRESLUM = "SOS_UsedAngles.txt"
SOS_DEFAULT_FICANGRESMIE = "Aer_UsedAngles.txt"
SOS_DEFAULT_FICGRANU = "Aerosols.txt"
SOS_DEFAULT_RESBIN = "SOS_Result.bin"
SOS_DEFAULT_RESUP = "SOS_Up.txt"
SOS_DEFAULT_RESDOWN = "SOS_Down.txt"

# inc/SOS.h constants used by the host-side restatements (REAL*4 literals are widened exactly as Fortran does)
_F = lambda x: float(np.float32(x))
CTE_OS_NBMU_MAX = 80
CTE_LENFIC2 = 500                    # SOS.h:59
CTE_OS_NT = 600                      # SOS.h:202
CTE_OS_NT_MIN = 100                  # SOS.h:229
CTE_TCOUCHE = _F(0.005)              # SOS.h:208
CTE_TOA_FIRST_LAYER = _F(0.0002)     # SOS.h:213
CTE_DELTA_Z = _F(0.05)               # SOS.h:218
CTE_TOA_ALT = 120.0                  # SOS.h:197
CTE_HT_STD_PSURF = 1013.0            # SOS.h:192
CTE_DEFAULT_IGMAX = 100              # SOS.h:383
CTE_DEFAULT_NBMU_LUM, CTE_DEFAULT_NBMU_MIE = 24, 40          # SOS.h:514,508
CTE_DEFAULT_OS_NB, CTE_DEFAULT_OS_NS, CTE_DEFAULT_OS_NM = 80, 48, 128   # SOS.h:521-535

# (dictionary key, sos_proc keyword, default) in the positional order of SOS_PROC (SOS_PROC.F:415-470)
_I, _D = SOS_NOT_DEFINED_VALUE_INT, SOS_NOT_DEFINED_VALUE_DBLE
PARAMS = [
    ("-SOS_Main.ResRoot", "resroot", ""), ("-SOS_Main.Log", "ficmain_log", "SOS_Main.Log"),
    ("-SOS_Main.Wa", "wa_simu", _D), ("-ANG.Rad.NbGauss", "nbmu_gauss_lum", _I),
    ("-ANG.Rad.UserAngFile", "ficangles_user_lum", "NO_USER_ANGLES"), ("-ANG.Thetas", "tetas", _D),
    ("-ANG.Rad.ResFile", "ficangles_res_lum", SOS_DEFAULT_FICANGRESLUM), ("-ANG.Aer.NbGauss", "nbmu_gauss_mie", _I),
    ("-ANG.Aer.UserAngFile", "ficangles_user_mie", "NO_USER_ANGLES"),
    ("-ANG.Aer.ResFile", "ficangles_res_mie", SOS_DEFAULT_FICANGRESMIE), ("-ANG.Log", "ficanglog", "Angles.Log"),
    ("-AER.Waref", "waref_aot", _D), ("-AER.AOTref", "aot_ref", _D), ("-AER.Tronca", "itronc_aer", 1),
    ("-AER.Log", "ficgranu_log", "NO_LOG_FILE"), ("-AER.MieLog", "ficmie_log", "NO_LOG_FILE"),
    ("-AER.DirMie", "dir_mie", ""), ("-AER.ResFile", "ficgranu", SOS_DEFAULT_FICGRANU), ("-AER.Model", "imod_aer", _I),
    ("-AER.MMD.MRwa", "rn_wa", _D), ("-AER.MMD.MIwa", "in_wa", _D), ("-AER.MMD.MRwaref", "rn_waref", _D),
    ("-AER.MMD.MIwaref", "in_waref", _D), ("-AER.MMD.SDtype", "igranu", _I),
    ("-AER.MMD.LNDradius", "lnd_radius_mmd_aer", _D), ("-AER.MMD.LNDvar", "lnd_lnvar_mmd_aer", _D),
    ("-AER.MMD.JD.slope", "jd_slope_mmd_aer", _D), ("-AER.MMD.JD.rmin", "jd_rmin_mmd_aer", _D),
    ("-AER.MMD.JD.rmax", "jd_rmax_mmd_aer", SOS_DEFAULT_AER_JUNGE_RMAX), ("-AER.WMO.Model", "imodele_wmo", _I),
    ("-AER.WMO.DL", "c_wmo_dl", _D), ("-AER.WMO.WS", "c_wmo_ws", _D), ("-AER.WMO.OC", "c_wmo_oc", _D),
    ("-AER.WMO.SO", "c_wmo_so", _D), ("-AER.SF.Model", "imodele_sf", _I), ("-AER.SF.RH", "rh", _D),
    ("-AER.BMD.VCdef", "mode_param_bilnd", _I), ("-AER.BMD.CoarseVC", "user_cv_coarse", _D),
    ("-AER.BMD.FineVC", "user_cv_fine", _D), ("-AER.BMD.RAOT", "rtauct_waref", _D),
    ("-AER.BMD.CM.MRwa", "bmd_cm_mrwa", _D), ("-AER.BMD.CM.MIwa", "bmd_cm_miwa", _D),
    ("-AER.BMD.CM.MRwaref", "bmd_cm_mrwaref", _D), ("-AER.BMD.CM.MIwaref", "bmd_cm_miwaref", _D),
    ("-AER.BMD.CM.SDradius", "bmd_cm_rmodal", _D), ("-AER.BMD.CM.SDvar", "bmd_cm_var", _D),
    ("-AER.BMD.FM.MRwa", "bmd_fm_mrwa", _D), ("-AER.BMD.FM.MIwa", "bmd_fm_miwa", _D),
    ("-AER.BMD.FM.MRwaref", "bmd_fm_mrwaref", _D), ("-AER.BMD.FM.MIwaref", "bmd_fm_miwaref", _D),
    ("-AER.BMD.FM.SDradius", "bmd_fm_rmodal", _D), ("-AER.BMD.FM.SDvar", "bmd_fm_var", _D),
    ("-AER.ExtData", "ficextdata_aer", "NO_USER_AEROSOLS_PHAZE_FCT"),
    ("-AER.DefMixture", "ficmixture_aer", "NO_USER_AEROSOLS_MIXTURE"), ("-AER.UserFile", "ficuser_aer", "NO_USER_AEROSOLS"),
    ("-AP.Log", "ficprofil_log", "Aerosols.Log"), ("-AP.MOT", "tr", _D), ("-AP.HR", "hr", _D), ("-AP.AerHS.HA", "ha", _D),
    ("-AP.AerProfile.Type", "iprofil", 1), ("-AP.AerLayer.Zmin", "zmin", _D), ("-AP.AerLayer.Zmax", "zmax", _D),
    ("-AP.Psurf", "psurf", _D), ("-AP.H2O", "h2o", _D), ("-AP.O3", "o3", _D), ("-AP.CO2", "co2", _D), ("-AP.CH4", "ch4", _D),
    ("-AP.AbsProfile.Type", "absprofil", _I), ("-AP.AbsProfile.UserFile", "ficabsprofil", "NO_USER_ABS_PROFILE_FILE"),
    ("-AP.SpectralResol", "nustep", _I), ("-SURF.Type", "isurf", 0), ("-SURF.Dir", "dir_surf", ""),
    ("-SURF.Log", "ficsurf_log", "NO_LOG_FILE"), ("-SURF.Ind", "surf_ind", _D), ("-SURF.Glitter.Wind", "wind", _D),
    ("-SURF.Roujean.K0", "k0_roujean", _D), ("-SURF.Roujean.K1", "k1_roujean", _D), ("-SURF.Roujean.K2", "k2_roujean", _D),
    ("-SURF.Nadal.Alpha", "alpha_nadal", _D), ("-SURF.Nadal.Beta", "beta_nadal", _D),
    ("-SURF.Maignan.C", "coef_c_maignan", _D), ("-SURF.Alb", "rho", _D), ("-SURF.File", "ficsurf", "DEFAULT"),
    ("-SOS.Log", "ficsos_log", "SOS.Log"), ("-SOS.ResBin", "ficsos_res_bin", SOS_DEFAULT_RESBIN),
    ("-SOS.Trans", "fictrans", "NO_OUTPUT"), ("-SOS.Flux", "ficflux", "FicFlux.txt"), ("-SOS.OutputAlt", "zout", -1.0),
    ("-SOS.IGmax", "igmax", 200), ("-SOS.Ipolar", "ipolar", 1), ("-SOS.View", "itrphi", 2),
    ("-SOS.View.Phi", "phios", _D), ("-SOS.View.Dphi", "pas_phi", _I), ("-SOS.AbsModeCKD", "imode_ckd_calcul", 1),
]
# keys the reference dictionary holds but never forwards to sos_proc (run_sos.py:548-549,557)
EXTRA_KEYS = {"-SOS.ResFileUp": SOS_DEFAULT_RESUP, "-SOS.ResFileDown": SOS_DEFAULT_RESDOWN, "-SOS.MDF": 0.0279}
SOS_PROC_KWARGS = [p[1] for p in PARAMS] + ["ier", "trace"]
OUTPUT_NAMES = ["nblum", "ind_angout", "phi", "vza", "sca_ang_up", "i_up", "q_up", "u_up", "pol_ang_up", "pol_rate_up",
                "l_pol_up", "sca_ang_down", "i_down", "q_down", "u_down", "pol_ang_down", "pol_rate_down", "l_pol_down",
                "flux_dir_down", "flux_diff_down", "flux_tot_down", "flux_diff_up", "coef_tronca"]


# columns of the per-altitude flux rows of sos_proc_levels / sos_spectrum_levels with fluxes=True (_level_flux_row)
LEVEL_FLUX_NAMES = ["flux_dir_down_tronc", "flux_diff_down_tronc", "flux_tot_down", "flux_diff_up", "flux_net"]
# ... with split=True: the down-going flux split into the true direct beam and the true diffuse light at the altitude
LEVEL_FLUX_SPLIT_NAMES = LEVEL_FLUX_NAMES + ["flux_dir_down", "flux_diff_down"]
# columns of the per-altitude rows of absorption=True (_level_absorption_row): the actinic flux and the absorbed power per km
LEVEL_ABSORPTION_NAMES = ["actinic_dir", "actinic_diff_down", "actinic_diff_up", "actinic_tot", "absorbed_per_km"]


class SosProcError(RuntimeError):
    """Raised where the reference prints a message and returns IER=1 (SOS_PROC.F:3895-4896)."""

    def __init__(self, msg, ier=1):
        super().__init__(msg)
        self.ier = ier


def default_parameters():
    """The reference's `dict_sos_all_parameters` (run_sos.py:459-559)."""
    d = {k: v for k, _, v in PARAMS}
    d.update(EXTRA_KEYS)
    return d


def update_parameters(defaults, user):
    """run_sos.py:606-609: user values override defaults; keys the default dictionary does not hold are dropped."""
    out = dict(defaults)
    for k, v in user.items():
        if k in defaults:
            out[k] = v
    return out


def set_sos_params(dict_sos, trace=True):
    """run_sos.py:319-441: the positional tuple handed to sos_proc (96 values: 94 parameters, ier, trace)."""
    return tuple(dict_sos[k] for k, _, _ in PARAMS) + (0, trace)


def sos_proc_kwargs(dict_sos, trace=True):
    return dict(zip(SOS_PROC_KWARGS, set_sos_params(dict_sos, trace)))


def validate_parameters(p):
    """The user-parameter checks of SOS_PROC in the reference's order (SOS_PROC.F:1310-1335, 1540-2475): the first violated
    rule raises SosProcError carrying the reference's error number (`.code`, the label of its message block at
    SOS_PROC.F:4074-4745) and the keyword to fix.  Side effects of that block are mirrored too: with a single wavelength
    the reference-wavelength refractive indices default to the simulation ones (:1704-1707, :1812-1818)."""
    def fail(code, text):
        e = SosProcError("SOS_PROC : ERROR_%s on parameters -- %s" % (code, text))
        e.code = code
        raise e
    und = lambda k: p[k] == _D                       # CTE_NOT_DEFINED_VALUE_DBLE = -999. and _INT = -999 compare equal
    user_aer = str(p["ficuser_aer"]).strip() != "NO_USER_AEROSOLS"
    # (ERROR_1000, -SOS_Main.ResRoot undefined, is not mirrored: without a results directory this implementation simply
    #  writes no files -- a deliberate difference, see the module docstring)
    if und("aot_ref"):
        fail(2301, "-AER.AOTref (aerosol optical thickness at the reference wavelength) must be defined")
    if p["aot_ref"] > 0.0:
        if und("imod_aer") and not user_aer:
            fail(2304, "-AER.Model must be defined (0 mono-modal, 1 WMO, 2 Shettle & Fenn, 3 bimodal log-normal, "
                       "4 external phase functions, 5 user mixture)")
        if und("waref_aot"):
            fail(2302, "-AER.Waref (reference wavelength of the aerosol optical thickness) must be defined")
    if und("wa_simu"):
        fail(2100, "-SOS_Main.Wa (simulation wavelength, microns) must be defined")
    if p["wa_simu"] < _F(0.364) or p["wa_simu"] > _F(4.0):                          # CTE_WAMIN, CTE_WAMAX (SOS.h:70-71)
        fail(2101, "-SOS_Main.Wa = %r outside [0.364, 4.0] microns" % p["wa_simu"])
    if und("tetas"):
        fail(2200, "-ANG.Thetas (solar zenith angle, degrees) must be defined")
    if p["tetas"] < 0.0 or p["tetas"] >= 90.0:
        fail(2201, "-ANG.Thetas out of [0, 90[")
    if p["aot_ref"] > 0.0 and not user_aer:
        imod = int(p["imod_aer"])
        one_wl = p["wa_simu"] == p["waref_aot"]
        if imod < 0 or imod > 5:
            fail(2305, "-AER.Model out of 0..5")
        if int(p["itronc_aer"]) not in (0, 1):
            fail(23141, "-AER.Tronca must be 0 or 1")
        if imod == 0:
            if und("rn_wa") or und("in_wa"):
                fail(2309, "-AER.MMD.MRwa and -AER.MMD.MIwa must be defined")
            if p["in_wa"] > 0.0:
                fail(2310, "-AER.MMD.MIwa must be negative or null")
            if und("igranu"):
                fail(2311, "-AER.MMD.SDtype must be defined (1 log-normal, 2 Junge)")
            if int(p["igranu"]) not in (1, 2):
                fail(2312, "-AER.MMD.SDtype must be 1 or 2")
            if int(p["igranu"]) == 1 and (und("lnd_radius_mmd_aer") or und("lnd_lnvar_mmd_aer")):
                fail(23131, "-AER.MMD.LNDradius and -AER.MMD.LNDvar must be defined")
            if int(p["igranu"]) == 2 and (und("jd_slope_mmd_aer") or und("jd_rmin_mmd_aer")):
                fail(23132, "-AER.MMD.JD.slope and -AER.MMD.JD.rmin must be defined")
            if not one_wl:
                if und("rn_waref") or und("in_waref"):
                    fail(2314, "-AER.MMD.MRwaref and -AER.MMD.MIwaref must be defined when -SOS_Main.Wa differs from -AER.Waref")
            else:
                p["rn_waref"], p["in_waref"] = p["rn_wa"], p["in_wa"]
        if imod == 1:
            if und("imodele_wmo"):
                fail(2315, "-AER.WMO.Model must be defined")
            if not 1 <= int(p["imodele_wmo"]) <= 4:
                fail(2316, "-AER.WMO.Model must be in 1..4")
            if int(p["imodele_wmo"]) == 4 and any(und(k) for k in ("c_wmo_dl", "c_wmo_ws", "c_wmo_oc", "c_wmo_so")):
                fail(2317, "-AER.WMO.DL, .WS, .OC and .SO must be defined for the user WMO model")
        if imod == 2:
            if und("imodele_sf"):
                fail(2318, "-AER.SF.Model must be defined")
            if und("rh"):
                fail(2319, "-AER.SF.RH must be defined")
            if not 1 <= int(p["imodele_sf"]) <= 4:
                fail(2320, "-AER.SF.Model must be in 1..4")
            if p["rh"] < 0.0 or p["rh"] > 99.0:
                fail(2321, "-AER.SF.RH must be in [0, 99] %")
        if imod == 3:
            if und("mode_param_bilnd"):
                fail(2322, "-AER.BMD.VCdef must be defined")
            if int(p["mode_param_bilnd"]) not in (1, 2):
                fail(2323, "-AER.BMD.VCdef must be 1 or 2")
            if int(p["mode_param_bilnd"]) == 1:
                if und("user_cv_coarse"):
                    fail(2324, "-AER.BMD.CoarseVC must be defined")
                if und("user_cv_fine"):
                    fail(2325, "-AER.BMD.FineVC must be defined")
            if int(p["mode_param_bilnd"]) == 2 and und("rtauct_waref"):
                fail(2326, "-AER.BMD.RAOT must be defined")
            if any(und("bmd_cm_" + k) for k in ("mrwa", "miwa", "rmodal", "var")):
                fail(2327, "the coarse-mode parameters -AER.BMD.CM.{MRwa, MIwa, SDradius, SDvar} must be defined")
            if any(und("bmd_fm_" + k) for k in ("mrwa", "miwa", "rmodal", "var")):
                fail(2328, "the fine-mode parameters -AER.BMD.FM.{MRwa, MIwa, SDradius, SDvar} must be defined")
            if not one_wl:
                if any(und(k) for k in ("bmd_cm_mrwaref", "bmd_cm_miwaref", "bmd_fm_mrwaref", "bmd_fm_miwaref")):
                    fail(2329, "-AER.BMD.{CM,FM}.{MRwaref, MIwaref} must be defined when -SOS_Main.Wa differs from -AER.Waref")
            else:
                for m in ("cm", "fm"):
                    p["bmd_%s_mrwaref" % m], p["bmd_%s_miwaref" % m] = p["bmd_%s_mrwa" % m], p["bmd_%s_miwa" % m]
        if imod == 4:
            if str(p["ficextdata_aer"]).strip() == "NO_USER_AEROSOLS_PHAZE_FCT":
                fail(2330, "-AER.ExtData (file of external phase functions) must be defined")
            if not one_wl:
                fail(2331, "-AER.Model 4 requires -SOS_Main.Wa equal to -AER.Waref")
        if imod == 5 and str(p["ficmixture_aer"]).strip() == "NO_USER_AEROSOLS_MIXTURE":
            fail(2340, "-AER.DefMixture (file of the user mixture) must be defined")
    if p["aot_ref"] > 0.0 and user_aer:
        if p["wa_simu"] != p["waref_aot"]:
            fail(2350, "-AER.UserFile requires -SOS_Main.Wa equal to -AER.Waref")
        if str(p["ficgranu"]).strip() != SOS_DEFAULT_FICGRANU:
            fail(2351, "-AER.ResFile must keep its default value when -AER.UserFile is given")
    if und("rho"):
        fail(2401, "-SURF.Alb must be defined")
    if p["rho"] < 0.0:
        fail(2402, "-SURF.Alb must be positive or null")
    if und("isurf"):
        fail(2403, "-SURF.Type must be defined")
    isurf = int(p["isurf"])
    if isurf not in range(8):
        fail(2404, "-SURF.Type must be in 0..7")
    if und("surf_ind") and isurf in (1, 2, 4, 5, 6, 7):
        fail(2405, "-SURF.Ind (refractive index of the surface) must be defined for this surface type")
    if isurf == 1:
        if und("wind"):
            fail(2406, "-SURF.Glitter.Wind must be defined")
        if p["wind"] < 0.0:
            fail(24061, "-SURF.Glitter.Wind must be positive or null")
    if isurf >= 3 and any(und(k) for k in ("k0_roujean", "k1_roujean", "k2_roujean")):
        fail(2407, "-SURF.Roujean.K0, .K1 and .K2 must be defined")
    if isurf == 6:                                        # SOS_PROC.F:2203-2208: the reference leaves here, before the later checks
        e = SosProcError("The Nadal's BPDF model is not supported ==> Select another surface model")
        e.code = -6
        raise e
    if isurf == 7 and und("coef_c_maignan"):
        fail(2411, "-SURF.Maignan.C must be defined")
    if not und("tr") and p["tr"] < 0.0:
        fail(2502, "-AP.MOT must be positive or null")
    if not und("tr") and p["tr"] > 0.0:                   # (with -AP.MOT left to the Rayleigh formula the reference skips these two)
        if und("hr"):
            fail(2503, "-AP.HR (molecular scale height) must be defined")
        if p["hr"] <= 0.0:
            fail(2504, "-AP.HR must be strictly positive")
    if und("iprofil"):
        fail(2505, "-AP.AerProfile.Type must be defined")
    if int(p["iprofil"]) not in (1, 2):
        fail(2506, "-AP.AerProfile.Type must be 1 or 2")
    if int(p["iprofil"]) == 1:
        if und("ha") and p["aot_ref"] > 0.0:
            fail(2507, "-AP.AerHS.HA (aerosol scale height) must be defined")
        if p["ha"] <= 0.0 and p["aot_ref"] >= 0.0:           # as written there: an undefined HA (-999) fails even without aerosols
            fail(2508, "-AP.AerHS.HA must be strictly positive")
    if int(p["iprofil"]) == 2 and (und("zmin") or und("zmax")):
        fail(2509, "-AP.AerLayer.Zmin and -AP.AerLayer.Zmax must be defined for -AP.AerProfile.Type 2")
    if und("absprofil"):
        fail(2510, "-AP.AbsProfile.Type must be defined")
    absprofil = int(p["absprofil"])
    if not 0 <= absprofil <= 7:
        fail(2511, "-AP.AbsProfile.Type must be in 0..7")
    if absprofil == 0 and str(p["ficabsprofil"]).strip() == "NO_USER_ABS_PROFILE_FILE":
        fail(2512, "-AP.AbsProfile.UserFile must be defined for -AP.AbsProfile.Type 0")
    if int(p["iprofil"]) == 2 and absprofil != 7:
        fail(2513, "-AP.AerProfile.Type 2 requires -AP.AbsProfile.Type 7 (no gas absorption)")
    if absprofil != 7:
        if und("nustep"):
            fail(2514, "-AP.SpectralResol must be defined (1, 5 or 10 cm-1)")
        if int(p["nustep"]) not in (1, 5, 10):
            fail(25141, "-AP.SpectralResol must be 1, 5 or 10 cm-1")
        if und("imode_ckd_calcul"):
            fail(2515, "-SOS.AbsModeCKD must be defined")
    if p["igmax"] != _I and int(p["igmax"]) < 1:
        fail(2604, "-SOS.IGmax must be at least 1")
    if und("itrphi"):
        fail(2605, "-SOS.View must be defined")
    if int(p["itrphi"]) not in (1, 2):
        fail(2606, "-SOS.View must be 1 or 2")
    if int(p["itrphi"]) == 1 and und("phios"):
        fail(2607, "-SOS.View.Phi must be defined for -SOS.View 1")
    if int(p["itrphi"]) == 2:
        if und("pas_phi"):
            fail(2608, "-SOS.View.Dphi must be defined for -SOS.View 2")
        if int(p["pas_phi"]) <= 0:
            fail(2609, "-SOS.View.Dphi must be strictly positive")
    if int(p["ipolar"]) not in (0, 1):
        fail(2610, "-SOS.Ipolar must be 0 or 1")
    if (p["zout"] < 0.0 and p["zout"] != -1.0) or p["zout"] > CTE_TOA_ALT:
        fail(2611, "-SOS.OutputAlt must be -1 (standard levels) or within [0, %g] km" % CTE_TOA_ALT)


def _angle_counts(p):
    """(nb_lum, nb_mie, os_nb, os_ns, os_nm) of SOS_ANGLES for the keyword set p (SOS_ANGLES.F:303-329)."""
    nb_lum = CTE_DEFAULT_NBMU_LUM if p["nbmu_gauss_lum"] == _I else int(p["nbmu_gauss_lum"])
    nb_mie = CTE_DEFAULT_NBMU_MIE if p["nbmu_gauss_mie"] == _I else int(p["nbmu_gauss_mie"])
    os_nb = CTE_DEFAULT_OS_NB if p["nbmu_gauss_mie"] == _I else 2 * nb_mie          # SOS_ANGLES.F:303-312
    if p["nbmu_gauss_lum"] == _I:
        os_ns, os_nm = CTE_DEFAULT_OS_NS, CTE_DEFAULT_OS_NM
    else:
        os_ns = 2 * nb_lum
        os_nm = os_nb + os_ns                                                        # SOS_ANGLES.F:325-329
    return nb_lum, nb_mie, os_nb, os_ns, os_nm
