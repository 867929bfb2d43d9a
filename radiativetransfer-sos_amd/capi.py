"""ctypes binding of libsosgpu.so (C ABI declared in include/sosgpu.h).

The product path has NO CPU fallback: if the HIP library is missing or cannot be loaded this module
raises at first use, loudly.  Build it with `python -m <pkg>.build` / __graft_entry__.build().
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SOSGPU_LIB selects an alternative build of the same library (A/B experiments); default = in-tree libsosgpu.so
SO_PATH = os.environ.get("SOSGPU_LIB") or os.path.join(HERE, "libsosgpu.so")

# every symbol include/sosgpu.h declares (checked by tests/test_cabi.py)
EXPORTS = [
    "sosgpu_strerror", "sosgpu_last_hip_error", "sosgpu_device_count", "sosgpu_version",
    "sosgpu_create", "sosgpu_destroy", "sosgpu_set_surface_matrices", "sosgpu_set_surface_matrices_async", "sosgpu_noyaux",
    "sosgpu_noyaux_fetch", "sosgpu_os_solve", "sosgpu_aggregate", "sosgpu_ctx_bytes",
    "sosgpu_os_flops", "sosgpu_last_solve_ms", "sosgpu_profile", "sosgpu_profile_nogas", "sosgpu_glitter", "sosgpu_mat_fresnel_host", "sosgpu_trphi",
    "sosgpu_debug_phase_buffer", "sosgpu_debug_scratch", "sosgpu_comm_unique_id", "sosgpu_comm_init_rank", "sosgpu_comm_destroy",
    "sosgpu_pack", "sosgpu_unpack", "sosgpu_reduce", "sosgpu_absprofile", "sosgpu_land_surface", "sosgpu_mie", "sosgpu_granu",
    "sosgpu_granu_batch", "sosgpu_mie_batch", "sosgpu_mie_batch_work_bytes",
    "sosgpu_ctx_table_entry_bytes", "sosgpu_ctx_table", "sosgpu_os_solve_multi", "sosgpu_trim",
    "sosgpu_os_solve_levels", "sosgpu_output_levels", "sosgpu_os_solve_multi_levels",
    "sosgpu_profile_spectrum", "sosgpu_profile_spectrum_work_bytes", "sosgpu_profile_nogas_levels", "sosgpu_debug_roundtrip",
    "sosgpu_debug_tables", "sosgpu_ckd_layer_tables", "sosgpu_ckd_layer_tables_work_bytes", "sosgpu_debug_solve_plan",
    "sosgpu_noyaux_spectrum", "sosgpu_noyaux_spectrum_work_bytes", "sosgpu_trphi_spectrum", "sosgpu_trphi_spectrum_work_bytes",
    "sosgpu_level_flux", "sosgpu_level_flux_spectrum", "sosgpu_level_flux_spectrum_work_bytes", "sosgpu_debug_stage_blocks",
    "sosgpu_profile_true", "sosgpu_profile_spectrum_true", "sosgpu_output_depths", "sosgpu_level_transmission",
    "sosgpu_channel_accumulate", "sosgpu_channel_accumulate_work_bytes", "sosgpu_channel_finish",
    "sosgpu_trans_spectrum", "sosgpu_trans_spectrum_work_bytes",
    "sosgpu_surface_batch", "sosgpu_surface_batch_work_bytes",
    "sosgpu_albedo_spectrum", "sosgpu_albedo_spectrum_work_bytes", "sosgpu_albedo_band",
    "sosgpu_level_absorption", "sosgpu_level_irradiance",
    "sosgpu_debug_order0_kpairs", "sosgpu_debug_ctx_order0_kpairs",
    "sosgpu_profile_layer_grid", "sosgpu_profile_layer", "sosgpu_profile_layer_spectrum", "sosgpu_profile_layer_spectrum_work_bytes",
    "sosgpu_create_spectrum", "sosgpu_create_spectrum_work_bytes",
]
NOGAS_LEVELS = 608     # SOSGPU_NOGAS_LEVELS
MAX_OUTPUT_LEVELS = 16  # SOSGPU_MAX_OUTPUT_LEVELS: output slots of one sosgpu_os_solve_levels call
SCAL_BASE = 10          # SOSGPU_SCAL_BASE: scalar block of sosgpu_aggregate = SCAL_BASE + N doubles
IRRADIANCE_COLS = 14   # SOSGPU_IRRADIANCE_COLS: columns of sosgpu_level_irradiance's block per slot and segment


class GranuJob(C.Structure):
    """sosgpu_granu_job (include/sosgpu.h)."""
    _fields_ = [("d_rec", C.c_void_p), ("nalpha", C.c_int32), ("igranu", C.c_int32), ("v1", C.c_double), ("v2", C.c_double),
                ("v3", C.c_double), ("wa", C.c_double), ("alphaf", C.c_double)]


class MieJob(C.Structure):
    """sosgpu_mie_job (include/sosgpu.h): one refractive index of sosgpu_mie_batch."""
    _fields_ = [("rn", C.c_double), ("in_", C.c_double), ("alphas", C.c_void_p), ("nalpha", C.c_int32), ("reserved", C.c_int32),
                ("d_rec", C.c_void_p), ("d_g", C.c_void_p)]


class ProfileWl(C.Structure):
    """sosgpu_profile_wl (include/sosgpu.h): one wavelength of sosgpu_profile_spectrum."""
    _fields_ = [("tr", C.c_double), ("hr", C.c_double), ("ta", C.c_double), ("ha", C.c_double),
                ("a_tronc", C.c_double), ("piz", C.c_double), ("piztr", C.c_double), ("zout", C.c_double),
                ("xk_off", C.c_int64), ("ro_off", C.c_int64), ("alt_off", C.c_int64),
                ("nterm", C.c_int32), ("nbins", C.c_int32), ("absprofil", C.c_int32), ("smax", C.c_int32)]


class LayerWl(C.Structure):
    """sosgpu_layer_wl (include/sosgpu.h): one wavelength of sosgpu_profile_layer_spectrum."""
    _fields_ = [("tr", C.c_double), ("hr", C.c_double), ("ta", C.c_double), ("zmin", C.c_double), ("zmax", C.c_double),
                ("a_tronc", C.c_double), ("piz", C.c_double), ("piztr", C.c_double), ("zout", C.c_double),
                ("smax", C.c_int32), ("reserved", C.c_int32)]


LAYER_WL_DTYPE = np.dtype(LayerWl)       # sosgpu_layer_wl as a numpy record
LAYER_ENTRY_BYTES = 96                   # sosgpu_profile_layer_spectrum_work_bytes(n) = n * this: the entry with its level grid


class CkdWl(C.Structure):
    """sosgpu_ckd_wl (include/sosgpu.h): one wavelength of sosgpu_ckd_layer_tables."""
    _fields_ = [("pres_off", C.c_int64), ("temp_off", C.c_int64), ("conc_off", C.c_int64),
                ("prs_off", C.c_int64), ("tmp_off", C.c_int64), ("cl_off", C.c_int64), ("xk_off", C.c_int64),
                ("nterm", C.c_int32), ("nt", C.c_int32), ("np", C.c_int32), ("nc", C.c_int32)]


class TablesInfo(C.Structure):
    """sosgpu_tables_info (include/sosgpu.h): layout numbers and scalars of a context's tables."""
    _fields_ = [(k, C.c_int32) for k in ("n", "w", "kp", "kh", "ks2h", "rtph", "nwgt", "prow", "os_nb", "smax", "n0", "ipolar")] + \
               [(k, C.c_double) for k in ("beta2", "gamma2", "alpha2", "f11sun", "f12sun", "mus", "ro")]


class SolvePlan(C.Structure):
    """sosgpu_solve_plan (include/sosgpu.h): launch form and scratch layout of a solve (sosgpu_debug_solve_plan)."""
    _fields_ = [(k, C.c_int32) for k in ("nw", "rtw", "ct", "big", "split", "kht", "form", "opl", "spec_k", "needs_nt",
                                         "per_launch", "lpb", "threads", "q_tail")] + \
               [(k, C.c_size_t) for k in ("lds_bytes", "per_bin", "regions", "off_i3", "i3_doubles", "off_queue", "queue_doubles",
                                          "off_slots", "slot_stride", "need")]


FORM_LDS, FORM_STREAM, FORM_PERSIST, FORM_SPEC = range(4)   # SOSGPU_FORM_*


class SosgpuError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib().sosgpu_strerror(code).decode()
        hip = lib().sosgpu_last_hip_error()
        super().__init__("%s failed: %s (code %d, hip error %d)" % (where, msg, code, hip))


class Wave(C.Structure):
    """struct sosgpu_wave"""
    _fields_ = [("n", C.c_int32), ("os_nb", C.c_int32), ("n0", C.c_int32), ("imat_surf", C.c_int32),
                ("ifresnel", C.c_int32), ("ipolar", C.c_int32), ("igmax", C.c_int32), ("reserved", C.c_int32),
                ("ro", C.c_double), ("ind_surf", C.c_double), ("ron", C.c_double)]


class CtxSpec(C.Structure):
    """sosgpu_ctx_spec (include/sosgpu.h): the arguments of one sosgpu_create, an entry of sosgpu_create_spectrum."""
    _fields_ = [("wv", Wave)] + [(k, C.c_void_p) for k in ("mu", "ga", "alpha", "beta", "gamma", "zeta")] + \
               [("iborm_max", C.c_int32), ("reserved", C.c_int32)]


class Land(C.Structure):
    """struct sosgpu_land"""
    _fields_ = [("isurf", C.c_int32), ("reserved", C.c_int32), ("k0", C.c_double), ("k1", C.c_double), ("k2", C.c_double),
                ("alpha", C.c_double), ("beta", C.c_double), ("coef_c", C.c_double)]


class TrphiJob(C.Structure):
    """sosgpu_trphi_job (include/sosgpu.h): one recomposition of sosgpu_trphi_spectrum."""
    _fields_ = [("cx", C.c_void_p), ("d_rec", C.c_void_p), ("nf", C.c_int32), ("igli", C.c_int32),
                ("phi_off", C.c_int32), ("nphi", C.c_int32), ("tau", C.c_double), ("tauout", C.c_double), ("wind", C.c_double),
                ("land", C.POINTER(Land))]


class SurfaceJob(C.Structure):
    """sosgpu_surface_job (include/sosgpu.h): one surface of sosgpu_surface_batch."""
    _fields_ = [("isurf", C.c_int32), ("reserved", C.c_int32), ("wind", C.c_double), ("ind", C.c_double), ("k0", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("coef_c", C.c_double), ("d_rsurf", C.c_void_p)]


class FluxJob(C.Structure):
    """sosgpu_flux_job (include/sosgpu.h): one (context, record) pair of sosgpu_level_flux_spectrum."""
    _fields_ = [("cx", C.c_void_p), ("d_rec", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "libsosgpu.so not found at %s: the HIP extension is required (no CPU fallback). "
                "Run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950)." % SO_PATH)
        # One HIP runtime per process: PyTorch ships its own libamdhip64 and this library links against the system's.  Loaded
        # first, the system runtime would be initialised here and torch's copy afterwards -- two runtimes, and the later one
        # sees no device.  Importing torch first makes both resolve to the runtime torch loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(SO_PATH)
        vp, i32, dbl = C.c_void_p, C.c_int, C.c_double
        L.sosgpu_strerror.restype = C.c_char_p
        L.sosgpu_strerror.argtypes = [i32]
        L.sosgpu_version.restype = C.c_char_p
        L.sosgpu_last_hip_error.restype = i32
        L.sosgpu_device_count.restype = i32
        L.sosgpu_create.restype = i32
        L.sosgpu_create.argtypes = [C.POINTER(vp), i32, C.POINTER(Wave), vp, vp, vp, vp, vp, vp, i32]
        L.sosgpu_create_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_create_spectrum_work_bytes.argtypes = [C.POINTER(CtxSpec), i32]
        L.sosgpu_create_spectrum.restype = i32
        L.sosgpu_create_spectrum.argtypes = [C.POINTER(vp), i32, C.POINTER(CtxSpec), i32, vp, C.c_size_t, vp]
        L.sosgpu_destroy.restype = i32
        L.sosgpu_destroy.argtypes = [vp]
        L.sosgpu_set_surface_matrices.restype = i32
        L.sosgpu_set_surface_matrices.argtypes = [vp, vp]
        L.sosgpu_set_surface_matrices_async.restype = i32
        L.sosgpu_set_surface_matrices_async.argtypes = [vp, vp, vp]
        L.sosgpu_noyaux.restype = i32
        L.sosgpu_noyaux.argtypes = [vp, vp]
        L.sosgpu_noyaux_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_noyaux_spectrum_work_bytes.argtypes = [i32]
        L.sosgpu_noyaux_spectrum.restype = i32
        L.sosgpu_noyaux_spectrum.argtypes = [C.POINTER(vp), i32, C.POINTER(vp), vp, C.c_size_t, vp]
        L.sosgpu_noyaux_fetch.restype = i32
        L.sosgpu_noyaux_fetch.argtypes = [vp, i32, vp]
        L.sosgpu_os_solve.restype = i32
        L.sosgpu_os_solve.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sosgpu_os_solve_levels.restype = i32
        L.sosgpu_os_solve_levels.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.sosgpu_output_levels.restype = i32
        L.sosgpu_output_levels.argtypes = [vp, i32, i32, vp, vp, vp, i32, C.POINTER(dbl), vp, vp, vp, vp]
        L.sosgpu_output_depths.restype = i32
        L.sosgpu_output_depths.argtypes = [i32, i32, i32, vp, C.c_size_t, vp, vp, i32, C.POINTER(dbl), vp, vp]
        L.sosgpu_level_transmission.restype = i32
        L.sosgpu_level_transmission.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp, vp, C.c_size_t, i32, vp]
        L.sosgpu_trim.restype = i32
        L.sosgpu_trim.argtypes = []
        L.sosgpu_ctx_table_entry_bytes.restype = C.c_size_t
        L.sosgpu_ctx_table_entry_bytes.argtypes = []
        L.sosgpu_ctx_table.restype = i32
        L.sosgpu_ctx_table.argtypes = [C.POINTER(vp), i32, vp, vp]
        L.sosgpu_os_solve_multi.restype = i32
        L.sosgpu_os_solve_multi.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sosgpu_os_solve_multi_levels.restype = i32
        L.sosgpu_os_solve_multi_levels.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.sosgpu_aggregate.restype = i32
        L.sosgpu_aggregate.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sosgpu_comm_unique_id.restype = i32
        L.sosgpu_comm_unique_id.argtypes = [vp]
        L.sosgpu_comm_init_rank.restype = i32
        L.sosgpu_comm_init_rank.argtypes = [C.POINTER(vp), i32, vp, i32]
        L.sosgpu_comm_destroy.restype = i32
        L.sosgpu_comm_destroy.argtypes = [vp]
        L.sosgpu_pack.restype = i32
        L.sosgpu_pack.argtypes = [vp, i32, vp, vp, vp, vp]
        L.sosgpu_unpack.restype = i32
        L.sosgpu_unpack.argtypes = [vp, i32, vp, vp, vp, vp]
        L.sosgpu_absprofile.restype = i32
        L.sosgpu_absprofile.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.sosgpu_mie.restype = i32
        L.sosgpu_mie.argtypes = [i32, i32, vp, dbl, dbl, i32, vp, vp, vp, vp]
        L.sosgpu_granu.restype = i32
        L.sosgpu_granu.argtypes = [i32, i32, i32, vp, i32, dbl, dbl, dbl, dbl, dbl, vp, vp]
        L.sosgpu_granu_batch.restype = i32
        L.sosgpu_granu_batch.argtypes = [i32, i32, i32, C.POINTER(GranuJob), vp, vp, C.c_size_t, vp]
        L.sosgpu_mie_batch_work_bytes.restype = C.c_size_t
        L.sosgpu_mie_batch_work_bytes.argtypes = [i32, i32, C.POINTER(MieJob)]
        L.sosgpu_mie_batch.restype = i32
        L.sosgpu_mie_batch.argtypes = [i32, i32, vp, i32, C.POINTER(MieJob), vp, C.c_size_t, vp, vp]
        L.sosgpu_reduce.restype = i32
        L.sosgpu_reduce.argtypes = [vp, vp, i32, vp, vp]
        L.sosgpu_ctx_bytes.restype = C.c_size_t
        L.sosgpu_ctx_bytes.argtypes = [vp]
        L.sosgpu_profile.restype = i32
        L.sosgpu_profile.argtypes = [vp, i32, dbl, dbl, dbl, dbl, i32, i32, vp, vp, dbl, dbl, dbl, dbl, i32,
                                     vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sosgpu_profile_true.restype = i32
        L.sosgpu_profile_true.argtypes = L.sosgpu_profile.argtypes[:-1] + [vp, vp]
        L.sosgpu_profile_nogas.restype = i32
        L.sosgpu_profile_nogas.argtypes = [i32, dbl, dbl, dbl, dbl, vp, vp]
        L.sosgpu_profile_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_profile_spectrum_work_bytes.argtypes = [i32]
        L.sosgpu_profile_nogas_levels.restype = i32
        L.sosgpu_profile_nogas_levels.argtypes = [dbl, dbl]
        L.sosgpu_profile_spectrum.restype = i32
        L.sosgpu_profile_spectrum.argtypes = [i32, i32, vp, i32, vp, vp, vp, C.c_size_t, i32, i32, vp, C.c_size_t, vp, vp, vp, vp,
                                              vp, vp, vp, vp, C.POINTER(i32), vp]
        L.sosgpu_profile_spectrum_true.restype = i32
        L.sosgpu_profile_spectrum_true.argtypes = L.sosgpu_profile_spectrum.argtypes[:-1] + [vp, vp]
        L.sosgpu_profile_layer_grid.restype = i32
        L.sosgpu_profile_layer_grid.argtypes = [dbl, dbl, dbl, dbl, dbl, C.POINTER(i32)]
        L.sosgpu_profile_layer.restype = i32
        L.sosgpu_profile_layer.argtypes = [vp] + [dbl] * 9 + [i32] + [vp] * 9
        L.sosgpu_profile_layer_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_profile_layer_spectrum_work_bytes.argtypes = [i32]
        L.sosgpu_profile_layer_spectrum.restype = i32
        L.sosgpu_profile_layer_spectrum.argtypes = [i32, i32, vp, i32, vp, C.c_size_t] + [vp] * 8 + [C.POINTER(i32), vp]
        L.sosgpu_ckd_layer_tables_work_bytes.restype = C.c_size_t
        L.sosgpu_ckd_layer_tables_work_bytes.argtypes = [i32, i32]
        L.sosgpu_ckd_layer_tables.restype = i32
        L.sosgpu_ckd_layer_tables.argtypes = [i32, i32, vp, i32, vp, vp, C.c_size_t, i32, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(i32),
                                              vp]
        L.sosgpu_os_flops.restype = i32
        L.sosgpu_os_flops.argtypes = [vp, i32, vp, vp, vp, C.POINTER(dbl)]
        L.sosgpu_last_solve_ms.restype = i32
        L.sosgpu_last_solve_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.sosgpu_glitter.restype = i32
        L.sosgpu_glitter.argtypes = [i32, i32, vp, vp, dbl, dbl, i32, i32, i32, vp, vp, vp, vp]
        L.sosgpu_mat_fresnel_host.restype = i32
        L.sosgpu_mat_fresnel_host.argtypes = [i32, vp, vp, dbl, i32, vp]
        L.sosgpu_trphi.restype = i32
        L.sosgpu_trphi.argtypes = [vp, i32, vp, dbl, dbl, i32, vp, i32, dbl, C.POINTER(Land), vp, vp]
        L.sosgpu_trphi_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_trphi_spectrum_work_bytes.argtypes = [i32]
        L.sosgpu_trphi_spectrum.restype = i32
        L.sosgpu_trphi_spectrum.argtypes = [C.POINTER(TrphiJob), i32, vp, i32, vp, vp, C.c_size_t, vp]
        L.sosgpu_level_flux.restype = i32
        L.sosgpu_level_flux.argtypes = [vp, vp, vp, vp]
        L.sosgpu_level_flux_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_level_flux_spectrum_work_bytes.argtypes = [i32]
        L.sosgpu_level_flux_spectrum.restype = i32
        L.sosgpu_level_flux_spectrum.argtypes = [C.POINTER(FluxJob), i32, vp, vp, C.c_size_t, vp]
        L.sosgpu_channel_accumulate_work_bytes.restype = C.c_size_t
        L.sosgpu_channel_accumulate_work_bytes.argtypes = [i32, i32]
        L.sosgpu_channel_accumulate.restype = i32
        L.sosgpu_channel_accumulate.argtypes = [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_size_t, vp]
        L.sosgpu_channel_finish.restype = i32
        L.sosgpu_channel_finish.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, vp]
        L.sosgpu_land_surface.restype = i32
        L.sosgpu_land_surface.argtypes = [i32, C.POINTER(Land), i32, vp, vp, dbl, i32, i32, i32, vp, C.POINTER(C.c_int32), vp]
        L.sosgpu_surface_batch_work_bytes.restype = C.c_size_t
        L.sosgpu_surface_batch_work_bytes.argtypes = [i32, i32, i32, i32, C.POINTER(SurfaceJob), i32]
        L.sosgpu_surface_batch.restype = i32
        L.sosgpu_surface_batch.argtypes = [i32, i32, vp, vp, i32, i32, i32, C.POINTER(SurfaceJob), i32, vp, vp, C.c_size_t, vp]
        L.sosgpu_debug_phase_buffer.restype = i32
        L.sosgpu_debug_phase_buffer.argtypes = [vp, vp]
        L.sosgpu_debug_scratch.restype = i32
        L.sosgpu_debug_scratch.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.sosgpu_trans_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_trans_spectrum_work_bytes.argtypes = [C.POINTER(vp), i32, i32, i32]
        L.sosgpu_trans_spectrum.restype = i32
        L.sosgpu_trans_spectrum.argtypes = [C.POINTER(vp), i32, vp, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]
        L.sosgpu_albedo_spectrum_work_bytes.restype = C.c_size_t
        L.sosgpu_albedo_spectrum_work_bytes.argtypes = [C.POINTER(vp), i32, i32, i32]
        L.sosgpu_albedo_spectrum.restype = i32
        L.sosgpu_albedo_spectrum.argtypes = [C.POINTER(vp), i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, C.c_size_t, vp]
        L.sosgpu_albedo_band.restype = i32
        L.sosgpu_albedo_band.argtypes = [i32, vp, vp, vp, vp, i32, vp]
        L.sosgpu_level_absorption.restype = i32
        L.sosgpu_level_absorption.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        L.sosgpu_level_irradiance.restype = i32
        L.sosgpu_level_irradiance.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp,
                                              vp, vp]
        L.sosgpu_debug_stage_blocks.restype = i32
        L.sosgpu_debug_stage_blocks.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
        L.sosgpu_debug_solve_plan.restype = i32
        L.sosgpu_debug_solve_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(SolvePlan)]
        L.sosgpu_debug_order0_kpairs.restype = i32
        L.sosgpu_debug_order0_kpairs.argtypes = [i32, i32]
        L.sosgpu_debug_ctx_order0_kpairs.restype = i32
        L.sosgpu_debug_ctx_order0_kpairs.argtypes = [vp, i32]
        L.sosgpu_debug_roundtrip.restype = i32
        L.sosgpu_debug_roundtrip.argtypes = [i32, i32, C.c_size_t, vp, vp, vp]
        L.sosgpu_debug_tables.restype = i32
        L.sosgpu_debug_tables.argtypes = [vp, C.POINTER(TablesInfo), vp, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def check(code, where):
    if code != 0:
        raise SosgpuError(code, where)
