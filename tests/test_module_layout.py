"""The layout under run_sos: params and geometry, the bottom layer, import only from the modules below them (so no cycle is
possible, and aerosols no longer reaches up into run_sos); run_sos offers its 69 public names, those of the bottom layer as the
objects of their home module, and of that layer's private names only the three its own code reads; importing it loads neither
torch nor the library binding.  (run_sos still holds the formats, the surface cache, the preparation, the band drivers and the
spectrum pass with their private names: "no private name in run_sos" can be asserted once they have moved too.)"""
import ast
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = "radiativetransfer-sos_amd"

# module -> the modules of the package it may import (top level or inside a function)
LAYERS = {"params": set(), "geometry": {"params", "synth"}, "aerosols": {"capi", "geometry", "absorption", "solver"}}

PUBLIC = {
    "params": ["SOS_NOT_DEFINED_VALUE_INT", "SOS_NOT_DEFINED_VALUE_DBLE", "SOS_DEFAULT_AER_JUNGE_RMAX", "SOS_DEFAULT_FICANGRESLUM",
               "SOS_DEFAULT_FICANGRESMIE", "SOS_DEFAULT_FICGRANU", "SOS_DEFAULT_RESBIN", "SOS_DEFAULT_RESUP", "SOS_DEFAULT_RESDOWN",
               "CTE_OS_NBMU_MAX", "CTE_LENFIC2", "CTE_OS_NT", "CTE_OS_NT_MIN", "CTE_TCOUCHE", "CTE_TOA_FIRST_LAYER", "CTE_DELTA_Z",
               "CTE_TOA_ALT", "CTE_HT_STD_PSURF", "CTE_DEFAULT_IGMAX", "CTE_DEFAULT_NBMU_LUM", "CTE_DEFAULT_NBMU_MIE",
               "CTE_DEFAULT_OS_NB", "CTE_DEFAULT_OS_NS", "CTE_DEFAULT_OS_NM", "PARAMS", "EXTRA_KEYS", "SOS_PROC_KWARGS",
               "OUTPUT_NAMES", "LEVEL_FLUX_NAMES", "LEVEL_FLUX_SPLIT_NAMES", "LEVEL_ABSORPTION_NAMES", "SosProcError",
               "default_parameters", "update_parameters", "set_sos_params", "sos_proc_kwargs", "validate_parameters"],
    "geometry": ["sos_gauss", "angles", "rayleigh_optical_thickness", "profile_nogas", "profile_layer"],
    "run_sos": ["fortran_e", "fortran_d", "read_aerosols_file", "write_aerosols_file", "write_used_angles", "write_mie_angles",
                "read_surface_file", "write_surface_file", "trans_quantities", "trans_entry", "write_trans_file", "write_flux_file",
                "write_result_bin", "main_output_header", "write_main_output", "gen_hdr_sos_output", "gen_sos_output",
                "PREPARE_SEGMENTS", "trphi_tables", "sos_proc", "sos_proc_levels", "sos_proc_many", "spectrum_costs",
                "sos_spectrum", "sos_spectrum_levels", "sos_spectrum_channels", "sos_spectrum_irradiances"],
}
PRIVATE_READ_BY_RUN_SOS = {"_D", "_I", "_angle_counts"}


def _package_imports(module):
    """The modules of the package that `module` imports, anywhere in its source."""
    with open(os.path.join(ROOT, PACKAGE, module + ".py")) as f:
        tree = ast.parse(f.read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            found |= {node.module.split(".")[0]} if node.module else {a.name for a in node.names}
        assert not (isinstance(node, ast.ImportFrom) and node.level > 1), "%s: import from above the package" % module
    return found


@pytest.mark.parametrize("module", sorted(LAYERS))
def test_imports_stay_within_the_layers_below(module):
    assert _package_imports(module) <= LAYERS[module], sorted(_package_imports(module) - LAYERS[module])


def test_run_sos_offers_the_public_names_of_their_home(pkg):
    assert sum(len(v) for v in PUBLIC.values()) == 69
    for home, names in PUBLIC.items():
        for name in names:
            assert getattr(pkg.run_sos, name) is getattr(getattr(pkg, home), name), name


def test_run_sos_takes_only_the_private_names_it_reads(pkg):
    for home in (pkg.params, pkg.geometry):
        private = {n for n in vars(home) if n.startswith("_") and not n.startswith("__")}
        assert private & set(vars(pkg.run_sos)) <= PRIVATE_READ_BY_RUN_SOS, home.__name__
    assert PRIVATE_READ_BY_RUN_SOS <= set(vars(pkg.run_sos))


def test_run_sos_imports_without_torch_or_the_library():
    code = ("import importlib, sys; sys.path.insert(0, %r); importlib.import_module(%r); "
            "print([m for m in ('torch', %r, %r) if m in sys.modules])"
            % (ROOT, PACKAGE + ".run_sos", PACKAGE + ".solver", PACKAGE + ".capi"))
    env = {k: v for k, v in os.environ.items() if k != "SOS_PREPARE_SEGMENTS"}      # (that diagnostic hooks into the solver)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "[]", out
