"""Blocks of vectors on one cone workspace (include/scs_amd.h, B1': scs_amd_cone_proj_dual_multi and the device entries): what can
be checked without a GPU -- exports, the width rule, the argument checks that come before any device call and before the workspace
is looked at, and the Python module's own checks.  (`ldx < m` needs a workspace to know m: tests/test_cones_multi_gpu.py.)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

from scs_amd import capi

NAMES = ("scs_amd_cone_multi_width", "scs_amd_cone_proj_dual_multi", "scs_amd_cone_proj_dual_dev", "scs_amd_cone_proj_dual_multi_dev",
         "scs_amd_cone_sync")
LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so")
# what the two partial libraries exported before block projections existed (scs_amd/csrc/exports_cones.map, exports_linsys.map)
CONES_EXPORTS = {"_scs_init_cone", "_scs_proj_dual_cone", "_scs_finish_cone", "_scs_set_r_y", "_scs_enforce_cone_boundaries",
                 "_scs_validate_cones", "_scs_get_cone_header", "_scs_deep_copy_cone", "_scs_free_cone", "scs_amd_cone_init",
                 "scs_amd_cone_proj_dual", "scs_amd_cone_finish", "scs_amd_device_count", "scs_amd_set_device", "scs_amd_test_fail_at",
                 "scs_amd_device_free_bytes", "scs_amd_set_option", "scs_amd_get_option", "scs_amd_list_options"}


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", LIBS)
def test_the_five_names_are_exported(lib):
    exp = _exported(lib)
    assert [n for n in NAMES if n not in exp] == []


def test_the_partial_libraries_export_nothing_new():
    assert _exported("libscsamd_cones.so") == CONES_EXPORTS
    assert [n for n in _exported("libscsamd_linsys.so") if "cone" in n] == []


@pytest.mark.parametrize("lib", LIBS)
def test_width_rule(lib):
    L = capi.load(lib)
    got = {k: L.scs_amd_cone_multi_width(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 0, 17, -1)}
    assert got == {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 0: 0, 17: 0, -1: 0}
    assert got == {k: L.scs_amd_linsys_multi_width(k) for k in got}  # one layout for the block solve and the block projection


@pytest.mark.parametrize("lib", LIBS)
def test_bad_arguments_are_refused_before_any_device_call(lib):
    L = capi.load(lib)
    T = L._scs_types
    X = np.ones((6, 2), dtype=T.np_float, order="F")
    keep = X.copy()
    assert L.scs_amd_cone_proj_dual_multi(None, 2, X.ctypes.data_as(T.fp), 6, None) == -1
    never = C.c_void_p(X.ctypes.data)  # stands for a workspace / a device pointer; never dereferenced: these checks come first
    for nrhs in (0, -3):
        assert L.scs_amd_cone_proj_dual_multi(never, nrhs, X.ctypes.data_as(T.fp), 6, None) == -1
    assert L.scs_amd_cone_proj_dual_multi(never, 2, None, 6, None) == -1
    assert np.array_equal(X, keep)
    assert L.scs_amd_cone_proj_dual_dev(None, never, None) == -1
    assert L.scs_amd_cone_proj_dual_multi_dev(None, 2, never, None) == -1
    for nrhs in (0, 17, -1):
        assert L.scs_amd_cone_proj_dual_multi_dev(never, nrhs, never, None) == -1
    assert L.scs_amd_cone_sync(None) == -1


def test_python_module_checks_shapes_without_a_workspace():
    from scs_amd import cones
    m = 5
    X = np.zeros((m, 4))
    assert cones.check_block(m, X) == 4
    assert cones.check_block(m, np.asfortranarray(X), np.ones(m)) == 4
    assert cones.check_block(m, np.zeros((m, 1))) == 1
    for bad_X in (np.zeros(m), np.zeros((m + 1, 4)), np.zeros((m, 0)), np.zeros((4, m))):
        with pytest.raises(ValueError):
            cones.check_block(m, bad_X)
    for bad_r in (np.ones(m + 1), np.ones((m, 4)), np.zeros(m), -np.ones(m)):
        with pytest.raises(ValueError):
            cones.check_block(m, X, bad_r)


def test_python_object_raises_where_init_fails():
    from scs_amd import cones
    with pytest.raises(ValueError):
        cones.Cones(dict(l=3), D=np.ones(4))  # D of the wrong length: refused before the library is called
