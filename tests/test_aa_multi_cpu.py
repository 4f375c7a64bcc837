"""A block of Anderson accelerations (include/scs_amd.h, scs_amd_aa_multi_*): what can be checked without a GPU -- exports, the
width rule, the argument checks that come before any device call, and the Python module's own checks."""
import subprocess

import numpy as np
import pytest

from scs_amd import capi

NAMES = ("scs_amd_aa_multi_width", "scs_amd_aa_multi_init", "scs_amd_aa_multi_apply", "scs_amd_aa_multi_safeguard",
         "scs_amd_aa_multi_apply_dev", "scs_amd_aa_multi_safeguard_dev", "scs_amd_aa_multi_reset", "scs_amd_aa_multi_get_stats",
         "scs_amd_aa_multi_get_counters", "scs_amd_aa_multi_finish")
LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so")


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", LIBS)
def test_the_block_entries_are_exported(lib):
    exp = _exported(lib)
    assert [n for n in NAMES if n not in exp] == []


def test_the_partial_libraries_do_not_export_them():
    for lib in ("libscsamd_linsys.so", "libscsamd_cones.so"):
        assert [n for n in _exported(lib) if "aa_multi" in n] == []


@pytest.mark.parametrize("lib", LIBS)
def test_width_rule(lib):
    L = capi.load(lib)
    assert [L.scs_amd_aa_multi_width(k) for k in (1, 2, 3, 4, 5, 16, 0, 17)] == [1, 2, 4, 4, 8, 16, 0, 0]
    got = {k: L.scs_amd_aa_multi_width(k) for k in range(-1, 19)}
    assert got == {k: L.scs_amd_linsys_multi_width(k) for k in got}  # one layout for every block entry


@pytest.mark.parametrize("lib", LIBS)
def test_bad_arguments_are_refused_before_any_device_call(lib):
    L = capi.load(lib)
    T = L._scs_types
    for nrhs in (0, 17, -1):
        assert not L.scs_amd_aa_multi_init(100, nrhs, 5, 5, 1, 1e-8, 1.0, 1.0, 1e10, 5)
    assert not L.scs_amd_aa_multi_init(0, 2, 5, 5, 1, 1e-8, 1.0, 1.0, 1e10, 5)
    F = np.ones((6, 2), dtype=T.np_float, order="F")
    keep = F.copy()
    nrm = np.full(2, 7.0, dtype=T.np_float)
    rej = np.full(2, 7, dtype=T.np_int)
    assert L.scs_amd_aa_multi_apply(None, F.ctypes.data_as(T.fp), 6, F.ctypes.data_as(T.fp), 6, None, nrm.ctypes.data_as(T.fp)) == -1
    assert L.scs_amd_aa_multi_safeguard(None, F.ctypes.data_as(T.fp), 6, F.ctypes.data_as(T.fp), 6, None, rej.ctypes.data_as(T.ip)) == -1
    assert L.scs_amd_aa_multi_apply_dev(None, None, None, None, nrm.ctypes.data_as(T.fp)) == -1
    assert L.scs_amd_aa_multi_safeguard_dev(None, None, None, None, rej.ctypes.data_as(T.ip)) == -1
    L.scs_amd_aa_multi_reset(None, -1)
    L.scs_amd_aa_multi_finish(None)
    assert np.array_equal(F, keep) and np.all(nrm == 7.0) and np.all(rej == 7)


def test_python_module_imports_and_checks_shapes_without_an_object():
    from scs_amd import accel
    assert accel.Accel.apply_many and accel.Accel.safeguard_many
    accel.check_block(5, 3, np.zeros((5, 3)))
    for bad in (np.zeros(5), np.zeros((5, 4)), np.zeros((6, 3)), np.zeros((3, 5))):
        with pytest.raises(ValueError):
            accel.check_block(5, 3, bad)
    assert accel.check_skip(3, None) is None
    with pytest.raises(ValueError):
        accel.check_skip(3, [0, 1])
    for ncols in (0, 17):
        with pytest.raises(ValueError):
            accel.Accel(10, ncols)  # refused by the width rule: no device call
