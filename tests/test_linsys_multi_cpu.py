"""Blocks of right-hand sides (include/scs_amd.h, B1: scs_amd_solve_lin_sys_multi and the block operator pieces): what can be
checked without a GPU -- exports, the width rule, the argument checks that come before any device call, and the Python object's
own checks."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi

NAMES = ("scs_amd_solve_lin_sys_multi", "scs_amd_linsys_multi_width", "scs_amd_linsys_mat_vec_multi_dev",
         "scs_amd_linsys_mul_a_multi_dev", "scs_amd_linsys_mul_at_multi_dev")
LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so", "libscsamd_linsys.so")


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", LIBS)
def test_the_five_names_are_exported(lib):
    exp = _exported(lib)
    assert [n for n in NAMES if n not in exp] == []


@pytest.mark.parametrize("lib", LIBS)
def test_width_rule(lib):
    L = capi.load(lib)
    got = {k: L.scs_amd_linsys_multi_width(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 0, 17, -1)}
    assert got == {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 0: 0, 17: 0, -1: 0}


@pytest.mark.parametrize("lib", LIBS)
def test_null_workspace_is_refused_before_any_device_call(lib):
    L = capi.load(lib)
    T = L._scs_types
    B = np.ones((6, 2), dtype=T.np_float, order="F")
    tol = np.full(2, 1e-9, dtype=T.np_float)
    it = np.zeros(2, dtype=T.np_int)
    keep = B.copy()
    assert L.scs_amd_solve_lin_sys_multi(None, 2, B.ctypes.data_as(T.fp), 6, None, 0, tol.ctypes.data_as(T.fp), it.ctypes.data_as(T.ip)) == -1
    assert np.array_equal(B, keep)
    dev = C.c_void_p(B.ctypes.data)  # never dereferenced: the workspace check comes first
    for fn in (L.scs_amd_linsys_mat_vec_multi_dev, L.scs_amd_linsys_mul_a_multi_dev, L.scs_amd_linsys_mul_at_multi_dev):
        assert fn(None, 2, dev, dev) == -1


def test_python_object_checks_shapes_without_a_workspace():
    from scs_amd import linsys
    n, m = 3, 5
    B = np.zeros((n + m, 4))
    assert linsys.check_block(n, m, B) == 4
    assert linsys.check_block(n, m, B, np.zeros((n, 4)), np.full(4, 1e-6)) == 4
    assert linsys.check_block(n, m, np.asfortranarray(B), None, 1e-3) == 4
    for bad_B in (np.zeros(n + m), np.zeros((n + m + 1, 4)), np.zeros((n + m, 0)), np.zeros((4, n + m))):
        with pytest.raises(ValueError):
            linsys.check_block(n, m, bad_B)
    for bad_S in (np.zeros(n), np.zeros((n, 3)), np.zeros((n + 1, 4)), np.zeros((4, n))):
        with pytest.raises(ValueError):
            linsys.check_block(n, m, B, bad_S)
    for bad_tol in (np.full(3, 1e-6), np.full((4, 1), 1e-6), 0.0, np.array([1e-6, 1e-6, -1.0, 1e-6])):
        with pytest.raises(ValueError):
            linsys.check_block(n, m, B, None, bad_tol)


def test_python_object_raises_where_init_fails():
    from scs_amd import linsys
    A = sp.random(5, 3, density=0.8, random_state=1, format="csc")
    with pytest.raises(ValueError):
        linsys.LinSys(A, np.ones(7))  # diag_r of the wrong length: refused before the library is called
    if capi.load("libscsamd.so").scs_amd_device_count() <= 0:
        with pytest.raises(ValueError):
            linsys.LinSys(A, np.ones(8))
