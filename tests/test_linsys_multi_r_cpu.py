"""Every column of a block solve under its own diag_r (include/scs_amd.h: scs_amd_solve_lin_sys_multi_r,
scs_amd_linsys_mat_vec_multi_r_dev): what can be checked without a GPU -- exports, the refusals that come before any device call,
and the Python object's own checks."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from scs_amd import capi

NAMES = ("scs_amd_solve_lin_sys_multi_r", "scs_amd_linsys_mat_vec_multi_r_dev")
LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so", "libscsamd_linsys.so")
# what libscsamd_cones.so exported before this entry existed (scs_amd/csrc/exports_cones.map)
CONES_EXPORTS = {"_scs_init_cone", "_scs_proj_dual_cone", "_scs_finish_cone", "_scs_set_r_y", "_scs_enforce_cone_boundaries",
                 "_scs_validate_cones", "_scs_get_cone_header", "_scs_deep_copy_cone", "_scs_free_cone",
                 "scs_amd_device_count", "scs_amd_set_device", "scs_amd_test_fail_at", "scs_amd_device_free_bytes",
                 "scs_amd_set_option", "scs_amd_get_option", "scs_amd_list_options",
                 "scs_amd_cone_init", "scs_amd_cone_proj_dual", "scs_amd_cone_finish"}


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", LIBS)
def test_the_two_names_are_exported(lib):
    exp = _exported(lib)
    assert [n for n in NAMES if n not in exp] == []
    assert not any("cone" in n for n in NAMES)  # the linsys library exports nothing that names a cone


def test_cones_library_exports_what_it_exported():
    exp = _exported("libscsamd_cones.so")
    assert exp == CONES_EXPORTS, sorted(exp ^ CONES_EXPORTS)


@pytest.mark.parametrize("lib", LIBS)
def test_refusals_before_any_device_call(lib):
    """every refusal of the header comment, on a NULL workspace (nothing else can be created without a device) or with pointers
    that are never dereferenced; B stays as it was"""
    L = capi.load(lib)
    T = L._scs_types
    nm, K = 6, 2
    B = np.ones((nm, K), dtype=T.np_float, order="F")
    DR = np.ones((nm, K), dtype=T.np_float, order="F")
    tol = np.full(K, 1e-9, dtype=T.np_float)
    it = np.zeros(K, dtype=T.np_int)
    keep = B.copy()
    fp = lambda a: a.ctypes.data_as(T.fp)
    fn = L.scs_amd_solve_lin_sys_multi_r
    fake = C.c_void_p(B.ctypes.data)  # stands for a workspace; the pointer checks that are listed first never read it
    assert fn(None, K, fp(DR), nm, fp(B), nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(fake, K, None, nm, fp(B), nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(fake, K, fp(DR), nm, None, nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(fake, K, fp(DR), nm, fp(B), nm, None, 0, None, it.ctypes.data_as(T.ip)) == -1
    assert fn(fake, 0, fp(DR), nm, fp(B), nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(fake, -3, fp(DR), nm, fp(B), nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    # the checks that need the sizes of a workspace (leading dimensions, the entries of DR) can only be reached with one; without
    # a device they are made on a NULL workspace: refused, nothing read, nothing written (on a live workspace: the GPU suite)
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        D2 = DR.copy(order="F")
        D2[3, 1] = bad
        assert fn(None, K, fp(D2), nm, fp(B), nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(None, K, fp(DR), nm - 1, fp(B), nm, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(None, K, fp(DR), nm, fp(B), nm - 1, None, 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert fn(None, K, fp(DR), nm, fp(B), nm, fp(B), 0, fp(tol), it.ctypes.data_as(T.ip)) == -1
    assert np.array_equal(B, keep) and np.all(it == 0)
    mv = L.scs_amd_linsys_mat_vec_multi_r_dev
    dev = C.c_void_p(B.ctypes.data)  # never dereferenced
    assert mv(None, 2, dev, dev, dev) == -1
    for args in ((fake, 2, None, dev, dev), (fake, 2, dev, None, dev), (fake, 2, dev, dev, None)):
        assert mv(*args) == -1
    assert np.array_equal(B, keep)


def test_check_block_with_diag_r():
    from scs_amd import linsys
    n, m, K = 3, 5, 4
    B = np.zeros((n + m, K))
    DR = np.full((n + m, K), 0.5)
    assert linsys.check_block(n, m, B, None, 1e-9, DR) == K
    assert linsys.check_block(n, m, B, np.zeros((n, K)), np.full(K, 1e-6), DR=np.asfortranarray(DR)) == K
    assert linsys.check_block(n, m, B, DR=DR.astype(np.float32)) == K
    assert linsys.check_block(n, m, B, np.zeros((n, K)), 1e-6) == K  # the positional use of before
    for bad in (np.ones(n + m), np.ones((n + m, K - 1)), np.ones((n + m + 1, K)), np.ones((K, n + m)), np.ones((n + m, K, 1))):
        with pytest.raises(ValueError):
            linsys.check_block(n, m, B, DR=bad)
    for v in (0.0, -1e-3, np.nan, np.inf, -np.inf):
        D2 = DR.copy()
        D2[n, K - 1] = v
        with pytest.raises(ValueError):
            linsys.check_block(n, m, B, DR=D2)
