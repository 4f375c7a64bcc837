"""Every column of a block with its own values of A and P (include/scs_amd.h: scs_amd_linsys_set_values_multi,
scs_amd_solve_lin_sys_multi_v, scs_amd_linsys_mat_vec_multi_v_dev, scs_amd_linsys_free_values_multi): what can be checked without a
GPU -- exports, the refusals that need no workspace, and the Python object's own argument checks."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from scs_amd import capi

NAMES = ("scs_amd_linsys_set_values_multi", "scs_amd_solve_lin_sys_multi_v", "scs_amd_linsys_mat_vec_multi_v_dev",
         "scs_amd_linsys_free_values_multi")
LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so", "libscsamd_linsys.so")


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", LIBS)
def test_the_four_names_are_exported(lib):
    exp = _exported(lib)
    assert [n for n in NAMES if n not in exp] == []


def test_cones_library_exports_none_of_them():
    assert [n for n in NAMES if n in _exported("libscsamd_cones.so")] == []


@pytest.mark.parametrize("lib", LIBS)
def test_refusals_that_need_no_workspace(lib):
    """w = NULL, and the NULL pointers that are checked before the workspace is read (`fake` stands for one and is never
    dereferenced); nothing is written"""
    L = capi.load(lib)
    T = L._scs_types
    nnz, nm, K = 7, 6, 2
    AX = np.ones((nnz, K), dtype=T.np_float, order="F")
    B = np.ones((nm, K), dtype=T.np_float, order="F")
    DR = np.ones((nm, K), dtype=T.np_float, order="F")
    tol = np.full(K, 1e-9, dtype=T.np_float)
    it = np.zeros(K, dtype=T.np_int)
    keep = B.copy()
    fp = lambda a: a.ctypes.data_as(T.fp)
    ip = it.ctypes.data_as(T.ip)
    fake = C.c_void_p(B.ctypes.data)
    setv, solve, mv = L.scs_amd_linsys_set_values_multi, L.scs_amd_solve_lin_sys_multi_v, L.scs_amd_linsys_mat_vec_multi_v_dev
    for k in (K, 0, 17, -1):
        assert setv(None, k, fp(AX), nnz, None, 0) == -1
        assert solve(None, k, fp(DR), nm, fp(B), nm, None, 0, fp(tol), ip) == -1
        assert solve(None, k, None, 0, fp(B), nm, None, 0, fp(tol), ip) == -1
        assert mv(None, k, fake, fake, fake) == -1
    assert setv(fake, K, None, nnz, None, 0) == -1
    assert solve(fake, K, fp(DR), nm, None, nm, None, 0, fp(tol), ip) == -1
    assert solve(fake, K, fp(DR), nm, fp(B), nm, None, 0, None, ip) == -1
    assert mv(fake, K, fake, None, fake) == -1 and mv(fake, K, fake, fake, None) == -1
    L.scs_amd_linsys_free_values_multi(None)  # NULL-safe
    assert np.array_equal(B, keep) and np.all(it == 0) and np.all(AX == 1)


def test_check_values_block():
    from scs_amd import linsys
    nnz_a, nnz_p, K = 9, 4, 3
    AX, PX = np.full((nnz_a, K), 0.5), np.full((nnz_p, K), 2.0)
    assert linsys.check_values_block(nnz_a, None, AX, None) == K
    assert linsys.check_values_block(nnz_a, nnz_p, np.asfortranarray(AX), PX.astype(np.float32)) == K
    assert linsys.check_values_block(nnz_a, None, AX[:, :1], None) == 1
    assert linsys.check_values_block(nnz_a, None, np.tile(AX, (1, 6))[:, :16], None) == 16
    assert linsys.check_values_block(0, 0, np.zeros((0, 2)), np.zeros((0, 2))) == 2
    bad = [(AX[0], None, None), (AX[:-1], None, None), (AX.T, None, None), (np.tile(AX, (1, 6)), None, None), (np.zeros((nnz_a, 0)), None, None),
           (AX, PX, None),          # P values for a workspace without P
           (AX, None, nnz_p),       # none for a workspace with P
           (AX, PX[:, :2], nnz_p), (AX, PX[:-1], nnz_p), (AX, PX[:, 0], nnz_p)]
    for a, p, np_ in bad:
        with pytest.raises(ValueError):
            linsys.check_values_block(nnz_a, np_, a, p)
    for v in (np.nan, np.inf, -np.inf):
        A2, P2 = AX.copy(), PX.copy()
        A2[nnz_a - 1, K - 1] = v
        P2[0, 1] = v
        with pytest.raises(ValueError):
            linsys.check_values_block(nnz_a, None, A2, None)
        with pytest.raises(ValueError):
            linsys.check_values_block(nnz_a, nnz_p, AX, P2)


class _NoLibrary:
    """stands for the loaded library: any call into it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _object_without_a_workspace(n, m, with_P):
    """a LinSys whose workspace cannot be reached: what its methods check, they check before any library call"""
    import scipy.sparse as sp
    from scs_amd.linsys import LinSys
    ls = LinSys.__new__(LinSys)
    ls._lib, ls._T, ls._w, ls._vcols = _NoLibrary(), capi.T64, 1, 0
    ls.n, ls.m = n, m
    A = sp.random(m, n, density=0.5, random_state=1, format="csc")
    P = sp.identity(n, format="csc") if with_P else None
    ls._prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), P=P)
    return ls


def test_python_argument_checks_raise_before_any_library_call():
    n, m, K = 4, 6, 3
    for with_P in (False, True):
        ls = _object_without_a_workspace(n, m, with_P)
        try:
            nnz = len(ls._prob.Ax)
            AX, PX = np.ones((nnz, K)), (np.ones((n, K)) if with_P else None)
            for a, p in ((AX[:-1], PX), (AX[:, 0], PX), (np.tile(AX, (1, 6)), None if PX is None else np.tile(PX, (1, 6))),
                         (np.where(AX > 0, np.inf, AX), PX), (AX, np.ones((n, K)) if not with_P else None)):
                with pytest.raises(ValueError):
                    ls.set_values_many(a, p)
            B, S = np.zeros((n + m, K)), np.zeros((n, K))
            with pytest.raises(ValueError):
                ls.solve_many(B, S, 1e-9, own_values=True)  # no values are set
            ls._vcols = K + 1
            with pytest.raises(ValueError):
                ls.solve_many(B, S, 1e-9, own_values=True)  # another K than the set call's
            ls._vcols = K
            with pytest.raises(ValueError):
                ls.solve_many(B, S, 1e-9, diag_r=-np.ones((n + m, K)), own_values=True)
            with pytest.raises(ValueError):
                ls.solve_many(B[:-1], S, 1e-9, own_values=True)
        finally:
            ls._w = None  # nothing to free
