"""scs_amd_family_set_values / scs_amd_solve_family_values / scs_amd_family_free_values (include/scs_amd.h): what can be checked
without a GPU -- exports, the refusals that need no workspace, the Python argument checks that raise before the library is called,
and the host helper that normalises a box cone's bounds with a column's own D."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi

NAMES = ("scs_amd_family_set_values", "scs_amd_solve_family_values", "scs_amd_family_free_values", "scs_amd_solve_family_values_refusal",
         "scs_amd_box_bounds")
LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so")
SCS_FAILED = -4


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", LIBS)
def test_the_names_are_exported(lib):
    exp = _exported(lib)
    assert [n for n in NAMES if n not in exp] == []


@pytest.mark.parametrize("lib", ("libscsamd_linsys.so", "libscsamd_cones.so"))
def test_the_partial_libraries_export_none_of_them(lib):
    assert [n for n in NAMES if n in _exported(lib)] == []


@pytest.mark.parametrize("lib", LIBS)
def test_refusals_that_need_no_workspace(lib):
    L = capi.load(lib)
    T = L._scs_types
    AX = np.ones((7, 2), dtype=T.np_float, order="F")
    B = np.ones((6, 2), dtype=T.np_float, order="F")
    fp = lambda a: a.ctypes.data_as(T.fp)
    sols, infos = (T.ScsSolution * 2)(), (T.ScsInfo * 2)()
    for k in (2, 0, 17):
        assert L.scs_amd_family_set_values(None, k, fp(AX), 7, None, 0) == SCS_FAILED
        assert L.scs_amd_solve_family_values(None, k, fp(B), 6, fp(B), 6, None, sols, infos, 0) == SCS_FAILED
    L.scs_amd_family_free_values(None)
    assert L.scs_amd_solve_family_values_refusal(None) is None
    assert np.all(AX == 1) and np.all(B == 1) and all(i.iter == 0 for i in infos)


# ---- the box cone's bounds under a column's own D: upload_box_bounds' formula, bu_j D_{j+1} / D_0 with 1e15 = infinite ----
@pytest.mark.parametrize("lib", LIBS)
def test_box_bounds_of_a_column(lib):
    L = capi.load(lib)
    T = L._scs_types
    f = T.np_float
    bu = np.array([1.0, 2.5, 1e15, 3e15, 0.0, 7.0], dtype=f)
    bl = np.array([-1.0, -1e15, -2.0, -4e15, 0.0, 6.0], dtype=f)
    k = capi.make_cone(dict(l=2, bu=bu, bl=bl, q=[3]), T)
    fp = lambda a: a.ctypes.data_as(T.fp)
    for D in (np.ones(7), np.array([2.0, 1.0, 0.5, 4.0, 8.0, 3.0, 0.25]), np.array([0.125, 3.0, 7.0, 1e-3, 1e3, 1.5, 2.0]),
              np.random.default_rng(1).uniform(0.1, 10.0, 7)):
        D = D.astype(f)
        hl, hu = np.full(6, 9.0, dtype=f), np.full(6, 9.0, dtype=f)
        assert L.scs_amd_box_bounds(C.byref(k), fp(D), fp(hl), fp(hu)) == 0
        fac = D[1:] / D[0]
        assert np.array_equal(hu, np.where(bu >= 1e15, np.inf, bu * fac).astype(f))
        assert np.array_equal(hl, np.where(bl <= -1e15, -np.inf, bl * fac).astype(f))
    hl, hu = np.zeros(6, dtype=f), np.zeros(6, dtype=f)
    assert L.scs_amd_box_bounds(C.byref(k), None, fp(hl), fp(hu)) == 0  # no scaling: as given, 1e15 stays a finite number
    assert np.array_equal(hl, bl) and np.array_equal(hu, bu)
    assert L.scs_amd_box_bounds(None, None, fp(hl), fp(hu)) == -1 and L.scs_amd_box_bounds(C.byref(k), None, None, fp(hu)) == -1


def test_values_block():
    f = np.float64
    V = np.full((9, 3), 0.5)
    out = capi.values_block(V, 9, "A", f)
    assert out.flags.f_contiguous and out.shape == (9, 3)
    assert capi.values_block(V.astype(np.float32), None, "A", f).dtype == f
    assert capi.values_block(np.tile(V, (1, 6))[:, :16], 9, "A", f).shape == (9, 16)
    for bad in (V[0], V[:-1], V.T, np.tile(V, (1, 6)), np.zeros((9, 0))):
        with pytest.raises(ValueError):
            capi.values_block(bad, 9, "A", f)
    for v in (np.nan, np.inf, -np.inf):
        W = V.copy()
        W[8, 2] = v
        with pytest.raises(ValueError, match="finite"):
            capi.values_block(W, 9, "A", f)


class _NoLibrary:
    """stands for the loaded library: any call into it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _object_without_a_workspace(n, m, with_P):
    """an SCS whose workspace cannot be reached: what its methods check, they check before any library call"""
    from scs_amd.solver import SCS
    s = SCS.__new__(SCS)
    s._lib, s._T, s._w = _NoLibrary(), capi.T64, 1
    A = sp.random(m, n, density=0.5, random_state=1, format="csc")
    P = sp.identity(n, format="csc") if with_P else None
    s._prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), P=P)
    return s, A, P


@pytest.mark.parametrize("with_P", [False, True])
def test_python_argument_checks_raise_before_any_library_call(with_P):
    n, m, K = 4, 6, 3
    s, A, P = _object_without_a_workspace(n, m, with_P)
    try:
        B, Cc = np.zeros((m, K)), np.zeros((n, K))
        mats = [A * (1.0 + 0.1 * k) for k in range(K)]
        Ps = [P * (1.0 + k) for k in range(K)] if with_P else None
        nnz = len(s._prob.Ax)
        other = A.tolil()
        other[:, :] = 1.0  # another pattern
        nonfinite = mats[1].copy()
        nonfinite.data[0] = np.inf
        cases = [dict(A=[mats[0], other.tocsc(), mats[2]], P=Ps),            # a pattern mismatch
                 dict(A=[mats[0], nonfinite, mats[2]], P=Ps),               # a non-finite value
                 dict(A=mats[:2], P=None if Ps is None else Ps[:2]),        # another K than B's
                 dict(A=np.ones((nnz - 1, K)), P=None if Ps is None else np.ones((n, K))),  # a short block
                 dict(A=np.ones(nnz), P=None if Ps is None else np.ones(n)),  # not 2-D
                 dict(A=[sp.random(m + 1, n, density=0.5, format="csc")] * K, P=Ps),  # another shape
                 dict(A=mats, P=Ps, stream=True),                            # the stream entry shares the values
                 dict(A=mats, P=Ps, own_values=True),                        # stored values or given ones, not both
                 dict(A=mats, P=None if with_P else [sp.identity(n, format="csc")] * K),  # P exactly when the object has one
                 dict(A=None, P=Ps if with_P else [sp.identity(n, format="csc")] * K),
                 dict(own_values=True, stream=True)]
        if with_P:
            cases.append(dict(A=mats, P=Ps[:2]))
            bad_p = [p.copy() for p in Ps]
            bad_p[2].data[0] = np.nan
            cases.append(dict(A=mats, P=bad_p))
        for kw in cases:
            with pytest.raises(ValueError):
                s.solve_family(B, Cc, **kw)
        with pytest.raises(ValueError):
            s.set_family_values([mats[0], other.tocsc()], None if Ps is None else Ps[:2])
        with pytest.raises(ValueError):
            s.set_family_values([], None if Ps is None else [])
        with pytest.raises(ValueError):
            s.set_family_values(np.ones((nnz, 17)), np.ones((n, 17)) if with_P else None)
    finally:
        s._w = None  # nothing to free
