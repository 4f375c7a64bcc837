"""scs_amd_solve_family_scaled (include/scs_amd.h): what can be checked without a GPU -- where the two symbols are exported, that the
header declares them, the argument checks that come before any device call, and the Python wrappers' own shape checks.  A missing
symbol is a failure here, not a skip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from scs_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so")
SCS_FAILED = -4


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", FULL)
def test_the_full_libraries_export_both_symbols(lib):
    assert {"scs_amd_solve_family_scaled", "scs_amd_solve_family_scaled_refusal"} <= _exported(lib)


@pytest.mark.parametrize("lib", ("libscsamd_linsys.so", "libscsamd_cones.so"))
def test_the_partial_libraries_do_not(lib):
    assert [s for s in _exported(lib) if "scaled" in s] == []


def test_the_header_declares_them_with_the_documented_signature():
    src = open(os.path.join(ROOT, "include", "scs_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(src.split())
    assert ("scs_int scs_amd_solve_family_scaled(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, "
            "scs_int ldc, const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start);") in flat
    assert "const char *scs_amd_solve_family_scaled_refusal(const ScsWork *w);" in flat


@pytest.mark.parametrize("lib", FULL)
def test_a_null_workspace_and_other_missing_arguments_return_scs_failed_without_touching_the_device(lib):
    L = capi.load(lib)
    T = L._scs_types
    m, n, K = 5, 3, 2
    B, Cc = np.ones((m, K), dtype=T.np_float, order="F"), np.ones((n, K), dtype=T.np_float, order="F")
    X = np.full((n + 2 * m, K), 7.0, dtype=T.np_float, order="F")
    scales = np.full(K, 0.1, dtype=T.np_float)
    sols, infos = (T.ScsSolution * K)(), (T.ScsInfo * K)()
    for k in range(K):
        base = X.ctypes.data + k * X.shape[0] * X.itemsize
        sols[k].x, sols[k].y, sols[k].s = (C.cast(base + o * X.itemsize, T.fp) for o in (0, n, n + m))
        infos[k].iter = 123
    bp, cp, sp = B.ctypes.data_as(T.fp), Cc.ctypes.data_as(T.fp), scales.ctypes.data_as(T.fp)
    f = L.scs_amd_solve_family_scaled
    for s in (sp, None):
        assert f(None, K, bp, m, cp, n, s, sols, infos, 0) == SCS_FAILED
        never = C.c_void_p(X.ctypes.data)  # stands for a workspace; never dereferenced: these checks come first
        assert f(never, K, None, m, cp, n, s, sols, infos, 0) == SCS_FAILED
        assert f(never, K, bp, m, None, n, s, sols, infos, 0) == SCS_FAILED
        assert f(never, K, bp, m, cp, n, s, None, infos, 0) == SCS_FAILED
        assert f(never, K, bp, m, cp, n, s, sols, None, 0) == SCS_FAILED
        for nprob in (0, -2):
            assert f(never, nprob, bp, m, cp, n, s, sols, infos, 0) == SCS_FAILED
    assert L.scs_amd_solve_family_scaled_refusal(None) is None
    assert np.all(X == 7.0) and [infos[k].iter for k in range(K)] == [123] * K


def test_the_python_binding_checks_shapes_before_the_library_is_called():
    L = capi.load("libscsamd.so")
    with pytest.raises(ValueError):
        capi.solve_family_scaled(L, None, np.zeros((5, 2)), np.zeros((3, 3)))  # K differs
    with pytest.raises(ValueError):
        capi.solve_family_scaled(L, None, np.zeros(5), np.zeros((3, 1)))       # B is not a block
    with pytest.raises(ValueError):
        capi.solve_family_scaled(L, None, np.zeros((5, 2)), np.zeros((3, 2)), scales=[0.1])            # one scale for two problems
    with pytest.raises(ValueError):
        capi.solve_family_scaled(L, None, np.zeros((5, 2)), np.zeros((3, 2)), scales=np.ones((2, 2)))  # not a vector


def test_the_solver_object_checks_the_length_of_scale_before_the_library_is_called():
    """SCS.solve_family validates its arguments before it looks at the workspace's settings: an object whose workspace is a stand-in
    raises ValueError for a `scale` of the wrong length and never reaches the library"""
    from scs_amd.solver import SCS

    class _Prob:
        m, n = 5, 3

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")
    s = SCS.__new__(SCS)
    s._w, s._prob, s._lib = 1, _Prob(), _NoLib()
    try:
        with pytest.raises(ValueError, match="scale"):
            s.solve_family(np.zeros((5, 2)), np.zeros((3, 2)), scale=[0.1, 0.2, 0.3])
    finally:
        s._w = None
