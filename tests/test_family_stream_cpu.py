"""scs_amd_solve_family_stream (include/scs_amd.h): what can be checked without a GPU -- where the three symbols are exported, that
the header declares them, the argument checks that come before the workspace is looked at, and the Python wrappers' own shape and
width checks.  A missing symbol is a failure here, not a skip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from scs_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so")
SYMBOLS = {"scs_amd_solve_family_stream", "scs_amd_solve_family_stream_refusal", "scs_amd_family_stream_get_counters"}
SCS_FAILED = -4


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("lib", FULL)
def test_the_full_libraries_export_the_three_symbols(lib):
    assert SYMBOLS <= _exported(lib)


@pytest.mark.parametrize("lib", ("libscsamd_linsys.so", "libscsamd_cones.so"))
def test_the_partial_libraries_do_not(lib):
    assert [s for s in _exported(lib) if "family_stream" in s] == []


def test_the_header_declares_them_with_the_documented_signatures():
    src = open(os.path.join(ROOT, "include", "scs_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(src.split())
    assert ("scs_int scs_amd_solve_family_stream(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, "
            "scs_int ldc, scs_int own_scale, const scs_float *scales, scs_int width, ScsSolution *sols, ScsInfo *infos, "
            "scs_int warm_start);") in flat
    assert "const char *scs_amd_solve_family_stream_refusal(const ScsWork *w, scs_int own_scale);" in flat
    assert "void scs_amd_family_stream_get_counters(const ScsWork *w, long long out[6]);" in flat


@pytest.mark.parametrize("lib", FULL)
def test_missing_arguments_and_a_bad_width_return_scs_failed_without_touching_the_outputs_or_the_device(lib):
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
    f = L.scs_amd_solve_family_stream
    never = C.c_void_p(X.ctypes.data)  # stands for a workspace; never dereferenced (nor written): these checks come first
    for own, s in ((1, sp), (1, None), (0, None)):
        for width in (0, 2, 16):
            assert f(None, K, bp, m, cp, n, own, s, width, sols, infos, 0) == SCS_FAILED
            assert f(never, K, None, m, cp, n, own, s, width, sols, infos, 0) == SCS_FAILED
            assert f(never, K, bp, m, None, n, own, s, width, sols, infos, 0) == SCS_FAILED
            assert f(never, K, bp, m, cp, n, own, s, width, None, infos, 0) == SCS_FAILED
            assert f(never, K, bp, m, cp, n, own, s, width, sols, None, 0) == SCS_FAILED
            for nprob in (0, -2):
                assert f(never, nprob, bp, m, cp, n, own, s, width, sols, infos, 0) == SCS_FAILED
        for width in (-1, 1, 3, 5, 6, 12, 17, 32):
            assert f(never, K, bp, m, cp, n, own, s, width, sols, infos, 0) == SCS_FAILED, width
    assert L.scs_amd_solve_family_stream_refusal(None, 0) is None and L.scs_amd_solve_family_stream_refusal(None, 1) is None
    out = (C.c_longlong * 6)(*([9] * 6))
    L.scs_amd_family_stream_get_counters(None, C.byref(out))
    assert list(out) == [0] * 6
    assert np.all(X == 7.0) and [infos[k].iter for k in range(K)] == [123] * K


def test_the_python_binding_checks_shapes_and_the_width_before_the_library_is_called():
    L = capi.load("libscsamd.so")
    ok = (np.zeros((5, 2)), np.zeros((3, 2)))
    with pytest.raises(ValueError):
        capi.solve_family_stream(L, None, np.zeros((5, 2)), np.zeros((3, 3)))  # K differs
    with pytest.raises(ValueError):
        capi.solve_family_stream(L, None, np.zeros(5), np.zeros((3, 1)))       # B is not a block
    for width in (3, 1, -2, 32, 4.0, None, True):
        with pytest.raises(ValueError, match="width"):
            capi.solve_family_stream(L, None, *ok, width=width)
    with pytest.raises(ValueError):
        capi.solve_family_stream(L, None, *ok, own_scale=True, scales=[0.1])            # one scale for two problems
    with pytest.raises(ValueError):
        capi.solve_family_stream(L, None, *ok, own_scale=True, scales=np.ones((2, 2)))  # not a vector


def test_the_solver_object_checks_the_width_before_the_library_is_called():
    """SCS.solve_family validates `width` before it looks at the workspace: an object whose workspace is a stand-in raises
    ValueError for a width that is no block width, and for a width without stream=True, and never reaches the library"""
    from scs_amd.solver import SCS

    class _Prob:
        m, n = 5, 3

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")
    s = SCS.__new__(SCS)
    s._w, s._prob, s._lib = 1, _Prob(), _NoLib()
    try:
        for width in (3, 0, 32, 2.0):
            with pytest.raises(ValueError, match="width"):
                s.solve_family(np.zeros((5, 2)), np.zeros((3, 2)), stream=True, width=width)
        with pytest.raises(ValueError, match="width"):
            s.solve_family(np.zeros((5, 2)), np.zeros((3, 2)), width=4)
    finally:
        s._w = None
