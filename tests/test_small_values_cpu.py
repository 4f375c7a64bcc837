"""scs_amd_small_set_values / scs_amd_small_solve_values / scs_amd_small_free_values: what needs no GPU.  Every refusal comes
before any device call (include/scs_amd.h), so the refusals of both entries, the Python argument checks and the exports are
checked here.  The checks of a solve's arguments come before the checks of the object's state (values set, their nprob), so every
one of them is reached without an accepted set call; the one refusal that needs an accepted set call first (a solve with another
nprob than the set call's) is in tests/test_small_values_gpu.py::test_life_cycle, which repeats the per-problem refusals with
values set.  test_the_reference_alone_is_stable_on_the_seeds runs no code of the library: it checks the seeds of
tests/small_values_util.py where oracle/_ref is built, and passes with or without the own-values entries."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi
from scs_amd.small import SmallBatch
from tests import small_values_util as V

ENTRIES = {"scs_amd_small_set_values", "scs_amd_small_solve_values", "scs_amd_small_free_values"}
OK = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)


def _lib():
    return capi.load("libscsamd.so")


def _prob(n=4, m=8, P=None, seed=0):
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(rng.uniform(-1, 1, (m, n)))
    return capi.Problem(A, rng.uniform(-1, 1, m), rng.uniform(-1, 1, n), dict(z=2, l=m - 2), P=P)


def _init(prob):
    lib = _lib()
    st = capi.default_settings(lib, **OK)
    h = lib.scs_amd_small_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    assert h and lib.scs_amd_small_refusal() is None
    return h


def _why(lib, word):
    why = lib.scs_amd_small_refusal()
    assert why and word in why.decode(), (word, why)


def test_set_values_refusals():
    lib = _lib()
    T = lib._scs_types
    K = 3
    plain, withp = _prob(), _prob(P=sp.csc_matrix(np.eye(4) + np.ones((4, 4))))
    nzA, nzP = len(plain.Ax), len(withp.Px)
    assert nzP == 10
    h, hp = _init(plain), _init(withp)
    AX = np.asfortranarray(np.repeat(plain.Ax[:, None], K, axis=1))
    PX = np.asfortranarray(np.repeat(withp.Px[:, None], K, axis=1))
    ax, px = AX.ctypes.data_as(T.fp), PX.ctypes.data_as(T.fp)

    def refused(word, *args):
        assert lib.scs_amd_small_set_values(*args) == -4
        _why(lib, word)

    refused("NULL", None, K, ax, nzA, None, 0)
    refused("NULL", h, K, None, nzA, None, 0)
    refused("without a P", h, K, ax, nzA, px, nzP)
    refused("PX missing", hp, K, ax, nzA, None, 0)
    refused("nprob", h, 0, ax, nzA, None, 0)
    refused("nprob", hp, -1, ax, nzA, px, nzP)
    refused("ldax", h, K, ax, nzA - 1, None, 0)
    refused("ldpx", hp, K, ax, nzA, px, nzP - 1)
    AX[5, 2] = np.nan
    refused("non-finite", h, K, ax, nzA, None, 0)
    refused("problem 2", h, K, ax, nzA, None, 0)
    AX[5, 2] = 0.0
    PX[1, 1] = np.inf
    refused("non-finite", hp, K, ax, nzA, px, nzP)
    refused("problem 1", hp, K, ax, nzA, px, nzP)
    lib.scs_amd_small_free_values(h)  # nothing set: fine
    lib.scs_amd_small_free_values(None)
    lib.scs_amd_small_finish(h)
    lib.scs_amd_small_finish(hp)


def test_solve_values_refusals_leave_the_outputs_untouched():
    lib = _lib()
    T = lib._scs_types
    prob = _prob()
    h = _init(prob)
    n, m, K = prob.n, prob.m, 3
    rng = np.random.default_rng(1)
    B, Cc = np.asfortranarray(rng.uniform(-1, 1, (m, K))), np.asfortranarray(rng.uniform(-1, 1, (n, K)))
    X, Y, S = np.full((n, K), 7.0, order="F"), np.full((m, K), 8.0, order="F"), np.full((m, K), 9.0, order="F")
    sols, infos = (T.ScsSolution * K)(), (T.ScsInfo * K)()
    for k in range(K):
        sols[k].x = C.cast(X.ctypes.data + 8 * k * n, T.fp)
        sols[k].y = C.cast(Y.ctypes.data + 8 * k * m, T.fp)
        sols[k].s = C.cast(S.ctypes.data + 8 * k * m, T.fp)
        infos[k].iter = 1234
    bp, cp = B.ctypes.data_as(T.fp), Cc.ctypes.data_as(T.fp)

    def refused(word, *args):
        assert lib.scs_amd_small_solve_values(*args) == -4
        _why(lib, word)
        assert np.all(X == 7.0) and np.all(Y == 8.0) and np.all(S == 9.0) and all(infos[k].iter == 1234 for k in range(K))

    refused("nprob", h, 0, bp, m, cp, n, sols, infos, 0)
    refused("NULL", None, K, bp, m, cp, n, sols, infos, 0)
    refused("NULL", h, K, None, m, cp, n, sols, infos, 0)
    refused("NULL", h, K, bp, m, None, n, sols, infos, 0)
    refused("NULL", h, K, bp, m, cp, n, None, infos, 0)
    refused("NULL", h, K, bp, m, cp, n, sols, None, 0)
    refused("leading dimension", h, K, bp, m - 1, cp, n, sols, infos, 0)
    refused("leading dimension", h, K, bp, m, cp, n - 1, sols, infos, 0)
    B[2, 1] = np.nan
    refused("non-finite", h, K, bp, m, cp, n, sols, infos, 0)
    refused("problem 1", h, K, bp, m, cp, n, sols, infos, 0)
    B[2, 1] = 0.0
    Cc[0, 2] = -np.inf
    refused("non-finite", h, K, bp, m, cp, n, sols, infos, 0)
    refused("problem 2", h, K, bp, m, cp, n, sols, infos, 0)
    Cc[0, 2] = 0.0
    for field, arr in (("x", X), ("y", Y), ("s", S)):
        setattr(sols[1], field, None)
        refused("sols[1]", h, K, bp, m, cp, n, sols, infos, 0)
        refused("NULL", h, K, bp, m, cp, n, sols, infos, 0)
        setattr(sols[1], field, C.cast(arr.ctypes.data + 8 * arr.shape[0], T.fp))  # a field read back aliases the struct: set it anew
    refused("no values are set", h, K, bp, m, cp, n, sols, infos, 0)  # a solve before a set call: the last check
    lib.scs_amd_small_finish(h)


def test_python_checks():
    rng = np.random.default_rng(2)
    n, m, K = 4, 8, 3
    A = sp.csc_matrix(rng.uniform(-1, 1, (m, n)))
    P = sp.csc_matrix(np.eye(n))
    B, Cc = rng.uniform(-1, 1, (m, K)), rng.uniform(-1, 1, (n, K))
    with SmallBatch(dict(A=A, b=np.zeros(m), c=np.zeros(n)), dict(z=2, l=6)) as sb:
        other = A.copy().tolil()
        other[3, 1] = 0.0  # one entry fewer: another pattern
        with pytest.raises(ValueError, match="pattern"):
            sb.set_values([A, sp.csc_matrix(other), A])
        with pytest.raises(ValueError, match="shape"):
            sb.set_values([A[:, :3]])
        with pytest.raises(ValueError, match="nnz x K"):
            sb.set_values(np.zeros((A.nnz - 1, K)))
        with pytest.raises(ValueError, match="empty"):
            sb.set_values([])
        with pytest.raises(ValueError, match="exactly when"):
            sb.set_values([A] * K, [P] * K)
        bad = np.repeat(A.data[:, None], K, axis=1)
        bad[0, 1] = np.nan
        with pytest.raises(ValueError, match="non-finite.*problem 1"):
            sb.set_values(bad)
        with pytest.raises(ValueError, match="no values are set"):
            sb.solve(B, Cc, own_values=True)
        nan_B = B.copy()
        nan_B[1, 2] = np.nan
        for kw in (dict(own_values=True), dict(A=[A] * K)):  # B and C are checked before the values are touched
            with pytest.raises(ValueError, match="finite"):
                sb.solve(nan_B, Cc, **kw)
            with pytest.raises(ValueError, match="m x K"):
                sb.solve(B[:-1], Cc, **kw)
            with pytest.raises(ValueError, match="warm"):
                sb.solve(B, Cc, warm=(np.zeros((n, K)),), **kw)
        with pytest.raises(ValueError, match="needs A="):
            sb.solve(B, Cc, P=[P] * K)
        sb.free_values()
    with SmallBatch(dict(A=A, P=P, b=np.zeros(m), c=np.zeros(n)), dict(z=2, l=6)) as sb:
        with pytest.raises(ValueError, match="exactly when"):
            sb.set_values([A] * K)
        with pytest.raises(ValueError, match="A holds 3 problems and P 2"):
            sb.set_values([A] * K, [P] * 2)
        with pytest.raises(ValueError, match="pattern"):
            sb.set_values([A] * K, [sp.csc_matrix(np.eye(n) + np.ones((n, n)))] * K)
    with pytest.raises(RuntimeError, match="closed"):
        sb.set_values([A])


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_exports():
    for lib in ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so"):
        assert ENTRIES <= _exported(lib), lib
    for lib in ("libscsamd_linsys.so", "libscsamd_cones.so"):
        assert not ENTRIES & _exported(lib), lib


@pytest.mark.parametrize("name", sorted(V.SEEDS))
def test_the_reference_alone_is_stable_on_the_seeds(name):
    """the serial and the OpenMP build of the exact-solve reference, a fresh scs_init per problem: the same iter and status_val"""
    from oracle import pyoracle
    for lib in ("libscsindir_ref_exactcg.so", "libscsindir_ref_exactcg_omp.so"):
        if not pyoracle.ref_available(lib):
            pytest.skip(f"oracle/_ref/{lib} not built")
    ok, its = V.reference_is_stable(pyoracle.load_ref("libscsindir_ref_exactcg.so"), pyoracle.load_ref("libscsindir_ref_exactcg_omp.so"), name)
    print(name, its)
    assert ok, (name, its)
