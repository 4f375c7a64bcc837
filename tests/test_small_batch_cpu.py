"""scs_amd_small_*: what needs no GPU.  Init is host work and every refusal comes before any device call (include/scs_amd.h), so
the refusals of init AND of solve, the limits, the Python argument checks and the exports are checked here."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, small
from scs_amd.small import SmallBatch

ENTRIES = {"scs_amd_small_init", "scs_amd_small_refusal", "scs_amd_small_limits", "scs_amd_small_solve", "scs_amd_small_set_grid",
           "scs_amd_small_get_counters", "scs_amd_small_get_occupancy", "scs_amd_small_finish"}
OK = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)


def _lib():
    return capi.load("libscsamd.so")


def _prob(n=4, m=8, cone=None, P=None, seed=0):
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(rng.uniform(-1, 1, (m, n)))
    return capi.Problem(A, rng.uniform(-1, 1, m), rng.uniform(-1, 1, n), cone or dict(z=2, l=m - 2), P=P)


def _init(prob, **over):
    lib = _lib()
    st = capi.default_settings(lib, **dict(OK, **over))
    h = lib.scs_amd_small_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    why = lib.scs_amd_small_refusal()
    return h, (why.decode() if why else None)


def _refused(prob, *words, **over):
    h, why = _init(prob, **over)
    assert not h and why, (words, why)
    for w in words:
        assert w in why, (w, why)


def test_limits():
    n, l = small.limits()
    assert n >= 128 and l >= 1024


@pytest.mark.parametrize("cone,m,word", [
    (dict(z=1, l=2, bu=[1.0, 2.0], bl=[-1.0, -2.0]), 6, "box"),
    (dict(l=2, s=[3]), 8, "PSD"),
    (dict(l=2, cs=[2]), 6, "complex PSD"),
    (dict(l=2, ep=1), 5, "exponential"),
    (dict(l=2, ed=1), 5, "exponential"),
    (dict(l=2, p=[0.3]), 5, "power"),
])
def test_init_refuses_cones(cone, m, word):
    _refused(_prob(3, m, cone), word)


@pytest.mark.parametrize("over,word", [
    (dict(adaptive_scale=1), "adaptive_scale"),
    (dict(acceleration_lookback=10), "acceleration_lookback"),
    (dict(time_limit_secs=1.0), "time_limit_secs"),
    (dict(log_csv_filename=b"small_batch_never_written.csv"), "log_csv_filename"),
    (dict(write_data_filename=b"small_batch_never_written.dat"), "write_data_filename"),
])
def test_init_refuses_settings(over, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _refused(_prob(), word, **over)
    assert not list(tmp_path.iterdir())  # refused before anything was written


def test_init_refuses_sizes_over_each_limit():
    nmax, lmax = small.limits()
    _refused(_prob(nmax + 1, nmax + 3), "n =", str(nmax))
    _refused(_prob(8, lmax - 8), "n + m + 1 =", str(lmax))
    h, why = _init(_prob(8, lmax - 9))  # exactly at the limit: served
    assert h and why is None
    _lib().scs_amd_small_finish(h)


def test_init_refuses_null_and_non_finite():
    lib = _lib()
    prob = _prob()
    st = capi.default_settings(lib, **OK)
    for args in ((None, C.byref(prob.k), C.byref(st)), (C.byref(prob.data), None, C.byref(st)), (C.byref(prob.data), C.byref(prob.k), None)):
        assert not lib.scs_amd_small_init(*args)
        assert b"NULL" in lib.scs_amd_small_refusal()
    bad = _prob()
    bad.Ax[3] = np.nan
    _refused(bad, "non-finite", "A")
    P = sp.csc_matrix(np.eye(4))
    badp = _prob(P=P)
    badp.Px[1] = np.inf
    _refused(badp, "non-finite", "P")
    indefinite = _prob(P=sp.csc_matrix(-5.0 * np.eye(4)))
    _refused(indefinite, "positive definite")


def test_solve_refusals_leave_the_outputs_untouched():
    lib = _lib()
    T = lib._scs_types
    prob = _prob()
    h, why = _init(prob)
    assert h and why is None
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
        assert lib.scs_amd_small_solve(*args) == -4
        why = lib.scs_amd_small_refusal()
        assert why and word in why.decode(), (word, why)
        assert np.all(X == 7.0) and np.all(Y == 8.0) and np.all(S == 9.0) and all(infos[k].iter == 1234 for k in range(K))

    refused("nprob", h, 0, bp, m, cp, n, sols, infos, 0)
    refused("nprob", h, -2, bp, m, cp, n, sols, infos, 0)
    refused("NULL", None, K, bp, m, cp, n, sols, infos, 0)
    refused("NULL", h, K, None, m, cp, n, sols, infos, 0)
    refused("NULL", h, K, bp, m, None, n, sols, infos, 0)
    refused("NULL", h, K, bp, m, cp, n, None, infos, 0)
    refused("NULL", h, K, bp, m, cp, n, sols, None, 0)
    refused("leading dimension", h, K, bp, m - 1, cp, n, sols, infos, 0)
    refused("leading dimension", h, K, bp, m, cp, n - 1, sols, infos, 0)
    B[2, 1] = np.nan
    refused("non-finite", h, K, bp, m, cp, n, sols, infos, 0)
    B[2, 1] = 0.0
    Cc[0, 2] = -np.inf
    refused("non-finite", h, K, bp, m, cp, n, sols, infos, 0)
    Cc[0, 2] = 0.0
    keep = sols[1].y
    sols[1].y = None
    refused("NULL", h, K, bp, m, cp, n, sols, infos, 0)
    sols[1].y = keep
    # an accepted init clears the message; set_grid checks its argument without a device
    assert lib.scs_amd_small_set_grid(h, -1) == -1 and lib.scs_amd_small_set_grid(h, 3) == 0
    out = (C.c_longlong * 4)()
    lib.scs_amd_small_get_counters(h, C.byref(out))
    assert list(out) == [0, 0, 0, 0]
    lib.scs_amd_small_finish(h)
    lib.scs_amd_small_finish(None)


def test_python_argument_checks():
    rng = np.random.default_rng(2)
    n, m = 4, 8
    A = sp.csc_matrix(rng.uniform(-1, 1, (m, n)))
    data = dict(A=A, b=np.zeros(m), c=np.zeros(n))
    with pytest.raises(ValueError, match="adaptive_scale"):
        SmallBatch(data, dict(z=2, l=6), adaptive_scale=1)
    with pytest.raises(ValueError, match="PSD"):
        SmallBatch(data, dict(l=2, s=[3]))
    with pytest.raises(ValueError, match="must contain"):
        SmallBatch(dict(A=A), dict(z=2, l=6))
    with SmallBatch(data, dict(z=2, l=6)) as sb:
        assert sb.limits == small.limits() and (sb.n, sb.m) == (n, m)
        good_B, good_C = rng.uniform(-1, 1, (m, 3)), rng.uniform(-1, 1, (n, 3))
        for B, Cc in ((good_B[:-1], good_C), (good_B, good_C[:, :2]), (good_B[:, :0], good_C[:, :0]), (good_B.ravel(), good_C),
                      (np.zeros((m, 3, 1)), good_C)):
            with pytest.raises(ValueError, match="m x K"):
                sb.solve(B, Cc)
        with pytest.raises(ValueError, match="numeric"):
            sb.solve([["a"] * 3] * m, good_C)
        bad = good_B.copy()
        bad[0, 0] = np.nan
        with pytest.raises(ValueError, match="finite"):
            sb.solve(bad, good_C)
        with pytest.raises(ValueError, match="warm"):
            sb.solve(good_B, good_C, warm=(np.zeros((n, 3)), np.zeros((m, 3))))
        with pytest.raises(ValueError, match="shape"):
            sb.solve(good_B, good_C, warm=(np.zeros((n, 2)), np.zeros((m, 3)), np.zeros((m, 3))))
        for g in (-1, 1.5, True, "2"):
            with pytest.raises(ValueError, match="workgroups"):
                sb.set_grid(g)
        sb.set_grid(0)
        assert sb.counters() == dict(launches=0, workgroups=0, problems=0, iterations=0)
    sb.close()  # twice is fine
    with pytest.raises(RuntimeError, match="closed"):
        sb.solve(good_B, good_C)


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_exports():
    for lib in ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so"):
        assert ENTRIES <= _exported(lib), lib
    for lib in ("libscsamd_linsys.so", "libscsamd_cones.so"):
        assert not {s for s in _exported(lib) if s.startswith("scs_amd_small")}, lib
