"""Device-resident Anderson acceleration (scs_amd/csrc/aa_dev.hip) vs the reference's
src/aa.c (oracle/_ref) and vs the host restatement, on the same fixed-point iteration.
The device path reorders the O(dim) sums, so agreement is to rounding amplified by the
(regularised) least-squares solve: 1e-6 relative on the iterates, identical accept /
reject and safeguard decisions."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from scs_amd import capi

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)


def _amd():
    amd = capi.load("libscsamd.so")
    for pre in ("scs_amd_aa_", "scs_amd_aa_dev_"):
        getattr(amd, pre + "init").restype = C.c_void_p
        getattr(amd, pre + "init").argtypes = [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int]
        getattr(amd, pre + "apply").restype = C.c_double
        getattr(amd, pre + "apply").argtypes = [dp, dp, C.c_void_p]
        getattr(amd, pre + "safeguard").restype = C.c_int
        getattr(amd, pre + "safeguard").argtypes = [dp, dp, C.c_void_p]
        getattr(amd, pre + "finish").argtypes = [C.c_void_p]
        getattr(amd, pre + "reset").argtypes = [C.c_void_p]
        getattr(amd, pre + "get_stats").argtypes = [C.c_void_p, C.POINTER(capi.T64.AaStats)]
    return amd


def _ref():
    ref = pyoracle.load_ref()
    ref.aa_init.restype = C.c_void_p
    ref.aa_init.argtypes = [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int, C.c_int]
    ref.aa_apply.restype = C.c_double
    ref.aa_apply.argtypes = [dp, dp, C.c_void_p]
    ref.aa_safeguard.restype = C.c_int
    ref.aa_safeguard.argtypes = [dp, dp, C.c_void_p]
    ref.aa_finish.argtypes = [C.c_void_p]
    ref.aa_get_stats.restype = capi.T64.AaStats  # returned by value; scs_int = int, scs_float = double in oracle/_ref
    ref.aa_get_stats.argtypes = [C.c_void_p]
    return ref


def _p(a):
    return a.ctypes.data_as(dp)


def _map(dim, seed):
    """A cheap contraction with a mild nonlinearity: banded mixing, no dense matrix."""
    rng = np.random.default_rng(seed)
    d0 = rng.uniform(0.3, 0.95, dim)
    d1 = rng.uniform(-0.02, 0.02, dim)
    c = rng.standard_normal(dim)
    return lambda v: d0 * v + d1 * np.roll(v, 1) + c + 0.03 * np.maximum(v, 0)


def _run(init, apply, safeguard, finish, extra, F, dim, mem, type1, reg, relax, iters=50, max_weight=1e10, x0=None,
         before_finish=None):
    a = init(dim, mem, mem, type1, reg, relax, 1.0, max_weight, 5, *extra)
    assert a
    x = np.zeros(dim) if x0 is None else x0.copy()
    x_prev = x.copy()
    norms, traj = [], []
    for i in range(iters):
        if i > 0:
            norms.append(apply(_p(x), _p(x_prev), a))
        x_prev = x.copy()
        x = F(x)
        rej = safeguard(_p(x), _p(x_prev), a)
        traj.append((rej, x.copy()))
    if before_finish:
        before_finish(a)
    finish(a)
    return norms, traj


CASES = [
    (1, 1e-8, 1.0, 10, 70001),   # SCS defaults (type-I, lookback 10); 21 panel columns = 2 batches
    (0, 1e-12, 1.0, 5, 5003),    # type-II
    (1, 1e-8, 1.3, 6, 40000),    # relaxation
    (1, -1e-6, 1.0, 4, 300),     # pinned regularisation, a single workgroup
    (0, 1e-10, 1.0, 20, 9000),   # lookback > one batch of pivot candidates
]


@pytest.mark.parametrize("type1,reg,relax,mem,dim", CASES)
def test_device_aa_matches_host_restatement(type1, reg, relax, mem, dim):
    amd = _amd()
    F = _map(dim, 7)
    nd, td = _run(amd.scs_amd_aa_dev_init, amd.scs_amd_aa_dev_apply, amd.scs_amd_aa_dev_safeguard,
                  amd.scs_amd_aa_dev_finish, (), F, dim, mem, type1, reg, relax)
    nh, th = _run(amd.scs_amd_aa_init, amd.scs_amd_aa_apply, amd.scs_amd_aa_safeguard,
                  amd.scs_amd_aa_finish, (), F, dim, mem, type1, reg, relax)
    assert [a[0] for a in td] == [b[0] for b in th]
    assert np.all(np.sign(nd) == np.sign(nh))
    assert any(v > 0 for v in nd)
    np.testing.assert_allclose(nd, nh, rtol=1e-5, atol=1e-9)
    for (_, xd), (_, xh) in zip(td, th):
        assert np.abs(xd - xh).max() <= 1e-6 * max(1.0, np.abs(xh).max())


@pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("type1,reg,relax,mem,dim", CASES[:3])
def test_device_aa_matches_reference(type1, reg, relax, mem, dim):
    amd, ref = _amd(), _ref()
    F = _map(dim, 11)
    nd, td = _run(amd.scs_amd_aa_dev_init, amd.scs_amd_aa_dev_apply, amd.scs_amd_aa_dev_safeguard,
                  amd.scs_amd_aa_dev_finish, (), F, dim, mem, type1, reg, relax)
    nr, tr = _run(ref.aa_init, ref.aa_apply, ref.aa_safeguard, ref.aa_finish, (0,), F, dim, mem, type1, reg, relax)
    assert [a[0] for a in td] == [b[0] for b in tr]
    assert np.all(np.sign(nd) == np.sign(nr))
    for (_, xd), (_, xr) in zip(td, tr):
        assert np.abs(xd - xr).max() <= 1e-6 * max(1.0, np.abs(xr).max())


def test_device_aa_reset_and_rejects_bad_parameters():
    amd = _amd()
    assert not amd.scs_amd_aa_dev_init(100, 5, 5, 1, 1e-8, 3.0, 1.0, 1e10, 5)   # relaxation out of range
    a = amd.scs_amd_aa_dev_init(1000, 5, 5, 1, 1e-8, 1.0, 1.0, 1e10, 5)
    F = _map(1000, 3)
    x = np.zeros(1000)
    for i in range(8):
        xp = x.copy()
        x = F(x)
        amd.scs_amd_aa_dev_apply(_p(x), _p(xp), a)
    amd.scs_amd_aa_dev_reset(a)
    xp = x.copy()
    x1 = F(x)
    keep = x1.copy()
    assert amd.scs_amd_aa_dev_apply(_p(x1), _p(xp), a) == 0.0   # first call after a reset only seeds
    np.testing.assert_array_equal(x1, keep)
    amd.scs_amd_aa_dev_finish(a)


# ---- rejected and degenerate solves --------------------------------------------------------------------------------
# Two settings under which src/aa.c rejects (or, for the identity under B, neither accepts nor rejects) every solve:
# the weight cap of 0.5 on a contraction, a rank-0 panel or gamma == 0 on the identity.  No step ever changes f, so
# the iterates are those of the plain iteration; what is compared is the bookkeeping: the counters against the
# reference's aa_get_stats, the signs of aa_norm, the safeguard decisions.  tests/test_aa_host.py runs the same
# cases through the host path and tests/test_aa_multi_gpu.py as columns of one block.
REJ_DIM, REJ_ITERS, REJ_CAP = 300, 50, 0.5
REJ_SETTINGS = {"A": (0, 1e-12, 5), "B": (1, -1e-6, 4)}  # type1, regularization, mem (= min_len)
REJ_MAPS = {"contraction100": 100, "identity": 500, "contraction101": 101}  # map -> seed of the start vector
COUNTERS = ("iter", "n_accept", "n_reject_lapack", "n_reject_rank0", "n_reject_nonfinite", "n_reject_weight_cap",
            "n_safeguard_reject", "last_rank")


def rej_map(name):
    return (lambda v: v.copy()) if name == "identity" else _map(REJ_DIM, REJ_MAPS[name])


def rej_start(name):
    return np.random.default_rng(REJ_MAPS[name]).standard_normal(REJ_DIM)


def counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


@functools.lru_cache(maxsize=None)
def rej_plain(name):
    """the iterates of x <- F(x), what every side has to reproduce bit for bit"""
    F, x, out = rej_map(name), rej_start(name), []
    for _ in range(REJ_ITERS):
        x = F(x)
        out.append(x.copy())
    return out


def rej_run(init, apply, safeguard, finish, extra, get_stats, setting, name):
    """(signs of aa_norm, safeguard decisions, iterates, counters) of one (setting, map) pair"""
    type1, reg, mem = REJ_SETTINGS[setting]
    got = {}
    norms, traj = _run(init, apply, safeguard, finish, extra, rej_map(name), REJ_DIM, mem, type1, reg, 1.0, iters=REJ_ITERS,
                       max_weight=REJ_CAP, x0=rej_start(name), before_finish=lambda a: got.update(st=counters(get_stats(a))))
    return np.sign(norms), [t[0] for t in traj], [t[1] for t in traj], got["st"]


@functools.lru_cache(maxsize=None)
def rej_reference(setting, name):
    ref = _ref()
    return rej_run(ref.aa_init, ref.aa_apply, ref.aa_safeguard, ref.aa_finish, (0,), ref.aa_get_stats, setting, name)


def rej_check(got, setting, name):
    signs, rejs, traj, st = got
    rsigns, rrejs, _, rst = rej_reference(setting, name)
    print(f"setting {setting}, {name}: counters {st}, reference {rst}")
    assert st == rst
    assert np.array_equal(signs, rsigns)
    assert rejs == rrejs
    for x, want in zip(traj, rej_plain(name)):
        assert np.array_equal(x.view(np.uint64), want.view(np.uint64))


def amd_stats(get_stats):
    def f(a):
        st = capi.T64.AaStats()
        get_stats(a, C.byref(st))
        return st
    return f


@pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", list(REJ_MAPS))
@pytest.mark.parametrize("setting", list(REJ_SETTINGS))
def test_device_aa_rejected_and_degenerate_solves_match_reference(setting, name):
    amd = _amd()
    rej_check(rej_run(amd.scs_amd_aa_dev_init, amd.scs_amd_aa_dev_apply, amd.scs_amd_aa_dev_safeguard,
                      amd.scs_amd_aa_dev_finish, (), amd_stats(amd.scs_amd_aa_dev_get_stats), setting, name), setting, name)
