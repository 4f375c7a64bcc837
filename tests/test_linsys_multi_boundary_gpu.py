"""The host boundary that the three block solves share (scs_amd_solve_lin_sys_multi, _multi_r, _multi_v; solve_multi_host in
scs_amd/csrc/linsys.hip): what one staging sequence for three entries could get wrong and the suites of the entries do not pin.

 1. gapped leading dimensions: lddr, ldb and lds larger than their columns, the gaps NaN-filled, through every entry, at K = 1, 3, 16
    and -- where the entry chunks -- 17, whose second chunk starts at an offset in all three host arrays at once;
 2. the same inputs through all three entries: the workspace's diag_r in every column of DR, the workspace's values in every column;
 3. a refused call leaves the workspace as it was: the next valid call of every entry returns the bits it returned before.
Every assertion is an equality of bits between two calls of the library; the tight-dimension calls are tied to the reference backend
by tests/test_linsys_multi_gpu.py, test_linsys_multi_r_gpu.py and test_linsys_multi_v_gpu.py.  Two legs of item 2 are held there
already and are not asserted again here (HELD_MULTI_R, HELD_MULTI_V below).  The systems here are small: n = 24, m = 40."""
import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi
from tests import probgen
from tests.test_linsys_multi_gpu import _init, _multi
from tests.test_linsys_multi_r_gpu import _bits, _drs, _multi_r
from tests.test_linsys_multi_v_gpu import _multi_v, _p_values, _perturbed, _set_values
# the tests that already hold a leg of item 2 (imported, so that renaming or removing one shows up here), and the cases they hold
from tests.test_linsys_multi_r_gpu import test_bit_identities as _held_multi_r  # multi == multi_r: K = 2, 5, warm and cold, without P
from tests.test_linsys_multi_v_gpu import test_workspace_values_in_every_column_give_the_shared_value_solves as _held_multi_v  # multi == multi_v, DR null: K = 5, warm, with and without P
HELD_MULTI_R = lambda warm, with_P, K: callable(_held_multi_r) and not with_P
HELD_MULTI_V = lambda warm, with_P, K: callable(_held_multi_v) and K == 5 and warm

pytestmark = pytest.mark.gpu

N, M, TOL = 24, 40, 1e-9


def _system(with_P, K, seed=0):
    """A (M x N, 3 or 4 entries per column), P or None, diag_r, K right-hand sides and K warm starts"""
    rng = np.random.default_rng(100 + seed)
    A = probgen.random_csc(M, N, 3 + seed % 2, seed=7 + seed)
    P = None
    if with_P:
        Bm = sp.random(N, N, density=0.15, random_state=5 + seed, format="csc")
        P = (Bm @ Bm.T + sp.identity(N) * 0.1).tocsc()
    prob = capi.Problem(A, np.zeros(M), np.zeros(N), dict(l=M), P=P)
    dr = probgen.diag_r(N, M, z=M // 10)
    return prob, dr, rng.uniform(-1, 1, (N + M, K)), rng.uniform(-1, 1, (N, K)) * 0.1


def _own_columns(prob, with_P, K, seed=0):
    """per-column diag_r, values of A and (with P) of the upper P for K columns"""
    rng = np.random.default_rng(200 + seed)
    DR = _drs(N, M, M // 10, np.geomspace(0.03, 3.0, K))
    return DR, _perturbed(prob.Ax, K, rng), (_p_values(prob, DR, K, rng) if with_P else None)


# ---- 1. gapped leading dimensions ----
ENTRIES = {
    "multi": lambda lib, w, DR, B, S, **ld: _multi(lib, w, B, S, TOL, **{k: v for k, v in ld.items() if k != "lddr"}),
    "multi_r": lambda lib, w, DR, B, S, **ld: _multi_r(lib, w, DR, B, S, TOL, **ld),
    "multi_v_dr": lambda lib, w, DR, B, S, **ld: _multi_v(lib, w, DR, B, S, TOL, **ld),
    "multi_v": lambda lib, w, DR, B, S, **ld: _multi_v(lib, w, None, B, S, TOL, **{k: v for k, v in ld.items() if k != "lddr"}),
}
GAPPED = [(e, K) for e in ENTRIES for K in (1, 3, 16, 17) if K < 17 or e in ("multi", "multi_r")]


@pytest.mark.parametrize("entry,K", GAPPED)
def test_gapped_leading_dimensions(entry, K):
    amd = capi.load("libscsamd_linsys.so")
    prob, dr, B, S = _system(False, K, seed=K)
    DR, AX, _ = _own_columns(prob, False, K, seed=K)
    w = _init(amd, prob, dr)
    try:
        if entry.startswith("multi_v"):
            _set_values(amd, w, AX, None)
        call = ENTRIES[entry]
        tight, it_t = call(amd, w, DR, B, S)
        wide, it_w = call(amd, w, DR, B, S, lddr=N + M + 7, ldb=N + M + 13, lds=N + 5)  # the helpers assert that the NaN gaps are still NaN
        assert np.all(it_t >= 0) and np.all(np.isfinite(tight))
        assert np.array_equal(_bits(wide), _bits(tight)), "the solutions depend on the leading dimensions"
        assert np.array_equal(it_w, it_t), "the iteration counts depend on the leading dimensions"
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 2. the same inputs through all three entries ----
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("with_P", [False, True])
@pytest.mark.parametrize("warm", [False, True])
def test_same_inputs_through_all_three_entries(warm, with_P, K):
    amd = capi.load("libscsamd_linsys.so")
    prob, dr, B, S = _system(with_P, K)
    if not warm:
        S = None
    w = _init(amd, prob, dr, with_P)
    try:
        shared, it_s = _multi(amd, w, B, S, TOL)
        assert np.any(it_s > 0)
        if not HELD_MULTI_R(warm, with_P, K):
            XY, it = _multi_r(amd, w, np.tile(dr[:, None], (1, K)), B, S, TOL)
            assert np.array_equal(_bits(XY), _bits(shared)) and np.array_equal(it, it_s), "the workspace's diag_r in every column of DR"
        if not HELD_MULTI_V(warm, with_P, K):
            _set_values(amd, w, np.tile(prob.Ax[:, None], (1, K)), np.tile(prob.Px[:, None], (1, K)) if with_P else None)
            XY, it = _multi_v(amd, w, None, B, S, TOL)
            assert np.array_equal(_bits(XY), _bits(shared)) and np.array_equal(it, it_s), "the workspace's values in every column, DR null"
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 3. a refusal leaves the workspace usable ----
@pytest.mark.parametrize("with_P", [False, True])
def test_a_refusal_leaves_the_workspace_as_it_was(with_P):
    amd = capi.load("libscsamd_linsys.so")
    T = amd._scs_types
    K = 3
    prob, dr, B, S = _system(with_P, K)
    DR, AX, PX = _own_columns(prob, with_P, K)
    nm = N + M
    w = _init(amd, prob, dr, with_P)

    def valid():
        return [_multi(amd, w, B, S, TOL), _multi_r(amd, w, DR, B, S, TOL), _multi_v(amd, w, DR, B, S, TOL), _multi_v(amd, w, None, B, S, TOL)]

    def unchanged(what):
        for (XY, it), (XY0, it0), name in zip(valid(), before, ("multi", "multi_r", "multi_v with DR", "multi_v")):
            assert np.array_equal(_bits(XY), _bits(XY0)) and np.array_equal(it, it0), f"{name} after {what}"

    try:
        _set_values(amd, w, AX, PX)
        before = valid()
        Bf, Df, Sf, tv = np.asfortranarray(B), np.asfortranarray(DR), np.asfortranarray(S), np.full(K, TOL)
        it = np.zeros(K, dtype=T.np_int)
        fp, ip = (lambda a: a.ctypes.data_as(T.fp)), it.ctypes.data_as(T.ip)
        raw = {
            "multi": lambda lddr, ldb, lds: amd.scs_amd_solve_lin_sys_multi(w, K, fp(Bf), ldb, fp(Sf), lds, fp(tv), ip),
            "multi_r": lambda lddr, ldb, lds: amd.scs_amd_solve_lin_sys_multi_r(w, K, fp(Df), lddr, fp(Bf), ldb, fp(Sf), lds, fp(tv), ip),
            "multi_v": lambda lddr, ldb, lds: amd.scs_amd_solve_lin_sys_multi_v(w, K, fp(Df), lddr, fp(Bf), ldb, fp(Sf), lds, fp(tv), ip),
        }
        # a leading dimension shorter than its column
        for name, call in raw.items():
            for lds_ in ((nm, nm - 1, N), (nm, nm, N - 1)) + (((nm - 1, nm, N),) if name != "multi" else ()):
                assert call(*lds_) == -1
                assert np.array_equal(Bf, B), "a refused call touched B"
                unchanged(f"{name} with leading dimensions {lds_}")
        # a diag_r that is not positive (the helpers assert that B, S and DR come back unchanged)
        for bad, where in ((0.0, (0, 0)), (-1.0, (nm - 1, K - 1)), (np.nan, (N, 1))):
            D2 = DR.copy()
            D2[where] = bad
            _multi_r(amd, w, D2, B, S, TOL, expect=-1)
            unchanged(f"multi_r with diag_r {bad}")
            _multi_v(amd, w, D2, B, S, TOL, expect=-1)
            unchanged(f"multi_v with diag_r {bad}")
        # another nrhs than the set call's
        _multi_v(amd, w, DR[:, :2], B[:, :2], S[:, :2], TOL, expect=-1)
        unchanged("multi_v with another nrhs than the set call's")
        # no values set: the two entries that need none answer as before, and so does multi_v once the same values are set again
        amd.scs_amd_linsys_free_values_multi(w)
        _multi_v(amd, w, DR, B, S, TOL, expect=-1)
        for (XY, it2), (XY0, it0) in zip((_multi(amd, w, B, S, TOL), _multi_r(amd, w, DR, B, S, TOL)), before[:2]):
            assert np.array_equal(_bits(XY), _bits(XY0)) and np.array_equal(it2, it0), "after multi_v without values"
        _set_values(amd, w, AX, PX)
        unchanged("multi_v without values, then the same values set again")
    finally:
        amd.scs_free_lin_sys_work(w)
