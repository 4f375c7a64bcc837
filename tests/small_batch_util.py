"""Helpers of the small-batch tests (tests/test_small_batch_gpu.py): the cases, the families of (b, c) on them, the reference side
(one workspace of a reference build driven problem after problem, computed once per case and shared) and the trajectory bar."""
import functools

import numpy as np
import scipy.sparse as sp

from scs_amd import capi, problems
from tests import family_util

REL = 1e-6
SETTINGS = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)


def _dense_cone_prob(n, m, cone, seed, density=0.5):
    """A (m x n) with about `density` of its entries U[-1, 1] and a full diagonal band so that no column is empty"""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (m, n)) * (rng.uniform(0, 1, (m, n)) < density)
    for j in range(n):
        A[(j * m) // n, j] = 1.0 + rng.uniform(0, 1)
    return sp.csc_matrix(A)


def psd_P(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n)) * (rng.uniform(0, 1, (n, n)) < 0.4)
    return sp.csc_matrix(G @ G.T + 0.1 * np.eye(n))


# name -> (n, m, cone, seed of A, P?, settings, K, seed of the family)
CASES = {
    "a_zl": (10, 25, dict(z=5, l=20), 1, False, {}, 6, 11),
    "b_odd_q": (17, 41, dict(z=6, l=15, q=[1, 2, 3, 5, 9]), 2, False, {}, 7, 12),
    "c_qp": (12, 30, dict(z=4, l=14, q=[5, 7]), 3, True, {}, 5, 13),
    "c_qp_nonorm": (12, 30, dict(z=4, l=14, q=[5, 7]), 3, True, dict(normalize=0), 5, 13),
    "d_wave": (65, 130, dict(z=13, l=39, q=[3, 10, 25, 40]), 4, False, {}, 5, 14),
    "ill_cond": (17, 41, dict(z=6, l=15, q=[1, 2, 3, 5, 9]), 2, False, {}, 6, 15),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, P or None, cone, B, Cc, settings) of a case; `ill_cond` is b_odd_q with columns 1 and 3 of A copies of columns 0 and 2"""
    n, m, cone, seed, has_P, over, K, fseed = CASES[name]
    A = _dense_cone_prob(n, m, cone, seed)
    if name == "ill_cond":
        A = A.toarray()
        A[:, 1] = A[:, 0]
        A[:, 3] = A[:, 2]
        A = sp.csc_matrix(A)
    P = psd_P(n, seed + 100) if has_P else None
    B, Cc = family_util.family_data(A, cone, K, fseed)
    return A, P, cone, B, Cc, dict(SETTINGS, **over)


def problem(A, P, cone, B, Cc, T=capi.T64):
    return capi.Problem(A, B[:, 0], Cc[:, 0], cone, P=P, T=T)


def reference_columns(lib, A, P, cone, B, Cc, settings, warm=None):
    """one workspace of `lib`, scs_update + scs_solve per column: list of dicts(x, y, s, info)"""
    with family_util.Work(lib, problem(A, P, cone, B, Cc, T=lib._scs_types), **settings) as w:
        return w.solve_columns(B, Cc, warm=warm)


_ref_cache = {}


def reference_case(lib, name):
    """reference_columns of a case, computed once"""
    if name not in _ref_cache:
        _ref_cache[name] = reference_columns(lib, *case(name))
    return _ref_cache[name]


def rel(a, b, floor=1e-3):
    return abs(a - b) / max(abs(a), abs(b), floor)


def same_num(a, b, tol=REL, floor=1e-3):
    """both NaN, both the same infinity, or within tol relative"""
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    if np.isinf(a) or np.isinf(b):
        return a == b
    return rel(a, b, floor) <= tol


def assert_trajectory(got, ref, what=""):
    """the bar of tests/test_solve_gpu.py::test_exact_cg_trajectory_parity, per problem"""
    assert len(got) == len(ref)
    for k, (ra, rr) in enumerate(zip(got, ref)):
        ia, ir = ra["info"], rr["info"]
        assert ia["status_val"] == ir["status_val"], (what, k, ia["status_val"], ir["status_val"])
        assert ia["iter"] == ir["iter"], (what, k, ia["iter"], ir["iter"])
        assert ia["scale_updates"] == ir["scale_updates"] == 0
        for key in ("pobj", "dobj", "res_pri", "res_dual", "gap"):
            assert same_num(ia[key], ir[key]), (what, k, key, ia[key], ir[key])
        for v in ("x", "y", "s"):
            a, r = ra[v], rr[v]
            assert np.array_equal(np.isnan(a), np.isnan(r)), (what, k, v)
            if not np.all(np.isnan(r)):
                d = np.nanmax(np.abs(a - r)) / max(1.0, np.nanmax(np.abs(r)))
                assert d <= REL, (what, k, v, d)


def same_bits(a, b):
    return all(np.array_equal(a[v], b[v], equal_nan=True) for v in ("x", "y", "s")) and all(
        (a["info"][k] == b["info"][k]) or (np.isnan(a["info"][k]) and np.isnan(b["info"][k]))
        for k in ("iter", "status_val", "pobj", "dobj", "res_pri", "res_dual", "gap", "res_infeas", "res_unbdd_a", "res_unbdd_p"))


def mixed_statuses(seed=0):
    """One A (z = 3, l = 8, q = [4, 3]; n = 8, m = 18) whose first two nonnegative rows read x0 + s = b, -x0 + s = b' and whose last
    column is zero.  Column 0: both rows' b = -1, infeasible.  Column 1: c[n - 1] = -1 on the zero column, unbounded.  Columns 2, 3:
    solvable by the generator's law (the two rows' b = 2, x0 = 0.5, zero multipliers there, c[n - 1] = 0).  Column 4: column 2 with b
    scaled by 1e3 -- solvable, but it needs many more iterations than the others, so a small max_iters stops it alone.
    Returns A, cone, B, Cc."""
    rng = np.random.default_rng(seed)
    cone = dict(z=3, l=8, q=[4, 3])
    n, m = 8, 18
    A = rng.uniform(-1, 1, (m, n)) * (rng.uniform(0, 1, (m, n)) < 0.6)
    for j in range(n):
        A[2 * j, j] = 1.5
    l0 = cone["z"]
    A[l0, :] = 0
    A[l0, 0] = 1.0
    A[l0 + 1, :] = 0
    A[l0 + 1, 0] = -1.0
    A[:, n - 1] = 0
    A = sp.csc_matrix(A)

    def solvable():
        z = rng.uniform(-1, 1, m)
        x = rng.uniform(-1, 1, n)
        x[0] = 0.5
        z[l0], z[l0 + 1] = -(2.0 - x[0]), -(2.0 + x[0])
        y = problems.proj_dual_cone_np(z, cone)
        return A @ x + (y - z), -(A.T @ y)
    cols = [solvable() for _ in range(3)]
    b_inf = rng.standard_normal(m)
    b_inf[l0] = b_inf[l0 + 1] = -1.0
    c_inf = rng.standard_normal(n)
    c_inf[n - 1] = 0.0
    c_unb = np.abs(rng.standard_normal(n))
    c_unb[n - 1] = -1.0
    bs = [b_inf, cols[0][0], cols[1][0], cols[2][0], cols[1][0] * 1e3]
    cs = [c_inf, c_unb, cols[1][1], cols[2][1], cols[1][1]]
    return A, cone, np.asfortranarray(np.column_stack(bs)), np.asfortranarray(np.column_stack(cs))
