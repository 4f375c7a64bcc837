"""Helpers of the own-values small-batch tests (tests/test_small_values_gpu.py): lists of problems that share a pattern but not
the values of A and P, derived from the cases of tests/small_batch_util.py, and the reference side -- a FRESH scs_init on
(A_p, P_p) per problem, computed once per case and shared.

Problem p of `derived(name)`: A_p = A o (1 + 0.2 xi_p), xi_p uniform in [-1, 1] per entry, on the pattern of the case's A;
P_p = P + delta_p I with delta_p uniform in [0, 0.5] where the case has a P; (b_p, c_p) by the generator's law on A_p
(family_util.family_data), so every problem is feasible and bounded.

The seeds (SEEDS) are chosen so that the reference alone is stable on every problem: oracle/_ref/libscsindir_ref_exactcg.so and
its OpenMP build (another summation order), each with a fresh scs_init per problem, agree on iter and status_val
(`reference_is_stable`, checked on the CPU by tests/test_small_values_cpu.py where oracle/_ref is built).  A seed that does not
pass is replaced, never a bar widened.  The reference's iteration counts on them:
  a_zl         2900, 175, 175, 200, 50, 125
  b_odd_q      425, 1075, 1075, 950, 350, 650, 1425
  c_qp         5175, 750, 1325, 1125, 900
  c_qp_nonorm  6925, 1225, 1700, 1000, 1775"""
import functools

import numpy as np
import scipy.sparse as sp

from scs_amd import capi
from tests import family_util
from tests import small_batch_util as U

SEEDS = {"a_zl": 101, "b_odd_q": 102, "c_qp": 103, "c_qp_nonorm": 103}


def derive(A, P, cone, K, seed):
    """K problems on the pattern of (A, P): lists As, Ps (None without P), and B (m x K), Cc (n x K)"""
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    As, Ps = [], (None if P is None else [])
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    for p in range(K):
        Ap = A.copy()
        Ap.data = A.data * (1.0 + 0.2 * rng.uniform(-1, 1, A.nnz))
        As.append(Ap)
        if P is not None:
            Ps.append(sp.csc_matrix(P + rng.uniform(0, 0.5) * sp.identity(n, format="csc")))
        b, c = family_util.family_data(Ap, cone, 1, int(rng.integers(1 << 30)))
        B[:, p], Cc[:, p] = b[:, 0], c[:, 0]
    return As, Ps, B, Cc


@functools.lru_cache(maxsize=None)
def derived(name, seed=None):
    """(As, Ps or None, cone, B, Cc, settings) of the case `name` of small_batch_util, K as there"""
    A, P, cone, B0, _, st = U.case(name)
    As, Ps, B, Cc = derive(A, P, cone, B0.shape[1], SEEDS[name] if seed is None else seed)
    return As, Ps, cone, B, Cc, st


def tiled(name):
    """the case itself with every problem's values equal to the shared ones: AX, PX (None without P) as nnz x K arrays"""
    A, P, cone, B, Cc, st = U.case(name)
    pr = U.problem(A, P, cone, B, Cc)
    K = B.shape[1]
    AX = np.asfortranarray(np.repeat(pr.Ax[:, None], K, axis=1))
    PX = None if P is None else np.asfortranarray(np.repeat(pr.Px[:, None], K, axis=1))
    return AX, PX


def fresh_columns(lib, As, Ps, cone, B, Cc, settings, warm=None):
    """a fresh workspace of `lib` per problem (scs_init on (A_p, P_p), one scs_solve): list of dicts(x, y, s, info)"""
    out = []
    for p, Ap in enumerate(As):
        prob = capi.Problem(Ap, B[:, p], Cc[:, p], cone, P=None if Ps is None else Ps[p], T=lib._scs_types)
        with family_util.Work(lib, prob, **settings) as w:
            out.append(w.solve(warm=None if warm is None else tuple(v[:, p] for v in warm)))
    return out


_ref_cache = {}


def reference_case(lib, name):
    """fresh_columns of a derived case on the reference, computed once"""
    if name not in _ref_cache:
        _ref_cache[name] = fresh_columns(lib, *derived(name))
    return _ref_cache[name]


def reference_is_stable(ref, ref_omp, name, seed=None):
    """(stable, iteration counts): the two reference builds agree on iter and status_val in every problem, all solved"""
    case = derived(name, seed)
    a = reference_case(ref, name) if seed is None else fresh_columns(ref, *case)
    b = fresh_columns(ref_omp, *case)
    ok = all(x["info"]["iter"] == y["info"]["iter"] and x["info"]["status_val"] == y["info"]["status_val"] == 1 for x, y in zip(a, b))
    return ok, [x["info"]["iter"] for x in a]
