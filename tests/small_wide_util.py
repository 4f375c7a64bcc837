"""Helpers of the wide small-batch tests (tests/test_small_wide_cpu.py, tests/test_small_wide_gpu.py): the cases at which the
thread mappings of the 1024-thread instantiation change, the families of (b, c) on them and the reference side, computed once per
case and shared.  The generators, the reference driver and the bar are those of tests/small_batch_util.py.

Why these shapes: n = 129 is the first wide n and l = 1025 the first wide n + m + 1; m = 513 is the first m at which a product
over the rows of A gives every output to one thread (cols > 1024 / 2); at n = 342 an output of the dense products goes from three
threads to two (1024 // 341 = 3, 1024 // 342 = 2); n = 512 is the limit; q = [1100] is a second-order cone longer than the block.

The cases whose reference is slow on the CPU (w_m513, w_n342, w_n512) run K = 2 problems for max_iters = 300: the unfinished
status and the iterate after 300 iterations meet the same bar.  The others run to convergence.  The seeds are chosen so that the
reference alone is stable on every case: its serial and its OpenMP build agree on iter and status_val in every column
(tests/test_small_wide_cpu.py::test_the_reference_alone_is_stable_on_the_seeds).  A seed that does not pass is replaced, never a
bar widened.  The reference's iteration counts:
  w_n129      2050, 1350, 2400
  w_m513      300, 300 (stopped; 775, 800 to convergence)
  w_n342      300, 300 (stopped; 1525, 1175 to convergence)
  w_l1025     50, 50, 50
  w_q1100     1975, 2725, 1400
  w_n512      300, 300 (stopped; 1225, 1100 to convergence)
  w_n24       275, 350, 175
and with a fresh scs_init per problem on derived('w_n129'): 1400, 2250."""
import functools

import numpy as np

from tests import family_util
from tests import small_batch_util as U
from tests import small_values_util as V

STOP = dict(max_iters=300)

# name -> (n, m, cone, seed of A, seed of P or None, density, K, settings over small_batch_util.SETTINGS)
CASES = {
    "w_n129": (129, 300, dict(z=40, l=160, q=[3, 17, 80]), 31, None, 0.08, 3, {}),
    "w_m513": (200, 513, dict(z=60, l=253, q=[200]), 32, 132, 0.05, 2, STOP),
    "w_n342": (342, 700, dict(z=100, l=400, q=[2, 70, 128]), 33, None, 0.03, 2, STOP),
    "w_l1025": (8, 1016, dict(z=3, l=513, q=[500]), 34, None, 0.5, 3, {}),
    "w_q1100": (60, 1300, dict(z=20, l=180, q=[1100]), 35, None, 0.1, 3, {}),
    "w_n512": (512, 1100, dict(z=150, l=600, q=[50, 300]), 36, None, 0.02, 2, STOP),
    # l = 1025 again, with an iteration long enough to show more than the mapping
    "w_n24": (24, 1000, dict(z=10, l=490, q=[4, 96, 400]), 37, None, 0.1, 3, {}),
}
DERIVED_SEEDS = {"w_n129": 131, "w_m513": 132}  # small_values_util.derive on the case, K = 2


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, P or None, cone, B, Cc, settings) of a case"""
    n, m, cone, seed, pseed, density, K, over = CASES[name]
    assert cone.get("z", 0) + cone.get("l", 0) + sum(cone.get("q", [])) == m
    A = U._dense_cone_prob(n, m, cone, seed, density)
    P = U.psd_P(n, pseed) if pseed is not None else None
    B, Cc = family_util.family_data(A, cone, K, seed + 10)
    return A, P, cone, B, Cc, dict(U.SETTINGS, **over)


@functools.lru_cache(maxsize=None)
def derived(name):
    """(As, Ps or None, cone, B, Cc, settings): two problems with their own values on the pattern of the case"""
    A, P, cone, _, _, st = case(name)
    As, Ps, B, Cc = V.derive(A, P, cone, 2, DERIVED_SEEDS[name])
    return As, Ps, cone, B, Cc, st


_ref_cache = {}


def reference_case(lib, name):
    """small_batch_util.reference_columns of a case, computed once and left unchanged"""
    if name not in _ref_cache:
        _ref_cache[name] = U.reference_columns(lib, *case(name))
    return _ref_cache[name]


def reference_derived(lib, name):
    """a fresh scs_init of the reference per problem of derived(name), computed once"""
    key = ("derived", name)
    if key not in _ref_cache:
        _ref_cache[key] = V.fresh_columns(lib, *derived(name))
    return _ref_cache[key]


def agree(a, b):
    return all(x["info"]["iter"] == y["info"]["iter"] and x["info"]["status_val"] == y["info"]["status_val"] for x, y in zip(a, b))


def mixed_statuses_wide(seed=1):
    """The construction of small_batch_util.mixed_statuses at a wide n: n = 130, m = 280, z = 30, l = 150, q = [60, 40]; the first
    two nonnegative rows read x0 + s = b and -x0 + s = b', the last column of A is zero.  Column 0 infeasible, column 1 unbounded,
    columns 2 and 3 solvable.  Returns A, cone, B, Cc."""
    import scipy.sparse as sp
    from scs_amd import problems
    rng = np.random.default_rng(seed)
    cone = dict(z=30, l=150, q=[60, 40])
    n, m = 130, 280
    A = rng.uniform(-1, 1, (m, n)) * (rng.uniform(0, 1, (m, n)) < 0.08)
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
    cols = [solvable() for _ in range(2)]
    b_inf = rng.standard_normal(m)
    b_inf[l0] = b_inf[l0 + 1] = -1.0
    c_inf = rng.standard_normal(n)
    c_inf[n - 1] = 0.0
    c_unb = np.abs(rng.standard_normal(n))
    c_unb[n - 1] = -1.0
    bs = [b_inf, cols[0][0], cols[0][0], cols[1][0]]
    cs = [c_inf, c_unb, cols[0][1], cols[1][1]]
    return A, cone, np.asfortranarray(np.column_stack(bs)), np.asfortranarray(np.column_stack(cs))
