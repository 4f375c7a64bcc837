"""The wide instantiation of the small batch (1024 threads, one workgroup per CU; n up to 512, n + m + 1 up to 2304) against the
reference (oracle/_ref/libscsindir_ref_exactcg.so, driven column after column on one workspace) at the trajectory bar of
tests/small_batch_util.py: the same iter and status_val, ScsInfo and (x, y, s) to 1e-6.  Cases, seeds and the reference's
iteration counts: tests/small_wide_util.py.  The largest shapes of the NARROW instantiation are stated here as literals: the tests
that used to reach them read the library's limits, which now are the wide ones."""
import numpy as np
import pytest

from scs_amd import capi, problems
from scs_amd.small import SmallBatch
from tests import family_util
from tests import small_batch_util as U
from tests import small_wide_util as W

pytestmark = pytest.mark.gpu


def _ref(name="libscsindir_ref_exactcg.so"):
    from oracle import pyoracle
    if not pyoracle.ref_available(name):
        pytest.skip(f"oracle/_ref/{name} not built")
    return pyoracle.load_ref(name)


def _batch(A, P, cone, B, Cc, settings):
    data = dict(A=A, b=B[:, 0], c=Cc[:, 0])
    if P is not None:
        data["P"] = P
    return SmallBatch(data, cone, **settings)


def _iters(rs):
    return [(r["info"]["iter"], r["info"]["status_val"]) for r in rs]


_shared_cache = {}


def _shared(name):
    """the shared-values solve of a case on the default grid, computed once and left unchanged"""
    if name not in _shared_cache:
        A, P, cone, B, Cc, st = W.case(name)
        with _batch(A, P, cone, B, Cc, st) as sb:
            got = sb.solve(B, Cc)
            _shared_cache[name] = (got, sb.occupancy())
    return _shared_cache[name]


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_trajectory_parity_with_the_reference(name):
    """every case of small_wide_util: the reference's iter and status_val in every column and the 1e-6 bar.  w_m513, w_n342 and
    w_n512 stop at max_iters = 300 (status 2), the others are solved.  w_n24 (n = 24, l = 1025): the reference's iteration
    counts are in small_wide_util."""
    ref = _ref()
    got, occ = _shared(name)
    exp = W.reference_case(ref, name)
    print(name, _iters(got), _iters(exp), occ)
    if "max_iters" in W.CASES[name][7]:
        assert all(r["info"]["iter"] == 300 and r["info"]["status_val"] == 2 for r in exp)
    else:
        assert all(r["info"]["status_val"] == 1 for r in exp)
    U.assert_trajectory(got, exp, name)
    assert occ["kernel"] == "wide" and occ["block_threads"] == 1024 and occ["wg_per_cu"] == 1
    assert occ["lds_bytes"] <= 160 * 1024 - 16


@pytest.mark.parametrize("n,m", [(128, 256), (64, 959)])
def test_the_narrow_limits_against_the_single_solve(n, m):
    """the largest n and the largest n + m + 1 of the narrow instantiation, as literals, against the project's own scs_solve with
    every linear solve at 1e-12; they run the narrow kernel, two workgroups per CU"""
    amd = capi.load("libscsamd.so")
    pr = problems.random_socp(n, m, 6, seed=5)
    A, cone = pr["A"], pr["cone"]
    B, Cc = family_util.family_data(A, cone, 2, 41)
    with family_util.Work(amd, capi.Problem(A, B[:, 0], Cc[:, 0], cone), cg_tol_override=1e-12, **U.SETTINGS) as w:
        exp = w.solve_columns(B, Cc)
    with _batch(A, None, cone, B, Cc, U.SETTINGS) as sb:
        got = sb.solve(B, Cc)
        occ = sb.occupancy()
    print(n, m, _iters(got), _iters(exp), occ)
    assert occ["kernel"] == "narrow" and occ["block_threads"] == 256 and occ["wg_per_cu"] >= 2
    assert occ["lds_bytes"] == 8 * (6 * (n + m + 1) + 2 * m + 3 * n + 264)
    U.assert_trajectory(got, exp, f"narrow {n} {m}")


def test_the_largest_lds_a_workgroup_may_ask_for():
    """(n, m) = (512, 1791): n and n + m + 1 both at their limits, 19982 values = 159 856 B of LDS, the most any accepted problem
    needs.  The function attribute, the occupancy query and the launch accept it; 50 iterations against the project's own scs_solve
    with every linear solve at 1e-12."""
    amd = capi.load("libscsamd.so")
    n, m = 512, 1791
    pr = problems.random_socp(n, m, 6, seed=7)
    A, cone = pr["A"], pr["cone"]
    B, Cc = family_util.family_data(A, cone, 1, 43)
    st = dict(U.SETTINGS, max_iters=50)
    with family_util.Work(amd, capi.Problem(A, B[:, 0], Cc[:, 0], cone), cg_tol_override=1e-12, **st) as w:
        exp = w.solve_columns(B, Cc)
    with _batch(A, None, cone, B, Cc, st) as sb:
        got = sb.solve(B, Cc)
        occ = sb.occupancy()
    print(_iters(got), _iters(exp), occ)
    assert occ["lds_bytes"] == 159856 and occ["wg_per_cu"] == 1 and occ["kernel"] == "wide"
    U.assert_trajectory(got, exp, "largest lds")


def test_bits_do_not_depend_on_grid_order_neighbours_or_run():
    A, P, cone, B, Cc, st = W.case("w_n129")
    K = B.shape[1]
    assert K == 3
    B6, C6 = np.hstack([B, B]), np.hstack([Cc, Cc])
    with _batch(A, P, cone, B, Cc, st) as sb:
        sb.set_grid(2)
        two = sb.solve(B6, C6)
        c = sb.counters()
        assert (c["launches"], c["workgroups"], c["problems"]) == (1, 2, 6)
        sb.set_grid(5)
        five = sb.solve(B6, C6)
        assert sb.counters()["workgroups"] == 2 + 5
        sb.set_grid(0)
        full = sb.solve(B6, C6)
        rev = sb.solve(B6[:, ::-1], C6[:, ::-1])[::-1]
        alone = sb.solve(B[:, 1], Cc[:, 1])
        again = sb.solve(B6, C6)
    for k in range(6):
        for other in (five, full, rev, again):
            assert U.same_bits(two[k], other[k]), k
        assert U.same_bits(two[k], two[k % K]), k  # its index and its neighbours
    assert U.same_bits(two[1], alone[0])
    assert all(U.same_bits(a, b) for a, b in zip(two, _shared("w_n129")[0]))  # another object, another run


def _fresh(As, Ps, cone, B, Cc, st):
    """scs_amd_small_init on (A_p, P_p) + scs_amd_small_solve of (b_p, c_p), per problem"""
    out = []
    for p, Ap in enumerate(As):
        with _batch(Ap, None if Ps is None else Ps[p], cone, B[:, p:p + 1], Cc[:, p:p + 1], st) as sb:
            out += sb.solve(B[:, p], Cc[:, p])
    return out


_own_cache = {}


def _own(name):
    if name not in _own_cache:
        As, Ps, cone, B, Cc, st = W.derived(name)
        with _batch(As[0], None if Ps is None else Ps[0], cone, B, Cc, st) as sb:
            _own_cache[name] = (sb.solve(B, Cc, A=As, P=Ps), sb.occupancy())
    return _own_cache[name]


@pytest.mark.parametrize("name", sorted(W.DERIVED_SEEDS))
def test_own_values_against_a_fresh_batch_per_problem(name):
    """every problem its own values of A (and P, w_m513) on the case's pattern: the factor on the 1024-thread block against H
    factored on the host, a fresh object per problem"""
    As, Ps, cone, B, Cc, st = W.derived(name)
    got, occ = _own(name)
    exp = _fresh(As, Ps, cone, B, Cc, st)
    print(name, _iters(got), _iters(exp))
    assert occ["kernel"] == "wide"
    U.assert_trajectory(got, exp, name)


def test_own_values_against_the_reference():
    """w_n129 with own values against the reference with a fresh scs_init per problem"""
    ref = _ref()
    got, _ = _own("w_n129")
    exp = W.reference_derived(ref, "w_n129")
    print(_iters(got), _iters(exp))
    assert all(r["info"]["status_val"] == 1 for r in exp)
    U.assert_trajectory(got, exp, "w_n129 own")


def test_equal_values_against_the_shared_entry():
    """every problem's values are the object's own: the device factor in working precision against the host's in long double"""
    A, P, cone, B, Cc, st = W.case("w_n129")
    pr = U.problem(A, P, cone, B, Cc)
    AX = np.asfortranarray(np.repeat(pr.Ax[:, None], B.shape[1], axis=1))
    with _batch(A, P, cone, B, Cc, st) as sb:
        got = sb.solve(B, Cc, A=AX)
        again = sb.solve(B, Cc)
    shared = _shared("w_n129")[0]
    print(_iters(got), _iters(shared))
    U.assert_trajectory(got, shared, "equal values")
    assert all(U.same_bits(a, b) for a, b in zip(shared, again))  # the shared entry is not disturbed


def test_warm_start():
    ref = _ref()
    A, P, cone, B, Cc, st = W.case("w_n129")
    cold = _shared("w_n129")[0]
    warm_in = tuple(np.column_stack([r[v] for r in cold]) for v in ("x", "y", "s"))
    with _batch(A, P, cone, B, Cc, st) as sb:
        warm = sb.solve(B, Cc, warm=warm_in)
    exp = U.reference_columns(ref, A, P, cone, B, Cc, st, warm=warm_in)
    print(_iters(cold), _iters(warm), _iters(exp))
    for c, w in zip(cold, warm):
        assert w["info"]["iter"] < c["info"]["iter"]
    U.assert_trajectory(warm, exp, "warm")


def test_mixed_statuses_in_one_call():
    """the construction of small_batch_util.mixed_statuses at n = 130: infeasible, unbounded and two solved problems in one call of
    the wide kernel; statuses, iterations, certificates and their NaN patterns are the reference's.  The reference's iteration counts:
    200, 50, 975, 1375."""
    ref = _ref()
    A, cone, B, Cc = W.mixed_statuses_wide()
    exp = U.reference_columns(ref, A, None, cone, B, Cc, U.SETTINGS)
    assert [r["info"]["status_val"] for r in exp] == [-2, -1, 1, 1]
    with _batch(A, None, cone, B, Cc, U.SETTINGS) as sb:
        got = sb.solve(B, Cc)
        assert sb.occupancy()["kernel"] == "wide"
    print(_iters(got), _iters(exp))
    U.assert_trajectory(got, exp, "mixed")
    for k, (ra, rr) in enumerate(zip(got, exp)):
        for key in ("res_infeas", "res_unbdd_a", "res_unbdd_p"):
            assert U.same_num(ra["info"][key], rr["info"][key]), (k, key, ra["info"][key], rr["info"][key])
    assert np.all(np.isnan(got[0]["x"])) and np.all(np.isnan(got[0]["s"])) and np.all(np.isfinite(got[0]["y"]))
    assert np.all(np.isnan(got[1]["y"])) and np.all(np.isfinite(got[1]["x"])) and np.all(np.isfinite(got[1]["s"]))
