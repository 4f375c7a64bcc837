"""scs_amd_small_set_values / scs_amd_small_solve_values: a batch of small problems that each bring their own values of A and P
on one pattern, every problem factored and solved by one workgroup inside one kernel.  Checked against the shared-values entry of
the same object (equal values), against the reference with a fresh scs_init per problem (oracle/_ref/libscsindir_ref_exactcg.so),
and against a fresh SmallBatch per problem, at the trajectory bar of tests/small_batch_util.py: the same iter and status_val,
ScsInfo and (x, y, s) to REL = 1e-6.  Cases and seeds: tests/small_values_util.py."""
import ctypes as C

import numpy as np
import pytest

from scs_amd import problems
from scs_amd.small import SmallBatch
from tests import family_util
from tests import small_batch_util as U
from tests import small_values_util as V

pytestmark = pytest.mark.gpu

DERIVED = ["a_zl", "b_odd_q", "c_qp", "c_qp_nonorm"]


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


def _fresh(As, Ps, cone, B, Cc, st, warm=None):
    """scs_amd_small_init on (A_p, P_p) + scs_amd_small_solve of (b_p, c_p), per problem"""
    out = []
    for p, Ap in enumerate(As):
        with _batch(Ap, None if Ps is None else Ps[p], cone, B[:, p:p + 1], Cc[:, p:p + 1], st) as sb:
            out += sb.solve(B[:, p], Cc[:, p], warm=None if warm is None else tuple(v[:, p] for v in warm))
    return out


_own_cache = {}


def _own(name):
    """the values solve of a derived case, computed once and left unchanged"""
    if name not in _own_cache:
        As, Ps, cone, B, Cc, st = V.derived(name)
        with _batch(As[0], None if Ps is None else Ps[0], cone, B, Cc, st) as sb:
            _own_cache[name] = sb.solve(B, Cc, A=As, P=Ps)
    return _own_cache[name]


def _iters(rs):
    return [(r["info"]["iter"], r["info"]["status_val"]) for r in rs]


@pytest.mark.parametrize("name", ["a_zl", "b_odd_q", "c_qp", "c_qp_nonorm", "d_wave", "ill_cond"])
def test_equal_values_against_the_shared_entry(name):
    """Every problem's values are the object's own: the values entry (H factored on the device in working precision) against the
    shared solve of the same object (H factored on the host in long double).  `ill_cond` (cond(H) about 1 / rho_x = 1e6) is the
    test of the device factor's precision."""
    A, P, cone, B, Cc, st = U.case(name)
    AX, PX = V.tiled(name)
    with _batch(A, P, cone, B, Cc, st) as sb:
        shared = sb.solve(B, Cc)
        got = sb.solve(B, Cc, A=AX, P=PX)
        again = sb.solve(B, Cc)
    print(name, _iters(got), _iters(shared))
    assert all(r["info"]["status_val"] == 1 for r in shared)
    U.assert_trajectory(got, shared, name)
    assert all(U.same_bits(a, b) for a, b in zip(shared, again))  # the shared entry is not disturbed


@pytest.mark.parametrize("name", DERIVED)
def test_own_values_against_the_reference(name):
    """every problem takes the reference's iter and status_val and meets the bar, the reference built fresh per problem"""
    ref = _ref()
    exp = V.reference_case(ref, name)
    got = _own(name)
    print(name, _iters(got), _iters(exp))
    assert all(r["info"]["status_val"] == 1 for r in exp)
    U.assert_trajectory(got, exp, name)


@pytest.mark.parametrize("name", DERIVED)
def test_own_values_against_a_fresh_batch_per_problem(name):
    As, Ps, cone, B, Cc, st = V.derived(name)
    exp = _fresh(As, Ps, cone, B, Cc, st)
    got = _own(name)
    print(name, _iters(got), _iters(exp))
    U.assert_trajectory(got, exp, name)


def test_bits_do_not_depend_on_grid_order_neighbours_or_run():
    As, Ps, cone, B, Cc, st = V.derived("c_qp")
    K = len(As)
    with _batch(As[0], Ps[0], cone, B, Cc, st) as sb:
        sb.set_values(As, Ps)
        sb.set_grid(2)
        two = sb.solve(B, Cc, own_values=True)
        c = sb.counters()
        assert (c["launches"], c["workgroups"], c["problems"]) == (1, 2, K)
        sb.set_grid(5)
        five = sb.solve(B, Cc, own_values=True)
        sb.set_grid(0)
        full = sb.solve(B, Cc, own_values=True)
        again = sb.solve(B, Cc, own_values=True)
        rev = sb.solve(B[:, ::-1], Cc[:, ::-1], A=As[::-1], P=Ps[::-1])[::-1]
        alone = sb.solve(B[:, 3], Cc[:, 3], A=[As[3]], P=[Ps[3]])
        assert len(alone) == 1
        for k in range(K):
            for other in (five, full, again, rev):
                assert U.same_bits(two[k], other[k]), k
        assert U.same_bits(two[3], alone[0])
    assert all(U.same_bits(a, b) for a, b in zip(two, _own("c_qp")))  # another object, another run


def test_one_indefinite_problem_fails_alone():
    """P_p = -5 I (on the pattern: the other entries explicit zeros) in one problem of five: the device factor's pivot test finds
    it; it alone is SCS_FAILED and NaN-filled, the call returns, and the others have the bits of the call without it"""
    As, Ps, cone, B, Cc, st = V.derived("c_qp")
    K, bad = len(As), 2
    with _batch(As[0], Ps[0], cone, B, Cc, st) as sb:
        pr = sb._prob
        PX = np.column_stack([pr.values_of(P, "P") for P in Ps])
        cols = np.repeat(np.arange(pr.n), np.diff(pr.Pp))
        PX[:, bad] = np.where(pr.Pi == cols, -5.0, 0.0)
        assert np.count_nonzero(PX[:, bad]) == pr.n
        got = sb.solve(B, Cc, A=As, P=PX)
    good = _own("c_qp")
    print(_iters(got))
    for k in range(K):
        if k == bad:
            assert got[k]["info"]["status_val"] == -4 and got[k]["info"]["iter"] == -1 and got[k]["info"]["status"] == "failure"
            assert all(np.all(np.isnan(got[k][v])) for v in ("x", "y", "s"))
        else:
            assert got[k]["info"]["status_val"] == 1 and U.same_bits(got[k], good[k]), k


def _check_against_fresh(A, P, cone, st, K, seed, what):
    As, Ps, B, Cc = V.derive(A, P, cone, K, seed)
    with _batch(As[0], None if Ps is None else Ps[0], cone, B, Cc, st) as sb:
        got = sb.solve(B, Cc, A=As, P=Ps)
    exp = _fresh(As, Ps, cone, B, Cc, st)
    print(what, _iters(got), _iters(exp))
    U.assert_trajectory(got, exp, what)


@pytest.mark.parametrize("cone,n,m", [(dict(l=1), 1, 1), (dict(z=0, l=6, q=[4]), 4, 10), (dict(z=4, l=0, q=[3, 3]), 5, 10),
                                      (dict(q=[12]), 5, 12)])
def test_edge_cones(cone, n, m):
    """n = m = 1; no zero cone; no nonnegative cone; only one second-order cone of size m"""
    A = U._dense_cone_prob(n, m, cone, 21, density=0.7)
    _check_against_fresh(A, None, cone, U.SETTINGS, 2, 51, str(cone))


@pytest.mark.parametrize("n", [2, 63, 64, 65])
def test_the_factor_thread_mapping(n):
    """n around the wave size: the factor's column pass, its trailing update and its inverse map threads to (row, column) by n"""
    m = 2 * n
    cone = dict(z=n // 2, l=m - n // 2)
    A = U._dense_cone_prob(n, m, cone, 22, density=0.3)
    _check_against_fresh(A, U.psd_P(n, 122), cone, U.SETTINGS, 2, 52, f"n={n}")


@pytest.mark.parametrize("which", ["n", "l"])
def test_the_limits(which):
    """the largest n (a full slab) and the largest n + m + 1, 2 problems each, against a fresh SmallBatch per problem"""
    from scs_amd import small
    nmax, lmax = small.limits()
    n, m = (nmax, 2 * nmax) if which == "n" else (nmax // 2, lmax - 1 - nmax // 2)
    pr = problems.random_socp(n, m, 6, seed=5)
    _check_against_fresh(pr["A"], None, pr["cone"], U.SETTINGS, 2, 53, which)


def test_life_cycle():
    """set once and solve two lists; a second set replaces the first; free, then a refused solve; a solve with another nprob than
    the set call's is refused; the shared solve returns the bits it returned at the start"""
    As, Ps, cone, B, Cc, st = V.derived("b_odd_q")
    K = len(As)
    B2, Cc2 = np.asfortranarray(B[:, ::-1]), np.asfortranarray(Cc[:, ::-1])
    with _batch(As[0], None, cone, B, Cc, st) as sb:
        shared0 = sb.solve(B, Cc)
        sb.set_values(As)
        one = sb.solve(B, Cc, own_values=True)
        two = sb.solve(B2, Cc2, own_values=True)
        assert all(U.same_bits(a, b) for a, b in zip(one, _own("b_odd_q")))
        U.assert_trajectory(two, _fresh(As, None, cone, B2, Cc2, st), "second list")
        with pytest.raises(ValueError, match="were set for 7"):
            sb.solve(B[:, :3], Cc[:, :3], own_values=True)
        X = np.zeros((sb.n, 3), order="F")
        Y, S = np.zeros((sb.m, 3), order="F"), np.zeros((sb.m, 3), order="F")
        T = sb._T
        sols, infos = (T.ScsSolution * 3)(), (T.ScsInfo * 3)()
        for k in range(3):
            sols[k].x, sols[k].y, sols[k].s = (C.cast(a.ctypes.data + 8 * k * a.shape[0], T.fp) for a in (X, Y, S))
        rc = sb._lib.scs_amd_small_solve_values(sb._h, 3, B.ctypes.data_as(T.fp), sb.m, Cc.ctypes.data_as(T.fp), sb.n, sols, infos, 0)
        assert rc == -4 and b"set for 7" in sb._lib.scs_amd_small_refusal()
        # with values set: the per-problem refusals of the C entry, the outputs untouched
        Xk, Yk, Sk = np.full((sb.n, K), 7.0, order="F"), np.full((sb.m, K), 8.0, order="F"), np.full((sb.m, K), 9.0, order="F")
        solk, infk = (T.ScsSolution * K)(), (T.ScsInfo * K)()
        for k in range(K):
            solk[k].x, solk[k].y, solk[k].s = (C.cast(a.ctypes.data + 8 * k * a.shape[0], T.fp) for a in (Xk, Yk, Sk))
            infk[k].iter = 1234
        Bn, Cn = B.copy(order="F"), Cc.copy(order="F")

        def refused(*words):
            rc = sb._lib.scs_amd_small_solve_values(sb._h, K, Bn.ctypes.data_as(T.fp), sb.m, Cn.ctypes.data_as(T.fp), sb.n, solk, infk, 0)
            why = sb._lib.scs_amd_small_refusal()
            assert rc == -4 and why and all(w in why.decode() for w in words), (words, why)
            assert np.all(Xk == 7.0) and np.all(Yk == 8.0) and np.all(Sk == 9.0) and all(infk[k].iter == 1234 for k in range(K))
        solk[1].y = None
        refused("sols[1]", "NULL")
        solk[1].y = C.cast(Yk.ctypes.data + 8 * sb.m, T.fp)
        Bn[0, 2] = np.nan
        refused("non-finite", "problem 2")
        Bn[0, 2] = B[0, 2]
        Cn[1, 4] = np.inf
        refused("non-finite", "problem 4")
        Cn[1, 4] = Cc[1, 4]
        assert sb._lib.scs_amd_small_solve_values(sb._h, K, Bn.ctypes.data_as(T.fp), sb.m, Cn.ctypes.data_as(T.fp), sb.n, solk, infk, 0) == 0
        assert all(np.array_equal(Xk[:, k], one[k]["x"]) and infk[k].iter == one[k]["info"]["iter"] for k in range(K))
        sb.set_values(As[::-1])  # replaces the first
        three = sb.solve(B2, Cc2, own_values=True)[::-1]
        assert all(U.same_bits(a, b) for a, b in zip(one, three))
        sb.free_values()
        with pytest.raises(ValueError, match="no values are set"):
            sb.solve(B, Cc, own_values=True)
        shared1 = sb.solve(B, Cc)
        assert all(U.same_bits(a, b) for a, b in zip(shared0, shared1))
        sb.set_values(As)  # and usable again
        assert all(U.same_bits(a, b) for a, b in zip(one, sb.solve(B, Cc, own_values=True)))


def test_warm_start():
    As, Ps, cone, B, Cc, st = V.derived("c_qp")
    cold = _own("c_qp")
    warm_in = tuple(np.column_stack([r[v] for r in cold]) for v in ("x", "y", "s"))
    with _batch(As[0], Ps[0], cone, B, Cc, st) as sb:
        warm = sb.solve(B, Cc, warm=warm_in, A=As, P=Ps)
    exp = _fresh(As, Ps, cone, B, Cc, st, warm=warm_in)
    print(_iters(cold), _iters(warm), _iters(exp))
    for c, w in zip(cold, warm):
        assert w["info"]["iter"] <= c["info"]["iter"]
    U.assert_trajectory(warm, exp, "warm")
