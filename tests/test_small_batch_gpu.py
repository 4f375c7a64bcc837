"""scs_amd_small_*: a batch of small problems, every problem solved by one workgroup inside one kernel, against the reference
(oracle/_ref/libscsindir_ref_exactcg.so: the unmodified sources with every linear solve at the 1e-12 floor -- the batch solves
exactly) driven problem after problem on one workspace.  Cases, seeds and the bar: tests/small_batch_util.py."""
import numpy as np
import pytest

from scs_amd import capi, problems
from scs_amd.small import SmallBatch
from tests import family_util
from tests import small_batch_util as U

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


@pytest.mark.parametrize("name", ["a_zl", "b_odd_q", "c_qp", "c_qp_nonorm", "d_wave"])
def test_trajectory_parity_with_the_reference(name):
    """Every problem: the reference's status_val and iter, scale_updates == 0, pobj / dobj / res_pri / res_dual / gap within 1e-6
    relative, x / y / s within 1e-6 of scale.  The seeds are chosen so that the reference alone is stable on them: its serial and its
    OpenMP build (another summation order) agree on iter and status in every column.  The reference's iteration counts:
      a_zl         100, 400, 725, 250, 325, 250
      b_odd_q      2925, 150, 950, 3675, 1775, 550, 1750
      c_qp         1650, 5575, 2175, 575, 10250
      c_qp_nonorm  12500, 7250, 2550, 375, 19475
      d_wave       1200, 575, 375, 625, 400"""
    ref = _ref()
    A, P, cone, B, Cc, st = U.case(name)
    with _batch(A, P, cone, B, Cc, st) as sb:
        got = sb.solve(B, Cc)
    exp = U.reference_case(ref, name)
    print(name, [r["info"]["iter"] for r in got], [r["info"]["iter"] for r in exp])
    assert all(r["info"]["status_val"] == 1 for r in exp)
    U.assert_trajectory(got, exp, name)


def test_ill_conditioned_reduced_matrix():
    """b_odd_q with two columns of A duplicated and no P: H = rho_x I + A' R_y^-1 A has two eigenvalues rho_x = 1e-6, cond(H) about
    1 / rho_x.  The bar of the test above; this is the test of how the factor of H is applied (a dense inverse plus one step of
    refinement).  The reference's iteration counts: 575, 775, 925, 425, 700, 1050."""
    ref = _ref()
    A, P, cone, B, Cc, st = U.case("ill_cond")
    Ad = A.toarray()
    assert np.array_equal(Ad[:, 1], Ad[:, 0]) and np.array_equal(Ad[:, 3], Ad[:, 2]) and P is None
    with _batch(A, P, cone, B, Cc, st) as sb:
        got = sb.solve(B, Cc)
    exp = U.reference_case(ref, "ill_cond")
    print([r["info"]["iter"] for r in got], [r["info"]["iter"] for r in exp])
    U.assert_trajectory(got, exp, "ill_cond")


def test_mixed_statuses_in_one_call():
    """infeasible, unbounded, two solved and one problem that max_iters = 400 stops (the reference needs 29275 iterations for it),
    in one call: statuses, iterations, certificates and their NaN patterns are the reference's"""
    ref = _ref()
    A, cone, B, Cc = U.mixed_statuses(1)
    st = dict(U.SETTINGS, max_iters=400)
    exp = U.reference_columns(ref, A, None, cone, B, Cc, st)
    assert [r["info"]["status_val"] for r in exp] == [-2, -1, 1, 1, 2]
    with _batch(A, None, cone, B, Cc, st) as sb:
        got = sb.solve(B, Cc)
    print([(r["info"]["iter"], r["info"]["status_val"]) for r in got])
    U.assert_trajectory(got, exp, "mixed")
    for k, (ra, rr) in enumerate(zip(got, exp)):
        for key in ("res_infeas", "res_unbdd_a", "res_unbdd_p"):
            assert U.same_num(ra["info"][key], rr["info"][key]), (k, key, ra["info"][key], rr["info"][key])
    assert np.all(np.isnan(got[0]["x"])) and np.all(np.isnan(got[0]["s"])) and np.all(np.isfinite(got[0]["y"]))
    assert np.all(np.isnan(got[1]["y"])) and np.all(np.isfinite(got[1]["x"])) and np.all(np.isfinite(got[1]["s"]))
    assert got[0]["info"]["pobj"] == np.inf and got[1]["info"]["dobj"] == -np.inf
    assert got[4]["info"]["iter"] == 400 and got[4]["info"]["status_val"] == 2
    assert got[4]["info"]["status"] == "solved (inaccurate - reached max_iters)"


def test_bits_do_not_depend_on_grid_order_neighbours_or_run():
    A, P, cone, B, Cc, st = U.case("b_odd_q")
    assert B.shape[1] == 7
    with _batch(A, P, cone, B, Cc, st) as sb:
        sb.set_grid(2)
        two = sb.solve(B, Cc)
        c = sb.counters()
        assert (c["launches"], c["workgroups"], c["problems"]) == (1, 2, 7)
        assert c["iterations"] == sum(r["info"]["iter"] for r in two)
        sb.set_grid(0)
        full = sb.solve(B, Cc)
        assert sb.counters()["workgroups"] == 2 + 7  # never more workgroups than problems
        rev = sb.solve(B[:, ::-1], Cc[:, ::-1])[::-1]
        alone = sb.solve(B[:, 3], Cc[:, 3])
        again = sb.solve(B, Cc)
        assert len(alone) == 1
        for k in range(7):
            assert U.same_bits(two[k], full[k]) and U.same_bits(two[k], rev[k]) and U.same_bits(two[k], again[k]), k
        assert U.same_bits(two[3], alone[0])
        # more problems than workgroups
        before = sb.counters()
        many = sb.solve(np.repeat(B[:, 1:2], 600, axis=1), np.repeat(Cc[:, 1:2], 600, axis=1))
        after = sb.counters()
        assert after["problems"] - before["problems"] == 600 and after["launches"] - before["launches"] == 1
        assert after["workgroups"] - before["workgroups"] < 600 or sb.occupancy()["default_grid"] >= 600
        assert all(U.same_bits(many[0], r) for r in many) and U.same_bits(many[0], two[1])
        sb.set_grid(5)
        few = sb.solve(np.repeat(B[:, 1:2], 600, axis=1), np.repeat(Cc[:, 1:2], 600, axis=1))
        assert sb.counters()["workgroups"] - after["workgroups"] == 5
        assert all(U.same_bits(many[0], r) for r in few)


def test_warm_start():
    ref = _ref()
    A, P, cone, B, Cc, st = U.case("d_wave")
    with _batch(A, P, cone, B, Cc, st) as sb:
        cold = sb.solve(B, Cc)
        warm_in = tuple(np.column_stack([r[v] for r in cold]) for v in ("x", "y", "s"))
        warm = sb.solve(B, Cc, warm=warm_in)
    exp = U.reference_columns(ref, A, P, cone, B, Cc, st, warm=warm_in)
    print([r["info"]["iter"] for r in cold], [r["info"]["iter"] for r in warm], [r["info"]["iter"] for r in exp])
    for c, w in zip(cold, warm):
        assert w["info"]["iter"] <= c["info"]["iter"]
    U.assert_trajectory(warm, exp, "warm")


@pytest.mark.parametrize("cone,n,m", [(dict(l=1), 1, 1), (dict(z=0, l=6, q=[4]), 4, 10), (dict(z=4, l=0, q=[3, 3]), 5, 10),
                                      (dict(q=[12]), 5, 12)])
def test_edge_cones(cone, n, m):
    """n = m = 1; no zero cone; no nonnegative cone; only one second-order cone of size m -- and nprob = 1"""
    ref = _ref()
    A = U._dense_cone_prob(n, m, cone, 21, density=0.7)
    B, Cc = family_util.family_data(A, cone, 1, 31)
    exp = U.reference_columns(ref, A, None, cone, B, Cc, U.SETTINGS)
    with _batch(A, None, cone, B, Cc, U.SETTINGS) as sb:
        got = sb.solve(B, Cc)
    print([(r["info"]["iter"], r["info"]["status_val"]) for r in got], [(r["info"]["iter"], r["info"]["status_val"]) for r in exp])
    U.assert_trajectory(got, exp, str(cone))


@pytest.mark.parametrize("which", ["n", "l"])
def test_the_limits_against_the_single_solve(which):
    """the largest n and the largest n + m + 1 the library serves, against the project's own scs_solve with every linear solve at
    1e-12"""
    from scs_amd import small
    amd = capi.load("libscsamd.so")
    nmax, lmax = small.limits(amd)
    n, m = (nmax, 2 * nmax) if which == "n" else (nmax // 2, lmax - 1 - nmax // 2)
    pr = problems.random_socp(n, m, 6, seed=5)
    A, cone = pr["A"], pr["cone"]
    B, Cc = family_util.family_data(A, cone, 2, 41)
    with family_util.Work(amd, capi.Problem(A, B[:, 0], Cc[:, 0], cone), cg_tol_override=1e-12, **U.SETTINGS) as w:
        exp = w.solve_columns(B, Cc)
    with _batch(A, None, cone, B, Cc, U.SETTINGS) as sb:
        got = sb.solve(B, Cc)
        assert sb.occupancy()["lds_bytes"] <= 160 * 1024
    print(which, n, m, [r["info"]["iter"] for r in got], [r["info"]["iter"] for r in exp])
    U.assert_trajectory(got, exp, which)


def test_the_object_survives_and_leaves_a_workspace_alone():
    amd = capi.load("libscsamd.so")
    A, P, cone, B, Cc, st = U.case("c_qp")
    with family_util.Work(amd, U.problem(A, P, cone, B, Cc), **st) as w:
        before = w.solve(B[:, 3], Cc[:, 3])
        with _batch(A, P, cone, B, Cc, st) as sb:
            first = sb.solve(B[:, :4], Cc[:, :4])
            second = sb.solve(B[:, 2:4], Cc[:, 2:4])
            after = w.solve(B[:, 3], Cc[:, 3])
            third = sb.solve(B[:, :4], Cc[:, :4])
    assert U.same_bits(before, after)
    assert U.same_bits(first[2], second[0]) and U.same_bits(first[3], second[1])
    assert all(U.same_bits(a, b) for a, b in zip(first, third))


def test_a_hip_failure_fails_every_problem_and_leaves_the_object_usable():
    """scs_amd_test_fail_at(k) makes the k-th checked HIP call of the library report an error (scs_amd/csrc/common.h): in the device
    side's creation by the first solve, in the staging, behind the launch and in the read-back.  Every problem of the call is
    NaN-filled with SCS_FAILED, and the next call on the same object returns the bits of an undisturbed one."""
    import ctypes as C
    amd = capi.load("libscsamd.so")
    T = amd._scs_types
    A, P, cone, B, Cc, st = U.case("a_zl")
    with _batch(A, P, cone, B, Cc, st) as sb:
        good = sb.solve(B, Cc)
    m, n, K = B.shape[0], Cc.shape[0], B.shape[1]

    def raw_solve(h):
        X, Y, S = np.zeros((n, K), order="F"), np.zeros((m, K), order="F"), np.zeros((m, K), order="F")
        sols, infos = (T.ScsSolution * K)(), (T.ScsInfo * K)()
        for k in range(K):
            sols[k].x = C.cast(X.ctypes.data + 8 * k * n, T.fp)
            sols[k].y = C.cast(Y.ctypes.data + 8 * k * m, T.fp)
            sols[k].s = C.cast(S.ctypes.data + 8 * k * m, T.fp)
        rc = amd.scs_amd_small_solve(h, K, B.ctypes.data_as(T.fp), m, Cc.ctypes.data_as(T.fp), n, sols, infos, 0)
        return rc, [dict(x=X[:, k].copy(), y=Y[:, k].copy(), s=S[:, k].copy(), info=capi.info_dict(infos[k])) for k in range(K)]

    prob = U.problem(A, P, cone, B, Cc)
    stg = capi.default_settings(amd, **st)
    big = 10 ** 12
    h = amd.scs_amd_small_init(C.byref(prob.data), C.byref(prob.k), C.byref(stg))
    assert h
    amd.scs_amd_test_fail_at(big)
    rc, out = raw_solve(h)  # the first solve: device side + one launch
    first_calls = big - amd.scs_amd_test_fail_at(0)
    assert rc == 0 and all(U.same_bits(a, b) for a, b in zip(out, good))
    amd.scs_amd_test_fail_at(big)
    raw_solve(h)
    later_calls = big - amd.scs_amd_test_fail_at(0)
    assert first_calls > later_calls >= 8
    amd.scs_amd_small_finish(h)
    for k in sorted({1, 2, first_calls // 2, first_calls - later_calls + 1, first_calls - 3, first_calls}):
        h = amd.scs_amd_small_init(C.byref(prob.data), C.byref(prob.k), C.byref(stg))  # host work only: no checked call
        amd.scs_amd_test_fail_at(k)
        rc, out = raw_solve(h)
        assert amd.scs_amd_test_fail_at(0) == 0, k  # the countdown fired
        assert rc == -4 and amd.scs_amd_small_refusal() is None, k
        for r in out:
            assert r["info"]["status_val"] == -4 and r["info"]["iter"] == -1 and r["info"]["status"] == "failure"
            assert np.all(np.isnan(r["x"])) and np.all(np.isnan(r["y"])) and np.all(np.isnan(r["s"]))
        rc, out = raw_solve(h)
        assert rc == 0 and all(U.same_bits(a, b) for a, b in zip(out, good)), k
        amd.scs_amd_small_finish(h)
