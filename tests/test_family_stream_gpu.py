"""scs_amd_solve_family_stream (include/scs_amd.h): a queue of problems through the slots of one block, a finished column's slot
going to the next problem of the queue.

The yardstick is exact: within one width the bits of a column of scs_amd_solve_family / scs_amd_solve_family_scaled depend neither
on its neighbours nor on its position (tests/test_family_gpu.py), so a problem that passes through a stream must come out with the
bits those entries give it in any call of that width that contains it.  Three rules throughout: the expected bits of problem p at
width W come from a call of the existing entry at that width; iteration counts used to plan or replay a schedule are the existing
entry's, never the stream's; and where a test needs several distinct iteration counts, the per-problem factors on b are from
{3, 10, 30} (tests/test_family_gpu.py's docstring: scaling b changes the iteration count and nothing else about the problem)."""
import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, problems
from tests.family_util import Work, family_data
from tests.test_family_gpu import _assert_same_as_reference, _qp, _ref, _same_bits, _socp
from tests.test_family_scaled_gpu import ADAPT, _assert_same_as, _fresh_columns, _same_bits_and_info

pytestmark = pytest.mark.gpu
SCS_FAILED = -4
KW = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)
INTERVAL = 25  # CONVERGED_INTERVAL


def stream(w, B, Cc, width=0, **kw):
    return capi.solve_family_stream(w.lib, w.w, B, Cc, width=width, **kw)


def counters(w):
    return capi.family_stream_counters(w.lib, w.w)


def _same(a, b):
    """the promise: (x, y, s), status, iter, scale, scale_updates and the residual and objective fields, bit for bit"""
    return _same_bits_and_info(a, b) and all(a["info"][k] == b["info"][k] for k in ("scale", "scale_updates"))


def _expected(B, Cc, W, call):
    """every problem's result from calls of the existing entry at width W: consecutive groups of W problems, the last wrapping round
    (width 2: pairs; width 4: groups of four; 17 problems at width 16: two calls of 16).  call(cols) -> (rc, results)"""
    n = B.shape[1]
    assert n >= W
    out = [None] * n
    for g0 in range(0, n, W):
        cols = [(g0 + t) % n for t in range(W)]
        rc, res = call(cols)
        assert rc == 0
        for c, r in zip(cols, res):
            if out[c] is None:
                out[c] = r
    return out


def _shared(w, B, Cc, **kw):
    return lambda cols: w.family(np.asfortranarray(B[:, cols]), np.asfortranarray(Cc[:, cols]), **kw)


def replay(iters, W, max_iters):
    """The schedule of include/scs_amd.h from the existing entry's iteration counts: a problem with iter = j < max_iters converged
    at its local iteration j and ran j + 1 iterations, one with iter = max_iters ran max_iters.  Returns the counters [0] .. [3]."""
    n, K = len(iters), min(W, len(iters))
    ran = [it + 1 if it < max_iters else max_iters for it in iters]
    slots = {k: ran[k] - 1 for k in range(K)}  # slot -> the global iteration at whose bottom its column ends
    nxt, refills, last = K, 0, 0
    while slots:
        i = last = min(slots.values())
        free = sorted(k for k, e in slots.items() if e == i)
        for k in free:
            del slots[k]
        for k in free:  # the lowest free slot takes the next problem, which starts at the next multiple of 25
            if nxt < n:
                slots[k] = (i // INTERVAL + 1) * INTERVAL + ran[nxt] - 1
                nxt, refills = nxt + 1, refills + 1
    return [last + 1, sum(ran), (last + 1) * W - sum(ran), refills]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. - 3., 13.: seventeen problems of the 60 x 150 shape
# ---------------------------------------------------------------------------------------------------------------------------------
# The 17 problems: the family of seed 8, problem k with its b scaled by FACTORS17[k]; problem 9 of that draw does not reach 1e-6
# within 2000 iterations at any of the three factors, so its place is taken by problem 0's data under another factor than problem 0's.
# scs_amd_solve_family's counts for them at width 2 / 4 / 16 (measured): 475, 275 / 200 / 275, 1050 / 1100 / 1200, 250 / 250 / 275,
# 275 / 225 / 225, 675 / 625 / 650, 375, 225 / 225 / 250, 375, 475 / 500 / 500, 275 / 275 / 300, 325, 200 / 200 / 175,
# 325 / 300 / 325, 325, 525 / 500 / 525, 325 / 275 / 250 -- all solved.
SOURCE17 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 10, 11, 12, 13, 14, 15, 16]
FACTORS17 = [3.0, 10.0, 30.0, 3.0, 10.0, 10.0, 3.0, 10.0, 30.0, 30.0, 10.0, 30.0, 3.0, 10.0, 30.0, 30.0, 10.0]
KW17 = dict(KW, eps_abs=1e-6, eps_rel=1e-6, max_iters=2000)


@pytest.fixture(scope="module")
def small():
    pr, prob = _socp(60, 150, 5, 3)
    B, Cc = family_data(pr["A"], pr["cone"], 17, seed=8)
    B, Cc = np.asfortranarray(B[:, SOURCE17] * np.array(FACTORS17)), np.asfortranarray(Cc[:, SOURCE17])
    return pr, prob, B, Cc


@pytest.fixture(scope="module")
def want17(small):
    """the 17 problems from scs_amd_solve_family at widths 2, 4 and 16, default CG schedule"""
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    with Work(amd, prob, **KW17) as w:
        out = {W: _expected(B, Cc, W, _shared(w, B, Cc)) for W in (2, 4, 16)}
    for W, res in out.items():
        print(W, [r["info"]["iter"] for r in res])
    return out


@pytest.mark.parametrize("W", [2, 4, 16])
def test_bits_through_refills_and_the_schedule_replayed(small, want17, W):
    """Every one of the 17 problems has the bits of scs_amd_solve_family at that width, and the counters are the schedule replayed
    from the existing entry's iteration counts (the counts: the comment at FACTORS17)."""
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    want = want17[W]
    iters = [r["info"]["iter"] for r in want]
    assert len(set(iters)) >= 3, iters
    assert all(r["info"]["status_val"] == 1 for r in want)
    with Work(amd, prob, **KW17) as w:
        rc, got = stream(w, B, Cc, width=W)
        cnt = counters(w)
    assert rc == 0
    print(cnt)
    for p in range(17):
        assert _same(got[p], want[p]), (p, got[p]["info"]["iter"], want[p]["info"]["iter"])
    assert cnt["refills"] == 17 - W and cnt["width"] == W
    assert [cnt[k] for k in ("block_iters", "run_slot_iters", "idle_slot_iters", "refills")] == replay(iters, W, 2000)
    assert cnt["resid_evals"] >= cnt["block_iters"] // INTERVAL


def test_the_order_of_the_queue_does_not_matter(small, want17):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    want = want17[4]
    with Work(amd, prob, **KW17) as w:
        for order in (list(range(16, -1, -1)), [int(v) for v in np.random.default_rng(5).permutation(17)]):
            rc, got = stream(w, np.asfortranarray(B[:, order]), np.asfortranarray(Cc[:, order]), width=4)
            assert rc == 0
            for q, p in enumerate(order):
                assert _same(got[q], want[p]), (order, q, p)


def test_a_hip_failure_after_the_first_refill_fails_every_problem_and_the_workspace_recovers(small, want17):
    """scs_amd_test_fail_at makes one checked HIP call report an error although it succeeded (no device fault).  17 problems through
    2 slots: half way through the call's checked HIP calls several problems have been returned and their slots refilled."""
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    with Work(amd, prob, **KW17) as w:
        big = 10 ** 12
        amd.scs_amd_test_fail_at(big)
        rc, good = stream(w, B, Cc, width=2)
        total = big - amd.scs_amd_test_fail_at(0)
        assert rc == 0 and total > 1000
        amd.scs_amd_test_fail_at(total // 2)
        rc, out = stream(w, B, Cc, width=2)
        assert amd.scs_amd_test_fail_at(0) == 0  # consumed inside the call
        assert rc == SCS_FAILED
        refills = counters(w)["refills"]  # counted as the loop goes: what the failed call had done when it failed
        print("refills before the injected failure:", refills)
        assert 1 <= refills < 15  # so problems had been returned and their slots refilled: those are failed below too
        for r in out:
            assert r["info"]["status_val"] == SCS_FAILED and r["info"]["iter"] == -1 and r["info"]["status"] == "failure"
            assert all(np.all(np.isnan(r[v])) for v in ("x", "y", "s"))
        rc, again = stream(w, B, Cc, width=2)
    assert rc == 0
    for p in range(17):
        assert _same(again[p], want17[2][p]) and _same(good[p], want17[2][p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. parity with the reference through a stream
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return _socp(200, 600, 8, 1)


def test_exact_cg_trajectory_parity_with_the_reference_through_a_stream(base):
    """the family of 8 of tests/test_family_gpu.py at b x 3, capped at 500: the reference's counts are 500, 500, 450, 500, 375, 350,
    500, 500 -- columns end by converging and at the cap, and four slots are refilled"""
    ref, amd = _ref(), capi.load("libscsamd.so")
    pr, prob = base
    B, Cc = family_data(pr["A"], pr["cone"], 8, seed=100, b_scale=[3.0] * 8)
    kw = dict(KW, max_iters=500)
    with Work(ref, prob, **kw) as wr:
        fr = wr.solve_columns(B, Cc)
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as wa:
        rc, fa = stream(wa, B, Cc, width=4)
        cnt = counters(wa)
    assert rc == 0 and cnt["refills"] == 4
    _assert_same_as_reference(fa, fr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a cap that is no multiple of 25
# ---------------------------------------------------------------------------------------------------------------------------------
FACTORS7 = [3.0, 10.0, 30.0, 10.0, 3.0, 3.0, 10.0]


def test_a_cap_that_is_no_multiple_of_25(small):
    """max_iters = 110: a column that does not converge at 25, 50, 75 or 100 ends after its local iteration 109 with iter = 110 and
    the residuals of that moment; the next problem starts at the next multiple of 25.  eps = 1e-3, so that some problems converge
    under the cap: scs_amd_solve_family's counts at width 2 are 100, 110, 110, 100, 110, 100, 75 (measured)."""
    amd = capi.load("libscsamd.so")
    pr, prob, _, _ = small
    B, Cc = family_data(pr["A"], pr["cone"], 7, seed=8, b_scale=FACTORS7)
    kw = dict(KW, max_iters=110, eps_abs=1e-3, eps_rel=1e-3)
    with Work(amd, prob, **kw) as w:
        want = _expected(B, Cc, 2, _shared(w, B, Cc))
        iters = [r["info"]["iter"] for r in want]
        print(iters, [r["info"]["status_val"] for r in want])
        assert sum(it == 110 for it in iters) >= 2 and sum(r["info"]["status_val"] == 1 for r in want) >= 1
        rc, got = stream(w, B, Cc, width=2)
        cnt = counters(w)
    assert rc == 0
    for p in range(7):
        assert _same(got[p], want[p]), p
        assert got[p]["info"]["status_val"] == 1 or got[p]["info"]["iter"] == 110
    assert [cnt[k] for k in ("block_iters", "run_slot_iters", "idle_slot_iters", "refills")] == replay(iters, 2, 110)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. statuses
# ---------------------------------------------------------------------------------------------------------------------------------
def _mixed_no_psd(seed=0, n_solvable=5):
    """tests/test_family_gpu.py::_mixed on a cone without PSD blocks (z, l and two second-order cones) and an A of its own: two
    contradictory nonnegative rows (x0 + s = b, -x0 + s = b') and a zeroed last column.  Problem 0: both rows -1, infeasible.
    Problem 1: c[n - 1] = -1, unbounded.  The others: solvable."""
    rng = np.random.default_rng(7000 + seed)
    cone = dict(z=2, l=6, q=[4, 5])
    m = capi.cone_rows(cone)
    n = 6
    A = sp.random(m, n, density=0.8, random_state=seed, format="lil", data_rvs=rng.standard_normal)
    l0 = cone["z"]
    A[l0, :] = 0; A[l0, 0] = 1.0
    A[l0 + 1, :] = 0; A[l0 + 1, 0] = -1.0
    A[:, n - 1] = 0
    A = sp.csc_matrix(A)

    def solvable():
        z = rng.uniform(-1, 1, m)
        x = rng.uniform(-1, 1, n)
        x[0] = 0.5
        z[l0], z[l0 + 1] = -(2.0 - x[0]), -(2.0 + x[0])  # y = 0 and s = 2 -+ x0 on the two rows
        y = problems.proj_dual_cone_np(z, cone)
        return A @ x + (y - z), -(A.T @ y)
    cols = [solvable() for _ in range(n_solvable + 1)]
    b_inf = rng.standard_normal(m)
    b_inf[l0] = b_inf[l0 + 1] = -1.0
    c_inf = rng.standard_normal(n)
    c_inf[n - 1] = 0.0
    c_unb = np.abs(rng.standard_normal(n))
    c_unb[n - 1] = -1.0
    bs = [b_inf, cols[0][0]] + [b for b, _ in cols[1:]]
    cs = [c_inf, c_unb] + [c for _, c in cols[1:]]
    B, Cc = np.asfortranarray(np.column_stack(bs)), np.asfortranarray(np.column_stack(cs))
    return capi.Problem(A, B[:, 2], Cc[:, 2], cone), B, Cc


def test_statuses_through_a_stream():
    ref, amd = _ref("libscsindir_ref.so"), capi.load("libscsamd.so")
    prob, B, Cc = _mixed_no_psd()
    kw = dict(eps_abs=1e-7, eps_rel=1e-7, max_iters=20000, **KW)
    with Work(ref, prob, **kw) as wr:
        fr = wr.solve_columns(B, Cc)
    with Work(amd, prob, **kw) as w:
        want = _expected(B, Cc, 2, _shared(w, B, Cc))
        rc, got = stream(w, B, Cc, width=2)
    assert rc == 0
    print([(g["info"]["status_val"], g["info"]["iter"], r["info"]["iter"]) for g, r in zip(got, fr)])
    assert [r["info"]["status_val"] for r in fr] == [-2, -1, 1, 1, 1, 1, 1]
    assert [r["info"]["status_val"] for r in got] == [-2, -1, 1, 1, 1, 1, 1]
    assert np.all(np.isnan(got[0]["x"])) and np.all(np.isnan(got[0]["s"])) and np.all(np.isnan(got[1]["y"]))
    assert not np.any(np.isnan(got[0]["y"])) and not np.any(np.isnan(got[1]["x"]))
    for p in range(7):
        assert _same(got[p], want[p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. own scales
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_scale_sweep_through_a_stream_holds_the_bits_of_the_scaled_entry(base):
    """6 scales x 2 problems = 12 queue entries at width 4, capped at 1000 iterations (the far scales end there)"""
    amd = capi.load("libscsamd.so")
    pr, prob = base
    B2, C2 = family_data(pr["A"], pr["cone"], 2, seed=100, b_scale=[10.0] * 2)
    sweep = [0.01, 0.03, 0.1, 0.3, 1.0, 3.0]
    B, Cc = np.asfortranarray(np.repeat(B2, 6, axis=1)), np.asfortranarray(np.repeat(C2, 6, axis=1))
    scales = np.array(sweep * 2)
    with Work(amd, prob, max_iters=1000, **KW) as w:
        want = _expected(B, Cc, 4, lambda cols: capi.solve_family_scaled(amd, w.w, np.asfortranarray(B[:, cols]),
                                                                          np.asfortranarray(Cc[:, cols]), scales=scales[cols]))
        rc, got = stream(w, B, Cc, width=4, own_scale=True, scales=scales)
        cnt = counters(w)
    assert rc == 0 and cnt["refills"] == 8
    print([(r["info"]["iter"], r["info"]["scale"]) for r in want])
    assert len({r["info"]["iter"] for r in want}) >= 3
    for p in range(12):
        assert got[p]["info"]["scale"] == scales[p] and _same(got[p], want[p]), p


def test_adaptive_scaling_through_a_stream_against_the_reference(base):
    """the unscaled family of 8, adaptive_scale = 1, exact CG: the reference (a fresh workspace per problem) takes 325, 425, 325, 375,
    225, 275, 300, 375 iterations with 1 or 2 scale updates each; through a stream of width 4 every problem updates its scale at
    checks of its own local iteration, in a slot whose R, preconditioner and g are rebuilt for it alone"""
    amd = capi.load("libscsamd.so")
    pr, prob = base
    B, Cc = family_data(pr["A"], pr["cone"], 8, seed=100)
    fr = _fresh_columns(_ref(), prob, B, Cc, **ADAPT)
    print([(r["info"]["iter"], r["info"]["scale_updates"]) for r in fr])
    assert len({r["info"]["iter"] for r in fr}) >= 3 and all(r["info"]["scale_updates"] >= 1 for r in fr)
    with Work(amd, prob, cg_tol_override=1e-12, **ADAPT) as w:
        rc, got = stream(w, B, Cc, width=4, own_scale=True)
        want = _expected(B, Cc, 4, lambda cols: capi.solve_family_scaled(amd, w.w, np.asfortranarray(B[:, cols]),
                                                                          np.asfortranarray(Cc[:, cols])))
    assert rc == 0
    _assert_same_as(got, fr)
    for p in range(8):
        assert _same(got[p], want[p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. warm start per problem
# ---------------------------------------------------------------------------------------------------------------------------------
def test_warm_start_per_problem(small):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    B, Cc = np.asfortranarray(B[:, :6]), np.asfortranarray(Cc[:, :6])
    with Work(amd, prob, **KW17) as w:
        rc, cold = stream(w, B, Cc, width=2)
        assert rc == 0
        warm0 = tuple(np.column_stack([r[v] for r in cold]) for v in ("x", "y", "s"))
        want = _expected(B, Cc, 2, lambda cols: w.family(np.asfortranarray(B[:, cols]), np.asfortranarray(Cc[:, cols]),
                                                          warm=tuple(np.asfortranarray(v[:, cols]) for v in warm0)))
        rc, warm = stream(w, B, Cc, width=2, warm=warm0)
        # with own scales the warm start reads the refilled column's own R_y (v_y = y + s / R_y): the scaled entry's bits
        scales = np.array([0.05, 0.2, 0.1, 0.3, 0.1, 0.07])
        want_sc = _expected(B, Cc, 2, lambda cols: capi.solve_family_scaled(
            amd, w.w, np.asfortranarray(B[:, cols]), np.asfortranarray(Cc[:, cols]), scales=scales[cols],
            warm=tuple(np.asfortranarray(v[:, cols]) for v in warm0)))
        rc2, warm_sc = stream(w, B, Cc, width=2, own_scale=True, scales=scales, warm=warm0)
    assert rc == 0 and rc2 == 0
    for p in range(6):
        assert _same(warm[p], want[p]), p
        assert warm[p]["info"]["status_val"] == 1 and warm[p]["info"]["iter"] < cold[p]["info"]["iter"], p
        assert _same(warm_sc[p], want_sc[p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the box cone through a reused slot
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_box_cone_through_a_reused_slot():
    """the box cone's Newton iteration starts from the slot's last root: a refilled slot has to start at 1 again, as the slot of a
    fresh call does"""
    amd = capi.load("libscsamd.so")
    nb = 40
    cone = dict(l=30, bu=np.ones(nb), bl=-np.ones(nb), bsize=nb + 1, q=[])
    m = capi.cone_rows(cone)
    pr = problems.random_cone_prob(300, m, 6, cone, seed=9)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    B, Cc = family_data(pr["A"], pr["cone"], 5, seed=5)
    with Work(amd, prob, cg_tol_override=1e-12, max_iters=60, **KW) as w:
        want = _expected(B, Cc, 2, _shared(w, B, Cc))
        rc, got = stream(w, B, Cc, width=2)
        cnt = counters(w)
    assert rc == 0 and cnt["refills"] == 3
    for p in range(5):
        assert _same(got[p], want[p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. with P
# ---------------------------------------------------------------------------------------------------------------------------------
def test_with_P():
    amd = capi.load("libscsamd.so")
    prob, B3, C3 = _qp()
    B, Cc = np.asfortranarray(np.tile(B3, (1, 2))), np.asfortranarray(np.tile(C3, (1, 2)))
    with Work(amd, prob, **KW) as w:
        want = _expected(B, Cc, 2, _shared(w, B, Cc))
        rc, got = stream(w, B, Cc, width=2)
    assert rc == 0 and all(r["info"]["status_val"] == 1 for r in want)
    for p in range(6):
        assert _same(got[p], want[p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(amd, prob, over, word, own_scale=False, scales=None):
    B = np.ones((prob.m, 3), order="F")
    Cc = np.ones((prob.n, 3), order="F")
    marks = tuple(np.full((r, 3), 7.0, order="F") for r in (prob.n, prob.m, prob.m))
    with Work(amd, prob, **dict(dict(KW, max_iters=50), **over)) as w:
        rc, out = stream(w, B, Cc, width=2, own_scale=own_scale, scales=scales, warm=marks, warm_start=0)
        why = amd.scs_amd_solve_family_stream_refusal(w.w, 1 if own_scale else 0)
        assert rc == SCS_FAILED
        assert why is not None and word in why, why
        assert all(np.all(r[v] == 7.0) for r in out for v in ("x", "y", "s")) and all(r["info"]["iter"] == 0 for r in out)
        assert w.solve()["info"]["iter"] > 0  # a following scs_solve works


def test_refusals_leave_the_outputs_alone_and_name_the_cause(small, tmp_path):
    amd = capi.load("libscsamd.so")
    pr, prob, _, _ = small
    cone = dict(l=4, q=[3], s=[3])
    ps = problems.random_cone_prob(5, capi.cone_rows(cone), 3, cone, seed=2)
    _refused(amd, capi.Problem(ps["A"], ps["b"], ps["c"], ps["cone"]), {}, b"PSD")
    _refused(amd, capi.Problem(ps["A"], ps["b"], ps["c"], ps["cone"]), {}, b"PSD", own_scale=True)
    _refused(amd, prob, dict(acceleration_lookback=10), b"acceleration_lookback")
    _refused(amd, prob, dict(log_csv_filename=str(tmp_path / "log.csv").encode()), b"log_csv_filename")
    _refused(amd, prob, dict(adaptive_scale=1), b"adaptive_scale")
    _refused(amd, prob, {}, b"scales must be NULL", scales=[0.1, 0.1, 0.1])
    for bad in (0.0, -0.1, float("nan")):
        _refused(amd, prob, {}, b"positive", own_scale=True, scales=[0.1, bad, 0.1])
    with Work(amd, prob, max_iters=50, **KW) as w:  # an accepted call clears the argument refusal
        assert stream(w, np.ones((prob.m, 3)), np.ones((prob.n, 3)), width=2, scales=[0.1] * 3)[0] == SCS_FAILED
        assert amd.scs_amd_solve_family_stream_refusal(w.w, 0) is not None
        assert stream(w, np.ones((prob.m, 3)), np.ones((prob.n, 3)), width=2)[0] == 0
        assert amd.scs_amd_solve_family_stream_refusal(w.w, 0) is None and amd.scs_amd_solve_family_stream_refusal(w.w, 1) is None


# ---------------------------------------------------------------------------------------------------------------------------------
# 12. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_single_solve_and_the_family_entry_return_the_same_bits_after_a_stream_call(small):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    with Work(amd, prob, max_iters=300, **KW) as w:
        before = w.solve()
        rc, fam_before = w.family(B[:, :5], Cc[:, :5])
        assert rc == 0
        assert stream(w, B[:, :9], Cc[:, :9], width=4)[0] == 0
        assert stream(w, B[:, :5], Cc[:, :5], width=2, own_scale=True, scales=[0.3] * 5)[0] == 0
        after = w.solve()
        rc, fam_after = w.family(B[:, :5], Cc[:, :5])
        assert rc == 0
    assert before["info"]["iter"] > 25 and _same_bits(before, after)
    assert all(_same(a, b) for a, b in zip(fam_before, fam_after))


# ---------------------------------------------------------------------------------------------------------------------------------
# 14. the other builds
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dlong_stream_equals_the_32_bit_library(small):
    l32, l64 = capi.load("libscsamd.so"), capi.load("libscsamd_dlong.so")
    pr, prob32, B, Cc = small
    B, Cc = B[:, :7], Cc[:, :7]
    prob64 = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=l64._scs_types)
    with Work(l64, prob64, **KW17) as w:
        rc, f64 = stream(w, B, Cc, width=2)
    with Work(l32, prob32, **KW17) as w:
        rc2, f32 = stream(w, B, Cc, width=2)
    assert rc == 0 and rc2 == 0
    for p in range(7):
        assert _same(f64[p], f32[p]), p


def test_f32_stream_equals_its_own_family_entry(small):
    lib = capi.load("libscsamd_f32.so")
    pr, _, B, Cc = small
    B, Cc = np.asfortranarray(B[:, :5]), np.asfortranarray(Cc[:, :5])
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=lib._scs_types)
    with Work(lib, prob, eps_abs=1e-3, eps_rel=1e-3, max_iters=1000, **KW) as w:  # fp32 stalls above 1e-3 on some of them: capped
        want = _expected(B, Cc, 2, _shared(w, B, Cc))
        rc, got = stream(w, B, Cc, width=2)
    assert rc == 0
    for p in range(5):
        assert got[p]["x"].dtype == np.float32 and _same(got[p], want[p]), p


# ---------------------------------------------------------------------------------------------------------------------------------
# 15. the Python object
# ---------------------------------------------------------------------------------------------------------------------------------
def test_python_solve_family_stream(small):
    from scs_amd.solver import SCS
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    B, Cc = np.asfortranarray(B[:, :9]), np.asfortranarray(Cc[:, :9])
    scales = np.array([0.03, 0.1, 0.3] * 3)
    kw = dict(KW, max_iters=500)
    with Work(amd, prob, **kw) as w:
        rc, want = stream(w, B, Cc, width=4)
        rc2, want_scaled = stream(w, B, Cc, width=4, own_scale=True, scales=scales)
    assert rc == 0 and rc2 == 0
    data = dict(A=pr["A"], b=pr["b"], c=pr["c"])
    with SCS(data, pr["cone"], adaptive_scale=0, acceleration_lookback=0, max_iters=500) as s:
        got = s.solve_family(B, Cc, stream=True, width=4)
        got_scaled = s.solve_family(B, Cc, stream=True, width=4, scale=scales)
        with pytest.raises(ValueError, match="width"):
            s.solve_family(B, Cc, stream=True, width=3)
        # a call the library refuses for its arguments raises ValueError with the library's message and does not stay with the
        # object: the calls after it are served, with the same bits
        for bad in ([0.1, -1.0, 0.1] * 3, [0.1, 0.0, float("nan")] * 3):
            with pytest.raises(ValueError, match="positive"):
                s.solve_family(B, Cc, stream=True, width=4, scale=bad)
            after = s.solve_family(B, Cc, stream=True, width=4)
            after_scaled = s.solve_family(B, Cc, stream=True, width=4, own_scale=True)
            assert all(_same(a, b) for a, b in zip(after, got)) and len(after_scaled) == 9
    for p in range(9):
        assert _same(got[p], want[p]) and _same(got_scaled[p], want_scaled[p]), p
    cone = dict(l=4, q=[3], s=[3])
    ps = problems.random_cone_prob(5, capi.cone_rows(cone), 3, cone, seed=2)
    with SCS(dict(A=ps["A"], b=ps["b"], c=ps["c"]), ps["cone"], adaptive_scale=0, acceleration_lookback=0) as s:
        with pytest.raises(ValueError, match="PSD"):
            s.solve_family(np.column_stack([ps["b"]] * 3), np.column_stack([ps["c"]] * 3), stream=True)
