"""scs_amd_solve_family (include/scs_amd.h): K problems that share A, P and the cones, solved in one device-resident ADMM loop.

Every column must be what scs_update + scs_solve computes for that problem alone:
 * against the reference build with exact linear solves on both sides (libscsindir_ref_exactcg.so driven column after column on ONE
   reference workspace; ours via scs_amd_set_cg_tol_override): equal status and iteration count, ScsInfo and (x, y, s) to 1e-6
   relative -- the bar and the floor of tests/test_solve_gpu.py::test_exact_cg_trajectory_parity;
 * against the project's own single solve where no reference is needed.
The families are built by the generator's law on the shared A (tests/family_util.py).  With adaptive_scale = 0 such a column needs
900 .. 4000 iterations at the default scale; scaling b up shortens that (still feasible and bounded: the cone is a cone).

How far b may be scaled where the 1e-6 bar applies: normalize_b_c divides b and c by max(|b|, |c|), so b scaled by f leaves the c part of
the normalised problem f times smaller, while both sides stop their linear solves at the ABSOLUTE residual 1e-12: the objectives of two
correct implementations then differ by about f x 1e-11 relative, and the gap -- a difference of the two objectives of about 1e-4 of
their size -- by 1e4 times that.  Measured on this A against the exact-CG reference, 20 columns: f = 10 gives gap differences of
1e-7 .. 3e-6 for the family AND for the project's own single solve (which meets the bar on unscaled data, tests/test_solve_gpu.py);
f = 3 gives at most 3e-7 for both.  So the parity families use f = 3 and cap the run at 500 iterations (a column takes 350 .. 1500
there): columns that converge freeze at 350, 375 and 450, the others end unfinished at the cap, and status, iteration count and every
figure are compared in both cases.  Families that are only compared with the project's own solves use f = 10 (125 .. 500 iterations).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, problems, verify
from tests.family_util import Work, family_data

pytestmark = pytest.mark.gpu
REL = 1e-6
SCS_FAILED = -4
KW = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)


def _ref(name="libscsindir_ref_exactcg.so"):
    from oracle import pyoracle
    if not pyoracle.ref_available(name):
        pytest.skip(f"oracle/_ref/{name} not built")
    return pyoracle.load_ref(name)


def _rel(a, b, floor=1e-3):
    return abs(a - b) / max(abs(a), abs(b), floor)


def _assert_same_as_reference(fam, ref_cols, rel=REL):
    for k, (ra, rr) in enumerate(zip(fam, ref_cols)):
        ia, ir = ra["info"], rr["info"]
        print(f"column {k}: status {ia['status_val']} / {ir['status_val']}, iter {ia['iter']} / {ir['iter']}, "
              + ", ".join(f"{key} {_rel(ia[key], ir[key]):.1e}" for key in ("pobj", "dobj", "res_pri", "res_dual", "gap")))
        assert ia["status_val"] == ir["status_val"], (k, ia["status"], ir["status"])
        assert ia["iter"] == ir["iter"], (k, ia["iter"], ir["iter"])
        for key in ("pobj", "dobj", "res_pri", "res_dual", "gap"):
            assert _rel(ia[key], ir[key]) <= rel, (k, key, ia[key], ir[key])
        for v in ("x", "y", "s"):
            d = np.abs(ra[v] - rr[v]).max() / max(1.0, np.abs(rr[v]).max())
            assert d <= rel, (k, v, d)


def _socp(n, m, col_nnz, seed, q_fixed=None):
    pr = problems.random_socp(n, m, col_nnz, seed=seed, q_fixed=q_fixed)
    return pr, capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])


@pytest.fixture(scope="module")
def base():
    """CASES[0] of tests/test_solve_gpu.py and a family of 8 on its A (b scaled by 10, see the module docstring)"""
    pr, prob = _socp(200, 600, 8, 1)
    B, Cc = family_data(pr["A"], pr["cone"], 8, seed=100, b_scale=[10.0] * 8)
    return pr, prob, B, Cc


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. trajectory parity with the reference, exact CG
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 8])
def test_exact_cg_trajectory_parity_with_the_reference(base, K):
    """K = 3: width 4 with a padding column.  K = 8: the reference's counts are 500, 500, 450, 500, 375, 350, 500, 500 -- three columns
    freeze at different checks while the others run on to the cap."""
    ref, amd = _ref(), capi.load("libscsamd.so")
    pr, prob, _, _ = base
    B, Cc = family_data(pr["A"], pr["cone"], 8, seed=100, b_scale=[3.0] * 8)
    B, Cc = B[:, :K], Cc[:, :K]
    kw = dict(KW, max_iters=500)
    with Work(ref, prob, **kw) as wr:
        fr = wr.solve_columns(B, Cc)
    if K == 8:  # the freeze path: columns must stop at different checks
        assert len({r["info"]["iter"] for r in fr}) >= 3, [r["info"]["iter"] for r in fr]
        assert sum(r["info"]["status_val"] == 1 for r in fr) >= 3
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as wa:
        rc, fa = wa.family(B, Cc)
    assert rc == 0
    assert all(r["info"]["status_val"] in (1, 2) for r in fr)
    _assert_same_as_reference(fa, fr)


@pytest.mark.parametrize("shape,over,b_scale", [((200, 600, 8, 1, None), dict(normalize=0), 30.0),
                                                 ((500, 1500, 6, 3, 5), dict(max_iters=200), 3.0)])  # many tiny cones
def test_exact_cg_trajectory_parity_unnormalised_and_with_many_tiny_cones(shape, over, b_scale):
    """K = 3 (width 4 with a padding column).  normalize = 0: nothing rescales c against b, so b may be scaled further (the reference
    takes 175, 550 and 200 iterations).  Many tiny cones: 200 iterations of the trajectory (a column needs thousands there)."""
    ref, amd = _ref(), capi.load("libscsamd.so")
    n, m, col_nnz, seed, q_fixed = shape
    pr, prob = _socp(n, m, col_nnz, seed, q_fixed)
    B, Cc = family_data(pr["A"], pr["cone"], 3, seed=100, b_scale=[b_scale] * 3)
    kw = dict(KW)
    kw.update(over)
    with Work(ref, prob, **kw) as wr:
        fr = wr.solve_columns(B, Cc)
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as wa:
        rc, fa = wa.family(B, Cc)
    assert rc == 0 and all(r["info"]["status_val"] in (1, 2) for r in fr)
    _assert_same_as_reference(fa, fr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the same bar with P
# ---------------------------------------------------------------------------------------------------------------------------------
def _qp():
    """the QP of tests/test_linsys_gpu.py::test_with_P_matches_reference (n = 300, m = 500, nonnegative cone) with K = 3 feasible
    right-hand sides b_k = A x_k + s_k, s_k >= 0, and random costs (P is positive definite: bounded)"""
    from tests import probgen
    n, m = 300, 500
    A = probgen.random_csc(m, n, 5, seed=11)
    Bm = sp.random(n, n, density=0.02, random_state=5, format="csc")
    P = (Bm @ Bm.T + sp.identity(n) * 0.1).tocsc()
    rng = np.random.default_rng(7)
    K = 3
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    for k in range(K):
        B[:, k] = A @ rng.uniform(-1, 1, n) + rng.uniform(0, 1, m)
        Cc[:, k] = rng.uniform(-1, 1, n)
    return capi.Problem(A, B[:, 0], Cc[:, 0], dict(l=m), P=P), B, Cc


def test_exact_cg_trajectory_parity_with_P():
    ref, amd = _ref(), capi.load("libscsamd.so")
    prob, B, Cc = _qp()
    with Work(ref, prob, **KW) as wr:
        fr = wr.solve_columns(B, Cc)
    with Work(amd, prob, cg_tol_override=1e-12, **KW) as wa:
        rc, fa = wa.family(B, Cc)
    assert rc == 0 and all(r["info"]["status_val"] == 1 for r in fr)
    _assert_same_as_reference(fa, fr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. mixed cones and mixed statuses in one family
# ---------------------------------------------------------------------------------------------------------------------------------
def _mixed(seed=0, n_solvable=3):
    """The A of tests/test_fuzz_parity_gpu.py::_base_problem (z, l, two SOCs, a PSD block of order 3) with its two contradictory
    nonnegative rows (x0 + s = b, -x0 + s = b') and its last column zeroed.  Column 0: both rows -1, infeasible.  Column 1:
    c[n - 1] = -1, unbounded.  Further columns: solvable -- the two rows' b are +2 (so |x0| <= 2), the rest is the generator's law
    with x0 = 0.5 and zero multipliers on the two rows, and c[n - 1] = 0 because the last column of A is zero."""
    from tests.test_fuzz_parity_gpu import _base_problem
    rng, cone, m, n, A = _base_problem(seed)
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
    assert all(abs(b[l0] - 2.0) < 1e-12 and abs(b[l0 + 1] - 2.0) < 1e-12 for b in bs[1:]) and all(abs(c[n - 1]) < 1e-12 for c in cs[2:])
    B, Cc = np.asfortranarray(np.column_stack(bs)), np.asfortranarray(np.column_stack(cs))
    return capi.Problem(A, B[:, 2], Cc[:, 2], cone), A, cone, B, Cc


def _check_certificates(ref, A, cone, B, Cc, fam):
    from tests.test_fuzz_parity_gpu import _ref_proj_dual
    y = fam[0]["y"]                      # infeasible: A'y ~ 0, b'y < 0, y in K*
    assert float(B[:, 0] @ y) < 0
    y = y / -float(B[:, 0] @ y)
    assert np.abs(A.T @ y).max() <= 1e-5
    assert np.abs(_ref_proj_dual(ref, cone, y) - y).max() <= 1e-6 * max(1.0, np.abs(y).max())
    x, s = fam[1]["x"], fam[1]["s"]      # unbounded: Ax + s ~ 0, s in K, c'x < 0
    cx = float(Cc[:, 1] @ x)
    assert cx < 0
    x, s = x / -cx, s / -cx
    assert np.abs(A @ x + s).max() <= 1e-5
    assert np.abs(_ref_proj_dual(ref, cone, -s)).max() <= 1e-6 * max(1.0, np.abs(s).max())


@pytest.mark.parametrize("renumber", [False, True])
def test_mixed_statuses_in_one_family(renumber, monkeypatch):
    """default CG schedule; renumber: the same through scs_init's internal numbering, forced"""
    if renumber:
        monkeypatch.setenv("SCS_AMD_REORDER", "1")
    ref, amd = _ref("libscsindir_ref.so"), capi.load("libscsamd.so")
    prob, A, cone, B, Cc = _mixed()
    kw = dict(eps_abs=1e-7, eps_rel=1e-7, max_iters=20000, **KW)
    with Work(ref, prob, **kw) as wr:
        fr = wr.solve_columns(B, Cc)
    with Work(amd, prob, **kw) as wa:
        rc, fa = wa.family(B, Cc)
    assert rc == 0
    print([(a["info"]["status_val"], a["info"]["iter"], r["info"]["iter"]) for a, r in zip(fa, fr)])
    assert [r["info"]["status_val"] for r in fr] == [-2, -1, 1, 1, 1]
    assert [r["info"]["status_val"] for r in fa] == [-2, -1, 1, 1, 1]
    assert np.all(np.isnan(fa[0]["x"])) and np.all(np.isnan(fa[0]["s"])) and np.all(np.isnan(fa[1]["y"]))
    _check_certificates(ref, A, cone, B, Cc, fa)
    for k in (2, 3, 4):
        ia, ir = fa[k]["info"], fr[k]["info"]
        scale = max(1.0, abs(ir["pobj"]))
        assert abs(ia["pobj"] - ir["pobj"]) <= 2e-5 * scale, (k, ia["pobj"], ir["pobj"])
        assert abs(ia["pobj"] - ia["dobj"]) <= 2e-5 * scale


def test_box_and_a_psd_block_of_order_73_from_the_loop():
    """a box cone (column after column on the column's Newton start) and a PSD block of order 73 (the three-matrix LDS form with its
    per-(column, block) scratch) driven from the family loop: 30 iterations, exact CG, every column against the project's own
    scs_update + scs_solve capped at 30 iterations, to 1e-9 relative (the reduction trees differ: not bit for bit)"""
    amd = capi.load("libscsamd.so")
    nb = 40
    cone = dict(l=30, bu=np.ones(nb), bl=-np.ones(nb), bsize=nb + 1, q=[], s=[73])
    m = capi.cone_rows(cone)
    pr = problems.random_cone_prob(300, m, 6, cone, seed=9)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    B, Cc = family_data(pr["A"], pr["cone"], 3, seed=5)
    with Work(amd, prob, cg_tol_override=1e-12, max_iters=30, **KW) as w:
        single = w.solve_columns(B, Cc)
        rc, fam = w.family(B, Cc)
    assert rc == 0
    for k, (a, b) in enumerate(zip(fam, single)):
        assert a["info"]["iter"] == b["info"]["iter"] == 30 and a["info"]["status_val"] == b["info"]["status_val"]
        for v in ("x", "y", "s"):
            d = np.abs(a[v] - b[v]).max() / max(1.0, np.abs(b[v]).max())
            print(f"column {k} {v}: {d:.2e}")
            assert d <= 1e-9, (k, v, d)
        for key in ("pobj", "dobj", "res_pri", "res_dual", "gap"):
            assert _rel(a["info"][key], b["info"][key]) <= 1e-9, (k, key)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. against the project's own single solve, default schedule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_schedule_same_optimum_as_the_single_solve(base):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = base
    B, Cc = B[:, :5], Cc[:, :5]
    with Work(amd, prob, **KW) as w:
        single = w.solve_columns(B, Cc)
        rc, fam = w.family(B, Cc)
    assert rc == 0
    A = prob.sparse()
    for k, (a, b) in enumerate(zip(fam, single)):
        ia, ib = a["info"], b["info"]
        assert ia["status_val"] == ib["status_val"] == 1
        assert 0.5 <= ia["iter"] / ib["iter"] <= 2.0, (k, ia["iter"], ib["iter"])
        scale = max(1.0, abs(ib["pobj"]))
        assert abs(ia["pobj"] - ib["pobj"]) <= 1e-3 * scale and abs(ia["dobj"] - ib["dobj"]) <= 1e-3 * scale
        chk = verify.verify_solved(A, B[:, k], Cc[:, k], pr["cone"], a["x"], a["y"], a["s"], ia)
        assert chk["ok"], (k, chk["failed"], chk["values"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. independence and determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a["info"]["iter"] == b["info"]["iter"] and a["info"]["status_val"] == b["info"]["status_val"] and all(
        np.array_equal(a[v], b[v], equal_nan=True) for v in ("x", "y", "s"))


@pytest.mark.parametrize("W", [4, 16])
def test_a_column_does_not_depend_on_its_neighbours_or_its_position(W):
    amd = capi.load("libscsamd.so")
    ns = max(2 * W, 12)
    prob, A, cone, B, Cc = _mixed(seed=1, n_solvable=ns)
    inf, P = 0, list(range(2, 2 + ns))  # P[j]: solvable problem j; column `inf` is infeasible
    first = P[:W]
    second = [P[3], P[9], P[0], P[1]] + (P[W:2 * W - 4] if W > 4 else [])
    third = [inf if j == P[1] else j for j in first]
    assert len(second) == W and set(first) & set(second) >= {P[0], P[1], P[3]}
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iters=1000, **KW)  # some columns end unfinished: their bits are compared too
    with Work(amd, prob, **kw) as w:
        runs = {}
        for name, cols in (("first", first), ("second", second), ("third", third), ("again", first)):
            rc, out = w.family(np.asfortranarray(B[:, cols]), np.asfortranarray(Cc[:, cols]))
            assert rc == 0
            runs[name] = dict(zip(cols, out))
    assert len({r["info"]["iter"] for r in runs["first"].values()}) > 1  # columns freeze at different checks
    for j in first:
        assert _same_bits(runs["first"][j], runs["again"][j]), j  # two identical calls
        if j in runs["second"]:
            assert _same_bits(runs["first"][j], runs["second"][j]), j  # other neighbours, another position
        if j in runs["third"]:
            assert _same_bits(runs["first"][j], runs["third"][j]), j  # an infeasible neighbour
    assert runs["third"][inf]["info"]["status_val"] == -2


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the workspace's own solve is untouched
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_psd", [False, True])
def test_the_single_solve_returns_the_same_bits_after_a_family_call(base, with_psd):
    amd = capi.load("libscsamd.so")
    if with_psd:
        prob, A, cone, B, Cc = _mixed()
        B, Cc = B[:, 2:], Cc[:, 2:]
    else:
        pr, prob, B, Cc = base
        B, Cc = B[:, :3], Cc[:, :3]
    with Work(amd, prob, max_iters=300, **KW) as w:
        before = w.solve()
        rc, _ = w.family(B, Cc)
        assert rc == 0
        after = w.solve()
    assert before["info"]["iter"] > 25 and _same_bits(before, after)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. chunks and edges
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    pr, prob = _socp(60, 150, 5, 3)
    B, Cc = family_data(pr["A"], pr["cone"], 17, seed=8, b_scale=[10.0] * 17)
    return pr, prob, B, Cc


def _close(a, b, rel):
    if a["info"]["iter"] != b["info"]["iter"] or a["info"]["status_val"] != b["info"]["status_val"]:
        return False
    return all(np.abs(a[v] - b[v]).max() <= rel * max(1.0, np.abs(b[v]).max()) for v in ("x", "y", "s"))


def test_seventeen_problems_are_two_chunks_and_one_problem_works(small):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    with Work(amd, prob, cg_tol_override=1e-12, max_iters=2000, **KW) as w:
        rc, all17 = w.family(B, Cc)
        assert rc == 0
        pairs = {}
        for k in range(0, 17, 2):
            cols = [k, (k + 1) % 17]
            rc, out = w.family(np.asfortranarray(B[:, cols]), np.asfortranarray(Cc[:, cols]))
            assert rc == 0
            pairs[cols[0]] = out[0]
            pairs.setdefault(cols[1], out[1])
        rc, one = w.family(B[:, 5:6], Cc[:, 5:6])
        assert rc == 0
    assert all(r["info"]["status_val"] == 1 for r in all17)
    for k in range(17):
        assert _close(all17[k], pairs[k], 1e-9), k
    assert _close(one[0], pairs[5], 1e-9)


def test_leading_dimensions_larger_than_m_and_n_are_honoured(small):
    amd = capi.load("libscsamd.so")
    T = amd._scs_types
    pr, prob, B, Cc = small
    K, m, n = 3, prob.m, prob.n
    ldb, ldc = m + 7, n + 3
    Bp, Cp = np.full((ldb, K), np.nan, order="F"), np.full((ldc, K), np.nan, order="F")
    Bp[:m], Cp[:n] = B[:, :K], Cc[:, :K]
    X, Y, S = np.zeros((n, K), order="F"), np.zeros((m, K), order="F"), np.zeros((m, K), order="F")
    sols, infos = (T.ScsSolution * K)(), (T.ScsInfo * K)()
    for k in range(K):
        sols[k].x, sols[k].y, sols[k].s = (C.cast(a.ctypes.data + k * a.shape[0] * 8, T.fp) for a in (X, Y, S))
    with Work(amd, prob, max_iters=2000, **KW) as w:
        assert amd.scs_amd_solve_family(w.w, K, Bp.ctypes.data_as(T.fp), ldb, Cp.ctypes.data_as(T.fp), ldc, sols, infos, 0) == 0
        rc, want = w.family(B[:, :K], Cc[:, :K])
    for k in range(K):
        assert infos[k].status_val == 1 and infos[k].iter == want[k]["info"]["iter"]
        assert np.array_equal(X[:, k], want[k]["x"]) and np.array_equal(Y[:, k], want[k]["y"]) and np.array_equal(S[:, k], want[k]["s"])


def test_warm_start_from_a_family_solution(small):
    ref, amd = _ref(), capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    B, Cc = B[:, :4], Cc[:, :4]
    with Work(amd, prob, cg_tol_override=1e-12, max_iters=2000, **KW) as w:
        rc, cold = w.family(B, Cc)
        warm0 = tuple(np.column_stack([r[v] for r in cold]) for v in ("x", "y", "s"))
        rc2, warm = w.family(B, Cc, warm=warm0)
    assert rc == 0 and rc2 == 0
    with Work(ref, prob, max_iters=2000, **KW) as wr:
        rcold = wr.solve_columns(B, Cc)
        rwarm = wr.solve_columns(B, Cc, warm=tuple(np.column_stack([r[v] for r in rcold]) for v in ("x", "y", "s")))
    for k in range(4):
        assert cold[k]["info"]["iter"] == rcold[k]["info"]["iter"]
        assert warm[k]["info"]["iter"] < cold[k]["info"]["iter"], (k, warm[k]["info"]["iter"], cold[k]["info"]["iter"])
        assert warm[k]["info"]["iter"] == rwarm[k]["info"]["iter"], (k, warm[k]["info"]["iter"], rwarm[k]["info"]["iter"])
        assert warm[k]["info"]["status_val"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,word", [(dict(adaptive_scale=1), b"adaptive_scale"), (dict(acceleration_lookback=10), b"acceleration_lookback"),
                                       (dict(log_csv_filename=True), b"log_csv_filename")])
def test_refused_settings_return_scs_failed_and_leave_the_outputs_alone(small, over, word, tmp_path):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    if "log_csv_filename" in over:
        over = dict(log_csv_filename=str(tmp_path / "log.csv").encode())
    kw = dict(KW, max_iters=50)
    kw.update(over)
    marks = tuple(np.full((r, 2), 7.0, order="F") for r in (prob.n, prob.m, prob.m))
    with Work(amd, prob, **kw) as w:
        assert word in amd.scs_amd_solve_family_refusal(w.w)
        rc, out = w.family(B[:, :2], Cc[:, :2], warm=marks, warm_start=0)
        assert rc == SCS_FAILED
        assert all(np.all(r[v] == 7.0) for r in out for v in ("x", "y", "s")) and all(r["info"]["iter"] == 0 for r in out)
        assert w.solve()["info"]["iter"] > 0  # a following scs_solve works


def test_bad_counts_and_leading_dimensions_are_refused(small):
    amd = capi.load("libscsamd.so")
    T = amd._scs_types
    pr, prob, B, Cc = small
    X = np.full((prob.n + 2 * prob.m, 2), 7.0, order="F")
    sols, infos = (T.ScsSolution * 2)(), (T.ScsInfo * 2)()
    for k in range(2):
        base = X.ctypes.data + k * X.shape[0] * 8
        sols[k].x, sols[k].y, sols[k].s = (C.cast(base + o * 8, T.fp) for o in (0, prob.n, prob.n + prob.m))
    bp, cp = B.ctypes.data_as(T.fp), Cc.ctypes.data_as(T.fp)
    with Work(amd, prob, max_iters=50, **KW) as w:
        assert amd.scs_amd_solve_family_refusal(w.w) is None
        assert amd.scs_amd_solve_family(w.w, 0, bp, prob.m, cp, prob.n, sols, infos, 0) == SCS_FAILED
        assert amd.scs_amd_solve_family(w.w, 2, bp, prob.m - 1, cp, prob.n, sols, infos, 0) == SCS_FAILED
        assert amd.scs_amd_solve_family(w.w, 2, bp, prob.m, cp, prob.n - 1, sols, infos, 0) == SCS_FAILED
        assert np.all(X == 7.0)
        assert w.solve()["info"]["iter"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the failure convention (scs_amd_test_fail_at: the simulated-failure hook of tests/test_fault_injection_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_hip_failure_inside_a_family_solve_fails_every_column_and_the_workspace_recovers():
    amd = capi.load("libscsamd.so")
    pr, prob = _socp(20000, 40000, 8, 5)
    B, Cc = family_data(pr["A"], pr["cone"], 16, seed=3)

    def free_bytes():
        v = amd.scs_amd_device_free_bytes()
        assert v >= 0
        return v
    with Work(amd, prob, max_iters=30, **KW) as w:  # warm: context, streams, code objects
        assert w.family(B[:, :2], Cc[:, :2])[0] == 0
    base = free_bytes()
    w = Work(amd, prob, max_iters=30, **KW)
    rc, good = w.family(B[:, :3], Cc[:, :3])  # width 4 first: the state grows to width 16 below
    assert rc == 0
    assert w.family(B, Cc)[0] == 0  # grows the state to width 16: the calls below allocate nothing
    big = 10 ** 12
    amd.scs_amd_test_fail_at(big)
    assert w.family(B, Cc)[0] == 0
    total = big - amd.scs_amd_test_fail_at(0)  # checked HIP calls of one such family solve
    assert total > 100
    held = base - free_bytes()
    assert held > 4 * (prob.n + prob.m) * 16 * 8 * 0.9  # the four iterate blocks alone
    for k in (3, total // 3, total - 4):  # in the set-up of the chunk, early and late in the loop
        amd.scs_amd_test_fail_at(k)
        rc, out = w.family(B, Cc)
        assert amd.scs_amd_test_fail_at(0) == 0, k  # consumed inside the call
        assert rc == SCS_FAILED
        for r in out:
            assert r["info"]["status_val"] == SCS_FAILED and r["info"]["iter"] == -1 and r["info"]["status"] == "failure"
            assert all(np.all(np.isnan(r[v])) for v in ("x", "y", "s"))
        rc, again = w.family(B[:, :3], Cc[:, :3])
        assert rc == 0 and all(_same_bits(a, b) for a, b in zip(again, good)), k
    w.close()
    assert abs(free_bytes() - base) <= 8 << 20


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the other builds
# ---------------------------------------------------------------------------------------------------------------------------------
def test_f32_family_against_its_own_single_solves(base):
    """the loose fp32 bounds of tests/test_scale_parity_gpu.py: eps = 1e-3, same status, objectives within 1e-2 of their scale"""
    lib = capi.load("libscsamd_f32.so")
    pr, _, B, Cc = base
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=lib._scs_types)
    B, Cc = B[:, :4], Cc[:, :4]
    with Work(lib, prob, eps_abs=1e-3, eps_rel=1e-3, **KW) as w:
        single = w.solve_columns(B, Cc)
        rc, fam = w.family(B, Cc)
    assert rc == 0
    for k, (a, b) in enumerate(zip(fam, single)):
        assert a["x"].dtype == np.float32
        assert a["info"]["status_val"] == b["info"]["status_val"] == 1, k
        sc = max(1.0, abs(b["info"]["pobj"]))
        assert abs(a["info"]["pobj"] - b["info"]["pobj"]) <= 1e-2 * sc and abs(a["info"]["dobj"] - b["info"]["dobj"]) <= 1e-2 * sc, k


def test_dlong_family_equals_the_32_bit_library(base):
    """64-bit scs_int at the ABI: the same family, bit for bit, as libscsamd.so, and close to the library's own single solves"""
    l32, l64 = capi.load("libscsamd.so"), capi.load("libscsamd_dlong.so")
    pr, prob32, B, Cc = base
    B, Cc = B[:, :4], Cc[:, :4]
    prob64 = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=l64._scs_types)
    with Work(l64, prob64, cg_tol_override=1e-12, **KW) as w:
        rc, f64 = w.family(B, Cc)
        single = w.solve_columns(B, Cc)
    with Work(l32, prob32, cg_tol_override=1e-12, **KW) as w:
        rc2, f32 = w.family(B, Cc)
    assert rc == 0 and rc2 == 0
    for k in range(4):
        assert _same_bits(f64[k], f32[k]), k
        assert _close(f64[k], single[k], 1e-6), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. the Python object
# ---------------------------------------------------------------------------------------------------------------------------------
def test_python_solve_family(base):
    from scs_amd.solver import SCS
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = base
    B, Cc = B[:, :3], Cc[:, :3]
    data = dict(A=pr["A"], b=pr["b"], c=pr["c"])
    with Work(amd, prob, **KW) as w:
        rc, want = w.family(B, Cc)
    with SCS(data, pr["cone"], adaptive_scale=0, acceleration_lookback=0) as s:
        got = s.solve_family(B, Cc)
        got_lists = s.solve_family([B[:, k] for k in range(3)], [Cc[:, k] for k in range(3)])
        warm = s.solve_family(B, Cc, warm_start=True, **{v: np.column_stack([r[v] for r in got]) for v in ("x", "y", "s")})
        with pytest.raises(ValueError):
            s.solve_family(B, Cc[:, :2])
    assert len(got) == 3
    for k in range(3):
        assert set(got[k]) == {"x", "y", "s", "info"} and got[k]["info"]["status"] == "solved"
        assert _same_bits(got[k], want[k]) and _same_bits(got_lists[k], want[k])
        assert warm[k]["info"]["iter"] < got[k]["info"]["iter"]
    for over, word in ((dict(acceleration_lookback=0), "adaptive_scale"), (dict(adaptive_scale=0), "acceleration_lookback")):
        with SCS(data, pr["cone"], **over) as s:
            with pytest.raises(ValueError, match=word):
                s.solve_family(B, Cc)
