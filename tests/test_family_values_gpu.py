"""scs_amd_family_set_values / scs_amd_solve_family_values (include/scs_amd.h): a family whose problems share the pattern of A and P
and the cones, but not the values.

The yardstick is bit equality: column k must be column k of scs_amd_solve_family_scaled, at the same nprob, on a second workspace
brought to values k by scs_amd_update_matrix -- the same loop on the same blocks, with the shared values, D, E, scales and box bounds
where this entry reads the column's own.  A block that reads a shared quantity where it should read the column's cannot pass that.
One case is held against the reference with exact linear solves, at the bar of tests/test_family_gpu.py (b scaled by 3, 500 iterations).
Base problem: problems.random_socp(200, 600, 8, seed=1); column values A.data * (1 + 0.3 u_k); data by family_data on the column's A_k.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, problems
from tests.family_util import Work, family_data
from tests.test_family_gpu import _assert_same_as_reference, _ref

pytestmark = pytest.mark.gpu
SCS_FAILED = -4
FIXED = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)
TIMES = ("setup_time", "solve_time", "lin_sys_time", "cone_time", "accel_time")
NUMERIC = [k for k in capi.INFO_FIELDS if k not in TIMES]


def _equal(a, b):
    """(x, y, s) bit for bit and every field of ScsInfo that is not a clock"""
    return all(np.array_equal(a[v], b[v], equal_nan=True) for v in ("x", "y", "s")) and a["info"]["status"] == b["info"]["status"] and all(
        a["info"][key] == b["info"][key] or (np.isnan(a["info"][key]) and np.isnan(b["info"][key])) for key in NUMERIC)


def _perturbed(x, K, rng, amp=0.3):
    """x * (1 + amp u_k), u_k uniform in (-1, 1): the law of tests/test_linsys_multi_v_gpu.py"""
    return np.asfortranarray(x[:, None] * (1.0 + amp * rng.uniform(-1, 1, (len(x), K))))


def _own_data(prob, AX, cone, seed, b_scale):
    """column k of family_data on A_k: every problem is feasible and bounded on its own matrix"""
    K = AX.shape[1]
    B, Cc = np.zeros((prob.m, K), order="F"), np.zeros((prob.n, K), order="F")
    for k in range(K):
        Ak = sp.csc_matrix((AX[:, k], prob.Ai, prob.Ap), shape=(prob.m, prob.n))
        Bk, Ck = family_data(Ak, cone, K, seed=seed, b_scale=[b_scale] * K)
        B[:, k], Cc[:, k] = Bk[:, k], Ck[:, k]
    return B, Cc


def set_values(w, AX, PX=None):
    return capi.family_set_values(w.lib, w.w, AX, PX)


def values(w, B, Cc, scales=None, warm=None):
    return capi.solve_family_values(w.lib, w.w, B, Cc, scales=scales, warm=warm)


def scaled(w, B, Cc, scales=None, warm=None):
    return capi.solve_family_scaled(w.lib, w.w, B, Cc, scales=scales, warm=warm)


def _update_matrix(w, ax, px=None):
    T = w.T
    ax = np.ascontiguousarray(ax, dtype=T.np_float)
    px = None if px is None else np.ascontiguousarray(px, dtype=T.np_float)
    assert w.lib.scs_amd_update_matrix(w.w, ax.ctypes.data_as(T.fp), None if px is None else px.ctypes.data_as(T.fp)) == 0


def _on_updated_workspaces(amd, prob, AX, PX, B, Cc, kw, scales=None, warm=None, cg=None):
    """column k of scs_amd_solve_family_scaled(B, Cc) on a workspace brought to values k, for every k"""
    out = []
    for k in range(AX.shape[1]):
        with Work(amd, prob, cg_tol_override=cg, **kw) as w:
            _update_matrix(w, AX[:, k], None if PX is None else PX[:, k])
            rc, cols = scaled(w, B, Cc, scales=scales, warm=warm)
            assert rc == 0
            out.append(cols[k])
    return out


def _assert_columns_equal(got, want):
    bad = [k for k, (a, b) in enumerate(zip(got, want)) if not _equal(a, b)]
    assert bad == [], [(k, got[k]["info"], want[k]["info"]) for k in bad]


@pytest.fixture(scope="module")
def base():
    pr = problems.random_socp(200, 600, 8, seed=1)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    AX = _perturbed(prob.Ax, 8, np.random.default_rng(42))
    B, Cc = _own_data(prob, AX, pr["cone"], 100, 10.0)
    return pr, prob, AX, B, Cc


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the workspace's own values in every column: the bits of scs_amd_solve_family_scaled
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 8])
def test_own_values_in_every_column_give_the_bits_of_the_scaled_entry(base, K):
    """K = 3: width 4 with a padding column"""
    amd = capi.load("libscsamd.so")
    pr, prob, _, _, _ = base
    B, Cc = family_data(pr["A"], pr["cone"], K, seed=100, b_scale=[10.0] * K)
    AX = np.asfortranarray(np.tile(prob.Ax[:, None], (1, K)))
    with Work(amd, prob, max_iters=300, **FIXED) as w:
        rc, want = scaled(w, B, Cc)
        assert rc == 0 and set_values(w, AX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    assert all(r["info"]["iter"] > 25 for r in want)
    _assert_columns_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. column k against a workspace brought to values k by scs_amd_update_matrix, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [1, 0])
def test_socp_columns_equal_the_updated_workspaces(base, normalize):
    amd = capi.load("libscsamd.so")
    pr, prob, AX, B, Cc = base
    AX, B, Cc = AX[:, :3], B[:, :3], Cc[:, :3]
    kw = dict(FIXED, max_iters=300, normalize=normalize)
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    want = _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw)
    assert all(r["info"]["iter"] > 25 for r in want)
    _assert_columns_equal(got, want)


def test_adaptive_scale_columns_equal_the_updated_workspaces(base):
    """unscaled b: a column needs 225 .. 425 iterations with one or two scale updates (tests/test_family_scaled_gpu.py)"""
    amd = capi.load("libscsamd.so")
    pr, prob, AX, _, _ = base
    AX = AX[:, :3]
    B, Cc = _own_data(prob, AX, pr["cone"], 100, 1.0)
    kw = dict(FIXED, adaptive_scale=1, max_iters=500)
    want = _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw)
    print([(r["info"]["iter"], r["info"]["scale_updates"], r["info"]["scale"]) for r in want])
    assert any(r["info"]["scale_updates"] > 0 for r in want)
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    _assert_columns_equal(got, want)


def test_explicit_scales_and_warm_start_equal_the_updated_workspaces(base):
    amd = capi.load("libscsamd.so")
    pr, prob, AX, B, Cc = base
    AX, B, Cc = AX[:, :3], B[:, :3], Cc[:, :3]
    kw = dict(FIXED, max_iters=200)
    scales = np.array([0.03, 0.4, 5.0])
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX) == 0
        rc, got = values(w, B, Cc, scales=scales)
        assert rc == 0
        warm0 = tuple(np.column_stack([r[v] for r in got]) for v in ("x", "y", "s"))
        rc, got_warm = values(w, B, Cc, scales=scales, warm=warm0)
        assert rc == 0
    assert [r["info"]["scale"] for r in got] == list(scales)
    _assert_columns_equal(got, _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw, scales=scales))
    _assert_columns_equal(got_warm, _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw, scales=scales, warm=warm0))
    assert not any(_equal(a, b) for a, b in zip(got, got_warm))


def _qp_values(K=3):
    """the QP of tests/test_family_gpu.py::_qp with every column its own A and its own P = B_k B_k' + 0.1 I (B_k: the values of B
    perturbed, so P_k stays positive definite on one pattern)"""
    from tests import probgen
    n, m = 300, 500
    rng = np.random.default_rng(7)
    A = probgen.random_csc(m, n, 5, seed=11)
    Bm = sp.random(n, n, density=0.02, random_state=5, format="csc")
    Ps = []
    for k in range(K + 1):  # the last one: the workspace's own
        Bk = Bm.copy()
        Bk.data = Bm.data * (1.0 + 0.3 * rng.uniform(-1, 1, len(Bm.data)))
        Ps.append((Bk @ Bk.T + sp.identity(n) * 0.1).tocsc())
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), P=Ps[K])
    AX = _perturbed(prob.Ax, K, rng)
    PX = np.asfortranarray(np.column_stack([prob.values_of(P, "P") for P in Ps[:K]]))
    for k in range(K):
        Ak = sp.csc_matrix((AX[:, k], prob.Ai, prob.Ap), shape=(m, n))
        B[:, k] = Ak @ rng.uniform(-1, 1, n) + rng.uniform(0, 1, m)
        Cc[:, k] = rng.uniform(-1, 1, n)
    return prob, AX, PX, B, Cc


def test_qp_with_its_own_P_per_column_equals_the_updated_workspaces():
    amd = capi.load("libscsamd.so")
    prob, AX, PX, B, Cc = _qp_values()
    assert not np.array_equal(PX[:, 0], PX[:, 1])
    kw = dict(FIXED, max_iters=300)
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX, PX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    want = _on_updated_workspaces(amd, prob, AX, PX, B, Cc, kw)
    assert all(r["info"]["iter"] > 25 for r in want)
    _assert_columns_equal(got, want)


def _cone_problem(cone, n, seed, K=3):
    m = capi.cone_rows(cone)
    pr = problems.random_cone_prob(n, m, 6, cone, seed=seed)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    AX = _perturbed(prob.Ax, K, np.random.default_rng(seed + 1))
    B, Cc = _own_data(prob, AX, pr["cone"], 5, 1.0)
    return pr, prob, AX, B, Cc


def test_box_cone_under_every_columns_own_bounds_equals_the_updated_workspaces():
    """normalize = 1: the box cone's bounds are normalised with the D of the column's own equilibration"""
    from tests.test_equilibrate import _equilibrate
    amd = capi.load("libscsamd.so")
    nb = 12
    cone = dict(l=30, bu=np.linspace(0.5, 2.0, nb), bl=-np.linspace(1.0, 0.3, nb), bsize=nb + 1, q=[5, 9])
    pr, prob, AX, B, Cc = _cone_problem(cone, 120, 9)
    box = slice(30, 30 + nb + 1)
    D = [_equilibrate(amd, sp.csc_matrix((AX[:, k], prob.Ai, prob.Ap), shape=(prob.m, prob.n)), None, cone, 0)[2][box] for k in (0, 1)]
    assert not np.array_equal(D[0][1:] / D[0][0], D[1][1:] / D[1][0])  # two columns under different normalised bounds
    kw = dict(FIXED, max_iters=200, normalize=1)
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    want = _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw)
    assert all(r["info"]["iter"] > 25 for r in want)
    _assert_columns_equal(got, want)


def test_small_sdp_equals_the_updated_workspaces():
    amd = capi.load("libscsamd.so")
    cone = dict(l=20, q=[], s=[3, 6, 4, 5])
    pr, prob, AX, B, Cc = _cone_problem(cone, 40, 3)
    kw = dict(FIXED, max_iters=200)
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    want = _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw)
    assert all(r["info"]["iter"] > 25 for r in want)
    _assert_columns_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reference parity, exact CG: one fresh reference workspace per column, initialised on A_k
# ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_cg_trajectory_parity_with_the_reference_on_every_columns_own_matrix(base):
    """the bar and the settings of tests/test_family_gpu.py (b scaled by 3, max_iters = 500, 1e-6 relative with its floor); K = 3"""
    ref, amd = _ref(), capi.load("libscsamd.so")
    pr, prob, AX, _, _ = base
    AX = AX[:, :3]
    B, Cc = _own_data(prob, AX, pr["cone"], 100, 3.0)
    kw = dict(FIXED, max_iters=500)
    fr = []
    for k in range(3):
        Ak = sp.csc_matrix((AX[:, k], prob.Ai, prob.Ap), shape=(prob.m, prob.n))
        with Work(ref, capi.Problem(Ak, B[:, k], Cc[:, k], pr["cone"]), **kw) as wr:
            fr.append(wr.solve())
    assert all(r["info"]["status_val"] in (1, 2) for r in fr), [r["info"]["status_val"] for r in fr]
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as wa:
        assert set_values(wa, AX) == 0
        rc, fa = values(wa, B, Cc)
    assert rc == 0
    _assert_same_as_reference(fa, fr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. independence
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_column_depends_neither_on_its_position_nor_on_its_neighbours_values(base):
    amd = capi.load("libscsamd.so")
    pr, prob, AX, B, Cc = base
    AX, B, Cc = AX[:, :4], B[:, :4], Cc[:, :4]
    perm = [2, 0, 3, 1]
    other = np.array(AX)
    other[:, 1] = prob.Ax * 1.7  # column 1 under other values; its data stay
    with Work(amd, prob, max_iters=200, **FIXED) as w:
        assert set_values(w, AX) == 0
        rc, first = values(w, B, Cc)
        assert rc == 0
        assert set_values(w, np.asfortranarray(AX[:, perm])) == 0
        rc, second = values(w, np.asfortranarray(B[:, perm]), np.asfortranarray(Cc[:, perm]))
        assert rc == 0
        assert set_values(w, np.asfortranarray(other)) == 0
        rc, third = values(w, B, Cc)
        assert rc == 0
    for pos, k in enumerate(perm):
        assert _equal(second[pos], first[k]), (pos, k)
    for k in (0, 2, 3):
        assert _equal(third[k], first[k]), k
    assert not _equal(third[1], first[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the workspace is untouched; set once, solve many
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_workspace_is_untouched_and_one_set_call_serves_many_solves(base):
    amd = capi.load("libscsamd.so")
    pr, prob, AX, B, Cc = base
    AX, B, Cc = AX[:, :3], B[:, :3], Cc[:, :3]
    B2, Cc2 = _own_data(prob, AX, pr["cone"], 200, 10.0)
    Bs, Cs = family_data(pr["A"], pr["cone"], 3, seed=100, b_scale=[10.0] * 3)
    kw = dict(FIXED, max_iters=200)
    with Work(amd, prob, **kw) as w:
        single, fam = [w.solve()], [w.family(Bs, Cs)[1]]
        assert set_values(w, AX) == 0
        single.append(w.solve())
        fam.append(w.family(Bs, Cs)[1])
        rc, got1 = values(w, B, Cc)
        assert rc == 0
        single.append(w.solve())
        fam.append(w.family(Bs, Cs)[1])
        rc, got2 = values(w, B2, Cc2)
        assert rc == 0
    assert single[0]["info"]["iter"] > 25
    for s_, f_ in zip(single[1:], fam[1:]):
        assert _equal(s_, single[0])
        _assert_columns_equal(f_, fam[0])
    _assert_columns_equal(got1, _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw))
    _assert_columns_equal(got2, _on_updated_workspaces(amd, prob, AX, None, B2, Cc2, kw))
    assert not _equal(got1[0], got2[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals on a live workspace
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_scs_failed_leave_the_outputs_alone_and_give_their_message(base, tmp_path):
    amd = capi.load("libscsamd.so")
    T = amd._scs_types
    pr, prob, AX, B, Cc = base
    K, m, n, nnz = 3, prob.m, prob.n, len(prob.Ax)
    AX, B, Cc = np.asfortranarray(AX[:, :K]), np.asfortranarray(B[:, :K]), np.asfortranarray(Cc[:, :K])
    X = np.full((n + 2 * m, K), 7.0, order="F")
    sols, infos = (T.ScsSolution * K)(), (T.ScsInfo * K)()
    for k in range(K):
        at = X.ctypes.data + k * X.shape[0] * 8
        sols[k].x, sols[k].y, sols[k].s = (C.cast(at + o * 8, T.fp) for o in (0, n, n + m))
    fp = lambda a: a.ctypes.data_as(T.fp)
    why = lambda w: amd.scs_amd_solve_family_values_refusal(w.w) or b""
    setv, solve = amd.scs_amd_family_set_values, amd.scs_amd_solve_family_values

    def refused(w, rc, word):
        assert rc == SCS_FAILED and word in why(w), (rc, word, why(w))
        assert np.all(X == 7.0) and all(infos[k].iter == 0 for k in range(K))

    with Work(amd, prob, max_iters=50, **FIXED) as w:
        refused(w, solve(w.w, K, fp(B), m, fp(Cc), n, None, sols, infos, 0), b"no values are set")
        PX = np.ones((n, K), order="F")
        refused(w, setv(w.w, K, fp(AX), nnz, fp(PX), n), b"PX")
        refused(w, setv(w.w, K, None, nnz, None, 0), b"AX")
        for k in (0, 17, -1):
            refused(w, setv(w.w, k, fp(AX), nnz, None, 0), b"nprob")
        refused(w, setv(w.w, K, fp(AX), nnz - 1, None, 0), b"leading dimension")
        for v in (np.nan, np.inf):
            bad = AX.copy(order="F")
            bad[nnz - 1, K - 1] = v
            refused(w, setv(w.w, K, fp(bad), nnz, None, 0), b"not finite")
        assert setv(w.w, K, fp(AX), nnz, None, 0) == 0 and why(w) == b""
        refused(w, solve(w.w, 2, fp(B), m, fp(Cc), n, None, sols, infos, 0), b"nprob differs")
        for k in (0, 17):
            refused(w, solve(w.w, k, fp(B), m, fp(Cc), n, None, sols, infos, 0), b"nprob")
        refused(w, solve(w.w, K, fp(B), m - 1, fp(Cc), n, None, sols, infos, 0), b"ldb")
        refused(w, solve(w.w, K, fp(B), m, fp(Cc), n - 1, None, sols, infos, 0), b"ldc")
        for args, word in (((None, m, fp(Cc), n, None, sols, infos, 0), b"missing"), ((fp(B), m, None, n, None, sols, infos, 0), b"missing"),
                           ((fp(B), m, fp(Cc), n, None, None, infos, 0), b"missing"), ((fp(B), m, fp(Cc), n, None, sols, None, 0), b"missing")):
            refused(w, solve(w.w, K, *args), word)
        for v in (0.0, -1.0, np.nan, np.inf):
            sc = np.array([1.0, v, 1.0])
            refused(w, solve(w.w, K, fp(B), m, fp(Cc), n, fp(sc), sols, infos, 0), b"scales")
        assert solve(None, K, fp(B), m, fp(Cc), n, None, sols, infos, 0) == SCS_FAILED and setv(None, K, fp(AX), nnz, None, 0) == SCS_FAILED
        assert np.all(X == 7.0)
        rc, out = values(w, B, Cc)  # a correct call afterwards succeeds
        assert rc == 0 and why(w) == b"" and all(r["info"]["iter"] == 50 for r in out)
    for over, word in ((dict(acceleration_lookback=10), b"acceleration_lookback"), (dict(log_csv_filename=str(tmp_path / "l.csv").encode()), b"log_csv")):
        kw = dict(FIXED, max_iters=50)
        kw.update(over)
        with Work(amd, prob, **kw) as w:
            refused(w, setv(w.w, K, fp(AX), nnz, None, 0), word)
            refused(w, solve(w.w, K, fp(B), m, fp(Cc), n, None, sols, infos, 0), word)
    qp, AXq, PXq, Bq, Cq = _qp_values()
    with Work(amd, qp, max_iters=50, **FIXED) as w:  # a workspace with P: PX is missing
        refused(w, setv(w.w, K, fp(AXq), AXq.shape[0], None, 0), b"PX")
        refused(w, setv(w.w, K, fp(AXq), AXq.shape[0], fp(PXq), PXq.shape[0] - 1), b"leading dimension")


def test_a_stale_workspace_is_refused_until_an_update_succeeds(base):
    """scs_amd_test_fail_at (the simulated-failure hook of tests/test_fault_injection_gpu.py) makes one scs_amd_update_matrix fail"""
    amd = capi.load("libscsamd.so")
    pr, prob, AX, B, Cc = base
    AX, B, Cc = AX[:, :3], B[:, :3], Cc[:, :3]
    T = amd._scs_types
    marks = tuple(np.full((r, 3), 7.0, order="F") for r in (prob.n, prob.m, prob.m))
    with Work(amd, prob, max_iters=50, **FIXED) as w:
        assert set_values(w, AX) == 0
        ax = np.ascontiguousarray(prob.Ax)
        amd.scs_amd_test_fail_at(2)
        rc = amd.scs_amd_update_matrix(w.w, ax.ctypes.data_as(T.fp), None)
        amd.scs_amd_test_fail_at(0)
        assert rc != 0
        rc, out = capi.solve_family_values(amd, w.w, B, Cc, warm=marks, warm_start=0)
        assert rc == SCS_FAILED and b"scs_amd_update_matrix failed" in amd.scs_amd_solve_family_values_refusal(w.w)
        assert all(np.all(r[v] == 7.0) for r in out for v in ("x", "y", "s"))
        assert set_values(w, AX) == SCS_FAILED
        _update_matrix(w, prob.Ax)
        rc, out = values(w, B, Cc)  # the stored blocks are still in force
        assert rc == 0 and all(r["info"]["iter"] == 50 for r in out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. memory: allocated by the first set call only, released by the free call; then a wider set
# ---------------------------------------------------------------------------------------------------------------------------------
def test_memory_is_allocated_by_the_first_set_call_and_released_by_free():
    amd = capi.load("libscsamd.so")
    pr = problems.random_socp(20000, 40000, 8, seed=5)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    nnz, n, m, slack = len(prob.Ax), prob.n, prob.m, 8 << 20
    AX = _perturbed(prob.Ax, 16, np.random.default_rng(2))
    B, Cc = family_data(pr["A"], pr["cone"], 16, seed=3)
    free_bytes = lambda: amd.scs_amd_device_free_bytes()
    kw = dict(FIXED, max_iters=5)
    with Work(amd, prob, **kw) as w:  # warm: context, streams, code objects of every path used below
        assert set_values(w, AX[:, :2]) == 0 and values(w, B[:, :2], Cc[:, :2])[0] == 0 and scaled(w, B[:, :2], Cc[:, :2])[0] == 0
        _update_matrix(w, prob.Ax)
    base_free = free_bytes()
    w = Work(amd, prob, **kw)
    assert scaled(w, B, Cc)[0] == 0   # the family state, the R blocks and the block solve's buffers at width 16
    _update_matrix(w, prob.Ax)        # the position maps of an update
    before = free_bytes()
    assert scaled(w, B, Cc)[0] == 0
    assert abs(free_bytes() - before) <= slack  # a caller who never sets values holds none of it
    assert set_values(w, AX[:, :3]) == 0        # width 4
    held4 = before - free_bytes()
    want4 = (2 * nnz + n + m) * 4 * 8
    assert 0.9 * want4 <= held4 <= want4 + (nnz + 2 * n + m) * 4 * 8 + slack, (held4, want4)
    assert values(w, B[:, :3], Cc[:, :3])[0] == 0
    assert before - free_bytes() <= held4 + slack  # the solve allocates nothing more (the cone's block state is rebuilt narrower)
    amd.scs_amd_family_free_values(w.w)
    freed = free_bytes()
    assert freed >= before - slack
    rc, _ = values(w, B[:, :3], Cc[:, :3])
    assert rc == SCS_FAILED and b"no values are set" in amd.scs_amd_solve_family_values_refusal(w.w)
    assert set_values(w, AX) == 0                # again, at width 16
    held16 = freed - free_bytes()
    assert 0.9 * 4 * want4 <= held16 <= 4 * want4 + (nnz + 2 * n + m) * 16 * 8 + slack, (held16, want4)
    assert set_values(w, AX[:, :3]) == 0         # narrower: on the blocks that are there
    assert abs((freed - free_bytes()) - held16) <= slack
    assert set_values(w, AX) == 0
    rc, out = values(w, B, Cc)
    assert rc == 0 and all(r["info"]["iter"] == 5 for r in out)
    w.close()
    assert abs(free_bytes() - base_free) <= slack
    amd.scs_amd_family_free_values(None)  # NULL-safe


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the Python object
# ---------------------------------------------------------------------------------------------------------------------------------
def test_python_object(base):
    from scs_amd.solver import SCS
    amd = capi.load("libscsamd.so")
    pr, prob, AX, B, Cc = base
    AX, B, Cc = AX[:, :3], B[:, :3], Cc[:, :3]
    mats = [sp.csc_matrix((AX[:, k], prob.Ai, prob.Ap), shape=(prob.m, prob.n)) for k in range(3)]
    with Work(amd, prob, max_iters=200, **FIXED) as w:
        assert set_values(w, AX) == 0
        rc, want = values(w, B, Cc)
        assert rc == 0
    data = dict(A=pr["A"], b=pr["b"], c=pr["c"])
    with SCS(data, pr["cone"], adaptive_scale=0, acceleration_lookback=0, max_iters=200) as s:
        got = s.solve_family(B, Cc, A=mats)
        got_arr = s.solve_family(B, Cc, A=AX)
        assert s.set_family_values(mats) == 3
        got_set = s.solve_family(B, Cc, own_values=True)
        other = mats[1].tolil()
        other[0, :] = 1.0
        with pytest.raises(ValueError, match="pattern"):
            s.solve_family(B, Cc, A=[mats[0], other.tocsc(), mats[2]])
        with pytest.raises(ValueError, match="stream"):
            s.solve_family(B, Cc, A=mats, stream=True)
        with pytest.raises(ValueError):
            s.solve_family(B, Cc, A=mats[:2])
        s.free_family_values()
        with pytest.raises(ValueError, match="no values are set"):
            s.solve_family(B, Cc, own_values=True)
    for k in range(3):
        assert _equal(got[k], want[k]) and _equal(got_arr[k], want[k]) and _equal(got_set[k], want[k])
    with SCS(data, pr["cone"], adaptive_scale=0, acceleration_lookback=5) as s:
        with pytest.raises(ValueError, match="acceleration_lookback"):
            s.solve_family(B, Cc, A=mats)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the set-up paths of a large problem: equilibration on the device (nnz(A) >= 1e5), scs_init's own choice of the numbering
# ---------------------------------------------------------------------------------------------------------------------------------
def test_columns_equal_the_updated_workspaces_where_scs_init_equilibrates_on_the_device():
    amd = capi.load("libscsamd.so")
    pr = problems.random_socp(20000, 40000, 8, seed=5)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    assert len(prob.Ax) >= 100000
    AX = _perturbed(prob.Ax, 3, np.random.default_rng(6))
    B, Cc = _own_data(prob, AX, pr["cone"], 7, 1.0)
    kw = dict(FIXED, adaptive_scale=1, max_iters=60)
    with Work(amd, prob, **kw) as w:
        assert set_values(w, AX) == 0
        rc, got = values(w, B, Cc)
        assert rc == 0
    want = _on_updated_workspaces(amd, prob, AX, None, B, Cc, kw)
    assert all(r["info"]["iter"] > 25 for r in want)
    _assert_columns_equal(got, want)
