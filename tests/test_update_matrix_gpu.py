"""New VALUES of A and P on a live workspace (scs_amd_update_matrix, include/scs_amd.h): scs_init's value-dependent half again, without
its pattern-dependent half.

The yardstick throughout is a FRESH workspace of this library on the new values.  The state after an update is the state scs_init
produces and every reduction is deterministic, so the comparison is bit for bit -- x, y, s, iter, status_val and every numeric ScsInfo
field except the times -- and no tolerance is invented.  Only the last case looks outside the library (the reference, exact CG, at the
bound tests/test_solve_gpu.py applies to a single solve).

Value sets: A1 = A0 o (1 + 0.3 u), u uniform in (-1, 1), 3 % of the entries sign-flipped and 1 % set to exactly 0 (the pattern keeps
them); P1 the same way, then made diagonally dominant (PSD) through its diagonal entries, which are in the pattern.

(The issue's "fused, tiny" shape lists cones that sum to 92 rows, not 90: the cone list is kept as stated and m follows it.)"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, problems

pytestmark = pytest.mark.gpu

TIMES = ("setup_time", "solve_time", "lin_sys_time", "cone_time", "accel_time")
NUMERIC = [k for k in capi.INFO_FIELDS if k not in TIMES]


class Work:
    """one workspace of `lib` on `prob`: solve, scs_update, scs_amd_update_matrix"""

    def __init__(self, lib, prob, cg_tol_override=None, **over):
        self.lib, self.prob, self.T = lib, prob, lib._scs_types
        over.setdefault("verbose", 0)
        self.st = capi.default_settings(lib, **over)
        self.w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(self.st))
        assert self.w, "scs_init returned NULL"
        if cg_tol_override is not None:
            lib.scs_amd_set_cg_tol_override(self.w, float(cg_tol_override))

    def _vals(self, v):
        return None if v is None else np.ascontiguousarray(v, dtype=self.T.np_float)

    def update_matrix(self, Ax=None, Px=None):
        ax, px = self._vals(Ax), self._vals(Px)
        return self.lib.scs_amd_update_matrix(self.w, None if ax is None else ax.ctypes.data_as(self.T.fp),
                                              None if px is None else px.ctypes.data_as(self.T.fp))

    def update(self, b=None, c=None):
        bb, cc = self._vals(b), self._vals(c)
        return self.lib.scs_update(self.w, None if bb is None else bb.ctypes.data_as(self.T.fp), None if cc is None else cc.ctypes.data_as(self.T.fp))

    def solve(self):
        T, f = self.T, self.T.np_float
        x, y, s = np.zeros(self.prob.n, dtype=f), np.zeros(self.prob.m, dtype=f), np.zeros(self.prob.m, dtype=f)
        sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
        info = T.ScsInfo()
        rc = self.lib.scs_solve(self.w, C.byref(sol), C.byref(info), 0)
        return dict(x=x, y=y, s=s, info=capi.info_dict(info), rc=rc)

    def family(self, B, Cc):
        return capi.solve_family(self.lib, self.w, B, Cc)

    def close(self):
        if self.w:
            self.lib.scs_finish(self.w)
            self.w = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def same_bits(a, b, what=""):
    """bit equality of x, y, s and of every numeric ScsInfo field except the times"""
    for v in ("x", "y", "s"):
        assert a[v].tobytes() == b[v].tobytes(), f"{what}: {v} differs in {int(np.count_nonzero(a[v] != b[v]))} of {len(a[v])} entries"
    for k in NUMERIC:
        assert np.float64(a["info"][k]).tobytes() == np.float64(b["info"][k]).tobytes(), (what, k, a["info"][k], b["info"][k])


def perturbed(data, seed):
    """v o (1 + 0.3 u), 3 % sign flips, 1 % exact zeros"""
    rng = np.random.default_rng(seed)
    out = np.asarray(data, dtype=np.float64) * (1.0 + 0.3 * rng.uniform(-1, 1, len(data)))
    out[rng.random(len(data)) < 0.03] *= -1.0
    out[rng.random(len(data)) < 0.01] = 0.0
    return out


def with_values(M, data):
    return sp.csc_matrix((np.asarray(data, dtype=M.dtype), M.indices, M.indptr), shape=M.shape)


def fresh(lib, A, b, c, cone, P=None, T=None, cg_tol_override=None, **over):
    prob = capi.Problem(A, b, c, cone, P=P, T=T or lib._scs_types)
    with Work(lib, prob, cg_tol_override=cg_tol_override, **over) as w:
        return w.solve()


# ---- shapes -------------------------------------------------------------------------------------------------------------------
TINY_CONE = dict(z=10, l=20, bu=np.linspace(0.5, 2.0, 10), bl=-np.linspace(1.0, 0.2, 10), q=[12, 8], s=[5, 4], ep=1, p=[0.3])


def mixed_problem(n, cone, seed, per_col=4):
    """feasible and bounded by construction on every cone type of `cone` (the oracle's projection gives the dual-cone point)"""
    from oracle import pyoracle
    rng = np.random.default_rng(seed)
    m = capi.cone_rows(cone)
    z = rng.standard_normal(m)
    y = pyoracle.oracle_proj_dual_cone(cone, z)
    s = y - z
    x = rng.standard_normal(n)
    A = sp.random(m, n, density=min(1.0, per_col / m), random_state=seed, format="csc", data_rvs=rng.standard_normal)
    A = (A + sp.csc_matrix((np.full(n, 0.7), (np.arange(n) % m, np.arange(n))), shape=(m, n))).tocsc()
    A.sort_indices()
    return dict(A=A, b=A @ x + s, c=-(A.T @ y), cone=cone)


_cache = {}


def tiny():
    if "tiny" not in _cache:
        pr = mixed_problem(40, TINY_CONE, 11, per_col=6)
        assert pr["A"].shape == (92, 40) and pr["A"].nnz <= 4096
        _cache["tiny"] = (pr, perturbed(pr["A"].data, 1))
    return _cache["tiny"]


def renumbered():
    if "band" not in _cache:
        pr = problems.random_socp(30000, 60000, 10, band=512, scramble=3)
        _cache["band"] = (pr, perturbed(pr["A"].data, 2))
    return _cache["band"]


def with_p():
    if "p" not in _cache:
        n, m = 2000, 4000
        pr = problems.random_socp(n, m, 10, seed=77)
        rng = np.random.default_rng(7)
        rows = np.concatenate([rng.integers(0, j + 1, 4) for j in range(n)] + [np.arange(n)])
        cols = np.concatenate([np.repeat(np.arange(n), 4), np.arange(n)])
        pat = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))  # duplicates merge: about 5 entries per column, diagonal present
        pat.sort_indices()

        diag = pat.indices == np.repeat(np.arange(n), np.diff(pat.indptr))
        rows, cols = pat.indices, np.repeat(np.arange(n), np.diff(pat.indptr))

        def psd(data):
            """diagonally dominant through the diagonal entries (all n are in the pattern); stored zeros stay stored"""
            d = np.array(data, dtype=np.float64)
            off = ~diag
            rowsum = np.bincount(rows[off], np.abs(d[off]), n) + np.bincount(cols[off], np.abs(d[off]), n)
            d[diag] = rowsum[cols[diag]] + 1.0
            return d
        assert int(diag.sum()) == n
        P0x = psd(rng.uniform(-1, 1, pat.nnz))
        P1x = psd(perturbed(P0x, 4))
        _cache["p"] = (pr, perturbed(pr["A"].data, 3), with_values(pat, P0x), P1x)
    return _cache["p"]


def three_step(lib, pr, A1x, over, cg_tol_override=None, T=None, P=None):
    """init on A0 and solve; update to A1, solve, compare with a fresh init on A1; update back to A0, compare with the first solve"""
    A0 = pr["A"]
    prob = capi.Problem(A0, pr["b"], pr["c"], pr["cone"], P=P, T=T or lib._scs_types)
    with Work(lib, prob, cg_tol_override=cg_tol_override, **over) as w:
        first = w.solve()
        assert w.update_matrix(A1x) == 0
        second = w.solve()
        assert w.update_matrix(prob.Ax) == 0
        third = w.solve()
    want = fresh(lib, with_values(A0, A1x), pr["b"], pr["c"], pr["cone"], P=P, T=T, cg_tol_override=cg_tol_override, **over)
    assert first["x"].tobytes() != second["x"].tobytes(), "the update changed nothing"
    same_bits(second, want, "update to A1 against a fresh workspace on A1")
    same_bits(third, first, "update back to A0 against the first solve")
    return first, second


def reorder_and_layout(lib, prob, **over):
    with Work(lib, prob, **over) as w:
        r, l = (C.c_double * 6)(), (C.c_double * 6)()
        lib.scs_amd_get_reorder_info(w.w, r)
        lib.scs_amd_get_layout_info(w.w, l)
        return list(r), list(l)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_fused_tiny_every_cone_type():
    lib = capi.load("libscsamd.so")
    pr, A1x = tiny()
    three_step(lib, pr, A1x, dict(max_iters=60))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", ["1", "0"])
@pytest.mark.parametrize("cg", [None, 1e-12], ids=["schedule", "exact_cg"])
def test_renumbered_wave_layouts(monkeypatch, reorder, cg):
    lib = capi.load("libscsamd.so")
    monkeypatch.setenv("SCS_AMD_REORDER", reorder)
    monkeypatch.setenv("SCS_AMD_WAVEROWS", "1")  # 3e5 nonzeros: below the size at which the library builds the layouts on its own
    pr, A1x = renumbered()
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    r, l = reorder_and_layout(lib, prob)
    assert r[0] == float(reorder == "1") and l[0] == 1.0 and l[3] == 1.0, (r, l)  # otherwise the case tests nothing
    three_step(lib, pr, A1x, dict(max_iters=100, acceleration_lookback=0), cg_tol_override=cg)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "P", "both"])
def test_with_p(which):
    lib = capi.load("libscsamd.so")
    pr, A1x, P0, P1x = with_p()
    over = dict(max_iters=100)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], P=P0)
    assert np.array_equal(prob.Pi, P0.indices)
    newA = A1x if which in ("A", "both") else None
    newP = P1x if which in ("P", "both") else None
    with Work(lib, prob, **over) as w:
        first = w.solve()
        assert w.update_matrix(newA, newP) == 0
        got = w.solve()
    want = fresh(lib, pr["A"] if newA is None else with_values(pr["A"], newA), pr["b"], pr["c"], pr["cone"],
                 P=P0 if newP is None else with_values(P0, newP), **over)
    assert first["x"].tobytes() != got["x"].tobytes()
    same_bits(got, want, f"update of {which}")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["bc_then_matrix", "matrix_then_bc"])
def test_update_ordering(order):
    lib = capi.load("libscsamd.so")
    pr, A1x = tiny()
    b2, c2 = pr["b"] * 1.05, pr["c"] * 0.9
    over = dict(max_iters=60)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    with Work(lib, prob, **over) as w:
        w.solve()
        if order == "bc_then_matrix":
            assert w.update(b2, c2) == 0 and w.update_matrix(A1x) == 0
        else:
            assert w.update_matrix(A1x) == 0 and w.update(b2, c2) == 0
        got = w.solve()
    same_bits(got, fresh(lib, with_values(pr["A"], A1x), b2, c2, pr["cone"], **over), order)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_factor", [1.0, 0.01], ids=["as_generated", "c_scaled"])
def test_adaptive_scale_and_anderson_do_not_leak(monkeypatch, c_factor):
    """the default settings (adaptive_scale = 1, acceleration_lookback = 10) to termination, then update and solve.  On the data as
    generated the first solve ends without a scale update; with c scaled by 0.01 the scale does move (asserted): a scale that stayed
    adapted across the update would show in the second solve."""
    lib = capi.load("libscsamd.so")
    monkeypatch.setenv("SCS_AMD_REORDER", "1")
    monkeypatch.setenv("SCS_AMD_WAVEROWS", "1")
    pr, A1x = renumbered()
    c = pr["c"] * c_factor
    prob = capi.Problem(pr["A"], pr["b"], c, pr["cone"])
    with Work(lib, prob) as w:
        first = w.solve()
        assert first["info"]["status_val"] == 1, first["info"]
        assert first["info"]["accepted_accel_steps"] + first["info"]["rejected_accel_steps"] > 0  # the acceleration was at work
        if c_factor != 1.0:
            assert first["info"]["scale_updates"] > 0 and first["info"]["scale"] != 0.1, first["info"]
        assert w.update_matrix(A1x) == 0
        got = w.solve()
    same_bits(got, fresh(lib, with_values(pr["A"], A1x), pr["b"], c, pr["cone"]), "after an adaptive-scale, accelerated solve")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny", "renumbered"])
def test_family_after_update(monkeypatch, shape):
    lib = capi.load("libscsamd.so")
    if shape == "renumbered":
        monkeypatch.setenv("SCS_AMD_REORDER", "1")
        monkeypatch.setenv("SCS_AMD_WAVEROWS", "1")
    pr, A1x = tiny() if shape == "tiny" else renumbered()
    over = dict(max_iters=60, adaptive_scale=0, acceleration_lookback=0)
    K = 3
    B = np.column_stack([pr["b"] * f for f in (1.0, 1.1, 0.8)])
    Cc = np.column_stack([pr["c"] * f for f in (1.0, 0.9, 1.2)])
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    with Work(lib, prob, **over) as w:
        rc0, before = w.family(B, Cc)  # the family state exists before the update
        assert rc0 == 0 and w.update_matrix(A1x) == 0
        rc, got = w.family(B, Cc)
    with Work(lib, capi.Problem(with_values(pr["A"], A1x), pr["b"], pr["c"], pr["cone"]), **over) as w:
        rcw, want = w.family(B, Cc)
    assert rc == rcw == 0 and len(got) == K
    for k in range(K):
        assert before[k]["x"].tobytes() != got[k]["x"].tobytes()
        same_bits(got[k], want[k], f"family column {k}")


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bias", [("libscsamd_f32.so", None), ("libscsamd_dlong.so", None), ("libscsamd_dlong.so", str(2**31 + 2**20))],
                         ids=["f32", "dlong", "dlong_offset_bias"])
def test_other_builds(monkeypatch, name, bias):
    lib = capi.load(name)
    monkeypatch.setenv("SCS_AMD_REORDER", "1")
    monkeypatch.setenv("SCS_AMD_WAVEROWS", "1")
    if bias:
        monkeypatch.setenv("SCS_AMD_TEST_OFFSET_BIAS", bias)
    else:
        monkeypatch.delenv("SCS_AMD_TEST_OFFSET_BIAS", raising=False)
    pr, A1x = renumbered()
    T = lib._scs_types
    A1x = A1x.astype(T.np_float)
    pr = dict(pr, A=pr["A"].astype(T.np_float))
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=T)
    r, l = reorder_and_layout(lib, prob)
    assert r[0] == 1.0 and l[0] == 1.0 and l[3] == 1.0, (r, l)
    three_step(lib, pr, A1x, dict(max_iters=100, acceleration_lookback=0), T=T)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_workspace_untouched():
    lib = capi.load("libscsamd.so")
    pr, A1x = tiny()
    over = dict(max_iters=60)
    with Work(lib, capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"]), **over) as w:
        first = w.solve()
        bad = A1x.copy()
        bad[len(bad) // 2] = np.nan
        assert w.update_matrix(bad) == -1
        assert w.update_matrix(None, np.ones(3)) == -1  # Px on a workspace without P
        assert w.update_matrix(None, None) == 0
        same_bits(w.solve(), first, "after refused updates")
    prp, A1p, P0, P1x = with_p()
    over = dict(max_iters=40)
    with Work(lib, capi.Problem(prp["A"], prp["b"], prp["c"], prp["cone"], P=P0), **over) as w:
        first = w.solve()
        bad = P1x.copy()
        bad[-1] = np.inf
        assert w.update_matrix(A1p, bad) == -1  # nothing of the call is applied, the good A values included
        assert w.update_matrix(None, None) == 0
        same_bits(w.solve(), first, "after an inf in Px")
    assert lib.scs_amd_update_matrix(None, None, None) == -1


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_failure_convention():
    """the simulated-failure hook of tests/test_fault_injection_gpu.py: the first checked HIP call of the update is reported as failed
    although it succeeded.  Nothing is provoked on the device."""
    lib = capi.load("libscsamd.so")
    pr, A1x = tiny()
    over = dict(max_iters=60)
    with Work(lib, capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"]), **over) as w:
        w.solve()
        lib.scs_amd_test_fail_at(1)
        try:
            assert w.update_matrix(A1x) == -1
        finally:
            lib.scs_amd_test_fail_at(0)
        r = w.solve()
        assert r["rc"] == -4 and r["info"]["status_val"] == -4  # SCS_FAILED
        assert np.all(np.isnan(r["x"])) and np.all(np.isnan(r["y"])) and np.all(np.isnan(r["s"]))
        assert w.update_matrix(A1x) == 0
        got = w.solve()
    same_bits(got, fresh(lib, with_values(pr["A"], A1x), pr["b"], pr["c"], pr["cone"], **over), "after a failed, then a successful update")


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
def test_against_the_reference_exact_cg():
    """case 1's cone at n = 200, m = 450, exact CG.  The workspace starts on (A0, b0, c0); the new values A1 come with the (b1, c1) that
    make THEIR problem feasible and bounded (scs_update; the two updates commute, see above); the reference is initialised fresh on
    (A1, b1, c1).  The comparison and the bound are those of tests/test_solve_gpu.py for a single solve."""
    from oracle import pyoracle
    if not pyoracle.ref_available("libscsindir_ref_exactcg.so"):
        pytest.skip("oracle/_ref/libscsindir_ref_exactcg.so not built")
    ref = pyoracle.load_ref("libscsindir_ref_exactcg.so")
    lib = capi.load("libscsamd.so")
    cone = dict(TINY_CONE, z=100, l=288)
    pr0 = mixed_problem(200, cone, 12, per_col=6)
    assert pr0["A"].shape == (450, 200)
    A1x = perturbed(pr0["A"].data, 5)
    A1 = with_values(pr0["A"], A1x)
    rng = np.random.default_rng(13)
    z = rng.standard_normal(450)
    y = pyoracle.oracle_proj_dual_cone(cone, z)
    b1, c1 = A1 @ rng.standard_normal(200) + (y - z), -(A1.T @ y)
    kw = dict(verbose=0, acceleration_lookback=0, eps_abs=1e-3, eps_rel=1e-3, max_iters=2000)  # (short trajectories: the case stays in the low seconds)
    with Work(lib, capi.Problem(pr0["A"], pr0["b"], pr0["c"], cone), cg_tol_override=1e-12, **kw) as w:
        w.solve()
        assert w.update_matrix(A1x) == 0 and w.update(b1, c1) == 0
        ra = w.solve()
    rr = capi.solve(ref, capi.Problem(A1, b1, c1, cone), **kw)
    ia, ir = ra["info"], rr["info"]
    assert ia["status_val"] == ir["status_val"] == 1, (ia["status"], ir["status"])
    assert ia["iter"] == ir["iter"], (ia["iter"], ir["iter"])
    assert ia["scale_updates"] == ir["scale_updates"]
    for k in ("pobj", "dobj", "res_pri", "res_dual", "gap", "scale"):
        assert abs(ia[k] - ir[k]) / max(abs(ia[k]), abs(ir[k]), 1e-3) <= 1e-6, (k, ia[k], ir[k])
    for v in ("x", "y", "s"):
        d = np.abs(ra[v] - rr[v]).max() / max(1.0, np.abs(rr[v]).max())
        assert d <= 1e-6, (v, d)


# ---- 11 --------------------------------------------------------------------------------------------------------------------------
def test_python_interface():
    from scs_amd.solver import SCS
    lib = capi.load("libscsamd.so")
    pr, A1x, P0, P1x = with_p()
    A1 = with_values(pr["A"], A1x)
    P1 = with_values(P0, P1x)
    kw = dict(max_iters=60)
    want_a = fresh(lib, A1, pr["b"], pr["c"], pr["cone"], P=P0, **kw)
    want_ap = fresh(lib, A1, pr["b"], pr["c"], pr["cone"], P=P1, **kw)
    for form in ("sparse", "values"):
        with SCS(dict(A=pr["A"], b=pr["b"], c=pr["c"], P=P0), pr["cone"], **kw) as s:
            s.solve()
            s.update(A=A1 if form == "sparse" else A1x)
            got = s.solve(warm_start=False)
            same_bits(got, want_a, f"SCS.update(A={form})")
            s.update(P=P1 if form == "sparse" else P1x)
            same_bits(s.solve(warm_start=False), want_ap, f"SCS.update(P={form})")
    with SCS(dict(A=pr["A"], b=pr["b"], c=pr["c"], P=P0), pr["cone"], **kw) as s:
        first = s.solve()
        other = pr["A"].tolil(copy=True)
        i, j = [(i, j) for i in range(5) for j in range(5) if pr["A"][i, j] == 0][0]
        other[i, j] = 1.0
        with pytest.raises(ValueError):
            s.update(A=other.tocsc())
        with pytest.raises(ValueError):
            s.update(A=A1x[:-1])
        with pytest.raises(ValueError):
            s.update(P=np.full(len(P1x), np.nan))
        same_bits(s.solve(warm_start=False), first, "after refused Python updates")
        b2 = pr["b"] * 1.05
        s.update(b=b2)  # as before
        same_bits(s.solve(warm_start=False), fresh(lib, pr["A"], b2, pr["c"], pr["cone"], P=P0, **kw), "update(b=)")
