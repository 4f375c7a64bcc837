"""scs_amd_solve_family_scaled (include/scs_amd.h): scs_amd_solve_family with a scale per problem, fixed or adapted by the column's
own update_scale.

Every column must be what scs_update + scs_solve computes for that problem alone on a FRESH workspace of that scale (the reference
and the project's single solve carry an adapted scale from one solve to the next on one workspace; a family column starts from the
scale it is given):
 * against the reference build with exact linear solves on both sides (libscsindir_ref_exactcg.so; ours via
   scs_amd_set_cg_tol_override): equal status, iteration count and number of scale updates, ScsInfo and (x, y, s) to 1e-6 relative
   -- the bar and the floor of tests/test_solve_gpu.py::test_exact_cg_trajectory_parity;
 * bit for bit against scs_amd_solve_family wherever both compute the same thing: equal fixed scales, and the columns of an adaptive
   family that never update.
The problems are those of tests/test_family_gpu.py.  Unscaled, the 200 x 600 family needs 225 .. 425 iterations with adaptive scaling
(1 or 2 updates per column); b scaled by 10 needs 125 .. 400 and only one column of eight updates.
"""
import ctypes as C

import numpy as np
import pytest

from scs_amd import capi, problems
from tests.family_util import Work, family_data
from tests.test_family_gpu import _mixed, _qp, _ref, _rel, _same_bits, _socp

pytestmark = pytest.mark.gpu
REL = 1e-6
SCS_FAILED = -4
FIXED = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)
ADAPT = dict(verbose=0, adaptive_scale=1, acceleration_lookback=0)
INFO_KEYS = ("pobj", "dobj", "res_pri", "res_dual", "gap")


def scaled(w, B, Cc, scales=None, warm=None, warm_start=None):
    """the call of the new entry on the workspace of a tests.family_util.Work"""
    return capi.solve_family_scaled(w.lib, w.w, B, Cc, scales=scales, warm=warm, warm_start=warm_start)


def _fresh_columns(lib, prob, B, Cc, cg_tol_override=None, scales=None, **kw):
    """column after column, each on a workspace of its own (at scales[k] when given)"""
    out = []
    for k in range(B.shape[1]):
        over = dict(kw) if scales is None else dict(kw, scale=float(scales[k]))
        with Work(lib, prob, cg_tol_override=cg_tol_override, **over) as w:
            out.append(w.solve(B[:, k], Cc[:, k]))
    return out


def _same_bits_and_info(a, b):
    return _same_bits(a, b) and all(a["info"][key] == b["info"][key] or (np.isnan(a["info"][key]) and np.isnan(b["info"][key]))
                                    for key in INFO_KEYS)


def _assert_same_as(fam, want, rel=REL):
    for k, (ra, rr) in enumerate(zip(fam, want)):
        ia, ir = ra["info"], rr["info"]
        print(f"column {k}: status {ia['status_val']} / {ir['status_val']}, iter {ia['iter']} / {ir['iter']}, updates "
              f"{ia['scale_updates']} / {ir['scale_updates']}, scale {ia['scale']:.6g} / {ir['scale']:.6g}, "
              + ", ".join(f"{key} {_rel(ia[key], ir[key]):.1e}" for key in INFO_KEYS)
              + ", " + ", ".join(f"{v} {np.abs(ra[v] - rr[v]).max() / max(1.0, np.abs(rr[v]).max()):.1e}" for v in ("x", "y", "s")))
    for k, (ra, rr) in enumerate(zip(fam, want)):
        ia, ir = ra["info"], rr["info"]
        assert ia["status_val"] == ir["status_val"], (k, ia["status"], ir["status"])
        assert ia["iter"] == ir["iter"], (k, ia["iter"], ir["iter"])
        assert ia["scale_updates"] == ir["scale_updates"], (k, ia["scale_updates"], ir["scale_updates"])
        for key in ("scale",) + INFO_KEYS:
            assert _rel(ia[key], ir[key]) <= rel, (k, key, ia[key], ir[key])
        for v in ("x", "y", "s"):
            d = np.abs(ra[v] - rr[v]).max() / max(1.0, np.abs(rr[v]).max())
            assert d <= rel, (k, v, d)


@pytest.fixture(scope="module")
def base():
    """CASES[0] of tests/test_solve_gpu.py (n = 200, m = 600, second-order cones)"""
    return _socp(200, 600, 8, 1)


def _family(base, f, K=8):
    pr, _ = base
    return family_data(pr["A"], pr["cone"], K, seed=100, b_scale=None if f == 1 else [float(f)] * K)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. / 2. trajectory parity with the reference, adaptive, exact CG
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unscaled_reference(base):
    """the unscaled family on the reference, a fresh workspace per column: 325, 425, 325, 375, 225, 275, 300, 375 iterations with
    2, 2, 2, 2, 2, 1, 2, 2 scale updates"""
    pr, prob = base
    B, Cc = _family(base, 1)
    fr = _fresh_columns(_ref(), prob, B, Cc, **ADAPT)
    print([(r["info"]["iter"], r["info"]["scale_updates"], r["info"]["scale"]) for r in fr])
    assert all(r["info"]["status_val"] == 1 for r in fr)
    assert len({r["info"]["iter"] for r in fr}) >= 3 and len({r["info"]["scale_updates"] for r in fr}) >= 2
    return B, Cc, fr


@pytest.mark.parametrize("K", [8, 3])
def test_adaptive_exact_cg_trajectory_parity_with_the_reference(base, unscaled_reference, K):
    """K = 3: width 4 with a padding column.  Every column updates its scale once or twice, at checks of its own, and freezes at a
    check of its own."""
    amd = capi.load("libscsamd.so")
    _, prob = base
    B, Cc, fr = unscaled_reference
    with Work(amd, prob, cg_tol_override=1e-12, **ADAPT) as wa:
        rc, fa = scaled(wa, B[:, :K], Cc[:, :K])
    assert rc == 0
    _assert_same_as(fa, fr[:K])


def test_adaptive_exact_cg_trajectory_parity_with_P():
    ref, amd = _ref(), capi.load("libscsamd.so")
    prob, B, Cc = _qp()
    fr = _fresh_columns(ref, prob, B, Cc, **ADAPT)
    assert all(r["info"]["status_val"] == 1 for r in fr)
    with Work(amd, prob, cg_tol_override=1e-12, **ADAPT) as wa:
        rc, fa = scaled(wa, B, Cc)
    assert rc == 0
    _assert_same_as(fa, fr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a scale sweep holds the bits of scs_amd_solve_family at each scale
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP = [0.01, 0.1, 1.0, 10.0]


def _box_psd():
    """the fixture of tests/test_family_gpu.py::test_box_and_a_psd_block_of_order_73_from_the_loop: the box cone's Newton iteration
    reads r_y"""
    nb = 40
    cone = dict(l=30, bu=np.ones(nb), bl=-np.ones(nb), bsize=nb + 1, q=[], s=[73])
    pr = problems.random_cone_prob(300, capi.cone_rows(cone), 6, cone, seed=9)
    B, Cc = family_data(pr["A"], pr["cone"], 1, seed=5)
    return capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"]), B, Cc, dict(max_iters=30), 1e-12


def _sweep_socp(base):
    """column 0 of the family with b scaled by 3: at exact CG the reference needs more than 2000, 900, 150 and 425 iterations at the
    four scales; default CG schedule here, capped at 500"""
    B, Cc = _family(base, 3, K=1)
    return base[1], B, Cc, dict(max_iters=500), None


def _sweep_zero_cone():
    """zero-cone rows: the 1 / (1000 scale) branch of diag_r (with a nonnegative cone, two second-order cones and a PSD block)"""
    prob, _, _, B, Cc = _mixed()
    return prob, B[:, 2:3], Cc[:, 2:3], dict(max_iters=300), None


@pytest.mark.parametrize("which,warm", [("socp", False), ("socp", True), ("box_psd", False), ("zero_cone", False)])
def test_a_scale_sweep_holds_the_bits_of_the_shared_scale_entry_at_each_scale(base, which, warm):
    """one problem four times, scales 0.01, 0.1, 1, 10, adaptive_scale = 0: column j must hold the bits of scs_amd_solve_family on a
    workspace initialised with scale = scales[j], the same column replicated at the same width.  warm: the same from a warm start (an
    unconverged iterate, the same in every column), where v_y = y + s / R_y reads the column's own R_y."""
    amd = capi.load("libscsamd.so")
    prob, b, c, over, tol = {"socp": lambda: _sweep_socp(base), "box_psd": _box_psd, "zero_cone": _sweep_zero_cone}[which]()
    B, Cc = np.asfortranarray(np.repeat(b, 4, axis=1)), np.asfortranarray(np.repeat(c, 4, axis=1))
    kw = dict(FIXED, **over)
    w0 = None
    if warm:
        with Work(amd, prob, cg_tol_override=tol, **dict(kw, max_iters=60)) as w:
            rc, part = w.family(B, Cc)
        assert rc == 0 and part[0]["info"]["status_val"] == 2
        w0 = tuple(np.column_stack([r[v] for r in part]) for v in ("x", "y", "s"))
    with Work(amd, prob, cg_tol_override=tol, **kw) as w:
        rc, sweep = scaled(w, B, Cc, scales=SWEEP, warm=w0)
    assert rc == 0
    print([(r["info"]["status_val"], r["info"]["iter"]) for r in sweep])
    assert len({r["info"]["res_pri"] for r in sweep}) == 4  # the scales matter
    for j, sc in enumerate(SWEEP):
        with Work(amd, prob, cg_tol_override=tol, **dict(kw, scale=sc)) as w:
            rc, want = w.family(B, Cc, warm=w0)
        assert rc == 0
        assert _same_bits_and_info(sweep[j], want[j]), (j, sc, sweep[j]["info"], want[j]["info"])
        assert sweep[j]["info"]["scale"] == want[j]["info"]["scale"] == sc and sweep[j]["info"]["scale_updates"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. without scales and without adaptive scaling: the old entry
# ---------------------------------------------------------------------------------------------------------------------------------
def test_without_scales_and_adaptive_scaling_it_is_the_shared_scale_entry_bit_for_bit(base):
    amd = capi.load("libscsamd.so")
    _, prob = base
    B, Cc = _family(base, 10, K=5)  # width 8 with three padding columns
    with Work(amd, prob, **FIXED) as w:
        rc, want = w.family(B, Cc)
        rc2, got = scaled(w, B, Cc)
    assert rc == 0 and rc2 == 0 and all(r["info"]["status_val"] == 1 for r in want)
    for k in range(5):
        assert _same_bits_and_info(got[k], want[k]), k
        assert got[k]["info"]["scale"] == want[k]["info"]["scale"] and got[k]["info"]["scale_updates"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a column does not depend on what its neighbours do to their scales
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,tol,some_update", [(10, None, False), (10, 1e-12, True), (3, None, True)])
def test_a_column_that_never_updates_holds_the_bits_of_a_fixed_scale_family_whatever_its_neighbours_do(base, f, tol, some_update):
    """A neighbour's update rewrites that neighbour's R, preconditioner, g and v and must not change one bit of a column that did not
    update: every column with zero updates holds the bits of scs_amd_solve_family on an adaptive_scale = 0 workspace at the same
    width; permuting the columns permutes the bits; a second call returns the same bits.
    b scaled by 10, default CG schedule: measured on the MI355X, NO column of this family updates its scale -- neither in the family
    (250, 300, 250, 500, 225, 225, 250, 275 iterations) nor in the project's own single solves on fresh workspaces (275, 250, 250,
    500, 250, 225, 200, 250), and the reference with its default schedule updates one column only, by a factor (0.27) just past the
    threshold of 1 / sqrt(10).  The figures 7 and 1 belong to exact CG.  So that family runs here under both schedules -- under the
    default one all eight columns must hold the fixed-scale bits, under exact CG seven do and column 3 updates, as on the reference
    -- and the default schedule is also run on b scaled by 3, where four columns never update and four update once or twice (the
    project's single solves and the reference's default schedule agree on which)."""
    amd = capi.load("libscsamd.so")
    _, prob = base
    B, Cc = _family(base, f)
    perm = [5, 3, 0, 7, 1, 6, 2, 4]
    with Work(amd, prob, cg_tol_override=tol, **ADAPT) as w:
        rc, first = scaled(w, B, Cc)
        rc2, again = scaled(w, B, Cc)
        rc3, moved = scaled(w, np.asfortranarray(B[:, perm]), np.asfortranarray(Cc[:, perm]))
    assert rc == 0 and rc2 == 0 and rc3 == 0
    ups = [r["info"]["scale_updates"] for r in first]
    print(ups, [r["info"]["iter"] for r in first], [r["info"]["scale"] for r in first])
    assert sum(u == 0 for u in ups) >= 4
    if some_update:
        assert sum(u >= 1 for u in ups) >= 1
    with Work(amd, prob, cg_tol_override=tol, **FIXED) as w:
        rc, fixed = w.family(B, Cc)
    assert rc == 0
    for k in range(8):
        assert _same_bits_and_info(first[k], again[k]), k
        assert _same_bits_and_info(first[perm[k]], moved[k]) and first[perm[k]]["info"]["scale"] == moved[k]["info"]["scale"], k
        if ups[k] == 0:
            assert _same_bits_and_info(first[k], fixed[k]), k
        else:
            assert first[k]["info"]["scale"] != fixed[k]["info"]["scale"] and not _same_bits(first[k], fixed[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the workspace is untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_workspace_own_solves_return_the_same_bits_after_a_scaled_call(base):
    """adaptive workspace (exact CG: the scales of this family change within 300 iterations then; under the default schedule they
    change later): scs_solve carries its adapted scale to the next scs_solve, so the sequence solve, solve is compared with solve,
    scaled family call (in which scales change), solve on a second workspace.  Fixed-scale workspace: scs_solve and
    scs_amd_solve_family before and after a sweep at other scales."""
    amd = capi.load("libscsamd.so")
    pr, prob = base
    B, Cc = _family(base, 1, K=3)
    kw = dict(ADAPT, max_iters=300)
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as w:
        plain = [w.solve(), w.solve(B[:, 1], Cc[:, 1])]
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as w:
        first = w.solve()
        rc, fam = scaled(w, B, Cc, scales=[0.1] * 3)  # NULL would be the workspace's scale, which the solve above has adapted
        second = w.solve(B[:, 1], Cc[:, 1])
    assert rc == 0 and any(r["info"]["scale_updates"] >= 1 for r in fam)
    assert plain[0]["info"]["scale_updates"] >= 1 and plain[0]["info"]["scale"] != 0.1  # the carried scale is not the initial one
    assert _same_bits_and_info(plain[0], first) and _same_bits_and_info(plain[1], second)
    assert plain[1]["info"]["scale"] == second["info"]["scale"] and plain[1]["info"]["scale_updates"] == second["info"]["scale_updates"]
    kw = dict(FIXED, max_iters=300)
    with Work(amd, prob, **kw) as w:
        before, (_, fbefore) = w.solve(), w.family(B, Cc)
        rc, _ = scaled(w, B, Cc, scales=[0.02, 1.0, 5.0])
        after, (_, fafter) = w.solve(), w.family(B, Cc)
    assert rc == 0 and before["info"]["iter"] > 25
    assert _same_bits_and_info(before, after) and before["info"]["scale"] == after["info"]["scale"] == 0.1
    assert all(_same_bits_and_info(a, b) and b["info"]["scale"] == 0.1 for a, b in zip(fbefore, fafter))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. chunks and edges
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    pr, prob = _socp(60, 150, 5, 3)
    B, Cc = family_data(pr["A"], pr["cone"], 17, seed=8, b_scale=[10.0] * 17)
    return pr, prob, B, Cc


def test_seventeen_problems_are_two_chunks_with_their_own_scales_and_one_problem_works(small):
    """17 = 16 + 1: the second chunk is one problem at width 2 and must read ITS scale.  Chunk for chunk the bits of the same call on
    the chunk alone; the single problem also against the project's own exact-CG solve on a fresh workspace of that scale."""
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    scales = np.array([0.05 * (1 + k % 5) for k in range(16)] + [1.0])  # at 1.0 the last problem updates its scale once (to 0.094)
    kw = dict(ADAPT, max_iters=2000)
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as w:
        rc, all17 = scaled(w, B, Cc, scales=scales)
        rc2, head = scaled(w, B[:, :16], Cc[:, :16], scales=scales[:16])
        rc3, one = scaled(w, B[:, 16:], Cc[:, 16:], scales=scales[16:])
    assert rc == 0 and rc2 == 0 and rc3 == 0
    print([(r["info"]["iter"], r["info"]["scale_updates"]) for r in all17])
    assert all(r["info"]["status_val"] == 1 for r in all17)
    for k in range(16):
        assert _same_bits_and_info(all17[k], head[k]) and all17[k]["info"]["scale"] == head[k]["info"]["scale"], k
    assert _same_bits_and_info(all17[16], one[0]) and one[0]["info"]["scale_updates"] >= 1
    single = _fresh_columns(amd, prob, B[:, 16:], Cc[:, 16:], cg_tol_override=1e-12, scales=scales[16:], **kw)
    _assert_same_as(one, single)


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
    scales = np.array([0.05, 0.1, 0.4])
    with Work(amd, prob, max_iters=2000, **ADAPT) as w:
        assert amd.scs_amd_solve_family_scaled(w.w, K, Bp.ctypes.data_as(T.fp), ldb, Cp.ctypes.data_as(T.fp), ldc,
                                               scales.ctypes.data_as(T.fp), sols, infos, 0) == 0
        rc, want = scaled(w, B[:, :K], Cc[:, :K], scales=scales)
    for k in range(K):
        assert infos[k].status_val == 1 and infos[k].iter == want[k]["info"]["iter"] and infos[k].scale == want[k]["info"]["scale"]
        assert np.array_equal(X[:, k], want[k]["x"]) and np.array_equal(Y[:, k], want[k]["y"]) and np.array_equal(S[:, k], want[k]["s"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. mixed cones, adaptive
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mixed_cones_adaptive_against_the_single_solve_on_fresh_workspaces():
    """the zero cone (the 1 / (1000 scale) rows of diag_r), the nonnegative cone, two second-order cones and a PSD block in one
    family, every column adapting its own scale: exact CG, against the project's own scs_update + scs_solve on a fresh workspace per
    column"""
    amd = capi.load("libscsamd.so")
    prob, A, cone, B, Cc = _mixed()
    B, Cc = np.asfortranarray(B[:, 2:]), np.asfortranarray(Cc[:, 2:])
    kw = dict(ADAPT, max_iters=5000)
    single = _fresh_columns(amd, prob, B, Cc, cg_tol_override=1e-12, **kw)
    with Work(amd, prob, cg_tol_override=1e-12, **kw) as w:
        rc, fam = scaled(w, B, Cc)
    assert rc == 0 and all(r["info"]["status_val"] == 1 for r in single)
    _assert_same_as(fam, single)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals and bad scales
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,word", [(dict(acceleration_lookback=10), b"acceleration_lookback"), (dict(log_csv_filename=True), b"log_csv_filename")])
def test_refused_settings_return_scs_failed_and_leave_the_outputs_alone(small, over, word, tmp_path):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    if "log_csv_filename" in over:
        over = dict(log_csv_filename=str(tmp_path / "log.csv").encode())
    kw = dict(ADAPT, max_iters=50)
    kw.update(over)
    marks = tuple(np.full((r, 2), 7.0, order="F") for r in (prob.n, prob.m, prob.m))
    with Work(amd, prob, **kw) as w:
        assert word in amd.scs_amd_solve_family_scaled_refusal(w.w)
        rc, out = scaled(w, B[:, :2], Cc[:, :2], warm=marks, warm_start=0)
        assert rc == SCS_FAILED
        assert all(np.all(r[v] == 7.0) for r in out for v in ("x", "y", "s")) and all(r["info"]["iter"] == 0 for r in out)
        assert w.solve()["info"]["iter"] > 0  # a following scs_solve works


@pytest.mark.parametrize("bad", [0.0, -0.1, float("nan"), float("inf")])
def test_a_scale_that_is_not_positive_and_finite_returns_scs_failed_and_leaves_the_outputs_alone(small, bad):
    amd = capi.load("libscsamd.so")
    pr, prob, B, Cc = small
    marks = tuple(np.full((r, 2), 7.0, order="F") for r in (prob.n, prob.m, prob.m))
    with Work(amd, prob, max_iters=50, **ADAPT) as w:
        assert amd.scs_amd_solve_family_scaled_refusal(w.w) is None  # adaptive_scale is served
        rc, out = scaled(w, B[:, :2], Cc[:, :2], scales=[0.1, bad], warm=marks, warm_start=0)
        assert rc == SCS_FAILED
        assert all(np.all(r[v] == 7.0) for r in out for v in ("x", "y", "s")) and all(r["info"]["iter"] == 0 for r in out)
        assert w.solve()["info"]["iter"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the other builds
# ---------------------------------------------------------------------------------------------------------------------------------
def test_f32_adaptive_family_against_its_own_single_solves(base):
    """the loose fp32 bounds of tests/test_family_gpu.py::test_f32_family_against_its_own_single_solves: eps = 1e-3, same status,
    objectives within 1e-2 of their scale; the single solves on a fresh workspace each"""
    lib = capi.load("libscsamd_f32.so")
    pr, _ = base
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=lib._scs_types)
    B, Cc = _family(base, 10, K=4)
    kw = dict(ADAPT, eps_abs=1e-3, eps_rel=1e-3)
    single = _fresh_columns(lib, prob, B, Cc, **kw)
    with Work(lib, prob, **kw) as w:
        rc, fam = scaled(w, B, Cc, scales=[0.01, 0.1, 0.1, 1.0])
    assert rc == 0
    for k, (a, b) in enumerate(zip(fam, single)):
        assert a["x"].dtype == np.float32
        assert a["info"]["status_val"] == b["info"]["status_val"] == 1, k
        sc = max(1.0, abs(b["info"]["pobj"]))
        assert abs(a["info"]["pobj"] - b["info"]["pobj"]) <= 1e-2 * sc and abs(a["info"]["dobj"] - b["info"]["dobj"]) <= 1e-2 * sc, k


def test_dlong_adaptive_family_equals_the_32_bit_library(base):
    l32, l64 = capi.load("libscsamd.so"), capi.load("libscsamd_dlong.so")
    pr, prob32 = base
    B, Cc = _family(base, 1, K=4)
    prob64 = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"], T=l64._scs_types)
    with Work(l64, prob64, cg_tol_override=1e-12, **ADAPT) as w:
        rc, f64 = scaled(w, B, Cc)
    with Work(l32, prob32, cg_tol_override=1e-12, **ADAPT) as w:
        rc2, f32 = scaled(w, B, Cc)
    assert rc == 0 and rc2 == 0 and any(r["info"]["scale_updates"] >= 1 for r in f32)
    for k in range(4):
        assert _same_bits_and_info(f64[k], f32[k]), k
        assert f64[k]["info"]["scale"] == f32[k]["info"]["scale"] and f64[k]["info"]["scale_updates"] == f32[k]["info"]["scale_updates"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. the Python object
# ---------------------------------------------------------------------------------------------------------------------------------
def test_python_solve_family_with_own_scales(base):
    from scs_amd.solver import SCS
    amd = capi.load("libscsamd.so")
    pr, prob = base
    B, Cc = _family(base, 10, K=3)
    data = dict(A=pr["A"], b=pr["b"], c=pr["c"])
    scales = [0.02, 0.1, 1.0]
    with Work(amd, prob, **ADAPT) as w:
        rc, want = scaled(w, B, Cc)
        rc2, want_s = scaled(w, B, Cc, scales=scales)
    assert rc == 0 and rc2 == 0
    with SCS(data, pr["cone"], adaptive_scale=1, acceleration_lookback=0) as s:
        got = s.solve_family(B, Cc, own_scale=True)
        got_s = s.solve_family(B, Cc, scale=scales)
        with pytest.raises(ValueError):
            s.solve_family(B, Cc, scale=scales[:2])
        with pytest.raises(ValueError, match="adaptive_scale"):
            s.solve_family(B, Cc)  # without the keywords: the shared-scale entry, refusal included
    for k in range(3):
        assert got[k]["info"]["status"] == "solved"
        assert _same_bits_and_info(got[k], want[k]) and _same_bits_and_info(got_s[k], want_s[k]), k
        assert got_s[k]["info"]["scale"] == want_s[k]["info"]["scale"] and got_s[k]["info"]["scale_updates"] == want_s[k]["info"]["scale_updates"]
    assert not _same_bits(got_s[0], got[0])  # the initial scales are used
