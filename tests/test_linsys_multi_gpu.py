"""Blocks of right-hand sides on one linear-system workspace (include/scs_amd.h, B1: scs_amd_solve_lin_sys_multi and the block
operator pieces scs_amd_linsys_{mat_vec,mul_a,mul_at}_multi_dev; kernels in scs_amd/csrc/spmm.h and linsys_multi.h).

 1. the block products against an exact product, on the edge shapes of tests/spmv_exact.py, every width, three builds;
 2. every column of a block solve against the reference backend (linsys/cpu/indirect/private.c:284-324) and against this library's
    scs_solve_lin_sys on that column, with the assertions tests/test_linsys_gpu.py makes for one vector;
 3. independence: a column's bits and its iteration count do not depend on its neighbours or on its position in the block;
 4. per-column control: zero short-circuit, converged warm start, a loose and a tight tolerance in one block; statistics;
 5. iteration counts against the single-vector path;
 6. the boundary of the interface: one column, 17 columns, leading dimensions, diag_r update, bad arguments, leaks, HIP failures;
 7. the Python object scs_amd.linsys.LinSys.
The yardstick of every comparison is the reference backend or the single-vector path, never the block path's own earlier output."""
import ctypes as C
import zlib

import numpy as np
import pytest

from scs_amd import capi
from tests import probgen
from tests import spmv_exact as sx
# device buffers through the HIP runtime the library links, the workspace wrapper and the shape / P pairing of the single-vector suite
from tests.test_spmv_exact_gpu import GUARD, LIBS, SHAPES, Workspace, _load, _pattern
from tests import test_spmv_exact_gpu as single_suite

pytestmark = pytest.mark.gpu

NRHS = (2, 3, 4, 5, 8, 11, 16)


def _hip():
    return single_suite._hip


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact block products
# ---------------------------------------------------------------------------------------------------------------------------------
def _apply_block(ws, op, cols):
    """op on the block whose columns are `cols` (list of vectors): NaN sentinels as in the single-vector suite; two calls, same bits.
    Returns the (out_len, nrhs) result."""
    L, dt = ws.L, ws.dtype
    nrhs = len(cols)
    W = L.scs_amd_linsys_multi_width(nrhs)
    assert W >= nrhs and W in (2, 4, 8, 16)
    fn, out_len = {"mul_a": (L.scs_amd_linsys_mul_a_multi_dev, ws.ops.m), "mul_at": (L.scs_amd_linsys_mul_at_multi_dev, ws.ops.n),
                   "mat_vec": (L.scs_amd_linsys_mat_vec_multi_dev, ws.ops.n)}[op]
    in_len = len(cols[0])
    X = np.zeros((in_len, W), dt)  # row-major block, padding columns zero
    for k, c in enumerate(cols):
        X[:, k] = c.astype(dt)
    inp = np.concatenate([X.ravel(), np.full(GUARD, np.nan, dt)])  # the input's guard: same allocation, right behind the block
    nan_out = np.full(out_len * W + GUARD, np.nan, dt)              # padding columns included in the fill
    hip = _hip()
    din, dout = hip.malloc(inp.nbytes), hip.malloc(nan_out.nbytes)
    try:
        hip.put(din, inp)
        res = []
        for _ in range(2):
            hip.put(dout, nan_out)
            hip.sync()
            assert fn(ws.w, nrhs, din, dout) == 0
            assert L.scs_amd_linsys_sync(ws.w) == 0
            got = np.empty(out_len * W + GUARD, dt)
            hip.get(got, dout)
            res.append(got)
    finally:
        hip.free(din)
        hip.free(dout)
    ib = np.uint64 if np.dtype(dt).itemsize == 8 else np.uint32
    blocks = []
    for got in res:
        assert np.array_equal(got[out_len * W:].view(ib), nan_out[out_len * W:].view(ib)), f"{op}: the guard behind the output was written"
        Y = got[:out_len * W].reshape(out_len, W)[:, :nrhs]
        bad = np.argwhere(~np.isfinite(Y))
        assert bad.size == 0, f"{op}: {len(bad)} elements not written or gathered past the input's end (NaN), first (row, column) {bad[:5].tolist()}"
        blocks.append(Y)
    assert np.array_equal(blocks[0].view(ib), blocks[1].view(ib)), f"{op}: a second call gave different bits"
    return blocks[0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lib", ["f64", "f32", "dlong"])
def test_block_products_exact_and_bounded(lib, shape):
    L = _load(lib)
    dtype = LIBS[lib][1]
    A_pat, P_pat = _pattern(shape)
    m, n = A_pat.shape
    rng = np.random.default_rng(zlib.crc32(f"multi-{lib}-{shape}".encode()))
    x_hi = 7 if dtype is np.float64 else 3  # the amplitudes of sx.exact_problem
    # (a) integer data, a different integer vector per column; no column may go vacuous
    ops, x0, y0 = sx.exact_problem(A_pat, P_pat, rng, dtype)
    xs = [x0] + [sx.int_values(n, rng, 1, x_hi) for _ in range(15)]
    ys = [y0] + [sx.int_values(m, rng, 1, x_hi) for _ in range(15)]
    refs = []
    for xk, yk in zip(xs, ys):
        bits, K = ops.exact_bits_needed(xk, yk)
        assert bits < sx.PREC_BITS[dtype], f"column needs {bits:.1f} bits (K = {K})"
        refs.append(ops.exact(xk, yk))
    ws = Workspace(L, ops, dtype)
    try:
        for nrhs in NRHS:
            for op, src, ri, what in (("mul_a", xs, 0, "A x"), ("mul_at", ys, 1, "A' y"), ("mat_vec", xs, 2, "R_x x + P x + A' R_y^-1 A x")):
                Y = _apply_block(ws, op, src[:nrhs])
                for k in range(nrhs):
                    sx.check_exact(np.ascontiguousarray(Y[:, k]), refs[k][ri], dtype, f"{what}, nrhs {nrhs}, column {k}")
    finally:
        ws.free()
    # (b) real data: every column within the rounding bound of the long-double product
    ops, x0, y0 = sx.cast(*sx.real_problem(A_pat, P_pat, rng), dtype)
    spread = lambda k: (rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-8, 8, k)).astype(dtype).astype(np.float64)
    xs = [x0] + [spread(n) for _ in range(15)]
    ys = [y0] + [spread(m) for _ in range(15)]
    lds = [ops.longdouble(xk, yk) for xk, yk in zip(xs, ys)]
    bnd = [ops.bounds(xk, yk, sx.UNIT_ROUNDOFF[dtype]) for xk, yk in zip(xs, ys)]
    ws = Workspace(L, ops, dtype)
    try:
        for nrhs in NRHS:
            for op, src, ri, what in (("mul_a", xs, 0, "A x"), ("mul_at", ys, 1, "A' y"), ("mat_vec", xs, 2, "R_x x + P x + A' R_y^-1 A x")):
                Y = _apply_block(ws, op, src[:nrhs])
                for k in range(nrhs):
                    sx.check_bound(Y[:, k], lds[k][ri], bnd[k][ri], f"{what}, nrhs {nrhs}, column {k}")
    finally:
        ws.free()


def test_block_product_entries_refuse_bad_widths():
    L = _load("f64")
    A_pat, P_pat = _pattern("1x1")
    ops, x, y = sx.exact_problem(A_pat, P_pat, np.random.default_rng(0), np.float64)
    ws = Workspace(L, ops, np.float64)
    hip = _hip()
    d = hip.malloc(64 * 8)
    try:
        for fn in (L.scs_amd_linsys_mat_vec_multi_dev, L.scs_amd_linsys_mul_a_multi_dev, L.scs_amd_linsys_mul_at_multi_dev):
            assert fn(ws.w, 0, d, d) == -1 and fn(ws.w, 17, d, d) == -1 and fn(ws.w, 2, None, d) == -1
    finally:
        hip.free(d)
        ws.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# solves
# ---------------------------------------------------------------------------------------------------------------------------------
def _ref():
    from oracle import pyoracle
    if not pyoracle.ref_available():
        pytest.skip("oracle/_ref not built (needs the reference tree at build time)")
    return pyoracle.load_ref()


def _init(lib, prob, dr, with_P=False):
    T = lib._scs_types
    w = lib.scs_init_lin_sys_work(C.byref(prob.matA), C.byref(prob.matP) if with_P else None, dr.ctypes.data_as(T.fp))
    assert w
    return w


def _single(lib, w, b, s, tol):
    T = lib._scs_types
    out = b.copy()
    assert lib.scs_solve_lin_sys(w, out.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp) if s is not None else None, tol) == 0
    return out


def _stats(lib, w):
    st = lib._scs_types.ScsAmdStats()
    lib.scs_amd_linsys_get_stats(w, C.byref(st))
    return st.cg_iters, st.lin_sys_solves, st.mat_vecs


def _single_counted(lib, w, b, s, tol):
    before = _stats(lib, w)[0]
    out = _single(lib, w, b, s, tol)
    return out, _stats(lib, w)[0] - before


def _multi(lib, w, B, S, tol, ldb=None, lds=None, expect=0):
    """scs_amd_solve_lin_sys_multi on copies: B (n + m, K), S (n, K) or None, tol scalar or K.  Returns (XY, iters)."""
    T = lib._scs_types
    nm, K = B.shape
    ldb = ldb or nm
    buf = np.full((K, ldb), np.nan)  # row k of this C array = column k of the column-major block, gap NaN-filled
    buf[:, :nm] = B.T
    sb = None
    if S is not None:
        lds = lds or S.shape[0]
        sb = np.full((K, lds), np.nan)
        sb[:, :S.shape[0]] = S.T
    tv = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (K,)))
    it = np.full(K, -7, dtype=T.np_int)
    rc = lib.scs_amd_solve_lin_sys_multi(w, K, buf.ctypes.data_as(T.fp), ldb, sb.ctypes.data_as(T.fp) if sb is not None else None,
                                         lds or 0, tv.ctypes.data_as(T.fp), it.ctypes.data_as(T.ip))
    assert rc == expect
    if ldb > nm:
        assert np.all(np.isnan(buf[:, nm:])), "the gap behind a column of B was written"
    if sb is not None:
        want = np.full_like(sb, np.nan)
        want[:, :S.shape[0]] = S.T
        assert np.array_equal(sb, want, equal_nan=True), "S was modified"
    return np.ascontiguousarray(buf[:, :nm].T), it.astype(np.int64)


def _check_column(Asp, Psp, dr, n, b, xa, tol, xr=None, xs=None, what=""):
    """the assertions of test_solve_lin_sys_matches_reference on one solution xa = [x; y] of right-hand side b, bounds unchanged;
    xr: the reference backend's solution, xs: scs_solve_lin_sys of this library on the same column"""
    for other, name in ((xr, "reference"), (xs, "single-vector path")):
        if other is not None and tol <= 1e-9:
            assert np.abs(xa - other).max() <= 1e-7 * np.abs(other).max(), f"{what}: differs from the {name}"
    x, y = xa[:n], xa[n:]
    r1 = dr[:n] * x + Asp.T @ y - b[:n]
    if Psp is not None:
        r1 = r1 + Psp @ x
    r2 = Asp @ x - dr[n:] * y - b[n:]
    red = r1 + Asp.T @ (r2 / dr[n:])
    assert np.abs(red).max() < max(tol, 1e-12) * 1.01 + 1e-10 * np.abs(b).max(), f"{what}: reduced KKT residual"
    assert np.abs(r2).max() < 1e-9 * max(1.0, np.abs(b).max()) * dr[n:].max(), f"{what}: second residual"


CASES = [
    (50, 150, 4, False, 1e-12),
    (1000, 3000, 32, False, 1e-12),
    (1000, 3000, 32, True, 1e-7),
    (3000, 7001, 9, True, 1e-4),
    (20000, 50000, 10, False, 1e-9),
]


def _case_data(n, m, col_nnz, warm, K):
    """generators, diag_r and seeds of test_solve_lin_sys_matches_reference; column 0 is that test's own right-hand side"""
    rng = np.random.default_rng(n + m)
    A = probgen.random_csc(m, n, col_nnz, seed=7)
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m))
    dr = probgen.diag_r(n, m, z=m // 10)
    B = np.empty((n + m, K))
    S = np.empty((n, K)) if warm else None
    for k in range(K):
        B[:, k] = rng.uniform(-1, 1, n + m)
        if warm:
            S[:, k] = rng.uniform(-1, 1, n) * 0.1
    return prob, dr, B, S


@pytest.mark.parametrize("n,m,col_nnz,warm,tol", CASES)
def test_columns_match_reference_and_single_vector_path(n, m, col_nnz, warm, tol):
    ref = _ref()
    amd = capi.load("libscsamd_linsys.so")
    K = 5
    prob, dr, B, S = _case_data(n, m, col_nnz, warm, K)
    Asp = prob.sparse()
    wa, wr = _init(amd, prob, dr), _init(ref, prob, dr)
    try:
        XY, iters = _multi(amd, wa, B, S, tol)
        assert np.all(iters >= 0)
        for k in range(K):
            s = S[:, k].copy() if warm else None
            xr = _single(ref, wr, B[:, k].copy(), s, tol)
            xs = _single(amd, wa, B[:, k].copy(), s, tol)
            _check_column(Asp, None, dr, n, B[:, k], XY[:, k], tol, xr, xs, f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(wa)
        ref.scs_free_lin_sys_work(wr)


def _p_case():
    import scipy.sparse as sp
    n, m = 300, 500
    rng = np.random.default_rng(3)
    A = probgen.random_csc(m, n, 5, seed=11)
    Bm = sp.random(n, n, density=0.02, random_state=5, format="csc")
    P = (Bm @ Bm.T + sp.identity(n) * 0.1).tocsc()
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), P=P)
    dr = probgen.diag_r(n, m, z=50)
    K = 5
    B = np.empty((n + m, K))
    S = np.empty((n, K))
    for k in range(K):
        B[:, k] = rng.uniform(-1, 1, n + m)
        S[:, k] = rng.uniform(-1, 1, n)
    return prob, P, dr, B, S


def test_columns_with_P_match_reference():
    ref = _ref()
    amd = capi.load("libscsamd_linsys.so")
    prob, P, dr, B, S = _p_case()
    n = prob.n
    wa, wr = _init(amd, prob, dr, True), _init(ref, prob, dr, True)
    try:
        XY, iters = _multi(amd, wa, B, S, 1e-12)
        for k in range(B.shape[1]):
            xr = _single(ref, wr, B[:, k].copy(), S[:, k].copy(), 1e-12)
            xs = _single(amd, wa, B[:, k].copy(), S[:, k].copy(), 1e-12)
            assert np.abs(XY[:, k] - xr).max() <= 1e-8 * np.abs(xr).max()  # the bound of test_with_P_matches_reference
            _check_column(prob.sparse(), P, dr, n, B[:, k], XY[:, k], 1e-12, xr, xs, f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(wa)
        ref.scs_free_lin_sys_work(wr)


# ---- 3. independence ----
@pytest.mark.parametrize("warm", [False, True])
def test_a_column_does_not_depend_on_its_neighbours(warm):
    amd = capi.load("libscsamd_linsys.so")
    n, m, K = 3000, 7001, 5
    prob, dr, B, S = _case_data(n, m, 9, True, K)
    if not warm:
        S = None
    w = _init(amd, prob, dr)
    try:
        tol = 1e-9
        XY, iters = _multi(amd, w, B, S, tol)
        other = np.random.default_rng(99)
        for j in (0, K // 2, K - 1):
            B2 = other.uniform(-3, 3, B.shape)
            S2 = other.uniform(-1, 1, S.shape) if warm else None
            tols = np.full(K, tol)
            rest = [k for k in range(K) if k != j]
            B2[:, rest[0]] = 0.0          # one neighbour all zero
            tols[rest[1]] = 1e-3          # one neighbour at a loose tolerance
            B2[:, j] = B[:, j]
            if warm:
                S2[:, j] = S[:, j]
            XY2, it2 = _multi(amd, w, B2, S2, tols)
            assert np.array_equal(XY2[:, j].view(np.uint64), XY[:, j].view(np.uint64)), f"column {j} changed with its neighbours"
            assert it2[j] == iters[j]
            assert np.all(XY2[:, rest[0]] == 0.0) and it2[rest[0]] == 0
            # the same column at another position of a block of the same width (K = 5 and K = 8 both have width 8)
            K8 = 8
            B8 = other.uniform(-1, 1, (n + m, K8))
            S8 = other.uniform(-1, 1, (n, K8)) * 0.1 if warm else None
            pos = (j + 3) % K8
            B8[:, pos] = B[:, j]
            if warm:
                S8[:, pos] = S[:, j]
            XY8, it8 = _multi(amd, w, B8, S8, tol)
            assert np.array_equal(XY8[:, pos].view(np.uint64), XY[:, j].view(np.uint64)), f"column {j} changed with its position"
            assert it8[pos] == iters[j]
        # another width: the reduction trees differ, the bounds of item 2 apply
        Asp = prob.sparse()
        for K2 in (2, 16):
            Bw = other.uniform(-1, 1, (n + m, K2))
            Sw = other.uniform(-1, 1, (n, K2)) * 0.1 if warm else None
            Bw[:, K2 - 1] = B[:, 0]
            if warm:
                Sw[:, K2 - 1] = S[:, 0]
            XYw, _ = _multi(amd, w, Bw, Sw, tol)
            _check_column(Asp, None, dr, n, B[:, 0], XYw[:, K2 - 1], tol, None, XY[:, 0], f"width of {K2} columns")
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 4. per-column control ----
def test_per_column_control_and_statistics():
    amd = capi.load("libscsamd_linsys.so")
    n, m = 3000, 7001
    prob, dr, B, _ = _case_data(n, m, 9, False, 4)
    Asp = prob.sparse()
    w = _init(amd, prob, dr)
    try:
        ZERO, WARM, LOOSE, TIGHT = 0, 1, 2, 3
        B[:, ZERO] = 1e-13  # |b|_inf <= 1e-12: private.c:296-299
        conv = _single(amd, w, B[:, WARM].copy(), None, 1e-12)
        S = np.zeros((n, 4))  # the columns that are not warm-started carry a zero warm start
        S[:, WARM] = conv[:n]
        tols = np.array([1e-9, 1e-6, 1e-3, 1e-12])
        before = _stats(amd, w)
        XY, iters = _multi(amd, w, B, S, tols)
        after = _stats(amd, w)
        assert np.all(XY[:, ZERO] == 0.0) and iters[ZERO] == 0
        assert iters[WARM] == 0 and np.array_equal(XY[:n, WARM], S[:, WARM])
        assert 0 < iters[LOOSE] < iters[TIGHT]
        for k in (WARM, LOOSE, TIGHT):
            _check_column(Asp, None, dr, n, B[:, k], XY[:, k], tols[k], None, None, f"column {k}")
        assert after[0] - before[0] == iters.sum()        # cg_iters: every column's iterations
        assert after[1] - before[1] == 4                  # lin_sys_solves: one per column
        assert after[2] - before[2] == iters.max() + 1    # mat_vecs: a block product counts once (+ 1 for G s of the warm start)
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 5. iteration counts against the single-vector path ----
# Both paths run the same recurrence with differently ordered sums.  These systems are ill conditioned (R_x = 1e-6: 55 to 1089
# iterations), so the rounding of the sums moves the count: the largest difference measured over these cases on an MI355X (every
# column, both tolerances; table in profiles/multi_rhs.md) is 27 iterations, at 963 of the single-vector path (2.8 %), with no sign
# preference.  The assertion is twice that, at least 2 (the stop test can fall either side of tol on one iteration, on either path).
ITERS_MEASURED = 27
ITERS_BOUND = max(2, 2 * ITERS_MEASURED)


@pytest.mark.parametrize("tol", [1e-4, 1e-7])
@pytest.mark.parametrize("case", range(len(CASES) + 1))
def test_iteration_counts_against_single_vector_path(case, tol):
    amd = capi.load("libscsamd_linsys.so")
    if case < len(CASES):
        n, m, col_nnz, warm, _ = CASES[case]
        prob, dr, B, S = _case_data(n, m, col_nnz, warm, 5)
        with_P = False
    else:
        prob, _, dr, B, S = _p_case()
        with_P = True
    w = _init(amd, prob, dr, with_P)
    try:
        _, iters = _multi(amd, w, B, S, tol)
        single = []
        for k in range(B.shape[1]):
            _, its = _single_counted(amd, w, B[:, k].copy(), S[:, k].copy() if S is not None else None, tol)
            single.append(its)
        diff = np.abs(iters - np.array(single))
        print(f"iteration counts case {case} tol {tol:g}: block {iters.tolist()} single {single} largest difference {diff.max()}")
        assert diff.max() <= ITERS_BOUND
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 6. boundary of the interface ----
def test_one_column_is_the_single_vector_path_bit_for_bit():
    amd = capi.load("libscsamd_linsys.so")
    for n, m, col_nnz, warm in ((50, 150, 4, False), (3000, 7001, 9, True), (20000, 50000, 10, True)):
        prob, dr, B, S = _case_data(n, m, col_nnz, warm, 1)
        w = _init(amd, prob, dr)
        try:
            xs, its = _single_counted(amd, w, B[:, 0].copy(), S[:, 0].copy() if warm else None, 1e-9)
            XY, iters = _multi(amd, w, B, S, 1e-9)
            assert np.array_equal(XY[:, 0].view(np.uint64), xs.view(np.uint64)) and iters[0] == its
        finally:
            amd.scs_free_lin_sys_work(w)


def test_seventeen_columns_in_two_chunks():
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 3000, 7001, 1e-9
    prob, dr, B, S = _case_data(n, m, 9, True, 17)
    Asp = prob.sparse()
    w = _init(amd, prob, dr)
    try:
        XY, iters = _multi(amd, w, B, S, tol)
        for k in range(17):
            xs = _single(amd, w, B[:, k].copy(), S[:, k].copy(), tol)
            _check_column(Asp, None, dr, n, B[:, k], XY[:, k], tol, None, xs, f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


def test_leading_dimensions_leave_the_gap_untouched():
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 1000, 3000, 1e-9
    prob, dr, B, S = _case_data(n, m, 32, True, 3)
    w = _init(amd, prob, dr)
    try:
        tight, it_t = _multi(amd, w, B, S, tol)
        wide, it_w = _multi(amd, w, B, S, tol, ldb=n + m + 13, lds=n + 5)  # _multi asserts the NaN-filled gaps are still NaN
        assert np.array_equal(tight.view(np.uint64), wide.view(np.uint64)) and np.array_equal(it_t, it_w)
    finally:
        amd.scs_free_lin_sys_work(w)


def test_diag_r_update_between_block_solves():
    ref = _ref()
    amd = capi.load("libscsamd_linsys.so")
    n, m, K = 1000, 3000, 4
    prob, dr, B, _ = _case_data(n, m, 32, False, K)
    Asp = prob.sparse()
    wa, wr = _init(amd, prob, dr), _init(ref, prob, dr)
    try:
        _multi(amd, wa, B, None, 1e-12)
        dr2 = probgen.diag_r(n, m, z=m // 10, scale=2.5)
        assert amd.scs_update_lin_sys_diag_r(wa, dr2.ctypes.data_as(capi.T64.fp)) == 0
        assert ref.scs_update_lin_sys_diag_r(wr, dr2.ctypes.data_as(capi.T64.fp)) == 0
        XY, _ = _multi(amd, wa, B, None, 1e-12)
        for k in range(K):
            xr = _single(ref, wr, B[:, k].copy(), None, 1e-12)
            _check_column(Asp, None, dr2, n, B[:, k], XY[:, k], 1e-12, xr, None, f"column {k} on the new diag_r")
    finally:
        amd.scs_free_lin_sys_work(wa)
        ref.scs_free_lin_sys_work(wr)


def test_bad_arguments_are_refused_and_the_workspace_stays_usable():
    amd = capi.load("libscsamd_linsys.so")
    T = amd._scs_types
    n, m = 50, 150
    prob, dr, B, S = _case_data(n, m, 4, True, 3)
    w = _init(amd, prob, dr)
    try:
        buf = np.asfortranarray(B)
        sb = np.asfortranarray(S)
        tv = np.full(3, 1e-9)
        it = np.zeros(3, dtype=T.np_int)
        fp = lambda a: a.ctypes.data_as(T.fp)
        call = lambda nrhs, Bp, ldb, Sp, lds, tp: amd.scs_amd_solve_lin_sys_multi(w, nrhs, Bp, ldb, Sp, lds, tp, it.ctypes.data_as(T.ip))
        assert call(0, fp(buf), n + m, None, 0, fp(tv)) == -1
        assert call(3, fp(buf), n + m - 1, None, 0, fp(tv)) == -1
        assert call(3, fp(buf), n + m, fp(sb), n - 1, fp(tv)) == -1
        assert call(3, fp(buf), n + m, None, 0, None) == -1
        assert call(3, None, n + m, None, 0, fp(tv)) == -1
        assert np.array_equal(buf, B)  # nothing was touched
        XY, _ = _multi(amd, w, B, S, 1e-9)
        Asp = prob.sparse()
        for k in range(3):
            _check_column(Asp, None, dr, n, B[:, k], XY[:, k], 1e-9, None, _single(amd, w, B[:, k].copy(), S[:, k].copy(), 1e-9), f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


def _free_bytes(lib):
    v = lib.scs_amd_device_free_bytes()
    assert v >= 0
    return v


def test_block_buffers_are_freed_with_the_workspace():
    """the "nothing leaked" check of tests/test_fault_injection_gpu.py (same allowance for the runtime's own caches); the block
    buffers of this system at width 16 hold about 40 MB"""
    amd = capi.load("libscsamd_linsys.so")
    n, m = 30000, 60000
    prob, dr, B, S = _case_data(n, m, 10, True, 16)
    w = _init(amd, prob, dr)  # warm: context, streams, code objects
    _multi(amd, w, B[:, :2], S[:, :2], 1e-6)
    amd.scs_free_lin_sys_work(w)
    base = _free_bytes(amd)
    w = _init(amd, prob, dr)
    _multi(amd, w, B[:, :3], S[:, :3], 1e-6)  # width 4 first, then the buffers grow to width 16
    _multi(amd, w, B, S, 1e-6)
    held = base - _free_bytes(amd)
    assert held > (7 * n + 2 * m) * 16 * 8 * 0.9
    amd.scs_free_lin_sys_work(w)
    assert abs(_free_bytes(amd) - base) <= 8 << 20


def test_hip_failure_inside_a_block_solve():
    """scs_amd_test_fail_at reports a successful runtime call as failed (it faults nothing): the call returns -1 and the next block
    solve on a new workspace is right"""
    amd = capi.load("libscsamd_linsys.so")
    n, m, K, tol = 3000, 7001, 5, 1e-9
    prob, dr, B, S = _case_data(n, m, 9, True, K)
    Asp = prob.sparse()
    w = _init(amd, prob, dr)
    _multi(amd, w, B, S, tol)  # allocates the block buffers and sizes the batches of enqueued iterations for the next call
    big = 10 ** 12
    amd.scs_amd_test_fail_at(big)
    _multi(amd, w, B, S, tol)
    total = big - amd.scs_amd_test_fail_at(0)  # checked runtime calls of one block solve: copies, control-record reads, synchronisations
    assert total > 5
    for k in sorted({1, 2, 3, total // 2, total}):  # uploads, the first control-record read, the middle, the last synchronisation
        amd.scs_amd_test_fail_at(k)
        _multi(amd, w, B, S, tol, expect=-1)
        assert amd.scs_amd_test_fail_at(0) == 0, k  # consumed inside the call
    XY, _ = _multi(amd, w, B, S, tol)  # the same workspace is still usable
    amd.scs_free_lin_sys_work(w)
    w = _init(amd, prob, dr)
    try:
        XY2, _ = _multi(amd, w, B, S, tol)
        assert np.array_equal(XY.view(np.uint64), XY2.view(np.uint64))
        for k in range(K):
            _check_column(Asp, None, dr, n, B[:, k], XY2[:, k], tol, None, _single(amd, w, B[:, k].copy(), S[:, k].copy(), tol), f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


def test_dlong_build_block_solve_matches_its_single_vector_path():
    amd = capi.load("libscsamd_dlong.so")
    T = amd._scs_types
    n, m, K, tol = 3000, 7001, 3, 1e-9
    rng = np.random.default_rng(n + m)
    A = probgen.random_csc(m, n, 9, seed=7)
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), T=T)
    dr = probgen.diag_r(n, m, z=m // 10)
    B = rng.uniform(-1, 1, (n + m, K))
    w = _init(amd, prob, dr)
    try:
        XY, iters = _multi(amd, w, B, None, tol)
        for k in range(K):
            _check_column(prob.sparse(), None, dr, n, B[:, k], XY[:, k], tol, None, _single(amd, w, B[:, k].copy(), None, tol), f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 7. the Python object ----
def test_python_linsys_object():
    from scs_amd.linsys import LinSys
    amd = capi.load("libscsamd.so")  # the library the object loads
    n, m, K, tol = 1000, 3000, 3, 1e-9
    prob, dr, B, S = _case_data(n, m, 32, True, K)
    w = _init(amd, prob, dr)
    try:
        want, want_it = _multi(amd, w, B, S, tol)
    finally:
        amd.scs_free_lin_sys_work(w)
    with LinSys(prob.sparse(), dr) as ls:
        for order in ("F", "C"):
            Bo, So = np.array(B, order=order), np.array(S, order=order)
            keepB, keepS = Bo.copy(), So.copy()
            XY, iters = ls.solve_many(Bo, So, tol)
            assert np.array_equal(XY.view(np.uint64), want.view(np.uint64)) and np.array_equal(iters, want_it)
            assert np.array_equal(Bo, keepB) and np.array_equal(So, keepS)
        one, _ = ls.solve_many(B[:, :1], S[:, :1], tol)
        assert np.array_equal(ls.solve(B[:, 0], S[:, 0], tol), one[:, 0])
        with pytest.raises(ValueError):
            ls.solve_many(B[:-1], S, tol)
        dr2 = probgen.diag_r(n, m, z=m // 10, scale=2.5)
        ls.update_diag_r(dr2)
        XY2, _ = ls.solve_many(B, None, np.full(K, 1e-10))
        for k in range(K):
            _check_column(prob.sparse(), None, dr2, n, B[:, k], XY2[:, k], 1e-10, None, None, f"column {k}")
        st = ls.stats()
        assert st["lin_sys_solves"] == 2 * K + 1 + 1 + K
    with pytest.raises(RuntimeError):
        ls.solve(B[:, 0])
