"""Every column of a block under its own diag_r = [R_x,k; R_y,k] and its own Jacobi preconditioner (include/scs_amd.h:
scs_amd_solve_lin_sys_multi_r, scs_amd_linsys_mat_vec_multi_r_dev; kernels in scs_amd/csrc/spmm.h and linsys_multi.h).

 1. the block product under per-column R against an exact product and a rounding bound, edge shapes, every width, three builds;
 2. every column of a per-column solve against the reference backend after scs_update_lin_sys_diag_r(column's diag_r), and against
    this library's single-vector solve after the same update, with the bounds of tests/test_linsys_multi_gpu.py unchanged;
 3. bit identities: equal R in every column = the shared-R block solve; a column depends neither on its neighbours' R nor on its
    position; two calls agree; the workspace's own diag_r is untouched;
 4. per-column control under per-column R; 5. seventeen columns in two chunks; 6. one column; 7. refusals on a live workspace;
 8. device memory; 9. the dlong build; 10. the Python object.
The yardstick of every comparison is the reference backend, an exact product, or the existing single-vector / shared-R paths, never
the per-column path's own earlier output."""
import ctypes as C
import zlib

import numpy as np
import pytest

from scs_amd import capi
from tests import probgen
from tests import spmv_exact as sx
from tests.test_spmv_exact_gpu import GUARD, LIBS, SHAPES, Workspace, _load, _pattern
from tests import test_spmv_exact_gpu as single_suite
from tests.test_linsys_multi_gpu import CASES, _case_data, _check_column, _init, _multi, _p_case, _ref, _single

pytestmark = pytest.mark.gpu

NRHS = (2, 3, 4, 5, 8, 11, 16)
SCALES = (0.003, 0.03, 0.1, 1.0, 3.0)  # the reference itself stays inside _check_column's bounds up to scale 3 (measured: 0.31 of it)


def _hip():
    return single_suite._hip


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact block products under per-column R
# ---------------------------------------------------------------------------------------------------------------------------------
def _apply_block_r(ws, cols, drs):
    """scs_amd_linsys_mat_vec_multi_r_dev on the block whose columns are `cols` under the diag_r's `drs`: NaN guards behind the
    input, behind R and behind the output, padding columns of X zero and of R one; two calls, same bits.  Returns (n, nrhs)."""
    L, dt = ws.L, ws.dtype
    n, m = ws.ops.n, ws.ops.m
    nrhs = len(cols)
    W = max(2, L.scs_amd_linsys_multi_width(nrhs))
    assert W >= nrhs and W in (2, 4, 8, 16)
    X = np.zeros((n, W), dt)
    R = np.ones((n + m, W), dt)
    for k in range(nrhs):
        X[:, k] = cols[k].astype(dt)
        R[:, k] = drs[k].astype(dt)
    guard = np.full(GUARD, np.nan, dt)
    inp = np.concatenate([X.ravel(), guard])
    rin = np.concatenate([R.ravel(), guard])
    nan_out = np.full(n * W + GUARD, np.nan, dt)
    hip = _hip()
    din, dr_, dout = hip.malloc(inp.nbytes), hip.malloc(rin.nbytes), hip.malloc(nan_out.nbytes)
    try:
        hip.put(din, inp)
        hip.put(dr_, rin)
        res = []
        for _ in range(2):
            hip.put(dout, nan_out)
            hip.sync()
            assert L.scs_amd_linsys_mat_vec_multi_r_dev(ws.w, nrhs, dr_, din, dout) == 0
            assert L.scs_amd_linsys_sync(ws.w) == 0
            got = np.empty(n * W + GUARD, dt)
            hip.get(got, dout)
            res.append(got)
    finally:
        hip.free(din)
        hip.free(dr_)
        hip.free(dout)
    blocks = []
    for got in res:
        assert np.array_equal(_bits(got[n * W:]), _bits(nan_out[n * W:])), "the guard behind the output was written"
        Y = got[:n * W].reshape(n, W)
        bad = np.argwhere(~np.isfinite(Y))  # padding columns included: they are ordinary finite columns (X = 0, R = 1)
        assert bad.size == 0, f"{len(bad)} elements not written or gathered past an input's end (NaN), first (row, column) {bad[:5].tolist()}"
        blocks.append(Y[:, :nrhs])
    assert np.array_equal(_bits(blocks[0]), _bits(blocks[1])), "a second call gave different bits"
    return blocks[0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lib", ["f64", "f32", "dlong"])
def test_block_product_per_column_r_exact_and_bounded(lib, shape):
    L = _load(lib)
    dtype = LIBS[lib][1]
    A_pat, P_pat = _pattern(shape)
    m, n = A_pat.shape
    rng = np.random.default_rng(zlib.crc32(f"multi-r-{lib}-{shape}".encode()))
    x_hi, e = (7, 2) if dtype is np.float64 else (3, 1)  # the amplitudes and the exponent range of sx.exact_problem
    # (a) integer data; every column its own power-of-two diag_r and its own integer vector; no column may go vacuous
    ops, x0, y0 = sx.exact_problem(A_pat, P_pat, rng, dtype)
    xs, opk, refs = [], [], []
    for k in range(16):
        exps_k = rng.integers(-e, e + 1, n + m, dtype=np.int8).astype(np.int64)
        xk = sx.int_values(n, rng, 1, x_hi)
        ok = sx.Operators(ops.A, ops.P, np.ldexp(1.0, exps_k), exps_k)
        bits, K = ok.exact_bits_needed(xk, y0)
        assert bits < sx.PREC_BITS[dtype], f"column {k} needs {bits:.1f} bits (K = {K})"
        xs.append(xk)
        opk.append(ok)
        refs.append(ok.exact(xk, y0)[2])
    ws = Workspace(L, ops, dtype)  # the workspace's own diag_r (ops.diag_r) is none of the columns'
    try:
        for nrhs in NRHS:
            Y = _apply_block_r(ws, xs[:nrhs], [o.diag_r for o in opk[:nrhs]])
            for k in range(nrhs):
                sx.check_exact(np.ascontiguousarray(Y[:, k]), refs[k], dtype, f"R_x,k x + P x + A' R_y,k^-1 A x, nrhs {nrhs}, column {k}")
    finally:
        ws.free()
    # (b) real data: diag_r_k = 10 ** U(-2, 2) per column; every column within the rounding bound of the long-double product
    ops, x0, y0 = sx.cast(*sx.real_problem(A_pat, P_pat, rng), dtype)
    spread = lambda k: (rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-8, 8, k)).astype(dtype).astype(np.float64)
    xs, opk, lds, bnd = [], [], [], []
    for k in range(16):
        dk = (10.0 ** rng.uniform(-2, 2, n + m)).astype(dtype).astype(np.float64)
        xk = spread(n)
        ok = sx.Operators(ops.A, ops.P, dk)
        xs.append(xk)
        opk.append(ok)
        lds.append(ok.longdouble(xk, y0)[2])
        bnd.append(ok.bounds(xk, y0, sx.UNIT_ROUNDOFF[dtype])[2])
    ws = Workspace(L, ops, dtype)
    try:
        for nrhs in NRHS:
            Y = _apply_block_r(ws, xs[:nrhs], [o.diag_r for o in opk[:nrhs]])
            for k in range(nrhs):
                sx.check_bound(Y[:, k], lds[k], bnd[k], f"per-column mat_vec, nrhs {nrhs}, column {k}")
    finally:
        ws.free()


def test_per_column_product_refuses_bad_widths_and_runs_one_column():
    L = _load("f64")
    A_pat, P_pat = _pattern("mod4")
    rng = np.random.default_rng(5)
    ops, x, y = sx.exact_problem(A_pat, P_pat, rng, np.float64)
    ws = Workspace(L, ops, np.float64)
    hip = _hip()
    d = hip.malloc(64 * 8)
    try:
        fn = L.scs_amd_linsys_mat_vec_multi_r_dev
        assert fn(ws.w, 0, d, d, d) == -1 and fn(ws.w, 17, d, d, d) == -1
        assert fn(ws.w, 2, None, d, d) == -1 and fn(ws.w, 2, d, None, d) == -1 and fn(ws.w, 2, d, d, None) == -1
        Y = _apply_block_r(ws, [x], [ops.diag_r])  # one column: a block of width 2
        sx.check_exact(np.ascontiguousarray(Y[:, 0]), ops.exact(x, y)[2], np.float64, "one column")
    finally:
        hip.free(d)
        ws.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# solves
# ---------------------------------------------------------------------------------------------------------------------------------
def _multi_r(lib, w, DR, B, S, tol, lddr=None, ldb=None, lds=None, expect=0):
    """scs_amd_solve_lin_sys_multi_r on copies: DR (n + m, K), B (n + m, K), S (n, K) or None, tol scalar or K.  Gaps behind the
    columns are NaN-filled and must stay so; DR and S must come back unchanged.  Returns (XY, iters)."""
    T = lib._scs_types
    nm, K = B.shape
    assert DR.shape == (nm, K)
    ldb, lddr = ldb or nm, lddr or nm
    buf = np.full((K, ldb), np.nan)  # row k of this C array = column k of the column-major block
    buf[:, :nm] = B.T
    dbuf = np.full((K, lddr), np.nan)
    dbuf[:, :nm] = DR.T
    dkeep = dbuf.copy()
    sb = None
    if S is not None:
        lds = lds or S.shape[0]
        sb = np.full((K, lds), np.nan)
        sb[:, :S.shape[0]] = S.T
        skeep = sb.copy()
    tv = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (K,)))
    it = np.full(K, -7, dtype=T.np_int)
    rc = lib.scs_amd_solve_lin_sys_multi_r(w, K, dbuf.ctypes.data_as(T.fp), lddr, buf.ctypes.data_as(T.fp), ldb,
                                           sb.ctypes.data_as(T.fp) if sb is not None else None, lds or 0, tv.ctypes.data_as(T.fp),
                                           it.ctypes.data_as(T.ip))
    assert rc == expect
    assert np.array_equal(_bits(dbuf), _bits(dkeep)), "DR or the gap behind one of its columns was modified"
    if ldb > nm:
        assert np.all(np.isnan(buf[:, nm:])), "the gap behind a column of B was written"
    if sb is not None:
        assert np.array_equal(_bits(sb), _bits(skeep)), "S was modified"
    if expect != 0:
        assert np.array_equal(buf[:, :nm], B.T), "a refused call touched B"
    return np.ascontiguousarray(buf[:, :nm].T), it.astype(np.int64)


def _set_r(lib, w, dr):
    assert lib.scs_update_lin_sys_diag_r(w, dr.ctypes.data_as(lib._scs_types.fp)) == 0


def _drs(n, m, z, scales):
    return np.stack([probgen.diag_r(n, m, z=z, scale=s) for s in scales], axis=1)


# ---- 2. against the reference backend ----
@pytest.mark.parametrize("n,m,col_nnz,warm,tol", CASES[:4])
def test_columns_match_reference_under_their_own_diag_r(n, m, col_nnz, warm, tol):
    ref = _ref()
    amd = capi.load("libscsamd_linsys.so")
    K = 5
    prob, dr, B, S = _case_data(n, m, col_nnz, warm, K)
    DR = _drs(n, m, m // 10, SCALES)
    Asp = prob.sparse()
    wa, wr = _init(amd, prob, dr), _init(ref, prob, dr)
    try:
        XY, iters = _multi_r(amd, wa, DR, B, S, tol)
        assert np.all(iters >= 0)
        for k in range(K):
            dk = np.ascontiguousarray(DR[:, k])
            _set_r(ref, wr, dk)
            _set_r(amd, wa, dk)
            s = S[:, k].copy() if warm else None
            xr = _single(ref, wr, B[:, k].copy(), s, tol)
            xs = _single(amd, wa, B[:, k].copy(), s, tol)
            _check_column(Asp, None, dk, n, B[:, k], XY[:, k], tol, xr, xs, f"column {k} (scale {SCALES[k]})")
    finally:
        amd.scs_free_lin_sys_work(wa)
        ref.scs_free_lin_sys_work(wr)


def test_columns_with_P_match_reference_under_their_own_diag_r():
    ref = _ref()
    amd = capi.load("libscsamd_linsys.so")
    prob, P, dr, B, S = _p_case()
    n, m = prob.n, prob.m
    DR = _drs(n, m, 50, SCALES)
    wa, wr = _init(amd, prob, dr, True), _init(ref, prob, dr, True)
    try:
        XY, iters = _multi_r(amd, wa, DR, B, S, 1e-12)
        for k in range(B.shape[1]):
            dk = np.ascontiguousarray(DR[:, k])
            _set_r(ref, wr, dk)
            _set_r(amd, wa, dk)
            xr = _single(ref, wr, B[:, k].copy(), S[:, k].copy(), 1e-12)
            xs = _single(amd, wa, B[:, k].copy(), S[:, k].copy(), 1e-12)
            assert np.abs(XY[:, k] - xr).max() <= 1e-8 * np.abs(xr).max()  # the bound of test_with_P_matches_reference
            _check_column(prob.sparse(), P, dk, n, B[:, k], XY[:, k], 1e-12, xr, xs, f"column {k} (scale {SCALES[k]})")
    finally:
        amd.scs_free_lin_sys_work(wa)
        ref.scs_free_lin_sys_work(wr)


# ---- 3. bit identities ----
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("K", [2, 5, 16])
def test_bit_identities(K, warm):
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 1000, 3000, 1e-9
    prob, dr, B, S = _case_data(n, m, 32, warm, K)
    w = _init(amd, prob, dr)
    try:
        # (iv, before) the workspace's own paths
        s0 = S[:, 0].copy() if warm else None
        one_before = _single(amd, w, B[:, 0].copy(), s0, tol)
        shared, shared_it = _multi(amd, w, B, S, tol)
        # (i) every column's R equal to the workspace's diag_r: the shared-R block solve, bit for bit
        XY, iters = _multi_r(amd, w, np.tile(dr[:, None], (1, K)), B, S, tol)
        assert np.array_equal(_bits(XY), _bits(shared)), "equal R in every column differs from the shared-R block solve"
        assert np.array_equal(iters, shared_it)
        # (iii) two calls, same bits
        scales = np.geomspace(0.003, 3.0, K)
        DR = _drs(n, m, m // 10, scales)
        XY1, it1 = _multi_r(amd, w, DR, B, S, tol)
        XY2, it2 = _multi_r(amd, w, DR, B, S, tol)
        assert np.array_equal(_bits(XY1), _bits(XY2)) and np.array_equal(it1, it2)
        # (ii) position: the block rotated by K // 2 (for K = 4 this would be [R_c, R_d, R_a, R_b])
        sh = K // 2
        XYr, itr = _multi_r(amd, w, np.roll(DR, sh, axis=1), np.roll(B, sh, axis=1), np.roll(S, sh, axis=1) if warm else None, tol)
        assert np.array_equal(_bits(np.roll(XYr, -sh, axis=1)), _bits(XY1)), "a column's bits depend on its position"
        assert np.array_equal(np.roll(itr, -sh), it1)
        # (ii) neighbours: column 0 moves to position K // 2 among columns of other R, other right-hand sides, other tolerances
        other = np.random.default_rng(99)
        DR2 = _drs(n, m, m // 10, other.uniform(0.005, 2.0, K))
        B2 = other.uniform(-3, 3, B.shape)
        S2 = other.uniform(-1, 1, S.shape) * 0.1 if warm else None
        tols = np.full(K, 1e-6)
        DR2[:, sh], B2[:, sh], tols[sh] = DR[:, 0], B[:, 0], tol
        if warm:
            S2[:, sh] = S[:, 0]
        XYn, itn = _multi_r(amd, w, DR2, B2, S2, tols)
        assert np.array_equal(_bits(XYn[:, sh]), _bits(XY1[:, 0])), "a column's bits depend on its neighbours' R"
        assert itn[sh] == it1[0]
        # (iv, after) the workspace's own diag_r, preconditioner and single-vector state are untouched
        assert np.array_equal(_bits(_single(amd, w, B[:, 0].copy(), s0, tol)), _bits(one_before))
        again, again_it = _multi(amd, w, B, S, tol)
        assert np.array_equal(_bits(again), _bits(shared)) and np.array_equal(again_it, shared_it)
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 4. per-column control ----
def _stats(lib, w):
    st = lib._scs_types.ScsAmdStats()
    lib.scs_amd_linsys_get_stats(w, C.byref(st))
    return st.cg_iters, st.lin_sys_solves, st.mat_vecs


def test_per_column_control_under_per_column_r():
    amd = capi.load("libscsamd_linsys.so")
    n, m = 3000, 7001
    prob, dr, B, _ = _case_data(n, m, 9, False, 3)
    Asp = prob.sparse()
    ZERO, LOOSE, TIGHT = 0, 1, 2
    DR = _drs(n, m, m // 10, (0.03, 3.0, 1.0))
    B[:, ZERO] = 1e-13  # |b|_inf <= 1e-12: private.c:296-299
    tols = np.array([1e-9, 1e-4, 1e-12])
    w = _init(amd, prob, dr)
    try:
        before = _stats(amd, w)
        XY, iters = _multi_r(amd, w, DR, B, None, tols)
        after = _stats(amd, w)
        assert np.all(XY[:, ZERO] == 0.0) and iters[ZERO] == 0
        assert iters[LOOSE] > 0 and iters[TIGHT] > 0
        for k in (LOOSE, TIGHT):
            _check_column(Asp, None, np.ascontiguousarray(DR[:, k]), n, B[:, k], XY[:, k], tols[k], None, None, f"column {k}")
        # a looser tolerance under the same R stops earlier: the tight column's R with the loose tolerance
        XYl, itl = _multi_r(amd, w, DR[:, [ZERO, TIGHT, TIGHT]], B[:, [ZERO, TIGHT, TIGHT]], None, tols)
        assert 0 < itl[1] < itl[2] and itl[2] == iters[TIGHT]
        assert after[0] - before[0] == iters.sum()  # counted as a block solve is counted
        assert after[1] - before[1] == 3
        assert after[2] - before[2] == iters.max()
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 5. seventeen columns ----
def test_seventeen_columns_in_two_chunks_under_per_column_r():
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol, K = 3000, 7001, 1e-9, 17
    prob, dr, B, S = _case_data(n, m, 9, True, K)
    DR = _drs(n, m, m // 10, np.geomspace(0.003, 3, K))
    Asp = prob.sparse()
    w = _init(amd, prob, dr)
    try:
        XY, iters = _multi_r(amd, w, DR, B, S, tol, lddr=n + m + 13)  # _multi_r asserts that DR and its NaN-filled gap are unchanged
        for k in range(K):
            dk = np.ascontiguousarray(DR[:, k])
            _set_r(amd, w, dk)
            xs = _single(amd, w, B[:, k].copy(), S[:, k].copy(), tol)
            _check_column(Asp, None, dk, n, B[:, k], XY[:, k], tol, None, xs, f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 6. one column ----
def test_one_column_under_its_own_r_matches_reference():
    ref = _ref()
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 1000, 3000, 1e-12
    prob, dr, B, _ = _case_data(n, m, 32, False, 1)
    DR = _drs(n, m, m // 10, (1.0,))
    dk = np.ascontiguousarray(DR[:, 0])
    wa, wr = _init(amd, prob, dr), _init(ref, prob, dk)
    try:
        one_before = _single(amd, wa, B[:, 0].copy(), None, tol)
        XY, iters = _multi_r(amd, wa, DR, B, None, tol)
        assert iters[0] > 0
        xr = _single(ref, wr, B[:, 0].copy(), None, tol)
        _check_column(prob.sparse(), None, dk, n, B[:, 0], XY[:, 0], tol, xr, None, "one column")
        assert np.array_equal(_bits(_single(amd, wa, B[:, 0].copy(), None, tol)), _bits(one_before))  # it stayed off the single-vector state
    finally:
        amd.scs_free_lin_sys_work(wa)
        ref.scs_free_lin_sys_work(wr)


# ---- 7. refusals on a live workspace ----
def test_refusals_on_a_live_workspace():
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 50, 150, 1e-9
    prob, dr, B, S = _case_data(n, m, 4, True, 3)
    DR = _drs(n, m, m // 10, (0.03, 0.1, 1.0))
    Asp = prob.sparse()
    w = _init(amd, prob, dr)
    try:
        for bad, where in ((0.0, (0, 0)), (-1.0, (n + m - 1, 2)), (np.nan, (n, 1)), (np.inf, (3, 2)), (-np.inf, (n + 5, 0))):
            D2 = DR.copy()
            D2[where] = bad
            _multi_r(amd, w, D2, B, S, tol, expect=-1)  # asserts B, S and D2 unchanged
        # leading dimensions that are too short (the caller's arrays are laid out for the right ones: nothing may be read)
        T = amd._scs_types
        fp = lambda a: a.ctypes.data_as(T.fp)
        Bf, Df, Sf, tv = np.asfortranarray(B), np.asfortranarray(DR), np.asfortranarray(S), np.full(3, tol)
        it = np.zeros(3, dtype=T.np_int)
        call = lambda lddr, ldb, lds: amd.scs_amd_solve_lin_sys_multi_r(w, 3, fp(Df), lddr, fp(Bf), ldb, fp(Sf), lds, fp(tv), it.ctypes.data_as(T.ip))
        assert call(n + m - 1, n + m, n) == -1 and call(n + m, n + m - 1, n) == -1 and call(n + m, n + m, n - 1) == -1
        assert np.array_equal(Bf, B)
        XY, _ = _multi_r(amd, w, DR, B, S, tol)  # the next call succeeds
        for k in range(3):
            dk = np.ascontiguousarray(DR[:, k])
            _set_r(amd, w, dk)
            _check_column(Asp, None, dk, n, B[:, k], XY[:, k], tol, None, _single(amd, w, B[:, k].copy(), S[:, k].copy(), tol), f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 8. device memory ----
def _free_bytes(lib):
    v = lib.scs_amd_device_free_bytes()
    assert v >= 0
    return v


def test_per_column_blocks_are_allocated_by_the_first_per_column_call_and_freed_with_the_workspace():
    """the per-column blocks of this system at width 16 hold (2 n + m) 16 x 8 bytes = 15 MB; allowance for the runtime's own caches
    as in test_block_buffers_are_freed_with_the_workspace"""
    amd = capi.load("libscsamd_linsys.so")
    n, m, K = 30000, 60000, 16
    prob, dr, B, S = _case_data(n, m, 10, True, K)
    DR = _drs(n, m, m // 10, np.geomspace(0.01, 1.0, K))
    slack = 8 << 20
    w = _init(amd, prob, dr)  # warm: context, streams, code objects of both paths
    _multi(amd, w, B[:, :2], S[:, :2], 1e-6)
    _multi_r(amd, w, DR[:, :2], B[:, :2], S[:, :2], 1e-6)
    amd.scs_free_lin_sys_work(w)
    base = _free_bytes(amd)
    w = _init(amd, prob, dr)
    _multi(amd, w, B, S, 1e-6)
    shared_only = _free_bytes(amd)
    _multi(amd, w, B, S, 1e-6)
    assert abs(_free_bytes(amd) - shared_only) <= slack  # a caller who never uses the feature allocates what it allocated
    _multi_r(amd, w, DR, B, S, 1e-6)
    with_r = _free_bytes(amd)
    r_bytes = (2 * n + m) * K * 8
    assert r_bytes * 0.9 <= shared_only - with_r <= r_bytes + slack
    _multi_r(amd, w, DR, B, S, 1e-6)
    assert abs(_free_bytes(amd) - with_r) <= slack  # reused
    amd.scs_free_lin_sys_work(w)
    assert abs(_free_bytes(amd) - base) <= slack


# ---- 9. dlong ----
def test_dlong_build_per_column_solve_matches_its_single_vector_path():
    amd = capi.load("libscsamd_dlong.so")
    T = amd._scs_types
    n, m, K, tol = 3000, 7001, 3, 1e-9
    rng = np.random.default_rng(n + m)
    A = probgen.random_csc(m, n, 9, seed=7)
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), T=T)
    dr = probgen.diag_r(n, m, z=m // 10)
    DR = _drs(n, m, m // 10, (0.03, 0.3, 3.0))
    B = rng.uniform(-1, 1, (n + m, K))
    w = _init(amd, prob, dr)
    try:
        XY, iters = _multi_r(amd, w, DR, B, None, tol)
        for k in range(K):
            dk = np.ascontiguousarray(DR[:, k])
            _set_r(amd, w, dk)
            _check_column(prob.sparse(), None, dk, n, B[:, k], XY[:, k], tol, None, _single(amd, w, B[:, k].copy(), None, tol), f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 10. the Python object ----
def test_python_solve_many_with_diag_r():
    from scs_amd.linsys import LinSys
    amd = capi.load("libscsamd.so")  # the library the object loads
    n, m, K, tol = 1000, 3000, 3, 1e-9
    prob, dr, B, S = _case_data(n, m, 32, True, K)
    DR = _drs(n, m, m // 10, (0.03, 0.3, 3.0))
    w = _init(amd, prob, dr)
    try:
        want, want_it = _multi(amd, w, B, S, tol)  # today's call
    finally:
        amd.scs_free_lin_sys_work(w)
    Asp = prob.sparse()
    with LinSys(Asp, dr) as ls:
        for order in ("F", "C"):
            Do = np.array(DR, order=order)
            keep = Do.copy()
            XY, iters = ls.solve_many(B, S, tol, diag_r=Do)
            assert np.array_equal(Do, keep), "diag_r was modified"
            XYn, itn = ls.solve_many(B, S, tol, diag_r=None)
            assert np.array_equal(_bits(XYn), _bits(want)) and np.array_equal(itn, want_it)
        for k in range(K):
            ls.update_diag_r(DR[:, k])
            xs = ls.solve(B[:, k], S[:, k], tol)
            _check_column(Asp, None, np.ascontiguousarray(DR[:, k]), n, B[:, k], XY[:, k], tol, None, xs, f"column {k}")
        for bad in (DR[:-1], DR[:, :2], -DR, np.where(DR > 1, np.nan, DR)):
            with pytest.raises(ValueError):
                ls.solve_many(B, S, tol, diag_r=bad)
