"""K KKT systems on one pattern, every column with its own values of A and P and its own diag_r (include/scs_amd.h:
scs_amd_linsys_set_values_multi, scs_amd_solve_lin_sys_multi_v, scs_amd_linsys_mat_vec_multi_v_dev, scs_amd_linsys_free_values_multi;
kernels in scs_amd/csrc/spmm.h and linsys_multi.h).  The contract, line by line:

 1. the block product with per-column values against an exact product and a rounding bound, edge shapes, every width, three builds;
 2. every column holding the workspace's own values = the shared-value block solves, bit for bit;
 3. different values = column k of scs_amd_solve_lin_sys_multi_r on a second workspace brought to values k by
    scs_amd_linsys_update_values, bit for bit;
 4. a column depends neither on its neighbours' values nor on its position; two calls agree;
 5. the workspace's own single solve, _multi and _multi_r are untouched by set, solve and free; update_values between a set and a
    solve does not change the solve;
 6. every column against the reference backend on (A_k, P_k, diag_r_k), with the bounds of tests/test_linsys_multi_gpu.py unchanged.
Then per-column control, one column, the dlong build with the offset-bias hook, refusals on a live workspace, the Python object,
free and set again at a wider nrhs.  The value blocks are allocated by the library, so no guard can sit behind them; X, R and Y of
the products carry NaN guards.
The yardstick of every comparison is the reference backend, an exact product, or the existing shared-value paths, never the
per-value path's own earlier output."""
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi
from tests import spmv_exact as sx
from tests.test_spmv_exact_gpu import GUARD, LIBS, SHAPES, Workspace, _load, _pattern
from tests import test_spmv_exact_gpu as single_suite
from tests.test_linsys_multi_gpu import CASES, _case_data, _check_column, _init, _multi, _p_case, _ref, _single
from tests.test_linsys_multi_r_gpu import SCALES, _bits, _drs, _multi_r

pytestmark = pytest.mark.gpu

NRHS = (1, 2, 3, 4, 5, 8, 11, 16)


def _hip():
    return single_suite._hip


def _set_values(lib, w, AX, PX, ldax=None, ldpx=None, expect=0):
    """scs_amd_linsys_set_values_multi on copies: AX (nnz(A), K), PX (nnz(upper P), K) or None; gaps behind the columns are NaN-filled;
    AX and PX must come back unchanged"""
    T = lib._scs_types
    K = AX.shape[1]
    ldax = ldax or max(1, AX.shape[0])
    abuf = np.full((K, ldax), np.nan, dtype=T.np_float)  # row k of this C array = column k of the column-major block
    abuf[:, :AX.shape[0]] = AX.T
    akeep = abuf.copy()
    pbuf = None
    if PX is not None:
        assert PX.shape[1] == K
        ldpx = ldpx or max(1, PX.shape[0])
        pbuf = np.full((K, ldpx), np.nan, dtype=T.np_float)
        pbuf[:, :PX.shape[0]] = PX.T
        pkeep = pbuf.copy()
    rc = lib.scs_amd_linsys_set_values_multi(w, K, abuf.ctypes.data_as(T.fp), ldax, pbuf.ctypes.data_as(T.fp) if pbuf is not None else None,
                                             ldpx or 0)
    assert rc == expect
    assert np.array_equal(_bits(abuf), _bits(akeep)), "AX was modified"
    if pbuf is not None:
        assert np.array_equal(_bits(pbuf), _bits(pkeep)), "PX was modified"


def _multi_v(lib, w, DR, B, S, tol, lddr=None, ldb=None, lds=None, expect=0):
    """scs_amd_solve_lin_sys_multi_v on copies: DR (n + m, K) or None, B (n + m, K), S (n, K) or None, tol scalar or K.  Gaps behind the
    columns are NaN-filled and must stay so; DR and S must come back unchanged; a refused call leaves B as it was.  Returns (XY, iters)."""
    T = lib._scs_types
    nm, K = B.shape
    ldb = ldb or nm
    buf = np.full((K, ldb), np.nan)
    buf[:, :nm] = B.T
    dbuf = None
    if DR is not None:
        assert DR.shape == (nm, K)
        lddr = lddr or nm
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
    rc = lib.scs_amd_solve_lin_sys_multi_v(w, K, dbuf.ctypes.data_as(T.fp) if dbuf is not None else None, lddr or 0,
                                           buf.ctypes.data_as(T.fp), ldb, sb.ctypes.data_as(T.fp) if sb is not None else None, lds or 0,
                                           tv.ctypes.data_as(T.fp), it.ctypes.data_as(T.ip))
    assert rc == expect
    if dbuf is not None:
        assert np.array_equal(_bits(dbuf), _bits(dkeep)), "DR or the gap behind one of its columns was modified"
    if ldb > nm:
        assert np.all(np.isnan(buf[:, nm:])), "the gap behind a column of B was written"
    if sb is not None:
        assert np.array_equal(_bits(sb), _bits(skeep)), "S was modified"
    if expect != 0:
        assert np.array_equal(buf[:, :nm], B.T), "a refused call touched B"
    return np.ascontiguousarray(buf[:, :nm].T), it.astype(np.int64)


def _update(lib, w, ax, px=None):
    T = lib._scs_types
    ax = np.ascontiguousarray(ax, dtype=T.np_float)
    px = None if px is None else np.ascontiguousarray(px, dtype=T.np_float)
    assert lib.scs_amd_linsys_update_values(w, ax.ctypes.data_as(T.fp), px.ctypes.data_as(T.fp) if px is not None else None) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact block products with per-column values
# ---------------------------------------------------------------------------------------------------------------------------------
def _apply_block_v(ws, opk, cols):
    """set the values of the operators `opk` (all on the workspace's pattern), then scs_amd_linsys_mat_vec_multi_v_dev on the block
    whose columns are `cols` under the operators' diag_r: NaN guards behind X, behind R and behind Y, the output NaN-filled, padding
    columns of X zero and of R one; two calls, same bits.  Returns (n, nrhs)."""
    L, dt = ws.L, ws.dtype
    n, m = ws.ops.n, ws.ops.m
    nrhs = len(cols)
    W = max(2, L.scs_amd_linsys_multi_width(nrhs))
    assert W >= nrhs and W in (2, 4, 8, 16)
    AX = np.stack([o.A.data for o in opk], axis=1).reshape(ws.ops.A.nnz, nrhs)
    PX = None if ws.ops.P is None else np.stack([o.P.data for o in opk], axis=1).reshape(ws.ops.P.nnz, nrhs)
    _set_values(L, ws.w, AX, PX)
    X = np.zeros((n, W), dt)
    R = np.ones((n + m, W), dt)
    for k in range(nrhs):
        X[:, k] = cols[k].astype(dt)
        R[:, k] = opk[k].diag_r.astype(dt)
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
            assert L.scs_amd_linsys_mat_vec_multi_v_dev(ws.w, nrhs, dr_, din, dout) == 0
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
        bad = np.argwhere(~np.isfinite(Y))  # padding columns included: they are ordinary finite columns (values 0, X = 0, R = 1)
        assert bad.size == 0, f"{len(bad)} elements not written or read past an input's end (NaN), first (row, column) {bad[:5].tolist()}"
        blocks.append(Y[:, :nrhs])
    assert np.array_equal(_bits(blocks[0]), _bits(blocks[1])), "a second call gave different bits"
    return blocks[0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lib", ["f64", "f32", "dlong"])
def test_block_product_per_column_values_exact_and_bounded(lib, shape):
    L = _load(lib)
    dtype = LIBS[lib][1]
    A_pat, P_pat = _pattern(shape)
    rng = np.random.default_rng(zlib.crc32(f"multi-v-{lib}-{shape}".encode()))
    # (a) integer data: every column its own integer A and P on the pattern, its own power-of-two diag_r and its own integer vector
    # (sx.exact_problem asserts that no column goes vacuous); the workspace's own values and diag_r are none of the columns'
    ops0, _, _ = sx.exact_problem(A_pat, P_pat, rng, dtype)
    opk, xs, refs = [], [], []
    for k in range(16):
        ok, xk, yk = sx.exact_problem(A_pat, P_pat, rng, dtype)
        opk.append(ok)
        xs.append(xk)
        refs.append(ok.exact(xk, yk)[2])
    ws = Workspace(L, ops0, dtype)
    try:
        for nrhs in NRHS:
            Y = _apply_block_v(ws, opk[:nrhs], xs[:nrhs])
            for k in range(nrhs):
                sx.check_exact(np.ascontiguousarray(Y[:, k]), refs[k], dtype, f"R_x,k x + P_k x + A_k' R_y,k^-1 A_k x, nrhs {nrhs}, column {k}")
    finally:
        ws.free()
    # (b) real data: every column within the rounding bound of the long-double product on its own operators
    ops0 = sx.cast(*sx.real_problem(A_pat, P_pat, rng), dtype)[0]
    opk, xs, lds, bnd = [], [], [], []
    for k in range(16):
        ok, xk, yk = sx.cast(*sx.real_problem(A_pat, P_pat, rng), dtype)
        opk.append(ok)
        xs.append(xk)
        lds.append(ok.longdouble(xk, yk)[2])
        bnd.append(ok.bounds(xk, yk, sx.UNIT_ROUNDOFF[dtype])[2])
    ws = Workspace(L, ops0, dtype)
    try:
        for nrhs in NRHS:
            Y = _apply_block_v(ws, opk[:nrhs], xs[:nrhs])
            for k in range(nrhs):
                sx.check_bound(Y[:, k], lds[k], bnd[k], f"per-value mat_vec, nrhs {nrhs}, column {k}")
    finally:
        ws.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# solves
# ---------------------------------------------------------------------------------------------------------------------------------
def _perturbed(x, K, rng, amp=0.3):
    """x * (1 + amp u_k), u_k uniform in (-1, 1): (len(x), K); every value keeps its sign"""
    return x[:, None] * (1.0 + amp * rng.uniform(-1, 1, (len(x), K)))


def _csc(prob, ax):
    return sp.csc_matrix((ax, prob.Ai, prob.Ap), shape=(prob.m, prob.n))


def _p_full(prob, px):
    U = sp.csc_matrix((px, prob.Pi, prob.Pp), shape=(prob.n, prob.n))
    return (U + sp.triu(U, 1).T).tocsc()


def _p_values(prob, DR, K, rng):
    """upper P per column, perturbed by 0.3; checked on the CPU that every P_k + R_x,k stays positive definite (the amplitude is halved
    until it does)"""
    amp = 0.3
    while amp > 1e-3:
        PX = _perturbed(prob.Px, K, rng, amp)
        if all(np.linalg.eigvalsh(_p_full(prob, PX[:, k]).toarray() + np.diag(DR[:prob.n, k])).min() > 0 for k in range(K)):
            return PX
        amp /= 2
    raise AssertionError("no amplitude keeps P_k + R_x positive definite")


def _p_setup(K=5):
    prob, P, dr, B, S = _p_case()
    rng = np.random.default_rng(17)
    DR = _drs(prob.n, prob.m, 50, SCALES[:K])
    return prob, dr, B[:, :K], S[:, :K], DR, _perturbed(prob.Ax, K, rng), _p_values(prob, DR, K, rng)


# ---- 2. equal values give the shared form ----
@pytest.mark.parametrize("with_P", [False, True])
def test_workspace_values_in_every_column_give_the_shared_value_solves(with_P):
    amd = capi.load("libscsamd_linsys.so")
    K, tol = 5, 1e-9
    if with_P:
        prob, dr, B, S, DR, _, _ = _p_setup(K)
    else:
        n, m = 1000, 3000
        prob, dr, B, S = _case_data(n, m, 32, True, K)
        DR = _drs(n, m, m // 10, SCALES)
    w = _init(amd, prob, dr, with_P)
    try:
        want_r, it_r = _multi_r(amd, w, DR, B, S, tol)
        want_s, it_s = _multi(amd, w, B, S, tol)
        _set_values(amd, w, np.tile(prob.Ax[:, None], (1, K)), np.tile(prob.Px[:, None], (1, K)) if with_P else None)
        XY, it = _multi_v(amd, w, DR, B, S, tol)
        assert np.array_equal(_bits(XY), _bits(want_r)) and np.array_equal(it, it_r), "differs from the per-column-R block solve"
        XY, it = _multi_v(amd, w, None, B, S, tol)
        assert np.array_equal(_bits(XY), _bits(want_s)) and np.array_equal(it, it_s), "DR = NULL differs from the shared-R block solve"
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- 3. and 6. different values: an updated workspace bit for bit, the reference backend within its bounds ----
def _compare_columns(amd, prob, dr, with_P, DR, B, S, AX, PX, tol, p_bound=False):
    """contract 3 on every column (always), contract 6 where the reference backend is built"""
    from oracle import pyoracle
    ref = pyoracle.load_ref() if pyoracle.ref_available() else None
    K = B.shape[1]
    n = prob.n
    wa, w2 = _init(amd, prob, dr, with_P), _init(amd, prob, dr, with_P)
    try:
        _set_values(amd, wa, AX, PX)
        XY, iters = _multi_v(amd, wa, DR, B, S, tol)
        assert np.all(iters >= 0)
        for k in range(K):
            _update(amd, w2, AX[:, k], PX[:, k] if with_P else None)
            XYk, itk = _multi_r(amd, w2, DR, B, S, tol)
            assert np.array_equal(_bits(XY[:, k]), _bits(XYk[:, k])), f"column {k} differs from the per-column-R solve on the updated workspace"
            assert iters[k] == itk[k]
            if ref is None:
                continue
            Ak = _csc(prob, AX[:, k])
            Pk = _p_full(prob, PX[:, k]) if with_P else None
            pk = capi.Problem(Ak, np.zeros(prob.m), np.zeros(n), dict(l=prob.m), P=Pk)
            dk = np.ascontiguousarray(DR[:, k])
            wr = _init(ref, pk, dk, with_P)
            try:
                xr = _single(ref, wr, B[:, k].copy(), S[:, k].copy() if S is not None else None, tol)
            finally:
                ref.scs_free_lin_sys_work(wr)
            if p_bound:
                assert np.abs(XY[:, k] - xr).max() <= 1e-8 * np.abs(xr).max()  # the bound of test_with_P_matches_reference
            _check_column(Ak, Pk, dk, n, B[:, k], XY[:, k], tol, xr, None, f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(wa)
        amd.scs_free_lin_sys_work(w2)
    return ref is not None


@pytest.mark.parametrize("n,m,col_nnz,warm,tol", CASES)
def test_columns_match_an_updated_workspace_and_the_reference(n, m, col_nnz, warm, tol):
    amd = capi.load("libscsamd_linsys.so")
    K = 5
    prob, dr, B, S = _case_data(n, m, col_nnz, warm, K)
    AX = _perturbed(prob.Ax, K, np.random.default_rng(n))
    if not _compare_columns(amd, prob, dr, False, _drs(n, m, m // 10, SCALES), B, S, AX, None, tol):
        _ref()  # contract 3 held; contract 6 needs the reference backend


def test_columns_with_P_match_an_updated_workspace_and_the_reference():
    amd = capi.load("libscsamd_linsys.so")
    prob, dr, B, S, DR, AX, PX = _p_setup()
    if not _compare_columns(amd, prob, dr, True, DR, B, S, AX, PX, 1e-12, p_bound=True):
        _ref()


# ---- 4. and 5. independence; nothing else moves ----
@pytest.mark.parametrize("with_P", [False, True])
@pytest.mark.parametrize("K", [2, 5, 16])
def test_bit_identities(K, with_P):
    amd = capi.load("libscsamd_linsys.so")
    tol = 1e-9
    rng = np.random.default_rng(K)
    if with_P:
        prob, P, dr, B5, S5 = _p_case()
        n, m = prob.n, prob.m
        B, S = rng.uniform(-1, 1, (n + m, K)), rng.uniform(-1, 1, (n, K))
        B[:, :min(K, 5)], S[:, :min(K, 5)] = B5[:, :K], S5[:, :K]
        DR = _drs(n, m, 50, np.geomspace(0.003, 3.0, K))
        PX = _p_values(prob, DR, K, rng)
        # the neighbours' P must stay positive definite under the neighbours' R too
        DR2 = _drs(n, m, 50, rng.uniform(0.005, 2.0, K))
        PX2 = _p_values(prob, DR2, K, rng)
    else:
        n, m = 1000, 3000
        prob, dr, B, S = _case_data(n, m, 32, True, K)
        DR = _drs(n, m, m // 10, np.geomspace(0.003, 3.0, K))
        DR2 = _drs(n, m, m // 10, rng.uniform(0.005, 2.0, K))
        PX = PX2 = None
    AX = _perturbed(prob.Ax, K, rng)
    w = _init(amd, prob, dr, with_P)
    try:
        # (5, before) the workspace's own paths
        one_before = _single(amd, w, B[:, 0].copy(), S[:, 0].copy(), tol)
        shared, shared_it = _multi(amd, w, B, S, tol)
        shared_r, shared_r_it = _multi_r(amd, w, DR, B, S, tol)
        _set_values(amd, w, AX, PX)
        XY1, it1 = _multi_v(amd, w, DR, B, S, tol)
        XY2, it2 = _multi_v(amd, w, DR, B, S, tol)
        assert np.array_equal(_bits(XY1), _bits(XY2)) and np.array_equal(it1, it2), "two calls differ"
        # (5) update_values / update_diag_r between a set and a solve change nothing of the solve
        _update(amd, w, AX[:, K - 1], PX[:, K - 1] if with_P else None)
        assert amd.scs_update_lin_sys_diag_r(w, np.ascontiguousarray(DR[:, K - 1]).ctypes.data_as(amd._scs_types.fp)) == 0
        XY3, it3 = _multi_v(amd, w, DR, B, S, tol)
        assert np.array_equal(_bits(XY3), _bits(XY1)) and np.array_equal(it3, it1), "update_values changed the stored blocks"
        _update(amd, w, prob.Ax, prob.Px if with_P else None)
        assert amd.scs_update_lin_sys_diag_r(w, dr.ctypes.data_as(amd._scs_types.fp)) == 0
        # (4) position: the block rotated by K // 2
        sh = K // 2
        roll = lambda a: None if a is None else np.roll(a, sh, axis=1)
        _set_values(amd, w, roll(AX), roll(PX))
        XYr, itr = _multi_v(amd, w, roll(DR), roll(B), roll(S), tol)
        assert np.array_equal(_bits(np.roll(XYr, -sh, axis=1)), _bits(XY1)), "a column's bits depend on its position"
        assert np.array_equal(np.roll(itr, -sh), it1)
        # (4) neighbours: column 0 moves to position K // 2 among columns of other values, other R, other right-hand sides
        AX2 = _perturbed(prob.Ax, K, rng)
        B2, S2, tols = rng.uniform(-3, 3, B.shape), rng.uniform(-1, 1, S.shape) * 0.1, np.full(K, 1e-6)
        AX2[:, sh], DR2[:, sh], B2[:, sh], S2[:, sh], tols[sh] = AX[:, 0], DR[:, 0], B[:, 0], S[:, 0], tol
        if with_P:
            PX2[:, sh] = PX[:, 0]
        _set_values(amd, w, AX2, PX2)
        XYn, itn = _multi_v(amd, w, DR2, B2, S2, tols)
        assert np.array_equal(_bits(XYn[:, sh]), _bits(XY1[:, 0])), "a column's bits depend on its neighbours"
        assert itn[sh] == it1[0]
        # (5, after) set, solve and free left the workspace's own paths as they were
        amd.scs_amd_linsys_free_values_multi(w)
        assert np.array_equal(_bits(_single(amd, w, B[:, 0].copy(), S[:, 0].copy(), tol)), _bits(one_before))
        again, again_it = _multi(amd, w, B, S, tol)
        assert np.array_equal(_bits(again), _bits(shared)) and np.array_equal(again_it, shared_it)
        again, again_it = _multi_r(amd, w, DR, B, S, tol)
        assert np.array_equal(_bits(again), _bits(shared_r)) and np.array_equal(again_it, shared_r_it)
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- per-column control ----
def test_per_column_tolerance_and_a_zero_right_hand_side():
    amd = capi.load("libscsamd_linsys.so")
    n, m = 3000, 7001
    prob, dr, B, _ = _case_data(n, m, 9, False, 3)
    ZERO, LOOSE, TIGHT = 0, 1, 2
    DR = _drs(n, m, m // 10, (0.03, 3.0, 1.0))
    AX = _perturbed(prob.Ax, 3, np.random.default_rng(4))
    B[:, ZERO] = 1e-13  # |b|_inf <= 1e-12: private.c:296-299
    tols = np.array([1e-9, 1e-4, 1e-12])
    w = _init(amd, prob, dr)
    try:
        _set_values(amd, w, AX, None)
        XY, iters = _multi_v(amd, w, DR, B, None, tols)
        assert np.all(XY[:, ZERO] == 0.0) and iters[ZERO] == 0
        assert iters[LOOSE] > 0 and iters[TIGHT] > 0
        for k in (LOOSE, TIGHT):
            _check_column(_csc(prob, AX[:, k]), None, np.ascontiguousarray(DR[:, k]), n, B[:, k], XY[:, k], tols[k], None, None, f"column {k}")
        # a looser tolerance on the same system stops earlier
        sel = [ZERO, TIGHT, TIGHT]
        _set_values(amd, w, AX[:, sel], None)
        XYl, itl = _multi_v(amd, w, DR[:, sel], B[:, sel], None, tols)
        assert 0 < itl[1] < itl[2] and itl[2] == iters[TIGHT]
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- one column ----
def test_one_column_runs_off_the_single_vector_state():
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 1000, 3000, 1e-12
    prob, dr, B, S = _case_data(n, m, 32, True, 1)
    DR = _drs(n, m, m // 10, (0.3,))
    AX = _perturbed(prob.Ax, 1, np.random.default_rng(8))
    w, w2 = _init(amd, prob, dr), _init(amd, prob, dr)
    try:
        one_before = _single(amd, w, B[:, 0].copy(), None, tol)
        _set_values(amd, w, AX, None)
        XY, iters = _multi_v(amd, w, DR, B, S, tol)
        assert iters[0] > 0
        _update(amd, w2, AX[:, 0])
        XYr, itr = _multi_r(amd, w2, DR, B, S, tol)
        assert np.array_equal(_bits(XY), _bits(XYr)) and np.array_equal(iters, itr)
        _check_column(_csc(prob, AX[:, 0]), None, np.ascontiguousarray(DR[:, 0]), n, B[:, 0], XY[:, 0], tol, None, None, "one column")
        assert np.array_equal(_bits(_single(amd, w, B[:, 0].copy(), None, tol)), _bits(one_before))
    finally:
        amd.scs_free_lin_sys_work(w)
        amd.scs_free_lin_sys_work(w2)


# ---- the dlong build, plain and with every stored entry position carrying 2^31 + 2^20 ----
@pytest.mark.parametrize("bias", [None, str(2**31 + 2**20)], ids=["dlong", "dlong_offset_bias"])
def test_dlong_build(monkeypatch, bias):
    amd = capi.load("libscsamd_dlong.so")
    if bias:
        monkeypatch.setenv("SCS_AMD_TEST_OFFSET_BIAS", bias)
    else:
        monkeypatch.delenv("SCS_AMD_TEST_OFFSET_BIAS", raising=False)
    T = amd._scs_types
    n, m, K, tol = 300, 500, 3, 1e-9
    rng = np.random.default_rng(n + m)
    p64, P, dr, B, S = _p_case()
    prob = capi.Problem(p64.sparse(), np.zeros(m), np.zeros(n), dict(l=m), P=P, T=T)
    B, S = B[:, :K], S[:, :K]
    DR = _drs(n, m, 50, (0.03, 0.3, 3.0))
    AX, PX = _perturbed(prob.Ax, K, rng), _p_values(prob, DR, K, rng)
    w, w2 = _init(amd, prob, dr, True), _init(amd, prob, dr, True)
    try:
        _set_values(amd, w, AX, PX)
        XY, iters = _multi_v(amd, w, DR, B, S, tol)
        for k in range(K):
            _update(amd, w2, AX[:, k], PX[:, k])
            XYk, itk = _multi_r(amd, w2, DR, B, S, tol)
            assert np.array_equal(_bits(XY[:, k]), _bits(XYk[:, k])) and iters[k] == itk[k], f"column {k}"
            _check_column(_csc(prob, AX[:, k]), _p_full(prob, PX[:, k]), np.ascontiguousarray(DR[:, k]), n, B[:, k], XY[:, k], tol, None, None,
                          f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)
        amd.scs_free_lin_sys_work(w2)


# ---- refusals on a live workspace ----
def test_refusals_on_a_live_workspace():
    amd = _load("f64")  # libscsamd_linsys.so, and the HIP runtime handle of _hip()
    T = amd._scs_types
    fp = lambda a: a.ctypes.data_as(T.fp)
    n, m, tol, K = 50, 150, 1e-9, 3
    prob, dr, B, S = _case_data(n, m, 4, True, K)
    DR = _drs(n, m, m // 10, (0.03, 0.1, 1.0))
    AX = _perturbed(prob.Ax, K, np.random.default_rng(2))
    nnz = len(prob.Ax)
    w = _init(amd, prob, dr)
    try:
        _multi_v(amd, w, DR, B, S, tol, expect=-1)  # a solve before any set call
        Af = np.asfortranarray(AX)
        setv = amd.scs_amd_linsys_set_values_multi
        assert setv(w, K, None, nnz, None, 0) == -1
        assert setv(w, 0, fp(Af), nnz, None, 0) == -1 and setv(w, 17, fp(Af), nnz, None, 0) == -1
        assert setv(w, K, fp(Af), nnz - 1, None, 0) == -1
        assert setv(w, K, fp(Af), nnz, fp(Af), nnz) == -1  # PX for a workspace without P
        for bad in (np.nan, np.inf, -np.inf):
            A2 = AX.copy()
            A2[nnz - 1, K - 1] = bad
            _set_values(amd, w, A2, None, expect=-1)
        _multi_v(amd, w, DR, B, S, tol, expect=-1)  # the refused set calls stored nothing
        _set_values(amd, w, AX, None)
        for bad, where in ((0.0, (0, 0)), (-1.0, (n + m - 1, 2)), (np.nan, (n, 1)), (np.inf, (3, 2))):
            D2 = DR.copy()
            D2[where] = bad
            _multi_v(amd, w, D2, B, S, tol, expect=-1)  # asserts B, S and D2 unchanged
        _multi_v(amd, w, DR[:, :2], B[:, :2], S[:, :2], tol, expect=-1)  # another nrhs than the set call's
        Bf, Df, Sf, tv = np.asfortranarray(B), np.asfortranarray(DR), np.asfortranarray(S), np.full(K, tol)
        it = np.zeros(K, dtype=T.np_int)
        call = lambda lddr, ldb, lds: amd.scs_amd_solve_lin_sys_multi_v(w, K, fp(Df), lddr, fp(Bf), ldb, fp(Sf), lds, fp(tv), it.ctypes.data_as(T.ip))
        assert call(n + m - 1, n + m, n) == -1 and call(n + m, n + m - 1, n) == -1 and call(n + m, n + m, n - 1) == -1
        assert amd.scs_amd_solve_lin_sys_multi_v(w, K, fp(Df), n + m, None, n + m, fp(Sf), n, fp(tv), it.ctypes.data_as(T.ip)) == -1
        assert amd.scs_amd_solve_lin_sys_multi_v(w, K, fp(Df), n + m, fp(Bf), n + m, fp(Sf), n, None, it.ctypes.data_as(T.ip)) == -1
        assert np.array_equal(Bf, B)
        hip = _hip()
        d = hip.malloc((n + m) * 4 * 8)
        try:
            mv = amd.scs_amd_linsys_mat_vec_multi_v_dev
            assert mv(w, 2, d, d, d) == -1 and mv(w, 0, d, d, d) == -1 and mv(w, 17, d, d, d) == -1
            assert mv(w, K, d, None, d) == -1 and mv(w, K, d, d, None) == -1
        finally:
            hip.free(d)
        XY, _ = _multi_v(amd, w, DR, B, S, tol)  # the next call works, on the values of the last accepted set call
        for k in range(K):
            _check_column(_csc(prob, AX[:, k]), None, np.ascontiguousarray(DR[:, k]), n, B[:, k], XY[:, k], tol, None, None, f"column {k}")
    finally:
        amd.scs_free_lin_sys_work(w)
    # a workspace with P refuses a set call without PX
    prob, P, dr, B, S = _p_case()
    w = _init(amd, prob, dr, True)
    try:
        Af = np.asfortranarray(np.tile(prob.Ax[:, None], (1, 2)))
        Pf = np.asfortranarray(np.tile(prob.Px[:, None], (1, 2)))
        assert amd.scs_amd_linsys_set_values_multi(w, 2, fp(Af), len(prob.Ax), None, 0) == -1
        assert amd.scs_amd_linsys_set_values_multi(w, 2, fp(Af), len(prob.Ax), fp(Pf), len(prob.Px) - 1) == -1
        assert amd.scs_amd_linsys_set_values_multi(w, 2, fp(Af), len(prob.Ax), fp(Pf), len(prob.Px)) == 0
    finally:
        amd.scs_free_lin_sys_work(w)


# ---- free, then set again at a wider nrhs ----
def test_free_then_set_again_wider():
    amd = capi.load("libscsamd_linsys.so")
    n, m, tol = 1000, 3000, 1e-9
    prob, dr, B, S = _case_data(n, m, 32, True, 16)
    DR = _drs(n, m, m // 10, np.geomspace(0.01, 1.0, 16))
    AX = _perturbed(prob.Ax, 16, np.random.default_rng(6))
    w, w2 = _init(amd, prob, dr), _init(amd, prob, dr)
    try:
        amd.scs_amd_linsys_free_values_multi(w)  # nothing to free yet
        amd.scs_amd_linsys_free_values_multi(None)
        for K in (3, 16, 2):  # wider (rebuilt), then narrower on the wider blocks
            _set_values(amd, w, AX[:, :K], None, ldax=len(prob.Ax) + 5)
            XY, iters = _multi_v(amd, w, DR[:, :K], B[:, :K], S[:, :K], tol, lddr=n + m + 3, ldb=n + m + 7, lds=n + 1)
            k = K - 1
            _update(amd, w2, AX[:, k])
            XYk, itk = _multi_r(amd, w2, DR[:, :K], B[:, :K], S[:, :K], tol)
            assert np.array_equal(_bits(XY[:, k]), _bits(XYk[:, k])) and iters[k] == itk[k], f"nrhs {K}"
            if K == 3:
                amd.scs_amd_linsys_free_values_multi(w)
                _multi_v(amd, w, DR[:, :K], B[:, :K], S[:, :K], tol, expect=-1)  # freed: a solve needs a new set call
    finally:
        amd.scs_free_lin_sys_work(w)
        amd.scs_free_lin_sys_work(w2)


# ---- device memory ----
def test_value_blocks_are_allocated_by_the_first_set_call_and_released_by_the_free_entry():
    """the value blocks of this system at width 16 hold 2 nnz 16 x 8 bytes = 77 MB, beside one staged column (nnz x 8 bytes);
    allowance for the runtime's own caches as in test_block_buffers_are_freed_with_the_workspace"""
    amd = capi.load("libscsamd_linsys.so")
    n, m, K = 30000, 60000, 16
    prob, dr, B, S = _case_data(n, m, 10, True, K)
    DR = _drs(n, m, m // 10, np.geomspace(0.01, 1.0, K))
    AX = _perturbed(prob.Ax, K, np.random.default_rng(12))
    nnz = len(prob.Ax)
    slack = 8 << 20
    free_bytes = lambda: amd.scs_amd_device_free_bytes()
    w = _init(amd, prob, dr)  # warm: context, streams, code objects of every path used below
    _multi_r(amd, w, DR[:, :2], B[:, :2], S[:, :2], 1e-6)
    _update(amd, w, prob.Ax)
    _set_values(amd, w, AX[:, :2], None)
    _multi_v(amd, w, DR[:, :2], B[:, :2], S[:, :2], 1e-6)
    amd.scs_free_lin_sys_work(w)
    base = free_bytes()
    w = _init(amd, prob, dr)
    _multi_r(amd, w, DR, B, S, 1e-6)  # the block buffers and the R blocks at width 16
    _update(amd, w, prob.Ax)          # the position maps of scs_amd_linsys_update_values
    before = free_bytes()
    _multi_r(amd, w, DR, B, S, 1e-6)
    assert abs(free_bytes() - before) <= slack  # a caller who never sets values allocates what they allocated
    _set_values(amd, w, AX, None)
    with_v = free_bytes()
    v_bytes = 2 * nnz * K * 8
    assert v_bytes * 0.9 <= before - with_v <= v_bytes + nnz * 8 + slack
    _multi_v(amd, w, DR, B, S, 1e-6)
    _set_values(amd, w, AX[:, :3], None)  # narrower: on the blocks that are there
    assert abs(free_bytes() - with_v) <= slack
    amd.scs_amd_linsys_free_values_multi(w)
    assert abs(free_bytes() - before) <= slack
    amd.scs_free_lin_sys_work(w)
    assert abs(free_bytes() - base) <= slack


# ---- the Python object ----
def test_python_object():
    from scs_amd.linsys import LinSys
    K, tol = 3, 1e-9
    prob, dr, B, S, DR, AX, PX = _p_setup(K)
    n, m = prob.n, prob.m
    Asp, Pup = prob.sparse(), sp.csc_matrix((prob.Px, prob.Pi, prob.Pp), shape=(n, n))
    with LinSys(Asp, dr, P=Pup) as ls, LinSys(Asp, dr, P=Pup) as ls2:
        with pytest.raises(ValueError):
            ls.solve_many(B, S, tol, diag_r=DR, own_values=True)  # before any set call
        ls.set_values_many(AX, PX)
        XY, iters = ls.solve_many(B, S, tol, diag_r=DR, own_values=True)
        XYn, itn = ls.solve_many(B, S, tol, own_values=True)
        for k in range(K):
            ls2.update_values(AX[:, k], PX[:, k])
            want, want_it = ls2.solve_many(B, S, tol, diag_r=DR)
            assert np.array_equal(_bits(XY[:, k]), _bits(want[:, k])) and iters[k] == want_it[k]
            want, want_it = ls2.solve_many(B, S, tol, diag_r=np.tile(dr[:, None], (1, K)))
            assert np.array_equal(_bits(XYn[:, k]), _bits(want[:, k])) and itn[k] == want_it[k]
        for bad_a, bad_p in ((AX[:-1], PX), (AX, PX[:, :2]), (AX, None), (np.where(AX > 0, np.nan, AX), PX), (np.tile(AX, (1, 6)), np.tile(PX, (1, 6)))):
            with pytest.raises(ValueError):
                ls.set_values_many(bad_a, bad_p)
        with pytest.raises(ValueError):
            ls.solve_many(B[:, :2], S[:, :2], tol, own_values=True)  # another K than the set call's
        ls.free_values_many()
        with pytest.raises(ValueError):
            ls.solve_many(B, S, tol, own_values=True)
        ls.set_values_many(AX, PX)
        again, again_it = ls.solve_many(B, S, tol, diag_r=DR, own_values=True)
        assert np.array_equal(_bits(again), _bits(XY)) and np.array_equal(again_it, iters)
