"""The lockstep product's register-slot epilogue (spmv_wave.h, wave_lockstep_rounds): rows per unit at and around every slot boundary.

csr_wave_lockstep_kernel<EPI_DIV | EPI_GP, ...> loads the epilogue operands of a lane's rows r0 + lane + 64 j, j < SLOTS, ahead of its
chunk loop, with SLOTS the smallest of 4 | 9 | 16 that covers the longest unit (EPI_GP stops at 9: rows from 576 on take the late loads).
What can go wrong there and tests/test_spmv_exact_gpu.py does not reach: a unit of exactly 64 j and 64 j + 1 rows for the j at which the
slot count changes (4 -> 9 at 256 / 257, 9 -> 16 or the late path at 576 / 577, the cap at 1023 / 1024), a last unit of 7 rows beside
full ones, waves without a unit in the same workgroup, and y0 live in EPI_GP (P present).

The pattern has exactly one entry per row of the orientation under test, column = a fixed hash of the row, so that under
SCS_AMD_WR_NNZ = R a unit holds exactly R rows: rows = 3 R + 7 gives three full units and one of 7 rows (4 live waves of 16 or 8).
The other orientation then has 37 long rows, a few per unit: the other extreme.  Checks (a), (b), (c) of tests/test_spmv_exact_gpu.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi
from tests import spmv_exact as sx
from tests.test_spmv_exact_gpu import FLAVOURS, LIBS, Workspace, _bound_checks, _exact_checks, _expect, _force, _load

gpu = pytest.mark.gpu  # (the first test below checks the patterns against the exact helpers on the host and carries no mark)

NCOL = 37
R_ALL = [64, 65, 128, 129, 256, 257, 512, 513, 576, 577, 1023, 1024]


def one_entry_per_row(rows):
    """rows x 37 pattern, one entry per row, column = a fixed hash of the row"""
    r = np.arange(rows, dtype=np.int64)
    c = ((r * 2654435761) % (1 << 32) >> 7) % NCOL
    M = sp.coo_matrix((np.ones(rows), (r, c)), shape=(rows, NCOL)).tocsc()
    assert M.nnz == rows and np.all(np.diff(M.tocsr().indptr) == 1)
    return M


_cache = {}


def _problems(lib, R, transposed):
    """(integer problem, its exact products, real problem) of one (library, R, orientation): built once, shared by the flavours"""
    key = (lib, R, transposed)
    if key not in _cache:
        dtype = LIBS[lib][1]
        A_pat = one_entry_per_row(3 * R + 7)
        if transposed:
            A_pat = sp.csc_matrix(A_pat.T)
        P_pat = sx.p_pattern("dup_diag", A_pat.shape[1])
        rng = np.random.default_rng(1000 * R + 2 * (lib == "f32") + transposed)
        ops, x, y = sx.exact_problem(A_pat, P_pat, rng, dtype)
        _cache[key] = ((ops, x, y, ops.exact(x, y)), sx.cast(*sx.real_problem(A_pat, P_pat, rng), dtype))
    return _cache[key]


def _run(monkeypatch, lib, flavour, R, transposed):
    L = _load(lib)
    dtype = LIBS[lib][1]
    env, name = FLAVOURS[flavour]
    _force(monkeypatch, {**env, "WR_NNZ": str(R)}, "dev")
    (ops, x, y, refs), (rops, rx, ry) = _problems(lib, R, transposed)
    ws = Workspace(L, ops, dtype)
    try:
        _expect(ws, name, name)
        _exact_checks(ws, x, y, dtype, refs)
    finally:
        ws.free()
    ws = Workspace(L, rops, dtype)
    try:
        _expect(ws, name, name)
        _bound_checks(ws, rx, ry, dtype)
    finally:
        ws.free()


def test_patterns_are_accepted_by_the_exact_helpers():
    """no GPU in this one's way: every (library, R, orientation) used below builds its integer problem inside the precision's exact range"""
    for lib, Rs, tr in (("f64", R_ALL, False), ("f64", [64, 513, 1024], True), ("f32", [65, 513, 1024], False)):
        for R in Rs:
            (ops, x, y, refs), (rops, rx, ry) = _problems(lib, R, tr)
            assert (ops.m, ops.n) == ((NCOL, 3 * R + 7) if tr else (3 * R + 7, NCOL))
            assert all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in refs + rops.longdouble(rx, ry))


@gpu
@pytest.mark.parametrize("R", R_ALL)
@pytest.mark.parametrize("flavour", ["ls_16_4", "ls_16_1", "ls_8_4"])
def test_rows_per_unit_at_slot_boundaries(monkeypatch, flavour, R):
    """units of A hold exactly R rows (EPI_DIV: 4, 9 and 16 slots); A' has 37 long rows (EPI_GP with y0)"""
    _run(monkeypatch, "f64", flavour, R, False)


@gpu
@pytest.mark.parametrize("R", [64, 513, 1024])
def test_rows_per_unit_transposed(monkeypatch, R):
    """units of A' hold exactly R rows (EPI_GP with y0: 4 and 9 slots, and rows 576 .. 1023 on the late loads)"""
    _run(monkeypatch, "f64", "ls_16_4", R, True)


@gpu
@pytest.mark.parametrize("R", [65, 513, 1024])
def test_rows_per_unit_fp32(monkeypatch, R):
    _run(monkeypatch, "f32", "ls_16_4", R, False)


@gpu
def test_solve_keeps_acc_and_negdiv(monkeypatch):
    """EPI_ACC and EPI_NEGDIV (no register slots) through one scs_solve_lin_sys on the R = 513 problem, checked as
    tests/test_spmv_exact_gpu.py::test_solve_epilogues does"""
    L = _load("f64")
    env, name = FLAVOURS["ls_16_4"]
    _force(monkeypatch, {**env, "WR_NNZ": "513"}, "dev")
    monkeypatch.setenv("SCS_AMD_FUSED", "0")
    A_pat = one_entry_per_row(3 * 513 + 7)
    m, n = A_pat.shape
    P_pat = sx.p_pattern("dup_diag", n)
    rng = np.random.default_rng(11)
    A = A_pat.astype(np.float64).tocsc(copy=True)
    A.data = rng.uniform(-1, 1, A.nnz)
    P = P_pat.astype(np.float64).tocsc(copy=True)
    P.data = np.where(P.data == 0, 0.0, rng.uniform(0, 1, P.nnz)) * (P.indices == np.repeat(np.arange(n), np.diff(P.indptr)))
    diag_r = np.concatenate([np.full(n, 1.0), 2.0 ** rng.integers(-1, 4, m)])
    ops = sx.Operators(A, P, diag_r)
    ws = Workspace(L, ops, np.float64)
    try:
        _expect(ws, name, name)
        b = rng.uniform(-1, 1, n + m)
        out = b.copy()
        tol = 1e-8
        assert L.scs_solve_lin_sys(ws.w, out.ctypes.data_as(capi.T64.fp), None, tol) == 0
    finally:
        ws.free()
    x, y = out[:n], out[n:]
    u = sx.UNIT_ROUNDOFF[np.float64]
    LD = sx.LD
    ia, ja, va = ops.a
    it, jt, vt = ops.at
    ip, jp, vp = ops.p
    absA, absAt, absP = ops.abs_products(x)
    ry = diag_r[n:]
    y_ref = (sx.row_products(ia, ja, va, x, LD) - b[n:].astype(LD)) / ry.astype(LD)
    sx.check_bound(y, y_ref, sx.C_ROUND * u * (ops.ka + 2) * (absA(x) + np.abs(b[n:])) / ry, "y = R_y^-1 (A x - b_y)")
    rhs = b[:n].astype(LD) + sx.row_products(it, jt, vt, b[n:].astype(LD) / ry.astype(LD), LD)
    gx = (diag_r[:n].astype(LD) * x.astype(LD) + sx.row_products(ip, jp, vp, x, LD)
          + sx.row_products(it, jt, vt, sx.row_products(ia, ja, va, x, LD) / ry.astype(LD), LD))
    res = np.abs(gx - rhs).max()
    scale = (np.abs(diag_r[:n] * x) + absP(x) + absAt(absA(x) / ry) + np.abs(b[:n]) + absAt(np.abs(b[n:]) / ry)).max()
    k = int(max(ops.kat.max(initial=0), ops.ka.max(initial=0), ops.kp.max(initial=0))) + 2
    assert res <= tol + sx.C_ROUND * k * u * scale, (float(res), tol)
