"""New values on a live linear-system workspace (scs_amd_linsys_update_values, include/scs_amd.h): afterwards the workspace cannot be
told from one scs_init_lin_sys_work created on the new values.

Two matrices: the scrambled banded SOCP matrix of tests/test_reorder_gpu.py's shape (30000 x 60000 transposed: m = 60000, n = 30000,
no P) and a 4000 x 2000 one with an upper-triangular P of about 5 entries per column.  After the update
  * mat_vec_dev, mul_a_dev, mul_at_dev and their _multi_dev forms (4 columns) against long-double products of the NEW matrices, row
    by row at the rounding bound tests/test_spmv_exact_gpu.py uses for the same kernels (tests/spmv_exact.py);
  * scs_solve_lin_sys (cold and warm, tol 1e-9) and scs_amd_solve_lin_sys_multi (5 columns): the bits of a fresh workspace;
the same after scs_update_lin_sys_diag_r (the preconditioner must see the new values under the diag_r in force), and once per forced
SpMV flavour, which reaches every value array that exists (stream, plain wave, lockstep, wide, and the layouts of the host builder)."""
import ctypes as C

import numpy as np
import pytest

from scs_amd import capi
from tests import probgen
from tests import spmv_exact as sx
from tests import test_spmv_exact_gpu as single_suite
from tests import test_linsys_multi_gpu as multi_suite
from tests import test_update_matrix_gpu as um

pytestmark = pytest.mark.gpu

FLAVOURS = {
    "default": ({}, "-"),
    "stream": (single_suite.FLAVOURS["stream"][0], "-"),
    "wave_p0": (single_suite.FLAVOURS["wave_p0"][0], "dev"),
    "wave_p0_host": (single_suite.FLAVOURS["wave_p0"][0], "host"),
    "ls_16_4": (single_suite.FLAVOURS["ls_16_4"][0], "dev"),
    "ls_16_4_host": (single_suite.FLAVOURS["ls_16_4"][0], "host"),
    "wide": (single_suite.FLAVOURS["wide"][0], "dev"),
}
KERNEL = {"stream": "csr_stream_kernel<EPI>", "wave_p0": "csr_wave_kernel<EPI,0>", "wave_p0_host": "csr_wave_kernel<EPI,0>",
          "ls_16_4": "csr_wave_lockstep_kernel<EPI,16,4>", "ls_16_4_host": "csr_wave_lockstep_kernel<EPI,16,4>", "wide": "csr_wave_wide_kernel<EPI>"}

_cache = {}


def _matrices(which):
    """(A0, P0 | None, A1 values, P1 values | None, diag_r, a second diag_r)"""
    if which not in _cache:
        if which == "band":
            pr, A1x = um.renumbered()
            A0, P0, P1x = pr["A"], None, None
        else:
            pr, A1x, P0, P1x = um.with_p()
            A0 = pr["A"]
        m, n = A0.shape
        A0 = A0.astype(np.float64)
        dr = probgen.diag_r(n, m, pr["cone"]["z"])
        dr2 = probgen.diag_r(n, m, pr["cone"]["z"], scale=0.7)
        rng = np.random.default_rng(17)
        vec = dict(x=rng.standard_normal(n), y=rng.standard_normal(m), b=rng.standard_normal(n + m), s=0.1 * rng.standard_normal(n),
                   B=rng.standard_normal((n + m, 5)), S=0.1 * rng.standard_normal((n, 5)))
        _cache[which] = (A0, P0, A1x, P1x, dr, dr2, vec)
    return _cache[which]


def _update(ws, Ax, Px):
    T = ws.L._scs_types
    ax = None if Ax is None else np.ascontiguousarray(Ax, dtype=T.np_float)
    px = None if Px is None else np.ascontiguousarray(Px, dtype=T.np_float)
    return ws.L.scs_amd_linsys_update_values(ws.w, None if ax is None else ax.ctypes.data_as(T.fp), None if px is None else px.ctypes.data_as(T.fp))


def _products_within_bound(ws, ops, vec):
    """every product entry of the workspace against the long-double product of `ops` (the NEW matrices), single and 4 columns"""
    ws.ops = ops
    x, y = vec["x"], vec["y"]
    u = sx.UNIT_ROUNDOFF[np.float64]
    ax, aty, mv = ops.longdouble(x, y)
    b_a, b_at, b_mv = ops.bounds(x, y, u)
    sx.check_bound(ws.apply("mul_a", x), ax, b_a, "A x")
    sx.check_bound(ws.apply("mul_at", y), aty, b_at, "A' y")
    sx.check_bound(ws.apply("mat_vec", x), mv, b_mv, "R_x x + P x + A' R_y^-1 A x")
    xs, ys = [x, -0.5 * x, x[::-1].copy(), 2.0 * x], [y, 3.0 * y, y[::-1].copy(), -y]
    for op, cols in (("mul_a", xs), ("mul_at", ys), ("mat_vec", xs)):
        Y = multi_suite._apply_block(ws, op, cols)
        for k in range(4):
            r = ops.longdouble(xs[k], ys[k])
            b = ops.bounds(xs[k], ys[k], u)
            i = {"mul_a": 0, "mul_at": 1, "mat_vec": 2}[op]
            sx.check_bound(Y[:, k], r[i], b[i], f"{op}, column {k} of 4")


def _solves(ws, vec):
    """cold solve, warm solve, block solve of 5 columns: the bytes of every result"""
    L, T = ws.L, ws.L._scs_types
    out = []
    for s in (None, vec["s"]):
        b = vec["b"].copy()
        assert L.scs_solve_lin_sys(ws.w, b.ctypes.data_as(T.fp), None if s is None else s.ctypes.data_as(T.fp), 1e-9) == 0
        out.append(b)
    B = np.asfortranarray(vec["B"].copy())
    S = np.asfortranarray(vec["S"])
    tol = np.full(5, 1e-9)
    its = np.zeros(5, dtype=T.np_int)
    n_m, n = B.shape[0], S.shape[0]
    assert L.scs_amd_solve_lin_sys_multi(ws.w, 5, B.ctypes.data_as(T.fp), n_m, S.ctypes.data_as(T.fp), n, tol.ctypes.data_as(T.fp),
                                         its.ctypes.data_as(T.ip)) == 0
    out += [B, its]
    return out


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.tobytes() == v.tobytes(), f"{what}: result {i} (cold, warm, block, block iterations) differs from the fresh workspace's"


def _run(monkeypatch, which, flavour, with_diag_r=False):
    env, build = FLAVOURS[flavour]
    single_suite._force(monkeypatch, env, build)
    L = single_suite._load("f64")
    A0, P0, A1x, P1x, dr, dr2, vec = _matrices(which)
    A1 = um.with_values(A0, A1x)
    P1 = None if P0 is None else um.with_values(P0, P1x)
    dr_new = dr2 if with_diag_r else dr
    ws = single_suite.Workspace(L, sx.Operators(A0, P0, dr), np.float64)
    ref = single_suite.Workspace(L, sx.Operators(A1, P1, dr_new), np.float64)
    try:
        if flavour in KERNEL:
            single_suite._expect(ws, KERNEL[flavour], KERNEL[flavour])
        first = _solves(ws, vec)
        if with_diag_r:
            assert L.scs_update_lin_sys_diag_r(ws.w, dr2.ctypes.data_as(capi.T64.fp)) == 0
        assert _update(ws, A1x, P1x) == 0
        _products_within_bound(ws, ref.ops, vec)
        got, want = _solves(ws, vec), _solves(ref, vec)
        assert got[0].tobytes() != first[0].tobytes(), "the update changed nothing"
        _same(got, want, f"{which}/{flavour}")
        if not with_diag_r:  # and back, one matrix at a time where there are two
            assert _update(ws, A0.data, None) == 0
            if P0 is not None:
                assert _update(ws, None, P0.data) == 0
            _same(_solves(ws, vec), first, f"{which}/{flavour}, back to the first values")
    finally:
        ws.free()
        ref.free()


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("which", ["band", "p"])
def test_update_values_equals_a_fresh_workspace(monkeypatch, which, flavour):
    _run(monkeypatch, which, flavour)


@pytest.mark.parametrize("which", ["band", "p"])
def test_update_after_a_new_diag_r_builds_the_preconditioner_from_both(monkeypatch, which):
    _run(monkeypatch, which, "default", with_diag_r=True)


def test_refusals():
    L = single_suite._load("f64")
    A0, P0, A1x, P1x, dr, dr2, vec = _matrices("band")
    ws = single_suite.Workspace(L, sx.Operators(A0, None, dr), np.float64)
    try:
        first = _solves(ws, vec)
        bad = A1x.copy()
        bad[7] = np.inf
        assert _update(ws, bad, None) == -1
        assert _update(ws, None, np.ones(4)) == -1  # no P
        assert _update(ws, None, None) == 0
        _same(_solves(ws, vec), first, "after refused updates")
    finally:
        ws.free()
    assert L.scs_amd_linsys_update_values(None, None, None) == -1


def test_linsys_object_round_trip():
    from scs_amd.linsys import LinSys
    A0, P0, A1x, P1x, dr, dr2, vec = _matrices("p")
    A1, P1 = um.with_values(A0, A1x), um.with_values(P0, P1x)
    with LinSys(A0, dr, P=P0) as ls, LinSys(A1, dr, P=P1) as want:
        first = ls.solve(vec["b"], tol=1e-9)
        ls.update_values(A_values=A1, P_values=P1x)
        assert ls.solve(vec["b"], tol=1e-9).tobytes() == want.solve(vec["b"], tol=1e-9).tobytes()
        XY, its = ls.solve_many(vec["B"], tol=1e-9)
        XYw, itsw = want.solve_many(vec["B"], tol=1e-9)
        assert XY.tobytes() == XYw.tobytes() and np.array_equal(its, itsw)
        with pytest.raises(ValueError):
            ls.update_values(A_values=A1x[:-1])
        with pytest.raises(ValueError):
            ls.update_values(P_values=A1)
        ls.update_values(A_values=A0.data, P_values=P0)
        assert ls.solve(vec["b"], tol=1e-9).tobytes() == first.tobytes()
