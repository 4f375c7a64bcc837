"""Every SpMV kernel flavour against an exact product, on shapes built to hit each flavour's own edge.

The linear-system workspace (scs_init_lin_sys_work) applies its CSR products to caller buffers through scs_amd_linsys_mul_a_dev,
_mul_at_dev and _mat_vec_dev (include/scs_amd.h); scs_amd_linsys_spmv_kernel_name says which kernel ran, and every case asserts it is the
one it forced.  Three checks per (library, flavour, shape), helpers in tests/spmv_exact.py:
  (a) integer data: the result equals the exact product bit for bit (no dropped, duplicated or misrouted entry hides under a tolerance);
  (b) real data over 1e-8 .. 1e8: every row within C_ROUND k u (|A||x|) of a long-double reference, and a second call gives the same bits;
  (c) NaN sentinels: the output is NaN-filled before the call (every row, empty ones included, must be written), a NaN guard behind the
      output must stay untouched, and a NaN guard right behind the input in the same allocation must not reach the result (nothing is
      gathered past the vector's end).
Device buffers come from the HIP runtime the library already links (ctypes); the entries' stream contract is kept: inputs are written
and the device synchronised before a call, scs_amd_linsys_sync before the output is read."""
import ctypes as C
import zlib

import numpy as np
import pytest

from scs_amd import capi
from tests import spmv_exact as sx

pytestmark = pytest.mark.gpu

GUARD = 256  # NaN entries behind every input and output vector

LIBS = {"f64": ("libscsamd_linsys.so", np.float64), "f32": ("libscsamd_f32.so", np.float32), "dlong": ("libscsamd_dlong.so", np.float64)}

_W = {"WAVEROWS": "1"}
_P0 = {**_W, "WR_LOCKSTEP": "0"}
FLAVOURS = {
    # name: (SCS_AMD_* forcing, kernel name the workspace must report for both orientations)
    "stream": ({"WAVEROWS": "0"}, "csr_stream_kernel<EPI>"),
    "stream_grid1": ({"WAVEROWS": "0", "SPMV_MAX_GRID": "1"}, "csr_stream_kernel<EPI>"),  # one workgroup strides over every row-block
    "stream_grid3": ({"WAVEROWS": "0", "SPMV_MAX_GRID": "3"}, "csr_stream_kernel<EPI>"),
    "wave_p0": ({**_P0, "WR_PIPE": "0"}, "csr_wave_kernel<EPI,0>"),
    "wave_p1": ({**_P0, "WR_PIPE": "1"}, "csr_wave_kernel<EPI,1>"),
    "wave_p2": ({**_P0, "WR_PIPE": "2"}, "csr_wave_kernel<EPI,2>"),
    "wave_p0_nnz64": ({**_P0, "WR_PIPE": "0", "WR_NNZ": "64"}, "csr_wave_kernel<EPI,0>"),  # many units, long rows alone in theirs
    "ls_16_4": ({**_W, "WR_LOCKSTEP": "1", "WR_LS_WPB": "16", "WR_LS_BARRIERS": "4"}, "csr_wave_lockstep_kernel<EPI,16,4>"),
    "ls_16_1": ({**_W, "WR_LOCKSTEP": "1", "WR_LS_WPB": "16", "WR_LS_BARRIERS": "1"}, "csr_wave_lockstep_kernel<EPI,16,1>"),
    "ls_8_4": ({**_W, "WR_LOCKSTEP": "1", "WR_LS_WPB": "8", "WR_LS_BARRIERS": "4"}, "csr_wave_lockstep_kernel<EPI,8,4>"),
    "ls_8_1": ({**_W, "WR_LOCKSTEP": "1", "WR_LS_WPB": "8", "WR_LS_BARRIERS": "1"}, "csr_wave_lockstep_kernel<EPI,8,1>"),
    "ls_16_4_no_order": ({**_W, "WR_LOCKSTEP": "1", "WR_LS_BARRIERS": "4", "WR_LS_ORDER": "0"}, "csr_wave_lockstep_kernel<EPI,16,4>"),
    "ls_16_1_nnz64": ({**_W, "WR_LOCKSTEP": "1", "WR_LS_BARRIERS": "1", "WR_NNZ": "64"}, "csr_wave_lockstep_kernel<EPI,16,1>"),
    "ls_order_plain": ({**_W, "WR_LOCKSTEP": "2", "WR_PIPE": "1"}, "csr_wave_kernel<EPI,1>"),  # the lockstep chunk order, plain kernel
    "wide": ({**_W, "WR_WIDE": "1"}, "csr_wave_wide_kernel<EPI>"),
}
STREAM = [f for f in FLAVOURS if f.startswith("stream")]
WAVE = [f for f in FLAVOURS if not f.startswith("stream")]

SHAPES = ["1x1", "m1", "n1", "empty", "longrows", "dense", "mod4", "random"]
P_OF_SHAPE = {"1x1": "dup_diag", "m1": "dense_col", "n1": "none", "empty": "zero_diag", "longrows": "diag", "dense": "dense_col",
              "mod4": "none", "random": "dup_diag"}


def _cases(lib, flavours, builds):
    out = []
    for f in flavours:
        for b in (builds if f in WAVE else ["-"]):
            for s in SHAPES:
                out.append(pytest.param(lib, f, b, s, id=f"{lib}-{f}-{b}-{s}"))
    return out


CASES = (_cases("f64", FLAVOURS, ["dev", "host"])
         + _cases("f32", ["stream", "stream_grid3", "wave_p0", "wave_p1", "wave_p2", "ls_16_4", "ls_8_1", "ls_order_plain", "wide"], ["dev"])
         + _cases("f32", ["wave_p0", "ls_16_4"], ["host"]))
DLONG_CASES = _cases("dlong", ["stream", "wave_p0", "ls_16_4"], ["dev"])


# ---- device memory through the HIP runtime the library links ----
class _Hip:
    H2D, D2H = 1, 2

    def __init__(self):
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        assert path, "the HIP runtime is not mapped (load a product library first)"
        self.rt = C.CDLL(path)
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0 and p.value
        return p.value

    def put(self, dptr, arr):
        assert self.rt.hipMemcpy(dptr, arr.ctypes.data, arr.nbytes, self.H2D) == 0

    def get(self, arr, dptr):
        assert self.rt.hipMemcpy(arr.ctypes.data, dptr, arr.nbytes, self.D2H) == 0

    def free(self, dptr):
        assert self.rt.hipFree(dptr) == 0

    def sync(self):
        assert self.rt.hipDeviceSynchronize() == 0


_hip = None


def _load(lib):
    global _hip
    L = capi.load(LIBS[lib][0])
    if _hip is None:
        _hip = _Hip()
    return L


class Workspace:
    """scs_init_lin_sys_work on (A, P, diag_r) under the forcing in force"""

    def __init__(self, L, ops, dtype):
        T = L._scs_types
        self.L, self.dtype, self.ops = L, dtype, ops
        self._keep = []

        def mat(M):
            x = np.ascontiguousarray(M.data, dtype=T.np_float)
            i = np.ascontiguousarray(M.indices, dtype=T.np_int)
            p = np.ascontiguousarray(M.indptr, dtype=T.np_int)
            self._keep += [x, i, p]
            return T.ScsMatrix(x.ctypes.data_as(T.fp), i.ctypes.data_as(T.ip), p.ctypes.data_as(T.ip), M.shape[0], M.shape[1])

        self._A = mat(ops.A)
        self._P = mat(ops.P) if ops.P is not None else None
        dr = ops.diag_r.astype(T.np_float)
        self.w = L.scs_init_lin_sys_work(C.byref(self._A), C.byref(self._P) if self._P is not None else None, dr.ctypes.data_as(T.fp))
        assert self.w, "scs_init_lin_sys_work returned NULL"

    def kernel(self, which):
        buf = C.create_string_buffer(128)
        n = self.L.scs_amd_linsys_spmv_kernel_name(self.w, which, buf, 128)
        assert 0 < n < 128
        return buf.value.decode()

    def apply(self, op, v):
        """op in (mul_a, mul_at, mat_vec) on v, with the NaN sentinels of check (c); called twice, the two results must agree bit for bit"""
        fn, out_len = {"mul_a": (self.L.scs_amd_linsys_mul_a_dev, self.ops.m), "mul_at": (self.L.scs_amd_linsys_mul_at_dev, self.ops.n),
                       "mat_vec": (self.L.scs_amd_linsys_mat_vec_dev, self.ops.n)}[op]
        dt = self.dtype
        isz = np.dtype(dt).itemsize
        inp = np.concatenate([v.astype(dt), np.full(GUARD, np.nan, dt)])  # the input's guard: in the same allocation, right behind it
        nan_out = np.full(out_len + GUARD, np.nan, dt)
        din, dout = _hip.malloc(inp.nbytes), _hip.malloc(nan_out.nbytes)
        try:
            _hip.put(din, inp)
            res = []
            for _ in range(2):
                _hip.put(dout, nan_out)
                _hip.sync()  # the entries run on the workspace's own stream: the caller's writes must be complete
                assert fn(self.w, din, dout) == 0
                assert self.L.scs_amd_linsys_sync(self.w) == 0
                got = np.empty(out_len + GUARD, dt)
                _hip.get(got, dout)
                res.append(got)
        finally:
            _hip.free(din)
            _hip.free(dout)
        ib = np.uint64 if isz == 8 else np.uint32
        for got in res:
            assert np.array_equal(got[out_len:].view(ib), nan_out[out_len:].view(ib)), f"{op}: the guard behind the output was written"
            bad = np.flatnonzero(~np.isfinite(got[:out_len]))
            assert bad.size == 0, f"{op}: {bad.size} rows not written or gathered past the input's end (NaN), first {bad[:5].tolist()}"
        assert np.array_equal(res[0][:out_len].view(ib), res[1][:out_len].view(ib)), f"{op}: a second call gave different bits"
        return res[0][:out_len]

    def free(self):
        if self.w:
            self.L.scs_free_lin_sys_work(self.w)
            self.w = None


def _force(monkeypatch, env, build):
    for k, v in env.items():
        monkeypatch.setenv("SCS_AMD_" + k, v)
    if build != "-":
        monkeypatch.setenv("SCS_AMD_WR_BUILD", build)


def _expect(ws, want_a, want_at):
    got = (ws.kernel(0), ws.kernel(1))
    assert got == (want_a, want_at), f"forced kernels {(want_a, want_at)}, the workspace runs {got}"


def _exact_checks(ws, x, y, dtype, refs=None):
    ax, aty, mv = refs or ws.ops.exact(x, y)
    sx.check_exact(ws.apply("mul_a", x), ax, dtype, "A x")
    sx.check_exact(ws.apply("mul_at", y), aty, dtype, "A' y")
    sx.check_exact(ws.apply("mat_vec", x), mv, dtype, "R_x x + P x + A' R_y^-1 A x")


def _bound_checks(ws, x, y, dtype):
    ops = ws.ops
    ax, aty, mv = ops.longdouble(x, y)
    b_a, b_at, b_mv = ops.bounds(x, y, sx.UNIT_ROUNDOFF[dtype])
    sx.check_bound(ws.apply("mul_a", x), ax, b_a, "A x")
    sx.check_bound(ws.apply("mul_at", y), aty, b_at, "A' y")
    sx.check_bound(ws.apply("mat_vec", x), mv, b_mv, "R_x x + P x + A' R_y^-1 A x")


_shape_cache = {}


def _pattern(name):
    if name not in _shape_cache:
        A = sx.shape(name)
        _shape_cache[name] = (A, sx.p_pattern(P_OF_SHAPE[name], A.shape[1]))
    return _shape_cache[name]


@pytest.mark.parametrize("lib,flavour,build,shape", CASES)
def test_flavour_exact_and_bounded(monkeypatch, lib, flavour, build, shape):
    L = _load(lib)
    dtype = LIBS[lib][1]
    env, name = FLAVOURS[flavour]
    _force(monkeypatch, env, build)
    A_pat, P_pat = _pattern(shape)
    rng = np.random.default_rng(zlib.crc32(f"{lib}-{flavour}-{build}-{shape}".encode()))
    ops, x, y = sx.exact_problem(A_pat, P_pat, rng, dtype)
    ws = Workspace(L, ops, dtype)
    try:
        _expect(ws, name, name)
        _exact_checks(ws, x, y, dtype)
    finally:
        ws.free()
    ops, x, y = sx.cast(*sx.real_problem(A_pat, P_pat, rng), dtype)
    ws = Workspace(L, ops, dtype)
    try:
        _expect(ws, name, name)
        _bound_checks(ws, x, y, dtype)
    finally:
        ws.free()


@pytest.mark.parametrize("lib,flavour,build,shape", DLONG_CASES)
def test_dlong_flavour_exact(monkeypatch, lib, flavour, build, shape):
    """64-bit scs_int at the ABI (and 64-bit entry positions inside): check (a); without the offset-bias hook (test_dlong_gpu.py pins it)"""
    L = _load(lib)
    env, name = FLAVOURS[flavour]
    _force(monkeypatch, env, build)
    A_pat, P_pat = _pattern(shape)
    ops, x, y = sx.exact_problem(A_pat, P_pat, np.random.default_rng(5), np.float64)
    ws = Workspace(L, ops, np.float64)
    try:
        _expect(ws, name, name)
        _exact_checks(ws, x, y, np.float64)
    finally:
        ws.free()


# ---- gathered-vector lengths at the packing edges (tall A: A' gathers from the long vector, A has that many rows) ----
STREAM_NAME = "csr_stream_kernel<EPI>"
EDGE_CASES = [
    # cols of A' = m, forcing, build, expected (A, A')
    # 2^22: 22 column bits, a unit of A' holds 1024 rows (local row 1023 fills the top 10 bits)
    pytest.param(1 << 22, "wave_p0", "dev", None, id="2^22-wave_p0-dev"),
    pytest.param(1 << 22, "ls_16_4", "host", None, id="2^22-ls_16_4-host"),
    # 2^22 + 1: 23 column bits, 512 rows per unit
    pytest.param((1 << 22) + 1, "wave_p0", "host", None, id="2^22+1-wave_p0-host"),
    pytest.param((1 << 22) + 1, "ls_16_1", "dev", None, id="2^22+1-ls_16_1-dev"),
    # 2^26: 26 column bits, 64 rows per unit -- the narrow layout's last size; A: 2^26 rows in 65536 units (16 lockstep rounds)
    pytest.param(1 << 26, "wave_p0", "dev", None, id="2^26-wave_p0-dev"),
    pytest.param(1 << 26, "ls_16_4", "host", None, id="2^26-ls_16_4-host"),
    pytest.param(1 << 26, "wide", "dev", None, id="2^26-wide-dev"),
    # 2^26 + 1: no room for the local row -- forcing the wave layout leaves A' on csr_stream; wr_wide gives the wide layout at its real width
    pytest.param((1 << 26) + 1, "wave_p0", "dev", ("csr_wave_kernel<EPI,0>", STREAM_NAME), id="2^26+1-waverows-dev"),
    pytest.param((1 << 26) + 1, "wide", "dev", None, id="2^26+1-wide-dev"),
]

_tall_cache = {}


def _tall(m, dtype, banded=False):
    """one integer problem per tall shape and precision (built once per module: the large ones take seconds)"""
    key = (m, dtype, banded)
    if key not in _tall_cache:
        _tall_cache.clear()  # one tall problem alive at a time (vectors of 2^26 entries)
        A_pat = sx.tall_pattern(m, seed=m & 0xFF, banded=banded)
        ops, x, y = sx.exact_problem(A_pat, sx.p_pattern("diag", A_pat.shape[1]), np.random.default_rng(m & 0xFFF), dtype)
        _tall_cache[key] = (ops, x, y, ops.exact(x, y))
    return _tall_cache[key]


@pytest.mark.parametrize("m,flavour,build,expect", EDGE_CASES)
def test_packing_edges_exact(monkeypatch, m, flavour, build, expect):
    L = _load("f64")
    env, name = FLAVOURS[flavour]
    _force(monkeypatch, env, build)
    ops, x, y, refs = _tall(m, np.float64)
    ws = Workspace(L, ops, np.float64)
    try:
        _expect(ws, *(expect or (name, name)))
        _exact_checks(ws, x, y, np.float64, refs)
    finally:
        ws.free()


# ---- lines_counted: the last gathered-vector length whose distinct lines are counted, and the first that is not ----
def _lines_cases():
    out = []
    for lib, rb in (("f64", 8), ("f32", 4)):
        last, first = sx.lines_counted_edge(rb)
        for cols in (last, first):
            for build in ("dev", "host"):
                out.append(pytest.param(lib, cols, build, id=f"{lib}-{cols}-{build}"))
    return out


def test_lines_counted_edges_are_where_the_header_puts_them():
    assert sx.lines_counted_edge(8) == ((1 << 23) + 127, (1 << 23) + 128)
    assert sx.lines_counted_edge(4) == ((1 << 24) + 255, (1 << 24) + 256)


@pytest.mark.parametrize("lib,cols,build", _lines_cases())
def test_lines_counted_edges(monkeypatch, lib, cols, build):
    """A' gathers in bands of 256 consecutive entries (0.07 distinct lines per entry when counted): where the lines are counted the
    planner picks the pipelined stream (csr_wave_kernel<EPI,1>, lines per entry < 0.8), where they are not it assumes one line per
    entry (csr_wave_kernel<EPI,0>) -- the kernel name shows which side of the edge both builders took"""
    L = _load(lib)
    dtype = LIBS[lib][1]
    counted = sx.lines_counted(cols, np.dtype(dtype).itemsize)
    assert counted == (cols == sx.lines_counted_edge(np.dtype(dtype).itemsize)[0])
    _force(monkeypatch, _P0, build)
    ops, x, y, refs = _tall(cols, dtype, banded=True)
    ws = Workspace(L, ops, dtype)
    try:
        assert ws.kernel(1) == ("csr_wave_kernel<EPI,1>" if counted else "csr_wave_kernel<EPI,0>")
        assert ws.kernel(0).startswith("csr_wave_kernel<EPI,")
        _exact_checks(ws, x, y, dtype, refs)
    finally:
        ws.free()


# ---- ACC and NEGDIV: the epilogues only scs_solve_lin_sys reaches ----
SOLVE_CASES = [pytest.param(f, s, id=f"{f}-{s}") for f in ("stream", "wave_p0", "ls_16_4", "wide") for s in ("empty", "dense", "random")]


@pytest.mark.parametrize("flavour,shape", SOLVE_CASES)
def test_solve_epilogues(monkeypatch, flavour, shape):
    """b_x += A' R_y^-1 b_y (EPI_ACC) before the CG loop and y = R_y^-1 (A x - b_y) (EPI_NEGDIV) after it: the returned y must be the
    long-double value of that formula at the returned x within bound (b), and the reduced residual the loop converged on, recomputed
    in long double, below the tolerance (plus the rounding of one application of the operator)"""
    L = _load("f64")
    env, name = FLAVOURS[flavour]
    _force(monkeypatch, env, "dev" if flavour in WAVE else "-")
    monkeypatch.setenv("SCS_AMD_FUSED", "0")  # the one-workgroup small-system path has epilogues of its own
    A_pat, P_pat = _pattern(shape)
    rng = np.random.default_rng(11)
    m, n = A_pat.shape
    A = A_pat.astype(np.float64).tocsc(copy=True)
    A.data = rng.uniform(-1, 1, A.nnz)
    P = None
    if P_pat is not None:
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
    # y = R_y^-1 (A x - b_y): k_A + 1 terms and a division
    y_ref = (sx.row_products(ia, ja, va, x, LD) - b[n:].astype(LD)) / ry.astype(LD)
    sx.check_bound(y, y_ref, sx.C_ROUND * u * (ops.ka + 2) * (absA(x) + np.abs(b[n:])) / ry, "y = R_y^-1 (A x - b_y)")
    # reduced system (R_x + P + A' R_y^-1 A) x = b_x + A' R_y^-1 b_y
    rhs = b[:n].astype(LD) + sx.row_products(it, jt, vt, b[n:].astype(LD) / ry.astype(LD), LD)
    gx = (diag_r[:n].astype(LD) * x.astype(LD) + sx.row_products(ip, jp, vp, x, LD)
          + sx.row_products(it, jt, vt, sx.row_products(ia, ja, va, x, LD) / ry.astype(LD), LD))
    res = np.abs(gx - rhs).max()
    scale = (np.abs(diag_r[:n] * x) + absP(x) + absAt(absA(x) / ry) + np.abs(b[:n]) + absAt(np.abs(b[n:]) / ry)).max()
    k = int(max(ops.kat.max(initial=0), ops.ka.max(initial=0), ops.kp.max(initial=0))) + 2
    assert res <= tol + sx.C_ROUND * k * u * scale, (float(res), tol)
