"""Blocks of vectors on one cone workspace (include/scs_amd.h, B1': scs_amd_cone_proj_dual_multi, scs_amd_cone_proj_dual_dev,
scs_amd_cone_proj_dual_multi_dev, scs_amd_cone_sync; kernels in scs_amd/csrc/cones_multi.h).

 1. goldens: every cone of tests/golden/cones_meta.json, both metrics, widths 2, 4, 8 and 16 -- column 0 against the reference's
    recorded output, every column against the single-vector entry on a fresh workspace and (where oracle/_ref is built) against
    the live reference's _scs_proj_dual_cone;
 2. shapes that exercise each kernel: second-order cones on both sides of the tiny / tiled switch and of a tile, a box cone on
    both sides of the one-workgroup / chip-wide switch, PSD orders on both sides of every switch of the LDS kernel and beyond it;
 3. a column's bits do not depend on its neighbours or its position; a repeat returns the same bits;
 4. the device entries: guard behind the block, all W columns written, bits of the host entry;
 5. - 7. the boundary of the interface: one column, seventeen columns, a leading dimension;
 8. - 9. carried state: accuracy over a drifting sequence, and isolation from the single-vector path's state;
10. the fp32 and the 64-bit-position builds;
11. - 12. bad arguments after good ones, memory;
13. the Python object scs_amd.cones.Cones.
Bounds (those of tests/test_cones_shim_gpu.py, error measured as there, max|got - want| / max(1, max|want|)): fp64 1e-12, or 1e-11
where a PSD block is present; fp32 2e-4 for PSD orders <= 92 and 5e-4 above.  The yardstick of every comparison is the
reference, numpy or the single-vector path, never the block path's own earlier output."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from scs_amd import capi, problems
from tests import test_spmv_exact_gpu as single_suite  # device buffers through the HIP runtime the library links

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = single_suite.GUARD
NRHS = (2, 3, 5, 8, 11, 16)


def _hip():
    single_suite._load("f64")
    return single_suite._hip


class Work:
    """one cone workspace of library L (fresh state: Newton start 1, no carried eigenbasis)"""

    def __init__(self, L, cone, D=None):
        self.L, self.T = L, L._scs_types
        self.cone, self.m = cone, capi.cone_rows(cone)
        self.k = capi.make_cone(cone, self.T)
        self.D = None if D is None else np.ascontiguousarray(D, dtype=self.T.np_float)
        self.w = L.scs_amd_cone_init(C.byref(self.k), self.m, self.D.ctypes.data_as(self.T.fp) if self.D is not None else None)
        assert self.w

    def _r(self, r):
        if r is None:
            return None, None
        r = np.ascontiguousarray(r, dtype=self.T.np_float)
        return r, r.ctypes.data_as(self.T.fp)

    def single(self, x, r=None):
        out = np.array(x, dtype=self.T.np_float, copy=True)
        assert out.shape == (self.m,)
        rv, rp = self._r(r)
        assert self.L.scs_amd_cone_proj_dual(self.w, out.ctypes.data_as(self.T.fp), rp) == 0
        return out

    def multi(self, X, r=None, expect=0):
        out = np.array(X, dtype=self.T.np_float, order="F", copy=True)
        assert out.ndim == 2 and out.shape[0] == self.m
        rv, rp = self._r(r)
        assert self.L.scs_amd_cone_proj_dual_multi(self.w, out.shape[1], out.ctypes.data_as(self.T.fp), self.m, rp) == expect
        return out

    def close(self):
        if self.w:
            self.L.scs_amd_cone_finish(self.w)
            self.w = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _err(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if len(want) else 0.0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _single_fresh(L, cone, x, r=None, D=None):
    with Work(L, cone, D) as w:
        return w.single(x, r)


def _ref():
    from oracle import pyoracle
    if not pyoracle.ref_available():
        return None
    ref = pyoracle.load_ref()
    ref._scs_proj_dual_cone.argtypes = [ref._scs_types.fp, C.c_void_p, C.c_void_p, ref._scs_types.fp]
    return ref


def _ref_columns(ref, cone, X, r):
    Tr = ref._scs_types
    kr = capi.make_cone(cone, Tr)
    wr = ref._scs_init_cone(C.byref(kr), X.shape[0])
    assert wr
    out = np.array(X, dtype=np.float64, order="F", copy=True)
    rv = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    for k in range(out.shape[1]):
        col = np.ascontiguousarray(out[:, k])
        assert ref._scs_proj_dual_cone(col.ctypes.data_as(Tr.fp), wr, None, rv.ctypes.data_as(Tr.fp) if rv is not None else None) == 0
        out[:, k] = col
    ref._scs_finish_cone(wr)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------------------------------------------------------------
_META = json.load(open(os.path.join(G, "cones_meta.json")))


@pytest.mark.parametrize("name", sorted(_META))
def test_goldens_every_width(name):
    L = capi.load("libscsamd.so")
    g = np.load(os.path.join(G, "cones.npz"))
    cone = _META[name]
    m = capi.cone_rows(cone)
    tol = 1e-11 if ("psd" in name or name in ("mixed", "all", "all_c")) else 1e-12  # the rule of tests/test_cones_shim_gpu.py
    ref = _ref()
    for variant in ("ry", "eucl"):
        x0 = np.array(g[f"{name}_{variant}_x"])
        want0 = np.array(g[f"{name}_{variant}_y"])
        r = np.array(g[f"{name}_{variant}_r"]) if variant == "ry" else None
        rng = np.random.default_rng(len(name) + (variant == "ry"))
        X = np.empty((m, 16), order="F")
        X[:, 0] = x0
        for k in range(1, 16):  # scaled and perturbed copies
            X[:, k] = x0 * (1.0 + 0.25 * k) * (-1.0 if k % 5 == 4 else 1.0) + (0.05 * k) * rng.standard_normal(m)
        singles = np.stack([_single_fresh(L, cone, X[:, k], r) for k in range(16)], axis=1)
        refs = _ref_columns(ref, cone, X, r) if ref is not None else None
        assert _err(singles[:, 0], want0) <= tol  # the yardstick itself
        for nrhs in NRHS:
            with Work(L, cone) as w:
                got = w.multi(X[:, :nrhs], r)
            e0 = _err(got[:, 0], want0)
            print(f"{name} {variant} nrhs {nrhs}: column 0 against the golden output {e0:.3e}")
            assert e0 <= tol, (name, variant, nrhs, e0)
            for k in range(nrhs):
                e = _err(got[:, k], singles[:, k])
                assert e <= tol, (name, variant, nrhs, k, "single-vector path", e)
                if refs is not None:
                    e = _err(got[:, k], refs[:, k])
                    assert e <= tol, (name, variant, nrhs, k, "live reference", e)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. shapes that exercise each kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_block(L, cone, X, r, tol, D=None, numpy_too=True, label=""):
    """a block on a fresh workspace: every column against the single-vector path on a fresh workspace, and against numpy where
    numpy's projection applies (Euclidean metric, bounds as given)"""
    with Work(L, cone, D) as w:
        got = w.multi(X, r)
    for k in range(X.shape[1]):
        one = _single_fresh(L, cone, X[:, k], r, D)
        e = _err(got[:, k], one)
        print(f"{label} column {k}: against the single-vector path {e:.3e}")
        assert e <= tol, (label, k, "single-vector path", e)
        if numpy_too and r is None and D is None:
            e = _err(got[:, k], problems.proj_dual_cone_np(X[:, k], cone))
            print(f"{label} column {k}: against numpy {e:.3e}")
            assert e <= tol, (label, k, "numpy", e)
    return got


def _soc_block(cone, K, seed):
    """columns that put the cones in all three cases of proj_soc (inside, polar, neither)"""
    rng = np.random.default_rng(seed)
    m = capi.cone_rows(cone)
    X = rng.standard_normal((m, K))
    off = cone.get("z", 0) + cone.get("l", 0)
    for j, q in enumerate(cone["q"]):
        for k in range(K):
            nrm = np.linalg.norm(X[off + 1:off + q, k])
            X[off, k] = (2.0 * nrm + 1.0, -2.0 * nrm - 1.0, 0.3 * nrm, -0.4 * nrm)[(j + k) % 4]
        off += q
    return np.asfortranarray(X)


@pytest.mark.parametrize("nrhs", [2, 3, 8, 16])
def test_second_order_cones_tiny_tiled_and_tile_edges(nrhs):
    L = capi.load("libscsamd.so")
    cone = dict(z=3, l=4, q=[1, 2, 16, 17, 2047, 2048, 2049, 6000, 5])
    X = _soc_block(cone, nrhs, 3 + nrhs)
    _check_block(L, cone, X, None, 1e-12, label=f"soc nrhs {nrhs}")
    r = np.random.default_rng(9).uniform(0.5, 3.0, X.shape[0])
    _check_block(L, cone, X, r, 1e-12, label=f"soc r_y nrhs {nrhs}")


@pytest.mark.parametrize("nb", [3000, 20000])  # the one-workgroup kernel / the chip-wide Newton steps (BOX_MULTI_MIN = 16384 rows)
def test_box_cone_both_sides_of_the_switch(nb):
    L = capi.load("libscsamd.so")
    rng = np.random.default_rng(nb)
    bu, bl = rng.uniform(0.1, 2.0, nb), -rng.uniform(0.1, 2.0, nb)
    cone = dict(l=2, bu=bu, bl=bl)
    m = nb + 3
    X = np.asfortranarray(rng.standard_normal((m, 3)) * 2.0)
    X[2, :] = (0.3, -1.0, 4.0)  # t: the clamp at zero included
    _check_block(L, cone, X, None, 1e-12, label=f"box {nb}")
    # the r_y metric and infinite bounds (|bound| >= 1e15 with a scaling D: src/cones.c:1161-1177)
    bu2, bl2 = bu.copy(), bl.copy()
    bu2[::7] = 1e20
    bl2[::11] = -1e20
    cone2 = dict(l=2, bu=bu2, bl=bl2)
    D = rng.uniform(0.5, 2.0, m)
    r = rng.uniform(0.5, 3.0, m)
    got = _check_block(L, cone2, X, r, 1e-12, D=D, label=f"box {nb} r_y inf")
    assert np.abs(got - X).max() > 1e-3
    ref = _ref()
    if ref is not None:  # the live reference with the same bounds (no scaling: 1e20 stays a finite bound there, as in this library)
        got = _check_block(L, cone2, X, r, 1e-12, numpy_too=False, label=f"box {nb} r_y")
        want = _ref_columns(ref, dict(l=2, bu=bu2.copy(), bl=bl2.copy()), X, r)
        for k in range(3):
            e = _err(got[:, k], want[:, k])
            assert e <= 1e-12, (nb, k, "live reference", e)


@pytest.mark.parametrize("nrhs", [2, 5])
def test_psd_orders_around_every_switch(nrhs):
    L = capi.load("libscsamd.so")
    cone = dict(l=1, s=[1, 50, 51, 72, 73, 92, 100])
    m = capi.cone_rows(cone)
    X = np.asfortranarray(np.random.default_rng(17 + nrhs).standard_normal((m, nrhs)))
    _check_block(L, cone, X, None, 1e-11, label=f"psd nrhs {nrhs}")


def test_psd_lds_orders_only_and_pipelined_orders_only():
    L = capi.load("libscsamd.so")
    for cone in (dict(s=[80, 92, 7]), dict(s=[50, 24, 2], cs=[5])):
        m = capi.cone_rows(cone)
        X = np.asfortranarray(np.random.default_rng(m).standard_normal((m, 4)))
        _check_block(L, cone, X, None, 1e-11, numpy_too=not cone.get("cs"), label=str(cone))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. neighbours and position
# ---------------------------------------------------------------------------------------------------------------------------------
_EVERY = dict(z=2, l=3, bu=[1.0, 2.0, 0.5, 3.0, 1.5], bl=[-1.0, -0.5, -2.0, 0.0, -1.5], q=[3, 17, 3000, 1], s=[6, 51, 95], cs=[4], ep=2, ed=2,
              p=[0.3, -0.6])


@pytest.mark.parametrize("nrhs,pos_a,pos_b", [(4, 0, 2), (5, 4, 1), (16, 15, 0), (2, 1, 0)])
def test_a_column_does_not_depend_on_its_neighbours_or_its_position(nrhs, pos_a, pos_b):
    L = capi.load("libscsamd.so")
    cone = _EVERY
    m = capi.cone_rows(cone)
    rng = np.random.default_rng(41 + nrhs)
    a = rng.standard_normal(m)
    r = rng.uniform(0.5, 2.0, m)
    A = np.asfortranarray(rng.standard_normal((m, nrhs)))
    A[:, (pos_a + 1) % nrhs] = 0.0
    if nrhs > 2:
        A[:, (pos_a + 2) % nrhs] *= 1e8
    A[:, pos_a] = a
    B = np.asfortranarray(rng.standard_normal((m, nrhs)) * 3.0)  # every other column holds different data
    if nrhs > 2:
        B[:, (pos_b + 1) % nrhs] = 0.0
        B[:, (pos_b + 2) % nrhs] *= 1e8
    B[:, pos_b] = a

    def run(X):
        with Work(L, cone) as w:
            out = np.array(X, order="F", copy=True)
            rc = L.scs_amd_cone_proj_dual_multi(w.w, nrhs, out.ctypes.data_as(w.T.fp), m, r.ctypes.data_as(w.T.fp))
            assert rc in (0, 1)  # 1: a PSD block of the 1e8 column at the sweep cap -- reported, not fatal
            return out

    ga, gb, ga2 = run(A), run(B), run(A)
    assert np.array_equal(_bits(ga[:, pos_a]), _bits(gb[:, pos_b])), "a column's bits depend on its neighbours or its position"
    assert np.array_equal(_bits(ga), _bits(ga2)), "a repeat on a fresh workspace gave different bits"
    zero = (pos_a + 1) % nrhs
    assert np.array_equal(ga[:, zero], np.zeros(m)), "the projection of 0 is 0"
    e = _err(ga[:, pos_a], _single_fresh(L, cone, a, r))
    assert e <= 1e-11, e


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. device entries
# ---------------------------------------------------------------------------------------------------------------------------------
def _device_block(L, w, cols, r, calls=1):
    """scs_amd_cone_proj_dual_multi_dev on the block whose columns are `cols`: NaN in the padding columns and in a guard behind the
    block.  Returns the (m, W) result of the last call."""
    hip = _hip()
    dt = w.T.np_float
    m, nrhs = w.m, len(cols)
    W = L.scs_amd_cone_multi_width(nrhs)
    assert W >= nrhs and W in (1, 2, 4, 8, 16)
    X = np.full((m, W), np.nan, dt)
    for k, c in enumerate(cols):
        X[:, k] = c
    buf = np.concatenate([X.ravel(), np.full(GUARD, np.nan, dt)])
    dx = hip.malloc(buf.nbytes)
    dr = None
    try:
        if r is not None:
            rv = np.concatenate([np.asarray(r, dt), np.full(GUARD, np.nan, dt)])
            dr = hip.malloc(rv.nbytes)
            hip.put(dr, rv)
        got = np.empty_like(buf)
        for _ in range(calls):
            hip.put(dx, buf)
            hip.sync()  # the entries run on the workspace's own stream: the caller's writes must be complete
            assert L.scs_amd_cone_proj_dual_multi_dev(w.w, nrhs, dx, dr) == 0
            assert L.scs_amd_cone_sync(w.w) == 0
            hip.get(got, dx)
    finally:
        hip.free(dx)
        if dr is not None:
            hip.free(dr)
    assert np.array_equal(_bits(got[m * W:]), _bits(buf[m * W:])), "the guard behind the block was written"
    Y = got[:m * W].reshape(m, W)
    assert np.isfinite(Y).all(), "a column of the block was not written"
    assert np.array_equal(Y[:, nrhs:], np.zeros((m, W - nrhs))), "padding columns come back zero"
    return Y


@pytest.mark.parametrize("lib", ["libscsamd.so", "libscsamd_f32.so"])
@pytest.mark.parametrize("nrhs", [2, 3, 8, 11])
def test_device_entry_has_the_bits_of_the_host_entry(lib, nrhs):
    L = capi.load(lib)
    cone = dict(z=2, l=5, bu=[1.0, 2.0, 0.5], bl=[-1.0, -0.5, -2.0], q=[3, 17, 2049, 5000], s=[6, 51], ep=3, ed=2, p=[0.3, -0.6])
    m = capi.cone_rows(cone)
    dt = L._scs_types.np_float
    rng = np.random.default_rng(nrhs)
    X = np.asfortranarray(rng.standard_normal((m, nrhs)).astype(dt))
    for r in (None, rng.uniform(0.5, 2.0, m).astype(dt)):
        with Work(L, cone) as w:
            host = w.multi(X, r)
        with Work(L, cone) as w:
            dev = _device_block(L, w, [X[:, k] for k in range(nrhs)], r)
        assert np.array_equal(_bits(dev[:, :nrhs]), _bits(host))


@pytest.mark.parametrize("lib", ["libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so"])
def test_single_vector_device_entry_is_the_host_entry_bit_for_bit(lib):
    L = capi.load(lib)
    hip = _hip()
    cone = dict(z=2, l=5, bu=[1.0, 2.0, 0.5], bl=[-1.0, -0.5, -2.0], q=[3, 17, 2049, 5000], s=[6, 51, 95], ep=3, ed=2, p=[0.3, -0.6])
    m = capi.cone_rows(cone)
    dt = L._scs_types.np_float
    rng = np.random.default_rng(5)
    seq = [rng.standard_normal(m).astype(dt) for _ in range(3)]
    r = rng.uniform(0.5, 2.0, m).astype(dt)
    with Work(L, cone) as w:
        want = [w.single(x, r) for x in seq]
    with Work(L, cone) as w:
        rv = np.concatenate([r, np.full(GUARD, np.nan, dt)])
        dx, dr = hip.malloc((m + GUARD) * rv.itemsize), hip.malloc(rv.nbytes)
        try:
            hip.put(dr, rv)
            for i, x in enumerate(seq):  # the carried state moves as it does through the host entry
                buf = np.concatenate([x, np.full(GUARD, np.nan, dt)])
                hip.put(dx, buf)
                hip.sync()
                fn = (lambda: L.scs_amd_cone_proj_dual_dev(w.w, dx, dr)) if i != 1 else (lambda: L.scs_amd_cone_proj_dual_multi_dev(w.w, 1, dx, dr))
                assert fn() == 0
                assert L.scs_amd_cone_sync(w.w) == 0
                got = np.empty_like(buf)
                hip.get(got, dx)
                assert np.array_equal(_bits(got[m:]), _bits(buf[m:])), "the guard behind the vector was written"
                assert np.array_equal(_bits(got[:m]), _bits(want[i])), i
        finally:
            hip.free(dx)
            hip.free(dr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. - 7. one column, seventeen columns, leading dimension
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_column_is_the_single_vector_path_bit_for_bit():
    L = capi.load("libscsamd.so")
    cone = _EVERY
    m = capi.cone_rows(cone)
    rng = np.random.default_rng(2)
    r = rng.uniform(0.5, 2.0, m)
    seq = [rng.standard_normal(m) for _ in range(3)]
    with Work(L, cone) as w:
        want = [w.single(x, r) for x in seq]
    with Work(L, cone) as w:
        for x, wv in zip(seq, want):
            got = w.multi(x.reshape(m, 1), r)
            assert np.array_equal(_bits(got[:, 0]), _bits(wv))


def test_seventeen_columns_in_two_chunks():
    L = capi.load("libscsamd.so")
    cone = dict(l=4, bu=[1.0, 2.0], bl=[-1.0, -0.5], q=[3, 40, 2500], s=[10, 3])
    m = capi.cone_rows(cone)
    X = np.asfortranarray(np.random.default_rng(17).standard_normal((m, 17)))
    got = _check_block(L, cone, X, None, 1e-11, label="17 columns")
    assert np.abs(got - X).max() > 1e-3


def test_leading_dimension_leaves_the_gap_untouched():
    L = capi.load("libscsamd.so")
    cone = dict(l=4, q=[3, 40, 2500], s=[10, 3])
    m = capi.cone_rows(cone)
    K, ld = 5, m + 7
    rng = np.random.default_rng(3)
    X = np.asfortranarray(rng.standard_normal((m, K)))
    buf = np.full((ld, K), -777.25, order="F")
    buf[:m, :] = X
    with Work(L, cone) as w:
        want = w.multi(X)
    with Work(L, cone) as w:
        assert L.scs_amd_cone_proj_dual_multi(w.w, K, buf.ctypes.data_as(w.T.fp), ld, None) == 0
    assert np.array_equal(buf[m:, :], np.full((7, K), -777.25))
    assert np.array_equal(_bits(buf[:m, :]), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. - 9. carried state
# ---------------------------------------------------------------------------------------------------------------------------------
def test_carried_state_stays_accurate_over_a_drifting_sequence():
    """The box cone's Newton start and every PSD block's eigenbasis are carried per column position.  One sequence of 71 block
    calls on one workspace: a slow drift, an unrelated input at call 40 (a useless basis must not be a harmful one), and the cold
    restart of call 64 (PSD_WARM_RESET) crossed on the way.  Every column of every call must match numpy at 1e-11."""
    L = capi.load("libscsamd.so")
    rng = np.random.default_rng(8)
    bu, bl = rng.uniform(0.5, 2.0, 30), -rng.uniform(0.5, 2.0, 30)
    cone = dict(l=2, bu=bu, bl=bl, s=[50, 24, 100])
    m = capi.cone_rows(cone)
    K = 4
    base, vel = rng.standard_normal((m, K)), rng.standard_normal((m, K))
    worst = 0.0
    with Work(L, cone) as w:
        for it in range(71):
            X = base + 0.01 * it * vel + 1e-3 * rng.standard_normal((m, K))
            if it == 40:
                X = rng.standard_normal((m, K)) * 5
            got = w.multi(X)
            for k in range(K):
                e = _err(got[:, k], problems.proj_dual_cone_np(X[:, k], cone))
                worst = max(worst, e)
                assert e <= 1e-11, (it, k, e)
    print(f"carried state: worst error over 71 block calls {worst:.3e}")


@pytest.mark.parametrize("nb", [30, 20000])  # the one-workgroup box kernel / the chip-wide Newton steps, whose control record and partials both paths use
def test_block_calls_leave_the_single_vector_state_alone(nb):
    L = capi.load("libscsamd.so")
    rng = np.random.default_rng(12)
    bu, bl = rng.uniform(0.5, 2.0, nb), -rng.uniform(0.5, 2.0, nb)
    cone = dict(l=2, bu=bu, bl=bl, q=[5, 3000], s=[50, 80, 100], ep=2, p=[0.4])
    m = capi.cone_rows(cone)
    base, vel = rng.standard_normal(m), rng.standard_normal(m)
    seq = [base + 0.01 * it * vel + 1e-3 * rng.standard_normal(m) for it in range(20)]
    r = rng.uniform(0.5, 2.0, m)
    with Work(L, cone) as a:
        want = [a.single(x, r) for x in seq]
    with Work(L, cone) as b:
        for it, x in enumerate(seq):
            if it % 2 == 0:
                b.multi(rng.standard_normal((m, 3 if it % 4 else 5)) * 2.0, r if it % 3 else None)  # widths 4 and 8 alternate
            got = b.single(x, r)
            assert np.array_equal(_bits(got), _bits(want[it])), it
            b.multi(rng.standard_normal((m, 17 if it == 7 else 2)), r)  # 17: a last chunk of one column is a block too


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. fp32 and the 64-bit-position build
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cone,tol", [(dict(z=1, l=3, bu=[1.0, 2.0], bl=[-1.0, -0.5], q=[5, 17, 3000], s=[20, 64, 51, 80]), 2e-4),
                                      (dict(l=2, s=[100, 30]), 5e-4)])
def test_fp32_build(cone, tol):
    L = capi.load("libscsamd_f32.so")
    m = capi.cone_rows(cone)
    rng = np.random.default_rng(23)
    v = rng.standard_normal((m, 5))
    with Work(L, cone) as w:
        for rep in range(4):  # cold, then warm started
            v = v + (0.3 if rep < 2 else 1e-3) * rng.standard_normal((m, 5))
            X = np.asfortranarray(v.astype(np.float32))
            got = w.multi(X)
            for k in range(5):
                e = _err(got[:, k].astype(np.float64), problems.proj_dual_cone_np(X[:, k].astype(np.float64), cone))
                print(f"fp32 rep {rep} column {k}: {e:.3e}")
                assert e <= tol, (rep, k, e)
            assert np.abs(got - X).max() > 1e-2


def test_dlong_build_matches_its_single_vector_path():
    L = capi.load("libscsamd_dlong.so")
    cone = _EVERY
    m = capi.cone_rows(cone)
    rng = np.random.default_rng(29)
    X = np.asfortranarray(rng.standard_normal((m, 6)))
    r = rng.uniform(0.5, 2.0, m)
    _check_block(L, cone, X, r, 1e-11, label="dlong")
    small = dict(l=3, q=[4, 2500], s=[9])
    _check_block(L, small, np.asfortranarray(rng.standard_normal((capi.cone_rows(small), 3))), None, 1e-11, label="dlong numpy")


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. - 12. bad arguments, memory
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_workspace_stays_usable():
    L = capi.load("libscsamd.so")
    cone = dict(l=4, bu=[1.0, 2.0], bl=[-1.0, -0.5], q=[3, 40], s=[10, 3])
    m = capi.cone_rows(cone)
    rng = np.random.default_rng(31)
    X = np.asfortranarray(rng.standard_normal((m, 3)))
    with Work(L, cone) as w:
        fp = w.T.fp
        first = w.multi(X)
        keep = X.copy(order="F")
        for nrhs, ptr, ld in ((0, X.ctypes.data_as(fp), m), (-2, X.ctypes.data_as(fp), m), (3, X.ctypes.data_as(fp), m - 1), (3, None, m)):
            assert L.scs_amd_cone_proj_dual_multi(w.w, nrhs, ptr, ld, None) == -1
            assert np.array_equal(_bits(X), _bits(keep))
        for nrhs in (0, 17, -1):
            assert L.scs_amd_cone_proj_dual_multi_dev(w.w, nrhs, C.c_void_p(X.ctypes.data), None) == -1  # refused before the pointer is used
        assert L.scs_amd_cone_proj_dual_multi_dev(w.w, 2, None, None) == -1
        assert L.scs_amd_cone_proj_dual_dev(w.w, None, None) == -1
        again = w.multi(X)
    for k in range(3):
        want = problems.proj_dual_cone_np(X[:, k], cone)
        assert _err(first[:, k], want) <= 1e-11
        assert _err(again[:, k], want) <= 1e-11


def test_hip_failure_inside_a_block_projection():
    """scs_amd_test_fail_at reports a successful runtime call as failed (it faults nothing): the call returns -1 and the same
    workspace projects correctly afterwards"""
    L = capi.load("libscsamd.so")
    cone = dict(l=4, bu=[1.0, 2.0], bl=[-1.0, -0.5], q=[3, 40, 2500], s=[10, 3])
    m = capi.cone_rows(cone)
    X = np.asfortranarray(np.random.default_rng(37).standard_normal((m, 5)))
    with Work(L, cone) as w:
        w.multi(X)  # allocates the block state
        big = 10 ** 12
        L.scs_amd_test_fail_at(big)
        w.multi(X)
        total = big - L.scs_amd_test_fail_at(0)  # checked runtime calls of one block projection
        assert total >= 3
        for k in sorted({1, 2, total}):
            L.scs_amd_test_fail_at(k)
            w.multi(X, expect=-1)
            assert L.scs_amd_test_fail_at(0) == 0, k  # consumed inside the call
        got = w.multi(X)
    for k in range(5):
        assert _err(got[:, k], problems.proj_dual_cone_np(X[:, k], cone)) <= 1e-11


def test_block_state_is_freed_with_the_workspace():
    """the "nothing leaked" check of tests/test_linsys_multi_gpu.py (same allowance for the runtime's own caches); the block state of
    this cone at width 16 holds three m x 16 buffers, about 115 MB"""
    L = capi.load("libscsamd.so")
    cone = dict(l=200000, q=[100000], s=[20])
    m = capi.cone_rows(cone)
    X = np.asfortranarray(np.random.default_rng(1).standard_normal((m, 16)))

    def free_bytes():
        v = L.scs_amd_device_free_bytes()
        assert v >= 0
        return v

    with Work(L, cone) as w:  # warm: context, streams, code objects
        w.multi(X[:, :2])
    base = free_bytes()
    w = Work(L, cone)
    w.multi(X[:, :3])  # width 4 first, then width 16
    w.multi(X)
    held = base - free_bytes()
    assert held > 3 * m * 16 * 8 * 0.9
    w.close()
    assert abs(free_bytes() - base) <= 8 << 20


# ---------------------------------------------------------------------------------------------------------------------------------
# 13. the Python object
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_python_cones_object(dtype):
    from scs_amd.cones import Cones
    cone = dict(z=1, l=3, bu=[1.0, 2.0], bl=[-1.0, -0.5], q=[5, 17, 3000], s=[20, 51])
    m = capi.cone_rows(cone)
    rng = np.random.default_rng(43)
    X = rng.standard_normal((m, 6))  # C order
    r = rng.uniform(0.5, 2.0, m)
    Xk, rk = X.copy(), r.copy()
    tol = 1e-11 if dtype == "f64" else 2e-4
    with Cones(cone, dtype=dtype) as c:
        got = c.project_many(X, r)
        gotf = c.project_many(np.asfortranarray(X), r)
    assert got.shape == (m, 6) and np.array_equal(X, Xk) and np.array_equal(r, rk)
    with Cones(cone, dtype=dtype) as c:
        for k in range(6):
            one = c.project(X[:, k], r)
            assert _err(got[:, k].astype(np.float64), one.astype(np.float64)) <= tol, k
            assert _err(gotf[:, k].astype(np.float64), one.astype(np.float64)) <= tol, k
        with pytest.raises(ValueError):
            c.project_many(X[:-1], r)
        with pytest.raises(ValueError):
            c.project(X[:, 0], r[:-1])
    with pytest.raises(RuntimeError):
        c.project(X[:, 0])  # closed
    with Cones(dict(l=3), dtype=dtype) as c:
        assert np.array_equal(c.project_many(np.array([[1.0, -2.0], [-1.0, 3.0], [0.5, 0.0]])), np.array([[1.0, 0.0], [0.0, 3.0], [0.5, 0.0]]))
