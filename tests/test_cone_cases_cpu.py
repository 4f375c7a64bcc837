"""The yardstick of tests/test_cones_degenerate_gpu.py, checked without a GPU: every closed-form `expected` of tests/cone_cases.py
against numpy (scs_amd.problems.proj_dual_cone_np; numpy's eigh of the Hermitian matrix for complex blocks) to 1e-13 of the case's
own scale -- max(1, t) for a box cone with finite bounds -- and, where oracle/_ref is built, against the live reference's
_scs_proj_dual_cone at the bounds the kernels are held to (1e-11 PSD, 1e-12 otherwise)."""
import ctypes as C

import numpy as np
import pytest

from scs_amd import capi, problems
from tests import cone_cases as cc


def _numpy_reference(case):
    cone = case.cone
    if cone.get("bsize") == 1:  # a box cone of t alone is the nonnegative half line
        cone = {"l": 1}
    real = {k: v for k, v in cone.items() if k != "cs"}
    n_real = capi.cone_rows(real)
    out = np.empty_like(case.x)
    out[:n_real] = problems.proj_dual_cone_np(case.x[:n_real], real)
    o = n_real
    for n in cone.get("cs", []):
        H = cc.unpack_herm(case.x[o:o + n * n], n)
        lam, V = np.linalg.eigh(H)
        out[o:o + n * n] = cc.pack_herm((V * np.maximum(lam, 0.0)) @ V.conj().T)
        o += n * n
    assert o == len(case.x)
    return out


def _ref():
    from oracle import pyoracle
    if not pyoracle.ref_available():
        return None
    ref = pyoracle.load_ref()
    ref._scs_proj_dual_cone.argtypes = [ref._scs_types.fp, C.c_void_p, C.c_void_p, ref._scs_types.fp]
    return ref


class _Scaling(C.Structure):  # include/scs_amd.h (reference include/scs_work.h)
    _fields_ = [("D", capi.T64.fp), ("E", capi.T64.fp), ("m", C.c_int), ("n", C.c_int), ("primal_scale", C.c_double),
                ("dual_scale", C.c_double)]


class _RefWork:
    """the live reference on one cone; it rescales box bounds in place, so it gets copies"""

    def __init__(self, ref, cone, D=None):
        self.ref, self.T = ref, ref._scs_types
        cone = {k: (np.array(v, dtype=np.float64) if k in ("bu", "bl") else v) for k, v in cone.items()}
        self.m = capi.cone_rows(cone)
        self.k = capi.make_cone(cone, self.T)
        self.w = ref._scs_init_cone(C.byref(self.k), self.m)
        assert self.w
        self.D = None if D is None else np.array(D, dtype=np.float64)
        self.scal = None if D is None else _Scaling(self.D.ctypes.data_as(self.T.fp), None, self.m, 0, 1.0, 1.0)

    def project(self, x, r=None):
        out = np.array(x, dtype=np.float64)
        rv = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
        rc = self.ref._scs_proj_dual_cone(out.ctypes.data_as(self.T.fp), self.w, C.byref(self.scal) if self.scal is not None else None,
                                          rv.ctypes.data_as(self.T.fp) if rv is not None else None)
        assert rc == 0
        return out

    def close(self):
        self.ref._scs_finish_cone(self.w)


def _check(case, tol_numpy, tol_ref, label, numpy_too=True):
    worst = 0.0
    if numpy_too:
        got = _numpy_reference(case)
        for p in case.parts:
            e = cc.rel_err(got, case, p.lo, p.hi)
            worst = max(worst, e)
            assert e <= tol_numpy, (label, p.label, "numpy", e)
    ref = _ref()
    if ref is not None:
        w = _RefWork(ref, case.cone, case.D)
        got = w.project(case.x)
        w.close()
        for p in case.parts:
            e = cc.rel_err(got, case, p.lo, p.hi)
            assert e <= tol_ref, (label, p.label, "live reference", e)
    print(f"{label}: worst distance from numpy {worst:.2e}")
    return worst


@pytest.mark.parametrize("cplx", [False, True])
def test_psd_families_have_the_projection_they_claim(cplx):
    for k, case in cc.psd_cases_by_order(cplx):
        _check(case, 1e-13, 1e-11, f"{'cs' if cplx else 's'} order {k}")


def test_psd_mixed_cone_and_dense_blocks():
    _check(cc.psd_mixed_case(), 1e-13, 1e-11, "mixed orders")
    _check(cc.psd_case([("dense", 7, 1.0, False), ("diagonal", 100, 2.0 ** 40, False), ("dense", 129, 2.0 ** -40, False)]), 1e-13, 1e-11, "dense")


def test_packing_round_trips():
    rng = np.random.default_rng(0)
    for k in (1, 2, 5):
        X = rng.standard_normal((k, k))
        X = X + X.T
        assert np.allclose(cc.unpack_psd(cc.pack_psd(X), k), X, rtol=0, atol=1e-15)
        assert abs(np.linalg.norm(cc.pack_psd(X)) - np.linalg.norm(X)) <= 1e-14 * np.linalg.norm(X)  # the packing is an isometry
        H = X + 1j * (rng.standard_normal((k, k)))
        H = H + H.conj().T
        assert np.allclose(cc.unpack_herm(cc.pack_herm(H), k), H, rtol=0, atol=1e-15)
        assert abs(np.linalg.norm(cc.pack_herm(H)) - np.linalg.norm(H)) <= 1e-14 * np.linalg.norm(H)


def test_second_order_families_have_the_projection_they_claim():
    case = cc.soc_all_sizes_case()
    assert sorted(set(case.cone["q"])) == list(cc.SOC_SIZES)
    _check(case, 1e-13, 1e-12, "soc, every size")
    for s in cc.SCALES:
        _check(cc.soc_all_sizes_one_scale(s), 1e-13, 1e-12, f"soc scale {s:g}")
    tiny = cc.soc_many_tiny_case()
    assert len(tiny.cone["q"]) == 40000 and len(tiny.x) == 120000
    _check(tiny, 1e-13, 1e-12, "soc 40000 x 3")
    # the cases that are equalities are equalities of the closed form too
    for c in (case, tiny):
        ex = c.exact
        assert np.all((c.expected[ex] == c.x[ex]) | (c.expected[ex] == 0))


def test_zero_and_nonnegative_rows():
    for z, l in cc.ZERO_NONNEG_SHAPES:
        case = cc.zero_nonneg_case(z, l)
        assert np.array_equal(_numpy_reference(case), case.expected)
        ref = _ref()
        if ref is not None:
            w = _RefWork(ref, case.cone)
            assert np.array_equal(w.project(case.x), case.expected)
            w.close()


@pytest.mark.parametrize("nb", (0, 1, 5) + cc.BOX_SIZES)
def test_box_root_is_the_minimiser(nb):
    """bsize = nb + 1.  Finite bounds: numpy's Newton iteration to 1e-13 of max(1, t).  Infinite bounds come into being only through a
    row scaling, which the numpy restatement does not take: those kinds are compared with the live reference alone."""
    for kind in cc.BOX_KINDS if nb else ("zero", "clamp", "inside"):
        case = cc.box_case(nb, kind)
        assert case.scale[0] >= 1.0
        worst = _check(case, 1e-13, 1e-12, f"box {kind} nb {nb}", numpy_too=case.D is None)
        assert worst <= 1e-13
    if nb:
        assert cc.box_case(nb, "clamp").expected[0] == cc.box_case(nb, "clamp").x[0]  # t = 0: y = x + 0
        assert np.array_equal(cc.box_case(nb, "zero").expected, np.zeros(nb + 1))


@pytest.mark.parametrize("nb", [5, 1025, 16385])
def test_box_sequence_against_numpy_and_the_live_reference(nb):
    cone, D, (ebl, ebu), xs = cc.box_sequence(nb)
    r = np.random.default_rng(nb).uniform(0.5, 3.0, nb + 1)
    ref = _ref()
    for use_r in (False, True):
        w = _RefWork(ref, cone, D) if ref is not None else None
        for i, x in enumerate(xs):
            y, t = cc.box_dual_expected(x, ebl, ebu, r if use_r else None)
            if not use_r and x[0] < 0:  # numpy with 1e100 for infinity; its Newton iteration starts at max(-x[0], 0), and at t = 0 the
                # two differ (0 * inf is NaN and compares false, 0 * 1e100 is 0)
                want = problems.proj_dual_cone_np(x, dict(bu=np.minimum(ebu, 1e100), bl=np.maximum(ebl, -1e100)))
                e = np.abs(y - want).max() / max(1.0, t)
                assert e <= 1e-13, (nb, i, "numpy", e)
            if w is not None:
                e = np.abs(w.project(x, r if use_r else None) - y).max() / max(1.0, t)
                assert e <= 1e-12, (nb, i, use_r, "live reference", e)
        if w is not None:
            w.close()
