"""Host equilibration (scs_amd/csrc/equilibrate.cpp, `where = 0` of scs_amd_equilibrate) against the reference's own
_scs_normalize_a_p on the edge shapes of tests/equilibrate_cases.py, in fp64 and in fp32, plus the properties of the result that
depend on neither implementation.  No GPU is needed; the comparison against the reference is skipped where oracle/_ref is not
built.  Measured differences and the reasoning behind every bar: profiles/equilibrate_edges.md."""
import ctypes as C

import numpy as np
import pytest

from scs_amd import capi
from tests import equilibrate_cases as ec
from tests.test_equilibrate import _equilibrate_raw, _raw_matrix

# fp64: both sides run the same passes in the same order and differ by a*b+c contraction and the order of the BLAS sums only
# (tests/test_equilibrate.py holds the random SOCP to the same number).  No case needs another bar.
RTOL_F64 = 1e-13
# fp32: four times the largest relative difference measured against the fp32 reference over all cases (3.524e-7, three units in
# the last place, on A.x of `empty/m257`; profiles/equilibrate_edges.md lists every case)
RTOL_F32 = 1.41e-6

FLAVOURS = {"f64": ("libscsamd.so", "libscsindir_ref.so", RTOL_F64), "f32": ("libscsamd_f32.so", "libscsindir_ref_f32.so", RTOL_F32)}


def _reference(ref, case):
    """_scs_init_cone + _scs_normalize_a_p (reference linsys/scs_matrix.c:433-496) on copies of the case's arrays"""
    T = ref._scs_types

    class ScsScaling(C.Structure):  # reference include/scs_work.h
        _fields_ = [("D", T.fp), ("E", T.fp), ("m", T.scs_int), ("n", T.scs_int), ("primal_scale", T.ftype),
                    ("dual_scale", T.ftype)]

    keep = []
    Am, Ax = _raw_matrix(T, case.m, case.n, case.Ap, case.Ai, case.Ax, keep)
    Pm, Px = None, None
    if case.P is not None:
        Pm, Px = _raw_matrix(T, case.n, case.n, *case.P, keep)
    k = capi.make_cone(case.cone, T)
    ref._scs_normalize_a_p.restype = C.POINTER(ScsScaling)
    ref._scs_normalize_a_p.argtypes = [C.POINTER(T.ScsMatrix), C.POINTER(T.ScsMatrix), C.c_void_p]
    work = ref._scs_init_cone(C.byref(k), case.m)
    assert work
    try:
        scal = ref._scs_normalize_a_p(C.byref(Pm) if Pm is not None else None, C.byref(Am), work)
        assert scal and scal.contents.m == case.m and scal.contents.n == case.n
        D = np.ctypeslib.as_array(scal.contents.D, shape=(case.m,)).copy()
        E = np.ctypeslib.as_array(scal.contents.E, shape=(case.n,)).copy()
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        for ptr in (scal.contents.D, scal.contents.E, scal):  # calloc'ed by the reference, released with free() in its scs_finish
            libc.free(C.cast(ptr, C.c_void_p))
    finally:
        ref._scs_finish_cone(work)
    del keep
    return Ax, Px, D, E


def rel_diff(got, want):
    """largest |got - want| / |want|; an entry the reference has at 0 must be 0 (atol = 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(want != 0, d / np.abs(want), np.where(d == 0, 0.0, np.inf))
    return float(e.max())


def _host(flavour, name):
    lib = capi.load(FLAVOURS[flavour][0])
    case = ec.build(name)
    return case, _equilibrate_raw(lib, case.m, case.n, (case.Ap, case.Ai, case.Ax), case.P, case.cone, 0)


@pytest.mark.parametrize("name", ec.NAMES)
@pytest.mark.parametrize("flavour", ["f64", "f32"])
def test_host_equilibration_matches_the_reference(flavour, name):
    from oracle import pyoracle
    _, ref_name, rtol = FLAVOURS[flavour]
    if not pyoracle.ref_available(ref_name):
        pytest.skip(f"oracle/_ref/{ref_name} not built")
    case, got = _host(flavour, name)
    want = _reference(pyoracle.load_ref(ref_name), case)
    worst = {}
    for g, w, what in zip(got, want, ("A.x", "P.x", "D", "E")):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape and g.dtype == w.dtype
        assert np.isfinite(w).all(), what
        worst[what] = rel_diff(g, w)
    print(f"equilibrate_edges {flavour} {name}: " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))
    for what, v in worst.items():
        assert v <= rtol, (flavour, name, what, v)


@pytest.mark.parametrize("name", ec.NAMES)
@pytest.mark.parametrize("flavour", ["f64", "f32"])
def test_host_equilibration_properties(flavour, name):
    """what holds whatever the implementation: finite positive scalings, one scale factor per cone after the first (row-wise)
    block, and returned values that are the inputs scaled entry by entry -- duplicates and explicit zeros included"""
    case, (Ax, Px, D, E) = _host(flavour, name)
    T = capi.load(FLAVOURS[flavour][0])._scs_types
    for v in (Ax, Px, D, E):
        assert v is None or np.isfinite(v).all()
    assert D.shape == (case.m,) and E.shape == (case.n,)
    assert (D > 0).all() and (E > 0).all()
    seg = ec.segments_of(case.cone)
    assert sum(seg) == case.m
    pos = seg[0]
    for ln in seg[1:]:
        assert (D[pos:pos + ln] == D[pos]).all(), (name, pos, ln)
        pos += ln
    # fp64: 1e-12, the bar of tests/test_equilibrate.py.  fp32: every entry is rescaled 26 times with two roundings each (the product
    # of the two factors, then the entry), D and E are products of 26 factors (25 roundings each): at most 102 roundings of 2^-24
    # between the two sides, 6.1e-6 (the same count in fp64 is 1.1e-14, inside the 1e-12)
    rtol = 1e-12 if flavour == "f64" else 102 * 2.0 ** -24
    A0 = np.array(case.Ax, dtype=T.np_float).astype(np.float64)
    cols = np.repeat(np.arange(case.n), np.diff(case.Ap))
    np.testing.assert_allclose(Ax, D.astype(np.float64)[case.Ai] * A0 * E.astype(np.float64)[cols], rtol=rtol, atol=0)
    if case.P is not None:
        Pp, Pi, P0 = case.P
        P0 = np.array(P0, dtype=T.np_float).astype(np.float64)
        pcols = np.repeat(np.arange(case.n), np.diff(Pp))
        Ed = E.astype(np.float64)
        np.testing.assert_allclose(Px, Ed[Pi] * P0 * Ed[pcols], rtol=rtol, atol=0)
    if case.Ap[-1] == 0 and case.P is None:
        assert (D == 1).all() and (E == 1).all()


def test_the_cases_hold_what_their_names_say():
    """the shapes the device thresholds turn on, checked on the arrays themselves"""
    rl, tl = ec.build("row_lengths"), ec.build("row_too_long")
    have = set(np.bincount(rl.Ai, minlength=rl.m).tolist())
    assert {0, 1, 2, ec.TR_SHORT, ec.TR_SHORT + 1, 64, 65, 1000, ec.TR_LONG_MAX} <= have and max(have) == ec.TR_LONG_MAX
    assert np.bincount(tl.Ai, minlength=tl.m).max() == ec.TR_LONG_MAX + 1
    du = ec.build("dups_unsorted")
    cols = np.repeat(np.arange(du.n), np.diff(du.Ap))
    pairs = du.Ai * du.n + cols
    assert 0.05 * len(pairs) <= len(pairs) - len(np.unique(pairs)) <= 0.2 * len(pairs)
    assert all((np.diff(du.Ai[du.Ap[j]:du.Ap[j + 1]]) <= 0).all() for j in range(0, du.n, 2))  # descending
    assert any((np.diff(du.Ai[du.Ap[j]:du.Ap[j + 1]]) > 0).any() for j in range(1, du.n, 2))   # shuffled
    sg = ec.build("segments")
    seg, pos = ec.segments_of(sg.cone), 0
    assert seg[0] == 0
    big = np.zeros(sg.m)
    np.maximum.at(big, sg.Ai, np.abs(sg.Ax))
    for ln in seg:
        if ln >= 2:
            assert np.argmax(big[pos:pos + ln]) == ln - 1 and big[pos + ln - 1] > 10 * big[pos:pos + ln - 1].max()
        pos += ln
    for name in ("clip/A", "clip/P"):
        cl = ec.build(name)
        rowmax, colmax = np.zeros(cl.m), np.zeros(cl.n)
        cols = np.repeat(np.arange(cl.n), np.diff(cl.Ap))
        np.maximum.at(rowmax, cl.Ai, np.abs(cl.Ax))
        np.maximum.at(colmax, cols, np.abs(cl.Ax))
        assert tuple(rowmax[:5]) == ec.CLIP_VALUES and tuple(colmax[:5]) == ec.CLIP_VALUES
        assert np.float32(rowmax[0]) == np.float32(1e-4)  # fp32 keeps the row exactly at the threshold as the library rounds it
    assert ec.build("empty/nnz0").Ap[-1] == 0
    for kind in ec.P_SHAPES:
        c = ec.build("p_shapes/" + kind)
        Pp, Pi, Px = c.P
        pcols = np.repeat(np.arange(c.n), np.diff(Pp))
        if kind == "diag":
            assert (Pi == pcols).all() and len(Pi) == c.n
        elif kind == "strict_upper":
            assert (Pi < pcols).all() and len(Pi) > 0
        elif kind == "empty_cols":
            assert (np.diff(Pp) == 0).sum() >= c.n // 3
        elif kind == "nnz0":
            assert len(Pi) == 0
        elif kind == "dense":
            assert len(Pi) == c.n * (c.n + 1) // 2
        elif kind == "zeros_dup":
            assert (Px == 0).sum() >= 2 and len(np.unique(Pi * c.n + pcols)) == len(Pi) - 1
