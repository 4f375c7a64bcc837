"""The cone projection on degenerate inputs whose answers are known in closed form (tests/cone_cases.py; the yardstick itself is
checked on the CPU by tests/test_cone_cases_cpu.py): scs_amd_cone_proj_dual and scs_amd_cone_proj_dual_multi of libscsamd.so and
libscsamd_f32.so.

Gaussian vectors never reach the zero block, the block that is diagonal on entry, the steps of a sweep with nothing to rotate, the
pair with a_pp == a_qq, the large block that is finished before the first sweep, the second-order cone on its boundary or the box
cone's size switches; and an error divided by max(1, |want|.max()) of the whole vector cannot see a block of norm 2^-40.  Here

 1. every case runs on a fresh workspace and is held to 1e-11 (PSD) / 1e-12 (everything else) of its OWN scale -- the block's
    Frobenius norm, the second-order cone's infinity norm, max(1, t) for the box cone (the reference's stopping rule is absolute
    below t = 1) -- and to equality where the answer is x or 0 by a branch that computes nothing;
 2. PSD blocks of order <= 72 run under the three forms of the step (psd_pipe 1, 0, 2), box cones under both paths (box_multi);
 3. one workspace is carried through dense -> zero -> dense -> rank one -> Householder (three times) -> diagonal -> dense;
 4. blocks of 2, 5 and 16 columns hold different families side by side;
 5. the fp32 build at scale 1, at 2e-4 (LDS path, second-order cones) and 5e-4 (blocked path) of the case's scale.
Every check prints its worst error as a line `DEGEN | kind | path | precision | error` (profiles/cones_degenerate.md)."""
import ctypes as C

import numpy as np
import pytest

from scs_amd import capi
from tests import cone_cases as cc

pytestmark = pytest.mark.gpu

TOL_PSD, TOL = 1e-11, 1e-12
LDS_KMAX = 92  # blocks above this order run the chip-wide iteration


class Work:
    """one cone workspace of library L, fresh: Newton start 1, no carried eigenbasis"""

    def __init__(self, L, cone, D=None):
        self.L, self.T = L, L._scs_types
        self.m = capi.cone_rows(cone)
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

    def multi(self, X, r=None):
        out = np.array(X, dtype=self.T.np_float, order="F", copy=True)
        assert out.ndim == 2 and out.shape[0] == self.m
        rv, rp = self._r(r)
        assert self.L.scs_amd_cone_proj_dual_multi(self.w, out.shape[1], out.ctypes.data_as(self.T.fp), self.m, rp) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.w:
            self.L.scs_amd_cone_finish(self.w)
            self.w = None


class option:
    """scs_amd_set_option for the workspaces created inside the block; back to the default afterwards"""

    def __init__(self, L, key, value):
        self.L, self.key, self.value = L, key.encode(), value

    def __enter__(self):
        if self.value is not None:
            assert self.L.scs_amd_set_option(self.key, str(self.value).encode()) == 0

    def __exit__(self, *exc):
        self.L.scs_amd_set_option(self.key, None)


def _part_errors(got, case):
    """worst |got - expected| / scale of every part; a row of scale 0 counts 0 when equal and inf when not"""
    d = np.abs(np.asarray(got, dtype=np.float64) - case.expected)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(case.scale > 0, d / case.scale, np.where(d == 0, 0.0, np.inf))
    lows = np.array([p.lo for p in case.parts])
    assert lows[0] == 0 and case.parts[-1].hi == len(case.x) and all(a.hi == b.lo for a, b in zip(case.parts, case.parts[1:]))
    return np.maximum.reduceat(e, lows)


def _is_psd(label):
    return label.startswith(("s ", "cs "))


def _kind(label):
    """the part's label without its scale: family and order"""
    return label.split(" scale ")[0]


def _check(got, case, path, prec="fp64", exact=True, tol=None):
    """every part of `got` against the case's known answer at its own scale; the equalities too"""
    errs = _part_errors(got, case)
    worst = {}
    for p, e in zip(case.parts, errs):
        worst[_kind(p.label)] = max(worst.get(_kind(p.label), 0.0), float(e))
    for kind, e in worst.items():
        print(f"DEGEN | {kind} | {path} | {prec} | {e:.3e}")
    for p, e in zip(case.parts, errs):
        t = tol(p.label) if tol else (TOL_PSD if _is_psd(p.label) else TOL)
        assert e <= t, (p.label, path, prec, float(e))
    if exact:
        rows = cc.exact_rows(case)
        bad = np.flatnonzero(rows & (np.asarray(got, dtype=np.float64) != case.expected))
        assert len(bad) == 0, (path, "rows that must be equal differ", bad[:8], [p.label for p in case.parts if p.lo <= bad[0] < p.hi])


def _agree(a, b, case, tol, what):
    """two results for the same case, each part at its own scale"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(case.scale > 0, d / case.scale, np.where(d == 0, 0.0, np.inf))
    i = int(np.argmax(e))
    assert e[i] <= tol, (what, float(e[i]), [p.label for p in case.parts if p.lo <= i < p.hi])
    return float(e[i])


def _metric_per_part(case, seed):
    """an r_y that is constant over each cone / block: the projection stays the Euclidean one"""
    rng = np.random.default_rng(seed)
    r = np.empty(len(case.x))
    for p in case.parts:
        r[p.lo:p.hi] = rng.uniform(0.5, 3.0)
    return r


def _lib():
    return capi.load("libscsamd.so")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. + 2. known answers on a fresh workspace, every form of the step
# ---------------------------------------------------------------------------------------------------------------------------------
def _psd_known(case, order, label):
    L = _lib()
    pipes = (1, 0, 2) if order <= 72 else (None,)
    got = {}
    for pipe in pipes:
        with option(L, "psd_pipe", pipe):
            with Work(L, case.cone) as w:
                got[pipe] = w.single(case.x)
            _check(got[pipe], case, f"{label} psd_pipe {pipe if pipe is not None else 'default'}")
            with Work(L, case.cone) as w:
                ry = w.single(case.x, _metric_per_part(case, order))
            e = _agree(ry, got[pipe], case, 1e-13, "r_y constant over each block")
            print(f"DEGEN | {label} r_y against NULL | psd_pipe {pipe} | fp64 | {e:.3e}")
    if len(pipes) == 3:
        _agree(got[1], got[0], case, 2e-12, "psd_pipe 1 against 0")
        _agree(got[2], got[0], case, 1e-13, "psd_pipe 2 against 0")


@pytest.mark.parametrize("k", cc.PSD_ORDERS)
def test_real_psd_families_every_order_and_scale(k):
    case = cc.psd_order_case(k)
    _psd_known(case, k, f"s order {k}")


@pytest.mark.parametrize("n", cc.CS_ORDERS)
def test_hermitian_psd_families_every_order_and_scale(n):
    case = cc.psd_order_case(n, cplx=True)
    _psd_known(case, 2 * n, f"cs order {n}")


def test_psd_blocks_of_every_order_and_scale_in_one_cone():
    case = cc.psd_mixed_case()
    L = _lib()
    with Work(L, case.cone) as w:
        got = w.single(case.x)
    _check(got, case, "mixed cone")
    with Work(L, case.cone) as w:
        ry = w.single(case.x, _metric_per_part(case, 3))
    _agree(ry, got, case, 1e-13, "r_y constant over each block")


@pytest.mark.parametrize("blocks", [
    [("diagonal", 100), ("dense", 129), ("zero", 93), ("diagonal", 128), ("dense", 7)],        # finished at sweep 0 next to blocks that are not
    [("diagonal", 93), ("zero", 128), ("diagonal", 129), ("plus_identity", 100)],              # every large block finished at once
    [("zero", 129), ("zero", 93)],
    [("householder", 51), ("diagonal", 129), ("two_householder", 100), ("zero", 72)]], ids=["next_to_dense", "all_finished", "all_zero", "mixed_paths"])
def test_large_blocks_finished_before_the_first_sweep(blocks):
    case = cc.psd_case([(f, k, cc.SCALES[i % 3], False) for i, (f, k) in enumerate(blocks)])
    L = _lib()
    with Work(L, case.cone) as w:
        first = w.single(case.x)
        again = w.single(case.x)  # warm started from the carried basis
    _check(first, case, "large blocks, cold")
    _check(again, case, "large blocks, warm")


def _soc_known(case, label):
    L = _lib()
    with Work(L, case.cone) as w:
        got = w.single(case.x)
    _check(got, case, label)
    with Work(L, case.cone) as w:
        ry = w.single(case.x, _metric_per_part(case, 5))
    e = _agree(ry, got, case, 1e-13, "r_y constant over each cone")
    print(f"DEGEN | {label} r_y against NULL | single | fp64 | {e:.3e}")


def test_second_order_cones_every_family_size_and_scale():
    _soc_known(cc.soc_all_sizes_case(), "soc scales mixed")
    for s in cc.SCALES:
        _soc_known(cc.soc_all_sizes_one_scale(s), f"soc scale {s:g}")


def test_forty_thousand_second_order_cones_of_size_three():
    _soc_known(cc.soc_many_tiny_case(), "soc 40000 x 3")


def test_zero_and_nonnegative_rows_are_exact():
    L = _lib()
    for z, l in cc.ZERO_NONNEG_SHAPES:
        case = cc.zero_nonneg_case(z, l)
        with Work(L, case.cone) as w:
            got = w.single(case.x)
            blk = w.multi(np.stack([case.x, -case.x, case.x], axis=1))
        assert np.array_equal(got, case.expected), (z, l)
        assert np.array_equal(blk[:, 0], case.expected) and np.array_equal(blk[:, 2], case.expected), (z, l)
        print(f"DEGEN | z {z} l {l} | single + block | fp64 | 0 (equal)")


_EVERY = dict(z=3, l=5, bu=[1.0, 2.0, 0.5, 1e20, 0.0, 3.0, 1.5], bl=[-1.0, -0.5, -2.0, 0.0, 0.0, -1e20, -1.5], q=[1, 2, 3, 17, 2049],
              s=[2, 51, 80, 100], cs=[3, 40, 50])


@pytest.mark.parametrize("lib", ["libscsamd.so", "libscsamd_f32.so"])
def test_zero_input_to_every_cone_gives_zero(lib):
    L = capi.load(lib)
    m = capi.cone_rows(_EVERY)
    D = np.random.default_rng(1).uniform(0.5, 2.0, m)
    for d in (None, D):
        with Work(L, _EVERY, d) as w:
            for rep in range(2):  # the second call is warm started from whatever the first one left
                assert np.array_equal(w.single(np.zeros(m)), np.zeros(m)), (lib, d is not None, rep)
            assert np.array_equal(w.multi(np.zeros((m, 5))), np.zeros((m, 5))), (lib, d is not None)
            assert np.array_equal(w.single(np.zeros(m), np.full(m, 2.0)), np.zeros(m))
    print(f"DEGEN | zero input, every cone | single + block | {lib} | 0 (equal)")


def _box_known(nb, kinds):
    L = _lib()
    for kind in kinds:
        case = cc.box_case(nb, kind)
        got = {}
        for multi in (0, 1):
            with option(L, "box_multi", multi):
                with Work(L, case.cone, case.D) as w:
                    got[multi] = w.single(case.x)
            _check(got[multi], case, f"box_multi {multi}")
        _agree(got[0], got[1], case, 1e-11, f"box {kind} nb {nb}: one workgroup against chip wide")
        with Work(L, case.cone, case.D) as w:  # the path the size selects
            _check(w.single(case.x), case, "box_multi default")


@pytest.mark.parametrize("nb", (1, 5) + cc.BOX_SIZES)
def test_box_cone_known_answers_both_paths(nb):
    """nb bounded rows, bsize = nb + 1: bsize 2, five rows (on the chip-wide path most workgroups then own none), and both sides of
    the block size, of the switch between the paths and of the chip-wide kernel's 256 x 256 lane stride"""
    _box_known(nb, cc.BOX_KINDS)


def test_box_cone_of_t_alone():
    L = _lib()
    for t0 in (-2.0, 0.0, 3.0):
        for multi in (None, 0, 1):
            with option(L, "box_multi", multi):
                with Work(L, dict(bsize=1, l=2)) as w:
                    x = np.array([1.0, -1.0, -t0])
                    assert np.array_equal(w.single(x), np.array([1.0, 0.0, -t0 + max(t0, 0.0)])), (t0, multi)
                    assert np.array_equal(w.multi(np.stack([x, x], axis=1))[:, 1], np.array([1.0, 0.0, -t0 + max(t0, 0.0)]))


@pytest.mark.parametrize("nb", [5, 1025, 16385])
def test_box_sequence_on_one_workspace_from_far_warm_starts(nb):
    """t0 = 1e3, 1e-3, -5, 1e3, 0, 2, 1e-9, 50 with row scales 1, 1, 1, 100, 1e-6, 0, 1e3, 1e3 on ONE workspace, so every Newton
    iteration starts from the previous call's t; with and without r_y; both paths.  The expected t is the exact root."""
    L = _lib()
    cone, D, (ebl, ebu), xs = cc.box_sequence(nb)
    r = np.random.default_rng(nb).uniform(0.5, 3.0, nb + 1)
    out = {}
    for multi in (0, 1):
        for use_r in (False, True):
            with option(L, "box_multi", multi):
                w = Work(L, cone, D)
            with w:
                for i, x in enumerate(xs):
                    got = w.single(x, r if use_r else None)
                    want, t = cc.box_dual_expected(x, ebl, ebu, r if use_r else None)
                    e = float(np.abs(got - want).max() / max(1.0, t))
                    print(f"DEGEN | box sequence nb {nb} step {i} t {t:.3e} r_y {use_r} | box_multi {multi} | fp64 | {e:.3e}")
                    assert e <= TOL, (nb, multi, use_r, i, t, e)
                    out[(multi, use_r, i)] = (got, t)
    for use_r in (False, True):
        for i in range(len(xs)):
            (a, t), (b, _) = out[(0, use_r, i)], out[(1, use_r, i)]
            assert np.abs(a - b).max() <= 1e-11 * max(1.0, t), (nb, use_r, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. carried state
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_workspace_through_dense_zero_rank_one_householder_diagonal():
    orders = (7, 51, 80, 100)
    seq = [("dense", 0), ("zero", 0), ("dense", 0), ("rank_one", 0), ("householder", 0), ("householder", 0), ("householder", 0),
           ("diagonal", 0), ("dense", 40)]
    cases = [cc.psd_case([(f, k, cc.SCALES[j % 3] if f != "dense" else 1.0, False) for j, k in enumerate(orders)], seed=seed)
             for i, (f, seed) in enumerate(seq)]
    assert np.array_equal(cases[0].x, cases[2].x) and np.array_equal(cases[4].x, cases[6].x) and not np.array_equal(cases[0].x, cases[8].x)
    L = _lib()
    got = []
    with Work(L, cases[0].cone) as w:
        for i, case in enumerate(cases):
            got.append(w.single(case.x))
            _check(got[-1], case, f"carried, call {i} ({seq[i][0]})")
    for first, again in ((0, 2), (4, 5), (4, 6)):  # warm started: nothing is left to rotate
        e = _agree(got[again], got[first], cases[first], 1e-13, f"call {again} repeats call {first}")
        print(f"DEGEN | carried, call {again} against call {first} | single | fp64 | {e:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. block form
# ---------------------------------------------------------------------------------------------------------------------------------
_BLOCK_PSD = ("zero", "dense", "diagonal", "rank_one", "householder", "positive_definite")
_BLOCK_SOC = ("inside", "polar", "boundary", "generic")
_SOC_OF_ONE = dict(inside="head_pos", polar="head_neg", boundary="zero", generic="head_pos")


def _check_block(L, cases, D=None, label=""):
    """columns that share a cone: each against its known answer, and against the single-vector path on a fresh workspace"""
    cone = cases[0].cone
    assert all(str(c.cone) == str(cone) for c in cases)
    with Work(L, cone, D) as w:
        got = w.multi(np.stack([c.x for c in cases], axis=1))
    for k, case in enumerate(cases):
        _check(got[:, k], case, f"{label} width {len(cases)} column {k}")
        with Work(L, cone, D) as w:
            one = w.single(case.x)
        for p, e in zip(case.parts, _part_errors(one, case._replace(expected=got[:, k]))):
            assert e <= (TOL_PSD if _is_psd(p.label) else TOL), (label, k, p.label, "single-vector path", float(e))


@pytest.mark.parametrize("width", [2, 5, 16])
def test_block_of_psd_families_side_by_side(width):
    orders = ((7, False), (51, False), (80, False), (100, False), (129, False), (5, True), (40, True))
    cases = []
    for c in range(width):
        blocks = []
        for i, (k, cplx) in enumerate(orders):
            f = _BLOCK_PSD[(i + c) % len(_BLOCK_PSD)]
            if f == "dense" and cplx:
                f = "two_householder"
            blocks.append((f, k, 1.0 if f == "dense" else cc.SCALES[(i + 2 * c) % 3], cplx))
        cases.append(cc.psd_case(blocks, seed=10 * c))
    _check_block(_lib(), cases, label="psd")


@pytest.mark.parametrize("width", [2, 5, 16])
def test_block_whose_large_psd_blocks_are_all_diagonal(width):
    """every large block of every column is finished at sweep 0: the host's next batch is sized from zero remaining sweeps"""
    orders = (93, 128, 129, 100)
    cases = [cc.psd_case([("diagonal" if (i + c) % 4 else "zero", k, cc.SCALES[(i + c) % 3], False) for i, k in enumerate(orders)], seed=7 * c)
             for c in range(width)]
    _check_block(_lib(), cases, label="psd large diagonal")


@pytest.mark.parametrize("width", [2, 5, 16])
def test_block_of_second_order_families_side_by_side(width):
    sizes = (1, 2, 3, 16, 17, 2048, 2049, 4097, 3)
    cases = []
    for c in range(width):
        fam = [_BLOCK_SOC[(i + c) % 4] for i in range(len(sizes))]
        cases.append(cc.soc_case([(_SOC_OF_ONE[f] if q == 1 else f, q, cc.SCALES[(i + c) % 3]) for i, (f, q) in enumerate(zip(fam, sizes))], seed=c))
    _check_block(_lib(), cases, label="soc")


@pytest.mark.parametrize("nb", [1025, 16385])
@pytest.mark.parametrize("width", [2, 5, 16])
def test_block_of_box_columns_with_t0_negative_zero_and_large(width, nb):
    cases = [cc.box_case(nb, "mixed", t0=(-3.0, 0.0, 50.0)[c % 3], xseed=c) for c in range(width)]
    _check_block(_lib(), cases, D=cases[0].D, label=f"box nb {nb}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the fp32 build
# ---------------------------------------------------------------------------------------------------------------------------------
def _tol32(label):
    if not _is_psd(label):
        return 2e-4
    order = int(label.split(" order ")[1].split()[0]) * (2 if label.startswith("cs ") else 1)
    return 2e-4 if order <= LDS_KMAX else 5e-4


def _check32(case, label):
    L = capi.load("libscsamd_f32.so")
    x32 = case.x.astype(np.float32)
    with Work(L, case.cone) as w:
        got = w.single(x32)
        blk = w.multi(np.stack([x32, x32], axis=1))
    _check(got.astype(np.float64), case, label, prec="fp32", exact=False, tol=_tol32)
    _check(blk[:, 1].astype(np.float64), case, label + " block", prec="fp32", exact=False, tol=_tol32)


@pytest.mark.parametrize("cplx", [False, True], ids=["s", "cs"])
def test_fp32_psd_families_at_scale_one(cplx):
    for k in (cc.CS_ORDERS if cplx else cc.PSD_ORDERS):
        _check32(cc.psd_case([(f, k, 1.0, cplx) for f in cc.PSD_FAMILIES]), f"{'cs' if cplx else 's'} order {k}")


def test_fp32_second_order_families_at_scale_one():
    _check32(cc.soc_all_sizes_one_scale(1.0), "soc")
