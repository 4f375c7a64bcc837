"""A block of Anderson accelerations in lock step (scs_amd/csrc/aa_multi.h, scs_amd_aa_multi_*) against the reference's
src/aa.c (oracle/_ref) and against the project's single-vector device path, column by column, on fixed-point iterations whose
columns desynchronise: safeguard rejections, resets and skipped calls put them in different phases of the same call.

The block form reorders the O(dim) sums, so agreement with either side is to rounding amplified by the (regularised)
least-squares solve: 1e-6 relative on the iterates (the bar of tests/test_aa_dev_gpu.py), identical safeguard decisions, equal
signs of aa_norm.  Within the block form itself results are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from scs_amd import capi
from tests import test_aa_dev_gpu as dev  # the rejected-solve cases and their reference side
from tests import test_spmv_exact_gpu as single_suite  # device buffers through the HIP runtime the library links

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

K16 = [0.03] * 5 + [-1.5, -1.5, -0.8, 0.03, 0.03, -1.5, 0.03, 0.03, -1.2, 0.03, 0.03]
ITERS = 50
RESET_AT, SKIP_AT = 17, (9, 10, 23)
MARK = -12345.678
# (type1, regularization, relaxation, lookback, dim)
CONFIG = {
    1: (1, 1e-8, 1.0, 10, 5003),     # the defaults; 21 panel columns = 2 batches
    2: (0, 1e-12, 1.0, 5, 5003),     # type II
    3: (1, 1e-8, 1.3, 6, 4099),      # relaxation: x_work per column
    4: (1, -1e-6, 1.0, 4, 300),      # pinned regularisation; one workgroup; dim below one transposition tile times W
    5: (0, 1e-10, 1.0, 20, 1031),    # more pivot candidates than one batch of 16
    6: (1, 1e-8, 1.0, 10, 140009),   # beyond 512 x 256 rows: every kernel grid-strides; odd dim
}


def _p(a):
    return a.ctypes.data_as(dp)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _map(dim, seed, kink):
    """tests/test_aa_dev_gpu.py::_map with its constant 0.03 as a parameter"""
    rng = np.random.default_rng(seed)
    d0 = rng.uniform(0.3, 0.95, dim)
    d1 = rng.uniform(-0.02, 0.02, dim)
    c = rng.standard_normal(dim)
    return lambda v: d0 * v + d1 * np.roll(v, 1) + c + kink * np.maximum(v, 0)


def _spec(K):
    """column k: (seed, kink, event class); class 1 is reset before iteration 17, class 2 skipped at iterations 9, 10, 23"""
    return [(100 + k, K16[k], k % 4) for k in range(K)]


# columns 0, 5, 6, 13 of the list with the four event classes: a block of four in which a rejected column is also reset and
# another one also skipped (the list's first four columns all carry the mild kink)
MIXED = [(100, K16[0], 0), (105, K16[5], 1), (106, K16[6], 2), (113, K16[13], 3)]


def _skipped(ev, i):
    return ev == 2 and i in SKIP_AT


# ---- the three sides ----------------------------------------------------------------------------------------------------------
def _amd(name="libscsamd.so"):
    L = capi.load(name)
    T = L._scs_types
    L.scs_amd_aa_dev_init.restype = C.c_void_p
    L.scs_amd_aa_dev_init.argtypes = [T.scs_int] * 4 + [T.ftype] * 4 + [T.scs_int]
    L.scs_amd_aa_dev_apply.restype = T.ftype
    L.scs_amd_aa_dev_apply.argtypes = [T.fp, T.fp, C.c_void_p]
    L.scs_amd_aa_dev_safeguard.restype = T.scs_int
    L.scs_amd_aa_dev_safeguard.argtypes = [T.fp, T.fp, C.c_void_p]
    L.scs_amd_aa_dev_finish.argtypes = [C.c_void_p]
    L.scs_amd_aa_dev_reset.argtypes = [C.c_void_p]
    return L


def _ref():
    ref = pyoracle.load_ref()
    ref.aa_init.restype = C.c_void_p
    ref.aa_init.argtypes = [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int, C.c_int]
    ref.aa_apply.restype = C.c_double
    ref.aa_apply.argtypes = [dp, dp, C.c_void_p]
    ref.aa_safeguard.restype = C.c_int
    ref.aa_safeguard.argtypes = [dp, dp, C.c_void_p]
    ref.aa_reset.restype = None
    ref.aa_reset.argtypes = [C.c_void_p]
    ref.aa_finish.argtypes = [C.c_void_p]
    return ref


def _run_single(init, apply, safeguard, reset, finish, extra, cfg, spec, dt=np.float64):
    """One column at a time through a single-vector implementation, `_run` of tests/test_aa_dev_gpu.py with the events.
    Returns (norms [ITERS-1][K], rejected [ITERS][K], iterates [ITERS][dim, K])."""
    type1, reg, relax, mem, dim = cfg
    K = len(spec)
    norms, rejs, traj = np.zeros((ITERS - 1, K)), np.zeros((ITERS, K), int), np.zeros((ITERS, dim, K), dt)
    fp = C.POINTER(C.c_double if dt == np.float64 else C.c_float)
    for k, (seed, kink, ev) in enumerate(spec):
        F = _map(dim, seed, kink)
        a = init(dim, mem, mem, type1, reg, relax, 1.0, 1e10, 5, *extra)
        assert a
        x = np.zeros(dim, dt)
        x_prev = x.copy()
        for i in range(ITERS):
            if ev == 1 and i == RESET_AT:
                reset(a)
            if i > 0 and not _skipped(ev, i):
                norms[i - 1, k] = apply(x.ctypes.data_as(fp), x_prev.ctypes.data_as(fp), a)
            x_prev = x.copy()
            x = F(x).astype(dt)
            if not _skipped(ev, i):
                rejs[i, k] = safeguard(x.ctypes.data_as(fp), x_prev.ctypes.data_as(fp), a)
            traj[i, :, k] = x
        finish(a)
    return norms, rejs, traj


class Block:
    """scs_amd_aa_multi_* on host arrays"""

    def __init__(self, L, cfg, K, max_weight=1e10):
        type1, reg, relax, mem, dim = cfg
        self.L, self.T, self.K, self.dim, self.mem = L, L._scs_types, K, dim, mem
        self.a = L.scs_amd_aa_multi_init(dim, K, mem, mem, type1, reg, relax, 1.0, max_weight, 5)
        assert self.a

    def _skip(self, skip):
        return np.ascontiguousarray(skip, dtype=self.T.np_int)

    def apply(self, F, X, skip, expect=0):
        T = self.T
        nrm = np.full(self.K, 99.0, T.np_float)
        sk = self._skip(skip)
        rc = self.L.scs_amd_aa_multi_apply(self.a, F.ctypes.data_as(T.fp), self.dim, X.ctypes.data_as(T.fp), self.dim,
                                           sk.ctypes.data_as(T.ip), nrm.ctypes.data_as(T.fp))
        assert rc == expect
        return nrm

    def safeguard(self, F, X, skip):
        T = self.T
        rej = np.full(self.K, 99, T.np_int)
        sk = self._skip(skip)
        assert self.L.scs_amd_aa_multi_safeguard(self.a, F.ctypes.data_as(T.fp), self.dim, X.ctypes.data_as(T.fp), self.dim,
                                                 sk.ctypes.data_as(T.ip), rej.ctypes.data_as(T.ip)) == 0
        return rej

    def reset(self, col):
        self.L.scs_amd_aa_multi_reset(self.a, col)

    def stats(self, k):
        st = self.T.AaStats()
        self.L.scs_amd_aa_multi_get_stats(self.a, k, C.byref(st))
        return st

    def iters(self):
        return [self.stats(k).iter for k in range(self.K)]

    def counters(self):
        out = (C.c_longlong * 4)()
        self.L.scs_amd_aa_multi_get_counters(self.a, C.byref(out))
        return list(out)

    def close(self):
        if self.a:
            self.L.scs_amd_aa_multi_finish(self.a)
            self.a = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _run_block(b, spec):
    """The same loop on the block object `b` (anything with apply / safeguard / reset / iters).  A skipped column goes in filled
    with a marker and has to come back bit for bit with its iteration count where it was.  Returns norms, rejected, iterates and
    lens [ITERS-1][K] (the memory length every column had when its apply was called)."""
    K, dim, mem = b.K, b.dim, b.mem
    dt = b.T.np_float
    maps = [_map(dim, seed, kink) for seed, kink, _ in spec]
    norms, rejs, traj = np.zeros((ITERS - 1, K)), np.zeros((ITERS, K), int), np.zeros((ITERS, dim, K), dt)
    lens = np.zeros((ITERS - 1, K), int)
    X = np.zeros((dim, K), dt, order="F")
    Xp = X.copy(order="F")
    for i in range(ITERS):
        skip = np.array([_skipped(ev, i) for _, _, ev in spec])
        if i == RESET_AT:
            for k, (_, _, ev) in enumerate(spec):
                if ev == 1:
                    b.reset(k)
        if i > 0:
            before = b.iters()
            lens[i - 1] = np.minimum(before, mem)
            Fc, Xc = X.copy(order="F"), Xp.copy(order="F")
            Fc[:, skip] = MARK
            Xc[:, skip] = MARK
            norms[i - 1] = b.apply(Fc, Xc, skip)
            after = b.iters()
            for k in range(K):
                if skip[k]:
                    assert np.array_equal(_bits(Fc[:, k]), _bits(np.full(dim, MARK, dt))) and after[k] == before[k] and norms[i - 1, k] == 0
                else:
                    X[:, k] = Fc[:, k]
        Xp = X.copy(order="F")
        for k in range(K):
            X[:, k] = maps[k](X[:, k]).astype(dt)
        Fc, Xc = X.copy(order="F"), Xp.copy(order="F")
        Fc[:, skip] = MARK
        Xc[:, skip] = MARK
        before = b.iters()
        rejs[i] = b.safeguard(Fc, Xc, skip)
        after = b.iters()
        for k in range(K):
            if skip[k]:
                assert np.array_equal(_bits(Fc[:, k]), _bits(np.full(dim, MARK, dt))) and rejs[i, k] == 0 and after[k] == before[k]
                assert np.array_equal(_bits(Xc[:, k]), _bits(np.full(dim, MARK, dt)))
            else:
                X[:, k], Xp[:, k] = Fc[:, k], Xc[:, k]
        traj[i] = X
    return norms, rejs, traj, lens


def _compare(got, want, label, rejects):
    nb, rb, tb, lens = got
    ns, rs, ts = want
    assert np.array_equal(rb, rs), f"{label}: safeguard decisions differ"
    assert np.array_equal(np.sign(nb), np.sign(ns)), f"{label}: accept / reject decisions differ"
    worst = 0.0
    for i in range(ITERS):
        for k in range(tb.shape[2]):
            e = np.abs(tb[i, :, k] - ts[i, :, k]).max() / max(1.0, np.abs(ts[i, :, k]).max())
            worst = max(worst, e)
    print(f"{label}: worst relative difference of an iterate {worst:.3e}, rejections per column {(-rb).sum(axis=0).tolist()}")
    assert worst <= 1e-6, (label, worst)
    if rejects:
        assert (rb == -1).any(), f"{label}: no column was safeguard-rejected"
    assert any(len(set(row.tolist())) > 1 for row in lens), f"{label}: the columns never had different memory lengths in one call"
    assert (nb > 0).any()


# ---- 1. against the reference ----------------------------------------------------------------------------------------------------
# (configuration, K, rejects): the first K columns of the list; K = "mixed": the block MIXED.  `rejects`: whether the safeguard
# rejects a column of the case at all -- what src/aa.c alone does on these inputs on the CPU (the columns with a kink of -1.2 or
# below are rejected under type I, never under configuration 2; the mild columns only under configurations 4 and 5).  Where it
# does, the case has to show it, so that it cannot pass on columns that stay synchronised.
@pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("cfg_no,K,rejects", [(1, 16, True), (2, 5, False), (3, 3, False), (6, 3, False), (2, "mixed", False),
                                              (3, "mixed", True)])
def test_block_matches_reference_column_by_column(cfg_no, K, rejects):
    ref = _ref()
    spec = MIXED if K == "mixed" else _spec(K)
    with Block(_amd(), CONFIG[cfg_no], len(spec)) as b:
        got = _run_block(b, spec)
    want = _run_single(ref.aa_init, ref.aa_apply, ref.aa_safeguard, ref.aa_reset, ref.aa_finish, (0,), CONFIG[cfg_no], spec)
    _compare(got, want, f"config {cfg_no} K={K} vs reference", rejects)


# ---- 2. against the single-vector device path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_no,K,rejects", [(4, 4, True), (5, 4, True), (1, 2, False), (4, "mixed", True), (5, "mixed", True),
                                              (1, "pair", True)])
def test_block_matches_single_vector_device_path(cfg_no, K, rejects):
    L = _amd()
    spec = MIXED if K == "mixed" else (MIXED[1:3] if K == "pair" else _spec(K))
    with Block(L, CONFIG[cfg_no], len(spec)) as b:
        got = _run_block(b, spec)
    want = _run_single(L.scs_amd_aa_dev_init, L.scs_amd_aa_dev_apply, L.scs_amd_aa_dev_safeguard, L.scs_amd_aa_dev_reset,
                       L.scs_amd_aa_dev_finish, (), CONFIG[cfg_no], spec)
    _compare(got, want, f"config {cfg_no} K={K} vs aa_dev", rejects)


# ---- 2a. rejected and degenerate solves ------------------------------------------------------------------------------------------
@pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("setting", list(dev.REJ_SETTINGS))
def test_a_block_of_rejected_and_degenerate_solves_matches_reference(setting):
    """The three maps of tests/test_aa_dev_gpu.py (REJ_MAPS) as columns 0, 1, 2 of one block (W = 4): every call holds a
    weight-capped column beside a rank-0 (setting A) or zero-gamma (setting B) column.  Per column: counters equal to the
    reference's, equal signs of aa_norm, equal safeguard decisions, iterates bit-equal to x <- F(x)."""
    type1, reg, mem = dev.REJ_SETTINGS[setting]
    names = list(dev.REJ_MAPS)
    K, dim = len(names), dev.REJ_DIM
    maps = [dev.rej_map(n) for n in names]
    none = np.zeros(K, bool)
    with Block(_amd(), (type1, reg, 1.0, mem, dim), K, max_weight=dev.REJ_CAP) as b:
        assert b.L.scs_amd_aa_multi_width(K) == 4
        X = np.asfortranarray(np.stack([dev.rej_start(n) for n in names], axis=1))
        Xp = X.copy(order="F")
        norms, rejs, traj = [], [], []
        for i in range(dev.REJ_ITERS):  # the loop of tests/test_aa_dev_gpu.py::_run
            if i > 0:
                norms.append(b.apply(X, Xp, none))
            Xp = X.copy(order="F")
            for k in range(K):
                X[:, k] = maps[k](X[:, k])
            rejs.append(b.safeguard(X, Xp, none))
            traj.append(X.copy(order="F"))
        stats = [dev.counters(b.stats(k)) for k in range(K)]
    for k, name in enumerate(names):
        dev.rej_check((np.sign([n[k] for n in norms]), [int(r[k]) for r in rejs], [np.ascontiguousarray(t[:, k]) for t in traj],
                       stats[k]), setting, name)


# ---- 3. independence and determinism ---------------------------------------------------------------------------------------------
def test_a_column_depends_neither_on_its_neighbours_nor_on_its_position():
    L = _amd()
    K = 8
    base = _spec(K)
    others = [(200 + k, [-1.5, 0.03, -0.8, 0.0, 0.03, -1.2, 0.5, 0.03][k], (k + 1) % 4) for k in range(K)]
    others[3] = base[3]
    moved = list(others)
    moved[3], moved[6] = others[6], base[3]  # column 3's map and events at position 6
    runs = []
    for spec in (base, others, moved, base):
        with Block(L, CONFIG[1], K) as b:
            runs.append(_run_block(b, spec))
    a, o, mv, again = runs
    assert (a[1][:, 3] == -1).sum() + (a[0][:, 3] > 0).sum() > 5  # column 3 does solve
    for other, pos, what in ((o, 3, "its neighbours"), (mv, 6, "its position")):
        assert np.array_equal(_bits(a[2][:, :, 3]), _bits(other[2][:, :, pos])), f"column 3's iterates depend on {what}"
        assert np.array_equal(_bits(a[0][:, 3]), _bits(other[0][:, pos])), f"column 3's aa_norm depends on {what}"
        assert np.array_equal(a[1][:, 3], other[1][:, pos])
    for x, y in zip(a[:3], again[:3]):
        assert np.array_equal(_bits(x), _bits(y)), "a second run gave different bits"
    # the skipped columns (class 2: k = 2, 6) came back bit for bit with their counters in place: asserted inside _run_block
    assert any(ev == 2 for _, _, ev in base)


# ---- 4. one column ---------------------------------------------------------------------------------------------------------------
def test_one_column_is_the_single_vector_path_bit_for_bit():
    L = _amd()
    assert [L.scs_amd_aa_multi_width(k) for k in (1, 2, 3, 4, 5, 16, 0, 17)] == [1, 2, 4, 4, 8, 16, 0, 0]
    spec = [(105, K16[5], 1)]
    with Block(L, CONFIG[1], 1) as b:
        nb, rb, tb, _ = _run_block(b, spec)
    ns, rs, ts = _run_single(L.scs_amd_aa_dev_init, L.scs_amd_aa_dev_apply, L.scs_amd_aa_dev_safeguard, L.scs_amd_aa_dev_reset,
                             L.scs_amd_aa_dev_finish, (), CONFIG[1], spec)
    assert (rb == -1).any() and (nb > 0).any()
    assert np.array_equal(rb, rs) and np.array_equal(_bits(nb), _bits(ns)) and np.array_equal(_bits(tb), _bits(ts))


# ---- 5. device entries -----------------------------------------------------------------------------------------------------------
class DevBlock(Block):
    """the _dev entries on device buffers in the block layout; the padding columns hold a marker"""

    def __init__(self, L, cfg, K):
        super().__init__(L, cfg, K)
        single_suite._load("f64")
        self.hip = single_suite._hip
        self.W = L.scs_amd_aa_multi_width(K)
        self.dF = self.hip.malloc(self.dim * self.W * 8)
        self.dX = self.hip.malloc(self.dim * self.W * 8)

    def _put(self, d, A, skip):
        blk = np.full((self.dim, self.W), MARK)
        blk[:, :self.K] = A
        self.hip.put(d, blk)

    def _get(self, d, A, skip):
        blk = np.empty((self.dim, self.W))
        self.hip.get(blk, d)
        assert np.array_equal(_bits(blk[:, self.K:]), _bits(np.full((self.dim, self.W - self.K), MARK))), "padding columns were written"
        A[:, :] = blk[:, :self.K]

    def apply(self, F, X, skip, expect=0):
        T = self.T
        nrm = np.full(self.K, 99.0)
        sk = self._skip(skip)
        self._put(self.dF, F, skip)
        self._put(self.dX, X, skip)
        self.hip.sync()  # the entries run on the object's own stream: the caller's writes must be complete
        assert self.L.scs_amd_aa_multi_apply_dev(self.a, self.dF, self.dX, sk.ctypes.data_as(T.ip), nrm.ctypes.data_as(T.fp)) == expect
        self._get(self.dF, F, skip)
        return nrm

    def safeguard(self, F, X, skip):
        T = self.T
        rej = np.full(self.K, 99, T.np_int)
        sk = self._skip(skip)
        self._put(self.dF, F, skip)
        self._put(self.dX, X, skip)
        self.hip.sync()
        assert self.L.scs_amd_aa_multi_safeguard_dev(self.a, self.dF, self.dX, sk.ctypes.data_as(T.ip), rej.ctypes.data_as(T.ip)) == 0
        self._get(self.dF, F, skip)
        self._get(self.dX, X, skip)
        return rej

    def close(self):
        if self.a:
            self.hip.free(self.dF)
            self.hip.free(self.dX)
        super().close()


def test_device_entries_give_the_bits_of_the_host_entries_and_leave_the_padding_alone():
    L = _amd()
    K = 5
    spec = MIXED + [(104, K16[4], 0)]
    with Block(L, CONFIG[1], K) as b:
        host = _run_block(b, spec)
    with DevBlock(L, CONFIG[1], K) as b:
        assert b.W == 8
        dev = _run_block(b, spec)
    assert (host[1] == -1).any() and (host[0] > 0).any()
    for x, y in zip(host, dev):
        assert np.array_equal(_bits(x), _bits(y))


# ---- 6. lock step ----------------------------------------------------------------------------------------------------------------
def test_synchronisations_and_launches_do_not_depend_on_the_number_of_columns():
    L = _amd()
    cfg = CONFIG[1]
    mem, dim = cfg[3], cfg[4]
    seen = {}
    for K in (2, 16):
        maps = [_map(dim, 100 + k, 0.03) for k in range(K)]
        with Block(L, cfg, K) as b:
            X = np.zeros((dim, K), order="F")
            Xp = X.copy(order="F")
            skip = np.zeros(K, bool)
            for i in range(mem + 3):
                before = b.counters()
                if i > 0:
                    nrm = b.apply(X, Xp, skip)
                after = b.counters()
                Xp = X.copy(order="F")
                for k in range(K):
                    X[:, k] = maps[k](X[:, k])
                b.safeguard(X, Xp, skip)
            assert min(b.iters()) > mem and (nrm > 0).all()  # the last apply: every memory full, every column solved
            seen[K] = (after[1] - before[1], after[3] - before[3], after[0] - before[0])
    print("per full apply (syncs, launches, applies):", seen)
    assert seen[2][2] == 1 and seen[2] == seen[16]
    assert 0 < seen[2][0] <= mem + 4


# ---- 7. arguments and the failure convention -------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_the_outputs_untouched():
    L = _amd()
    T = L._scs_types
    cfg = CONFIG[4]
    dim = cfg[4]
    for nrhs in (0, 17):
        assert not L.scs_amd_aa_multi_init(dim, nrhs, 4, 4, 1, 1e-8, 1.0, 1.0, 1e10, 5)
    assert not L.scs_amd_aa_multi_init(dim, 4, 4, 4, 1, 1e-8, 3.0, 1.0, 1e10, 5)  # relaxation out of range
    with Block(L, cfg, 4) as b:
        F = np.asfortranarray(np.random.default_rng(1).standard_normal((dim, 4)))
        keep = F.copy(order="F")
        nrm = np.full(4, 7.0)
        rej = np.full(4, 7, T.np_int)
        fpp, npp, rpp = F.ctypes.data_as(T.fp), nrm.ctypes.data_as(T.fp), rej.ctypes.data_as(T.ip)
        for args in ((fpp, dim - 1, fpp, dim), (fpp, dim, fpp, dim - 1), (None, dim, fpp, dim), (fpp, dim, None, dim)):
            assert L.scs_amd_aa_multi_apply(b.a, *args, None, npp) == -1
            assert L.scs_amd_aa_multi_safeguard(b.a, *args, None, rpp) == -1
        assert L.scs_amd_aa_multi_apply(b.a, fpp, dim, fpp, dim, None, None) == -1
        assert L.scs_amd_aa_multi_safeguard(b.a, fpp, dim, fpp, dim, None, None) == -1
        assert L.scs_amd_aa_multi_apply_dev(b.a, None, None, None, npp) == -1
        assert L.scs_amd_aa_multi_safeguard_dev(b.a, None, None, None, rpp) == -1
        assert np.array_equal(_bits(F), _bits(keep)) and (nrm == 7.0).all() and (rej == 7).all()
        assert b.iters() == [0] * 4 and b.counters() == [0] * 4


def test_objects_without_memory_do_nothing():
    """lookback 0: every apply returns 0 and leaves F alone, the safeguard returns 0 -- the single-vector path and blocks alike"""
    L = _amd()
    dim = 300
    rng = np.random.default_rng(4)
    a = L.scs_amd_aa_dev_init(dim, 0, 0, 1, 1e-8, 1.0, 1.0, 1e10, 5)
    assert a
    f, x = rng.standard_normal(dim), rng.standard_normal(dim)
    keep = f.copy()
    for _ in range(3):
        assert L.scs_amd_aa_dev_apply(_p(f), _p(x), a) == 0.0
        assert L.scs_amd_aa_dev_safeguard(_p(f), _p(x), a) == 0
    assert np.array_equal(_bits(f), _bits(keep))
    L.scs_amd_aa_dev_finish(a)
    for K in (1, 3):
        with Block(L, (1, 1e-8, 1.0, 0, dim), K) as b:
            F = np.asfortranarray(rng.standard_normal((dim, K)))
            X = np.asfortranarray(rng.standard_normal((dim, K)))
            keep = F.copy(order="F")
            for _ in range(3):
                assert (b.apply(F, X, np.zeros(K, bool)) == 0).all()
                assert (b.safeguard(F, X, np.zeros(K, bool)) == 0).all()
            assert np.array_equal(_bits(F), _bits(keep)) and b.iters() == [0] * K


def test_hip_failure_inside_an_apply():
    """scs_amd_test_fail_at reports a successful runtime call as failed (it faults nothing): the call returns -1 with every column
    reset, and a run from reset(-1) on the same object reproduces a clean run's bits"""
    L = _amd()
    K = 4
    spec = MIXED
    dim = CONFIG[4][4]
    F = np.asfortranarray(np.random.default_rng(2).standard_normal((dim, K)))
    X = np.asfortranarray(np.random.default_rng(3).standard_normal((dim, K)))
    none = np.zeros(K, bool)
    with Block(L, CONFIG[4], K) as b:
        clean = _run_block(b, spec)
        for where in (0.0, 0.5, 1.0):
            b.reset(-1)
            _run_block(b, spec)  # fills the memories, so that the apply below is a full solve
            big = 10 ** 12
            L.scs_amd_test_fail_at(big)
            b.apply(F.copy(order="F"), X, none)
            total = big - L.scs_amd_test_fail_at(0)  # checked runtime calls of that apply
            assert total >= 8
            b.reset(-1)
            _run_block(b, spec)  # the same state again: the same apply makes the same calls
            k = max(1, int(where * total))
            L.scs_amd_test_fail_at(k)
            b.apply(F.copy(order="F"), X, none, expect=-1)
            assert L.scs_amd_test_fail_at(0) == 0, k  # consumed inside the call
            assert b.iters() == [0] * K  # every column reset
        b.reset(-1)
        again = _run_block(b, spec)
    for x, y in zip(clean, again):
        assert np.array_equal(_bits(x), _bits(y))


def test_memory_is_freed_with_the_object():
    L = _amd()
    cfg = (1, 1e-8, 1.0, 10, 200001)

    def free_bytes():
        v = L.scs_amd_device_free_bytes()
        assert v >= 0
        return v

    def touch(b):
        F = np.zeros((b.dim, b.K), order="F")
        b.apply(F, F.copy(order="F"), np.zeros(b.K, bool))

    with Block(L, cfg, 2) as b:  # warm: context, streams, code objects
        touch(b)
    base = free_bytes()
    b = Block(L, cfg, 8)
    touch(b)
    held = base - free_bytes()
    assert held > 8 * (3 * 10 + 2 * 10 + 1 + 4) * 200001 * 8 * 0.9  # the formula of include/scs_amd.h
    b.close()
    assert abs(free_bytes() - base) <= 8 << 20


# ---- 8. other builds -------------------------------------------------------------------------------------------------------------
def test_dlong_build_gives_the_same_bits():
    spec = MIXED
    res = []
    for lib in ("libscsamd.so", "libscsamd_dlong.so"):
        with Block(_amd(lib), CONFIG[4], 4) as b:
            res.append(_run_block(b, spec))
    assert (res[0][0] > 0).any()
    for x, y in zip(*res):
        assert np.array_equal(_bits(x), _bits(y))


def test_fp32_build_runs():
    """no accuracy bar: fp32 acceleration has none in this project yet"""
    spec = MIXED
    with Block(_amd("libscsamd_f32.so"), CONFIG[4], 4) as b:
        assert b.T.np_float is np.float32
        nrm, rej, traj, _ = _run_block(b, spec)
    assert np.isfinite(traj).all() and (nrm > 0).any()


# ---- 9. the Python object --------------------------------------------------------------------------------------------------------
class PyBlock:
    """scs_amd.accel.Accel behind the interface of Block"""

    def __init__(self, cfg, K):
        from scs_amd.accel import Accel
        type1, reg, relax, mem, dim = cfg
        self.o = Accel(dim, K, lookback=mem, type1=bool(type1), regularization=reg, relaxation=relax)
        self.K, self.dim, self.mem, self.T = K, dim, mem, capi.T64

    def apply(self, F, X, skip):
        return self.o.apply_many(F, X, skip)

    def safeguard(self, F, X, skip):
        return self.o.safeguard_many(F, X, skip)

    def reset(self, col):
        self.o.reset(None if col < 0 else col)

    def iters(self):
        return [self.o.stats(k)["iter"] for k in range(self.K)]


def test_python_object():
    from scs_amd.accel import Accel
    L = _amd()
    K = 4
    spec = MIXED
    with Block(L, CONFIG[4], K) as b:
        want = _run_block(b, spec)
    pb = PyBlock(CONFIG[4], K)
    with pb.o:
        got = _run_block(pb, spec)
        c = pb.o.counters()
        assert c["applies"] == ITERS - 1 and c["launches"] > 0
        dim = pb.dim
        F = np.zeros((dim, K), order="F")
        for bad in (np.zeros((dim, K + 1), order="F"), np.zeros((dim, K - 1), order="F"), np.zeros(dim)):
            with pytest.raises(ValueError):
                pb.o.apply_many(bad, F)
            with pytest.raises(ValueError):
                pb.o.apply_many(F, bad)
            with pytest.raises(ValueError):
                pb.o.safeguard_many(F, bad)
        with pytest.raises(ValueError):
            pb.o.apply_many(F, F, skip=[0] * (K + 1))
    for x, y in zip(want, got):
        assert np.array_equal(_bits(x), _bits(y))
    assert pb.o._a is None  # the context manager freed the object
    with pytest.raises(RuntimeError):
        pb.o.apply_many(F, F)
    with pytest.raises(ValueError):
        Accel(100, 17)
