"""Inputs to data equilibration at the shapes where it can go wrong unnoticed (tests/test_equilibrate_edges_cpu.py holds the host
code to the reference on them, tests/test_equilibrate_edges_gpu.py the device code to the host code; profiles/equilibrate_edges.md
says which kernel or branch each one is the only case to reach).

Every case is RAW CSC: (Ap, Ai, Ax) for A, the same for the upper triangle of P or None, and a cone dict.  Nothing goes through
scipy.sparse: columns may be unsorted, hold the same (row, column) twice with different values, and hold explicit zeros -- the
reference accepts all of that, and a canonicalising round trip would keep it out of the tests.  All arrays are float64 / int64
here; tests/test_equilibrate.py::_equilibrate_raw casts them to the types of the library it calls (fp32, 64-bit indices).

`CASES` maps a name to a builder; `build(name)` memoises, and hands out the same read-only arrays every time."""
from collections import namedtuple

import numpy as np

from scs_amd import capi

Case = namedtuple("Case", "name m n Ap Ai Ax P cone")  # P: None or (Pp, Pi, Px)

TR_SHORT, TR_LONG_MAX, SMALL_CONE = 32, 4096, 64  # the thresholds of equilibrate_dev.hip that the shapes below straddle
MIN_CLIP, MAX_CLIP = 1e-4, 1e4


def _csc(m, n, cols):
    """cols: one (rows, vals) pair per column, kept in the order given"""
    assert len(cols) == n
    Ap = np.zeros(n + 1, dtype=np.int64)
    Ap[1:] = np.cumsum([len(r) for r, _ in cols])
    Ai = np.concatenate([np.asarray(r, dtype=np.int64) for r, _ in cols]) if Ap[-1] else np.zeros(0, dtype=np.int64)
    Ax = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in cols]) if Ap[-1] else np.zeros(0)
    assert len(Ai) == len(Ax) == Ap[-1] and (len(Ai) == 0 or (Ai.min() >= 0 and Ai.max() < m))
    return Ap, Ai, Ax


def _from_triplets(m, n, rows, cols, vals, rng=None):
    """entries grouped by column; inside a column in the order given, or shuffled when an rng is passed"""
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    out = []
    for j in range(n):
        sel = np.flatnonzero(cols == j)
        if rng is not None:
            sel = rng.permutation(sel)
        out.append((rows[sel], vals[sel]))
    return _csc(m, n, out)


def _case(name, m, n, A, P, cone):
    assert capi.cone_rows(cone) == m, (name, capi.cone_rows(cone), m)
    if P is not None:
        Pp, Pi, _ = P
        assert len(Pp) == n + 1
        assert all(Pi[k] <= j for j in range(n) for k in range(Pp[j], Pp[j + 1])), "P must be upper triangular"
    for a in A + (P or ()):
        a.setflags(write=False)
    return Case(name, m, n, A[0], A[1], A[2], P, cone)


def _col_scales(rng, n):
    """entry magnitudes spread over 1e-3 .. 50, one scale per column"""
    return rng.choice([1e-3, 1.0, 50.0], size=n)


# ---------------------------------------------------------------------------------------------------------------------------------
# row_lengths / row_too_long: the device transpose sorts a row's slots with one lane up to TR_SHORT entries, with a bitonic sort in
# LDS (padded to a power of two, at least 64) up to TR_LONG_MAX, and leaves the whole pattern to the host beyond
# ---------------------------------------------------------------------------------------------------------------------------------
def _row_lengths(name, longest):
    rng = np.random.default_rng(11)
    n, z, q = 4200, 580, 20
    m = z + q
    length = rng.integers(2, 5, size=m)
    length[:3] = (0, 1, 2)
    length[z:z + 6] = (32, 33, 64, 65, 1000, longest)  # the long rows share one second-order cone
    rows, cols = [], []
    for i in range(m):
        cols.append(rng.choice(n, size=length[i], replace=False))  # distinct columns: the row has exactly this many entries
        rows.append(np.full(length[i], i))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(-1, 1, size=len(rows)) * _col_scales(rng, n)[cols]
    vals[vals == 0] = 0.5
    A = _from_triplets(m, n, rows, cols, vals, rng)
    assert np.array_equal(np.bincount(A[1], minlength=m), length)
    return _case(name, m, n, A, None, dict(z=z, q=[q]))


def _dups_unsorted():
    rng = np.random.default_rng(12)
    m, n = 70, 50
    cone = dict(z=10, l=20, q=[15, 25])
    out = []
    for j in range(n):
        r = rng.choice(m, size=7, replace=False)
        v = rng.uniform(-1, 1, size=7) * rng.choice([1e-3, 1.0, 50.0])
        dup = rng.random(7) < 0.1
        if j == 0:
            dup[0] = True
        r, v = np.concatenate([r, r[dup]]), np.concatenate([v, rng.uniform(-2, 2, size=int(dup.sum()))])  # stored twice
        if j % 7 == 3:
            v[rng.integers(len(v))] = 0.0  # explicit zero
        order = np.argsort(-r, kind="stable") if j % 2 == 0 else rng.permutation(len(r))
        out.append((r[order], v[order]))
    A = _csc(m, n, out)
    assert any(len(np.unique(r)) < len(r) for r, _ in out) and (A[2] == 0).sum() >= 3
    return _case("dups_unsorted", m, n, A, None, cone)


# ---------------------------------------------------------------------------------------------------------------------------------
# empty: rows, columns and whole cones without an entry (statistic 0 -> scale 1), and the smallest problems there are
# ---------------------------------------------------------------------------------------------------------------------------------
def _empty_rows_cols():
    rng = np.random.default_rng(13)
    cone = dict(z=3, l=5, q=[6, 4, 8], s=[3], ep=1)
    m, n = capi.cone_rows(cone), 12
    off_q4 = 3 + 5 + 6
    dead_rows = {1, 5, 9} | set(range(off_q4, off_q4 + 4))  # two first-segment rows, one cone row, and ALL rows of the q = 4 cone
    dead_cols = {0, 7, 11}
    zero_rows = {6, off_q4 + 4 + 2}  # rows that hold nothing but explicit zeros: one row-wise, one inside the q = 8 cone
    rows, cols, vals = [], [], []
    for j in range(n):
        if j in dead_cols:
            continue
        for i in rng.choice(m, size=9, replace=False):
            if i in dead_rows:
                continue
            rows.append(i), cols.append(j)
            vals.append(0.0 if i in zero_rows else rng.uniform(0.1, 1.0) * rng.choice([-1, 1]) * rng.choice([1e-3, 1.0, 50.0]))
    for i in zero_rows:
        rows.append(i), cols.append(3), vals.append(0.0)
    A = _from_triplets(m, n, rows, cols, vals, rng)
    return _case("empty/rows_cols", m, n, A, None, cone)


def _empty_1x1():
    return _case("empty/1x1", 1, 1, _csc(1, 1, [([0], [-3.0])]), None, dict(l=1))


def _empty_one_column():
    rng = np.random.default_rng(14)
    m = 300
    r = rng.permutation(m)[:200]
    v = rng.uniform(-1, 1, size=200) * rng.choice([1e-3, 1.0, 50.0], size=200)
    return _case("empty/n1_m300", m, 1, _csc(m, 1, [(r, v)]), None, dict(z=10, l=20, q=[270]))


def _empty_m257():
    rng = np.random.default_rng(15)
    m, n = 257, 5  # one row past a block of the one-lane-per-row kernels
    out = []
    for j in range(n):
        r = rng.permutation(m)[:60]
        if j == 0:
            r = np.concatenate([r[r != m - 1], [m - 1]])  # the last row is not empty
        out.append((r, rng.uniform(-1, 1, size=len(r)) * rng.choice([1e-3, 1.0, 50.0])))
    return _case("empty/m257", m, n, _csc(m, n, out), None, dict(l=100, q=[157]))


def _empty_nnz0():
    e = np.zeros(0, dtype=np.int64)
    return _case("empty/nnz0", 6, 3, _csc(6, 3, [(e, np.zeros(0))] * 3), None, dict(l=2, q=[4]))


# ---------------------------------------------------------------------------------------------------------------------------------
# clip: a statistic below 1e-4 is replaced by 1, one above 1e4 is clamped to 1e4.  The special rows meet only ordinary columns and
# the special columns only ordinary rows, so that each one's largest entry is exactly the value named.
# ---------------------------------------------------------------------------------------------------------------------------------
CLIP_VALUES = (MIN_CLIP, 9.9e-5, MAX_CLIP, 1e6, 1e-9)


def _clip(with_p):
    rng = np.random.default_rng(16 + with_p)
    n, cone = 40, dict(l=40, q=[5, 5, 10])
    m = capi.cone_rows(cone)
    sp_rows = list(range(5))        # row-wise rows whose largest entry is CLIP_VALUES[i]
    sp_cols = list(range(5))        # columns whose largest entry is CLIP_VALUES[j]
    cone_a, cone_b = range(40, 45), range(45, 50)  # cones whose largest entry is 1e6 (clamped) and 9.9e-5 (replaced by 1)
    rows, cols, vals = [], [], []

    def put(i, j, v):
        rows.append(i), cols.append(j), vals.append(v)

    small_rows = set(sp_rows) | set(cone_a) | set(cone_b)
    for j in range(5, n):  # ordinary columns over ordinary rows
        for i in rng.choice([i for i in range(m) if i not in small_rows], size=8, replace=False):
            put(i, j, rng.uniform(0.2, 1.0) * rng.choice([-1, 1]) * rng.choice([0.05, 1.0, 30.0]))
    for t, top in enumerate(CLIP_VALUES):
        cs_ = rng.choice(range(5, n), size=4, replace=False)  # special row t: entries <= top, in ordinary columns
        for u, j in enumerate(cs_):
            put(sp_rows[t], j, (top if u == 0 else top * rng.uniform(0.1, 0.9)) * (-1) ** u)
        rs_ = rng.choice(range(5, 40), size=4, replace=False)  # special column t: entries <= top, in ordinary row-wise rows
        for u, i in enumerate(rs_):
            put(i, sp_cols[t], (top if u == 0 else top * rng.uniform(0.1, 0.9)) * (-1) ** u)
    for rws, top in ((cone_a, 1e6), (cone_b, 9.9e-5)):
        for u, i in enumerate(rws):
            put(i, int(rng.integers(5, n)), (top if u == 4 else top * rng.uniform(0.1, 0.9)) * (-1) ** u)
    A = _from_triplets(m, n, rows, cols, vals, rng)
    P = None
    if with_p:
        d = rng.uniform(0.5, 2.0, size=n)
        d[7], d[8] = 1e8, 1e-7
        pc = [([j], [d[j]]) for j in range(n)]
        pc[20] = ([3, 20], [0.3, d[20]])  # one off-diagonal entry, so that P is not a pure diagonal
        P = _csc(n, n, pc)
    return _case("clip/P" if with_p else "clip/A", m, n, A, P, cone)


# ---------------------------------------------------------------------------------------------------------------------------------
# segments: every cone family that has its own segment, no row-wise rows at all, and second-order cones on both sides of the
# one-lane / one-workgroup switch (SMALL_CONE) and of the workgroup's 256 lanes.  The largest entry of every cone sits in its LAST
# row, so that a strided loop that drops its tail finds another maximum.
# ---------------------------------------------------------------------------------------------------------------------------------
def _segments():
    rng = np.random.default_rng(18)
    cone = dict(q=[0, 1, 2, 63, 64, 65, 255, 256, 257, 1000], s=[0, 1, 10, 11], cs=[8, 9], ep=2, ed=1, p=[0.3, -0.6])
    seg = list(cone["q"]) + [s * (s + 1) // 2 for s in cone["s"]] + [c * c for c in cone["cs"]] + [3] * 5
    m, n = capi.cone_rows(cone), 60
    assert sum(seg) == m
    scale = _col_scales(rng, n)
    rows, cols, vals = [], [], []
    for j in range(n):
        r = rng.choice(m, size=40, replace=False)
        rows.append(r), cols.append(np.full(40, j)), vals.append(rng.uniform(-1, 1, size=40) * scale[j])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    pos, last_r, last_c, last_v = 0, [], [], []
    for ln in seg:
        if ln >= 2:
            keep = rows != pos + ln - 1  # the last row holds the cone's largest entry and nothing else
            rows, cols, vals = rows[keep], cols[keep], vals[keep]
            last_r.append(pos + ln - 1), last_c.append(int(rng.integers(n))), last_v.append(-rng.uniform(1e3, 2e3))
        pos += ln
    rows, cols, vals = np.concatenate([rows, last_r]), np.concatenate([cols, last_c]), np.concatenate([vals, last_v])
    A = _from_triplets(m, n, rows, cols, vals, rng)
    return _case("segments", m, n, A, None, cone)


def _first_segment(with_q):
    rng = np.random.default_rng(19)
    cone = dict(z=5, l=7, bu=[1.0, 2.0, 3.0], bl=[-1.0, -2.0, 0.0])
    if with_q:
        cone["q"] = [3]
    m, n = capi.cone_rows(cone), 10
    out = []
    for j in range(n):
        r = rng.permutation(16)[:5]  # the same rows in both variants ...
        v = rng.uniform(-1, 1, size=5) * rng.choice([1e-3, 1.0, 50.0])
        if with_q:  # ... and one more in the appended cone
            r, v = np.concatenate([r, [16 + j % 3]]), np.concatenate([v, [3.0 + j]])
        out.append((r, v))
    return _case("first_segment_only/q3" if with_q else "first_segment_only/box", m, n, _csc(m, n, out), None, cone)


# ---------------------------------------------------------------------------------------------------------------------------------
# p_shapes: one A, eight P
# ---------------------------------------------------------------------------------------------------------------------------------
P_SHAPES = ("diag", "strict_upper", "empty_cols", "nnz0", "dense", "zeros_dup", "dominant", "negligible")


def _p_shape(kind):
    rng = np.random.default_rng(20)
    n, cone = 40, dict(z=10, l=20, q=[30])
    m = capi.cone_rows(cone)
    scale = _col_scales(rng, n)
    out = []
    for j in range(n):
        out.append((rng.permutation(m)[:6], rng.uniform(-1, 1, size=6) * scale[j]))
    A = _csc(m, n, out)
    rng = np.random.default_rng(21 + P_SHAPES.index(kind))
    full = np.triu(rng.uniform(-1, 1, size=(n, n)))

    def cols_of(mask, M=full, shuffle=True):
        pc = []
        for j in range(n):
            r = np.flatnonzero(mask[:j + 1, j])
            if shuffle:
                r = rng.permutation(r)
            pc.append((r, M[r, j]))
        return pc

    sparse = np.triu(rng.random((n, n)) < 0.15)
    if kind == "diag":
        pc = cols_of(np.eye(n, dtype=bool), np.diag(rng.uniform(0.1, 5.0, size=n)))
    elif kind == "strict_upper":
        pc = cols_of(sparse & ~np.eye(n, dtype=bool))
    elif kind == "empty_cols":
        mask = sparse | np.eye(n, dtype=bool)
        mask[:, ::3] = False  # every third column empty; their rows still receive the mirrored entries
        pc = cols_of(mask)
    elif kind == "nnz0":
        pc = cols_of(np.zeros((n, n), dtype=bool))
    elif kind == "dense":
        pc = cols_of(np.triu(np.ones((n, n), dtype=bool)))
        assert sum(len(r) for r, _ in pc) == 820
    elif kind == "zeros_dup":
        M = full.copy()
        mask = sparse | np.eye(n, dtype=bool)
        zr, zc = np.nonzero(mask)
        pick = rng.choice(len(zr), size=6, replace=False)
        M[zr[pick], zc[pick]] = 0.0  # explicit zeros, one of them possibly on the diagonal
        M[5, 5] = 0.0
        pc = cols_of(mask, M)
        r, v = pc[17]
        pc[17] = (np.concatenate([r, r[:1]]), np.concatenate([v, [0.75]]))  # one entry stored twice
    elif kind == "dominant":
        pc = cols_of(sparse | np.eye(n, dtype=bool), full * 1e3 + np.diag(rng.uniform(1e3, 5e3, size=n)))
    elif kind == "negligible":
        pc = cols_of(sparse | np.eye(n, dtype=bool), full * 1e-7)
    else:
        raise KeyError(kind)
    return _case("p_shapes/" + kind, m, n, A, _csc(n, n, pc), cone)


CASES = {
    "row_lengths": lambda: _row_lengths("row_lengths", TR_LONG_MAX),
    "row_too_long": lambda: _row_lengths("row_too_long", TR_LONG_MAX + 1),
    "dups_unsorted": _dups_unsorted,
    "empty/rows_cols": _empty_rows_cols,
    "empty/1x1": _empty_1x1,
    "empty/n1_m300": _empty_one_column,
    "empty/m257": _empty_m257,
    "empty/nnz0": _empty_nnz0,
    "clip/A": lambda: _clip(False),
    "clip/P": lambda: _clip(True),
    "segments": _segments,
    "first_segment_only/box": lambda: _first_segment(False),
    "first_segment_only/q3": lambda: _first_segment(True),
}
CASES.update({"p_shapes/" + kind: (lambda kind=kind: _p_shape(kind)) for kind in P_SHAPES})
NAMES = tuple(CASES)
_built = {}


def build(name):
    if name not in _built:
        _built[name] = CASES[name]()
        assert _built[name].name == name
    return _built[name]


def segments_of(cone):
    """row counts of the first (row-wise) block and of every cone after it, in the order the rows come"""
    seg = [capi.cone_rows({k: cone[k] for k in ("z", "l", "bu", "bl", "bsize") if k in cone})]
    seg += [int(q) for q in cone.get("q", [])]
    seg += [int(s) * (int(s) + 1) // 2 for s in cone.get("s", [])]
    seg += [int(c) ** 2 for c in cone.get("cs", [])]
    seg += [3] * (cone.get("ep", 0) + cone.get("ed", 0) + len(cone.get("p", [])))
    return seg
