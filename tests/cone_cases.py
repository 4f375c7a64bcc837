"""Inputs to the cone projection whose answers are known in closed form (tests/test_cones_degenerate_gpu.py runs them through
the kernels, tests/test_cone_cases_cpu.py checks them against numpy without a GPU).

The entries under test compute y = x + Proj_K(-x) = Proj_{K*}(x).  The second-order, PSD and nonnegative cones are self dual, so
there `expected` is simply Proj_K(x); the zero cone's dual is everything (y = x); the box cone is not self dual and its expected
vector is x + Proj_K(-x) with t the exact root of the piecewise-linear gradient.

Every generator returns a `Case`: (cone dict, x, expected, scale, ...).  `scale` holds one number per ROW: the Frobenius norm of
the PSD block the row belongs to, the infinity norm of its second-order cone, max(1, t) for the box cone.  An error is measured as
|got - expected| / scale row by row -- never against max(1, .) of the whole vector -- and rows whose `exact` flag is set (and every
row of scale 0) must come back bit for bit equal.  `parts` names the row ranges (family, order, scale) for the reports."""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "cone x expected scale exact parts D")
Part = namedtuple("Part", "label lo hi")

SCALES = (2.0 ** -40, 1.0, 2.0 ** 40)  # powers of two: scaling a case is exact
PSD_ORDERS = (2, 3, 7, 50, 51, 72, 73, 92, 93, 128, 129)  # both sides of every switch of the PSD kernels
CS_ORDERS = (1, 2, 3, 25, 26, 36, 37, 46, 47, 64, 65)     # Hermitian blocks: real embeddings of twice the order
SOC_SIZES = (1, 2, 3, 16, 17, 2048, 2049, 4096, 4097)
BOX_SIZES = (1023, 1024, 1025, 16383, 16384, 16385, 65536, 65537)
SQRT2 = math.sqrt(2.0)


def _case(cone, x, expected, scale, exact, parts, D=None):
    x, expected = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(expected, dtype=np.float64)
    scale, exact = np.ascontiguousarray(scale, dtype=np.float64), np.ascontiguousarray(exact, dtype=bool)
    assert x.shape == expected.shape == scale.shape == exact.shape and x.ndim == 1
    return Case(cone, x, expected, scale, exact, parts, D)


def rel_err(got, case, lo=0, hi=None):
    """max over rows lo..hi of |got - expected| / scale; rows of scale 0 count as 0 when equal and inf when not"""
    hi = len(case.x) if hi is None else hi
    d = np.abs(np.asarray(got, dtype=np.float64)[lo:hi] - case.expected[lo:hi])
    s = case.scale[lo:hi]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(s > 0, d / s, np.where(d == 0, 0.0, np.inf))
    return float(e.max()) if len(e) else 0.0


def exact_rows(case):
    return case.exact | (case.scale == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# PSD blocks, real (packed lower triangle, column major, off-diagonals * sqrt 2) and complex Hermitian (column c: the real diagonal
# entry, then (re, im) * sqrt 2 of the rows below it)
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_psd(X):
    k = X.shape[0]
    cols, rows = np.triu_indices(k)  # (col <= row): the lower triangle in column-major order
    return X[rows, cols] * np.where(rows == cols, 1.0, SQRT2)


def unpack_psd(v, k):
    cols, rows = np.triu_indices(k)
    X = np.zeros((k, k))
    X[rows, cols] = v / np.where(rows == cols, 1.0, SQRT2)
    return X + np.tril(X, -1).T


def pack_herm(H):
    n = H.shape[0]
    out = np.empty(n * n)
    for c in range(n):
        o = c * (2 * n - c)
        out[o] = H[c, c].real
        out[o + 1:o + 1 + 2 * (n - c - 1):2] = H[c + 1:, c].real * SQRT2
        out[o + 2:o + 2 + 2 * (n - c - 1):2] = H[c + 1:, c].imag * SQRT2
    return out


def unpack_herm(v, n):
    H = np.zeros((n, n), dtype=complex)
    for c in range(n):
        o = c * (2 * n - c)
        H[c, c] = v[o]
        H[c + 1:, c] = (v[o + 1:o + 1 + 2 * (n - c - 1):2] + 1j * v[o + 2:o + 2 + 2 * (n - c - 1):2]) / SQRT2
    return H + np.tril(H, -1).conj().T


def _unit(k, rng, cplx):
    v = rng.standard_normal(k) + (1j * rng.standard_normal(k) if cplx else 0.0)
    return v / np.linalg.norm(v)


def _unit_pair(k, rng, cplx):
    v = _unit(k, rng, cplx)
    if k == 1:
        return v, np.zeros_like(v)
    w = _unit(k, rng, cplx)
    w = w - v * np.vdot(v, w)
    return v, w / np.linalg.norm(w)


def _outer(v):
    return np.outer(v, np.conj(v))


def _householder(k, rng, cplx):
    I, vv = np.eye(k, dtype=complex if cplx else float), _outer(_unit(k, rng, cplx))
    return I - 2.0 * vv, I - vv


def _spd(k, rng, cplx):
    """strictly positive definite, eigenvalues 1 .. 1e3"""
    Z = rng.standard_normal((k, k)) + (1j * rng.standard_normal((k, k)) if cplx else 0.0)
    Q, _ = np.linalg.qr(Z)
    lam = np.logspace(0.0, 3.0, k) if k > 1 else np.array([7.0])
    A = (Q * lam) @ Q.conj().T
    return 0.5 * (A + A.conj().T)


def _psd_family(family, k, rng, cplx):
    """(X, Proj_PSD(X), exact) of order k at scale 1"""
    dt = complex if cplx else float
    I, Z = np.eye(k, dtype=dt), np.zeros((k, k), dtype=dt)
    if family == "zero":
        return Z, Z, True
    if family == "plus_identity":
        return I, I, True  # positive definite: Proj(-x) is all zeros, y == x
    if family == "minus_identity":
        return -I, Z, False
    if family == "diagonal":  # mixed sign, repeated values (a_pp == a_qq) and zeros
        d = rng.choice(np.array([-3.0, -1.0, 0.0, 0.5, 2.0, 2.0]), size=k)
        if k >= 2:
            d[0], d[1] = 2.0, -3.0
        return np.diag(d).astype(dt), np.diag(np.maximum(d, 0.0)).astype(dt), False
    if family == "householder":  # eigenvalue +1 with multiplicity k - 1: d = 0 pairs everywhere
        H, P = _householder(k, rng, cplx)
        return H, P, False
    if family in ("rank_one", "minus_rank_one"):
        R = 3.0 * _outer(_unit(k, rng, cplx))
        return (R, R, False) if family == "rank_one" else (-R, Z, False)
    if family == "rank_two":
        v, w = _unit_pair(k, rng, cplx)
        return 2.0 * _outer(v) - 5.0 * _outer(w), 2.0 * _outer(v), False
    if family == "two_householder":  # block diagonal under a symmetric permutation: most off-diagonal entries are exactly zero
        k1 = k // 2
        X, P = Z.copy(), Z.copy()
        for lo, hi in ((0, k1), (k1, k)):
            if hi > lo:
                X[lo:hi, lo:hi], P[lo:hi, lo:hi] = _householder(hi - lo, rng, cplx)
        p = rng.permutation(k)
        return X[np.ix_(p, p)], P[np.ix_(p, p)], False
    if family == "corner_householder":
        # a Householder block in the leading corner, diagonal elsewhere, not permuted: whole groups of columns stop rotating
        # while their neighbours still do, so the blocked iteration moves tiles that no rotation touches right after a step
        # that changed them
        c = max(1, (3 * k) // 8)
        d = rng.choice(np.array([-3.0, -1.0, 0.0, 0.5, 2.0, 2.0]), size=k)
        X, P = np.diag(d).astype(dt), np.diag(np.maximum(d, 0.0)).astype(dt)
        X[:c, :c], P[:c, :c] = _householder(c, rng, cplx)
        return X, P, False
    if family == "positive_definite":
        A = _spd(k, rng, cplx)
        return A, A, True
    if family == "negative_definite":
        return -_spd(k, rng, cplx), Z, False
    raise KeyError(family)


PSD_FAMILIES = ("zero", "plus_identity", "minus_identity", "diagonal", "householder", "rank_one", "minus_rank_one", "rank_two",
                "two_householder", "positive_definite", "negative_definite", "corner_householder")


def psd_block(family, k, scale=1.0, seed=0, cplx=False):
    """(x, expected, Frobenius norm, exact) of one packed block"""
    rng = np.random.default_rng([seed, k, PSD_FAMILIES.index(family), int(cplx)])
    X, P, exact = _psd_family(family, k, rng, cplx)
    X, P = X * scale, P * scale
    pack = pack_herm if cplx else pack_psd
    return pack(X), pack(P), float(np.linalg.norm(X)), exact


def psd_dense_block(k, scale=1.0, seed=0):
    """the generic case the other tests use: a Gaussian vector, its answer from numpy's eigh"""
    rng = np.random.default_rng([seed, k, 99])
    x = rng.standard_normal(k * (k + 1) // 2) * scale
    X = unpack_psd(x, k)
    lam, V = np.linalg.eigh(X)
    return x, pack_psd((V * np.maximum(lam, 0.0)) @ V.T), float(np.linalg.norm(X)), False


def psd_case(blocks, seed=0):
    """blocks: list of (family, order, scale, cplx) -- real blocks first, as the cone lists them.  family "dense": Gaussian (real
    blocks only).  Block i draws from the stream (seed + i)."""
    assert all(not b[3] for b in blocks[:sum(1 for b in blocks if not b[3])])
    xs, es, sc, ex, parts, o = [], [], [], [], [], 0
    for i, (family, k, scale, cplx) in enumerate(blocks):
        x, e, fro, exact = psd_dense_block(k, scale, seed + i) if family == "dense" else psd_block(family, k, scale, seed + i, cplx)
        xs.append(x), es.append(e), sc.append(np.full(len(x), fro)), ex.append(np.full(len(x), exact))
        parts.append(Part(f"{'cs' if cplx else 's'} {family} order {k} scale 2^{int(round(math.log2(scale)))}", o, o + len(x)))
        o += len(x)
    cone = {}
    if any(not b[3] for b in blocks):
        cone["s"] = [b[1] for b in blocks if not b[3]]
    if any(b[3] for b in blocks):
        cone["cs"] = [b[1] for b in blocks if b[3]]
    return _case(cone, np.concatenate(xs), np.concatenate(es), np.concatenate(sc), np.concatenate(ex), parts)


def psd_order_case(k, cplx=False):
    """one cone of blocks of order k alone (so every order is also its launch's largest block): every family at every scale"""
    return psd_case([(f, k, s, cplx) for f in PSD_FAMILIES for s in SCALES])


def psd_cases_by_order(cplx=False):
    for k in (CS_ORDERS if cplx else PSD_ORDERS):
        yield k, psd_order_case(k, cplx)


def psd_mixed_case():
    """every order in ONE cone, real and Hermitian, family and scale changing from block to block: a block of norm 2^-40 sits
    next to one of norm 2^40"""
    blocks = [(PSD_FAMILIES[(3 * i) % len(PSD_FAMILIES)], k, SCALES[i % 3], False) for i, k in enumerate(PSD_ORDERS + PSD_ORDERS[::-1])]
    blocks += [(PSD_FAMILIES[(5 * i + 1) % len(PSD_FAMILIES)], k, SCALES[(i + 1) % 3], True) for i, k in enumerate(CS_ORDERS)]
    return psd_case(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------
# second-order cones
# ---------------------------------------------------------------------------------------------------------------------------------
def soc_closed_form(x):
    """Proj_SOC of a generic point: the tail norm from an exactly rounded sum, then the closed form"""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 1:
        return np.maximum(x, 0.0)
    s = math.sqrt(math.fsum(float(t) * float(t) for t in x[1:]))
    v = float(x[0])
    if s <= v:
        return x.copy()
    if s <= -v:
        return np.zeros_like(x)
    a = 0.5 * (s + v)
    out = x * (a / s)
    out[0] = a
    return out


SOC_FAMILIES = ("zero", "head_pos", "head_neg", "boundary", "boundary_polar", "ulp_outside", "ulp_outside_polar", "single_first",
                "single_2047", "single_2048", "single_last", "single_last_neg_head", "inside", "polar", "generic")


def soc_vector(family, q, rng):
    """(x, Proj_SOC(x), exact) at scale 1, or None where the family needs a longer cone"""
    x = np.zeros(q)
    if family == "zero":
        return x, x.copy(), True
    if family in ("head_pos", "head_neg"):  # the tail is zero
        x[0] = 2.5 if family == "head_pos" else -2.5
        return x, np.maximum(x, 0.0), True
    if q == 1:
        return None
    if family in ("boundary", "boundary_polar", "ulp_outside", "ulp_outside_polar"):
        if q == 2:
            x[1] = -5.0
        else:  # 3, 4, 5 padded with zeros; the two entries in different tiles of a tiled cone
            x[1], x[q - 1] = 3.0, -4.0
        if family == "boundary":  # |tail| == head exactly: unchanged
            x[0] = 5.0
            return x, x.copy(), True
        if family == "boundary_polar":  # |tail| == -head exactly: 0
            x[0] = -5.0
            return x, np.zeros(q), True
        x[0] = math.nextafter(5.0, 0.0) if family == "ulp_outside" else math.nextafter(-5.0, 0.0)
        a = (5.0 + x[0]) / 2.0  # exact: both are multiples of the same ulp
        e = x * (a / 5.0)
        e[0] = a
        return x, e, False
    if family.startswith("single"):  # one nonzero tail entry: alpha = (|a| + v) / 2 exactly
        row = dict(single_first=1, single_2047=2047, single_2048=2048).get(family, q - 1)
        if row >= q or (family in ("single_2047", "single_2048") and row == q - 1):
            return None
        v, a = (-1.0, 3.0) if family == "single_last_neg_head" else (1.0, -3.0)
        x[0], x[row] = v, a
        e = np.zeros(q)
        e[0] = (abs(a) + v) / 2.0
        e[row] = math.copysign(e[0], a)
        return x, e, False
    x[1:] = rng.standard_normal(q - 1)
    nrm = float(np.linalg.norm(x[1:]))
    if family == "inside":
        x[0] = 2.0 * nrm + 1.0
        return x, x.copy(), True
    if family == "polar":
        x[0] = -2.0 * nrm - 1.0
        return x, np.zeros(q), True
    if family == "generic":
        x[0] = 0.3 * nrm
        return x, soc_closed_form(x), False
    raise KeyError(family)


def soc_case(cones, seed=0):
    """cones: list of (family, q, scale) laid one after another in one cone; entries whose family does not fit q are dropped"""
    xs, es, sc, ex, parts, qs, o = [], [], [], [], [], [], 0
    for i, (family, q, scale) in enumerate(cones):
        got = soc_vector(family, q, np.random.default_rng([seed, i, q]))
        if got is None:
            continue
        x, e, exact = got
        x, e = x * scale, e * scale
        xs.append(x), es.append(e), sc.append(np.full(q, np.abs(x).max())), ex.append(np.full(q, exact)), qs.append(q)
        parts.append(Part(f"q {family} size {q} scale 2^{int(round(math.log2(scale)))}", o, o + q))
        o += q
    return _case(dict(q=qs), np.concatenate(xs), np.concatenate(es), np.concatenate(sc), np.concatenate(ex), parts)


def soc_all_sizes_case():
    """every family at every size, the scale changing from cone to cone"""
    return soc_case([(f, q, SCALES[(i + j) % 3]) for i, f in enumerate(SOC_FAMILIES) for j, q in enumerate(SOC_SIZES)])


def soc_all_sizes_one_scale(scale):
    return soc_case([(f, q, scale) for f in SOC_FAMILIES for q in SOC_SIZES], seed=1)


def soc_many_tiny_case(n=40000):
    """n cones of size 3 cycling through the families and the scales: the grid-stride loop of the one-lane-per-cone kernel"""
    fams = [f for f in SOC_FAMILIES if f not in ("single_2047", "single_2048")]
    return soc_case([(fams[i % len(fams)], 3, SCALES[(i // len(fams)) % 3]) for i in range(n)], seed=2)


# ---------------------------------------------------------------------------------------------------------------------------------
# zero cone and nonnegative orthant
# ---------------------------------------------------------------------------------------------------------------------------------
def zero_nonneg_case(z, l, seed=0):
    rng = np.random.default_rng([seed, z, l])
    n = z + l
    x = rng.standard_normal(n) * rng.choice(np.array(SCALES), size=n)
    x[::5] = 0.0
    x[1::7] = -0.0
    e = x.copy()
    e[z:] = np.maximum(x[z:], 0.0)
    cone = {}
    if z:
        cone["z"] = z
    if l:
        cone["l"] = l
    return _case(cone, x, e, np.maximum(np.abs(x), 1.0), np.ones(n, dtype=bool), [Part(f"z {z} l {l}", 0, n)])


ZERO_NONNEG_SHAPES = ((0, 1), (1, 0), (0, 257), (255, 0), (100, 157), (1000, 1001), (300, 0), (0, 513))


# ---------------------------------------------------------------------------------------------------------------------------------
# box cone {(t, s): t bl <= s <= t bu, t >= 0}
# ---------------------------------------------------------------------------------------------------------------------------------
def box_effective_bounds(bl, bu, D=None):
    """the bounds the projection uses: with a row scaling D, |bound| >= 1e15 becomes infinite and the others are rescaled by
    D[j + 1] / D[0]; without one they are used as given"""
    bl, bu = np.asarray(bl, dtype=np.float64), np.asarray(bu, dtype=np.float64)
    if D is None:
        return bl.copy(), bu.copy()
    f = np.asarray(D, dtype=np.float64)[1:] / float(D[0])
    return np.where(bl <= -1e15, -np.inf, bl * f), np.where(bu >= 1e15, np.inf, bu * f)


def _active(w, t, bl, bu):
    """rows above t bu / below t bl, with the convention of the reference's comparisons: at t = 0 an infinite bound gives
    0 * inf = NaN, which compares false, so an infinitely bounded row is left alone there"""
    with np.errstate(invalid="ignore"):
        tu, tl = t * bu, t * bl
        hi = w > tu
        lo = ~hi & (w < tl)
    return hi, lo, tu, tl


def box_root(w0, w, bl, bu, wt0=1.0, wt=None):
    """the exact minimiser t >= 0 of wt0 (t - w0)^2 + sum wt_j dist(w_j, [t bl_j, t bu_j])^2: the root of its piecewise-linear,
    nondecreasing gradient, by bisection and then Newton steps inside the bracket, in long double"""
    L = np.longdouble
    w, bl, bu = np.asarray(w, dtype=L), np.asarray(bl, dtype=L), np.asarray(bu, dtype=L)
    wt = np.ones(len(w), dtype=L) if wt is None else np.asarray(wt, dtype=L)
    w0, wt0 = L(w0), L(wt0)

    def gh(t):
        hi, lo, tu, tl = _active(w, t, bl, bu)
        g = wt0 * (t - w0) + np.sum(wt[hi] * (tu[hi] - w[hi]) * bu[hi]) + np.sum(wt[lo] * (tl[lo] - w[lo]) * bl[lo])
        h = wt0 + np.sum(wt[hi] * bu[hi] * bu[hi]) + np.sum(wt[lo] * bl[lo] * bl[lo])
        return g, h

    if gh(L(0))[0] >= 0:
        return L(0)
    # a bracket from bisection in double precision (cheap), widened until long double confirms it
    wd, bld, bud, wtd = (v.astype(np.float64) for v in (w, bl, bu, wt))

    def g64(t):
        hi, lo, tu, tl = _active(wd, t, bld, bud)
        return float(wt0) * (t - float(w0)) + np.sum(wtd[hi] * (tu[hi] - wd[hi]) * bud[hi]) + np.sum(wtd[lo] * (tl[lo] - wd[lo]) * bld[lo])

    a, b = 0.0, max(1.0, float(w0))
    while g64(b) < 0:
        b *= 2.0
    for _ in range(44):
        mid = 0.5 * (a + b)
        a, b = (mid, b) if g64(mid) < 0 else (a, mid)
    pad = L(4.0 * (b - a)) + L(b) * L(1e-15)
    a, b = max(L(0), L(a) - pad), L(b) + pad
    while a > 0 and gh(a)[0] > 0:
        pad *= 4
        a = max(L(0), a - pad)
    while gh(b)[0] < 0:
        pad *= 4
        b = b + pad
    t = (a + b) / 2
    for _ in range(80):  # Newton is exact on the linear piece that holds the root; bisection where it leaves the bracket
        g, h = gh(t)
        if g == 0:
            break
        a, b = (t, b) if g < 0 else (a, t)
        tn = t - g / h
        if not (a <= tn <= b):
            tn = (a + b) / 2
        if tn == t:
            break
        t = tn
    return t


def box_dual_expected(x, bl, bu, r=None):
    """y = x + Proj_K(-x) for the rows [t; s] of a box cone with the bounds as used (box_effective_bounds); r: the metric, y =
    Proj^{1/r}_K(-r x) / r + x as the entries apply it.  Returns (y, t)."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 1:
        t = max(-x[0] * (1.0 if r is None else r[0]), 0.0)
        return np.array([t / (1.0 if r is None else r[0]) + x[0]]), t
    w = -x if r is None else x * (-np.asarray(r, dtype=np.float64))
    L = np.longdouble
    t = float(box_root(w[0], w[1:], bl, bu, 1.0 if r is None else L(1) / L(r[0]), None if r is None else L(1) / np.asarray(r[1:], dtype=L)))
    p = w.copy()
    hi, lo, tu, tl = _active(w[1:], t, bl, bu)
    p[0] = t
    p[1:][hi] = tu[hi]
    p[1:][lo] = tl[lo]
    return (p + x if r is None else p / r + x), t


BOX_KINDS = ("zero", "clamp", "inside", "zero_bounds", "all_infinite", "mixed", "all_active")


def box_bounds(nb, kind, rng):
    """(bl, bu, D) as handed to the cone"""
    bu, bl = rng.uniform(0.1, 2.0, nb), -rng.uniform(0.1, 2.0, nb)
    D = None
    if kind == "zero_bounds":
        bu[::3], bl[::3] = 0.0, 0.0
        bu[1::7] = 0.0  # one-sided: [t bl, 0]
    elif kind == "all_infinite":
        bu[:], bl[:] = 1e20, -1e20
        D = rng.uniform(0.5, 2.0, nb + 1)
    elif kind == "mixed":
        bu[::7], bl[::11] = 1e20, -1e20
        bu[2::13], bl[2::13] = 0.0, 0.0
        bl[3::17] = 0.0
        D = rng.uniform(0.5, 2.0, nb + 1)
    elif kind == "all_active":  # narrow bounds: at the root every row is clamped, so every row enters the gradient
        bu, bl = bu * 1e-3, bl * 1e-3
    return bl, bu, D


def box_case(nb, kind, seed=0, t0=None, row_scale=1.0, xseed=0):
    """one box cone of nb bounded rows.  t0: the head of the vector that is projected onto K, i.e. -x[0].  The bounds depend on
    (seed, nb, kind) only, the vector on xseed too: cases that differ in xseed share a cone."""
    bl, bu, D = box_bounds(nb, kind, np.random.default_rng([seed, nb, BOX_KINDS.index(kind)]))
    rng = np.random.default_rng([seed, nb, BOX_KINDS.index(kind), xseed])
    ebl, ebu = box_effective_bounds(bl, bu, D)
    w = np.empty(nb + 1)
    w[1:] = rng.standard_normal(nb) * 2.0 * row_scale
    w[0] = {"zero": 0.0, "clamp": -1e6, "inside": 3.0}.get(kind, 0.7)
    if kind == "zero":
        w[:] = 0.0
    elif kind == "inside":
        w[1:] = 3.0 * 0.9 * np.where(w[1:] > 0, ebu, ebl) * rng.uniform(0.0, 1.0, nb)
    elif kind == "all_active":
        w[1:] = np.where(rng.uniform(size=nb) < 0.5, -1.0, 1.0) * (2.0 + np.abs(rng.standard_normal(nb)))
    if t0 is not None:
        w[0] = t0
    x = -w
    cone = dict(bu=bu, bl=bl) if nb else dict(bsize=1)
    e, t = box_dual_expected(x, ebl, ebu)
    return _case(cone, x, e, np.full(nb + 1, max(1.0, t)), np.full(nb + 1, kind == "zero"), [Part(f"box {kind} nb {nb}", 0, nb + 1)], D)


BOX_SEQUENCE_T0 = (1e3, 1e-3, -5.0, 1e3, 0.0, 2.0, 1e-9, 50.0)
BOX_SEQUENCE_ROW_SCALE = (1.0, 1.0, 1.0, 100.0, 1e-6, 0.0, 1e3, 1e3)


def box_sequence(nb, seed=0):
    """(cone, D, effective bounds, [x_0 .. x_7]) for one workspace: every Newton iteration starts from a far t_warm"""
    rng = np.random.default_rng([seed, nb, 77])
    bl, bu, D = box_bounds(nb, "mixed", rng)
    ebl, ebu = box_effective_bounds(bl, bu, D)
    xs = []
    for t0, rs in zip(BOX_SEQUENCE_T0, BOX_SEQUENCE_ROW_SCALE):
        w = np.concatenate([[t0], rng.standard_normal(nb) * 2.0 * rs])
        xs.append(-w)
    return dict(bu=bu, bl=bl), D, (ebl, ebu), xs

