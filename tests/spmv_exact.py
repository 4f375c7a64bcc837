"""Exact and rounding-bounded references for the CSR products of the linear-system workspace (numpy only, no GPU).

The operators (include/scs_amd.h, scs_amd_linsys_*_dev):
    mul_a    y(m) = A x
    mul_at   x(n) = A' y
    mat_vec  y(n) = R_x x + P x + A' (R_y^-1 A x)      P = the stored upper triangle expanded to the full symmetric matrix,
                                                       duplicate diagonal entries summed (reference linsys/cpu/indirect/private.c:69-75)

Check (a), exact: A, P and x hold small integers and R_x, R_y powers of two.  Every partial sum of every summation order is then an
integer multiple of 2^-K whose magnitude stays below 2^(p - K) (p = 53 for fp64, 24 for fp32): each one is representable, so every
order gives the exact result and a kernel must equal the integer reference bit for bit.  `exact_problem` asserts that bound.

Check (b), rounding: with real data a row of k terms obeys |y_r - y*_r| <= gamma_k (|A||x|)_r, gamma_k = k u / (1 - k u) (Higham, Accuracy
and Stability of Numerical Algorithms, 2nd ed., eq. 3.5); `C_ROUND` = 2 covers the 1 / (1 - k u) and the epilogue operations (one division
by R_y, one product R_x x, one addition of P x), each counted as a term below.  The reference is evaluated in np.longdouble."""
import numpy as np
import scipy.sparse as sp

C_ROUND = 2.0  # the one constant of every rounding bound below
PREC_BITS = {np.float64: 53, np.float32: 24}
UNIT_ROUNDOFF = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
LD = np.longdouble


def csr_arrays(M):
    """(indptr, indices, data) of M in CSR, duplicates kept, columns in stored order per row"""
    M = sp.csr_matrix(M) if not sp.isspmatrix_csr(M) else M
    return M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data


def row_products(indptr, indices, data, x, dtype):
    """y_r = sum_k data[k] x[indices[k]] with every product and sum in `dtype` (int64: exact; longdouble: the reference of check (b)).
    Empty rows give 0."""
    rows = len(indptr) - 1
    out = np.zeros(rows, dtype=dtype)
    if len(data) == 0:
        return out
    prod = data.astype(dtype) * np.asarray(x)[indices].astype(dtype)
    nonempty = np.flatnonzero(np.diff(indptr) > 0)
    out[nonempty] = np.add.reduceat(prod, indptr[:-1][nonempty])
    return out


def expand_p(P, n):
    """the full symmetric matrix the library multiplies by (linsys.hip, LinSys::init): every stored (i, j) of the upper triangle, and
    (j, i) for i != j; duplicates stay separate entries (they are summed by the product)"""
    if P is None:
        return sp.csr_matrix((n, n))
    C = sp.coo_matrix(P)
    off = C.row != C.col
    r = np.concatenate([C.row, C.col[off]])
    c = np.concatenate([C.col, C.row[off]])
    v = np.concatenate([C.data, C.data[off]])
    order = np.argsort(r, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return sp.csr_matrix((v[order], c[order], np.cumsum(indptr)), shape=(n, n))


class Operators:
    """A (m x n, CSC as handed to scs_init_lin_sys_work), optional upper-triangular P, diag_r = [R_x; R_y]; both orientations' CSR arrays"""

    def __init__(self, A, P, diag_r, exps=None):
        self.A = sp.csc_matrix(A)
        self.m, self.n = self.A.shape
        self.P = None if P is None else sp.csc_matrix(P)
        self.diag_r = np.asarray(diag_r)
        self.a = csr_arrays(self.A)            # rows of A
        self.at = csr_arrays(self.A.T.tocsr())  # rows of A' (= columns of A, in stored order)
        self.p = csr_arrays(expand_p(self.P, self.n))
        self.ka = np.diff(self.a[0])    # row lengths of A
        self.kat = np.diff(self.at[0])  # row lengths of A'
        self.kp = np.diff(self.p[0])
        self._exps = exps  # diag_r = 2^exps when the caller drew it so (check (a)); else derived and verified on first use

    def exps(self):
        """(e_x, e_y, K): R_x = 2^e_x, R_y = 2^e_y, and the fraction bits K of every value of the exact products"""
        if self._exps is None:
            self._exps = _pow2_exponents(self.diag_r)
        e = self._exps
        ex_x, ex_y = e[:self.n], e[self.n:]
        return ex_x, ex_y, int(max(0, ex_y.max(initial=0), -ex_x.min(initial=0)))

    def abs_products(self, x):
        """|A||x|, |A'||.|, |P||x| as functions (float64)"""
        ia, ja, va = self.a
        it, jt, vt = self.at
        ip, jp, vp = self.p
        f = np.float64
        return (lambda v: row_products(ia, ja, np.abs(va), np.abs(v), f),
                lambda v: row_products(it, jt, np.abs(vt), np.abs(v), f),
                lambda v: row_products(ip, jp, np.abs(vp), np.abs(v), f))

    # ---- exact references (check (a)): integer arithmetic on values scaled by 2^K ----
    def exact(self, x_n, y_m):
        """exact A x_n, A' y_m, mat_vec(x_n) as float64 (every value is a dyadic rational fp64 holds exactly: asserted)"""
        ia, ja, va = self.a
        it, jt, vt = self.at
        ip, jp, vp = self.p
        vi = lambda v: _as_int(v)
        ax = row_products(ia, ja, vi(va), vi(x_n), np.int64)
        aty = row_products(it, jt, vi(vt), vi(y_m), np.int64)
        ex_x, ex_y, K = self.exps()
        tmp_s = ax << (K - ex_y)                                         # 2^K (A x) / R_y, integers
        y_s = ((vi(x_n) << (K + ex_x))                                   # 2^K R_x x
               + row_products(ip, jp, vi(vp), vi(x_n), np.int64) * (2 ** K)  # 2^K P x
               + row_products(it, jt, vi(vt), tmp_s, np.int64))         # 2^K A' R_y^-1 A x
        for v in (ax, aty, y_s):
            assert np.abs(v).max(initial=0) < 2 ** 53
        return ax.astype(np.float64), aty.astype(np.float64), y_s.astype(np.float64) / 2.0 ** K

    def exact_bits_needed(self, x_n, y_m):
        """max over every product of log2 of (largest partial-sum magnitude x 2^K): the exponent range check (a) needs"""
        absA, absAt, absP = self.abs_products(x_n)
        ex_x, ex_y, K = self.exps()
        b_ax = absA(x_n)
        b_aty = absAt(y_m)
        b_tmp = np.ldexp(b_ax, K - ex_y)                                   # |tmp| 2^K
        b_mv = absP(x_n) * 2.0 ** K + absAt(b_tmp) + np.ldexp(np.abs(x_n), K + ex_x)
        worst = max(b_ax.max(initial=0), b_aty.max(initial=0), b_tmp.max(initial=0), b_mv.max(initial=0), 1.0)
        return float(np.log2(worst)), K

    # ---- long-double references and rounding bounds (check (b)) ----
    def longdouble(self, x_n, y_m):
        ia, ja, va = self.a
        it, jt, vt = self.at
        ip, jp, vp = self.p
        ax = row_products(ia, ja, va, x_n, LD)
        aty = row_products(it, jt, vt, y_m, LD)
        tmp = ax / self.diag_r[self.n:].astype(LD)
        mv = (self.diag_r[:self.n].astype(LD) * x_n.astype(LD) + row_products(ip, jp, vp, x_n, LD)
              + row_products(it, jt, vt, tmp, LD))
        return ax, aty, mv

    def bounds(self, x_n, y_m, u):
        """per-row rounding bounds of mul_a, mul_at, mat_vec: C_ROUND u k_r (|op| |input|)_r, composed for mat_vec:
        tmp_i = (A x)_i / R_y,i carries (k_A,i + 1) roundings of (|R_y^-1||A||x|)_i; row j of the result sums k_A',j + 2 terms (P x, the
        products, R_x x) on top of P x's own k_P,j"""
        absA, absAt, absP = self.abs_products(x_n)
        b_a = C_ROUND * u * np.maximum(self.ka, 1) * absA(x_n)
        b_at = C_ROUND * u * np.maximum(self.kat, 1) * absAt(y_m)
        abs_tmp = absA(x_n) / np.abs(self.diag_r[self.n:])
        b1 = absP(x_n) + np.abs(self.diag_r[:self.n] * x_n)
        b2 = absAt(abs_tmp)
        b3 = absAt((self.ka + 1) * abs_tmp)
        b_mv = C_ROUND * u * ((self.kat + self.kp + 2) * (b1 + b2) + b3)
        return b_a, b_at, b_mv


def _as_int(v):
    iv = np.asarray(v).astype(np.int64)
    assert np.array_equal(iv, v), "exact check needs integer-valued data"
    return iv


def _pow2_exponents(d):
    e = np.log2(np.asarray(d, dtype=np.float64)).round().astype(np.int64)
    assert np.array_equal(2.0 ** e, d), "exact check needs powers of two in diag_r"
    return e


# ---- data generators ----
def int_values(k, rng, lo, hi):
    """nonzero integers in +-[lo, hi]"""
    return (rng.integers(lo, hi + 1, k, dtype=np.int8) * rng.choice(np.array([-1, 1], np.int8), k)).astype(np.float64)


def exact_problem(A_pat, P_pat, rng, dtype, amp=None):
    """check (a) data on the given patterns: integer A, P, x, y and power-of-two diag_r.  Asserts that every partial sum of every
    order fits the precision's exact range, so the case cannot go vacuous (an inexact reference would make a bit-for-bit test a
    rounding lottery instead).  Returns (Operators, x_n, y_m)."""
    a_hi, x_hi, e = amp or ((7, 7, 2) if dtype is np.float64 else (3, 3, 1))
    m, n = A_pat.shape
    A = sp.csc_matrix(A_pat, dtype=np.float64, copy=True)
    A.data = int_values(A.nnz, rng, 1, a_hi)
    P = None
    if P_pat is not None:
        P = sp.csc_matrix(P_pat, dtype=np.float64, copy=True)
        P.data = np.where(P.data == 0, 0.0, int_values(P.nnz, rng, 1, a_hi))  # an explicit stored zero stays zero
    exps = rng.integers(-e, e + 1, n + m, dtype=np.int8).astype(np.int64)
    x = int_values(n, rng, 1, x_hi)  # no zeros: every stored entry contributes to its row
    y = int_values(m, rng, 1, x_hi)
    ops = Operators(A, P, np.ldexp(1.0, exps), exps)
    bits, K = ops.exact_bits_needed(x, y)
    assert bits < PREC_BITS[dtype], f"exact-check data needs {bits:.1f} bits (K = {K}), {dtype.__name__} holds {PREC_BITS[dtype]}"
    return ops, x, y


def real_problem(A_pat, P_pat, rng):
    """check (b) data: values of mixed signs with magnitudes spread log-uniformly over 1e-8 .. 1e8; diag_r positive, 1e-2 .. 1e2"""
    m, n = A_pat.shape
    spread = lambda k: rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-8, 8, k)
    A = sp.csc_matrix(A_pat, dtype=np.float64, copy=True)
    A.data = spread(A.nnz)
    P = None
    if P_pat is not None:
        P = sp.csc_matrix(P_pat, dtype=np.float64, copy=True)
        P.data = np.where(P.data == 0, 0.0, spread(P.nnz))
    diag_r = 10.0 ** rng.uniform(-2, 2, n + m)
    return Operators(A, P, diag_r), spread(n), spread(m)


def cast(ops, x, y, dtype):
    """the same operators and vectors rounded to the library's precision (the reference must see what the kernel sees)"""
    c = lambda M: None if M is None else sp.csc_matrix((M.data.astype(dtype).astype(np.float64), M.indices, M.indptr), shape=M.shape)
    return (Operators(c(ops.A), c(ops.P), ops.diag_r.astype(dtype).astype(np.float64)),
            x.astype(dtype).astype(np.float64), y.astype(dtype).astype(np.float64))


# ---- checks ----
def check_exact(got, ref, dtype, what):
    """check (a): bit for bit (the reference is exactly representable in `dtype`: asserted)"""
    ref_t = ref.astype(dtype)
    assert np.array_equal(ref_t.astype(np.float64), ref), f"{what}: the exact result does not fit {dtype.__name__}"
    got = np.asarray(got, dtype=dtype)
    bad = np.flatnonzero(got.view(np.uint64 if dtype is np.float64 else np.uint32) != ref_t.view(np.uint64 if dtype is np.float64 else np.uint32))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(ref)} rows differ from the exact product, first rows {bad[:5].tolist()}: "
                           f"got {got[bad[:5]].tolist()} want {ref_t[bad[:5]].tolist()}")


def check_bound(got, ref_ld, bound, what):
    """check (b): |got - ref| <= bound row by row (ref in long double); rows whose bound is 0 must be exact"""
    assert np.finfo(LD).nmant >= 63, "the rounding reference needs an 80-bit long double"
    err = np.abs(np.asarray(got).astype(LD) - ref_ld)
    bad = np.flatnonzero(~(err <= bound.astype(LD)))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(bound)} rows outside the rounding bound, first rows {bad[:5].tolist()}: "
                           f"error {[float(e) for e in err[bad[:5]]]} bound {bound[bad[:5]].tolist()}")


# ---- shapes: (m x n pattern with every value 1, note) ----
def _from_rows(m, n, rows):
    """CSC pattern from {row: column array}"""
    r = np.concatenate([np.full(len(c), i, dtype=np.int64) for i, c in rows.items()] or [np.zeros(0, np.int64)])
    c = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows.values()] or [np.zeros(0, np.int64)])
    M = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(m, n)).tocsc()
    M.sum_duplicates()
    M.data[:] = 1.0
    return M


def _random_pattern(m, n, density_per_col, rng, rows_ok=None, cols_ok=None):
    rows_ok = np.arange(m) if rows_ok is None else rows_ok
    cols_ok = np.arange(n) if cols_ok is None else cols_ok
    k = int(density_per_col * len(cols_ok))
    r = rng.choice(rows_ok, k)
    c = rng.choice(cols_ok, k)
    M = sp.coo_matrix((np.ones(k), (r, c)), shape=(m, n)).tocsc()
    M.sum_duplicates()
    M.data[:] = 1.0
    return M


def shape(name, seed=0):
    """the test shapes; each is built for one edge of the kernels or their planners (spmv.h, spmv_wave.h, spmv_wave_build.h)"""
    rng = np.random.default_rng(seed)
    if name == "1x1":  # one entry: one row-block, one unit of one row, a chunk of one valid entry
        return sp.csc_matrix(np.ones((1, 1)))
    if name == "m1":  # one dense row (m = 1): A' has 300 one-entry rows, A one row of 300
        return sp.csc_matrix(np.ones((1, 300)))
    if name == "n1":  # one dense column (n = 1)
        return sp.csc_matrix(np.ones((300, 1)))
    if name == "empty":
        # empty rows: the first, the last and a run of 2600 > ROWS_PER_BLOCK_MAX = 2048 (a row-block of empty rows; with rows of A of
        # ~1.4 entries a unit reaches its 1024-row cap inside the run: a whole wave unit of empty rows); empty columns likewise (the first,
        # the last and a run of 2300), so that A' has empty rows too
        m, n = 7000, 5000
        rows_ok = np.setdiff1d(np.arange(1, m - 1), np.arange(1000, 3600))
        cols_ok = np.setdiff1d(np.arange(1, n - 1), np.arange(2000, 4300))
        return _random_pattern(m, n, 5, rng, rows_ok, cols_ok)
    if name == "longrows":
        # rows of exactly 2047, 2048 and 2049 entries: the last short-row block and the first long-row block of csr_stream
        # (NNZ_PER_BLOCK = 2048); the 2049-entry row has empty rows directly before and after it.  Columns 20, 22, 24 likewise, so that
        # A' has the same rows (the long-row path under the GP epilogue of mat_vec, whose sum starts at P x); the rest a few entries
        m = n = 3000
        rows_free = np.setdiff1d(np.arange(m), [2, 4, 5, 6, 7])
        cols_free = np.setdiff1d(np.arange(n), [20, 22, 23, 24, 25])
        M = _random_pattern(m, n, 1, rng, rows_free[rows_free > 10], cols_free[cols_free > 30]).tolil()
        for i, k in ((2, 2047), (4, 2048), (6, 2049)):
            M[i, rng.choice(cols_free, k, replace=False)] = 1.0
        for j, k in ((20, 2047), (22, 2048), (24, 2049)):
            M[rng.choice(rows_free, k, replace=False), j] = 1.0
        return sp.csc_matrix(M)
    if name == "dense":
        # a dense row of n entries and a dense column of m = 9000 > WR_DEV_UNIT_MAX = 8192 entries: A' gets a row longer than the wave
        # budget and than the device builder's in-LDS sort (that unit goes to the host builder)
        m, n = 9000, 3000
        M = _random_pattern(m, n, 3, rng).tolil()
        M[17, :] = 1.0
        M[:, 5] = 1.0
        return sp.csc_matrix(M)
    if name == "mod4":
        # rows longer than the default unit budget (1024 entries) form single-row units, so each unit holds exactly one row's count:
        # counts = 1, 2, 3 (mod 4) and (mod 256) -- the masks of a unit's last 256-entry chunk and of a lane's last 4 entries, and the
        # 4-aligned start of the next unit behind the padding
        counts = [1025, 1026, 1027, 1281, 1282, 1283, 1793, 1794, 1795, 1024, 1100, 5, 6, 7, 1281]
        n = 2000
        rows = {i: rng.choice(n, c, replace=False) for i, c in enumerate(counts)}
        return _from_rows(len(counts), n, rows)
    if name == "random":
        # the general case: many row-blocks and units (grid striding of csr_stream under SPMV_MAX_GRID, several lockstep rounds under
        # WR_NNZ = 64), Poisson row lengths, duplicate-free
        return _random_pattern(20000, 8000, 8, rng)
    raise KeyError(name)


def p_pattern(name, n, seed=0):
    """upper-triangular P patterns for mat_vec (value 1 marks an entry, 0 an explicitly stored zero)"""
    rng = np.random.default_rng(seed + 1)
    if name == "none":
        return None
    if name == "diag":  # diagonal only
        return sp.identity(n, format="csc")
    if name == "zero_diag":  # an explicit zero on the diagonal (stored, value 0) among diagonal entries and a few off-diagonal ones
        D = sp.lil_matrix((n, n))
        D.setdiag(1.0)
        for j in rng.choice(n, min(n, 20), replace=False):
            if j > 0:
                D[rng.integers(0, j), j] = 1.0
        D = sp.csc_matrix(D)
        D.data[D.indptr[n // 2]:D.indptr[n // 2 + 1]][D.indices[D.indptr[n // 2]:D.indptr[n // 2 + 1]] == n // 2] = 0.0
        return D
    if name == "dense_col":  # one dense upper-triangular column (its transpose: a dense row of the expanded P)
        j = n - 1
        D = sp.lil_matrix((n, n))
        D[:, j] = 1.0
        D.setdiag(1.0)
        return sp.csc_matrix(D)
    if name == "dup_diag":  # duplicate diagonal entries in a column, summed like private.c:69-75 (the reference's validation accepts them)
        r = np.concatenate([np.arange(n), [0, n // 2]])
        c = np.concatenate([np.arange(n), [0, n // 2]])
        order = np.lexsort((r, c))
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.add.at(indptr, c + 1, 1)
        return sp.csc_matrix((np.ones(n + 2), r[order], np.cumsum(indptr)), shape=(n, n))
    raise KeyError(name)


# the gathered-vector lengths up to which the wave layout counts the distinct 128-byte lines its units gather from: the formula of
# WaveRowsDev::lines_counted (spmv_wave.h), restated; beyond, both layout builders report one line per entry
def lines_counted(cols, real_bytes):
    return ((cols >> (4 if real_bytes == 8 else 5)) // 8) <= 64 * 1024


def lines_counted_edge(real_bytes):
    """(last size counted, first size not counted), found from the formula itself"""
    lo, hi = 1, 1 << 30
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lines_counted(mid, real_bytes):
            lo = mid
        else:
            hi = mid
    return lo, hi


def tall_pattern(m, n=4096, seed=0, banded=False):
    """m x n with m at a packing edge (the gathered vector of A' is m long; A has m rows, mostly empty, in many units).
    Rows 0 .. n/2 - 1 of A' (columns of A) hold one entry each, so that a unit of A' fills its whole row cap
    (min(1024, 2^(32 - cbits))) and the top local rows reach the top bits of the packed word; the other columns hold 256 entries each,
    spread over all of [0, m) -- or, banded, 256 consecutive rows at a random offset (gathers that share lines).  Rows 0 and m - 1 of A
    are never empty (the first and the last entry of the gathered vector are read)."""
    rng = np.random.default_rng(seed)
    half = n // 2
    k = 256
    cols = [np.array([0])] + [rng.integers(0, m, 1) for _ in range(1, half - 1)] + [np.array([m - 1])]
    for j in range(half, n):
        if banded:
            s = int(rng.integers(0, m - k))
            cols.append(np.arange(s, s + k))
        else:
            cols.append(np.unique(rng.integers(0, m, k)))
    if banded:
        cols[-1] = np.arange(m - k, m)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(c) for c in cols])
    idx = np.concatenate(cols).astype(np.int64)
    return sp.csc_matrix((np.ones(len(idx)), idx, indptr), shape=(m, n))
