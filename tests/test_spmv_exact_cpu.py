"""The generators and checks of tests/spmv_exact.py on their own (no GPU): the exact-check data stays within each precision's exact range
for every order, check (a) rejects a product with one entry dropped or moved to the next row, and check (b) accepts scipy's fp64
product and rejects one accumulated in fp32."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import spmv_exact as sx

SMALL = ["1x1", "m1", "n1", "empty", "longrows", "dense", "mod4", "random"]
P_NAMES = ["none", "diag", "zero_diag", "dense_col", "dup_diag"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", SMALL)
def test_integer_data_is_exact_in_every_order(name, dtype):
    A_pat = sx.shape(name)
    n = A_pat.shape[1]
    for pn in P_NAMES:
        ops, x, y = sx.exact_problem(A_pat, sx.p_pattern(pn, n), np.random.default_rng(3), dtype)  # asserts the magnitude bound
        ax, aty, mv = ops.exact(x, y)
        rng = np.random.default_rng(4)
        # A' y summed in `dtype` in a random order per row (and in the reverse order) equals the exact value
        it, jt, vt = ops.at
        prod = (vt * y[jt]).astype(dtype)
        for perm in (rng.permutation(len(prod)), np.arange(len(prod))[::-1]):
            rows = np.repeat(np.arange(ops.n), np.diff(it))[perm]
            acc = np.zeros(ops.n, dtype)
            np.add.at(acc, rows, prod[perm])
            assert np.array_equal(acc.astype(np.float64), aty)
        # the exact references agree with a plain float64 product (the data are small enough for that too)
        assert np.array_equal(ax, ops.A @ x)
        Pf = sx.expand_p(ops.P, n)
        assert np.array_equal(mv, ops.diag_r[:n] * x + Pf @ x + ops.A.T @ ((ops.A @ x) / ops.diag_r[n:]))


def test_generator_refuses_data_beyond_the_exact_range():
    A_pat = sp.csc_matrix(np.ones((4, 40000)))  # rows of 40000 entries of up to 100 x 100: 2^28.6
    with pytest.raises(AssertionError, match="bits"):
        sx.exact_problem(A_pat, None, np.random.default_rng(0), np.float32, amp=(100, 100, 1))


def test_expand_p_sums_duplicate_diagonal_entries():
    P = sx.p_pattern("dup_diag", 6)
    P.data = np.arange(1.0, P.nnz + 1)
    F = sx.expand_p(P, 6).toarray()
    D = P.toarray()  # scipy sums the duplicates
    assert np.array_equal(F, D + D.T - np.diag(np.diag(D)))
    assert P.nnz == 8 and F[0, 0] == D[0, 0]


def _ops(name, dtype=np.float64):
    return sx.exact_problem(sx.shape(name), None, np.random.default_rng(1), dtype)


@pytest.mark.parametrize("name", ["empty", "longrows", "random"])
def test_exact_check_catches_a_dropped_or_moved_entry(name):
    ops, x, y = _ops(name)
    ax = ops.exact(x, y)[0]
    sx.check_exact(ops.A @ x, ax, np.float64, "A x")
    ia, ja, va = ops.a
    contrib = va * x[ja]
    k = int(np.flatnonzero(contrib != 0)[len(va) // 3 % np.count_nonzero(contrib)])  # an entry that changes its row's sum
    r = int(np.searchsorted(ia, k, side="right") - 1)
    dropped = ax.copy()
    dropped[r] -= va[k] * x[ja[k]]
    moved = dropped.copy()
    moved[(r + 1) % ops.m] += va[k] * x[ja[k]]
    for bad in (dropped, moved):
        with pytest.raises(AssertionError, match="differ from the exact product"):
            sx.check_exact(bad, ax, np.float64, "A x")


def test_exact_check_catches_a_row_left_unwritten():
    ops, x, y = _ops("empty")
    ax = ops.exact(x, y)[0]
    got = ax.copy()
    got[0] = np.nan  # an empty row (exact result 0) never written over the NaN fill
    with pytest.raises(AssertionError):
        sx.check_exact(got, ax, np.float64, "A x")


@pytest.mark.parametrize("name", ["longrows", "dense", "random"])
def test_bound_accepts_scipy_fp64_and_rejects_fp32_accumulation(name):
    A_pat = sx.shape(name)
    ops, x, y = sx.real_problem(A_pat, sx.p_pattern("dense_col", A_pat.shape[1]), np.random.default_rng(2))
    ax, aty, mv = ops.longdouble(x, y)
    b_a, b_at, b_mv = ops.bounds(x, y, sx.UNIT_ROUNDOFF[np.float64])
    sx.check_bound(ops.A @ x, ax, b_a, "A x")
    sx.check_bound(ops.A.T @ y, aty, b_at, "A' y")
    Pf = sx.expand_p(ops.P, ops.n)
    sx.check_bound(ops.diag_r[:ops.n] * x + Pf @ x + ops.A.T @ ((ops.A @ x) / ops.diag_r[ops.n:]), mv, b_mv, "mat_vec")
    # the same product with fp64 loads but an fp32 accumulator
    ia, ja, va = ops.a
    acc32 = np.zeros(ops.m, np.float32)
    for r in range(ops.m):
        for k in range(ia[r], ia[r + 1]):
            acc32[r] = np.float32(acc32[r] + va[k] * x[ja[k]])
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        sx.check_bound(acc32.astype(np.float64), ax, b_a, "A x")


def test_bound_is_exact_on_empty_rows():
    ops, x, y = sx.real_problem(sx.shape("empty"), None, np.random.default_rng(2))
    ax = ops.longdouble(x, y)[0]
    b_a = ops.bounds(x, y, sx.UNIT_ROUNDOFF[np.float64])[0]
    got = ops.A @ x
    got[0] = 1e-300  # row 0 is empty: its bound is 0
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        sx.check_bound(got, ax, b_a, "A x")


def test_lines_counted_edges_follow_the_header_formula():
    last, first = sx.lines_counted_edge(8)
    assert (last, first) == ((1 << 23) + 127, (1 << 23) + 128)
    assert sx.lines_counted(last, 8) and not sx.lines_counted(first, 8)
    last, first = sx.lines_counted_edge(4)
    assert (last, first) == ((1 << 24) + 255, (1 << 24) + 256)


@pytest.mark.parametrize("m", [(1 << 22) + 1, (1 << 23) + 128])
def test_tall_pattern_reaches_the_row_cap_and_both_ends(m):
    A = sx.tall_pattern(m)
    assert A.shape == (m, 4096)
    cnt = np.diff(A.indptr)
    assert (cnt[:2048] == 1).all() and A.indices[0] == 0 and A.indices[A.indptr[2047]] == m - 1
    assert A.indices.max() == m - 1 and A.indices.min() == 0
