"""Blocks of right-hand sides on the B1 path, one GPU: what K interleaved vectors cost against K single-vector calls.

On the headline shape (n x 2n, 10 entries per column, the generator of scripts/bench_linsys.py) and for every K of --ks:
  (i)  the block product scs_amd_linsys_mat_vec_multi_dev alone, --calls calls between two device synchronisations after a warm-up,
       against scs_amd_linsys_mat_vec_dev on the same workspace in the same process, the two alternated --reps times;
  (ii) one block solve of K random columns at --tol against K successive scs_solve_lin_sys calls on the same columns.
One JSON line per K: time per block product, time per column, its ratio to the single-vector product of the SAME run, the spread
over the repeats, the algorithmic bytes of a block product (the entries of both orientations once, the vector traffic times K) and
the share of the HBM peak that gives, and the per-column PCG iteration counts of both paths.  No pass mark: it reports.

--per-column-r: what it costs to give every column its own diag_r (scs_amd_linsys_mat_vec_multi_r_dev,
scs_amd_solve_lin_sys_multi_r) against the shared-R block of the SAME run, the two alternated --reps times: the block product, the
block solve (every column's R equal to the workspace's diag_r, so that both solves run the same iterations), and the one-off work
of a per-column call -- upload and transposition of DR and the preconditioner pass -- as the difference of the two solve entries
on an all-zero block (every column short-circuits: no iteration runs).  One JSON line per K; no pass mark here either."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


class Hip:
    """device buffers through the HIP runtime the library already links"""

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
        assert self.rt.hipMemcpy(dptr, arr.ctypes.data, arr.nbytes, 1) == 0

    def free(self, dptr):
        assert self.rt.hipFree(dptr) == 0

    def sync(self):
        assert self.rt.hipDeviceSynchronize() == 0


def block_bytes(n, m, nnz, K, sf):
    """algorithmic bytes of one block mat_vec: entries (value + 32-bit index) and row pointers of A and A' once; per column the
    gathered vectors (n and m), tmp written and read (m), R_x x read (n) and the result written (n); R_x, R_y once"""
    matrix = 2 * nnz * (sf + 4) + (n + 1 + m + 1) * 4
    return matrix + (n + m) * sf + K * (3 * n + 2 * m) * sf


def timed(fn, calls, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--lib", default="libscsamd_linsys.so")
    ap.add_argument("--per-column-r", action="store_true", help="per-column diag_r against the shared-R block of the same run")
    a = ap.parse_args()
    n, m = a.n, a.m or 2 * a.n
    lib = capi.load(a.lib)
    if lib.scs_amd_device_count() <= 0:
        sys.exit("bench_linsys_multi: no GPU (a measurement path does not fall back)")
    T = lib._scs_types
    sf = np.dtype(T.np_float).itemsize
    rng = np.random.default_rng(0)
    t0 = time.time()
    rows = problems.random_rows(m, n, a.col_nnz, rng)
    vals = rng.uniform(-1, 1, size=(n, a.col_nnz)).astype(T.np_float)
    import scipy.sparse as sp
    A = sp.csc_matrix((vals.ravel(), rows.ravel().astype(np.int32),
                       np.arange(0, (n + 1) * a.col_nnz, a.col_nnz, dtype=np.int32)), shape=(m, n))
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), T=T)
    dr = np.empty(n + m, dtype=T.np_float)
    dr[:n] = 1e-6
    dr[n:n + m // 10] = 1.0 / 100.0
    dr[n + m // 10:] = 10.0
    print(f"gen {time.time() - t0:.1f}s n={n} m={m} nnz={A.nnz}", file=sys.stderr, flush=True)
    w = lib.scs_init_lin_sys_work(C.byref(prob.matA), None, dr.ctypes.data_as(T.fp))
    assert w
    hip = Hip()
    sync = lambda: (hip.sync(), lib.scs_amd_linsys_sync(w))
    x1 = hip.malloc(n * sf)
    y1 = hip.malloc(n * sf)
    hip.put(x1, rng.uniform(-1, 1, n).astype(T.np_float))
    single_fn = lambda: lib.scs_amd_linsys_mat_vec_dev(w, x1, y1)
    st = T.ScsAmdStats()

    def its_of(fn):
        lib.scs_amd_linsys_get_stats(w, C.byref(st))
        before = st.cg_iters
        fn()
        lib.scs_amd_linsys_get_stats(w, C.byref(st))
        return st.cg_iters - before

    med = lambda v: float(np.median(v))
    spread = lambda v: round((max(v) - min(v)) / med(v), 4)
    for K in [int(v) for v in a.ks.split(",")] if a.per_column_r else []:
        W = max(2, lib.scs_amd_linsys_multi_width(K))
        xb, yb, rb = hip.malloc(n * W * sf), hip.malloc(n * W * sf), hip.malloc((n + m) * W * sf)
        hip.put(xb, rng.uniform(-1, 1, n * W).astype(T.np_float))
        R = np.ones((n + m, W), dtype=T.np_float)  # padding columns 1
        R[:, :K] = dr[:, None] * rng.uniform(0.5, 2.0, K).astype(T.np_float)[None, :]
        hip.put(rb, R)
        percol_fn = lambda: lib.scs_amd_linsys_mat_vec_multi_r_dev(w, K, rb, xb, yb)
        shared_fn = (lambda: lib.scs_amd_linsys_mat_vec_multi_dev(w, K, xb, yb)) if K > 1 else single_fn
        assert percol_fn() == 0 and shared_fn() == 0
        for _ in range(20):
            percol_fn()
            shared_fn()
        tp, tsh = [], []
        for _ in range(a.reps):  # alternated
            tp.append(timed(percol_fn, a.calls, sync))
            tsh.append(timed(shared_fn, a.calls, sync))
        for d in (xb, yb, rb):
            hip.free(d)
        rec = dict(mode="per_column_r", K=K, width=W, n=n, m=m, nnz=int(A.nnz), calls=a.calls, reps=a.reps,
                   percol_product_us=round(1e6 * med(tp), 2), shared_product_us=round(1e6 * med(tsh), 2),
                   percol_over_shared=round(med(tp) / med(tsh), 4), percol_spread=spread(tp), shared_spread=spread(tsh),
                   extra_MB_read=round((n + m) * (W - 1) * sf / 1e6, 1))
        if not a.no_solve and K > 1:
            B = np.asfortranarray(rng.uniform(-1, 1, (n + m, K)).astype(T.np_float))
            DR = np.asfortranarray(np.tile(dr[:, None], (1, K)))
            fp = lambda v: v.ctypes.data_as(T.fp)
            it_p, it_s = np.zeros(K, dtype=T.np_int), np.zeros(K, dtype=T.np_int)

            def solve(percol, rhs, tolv, it):
                out = rhs.copy(order="F")
                tv = np.full(K, tolv, dtype=T.np_float)
                t0 = time.perf_counter()
                if percol:
                    rc = lib.scs_amd_solve_lin_sys_multi_r(w, K, fp(DR), n + m, fp(out), n + m, None, 0, fp(tv), it.ctypes.data_as(T.ip))
                else:
                    rc = lib.scs_amd_solve_lin_sys_multi(w, K, fp(out), n + m, None, 0, fp(tv), it.ctypes.data_as(T.ip))
                dt = time.perf_counter() - t0
                assert rc == 0
                return dt, out

            solve(True, B, 0.5, it_p)  # allocate the buffers of both paths outside the timed solves
            solve(False, B, 0.5, it_s)
            sp_, ss_, zp, zs = [], [], [], []
            Z = np.zeros_like(B)
            for _ in range(a.reps):  # alternated
                dt, out_p = solve(True, B, a.tol, it_p)
                sp_.append(dt)
                dt, out_s = solve(False, B, a.tol, it_s)
                ss_.append(dt)
                zp.append(solve(True, Z, a.tol, np.zeros(K, dtype=T.np_int))[0])
                zs.append(solve(False, Z, a.tol, np.zeros(K, dtype=T.np_int))[0])
            rec.update(solve_percol_s=round(med(sp_), 4), solve_shared_s=round(med(ss_), 4), solve_percol_over_shared=round(med(sp_) / med(ss_), 4),
                       solve_percol_spread=spread(sp_), solve_shared_spread=spread(ss_), iters_percol=[int(v) for v in it_p],
                       iters_shared=[int(v) for v in it_s], same_bits=bool(np.array_equal(out_p, out_s)),
                       zero_block_percol_ms=round(1e3 * med(zp), 3), zero_block_shared_ms=round(1e3 * med(zs), 3),
                       r_setup_ms=round(1e3 * (med(zp) - med(zs)), 3))
        print(json.dumps(rec), flush=True)
    for K in [int(v) for v in a.ks.split(",")] if not a.per_column_r else []:
        W = lib.scs_amd_linsys_multi_width(K)
        xb = hip.malloc(n * W * sf)
        yb = hip.malloc(n * W * sf)
        hip.put(xb, rng.uniform(-1, 1, n * W).astype(T.np_float))
        block_fn = lambda: lib.scs_amd_linsys_mat_vec_multi_dev(w, K, xb, yb)
        assert block_fn() == 0 and single_fn() == 0
        for _ in range(20):  # warm-up of both
            block_fn()
            single_fn()
        tb, ts = [], []
        for _ in range(a.reps):  # alternated
            tb.append(timed(block_fn, a.calls, sync))
            ts.append(timed(single_fn, a.calls, sync))
        hip.free(xb)
        hip.free(yb)
        tb_med, ts_med = float(np.median(tb)), float(np.median(ts))
        bts = block_bytes(n, m, A.nnz, K, sf)
        rec = dict(K=K, width=W, n=n, m=m, nnz=int(A.nnz), calls=a.calls, reps=a.reps,
                   block_product_us=round(1e6 * tb_med, 2), per_column_us=round(1e6 * tb_med / K, 2),
                   single_product_us=round(1e6 * ts_med, 2), per_column_over_single=round(tb_med / K / ts_med, 4),
                   block_spread=round((max(tb) - min(tb)) / tb_med, 4), single_spread=round((max(ts) - min(ts)) / ts_med, 4),
                   block_product_MB=round(bts / 1e6, 1), share_of_8TBps=round(bts / tb_med / HBM_PEAK, 4))
        if not a.no_solve:
            B = np.asfortranarray(rng.uniform(-1, 1, (n + m, K)).astype(T.np_float))
            out = B.copy(order="F")
            tol = np.full(K, a.tol, dtype=T.np_float)
            iters = np.zeros(K, dtype=T.np_int)
            warm = B.copy(order="F")  # allocates the block buffers of this width outside the timed solve
            assert lib.scs_amd_solve_lin_sys_multi(w, K, warm.ctypes.data_as(T.fp), n + m, None, 0,
                                                   np.full(K, 0.5, dtype=T.np_float).ctypes.data_as(T.fp), None) == 0
            t0 = time.perf_counter()
            rc = lib.scs_amd_solve_lin_sys_multi(w, K, out.ctypes.data_as(T.fp), n + m, None, 0, tol.ctypes.data_as(T.fp),
                                                 iters.ctypes.data_as(T.ip))
            t_block = time.perf_counter() - t0
            assert rc == 0
            single_its, worst = [], 0.0
            t_single = 0.0
            for k in range(K):
                b = np.ascontiguousarray(B[:, k])
                t0 = time.perf_counter()
                single_its.append(int(its_of(lambda: lib.scs_solve_lin_sys(w, b.ctypes.data_as(T.fp), None, a.tol))))
                t_single += time.perf_counter() - t0
                worst = max(worst, float(np.abs(b - out[:, k]).max() / np.abs(b).max()))
            rec.update(solve_block_s=round(t_block, 4), solve_singles_s=round(t_single, 4), solve_ratio=round(t_block / t_single, 4),
                       iters_block=[int(v) for v in iters], iters_single=single_its, solution_rel_diff=float(f"{worst:.3e}"))
        print(json.dumps(rec), flush=True)
    hip.free(x1)
    hip.free(y1)
    lib.scs_free_lin_sys_work(w)


if __name__ == "__main__":
    main()
