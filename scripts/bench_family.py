"""A family of problems in one ADMM loop, one GPU: what scs_amd_solve_family costs against K times scs_update + scs_solve.

On the headline shape (n x 2n, 10 entries per column, fp64, adaptive_scale = 0, acceleration_lookback = 0, eps 1e-4) and for every K
of --ks: a family of K columns (b_k, c_k) drawn by the generator's law on the shared A, solved (i) by one scs_amd_solve_family call
and (ii) by K successive scs_update + scs_solve on the SAME workspace, the two sides alternated --pairs times in one process after
one warm-up of each.  Wall time is a host clock around calls that return with the stream idle.  With --identical K the same
measurement runs on a family of K copies of column 0, so that the cost of a slow column dragging the chunk can be told from the
cost of the block form itself.  --max-iters caps every solve (both sides run the same number of iterations then: a per-iteration
comparison; the drag of slow columns does not show).
One JSON line per family: wall times, the per-problem ratio family / singles, its spread over the pairs, and the iteration counts
of every column on both sides.  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402


def family_data(A, cone, K, seed):
    m, n = A.shape
    rng = np.random.default_rng(seed)
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    for k in range(K):
        z = rng.uniform(-1, 1, m)
        y = problems.proj_dual_cone_np(z, cone)
        B[:, k] = A @ rng.uniform(-1, 1, n) + (y - z)
        Cc[:, k] = -(A.T @ y)
    return B, Cc


def singles(lib, w, prob, B, Cc):
    T = lib._scs_types
    x, y, s = np.zeros(prob.n), np.zeros(prob.m), np.zeros(prob.m)
    sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
    info = T.ScsInfo()
    its, st = [], []
    t0 = time.perf_counter()
    for k in range(B.shape[1]):
        b, c = np.ascontiguousarray(B[:, k]), np.ascontiguousarray(Cc[:, k])
        assert lib.scs_update(w, b.ctypes.data_as(T.fp), c.ctypes.data_as(T.fp)) == 0
        lib.scs_solve(w, C.byref(sol), C.byref(info), 0)
        its.append(int(info.iter))
        st.append(int(info.status_val))
    return time.perf_counter() - t0, its, st


def family(lib, w, B, Cc):
    t0 = time.perf_counter()
    rc, out = capi.solve_family(lib, w, B, Cc)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt, [r["info"]["iter"] for r in out], [r["info"]["status_val"] for r in out]


def measure(lib, w, prob, B, Cc, pairs, label):
    singles(lib, w, prob, B[:, :1], Cc[:, :1])  # warm-up of both sides at this width
    family(lib, w, B, Cc)
    ts, tf = [], []
    for _ in range(pairs):
        a = family(lib, w, B, Cc)
        b = singles(lib, w, prob, B, Cc)
        tf.append(a[0])
        ts.append(b[0])
    K = B.shape[1]
    ratios = [f / s for f, s in zip(tf, ts)]
    row = dict(family=label, K=K, pairs=pairs, family_s=tf, singles_s=ts, per_problem_ratio=float(np.median(ratios)),
               ratio_min=min(ratios), ratio_max=max(ratios), spread=(max(ratios) - min(ratios)) / float(np.median(ratios)),
               iters_family=a[1], iters_singles=b[1], status_family=a[2], status_singles=b[2])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--identical", type=int, default=8, help="also a family of this many copies of column 0 (0 = skip)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--max-iters", type=int, default=100000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    ks = [int(v) for v in a.ks.split(",") if v]
    pr = problems.random_socp(a.n, 2 * a.n, a.col_nnz, seed=a.seed)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    B, Cc = family_data(pr["A"], pr["cone"], max(ks + [1]), a.seed + 1)
    st = capi.default_settings(lib, verbose=0, adaptive_scale=0, acceleration_lookback=0, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.max_iters)
    w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    assert w
    rows = []
    try:
        for K in ks:
            rows.append(measure(lib, w, prob, np.asfortranarray(B[:, :K]), np.asfortranarray(Cc[:, :K]), a.pairs, "random"))
        if a.identical:
            K = a.identical
            rows.append(measure(lib, w, prob, np.asfortranarray(np.repeat(B[:, :1], K, axis=1)), np.asfortranarray(np.repeat(Cc[:, :1], K, axis=1)),
                                a.pairs, "identical"))
    finally:
        lib.scs_finish(w)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(n=a.n, m=2 * a.n, col_nnz=a.col_nnz, eps=a.eps, max_iters=a.max_iters, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
