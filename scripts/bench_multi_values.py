"""K KKT systems on one pattern with their own values (scs_amd_linsys_set_values_multi, scs_amd_solve_lin_sys_multi_v), one GPU: what
the per-value block costs against what a caller has today.

On the headline shape (n x 2n, 10 entries per column, the generator of scs_amd/problems.py as scripts/bench_linsys_multi.py uses
it; --n 200000 for the smaller one), the values of column k being A's times (1 + 0.3 u_k), u_k uniform in (-1, 1), and for every K
of --ks:
  (a) the per-value block solve of K random columns at --tol;
  (b) the same columns as a loop of scs_amd_linsys_update_values + scs_solve_lin_sys: the code a caller runs today, the baseline;
  (c) the shared-value block scs_amd_solve_lin_sys_multi_r on the same right-hand sides (the workspace's values in every column): what
      the per-column values cost over shared ones;
  (d) the set call.
(a) and (b) are alternated --reps times, then (a) and (c), and the medians are reported with the spread over the repeats; every
timed call ends with the stream idle (the entries return so).  One JSON line per K; with --out the records are also written to
OUT.json and a table to OUT.md.  --shared-only runs (c) alone and needs none of the per-value entries, so it also runs on a build
from before them; --parent FILE puts such a run's (c) beside this build's in the table.  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--amp", type=float, default=0.3)
    ap.add_argument("--lib", default="libscsamd_linsys.so")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose scs_amd package and libraries are measured")
    ap.add_argument("--shared-only", action="store_true")
    ap.add_argument("--parent", default=None, help="JSON lines of a --shared-only run on the parent build")
    ap.add_argument("--out", default=None, help="write OUT.json and OUT.md")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    from scs_amd import capi, problems
    import scipy.sparse as sp

    n, m = a.n, a.m or 2 * a.n
    lib = capi.load(a.lib)
    if lib.scs_amd_device_count() <= 0:
        sys.exit("bench_multi_values: no GPU (a measurement path does not fall back)")
    T = lib._scs_types
    fp = lambda v: v.ctypes.data_as(T.fp)
    rng = np.random.default_rng(0)
    t0 = time.time()
    rows = problems.random_rows(m, n, a.col_nnz, rng)
    vals = rng.uniform(-1, 1, size=(n, a.col_nnz)).astype(T.np_float)
    A = sp.csc_matrix((vals.ravel(), rows.ravel().astype(np.int32), np.arange(0, (n + 1) * a.col_nnz, a.col_nnz, dtype=np.int32)), shape=(m, n))
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m), T=T)
    nnz = len(prob.Ax)
    dr = np.empty(n + m, dtype=T.np_float)
    dr[:n] = 1e-6
    dr[n:n + m // 10] = 1.0 / 100.0
    dr[n + m // 10:] = 10.0
    print(f"gen {time.time() - t0:.1f}s n={n} m={m} nnz={nnz}", file=sys.stderr, flush=True)
    w = lib.scs_init_lin_sys_work(C.byref(prob.matA), None, fp(dr))
    assert w
    med = lambda v: float(np.median(v))
    spread = lambda v: round((max(v) - min(v)) / med(v), 4)
    recs = []
    for K in [int(v) for v in a.ks.split(",")]:
        B = np.asfortranarray(rng.uniform(-1, 1, (n + m, K)).astype(T.np_float))
        DR = np.asfortranarray(np.tile(dr[:, None], (1, K)))
        AX = np.asfortranarray(prob.Ax[:, None] * (1.0 + a.amp * rng.uniform(-1, 1, (nnz, K))).astype(T.np_float))
        tv = np.full(K, a.tol, dtype=T.np_float)
        it_v, it_r, it_1 = (np.zeros(K, dtype=T.np_int) for _ in range(3))

        def block(entry, it, tolv=tv):
            out = B.copy(order="F")
            t0 = time.perf_counter()
            rc = entry(w, K, fp(DR), n + m, fp(out), n + m, None, 0, fp(tolv), it.ctypes.data_as(T.ip))
            dt = time.perf_counter() - t0
            assert rc == 0
            return dt, out

        def loop():
            out = B.copy(order="F")
            t0 = time.perf_counter()
            for k in range(K):
                assert lib.scs_amd_linsys_update_values(w, fp(AX[:, k]), None) == 0
                assert lib.scs_solve_lin_sys(w, fp(out[:, k]), None, a.tol) == 0
            dt = time.perf_counter() - t0
            return dt, out

        def set_call():
            t0 = time.perf_counter()
            assert lib.scs_amd_linsys_set_values_multi(w, K, fp(AX), nnz, None, 0) == 0
            return time.perf_counter() - t0

        half = np.full(K, 0.5, dtype=T.np_float)
        rec = dict(K=K, width=max(2, lib.scs_amd_linsys_multi_width(K)), n=n, m=m, nnz=nnz, tol=a.tol, reps=a.reps, lib=a.lib)
        block(lib.scs_amd_solve_lin_sys_multi_r, it_r, half)  # buffers and code objects outside the timed calls
        if a.shared_only:
            tc = [block(lib.scs_amd_solve_lin_sys_multi_r, it_r)[0] for _ in range(a.reps)]
            rec.update(shared_block_s=round(med(tc), 4), shared_block_spread=spread(tc), iters_shared=[int(v) for v in it_r])
        else:
            td = [set_call() for _ in range(a.reps + 1)][1:]  # the first one allocates
            block(lib.scs_amd_solve_lin_sys_multi_v, it_v, half)
            ta, tb, ta2, tc = [], [], [], []
            for _ in range(a.reps):  # alternated pairs: block against the loop a caller runs today
                dt, out_v = block(lib.scs_amd_solve_lin_sys_multi_v, it_v)
                ta.append(dt)
                dt, out_1 = loop()
                tb.append(dt)
            assert lib.scs_amd_linsys_update_values(w, fp(prob.Ax), None) == 0  # the workspace's own values back
            for _ in range(a.reps):  # alternated pairs: per-column values against shared ones
                ta2.append(block(lib.scs_amd_solve_lin_sys_multi_v, it_v)[0])
                tc.append(block(lib.scs_amd_solve_lin_sys_multi_r, it_r)[0])
            worst = max(float(np.abs(out_v[:, k] - out_1[:, k]).max() / np.abs(out_1[:, k]).max()) for k in range(K))
            rec.update(values_block_s=round(med(ta), 4), values_block_spread=spread(ta), update_solve_loop_s=round(med(tb), 4),
                       update_solve_loop_spread=spread(tb), block_over_loop=round(med(ta) / med(tb), 4),
                       values_block_2_s=round(med(ta2), 4), shared_block_s=round(med(tc), 4), shared_block_spread=spread(tc),
                       values_over_shared=round(med(ta2) / med(tc), 4), set_call_s=round(med(td), 4), set_call_spread=spread(td),
                       set_call_GBps=round(nnz * K * np.dtype(T.np_float).itemsize / med(td) / 1e9, 2),
                       iters_values=[int(v) for v in it_v], iters_shared=[int(v) for v in it_r], block_vs_loop_rel_diff=float(f"{worst:.3e}"),
                       value_blocks_MB=round(2 * nnz * rec["width"] * np.dtype(T.np_float).itemsize / 1e6, 1))
            lib.scs_amd_linsys_free_values_multi(w)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    lib.scs_free_lin_sys_work(w)
    if a.out:
        write(a, recs)


def write(a, recs):
    parent = {}
    if a.parent and os.path.exists(a.parent):
        with open(a.parent) as f:
            for line in f:
                if line.startswith("{"):
                    r = json.loads(line)
                    parent[(r["n"], r["K"])] = r
    for r in recs:
        p = parent.get((r["n"], r["K"]))
        if p:
            r["parent_shared_block_s"] = p["shared_block_s"]
            r["parent_shared_block_spread"] = p["shared_block_spread"]
    mode = "a" if os.path.exists(a.out + ".json") else "w"
    with open(a.out + ".json", mode) as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    with open(a.out + ".md", mode) as f:
        if mode == "w":
            f.write("# Per-column values: the block solve against update + solve, one MI355X\n\n"
                    "scripts/bench_multi_values.py; medians of %d alternated pairs, seconds per call of K columns, host clock around entries\n"
                    "that return with the stream idle; spread = (max - min) / median over the repeats.\n"
                    "(a) scs_amd_solve_lin_sys_multi_v; (b) K x (scs_amd_linsys_update_values + scs_solve_lin_sys); (c) scs_amd_solve_lin_sys_multi_r\n"
                    "on the workspace's shared values, this build and the parent commit's; (d) scs_amd_linsys_set_values_multi.\n" % a.reps)
        r0 = recs[0]
        f.write(f"\n## n = {r0['n']}, m = {r0['m']}, nnz = {r0['nnz']}, tol = {r0['tol']}\n\n"
                "| K | W | (a) block, values | (b) update + solve loop | (a) / (b) | (a) again | (c) shared block | (a) / (c) | (c) parent | (d) set call | value blocks MB | iterations (a) |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in recs:
            if "values_block_s" not in r:
                continue
            f.write(f"| {r['K']} | {r['width']} | {r['values_block_s']} ({r['values_block_spread']}) | {r['update_solve_loop_s']} ({r['update_solve_loop_spread']}) "
                    f"| {r['block_over_loop']} | {r['values_block_2_s']} | {r['shared_block_s']} ({r['shared_block_spread']}) | {r['values_over_shared']} "
                    f"| {r.get('parent_shared_block_s', 'not measured')} | {r['set_call_s']} ({r['set_call_GBps']} GB/s) | {r['value_blocks_MB']} "
                    f"| {min(r['iters_values'])} .. {max(r['iters_values'])} |\n")


if __name__ == "__main__":
    main()
