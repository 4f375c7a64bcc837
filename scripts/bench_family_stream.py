"""A queue of problems through one block, one GPU: what scs_amd_solve_family_stream costs against scs_amd_solve_family's chunks.

On the headline shape (n x 2n, 10 entries per column, fp64, adaptive_scale = 0, acceleration_lookback = 0, eps 1e-4): a queue of
--nprob problems (b_k, c_k) drawn by the generator's law on the shared A, b_k scaled by a factor from a seeded list over
{3, 10, 30} so that the iteration counts differ, solved (i) by one scs_amd_solve_family_stream call at every width of --widths and
(ii) by scs_amd_solve_family on the same queue (chunks of 16, each waiting for its slowest column), on the SAME workspace, the two
sides alternated --pairs times in one process after one warm-up of each.  Wall time is a host clock around calls that return with
the stream idle.
One JSON line per width: both wall times, their ratio stream / chunks per pair with its median and spread, the iteration count of
every problem on both sides (equal at width 16, the chunks' width, where the bits are; at another width the reduction trees and
with them the counts may differ), the six counters of the stream call, its idle share [2] / ([1] + [2]), and the block iterations
the chunked call needs, computed from its iteration counts (the sum over the chunks of the largest count, a converged column
counting its last iteration too).  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402

FACTORS = (3.0, 10.0, 30.0)


def queue_data(A, cone, K, seed):
    m, n = A.shape
    rng = np.random.default_rng(seed)
    f = np.array(FACTORS)[np.random.default_rng(seed + 1).integers(0, len(FACTORS), K)]
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    for k in range(K):
        z = rng.uniform(-1, 1, m)
        y = problems.proj_dual_cone_np(z, cone)
        B[:, k] = (A @ rng.uniform(-1, 1, n) + (y - z)) * f[k]
        Cc[:, k] = -(A.T @ y)
    return B, Cc, [float(v) for v in f]


def timed(call):
    t0 = time.perf_counter()
    rc, out = call()
    dt = time.perf_counter() - t0
    assert rc == 0
    print(f"{call.__name__}: {dt:.2f} s", file=sys.stderr, flush=True)  # progress: a call takes tens of seconds at the default size
    return dt, [r["info"]["iter"] for r in out], [r["info"]["status_val"] for r in out]


def measure(lib, w, B, Cc, width, pairs, max_iters):
    def stream():
        return capi.solve_family_stream(lib, w, B, Cc, width=width)

    def chunks():
        return capi.solve_family(lib, w, B, Cc)
    timed(stream)  # warm-up of both sides
    timed(chunks)
    ts, tc = [], []
    for _ in range(pairs):
        a = timed(stream)
        cnt = capi.family_stream_counters(lib, w)
        b = timed(chunks)
        ts.append(a[0])
        tc.append(b[0])
    ratios = [s / c for s, c in zip(ts, tc)]
    ran = [it + 1 if it < max_iters else max_iters for it in b[1]]
    row = dict(width=width, nprob=B.shape[1], pairs=pairs, stream_s=ts, chunks_s=tc, ratio=ratios, ratio_median=float(np.median(ratios)),
               spread=(max(ratios) - min(ratios)) / float(np.median(ratios)), iters_stream=a[1], iters_chunks=b[1],
               iters_equal=a[1] == b[1], status_stream=a[2], status_chunks=b[2], counters=cnt,
               idle_share=cnt["idle_slot_iters"] / max(1, cnt["run_slot_iters"] + cnt["idle_slot_iters"]),
               block_iters_chunks=sum(max(ran[g:g + 16]) for g in range(0, len(ran), 16)))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--nprob", type=int, default=48)
    ap.add_argument("--widths", default="8,16")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--max-iters", type=int, default=100000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    pr = problems.random_socp(a.n, 2 * a.n, a.col_nnz, seed=a.seed)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    B, Cc, factors = queue_data(pr["A"], pr["cone"], a.nprob, a.seed + 1)
    st = capi.default_settings(lib, verbose=0, adaptive_scale=0, acceleration_lookback=0, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.max_iters)
    w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    assert w
    rows = []
    try:
        for width in (int(v) for v in a.widths.split(",") if v):
            rows.append(measure(lib, w, B, Cc, width, a.pairs, a.max_iters))
    finally:
        lib.scs_finish(w)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(n=a.n, m=2 * a.n, col_nnz=a.col_nnz, eps=a.eps, max_iters=a.max_iters, b_factors=factors, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
