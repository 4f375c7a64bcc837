"""scs_amd_solve_family_scaled on one GPU: what a scale per problem costs per iteration, and what an adaptive family saves.

The shape and the family are those of scripts/bench_family.py (n x 2n second-order cone program, --col-nnz entries per column, fp64,
acceleration_lookback = 0, K columns (b_k, c_k) by the generator's law on the shared A).  Two measurements, each with the two sides
alternated --pairs times in one process after one warm-up of each, wall time by a host clock around calls that return with the
stream idle, medians reported:
 (a) per iteration: adaptive_scale = 0, every solve capped at --cap-iters (both sides then run the same iterations), the scaled
     entry with scales = NULL against scs_amd_solve_family on the same workspace -- the cost of the per-column R alone;
 (b) to termination: adaptive_scale = 1, the K columns as ONE scaled family against K successive scs_update + scs_solve on one
     workspace (where the single solve carries its adapted scale from one problem to the next).
One JSON line per measurement.  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402
from scripts.bench_family import family, family_data, singles  # noqa: E402


def family_scaled(lib, w, B, Cc, scales=None):
    t0 = time.perf_counter()
    rc, out = capi.solve_family_scaled(lib, w, B, Cc, scales=scales)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt, [r["info"]["iter"] for r in out], [r["info"]["status_val"] for r in out], [r["info"]["scale_updates"] for r in out]


def work(lib, prob, **over):
    st = capi.default_settings(lib, verbose=0, acceleration_lookback=0, **over)
    w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    assert w
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--cap-iters", type=int, default=100, help="iterations of every solve of measurement (a)")
    ap.add_argument("--max-iters", type=int, default=100000, help="cap of measurement (b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    K = a.k
    pr = problems.random_socp(a.n, 2 * a.n, a.col_nnz, seed=a.seed)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    B, Cc = family_data(pr["A"], pr["cone"], K, a.seed + 1)
    rows = []

    # (a) the per-column R alone: same iterations on both sides
    w = work(lib, prob, adaptive_scale=0, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.cap_iters)
    try:
        family(lib, w, B, Cc)
        family_scaled(lib, w, B, Cc)
        t_old, t_new = [], []
        for _ in range(a.pairs):
            t_old.append(family(lib, w, B, Cc)[0])
            t_new.append(family_scaled(lib, w, B, Cc)[0])
    finally:
        lib.scs_finish(w)
    ratios = [x / y for x, y in zip(t_new, t_old)]
    rows.append(dict(measurement="per_iteration", K=K, iters=a.cap_iters, pairs=a.pairs, shared_s=t_old, scaled_s=t_new,
                     shared_ms_per_iter=1e3 * float(np.median(t_old)) / a.cap_iters, scaled_ms_per_iter=1e3 * float(np.median(t_new)) / a.cap_iters,
                     ratio=float(np.median(ratios)), ratio_min=min(ratios), ratio_max=max(ratios)))
    print(json.dumps(rows[-1]), flush=True)

    # (b) adaptive, to termination: one family against K single solves in a loop
    w = work(lib, prob, adaptive_scale=1, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.max_iters)
    try:
        singles(lib, w, prob, B[:, :1], Cc[:, :1])
        fam = family_scaled(lib, w, B, Cc)
        t_fam, t_one = [], []
        for _ in range(a.pairs):
            fam = family_scaled(lib, w, B, Cc)
            one = singles(lib, w, prob, B, Cc)
            t_fam.append(fam[0])
            t_one.append(one[0])
    finally:
        lib.scs_finish(w)
    ratios = [x / y for x, y in zip(t_fam, t_one)]
    rows.append(dict(measurement="adaptive_to_termination", K=K, pairs=a.pairs, family_s=t_fam, singles_s=t_one,
                     family_median_s=float(np.median(t_fam)), singles_median_s=float(np.median(t_one)), ratio=float(np.median(ratios)),
                     ratio_min=min(ratios), ratio_max=max(ratios), iters_family=fam[1], iters_singles=one[1], status_family=fam[2],
                     status_singles=one[2], scale_updates_family=fam[3]))
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(n=a.n, m=2 * a.n, col_nnz=a.col_nnz, eps=a.eps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
