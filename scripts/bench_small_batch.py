"""Batches of small problems, one GPU: what scs_amd_small_solve (one workgroup per problem, one launch) costs against what the
library offered before it for the same list of problems.

Workload: random_socp-law problems (scs_amd/problems.py) at the shapes of --shapes, a shared A and --nprobs problems (b_k, c_k)
drawn by the generator's law, fp64, eps 1e-4, adaptive_scale = 0, acceleration_lookback = 0, to termination.  Sides:
  small   SmallBatch.solve on the whole list (exact linear solves);
  loop    scs_update + scs_solve problem after problem on one workspace (the default inexact CG schedule);
  stream  solve_family_stream at width 16 on one workspace.
The three sides are alternated --pairs times in one process after one warm-up of each; wall time is a host clock around calls that
return with the stream idle.  `loop` and `stream` cost the same per problem whatever the length of the list (the loop exactly, the
stream up to its tail), and a pass of either over 16384 problems takes an hour or more: they run on the first --base-nprob problems of the
list only, and their rate in problems per second is what a longer list is compared with.  Every row says on how many problems each
side ran.  The iteration counts of the sides differ (exact against inexact solves): a ratio compares the time to the same
tolerance, not equal work.
Writes one JSON line per (shape, nprob) and, with --md, the table of profiles/small_batch.md.  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402
from scs_amd.small import SmallBatch  # noqa: E402


def family(A, cone, K, seed):
    m, n = A.shape
    rng = np.random.default_rng(seed)
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    for k in range(K):
        z = rng.uniform(-1, 1, m)
        y = problems.proj_dual_cone_np(z, cone)
        B[:, k] = A @ rng.uniform(-1, 1, n) + (y - z)
        Cc[:, k] = -(A.T @ y)
    return B, Cc


def med(v):
    return float(np.median(v))


def spread(v):
    return (max(v) - min(v)) / med(v)


class Loop:
    """scs_update + scs_solve per problem on one workspace"""

    def __init__(self, lib, prob, st):
        self.lib, self.prob, self.T = lib, prob, lib._scs_types
        self.w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
        assert self.w

    def run(self, B, Cc):
        T, lib = self.T, self.lib
        x, y, s = np.zeros(self.prob.n), np.zeros(self.prob.m), np.zeros(self.prob.m)
        sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
        info = T.ScsInfo()
        its = 0
        for k in range(B.shape[1]):
            b, c = np.ascontiguousarray(B[:, k]), np.ascontiguousarray(Cc[:, k])
            assert lib.scs_update(self.w, b.ctypes.data_as(T.fp), c.ctypes.data_as(T.fp)) == 0
            lib.scs_solve(self.w, C.byref(sol), C.byref(info), 0)
            its += info.iter
        return its

    def stream(self, B, Cc):
        rc, out = capi.solve_family_stream(self.lib, self.w, B, Cc, width=16)
        assert rc == 0
        return sum(r["info"]["iter"] for r in out)

    def close(self):
        self.lib.scs_finish(self.w)


def clock(f, *a):
    t0 = time.perf_counter()
    r = f(*a)
    return time.perf_counter() - t0, r


def measure(lib, n, m, nprobs, base_nprob, pairs, eps, seed):
    pr = problems.random_socp(n, m, min(10, m), seed=seed)
    A, cone = pr["A"], pr["cone"]
    B, Cc = family(A, cone, max(nprobs), seed + 1)
    kw = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0, eps_abs=eps, eps_rel=eps)
    st = capi.default_settings(lib, **kw)
    t_setup, sb = clock(lambda: SmallBatch(dict(A=A, b=pr["b"], c=pr["c"]), cone, **kw))
    base = Loop(lib, capi.Problem(A, pr["b"], pr["c"], cone), st)
    rows = []
    try:
        def small(K):
            out = sb.solve(B[:, :K], Cc[:, :K])
            return sum(r["info"]["iter"] for r in out), max(r["info"]["iter"] for r in out)
        Kb = min(base_nprob, max(nprobs))
        small(min(nprobs))  # warm-up of the three sides (the first small call also creates the object's device side)
        base.run(B[:, :16], Cc[:, :16])
        base.stream(B[:, :32], Cc[:, :32])
        occ = sb.occupancy()
        t1, (it1, _) = clock(small, 1)  # one problem alone: the latency of one workgroup
        tl, ts = [], []
        per_k = {K: [] for K in nprobs}
        for _ in range(pairs):
            for K in nprobs:
                per_k[K].append(clock(small, K))
            tl.append(clock(base.run, B[:, :Kb], Cc[:, :Kb]))
            ts.append(clock(base.stream, B[:, :Kb], Cc[:, :Kb]))
            print(f"pair done: n={n} small {[round(per_k[K][-1][0], 4) for K in nprobs]} loop {tl[-1][0]:.2f} stream {ts[-1][0]:.2f}",
                  file=sys.stderr, flush=True)
        loop_rate = [Kb / t for t, _ in tl]
        stream_rate = [Kb / t for t, _ in ts]
        for K in nprobs:
            t = [v[0] for v in per_k[K]]
            its, itmax = per_k[K][0][1]
            wgs = min(K, occ["default_grid"])
            row = dict(n=n, m=m, nprob=K, pairs=pairs, eps=eps, small_s=t, small_s_median=med(t), small_spread=spread(t),
                       small_rate=K / med(t), small_iters=its, small_iters_max=itmax,
                       us_per_problem_iteration=1e6 * med(t) / its, workgroup_us_per_iteration=1e6 * med(t) * wgs / its,
                       one_problem_us_per_iteration=1e6 * t1 / max(it1, 1), one_problem_iters=it1,
                       base_nprob=Kb, loop_s=[v[0] for v in tl], loop_rate=med(loop_rate), loop_spread=spread(loop_rate),
                       loop_iters=tl[0][1], stream_s=[v[0] for v in ts], stream_rate=med(stream_rate), stream_spread=spread(stream_rate),
                       stream_iters=ts[0][1], small_iters_on_base=small(Kb)[0],
                       speedup_vs_loop=[(K / a) / b for a, b in zip(t, loop_rate)], speedup_vs_stream=[(K / a) / b for a, b in zip(t, stream_rate)],
                       setup_s=occ["setup_s"], setup_python_s=t_setup, occupancy=occ, workgroups=wgs)
            row["speedup_vs_loop_median"] = med(row["speedup_vs_loop"])
            row["speedup_vs_stream_median"] = med(row["speedup_vs_stream"])
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        base.close()
        sb.close()
    return rows


def write_md(path, rows, regs):
    L = ["# Batches of small problems: one workgroup per problem (scs_amd_small_solve)", "",
         "Written by `scripts/bench_small_batch.py` on one MI355X; fp64, eps 1e-4, adaptive_scale = 0, acceleration_lookback = 0, random_socp-law",
         "problems on a shared A, to termination.  Medians of %d alternated rounds (small at every list length, then loop, then stream);" % rows[0]["pairs"],
         "spread = (max - min) / median over the rounds.  Wall time is a host clock around the call (staging, launch, read-back and the",
         "host's finalize included).  `loop` = scs_update + scs_solve per problem on one workspace; `stream` = solve_family_stream, width 16.",
         "`loop` and `stream` ran on the first %d problems of each list only (a pass of the loop over 16384 takes more than an hour); their rate is what the" % rows[0]["base_nprob"],
         "lists are compared with -- the two baselines are NOT measured at the full length of any list longer than that.",
         "The iteration counts differ between the sides (exact against inexact linear solves), so a ratio compares the time to the same",
         "tolerance, not equal work.", "",
         "| n | m | problems | small: s (spread) | small: problems/s | loop: problems/s (spread) | stream: problems/s (spread) | small / loop | small / stream |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %d | %d | %d | %.4f (%.0f%%) | %.0f | %.2f (%.0f%%) | %.2f (%.0f%%) | %.0fx | %.0fx |" % (
            r["n"], r["m"], r["nprob"], r["small_s_median"], 100 * r["small_spread"], r["small_rate"], r["loop_rate"], 100 * r["loop_spread"],
            r["stream_rate"], 100 * r["stream_spread"], r["speedup_vs_loop_median"], r["speedup_vs_stream_median"]))
    L += ["", "Iterations, summed over the problems each side ran:", "",
          "| n | m | problems | small: iterations (largest of one problem) | on the first %d: small | loop | stream |" % rows[0]["base_nprob"], "|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %d | %d | %d | %d (%d) | %d | %d | %d |" % (r["n"], r["m"], r["nprob"], r["small_iters"], r["small_iters_max"],
                                                         r["small_iters_on_base"], r["loop_iters"], r["stream_iters"]))
    L += ["", "The kernel, from the same wall times (so with the staging and the read-back inside):", "",
          "| n | m | problems | workgroups | us per problem-iteration (wall / iterations) | x workgroups (a launch lasts as long as its slowest workgroup, so this holds idle time) | one problem alone: us per iteration |",
          "|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %d | %d | %d | %d | %.4f | %.2f | %.2f |" % (r["n"], r["m"], r["nprob"], r["workgroups"], r["us_per_problem_iteration"],
                                                          r["workgroup_us_per_iteration"], r["one_problem_us_per_iteration"]))
    L += ["", "Occupancy and setup:", "", "| n | m | workgroups per CU | LDS per workgroup (bytes) | default grid | setup (s): init on the host + device side at the first solve |",
          "|---|---|---|---|---|---|"]
    seen = set()
    for r in rows:
        if (r["n"], r["m"]) in seen:
            continue
        seen.add((r["n"], r["m"]))
        o = r["occupancy"]
        L.append("| %d | %d | %d | %d | %d | %.4f |" % (r["n"], r["m"], o["wg_per_cu"], o["lds_bytes"], o["default_grid"], r["setup_s"]))
    L += ["", "Registers of `k_small_batch` (the compiler's resource report for gfx950): %s." % regs, "",
          "Not measured: the fp32 and the 64-bit-index builds; problems with P; the two baselines at full list length (above); a kernel",
          "time separated from the call's staging and read-back; anything on more than one GPU.", ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x96,128x384")
    ap.add_argument("--nprobs", default="256,2048,16384")
    ap.add_argument("--base-nprob", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    ap.add_argument("--regs", default="not recorded")
    a = ap.parse_args()
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    rows = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        rows += measure(lib, n, m, [int(v) for v in a.nprobs.split(",")], a.base_nprob, a.pairs, a.eps, a.seed)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        if a.md:
            write_md(a.md, rows, a.regs)


if __name__ == "__main__":
    main()
