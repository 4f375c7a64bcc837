"""Batches of small problems that each bring their own values of A and P (scs_amd_small_set_values / scs_amd_small_solve_values),
one GPU: what own values cost against the shared-values entry, what the set call and the per-problem factor cost, and what the
library offered before for the same list.

Workload: random_socp-law problems (scs_amd/problems.py) at the shapes of --shapes, fp64, eps 1e-4, adaptive_scale = 0,
acceleration_lookback = 0, to termination; --nprobs problems (b_k, c_k) drawn by the generator's law.  Every problem's values are
the shared A (AX = A.data tiled): the values entry still reads every problem's own blocks in HBM and factors every problem, and
the iteration counts are those of the shared entry, so the ratio of the two is what own values cost.  Sides:
  values  SmallBatch.solve(B, C, own_values=True) after one set_values (timed apart);
  shared  SmallBatch.solve(B, C) on the same object;
  loop    scs_amd_update_matrix + scs_update + scs_solve problem after problem on one workspace, on the first --base-nprob
          problems (its cost per problem does not depend on the length of the list);
  factor  both entries with max_iters = 1 on objects of their own: the difference is the per-problem factor (assembly, Cholesky,
          inverse) plus the first read of the problem's blocks.
With --parent-lib (a libscsamd.so built from the parent commit) the shared entry of the two builds is timed in alternated pairs,
beside an A/A pair of two objects of this build.
--compare-bits FILE (with --parent-lib) measures nothing: it solves the cases of tests/small_batch_util.py with the shared entry of
both builds, writes whether x, y, s, iter, status_val and the residuals are bit-identical, and exits.  --render JSON writes --md
from the rows of an earlier --out (with --notes appended) without a GPU.
The sides are alternated --rounds times in one process after one warm-up of each; wall time is a host clock around calls that
return with the stream idle.  Writes one JSON line per (shape, nprob) and, with --md, the tables of profiles/small_values.md.
No pass mark: it reports."""
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
from scripts.bench_small_batch import clock, family, med, spread  # noqa: E402


class Loop:
    """scs_amd_update_matrix + scs_update + scs_solve per problem on one workspace"""

    def __init__(self, lib, prob, st):
        self.lib, self.prob, self.T = lib, prob, lib._scs_types
        self.w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
        assert self.w

    def run(self, AX, B, Cc):
        T, lib = self.T, self.lib
        x, y, s = np.zeros(self.prob.n), np.zeros(self.prob.m), np.zeros(self.prob.m)
        sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
        info = T.ScsInfo()
        its = 0
        for k in range(B.shape[1]):
            ax, b, c = (np.ascontiguousarray(v[:, k]) for v in (AX, B, Cc))
            assert lib.scs_amd_update_matrix(self.w, ax.ctypes.data_as(T.fp), None) == 0
            assert lib.scs_update(self.w, b.ctypes.data_as(T.fp), c.ctypes.data_as(T.fp)) == 0
            lib.scs_solve(self.w, C.byref(sol), C.byref(info), 0)
            its += info.iter
        return its

    def close(self):
        self.lib.scs_finish(self.w)


def other_build(path):
    """SmallBatch objects of another build of libscsamd.so: the class takes its library from capi's table by name"""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    here = capi.load("libscsamd.so")
    # the shared-values entries only, with this build's signatures: an older build has no own-values entries to bind
    for name in ("scs_set_default_settings", "scs_amd_small_init", "scs_amd_small_refusal", "scs_amd_small_limits", "scs_amd_small_solve",
                 "scs_amd_small_set_grid", "scs_amd_small_get_counters", "scs_amd_small_get_occupancy", "scs_amd_small_finish"):
        f, g = getattr(lib, name), getattr(here, name)
        f.restype, f.argtypes = g.restype, g.argtypes
    lib._scs_types = here._scs_types

    def make(*a, **kw):
        mine = capi._cache["libscsamd.so"]
        capi._cache["libscsamd.so"] = lib
        try:
            return SmallBatch(*a, **kw)
        finally:
            capi._cache["libscsamd.so"] = mine
    return make


def measure(lib, n, m, nprobs, base_nprob, rounds, eps, seed, parent):
    pr = problems.random_socp(n, m, min(10, m), seed=seed)
    A, cone = pr["A"], pr["cone"]
    Kmax = max(nprobs)
    B, Cc = family(A, cone, Kmax, seed + 1)
    kw = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0, eps_abs=eps, eps_rel=eps)
    data = dict(A=A, b=pr["b"], c=pr["c"])
    prob = capi.Problem(A, pr["b"], pr["c"], cone)
    AX = np.asfortranarray(np.repeat(prob.Ax[:, None], Kmax, axis=1))
    sb, sb2, sb1 = SmallBatch(data, cone, **kw), SmallBatch(data, cone, **kw), SmallBatch(data, cone, **dict(kw, max_iters=1))
    sbp = parent(data, cone, **kw) if parent else None
    base = Loop(lib, prob, capi.default_settings(lib, **kw))
    rows = []
    try:
        def its(out):
            return sum(r["info"]["iter"] for r in out)
        Kb = min(base_nprob, Kmax)
        for o in (sb, sb2, sb1) + ((sbp,) if sbp else ()):  # warm-up: the device side of every object
            o.solve(B[:, :min(nprobs)], Cc[:, :min(nprobs)])
        base.run(AX[:, :4], B[:, :4], Cc[:, :4])
        sb.set_values(AX[:, :min(nprobs)])
        sb.solve(B[:, :min(nprobs)], Cc[:, :min(nprobs)], own_values=True)
        occ = sb.occupancy()
        tl = []
        per = {K: dict(set=[], values=[], shared=[], shared_b=[], parent=[], f_own=[], f_sh=[]) for K in nprobs}
        for _ in range(rounds):
            for K in nprobs:
                b, c, d = B[:, :K], Cc[:, :K], per[K]
                d["set"].append(clock(sb.set_values, AX[:, :K])[0])
                t, out = clock(lambda: sb.solve(b, c, own_values=True))
                d["values"].append(t)
                d["iters_values"] = its(out)
                t, out = clock(sb.solve, b, c)
                d["shared"].append(t)
                d["iters_shared"] = its(out)
                d["shared_b"].append(clock(sb2.solve, b, c)[0])
                if sbp:
                    d["parent"].append(clock(sbp.solve, b, c)[0])
                sb1.set_values(AX[:, :K])
                d["f_own"].append(clock(lambda: sb1.solve(b, c, own_values=True))[0])
                d["f_sh"].append(clock(sb1.solve, b, c)[0])
                sb1.free_values()
            tl.append(clock(base.run, AX[:, :Kb], B[:, :Kb], Cc[:, :Kb]))
            print(f"round done: n={n} values {[round(per[K]['values'][-1], 4) for K in nprobs]} loop {tl[-1][0]:.2f}", file=sys.stderr, flush=True)
        loop_rate = [Kb / t for t, _ in tl]
        for K in nprobs:
            d = per[K]
            fac = [a - b for a, b in zip(d["f_own"], d["f_sh"])]
            row = dict(n=n, m=m, nprob=K, rounds=rounds, eps=eps, values_s=d["values"], values_s_median=med(d["values"]),
                       values_spread=spread(d["values"]), values_rate=K / med(d["values"]), shared_s=d["shared"],
                       shared_s_median=med(d["shared"]), shared_spread=spread(d["shared"]), shared_rate=K / med(d["shared"]),
                       values_over_shared=[a / b for a, b in zip(d["values"], d["shared"])], iters_values=d["iters_values"],
                       iters_shared=d["iters_shared"], set_s=d["set"], set_us_per_problem=1e6 * med(d["set"]) / K, set_spread=spread(d["set"]),
                       factor_s=fac, factor_us_per_problem=1e6 * med(fac) / K, factor_share=med(fac) / med(d["values"]),
                       base_nprob=Kb, loop_s=[v[0] for v in tl], loop_rate=med(loop_rate), loop_spread=spread(loop_rate), loop_iters=tl[0][1],
                       values_vs_loop=[(K / a) / b for a, b in zip(d["values"], loop_rate)],
                       aa=[a / b for a, b in zip(d["shared"], d["shared_b"])],
                       vs_parent=[a / b for a, b in zip(d["shared"], d["parent"])] if sbp else None, occupancy=occ)
            for k in ("values_over_shared", "values_vs_loop", "aa") + (("vs_parent",) if sbp else ()):
                row[k + "_median"] = med(row[k])
                row[k + "_spread"] = spread(row[k])
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        base.close()
        for o in (sb, sb2, sb1, sbp):
            if o:
                o.close()
    return rows


def compare_bits(parent):
    """The shared entry of this build against another build's: x, y, s and the ScsInfo fields of tests/small_batch_util.same_bits
    (iter, status_val, objectives, residuals) on that module's six cases and its mixed-status list.  Lines of text, and whether
    every problem was bit-identical."""
    from tests import small_batch_util as U
    lists = [(name,) + U.case(name) for name in U.CASES]
    A, cone, B, Cc = U.mixed_statuses(1)
    lists.append(("mixed_statuses", A, None, cone, B, Cc, dict(U.SETTINGS, max_iters=400)))
    lines, ok = [], True
    for name, A, P, cone, B, Cc, st in lists:
        data = dict(A=A, b=B[:, 0], c=Cc[:, 0])
        if P is not None:
            data["P"] = P
        with SmallBatch(data, cone, **st) as a, parent(data, cone, **st) as b:
            assert a._lib is not b._lib
            ra, rb = a.solve(B, Cc), b.solve(B, Cc)
        same = [U.same_bits(x, y) for x, y in zip(ra, rb)]
        ok = ok and all(same)
        lines.append("%s: %d of %d problems bit-identical; iterations %s" % (name, sum(same), len(same), [r["info"]["iter"] for r in ra]))
    return lines, ok


def write_md(path, rows, notes):
    r0 = rows[0]
    L = ["# Batches of small problems with their own A and P (scs_amd_small_set_values / scs_amd_small_solve_values)", "",
         "Written by `scripts/bench_small_values.py` on one MI355X; fp64, eps %g, adaptive_scale = 0, acceleration_lookback = 0," % r0["eps"],
         "random_socp-law problems, to termination.  Every problem's values are the shared A tiled, so both entries run the same",
         "iterations; the values entry reads every problem's own blocks and factors every problem.  Medians of %d alternated rounds;" % r0["rounds"],
         "spread = (max - min) / median over the rounds.  Wall time is a host clock around the call (staging, launch, read-back and the",
         "host's finalize included).  `loop` = scs_amd_update_matrix + scs_update + scs_solve per problem on one workspace, on the first",
         "%d problems of each list only; its rate is what the lists are compared with." % r0["base_nprob"], "",
         "| n | m | problems | values: s (spread) | values: problems/s | shared: s (spread) | values / shared time (spread) | loop: problems/s (spread) | values / loop |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %d | %d | %d | %.4f (%.0f%%) | %.0f | %.4f (%.0f%%) | %.2f (%.0f%%) | %.2f (%.0f%%) | %.0fx |" % (
            r["n"], r["m"], r["nprob"], r["values_s_median"], 100 * r["values_spread"], r["values_rate"], r["shared_s_median"],
            100 * r["shared_spread"], r["values_over_shared_median"], 100 * r["values_over_shared_spread"], r["loop_rate"],
            100 * r["loop_spread"], r["values_vs_loop_median"]))
    L += ["", "The set call (host: check, equilibrate, scatter into the padded rows; upload) and the per-problem factor (the values entry",
          "against the shared entry, both at max_iters = 1: assembly, Cholesky, inverse and the first read of the problem's blocks).  The",
          "factor is a DIFFERENCE of two wall times: its median is given with the smallest and the largest round, and where that range",
          "reaches zero the factor is not resolved from the noise of the two calls:", "",
          "| n | m | problems | set: us per problem (spread) | factor: us of wall per problem | factor's share of the values solve: median (smallest .. largest round) | iterations: values | shared | loop on %d |" % r0["base_nprob"],
          "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %d | %d | %d | %.1f (%.0f%%) | %.2f | %.1f%% (%.1f%% .. %.1f%%) | %d | %d | %d |" % (
            r["n"], r["m"], r["nprob"], r["set_us_per_problem"], 100 * r["set_spread"], r["factor_us_per_problem"], 100 * r["factor_share"],
            100 * min(r["factor_s"]) / r["values_s_median"], 100 * max(r["factor_s"]) / r["values_s_median"],
            r["iters_values"], r["iters_shared"], r["loop_iters"]))
    L += ["", "The shared entry: this build against a second object of this build (A/A)" + (" and against the parent commit's build" if r0["vs_parent"] else "") +
          ", time ratios of alternated pairs:", "",
          "| n | m | problems | A/A: median (spread) | this / parent: median (spread) |", "|---|---|---|---|---|"]
    for r in rows:
        L.append("| %d | %d | %d | %.3f (%.1f%%) | %s |" % (r["n"], r["m"], r["nprob"], r["aa_median"], 100 * r["aa_spread"],
                                                      "%.3f (%.1f%%)" % (r["vs_parent_median"], 100 * r["vs_parent_spread"]) if r["vs_parent"] else "not run"))
    L += [""] + notes + [""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x96,128x384")
    ap.add_argument("--nprobs", default="256,2048,16384")
    ap.add_argument("--base-nprob", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    ap.add_argument("--notes", default="", help="a text file whose lines are appended to the --md file")
    ap.add_argument("--compare-bits", default="", help="with --parent-lib: only compare the shared entry's bits of the two builds on the "
                    "cases of tests/small_batch_util.py, write the outcome to this file and exit (1 when a problem differs)")
    ap.add_argument("--render", default="", help="no measurement: write --md from the rows of this JSON file (an earlier --out)")
    a = ap.parse_args()
    notes = open(a.notes).read().splitlines() if a.notes else []
    if a.render:
        write_md(a.md, json.load(open(a.render)), notes)
        return
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    parent = other_build(a.parent_lib) if a.parent_lib else None
    if a.compare_bits:
        if not parent:
            raise SystemExit("--compare-bits needs --parent-lib")
        lines, ok = compare_bits(parent)
        with open(a.compare_bits, "w") as f:
            f.write("\n".join(lines + ["every problem bit-identical" if ok else "NOT bit-identical"]) + "\n")
        print("\n".join(lines))
        raise SystemExit(0 if ok else 1)
    rows = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        rows += measure(lib, n, m, [int(v) for v in a.nprobs.split(",")], a.base_nprob, a.rounds, a.eps, a.seed, parent)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        if a.md:
            write_md(a.md, rows, notes)


if __name__ == "__main__":
    main()
