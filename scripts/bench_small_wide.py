"""The WIDE instantiation of the small batch (1024 threads, one workgroup per CU: n over 128 or n + m + 1 over 1024), one GPU: what
scs_amd_small_solve costs at those sizes against what the library offered for them before, what own values cost there, and whether
the NARROW instantiation kept its time.

Workload: random_socp-law problems (scs_amd/problems.py) at the shapes of --shapes, a shared A and --nprobs problems (b_k, c_k)
drawn by the generator's law, fp64, eps 1e-4, adaptive_scale = 0, acceleration_lookback = 0, to termination.  Parts:
  sizes   SmallBatch.solve on every list against `loop` (scs_update + scs_solve problem after problem on one workspace) and `stream`
          (solve_family_stream at width 16), both on the first --base-nprob problems of the list: scripts/bench_small_batch.py's
          sides, alternated --rounds times after one warm-up of each.  Per size: one problem alone, the instantiation that ran and
          its LDS, and the wall time of the object's construction (the host's factor of H in long double is inside it).
  own     at --own-shape, --own-nprob problems whose values are the shared A tiled: the values entry against the shared entry of
          the same object, and both at max_iters = 1 on an object of their own -- the difference is the per-problem factor.
  narrow  with --parent-lib (a libscsamd.so built from the parent commit): the shared entry at --narrow-shape, --narrow-nprob
          problems, this build against the parent's in alternated pairs beside an A/A pair of two objects of this build.
Wall time is a host clock around calls that return with the stream idle.  Writes --out (JSON) and, with --md, the tables of
profiles/small_wide.md; --render JSON writes --md from an earlier --out (with --notes appended) without a GPU.  No pass mark: it
reports."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402
from scs_amd.small import SmallBatch  # noqa: E402
from scripts.bench_small_batch import Loop, clock, family, med, spread  # noqa: E402
from scripts.bench_small_values import other_build  # noqa: E402

KW = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)


def its(out):
    return sum(r["info"]["iter"] for r in out)


def setup(n, m, K, eps, seed):
    pr = problems.random_socp(n, m, min(10, m), seed=seed)
    B, Cc = family(pr["A"], pr["cone"], K, seed + 1)
    return pr, B, Cc, dict(KW, eps_abs=eps, eps_rel=eps)


def measure_size(lib, n, m, nprobs, base_nprob, rounds, eps, seed):
    pr, B, Cc, kw = setup(n, m, max(nprobs), eps, seed)
    A, cone = pr["A"], pr["cone"]
    t_init, sb = clock(lambda: SmallBatch(dict(A=A, b=pr["b"], c=pr["c"]), cone, **kw))
    base = Loop(lib, capi.Problem(A, pr["b"], pr["c"], cone), capi.default_settings(lib, **kw))
    rows = []
    try:
        Kb = min(base_nprob, max(nprobs))
        sb.solve(B[:, :min(nprobs)], Cc[:, :min(nprobs)])  # warm-up of the three sides
        base.run(B[:, :4], Cc[:, :4])
        base.stream(B[:, :16], Cc[:, :16])
        occ = sb.occupancy()
        t1, out1 = clock(sb.solve, B[:, 0], Cc[:, 0])
        per = {K: [] for K in nprobs}
        tl, ts = [], []
        for _ in range(rounds):
            for K in nprobs:
                t, out = clock(sb.solve, B[:, :K], Cc[:, :K])
                per[K].append((t, its(out), max(r["info"]["iter"] for r in out)))
            tl.append(clock(base.run, B[:, :Kb], Cc[:, :Kb]))
            ts.append(clock(base.stream, B[:, :Kb], Cc[:, :Kb]))
            print(f"round done: n={n} small {[round(per[K][-1][0], 4) for K in nprobs]} loop {tl[-1][0]:.2f} stream {ts[-1][0]:.2f}",
                  file=sys.stderr, flush=True)
        loop_rate, stream_rate = [Kb / t for t, _ in tl], [Kb / t for t, _ in ts]
        on_base = its(sb.solve(B[:, :Kb], Cc[:, :Kb]))
        for K in nprobs:
            t = [v[0] for v in per[K]]
            row = dict(part="sizes", n=n, m=m, nprob=K, rounds=rounds, eps=eps, small_s=t, small_s_median=med(t), small_spread=spread(t),
                       small_rate=K / med(t), small_iters=per[K][0][1], small_iters_max=per[K][0][2],
                       one_problem_us_per_iteration=1e6 * t1 / max(its(out1), 1), one_problem_iters=its(out1), base_nprob=Kb,
                       loop_s=[v[0] for v in tl], loop_rate=med(loop_rate), loop_spread=spread(loop_rate), loop_iters=tl[0][1],
                       stream_s=[v[0] for v in ts], stream_rate=med(stream_rate), stream_spread=spread(stream_rate), stream_iters=ts[0][1],
                       small_iters_on_base=on_base, vs_loop=[(K / a) / b for a, b in zip(t, loop_rate)],
                       vs_stream=[(K / a) / b for a, b in zip(t, stream_rate)], init_python_s=t_init, occupancy=occ)
            for k in ("vs_loop", "vs_stream"):
                row[k + "_median"], row[k + "_min"] = med(row[k]), min(row[k])
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        base.close()
        sb.close()
    return rows


def measure_own(n, m, K, rounds, eps, seed):
    pr, B, Cc, kw = setup(n, m, K, eps, seed)
    A, cone = pr["A"], pr["cone"]
    data = dict(A=A, b=pr["b"], c=pr["c"])
    AX = np.asfortranarray(np.repeat(capi.Problem(A, pr["b"], pr["c"], cone).Ax[:, None], K, axis=1))
    sb, sb1 = SmallBatch(data, cone, **kw), SmallBatch(data, cone, **dict(kw, max_iters=1))
    try:
        t_set = clock(sb.set_values, AX)[0]
        sb1.set_values(AX)
        for o in (sb, sb1):  # warm-up: the device side and both kernels of every object
            o.solve(B, Cc)
            o.solve(B, Cc, own_values=True)
        d = dict(values=[], shared=[], f_own=[], f_sh=[])
        for _ in range(rounds):
            t, out = clock(lambda: sb.solve(B, Cc, own_values=True))
            d["values"].append(t)
            iv = its(out)
            t, out = clock(sb.solve, B, Cc)
            d["shared"].append(t)
            ish = its(out)
            d["f_own"].append(clock(lambda: sb1.solve(B, Cc, own_values=True))[0])
            d["f_sh"].append(clock(sb1.solve, B, Cc)[0])
            print(f"own round done: values {d['values'][-1]:.3f} shared {d['shared'][-1]:.3f} factor {d['f_own'][-1] - d['f_sh'][-1]:.3f}",
                  file=sys.stderr, flush=True)
        fac = [a - b for a, b in zip(d["f_own"], d["f_sh"])]
        ratio = [a / b for a, b in zip(d["values"], d["shared"])]
        row = dict(part="own", n=n, m=m, nprob=K, rounds=rounds, eps=eps, values_s=d["values"], values_s_median=med(d["values"]),
                   values_spread=spread(d["values"]), shared_s=d["shared"], shared_s_median=med(d["shared"]), shared_spread=spread(d["shared"]),
                   values_over_shared=ratio, values_over_shared_median=med(ratio), values_over_shared_spread=spread(ratio),
                   iters_values=iv, iters_shared=ish, set_s=t_set, factor_s=fac, factor_s_median=med(fac),
                   factor_share=med(fac) / med(d["values"]), factor_share_min=min(fac) / med(d["values"]),
                   factor_share_max=max(fac) / med(d["values"]), workgroups=min(K, sb.occupancy()["default_grid"]), occupancy=sb.occupancy())
        print(json.dumps(row), flush=True)
        return [row]
    finally:
        sb.close()
        sb1.close()


def measure_narrow(parent, n, m, K, rounds, eps, seed):
    pr, B, Cc, kw = setup(n, m, K, eps, seed)
    data = dict(A=pr["A"], b=pr["b"], c=pr["c"])
    a, b, p = SmallBatch(data, pr["cone"], **kw), SmallBatch(data, pr["cone"], **kw), parent(data, pr["cone"], **kw)
    try:
        assert p._lib is not a._lib
        outs = [o.solve(B, Cc) for o in (a, b, p)]  # warm-up
        same = sum(all(np.array_equal(x[v], y[v], equal_nan=True) for v in ("x", "y", "s")) and x["info"]["iter"] == y["info"]["iter"]
                   for x, y in zip(outs[0], outs[2]))
        ta, tb, tp = [], [], []
        for _ in range(rounds):
            ta.append(clock(a.solve, B, Cc)[0])
            tb.append(clock(b.solve, B, Cc)[0])
            tp.append(clock(p.solve, B, Cc)[0])
        aa, vp = [x / y for x, y in zip(ta, tb)], [x / y for x, y in zip(ta, tp)]
        row = dict(part="narrow", n=n, m=m, nprob=K, rounds=rounds, eps=eps, this_s=ta, this_b_s=tb, parent_s=tp, this_s_median=med(ta),
                   parent_s_median=med(tp), aa=aa, aa_median=med(aa), aa_spread=spread(aa), vs_parent=vp, vs_parent_median=med(vp),
                   vs_parent_spread=spread(vp), bit_identical_problems=int(same), occupancy=a.occupancy())
        print(json.dumps(row), flush=True)
        return [row]
    finally:
        for o in (a, b, p):
            o.close()


def write_md(path, rows, notes):
    sizes = [r for r in rows if r["part"] == "sizes"]
    L = ["# The wide instantiation of the small batch: n up to 512, n + m + 1 up to 2304 (scs_amd_small_solve)", "",
         "Written by `scripts/bench_small_wide.py` on one MI355X; fp64, eps %g, adaptive_scale = 0, acceleration_lookback = 0, random_socp-law" % sizes[0]["eps"],
         "problems on a shared A, to termination.  Medians of %d alternated rounds (small at every list length, then loop, then stream);" % sizes[0]["rounds"],
         "spread = (max - min) / median over the rounds.  Wall time is a host clock around the call (staging, launch, read-back and the",
         "host's finalize included).  `loop` = scs_update + scs_solve per problem on one workspace; `stream` = solve_family_stream, width 16;",
         "both ran on the first %d problems of each list only, and their rate is what the lists are compared with.  The iteration counts" % sizes[0]["base_nprob"],
         "differ between the sides (exact against inexact linear solves): a ratio compares the time to the same tolerance, not equal work.", "",
         "| n | m | problems | small: s (spread) | small: problems/s | loop: problems/s (spread) | stream: problems/s (spread) | small / loop: median (smallest round) | small / stream: median (smallest round) |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in sizes:
        L.append("| %d | %d | %d | %.4f (%.0f%%) | %.1f | %.2f (%.0f%%) | %.2f (%.0f%%) | %.1fx (%.1fx) | %.1fx (%.1fx) |" % (
            r["n"], r["m"], r["nprob"], r["small_s_median"], 100 * r["small_spread"], r["small_rate"], r["loop_rate"], 100 * r["loop_spread"],
            r["stream_rate"], 100 * r["stream_spread"], r["vs_loop_median"], r["vs_loop_min"], r["vs_stream_median"], r["vs_stream_min"]))
    L += ["", "Iterations, summed over the problems each side ran:", "",
          "| n | m | problems | small: iterations (largest of one problem) | on the first %d: small | loop | stream |" % sizes[0]["base_nprob"],
          "|---|---|---|---|---|---|---|"]
    for r in sizes:
        L.append("| %d | %d | %d | %d (%d) | %d | %d | %d |" % (r["n"], r["m"], r["nprob"], r["small_iters"], r["small_iters_max"],
                                                         r["small_iters_on_base"], r["loop_iters"], r["stream_iters"]))
    L += ["", "Per size: one problem alone (wall / iterations, the staging and the read-back inside), the instantiation that ran, and the",
          "wall time of the object's construction (host: equilibration, H, its Cholesky factor and inverse in long double, the padded rows):", "",
          "| n | m | one problem alone: us per iteration (iterations) | instantiation | threads | workgroups per CU | LDS per workgroup (bytes) | default grid | construction (s) |",
          "|---|---|---|---|---|---|---|---|---|"]
    seen = set()
    for r in sizes:
        if (r["n"], r["m"]) in seen:
            continue
        seen.add((r["n"], r["m"]))
        o = r["occupancy"]
        L.append("| %d | %d | %.1f (%d) | %s | %d | %d | %d | %d | %.3f |" % (
            r["n"], r["m"], r["one_problem_us_per_iteration"], r["one_problem_iters"], o["kernel"], o["block_threads"], o["wg_per_cu"],
            o["lds_bytes"], o["default_grid"], r["init_python_s"]))
    for r in rows:
        if r["part"] == "own":
            L += ["", "Own values at (n, m) = (%d, %d), %d problems (%d workgroups), every problem's values the shared A tiled, so both entries run"
                  % (r["n"], r["m"], r["nprob"], r["workgroups"]),
                  "the same iterations (%d and %d); the factor is the values entry minus the shared entry, both at max_iters = 1, a DIFFERENCE of" % (r["iters_values"], r["iters_shared"]),
                  "two wall times:", "",
                  "| values: s (spread) | shared: s (spread) | values / shared time (spread) | set call: s | factor: s of wall for the list | factor's share of the values solve: median (smallest .. largest round) |",
                  "|---|---|---|---|---|---|",
                  "| %.3f (%.0f%%) | %.3f (%.0f%%) | %.2f (%.0f%%) | %.3f | %.3f | %.1f%% (%.1f%% .. %.1f%%) |" % (
                      r["values_s_median"], 100 * r["values_spread"], r["shared_s_median"], 100 * r["shared_spread"], r["values_over_shared_median"],
                      100 * r["values_over_shared_spread"], r["set_s"], r["factor_s_median"], 100 * r["factor_share"], 100 * r["factor_share_min"],
                      100 * r["factor_share_max"])]
        if r["part"] == "narrow":
            L += ["", "The narrow instantiation at (n, m) = (%d, %d), %d problems: this build against a second object of this build (A/A) and" % (r["n"], r["m"], r["nprob"]),
                  "against the parent commit's build, time ratios of %d alternated rounds; %d of %d problems bit-identical (x, y, s, iter) between" % (r["rounds"], r["bit_identical_problems"], r["nprob"]),
                  "the two builds:", "", "| this: s | parent: s | A/A: median (spread) | this / parent: median (spread) |", "|---|---|---|---|",
                  "| %.4f | %.4f | %.3f (%.1f%%) | %.3f (%.1f%%) |" % (r["this_s_median"], r["parent_s_median"], r["aa_median"], 100 * r["aa_spread"],
                                                               r["vs_parent_median"], 100 * r["vs_parent_spread"])]
    L += [""] + notes + [""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x768,512x1536")
    ap.add_argument("--nprobs", default="256,2048")
    ap.add_argument("--base-nprob", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--own-shape", default="512x1536")
    ap.add_argument("--own-nprob", type=int, default=256)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--narrow-shape", default="128x384")
    ap.add_argument("--narrow-nprob", type=int, default=2048)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    ap.add_argument("--notes", default="", help="a text file whose lines are appended to the --md file")
    ap.add_argument("--render", default="", help="no measurement: write --md from the rows of this JSON file (an earlier --out)")
    a = ap.parse_args()
    notes = open(a.notes).read().splitlines() if a.notes else []
    if a.render:
        write_md(a.md, json.load(open(a.render)), notes)
        return
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    rows = []

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        if a.md and any(r["part"] == "sizes" for r in rows):
            write_md(a.md, rows, notes)
    shape = lambda s: tuple(int(v) for v in s.split("x"))  # noqa: E731
    if a.parent_lib:
        rows += measure_narrow(other_build(a.parent_lib), *shape(a.narrow_shape), a.narrow_nprob, a.rounds, a.eps, a.seed)
        save()
    for s in [v for v in a.shapes.split(",") if v]:
        rows += measure_size(lib, *shape(s), [int(v) for v in a.nprobs.split(",")], a.base_nprob, a.rounds, a.eps, a.seed)
        save()
    if a.own_shape:
        rows += measure_own(*shape(a.own_shape), a.own_nprob, a.rounds, a.eps, a.seed)
        save()


if __name__ == "__main__":
    main()
