"""scs_amd_family_set_values / scs_amd_solve_family_values on one GPU: what a family with its own values of A per problem costs.

The shape is that of scripts/bench_family_scaled.py (n x 2n second-order cone program, --col-nnz entries per column, fp64,
acceleration_lookback = 0).  Column k has the values A.data * (1 + 0.3 u_k), u_k uniform in (-1, 1), and data (b_k, c_k) by the
generator's law on its own A_k.  For every K of --ks, each measurement with its sides alternated --pairs times in one process after
one warm-up of each, wall time by a host clock around calls that return with the stream idle, medians reported:
 (s) the set call alone;
 (a) to termination, adaptive_scale = 1: one solve call (after one set call) against the loop
     scs_amd_update_matrix + scs_update + scs_solve over the same K problems on one workspace; every column is given the scale of
     scs_init as its starting scale, which is where scs_amd_update_matrix puts the loop's solves (with scales = NULL the columns
     would start from the scale the last single solve on the workspace adapted to, and the two sides would not do the same work);
 (b) per iteration, adaptive_scale = 0, every solve capped at --cap-iters: the solve call against scs_amd_solve_family_scaled on the
     workspace's shared values -- the cost of the value blocks, D / E blocks and per-column bounds alone.
With --parent-lib (a libscsamd.so built from the parent commit):
 (c) scs_amd_solve_family_scaled of that build against this build's, capped at --cap-iters, alternated parent / this / this so that
     the second and third give the A/A spread of the same run.
One JSON line per measurement.  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402
from scripts.bench_family import family_data  # noqa: E402
from scripts.bench_family_scaled import family_scaled, work  # noqa: E402


def set_values(lib, w, AX):
    t0 = time.perf_counter()
    rc = capi.family_set_values(lib, w, AX)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt


def family_values(lib, w, B, Cc, scales=None):
    t0 = time.perf_counter()
    rc, out = capi.solve_family_values(lib, w, B, Cc, scales=scales)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt, [r["info"]["iter"] for r in out], [r["info"]["status_val"] for r in out], [r["info"]["scale_updates"] for r in out]


def update_loop(lib, w, prob, AX, B, Cc):
    """scs_amd_update_matrix + scs_update + scs_solve, problem after problem; the time of the updates alone is returned too"""
    T = lib._scs_types
    x, y, s = np.zeros(prob.n), np.zeros(prob.m), np.zeros(prob.m)
    sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
    info = T.ScsInfo()
    its, st, t_upd = [], [], 0.0
    t0 = time.perf_counter()
    for k in range(B.shape[1]):
        ax, b, c = (np.ascontiguousarray(v[:, k]) for v in (AX, B, Cc))
        t1 = time.perf_counter()
        assert lib.scs_amd_update_matrix(w, ax.ctypes.data_as(T.fp), None) == 0
        t_upd += time.perf_counter() - t1
        assert lib.scs_update(w, b.ctypes.data_as(T.fp), c.ctypes.data_as(T.fp)) == 0
        lib.scs_solve(w, C.byref(sol), C.byref(info), 0)
        its.append(int(info.iter))
        st.append(int(info.status_val))
    return time.perf_counter() - t0, its, st, t_upd


def parent_library(path):
    """the few entries measurement (c) calls, bound on a library that lacks this change's names"""
    lib = C.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    T = capi.T64
    lib._scs_types = T
    lib.scs_set_default_settings.restype = None
    lib.scs_set_default_settings.argtypes = [C.POINTER(T.ScsSettings)]
    lib.scs_init.restype = C.c_void_p
    lib.scs_init.argtypes = [C.POINTER(T.ScsData), C.POINTER(T.ScsCone), C.POINTER(T.ScsSettings)]
    lib.scs_finish.restype = None
    lib.scs_finish.argtypes = [C.c_void_p]
    lib.scs_amd_solve_family_scaled.restype = T.scs_int
    lib.scs_amd_solve_family_scaled.argtypes = [C.c_void_p, T.scs_int, T.fp, T.scs_int, T.fp, T.scs_int, T.fp, C.POINTER(T.ScsSolution),
                                                C.POINTER(T.ScsInfo), T.scs_int]
    return lib


def measure_a(lib, prob, a, K, AXk, Bk, Ck, emit):
    scales = np.full(K, capi.default_settings(lib).scale)  # where scs_amd_update_matrix puts every solve of the loop
    w = work(lib, prob, adaptive_scale=1, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.max_iters)
    try:
        set_values(lib, w, AXk)
        fam = family_values(lib, w, Bk, Ck, scales)
        update_loop(lib, w, prob, AXk[:, :1], Bk[:, :1], Ck[:, :1])
        t_set, t_fam, t_loop, t_upd = [], [], [], []
        for _ in range(a.pairs):
            t_set.append(set_values(lib, w, AXk))
            fam = family_values(lib, w, Bk, Ck, scales)
            one = update_loop(lib, w, prob, AXk, Bk, Ck)
            t_fam.append(fam[0])
            t_loop.append(one[0])
            t_upd.append(one[3])
    finally:
        lib.scs_finish(w)
    emit(dict(measurement="set_call", K=K, pairs=a.pairs, set_s=t_set, set_median_s=med(t_set), per_column_ms=1e3 * med(t_set) / K,
              loop_updates_s=t_upd, loop_update_per_problem_ms=1e3 * med(t_upd) / K))
    r_solve = [x / y for x, y in zip(t_fam, t_loop)]
    r_total = [(x + s_) / y for x, s_, y in zip(t_fam, t_set, t_loop)]
    emit(dict(measurement="to_termination", K=K, pairs=a.pairs, values_s=t_fam, loop_s=t_loop, values_median_s=med(t_fam),
              loop_median_s=med(t_loop), ratio_solve=med(r_solve), ratio_solve_min=min(r_solve), ratio_solve_max=max(r_solve),
              ratio_set_plus_solve=med(r_total), ratio_set_plus_solve_min=min(r_total), ratio_set_plus_solve_max=max(r_total),
              iters_values=fam[1], iters_loop=one[1], status_values=fam[2], status_loop=one[2], scale_updates_values=fam[3]))


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--ks", default="8,16")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--cap-iters", type=int, default=100, help="iterations of every solve of measurements (b) and (c)")
    ap.add_argument("--max-iters", type=int, default=100000, help="cap of measurement (a)")
    ap.add_argument("--parent-lib", default="", help="libscsamd.so of the parent commit: measurement (c)")
    ap.add_argument("--only", default="sabc", help="the measurements to take: letters of s, a, b, c (s and a are taken together, and so are b and c)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = capi.load("libscsamd.so")
    if lib.scs_amd_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    Ks = [int(v) for v in a.ks.split(",")]
    pr = problems.random_socp(a.n, 2 * a.n, a.col_nnz, seed=a.seed)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    rng = np.random.default_rng(a.seed + 2)
    Kmax = max(Ks)
    AX = np.asfortranarray(prob.Ax[:, None] * (1.0 + 0.3 * rng.uniform(-1, 1, (len(prob.Ax), Kmax))))
    B, Cc = np.zeros((prob.m, Kmax), order="F"), np.zeros((prob.n, Kmax), order="F")
    for k in range(Kmax):  # column k by the generator's law on its own A_k
        Ak = sp.csc_matrix((AX[:, k], prob.Ai, prob.Ap), shape=(prob.m, prob.n))
        Bk, Ck = family_data(Ak, pr["cone"], 1, a.seed + 10 + k)
        B[:, k], Cc[:, k] = Bk[:, 0], Ck[:, 0]
    Bs, Cs = family_data(pr["A"], pr["cone"], Kmax, a.seed + 1)  # data on the shared A, for (b) and (c)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for K in Ks:
        AXk, Bk, Ck = np.asfortranarray(AX[:, :K]), np.asfortranarray(B[:, :K]), np.asfortranarray(Cc[:, :K])
        # (s) and (a): adaptive, to termination
        if "a" in a.only or "s" in a.only:
            measure_a(lib, prob, a, K, AXk, Bk, Ck, emit)
        if "b" not in a.only and "c" not in a.only:
            continue
        # (b): the same iterations on both sides, shared values against own values
        Bsk, Csk = np.asfortranarray(Bs[:, :K]), np.asfortranarray(Cs[:, :K])
        own = np.asfortranarray(np.tile(prob.Ax[:, None], (1, K)))  # the workspace's values in every column: the same arithmetic
        w = work(lib, prob, adaptive_scale=0, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.cap_iters)
        try:
            set_values(lib, w, own)
            family_scaled(lib, w, Bsk, Csk)
            family_values(lib, w, Bsk, Csk)
            t_old, t_new = [], []
            for _ in range(a.pairs):
                t_old.append(family_scaled(lib, w, Bsk, Csk)[0])
                t_new.append(family_values(lib, w, Bsk, Csk)[0])
        finally:
            lib.scs_finish(w)
        r = [x / y for x, y in zip(t_new, t_old)]
        emit(dict(measurement="per_iteration", K=K, iters=a.cap_iters, pairs=a.pairs, scaled_s=t_old, values_s=t_new,
                  scaled_ms_per_iter=1e3 * med(t_old) / a.cap_iters, values_ms_per_iter=1e3 * med(t_new) / a.cap_iters, ratio=med(r),
                  ratio_min=min(r), ratio_max=max(r)))
        # (c): shared-value callers pay nothing -- the parent's scaled entry against this build's, with the A/A spread of the run
        if a.parent_lib:
            par = parent_library(a.parent_lib)
            wp = work(par, prob, adaptive_scale=0, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.cap_iters)
            w = work(lib, prob, adaptive_scale=0, eps_abs=a.eps, eps_rel=a.eps, max_iters=a.cap_iters)
            try:
                family_scaled(par, wp, Bsk, Csk)
                family_scaled(lib, w, Bsk, Csk)
                t_par, t_a, t_b = [], [], []
                for _ in range(a.pairs):
                    t_par.append(family_scaled(par, wp, Bsk, Csk)[0])
                    t_a.append(family_scaled(lib, w, Bsk, Csk)[0])
                    t_b.append(family_scaled(lib, w, Bsk, Csk)[0])
            finally:
                par.scs_finish(wp)
                lib.scs_finish(w)
            r = [x / y for x, y in zip(t_a, t_par)]
            aa = [x / y for x, y in zip(t_b, t_a)]
            emit(dict(measurement="scaled_entry_this_vs_parent", K=K, iters=a.cap_iters, pairs=a.pairs, parent_s=t_par, this_s=t_a,
                      this_again_s=t_b, ratio_this_over_parent=med(r), ratio_min=min(r), ratio_max=max(r), aa_ratio=med(aa),
                      aa_min=min(aa), aa_max=max(aa)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(n=a.n, m=2 * a.n, col_nnz=a.col_nnz, eps=a.eps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
