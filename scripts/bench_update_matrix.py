"""New matrix values on a live workspace, one GPU: what scs_amd_update_matrix costs against the only way there was before it,
scs_finish + scs_init on the same values.

At every size of --ns (default: the headline problem n = 1e6, m = 2n, 10 entries per column, and n = 2e5), fp64, in one process: a
workspace is created on A0; then the two forms are alternated --pairs times (default 5) after one warm-up of each -- (i)
scs_amd_update_matrix(w, A1 values) on the live workspace, (ii) scs_finish(w); w = scs_init(A1) -- with the values flipping between
two sets so that every call has work to do.  Wall time is a host clock around calls that return with the stream idle.  With
--debug-phases one more call of each form runs with the `debug` option set, and the phase lines the library prints on stderr
([scs_amd init] / [scs_amd update] / [scs_amd linsys init]) are captured into the record: where the time goes.
One JSON line per size: every sample, medians, min / max of both forms, the ratio of the medians, and whether the workspace was
renumbered (scs_amd_get_reorder_info) and which SpMV kernels it runs.  No pass mark: it reports.  --out writes the records as a
JSON list (profiles/update_matrix.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402


def capture_stderr(fn):
    """run fn() with file descriptor 2 redirected into a file; returns (result, text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return res, tmp.read().decode(errors="replace")


def run_size(lib, n, col_nnz, seed, pairs, debug_phases):
    T = lib._scs_types
    pr = problems.random_socp(n, 2 * n, col_nnz, seed=seed)
    rng = np.random.default_rng(seed + 1)
    vals = [np.ascontiguousarray(pr["A"].data, dtype=np.float64),
            np.ascontiguousarray(pr["A"].data * (1.0 + 0.3 * rng.uniform(-1, 1, pr["A"].nnz)), dtype=np.float64)]
    probs = []
    for v in vals:
        A = pr["A"].copy()
        A.data = v.copy()
        probs.append(capi.Problem(A, pr["b"], pr["c"], pr["cone"]))
    st = capi.default_settings(lib, verbose=0)

    def init(k):
        w = lib.scs_init(C.byref(probs[k].data), C.byref(probs[k].k), C.byref(st))
        assert w, "scs_init returned NULL"
        return w

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def update(w, k):
        assert lib.scs_amd_update_matrix(w, vals[k].ctypes.data_as(T.fp), None) == 0

    w = init(0)
    info = (C.c_double * 6)()
    lib.scs_amd_get_reorder_info(w, info)
    names = []
    for which in (0, 1):
        buf = C.create_string_buffer(128)
        lib.scs_amd_get_spmv_kernel_name(w, which, buf, 128)
        names.append(buf.value.decode())
    # warm-up of each form (the first update also builds the position maps: reported on its own)
    t_first_update, _ = timed(lambda: update(w, 1))
    lib.scs_finish(w)
    w = init(0)
    update(w, 1)
    cur = 1
    t_upd, t_re = [], []
    for _ in range(pairs):
        cur ^= 1
        t, _ = timed(lambda: update(w, cur))
        t_upd.append(t)
        cur ^= 1

        def reinit():
            lib.scs_finish(w)
            return init(cur)
        t, w = timed(reinit)
        t_re.append(t)
        update(w, cur)  # the maps of the new workspace: built outside the timed calls, as on the long-lived workspace of form (i)
    rec = dict(n=n, m=2 * n, nnz=int(pr["A"].nnz), dtype="f64", pairs=pairs, renumbered=bool(info[0]), reorder_seconds=info[5],
               spmv_kernels=names, first_update_s=t_first_update,
               update_s=t_upd, reinit_s=t_re, update_median_s=statistics.median(t_upd), reinit_median_s=statistics.median(t_re),
               update_min_max_s=[min(t_upd), max(t_upd)], reinit_min_max_s=[min(t_re), max(t_re)])
    rec["reinit_over_update"] = rec["reinit_median_s"] / rec["update_median_s"]
    if debug_phases:
        capi.set_option("debug", "1", libs=[lib])
        try:
            cur ^= 1
            _, txt_u = capture_stderr(lambda: update(w, cur))
            lib.scs_finish(w)
            w, txt_i = capture_stderr(lambda: init(cur))
        finally:
            capi.set_option("debug", None, libs=[lib])
        keep = lambda txt: [ln.strip() for ln in txt.splitlines() if ln.startswith("[scs_amd")]
        rec["debug_phases"] = dict(update=keep(txt_u), reinit=keep(txt_i))
    lib.scs_finish(w)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[1000000, 200000])
    ap.add_argument("--col-nnz", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--debug-phases", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = capi.load("libscsamd.so")
    recs = []
    for n in args.ns:
        rec = run_size(lib, n, args.col_nnz, args.seed, args.pairs, args.debug_phases)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
