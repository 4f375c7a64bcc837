"""Blocks of vectors on the cone projection (B1'), one GPU: what K interleaved vectors cost against K single-vector calls.

On three cones -- the headline one (m = 2e6: zero, nonnegative, the large second-order cones of problems.socp_cone_sizes), the
configs[3] size (m = 4e5, same recipe) and the configs[2] cone (200 PSD blocks of 50 x 50 + box 1001) -- and for every K of --ks:
the block projection scs_amd_cone_proj_dual_multi_dev, --calls calls between two device synchronisations after a warm-up, against
scs_amd_cone_proj_dual_dev (the single-vector ConeDev::proj_dual, unchanged) on a workspace of the same cone in the same process,
the two alternated --reps times.  The projection works in place and a projected vector is a fixed point, so a run that called it
over and over on one buffer would time the do-nothing branches after the first call: every call of a run gets its own buffer,
filled from one pristine input by device-to-device copies before the clock starts.  (The carried state then sees the same input
at every call: the PSD cone is timed warm started from an exact eigenbasis, as late ADMM iterations are.)
One JSON line per (cone, K): time per block projection, time per column, its ratio to the single-vector projection of the SAME run
and the spread over the repeats.  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi, problems  # noqa: E402


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

    def copy(self, dst, src, nbytes):  # device to device, synchronous with respect to the host
        assert self.rt.hipMemcpy(dst, src, nbytes, 3) == 0

    def free(self, dptr):
        assert self.rt.hipFree(dptr) == 0

    def sync(self):
        assert self.rt.hipDeviceSynchronize() == 0


def cones_of(names):
    out = []
    for nm in names:
        if nm == "headline":
            out.append((nm, problems.socp_cone_sizes(2000000)))
        elif nm == "configs3":
            out.append((nm, problems.socp_cone_sizes(400000)))
        elif nm == "configs2":
            out.append((nm, dict(bu=np.ones(1000), bl=-np.ones(1000), s=[50] * 200)))
        else:
            sys.exit(f"bench_cones_multi: unknown cone {nm}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cones", default="headline,configs3,configs2")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--lib", default="libscsamd.so")
    a = ap.parse_args()
    lib = capi.load(a.lib)
    if lib.scs_amd_device_count() <= 0:
        sys.exit("bench_cones_multi: no GPU (a measurement path does not fall back)")
    T = lib._scs_types
    sf = np.dtype(T.np_float).itemsize
    hip = Hip()
    for name, cone in cones_of(a.cones.split(",")):
        m = capi.cone_rows(cone)
        rng = np.random.default_rng(0)
        k = capi.make_cone(cone, T)
        ws, wb = lib.scs_amd_cone_init(C.byref(k), m, None), lib.scs_amd_cone_init(C.byref(k), m, None)
        assert ws and wb
        sync = lambda: (hip.sync(), lib.scs_amd_cone_sync(ws), lib.scs_amd_cone_sync(wb))
        r = hip.malloc(m * sf)
        hip.put(r, rng.uniform(0.5, 2.0, m).astype(T.np_float))
        x0 = hip.malloc(m * sf)
        hip.put(x0, rng.standard_normal(m).astype(T.np_float))
        xs = [hip.malloc(m * sf) for _ in range(a.calls)]

        def timed(fn, bufs, src, nbytes):
            for b in bufs:  # every call of the run projects a fresh copy of the same input (see the module comment); not timed
                hip.copy(b, src, nbytes)
            sync()
            t0 = time.perf_counter()
            for b in bufs:
                assert fn(b) == 0
            sync()
            return (time.perf_counter() - t0) / len(bufs)

        single_fn = lambda b: lib.scs_amd_cone_proj_dual_dev(ws, b, r)
        for K in [int(v) for v in a.ks.split(",")]:
            W = lib.scs_amd_cone_multi_width(K)
            b0 = hip.malloc(m * W * sf)
            hip.put(b0, rng.standard_normal(m * W).astype(T.np_float))
            bs = [hip.malloc(m * W * sf) for _ in range(a.calls)]
            block_fn = lambda b: lib.scs_amd_cone_proj_dual_multi_dev(wb, K, b, r)
            timed(block_fn, bs[:3], b0, m * W * sf)  # warm-up of both (allocates the block state of this width)
            timed(single_fn, xs[:3], x0, m * sf)
            tb, ts = [], []
            for _ in range(a.reps):  # alternated
                tb.append(timed(block_fn, bs, b0, m * W * sf))
                ts.append(timed(single_fn, xs, x0, m * sf))
            for b in bs + [b0]:
                hip.free(b)
            tbm, tsm = float(np.median(tb)), float(np.median(ts))
            rec = dict(cone=name, K=K, width=W, m=m, calls=a.calls, reps=a.reps, lib=a.lib,
                       block_us=round(1e6 * tbm, 2), per_column_us=round(1e6 * tbm / K, 2), single_us=round(1e6 * tsm, 2),
                       per_column_over_single=round(tbm / K / tsm, 4),
                       block_spread=round((max(tb) - min(tb)) / tbm, 4), single_spread=round((max(ts) - min(ts)) / tsm, 4))
            print(json.dumps(rec), flush=True)
        for p in [r, x0] + xs:
            hip.free(p)
        lib.scs_amd_cone_finish(ws)
        lib.scs_amd_cone_finish(wb)


if __name__ == "__main__":
    main()
