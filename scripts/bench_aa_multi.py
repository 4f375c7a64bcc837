"""A block of Anderson accelerations (scs_amd_aa_multi_*), one GPU: what one apply of K columns costs per column against the
single-vector device path on the same data.

For every dim of --dims and every K of --ks: the block apply scs_amd_aa_multi_apply_dev on device buffers in the block layout,
against the single-vector path aa_dev_apply, reached through the same entry with nrhs == 1 (which is that path bit for bit, on a
device pointer, with nothing staged).  Lookback --lookback, type I, the reference's default regularisation.  The iterates are a
trajectory of the contraction of tests/test_aa_dev_gpu.py computed once on the host; column k of a block is that trajectory scaled
by 1 + k / 64 (the algorithm is scale-equivariant and the columns are independent, so every column does the work of the single
run).  Both sides first take lookback + 2 applies (seed, fill, first full solves: not timed), then --reps applies with a full
memory are timed one by one, with HIP events on the null stream around the call and with the wall clock; the uploads of the next
pair of blocks are outside both.  Every apply returns with its stream idle, so the two clocks see the same interval.
One JSON line per (dim, K): medians, time per column, its ratio to the single-vector apply, host synchronisations and kernel
launches per apply.  --lib-dir measures a library built elsewhere (an A/B against another commit's build, one process per
library).  No pass mark: it reports."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scs_amd import capi  # noqa: E402


class Hip:
    """device buffers and events through the HIP runtime the library already links"""

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
        self.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.rt.hipEventSynchronize.argtypes = [C.c_void_p]
        self.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.rt.hipEventDestroy.argtypes = [C.c_void_p]

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0 and p.value
        return p.value

    def put(self, dptr, arr):
        assert self.rt.hipMemcpy(dptr, arr.ctypes.data, arr.nbytes, 1) == 0

    def free(self, dptr):
        assert self.rt.hipFree(dptr) == 0

    def sync(self):
        assert self.rt.hipDeviceSynchronize() == 0

    def event(self):
        e = C.c_void_p()
        assert self.rt.hipEventCreate(C.byref(e)) == 0
        return e

    def record(self, e):
        assert self.rt.hipEventRecord(e, None) == 0

    def elapsed_ms(self, a, b):
        assert self.rt.hipEventSynchronize(b) == 0
        ms = C.c_float()
        assert self.rt.hipEventElapsedTime(C.byref(ms), a, b) == 0
        return ms.value


def trajectory(dim, n, seed=7):
    """x_0 = 0, x_{i+1} = F(x_i) of the contraction of tests/test_aa_dev_gpu.py: n + 1 iterates"""
    rng = np.random.default_rng(seed)
    d0 = rng.uniform(0.3, 0.95, dim)
    d1 = rng.uniform(-0.02, 0.02, dim)
    c = rng.standard_normal(dim)
    xs = [np.zeros(dim)]
    for _ in range(n):
        v = xs[-1]
        xs.append(d0 * v + d1 * np.roll(v, 1) + c + 0.03 * np.maximum(v, 0))
    return xs


def run(lib, hip, T, dim, K, mem, xs, reps):
    """warm, then time `reps` applies with a full memory.  Returns (event ms, wall ms, syncs per apply, launches per apply)."""
    W = lib.scs_amd_aa_multi_width(K)
    sf = np.dtype(T.np_float).itemsize
    a = lib.scs_amd_aa_multi_init(dim, K, mem, mem, 1, 1e-8, 1.0, 1.0, 1e10, 5)
    assert a, "scs_amd_aa_multi_init failed"
    dF, dX = hip.malloc(dim * W * sf), hip.malloc(dim * W * sf)
    scale = (1.0 + np.arange(W) / 64.0).astype(T.np_float)
    nrm = np.zeros(K, dtype=T.np_float)
    e0, e1 = hip.event(), hip.event()
    cnt = (C.c_longlong * 4)()
    ev, wall, syncs, launches = [], [], [], []
    try:
        for i in range(mem + 2 + reps):
            hip.put(dX, np.ascontiguousarray(xs[i][:, None].astype(T.np_float) * scale[None, :]))
            hip.put(dF, np.ascontiguousarray(xs[i + 1][:, None].astype(T.np_float) * scale[None, :]))
            hip.sync()
            lib.scs_amd_aa_multi_get_counters(a, C.byref(cnt))
            c0 = list(cnt)
            hip.record(e0)
            t0 = time.perf_counter()
            rc = lib.scs_amd_aa_multi_apply_dev(a, dF, dX, None, nrm.ctypes.data_as(T.fp))
            t1 = time.perf_counter()
            hip.record(e1)
            assert rc == 0
            if i >= mem + 2:
                assert (nrm > 0).all(), f"apply {i}: a column did not solve ({nrm})"
                lib.scs_amd_aa_multi_get_counters(a, C.byref(cnt))
                ev.append(hip.elapsed_ms(e0, e1))
                wall.append(1e3 * (t1 - t0))
                syncs.append(cnt[1] - c0[1])
                launches.append(cnt[3] - c0[3])
    finally:
        lib.scs_amd_aa_multi_finish(a)
        hip.free(dF)
        hip.free(dX)
        hip.rt.hipEventDestroy(e0)
        hip.rt.hipEventDestroy(e1)
    return ev, wall, max(syncs), max(launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="600001,3000001")
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--lookback", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default="libscsamd.so")
    ap.add_argument("--lib-dir", default=None, help="load --lib from this directory instead of scs_amd/lib (another build of it)")
    a = ap.parse_args()
    if a.lib_dir:
        capi.LIB_DIR = os.path.abspath(a.lib_dir)
    lib = capi.load(a.lib)
    if lib.scs_amd_device_count() <= 0:
        sys.exit("bench_aa_multi: no GPU (a measurement path does not fall back)")
    T = lib._scs_types
    hip = Hip()
    for dim in [int(v) for v in a.dims.split(",")]:
        xs = trajectory(dim, a.lookback + 2 + a.reps)
        run(lib, hip, T, dim, 1, a.lookback, xs, 2)  # warm: context, streams, code objects
        es, ws, _, _ = run(lib, hip, T, dim, 1, a.lookback, xs, a.reps)
        single_ev, single_wall = float(np.median(es)), float(np.median(ws))
        print(json.dumps(dict(dim=dim, K=1, width=1, lookback=a.lookback, reps=a.reps, lib=a.lib, apply_ms=round(single_ev, 4),
                              apply_wall_ms=round(single_wall, 4), spread=round((max(es) - min(es)) / single_ev, 4))), flush=True)
        for K in [int(v) for v in a.ks.split(",")]:
            eb, wb, syncs, launches = run(lib, hip, T, dim, K, a.lookback, xs, a.reps)
            em, wm = float(np.median(eb)), float(np.median(wb))
            print(json.dumps(dict(dim=dim, K=K, width=lib.scs_amd_aa_multi_width(K), lookback=a.lookback, reps=a.reps, lib=a.lib,
                                  apply_ms=round(em, 4), apply_wall_ms=round(wm, 4), per_column_ms=round(em / K, 4),
                                  single_ms=round(single_ev, 4), per_column_over_single=round(em / K / single_ev, 4),
                                  wall_per_column_over_single=round(wm / K / single_wall, 4),
                                  spread=round((max(eb) - min(eb)) / em, 4), syncs_per_apply=int(syncs),
                                  launches_per_apply=int(launches))), flush=True)


if __name__ == "__main__":
    main()
