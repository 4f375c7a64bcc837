"""`Accel` -- a block of Anderson accelerations of the C ABI (include/scs_amd.h, scs_amd_aa_multi_*) as a Python object.

`ncols` independent accelerations of fixed-point iterates of length `dim` on the GPU: column k computes what the reference's
aa_apply / aa_safeguard / aa_reset (src/aa.c) compute for that column alone, with its own memory, counters and statistics, while
the kernels and the read-backs of the reflector sweep are shared by the columns (scs_amd/csrc/aa_multi.h).  One object lives for
the lifetime of the Python object (scs_amd_aa_multi_init once, scs_amd_aa_multi_finish on close / garbage collection).  Host code
only: every flop is in the library.

lookback       : memory of every column (the reference's acceleration_lookback); also the shortest memory that is solved with
type1          : type-I (True) or type-II (False) acceleration
regularization : > 0 scaled, < 0 pinned to its absolute value, 0 none
relaxation     : in [0, 2]
dtype          : "f64" (default) or "f32" (the SFLOAT library)
"""
import ctypes as C

import numpy as np

from . import capi

SAFEGUARD_FACTOR = 1.0   # the values scs_init hands to aa_init (reference src/scs.c)
MAX_WEIGHT_NORM = 1e10
IR_MAX_STEPS = 5


def check_block(dim, ncols, A, name="F"):
    """Shape of a block of iterates, checked before the library is called (needs no object): (dim, ncols)."""
    A = np.asarray(A)
    if A.ndim != 2 or A.shape != (dim, ncols):
        raise ValueError(f"{name} must have shape ({dim}, {ncols}), got {A.shape}")


def check_skip(ncols, skip):
    """skip: None or ncols flags.  Returns an integer array or None."""
    if skip is None:
        return None
    s = np.asarray(skip)
    if s.shape != (ncols,):
        raise ValueError(f"skip must have shape ({ncols},), got {s.shape}")
    return s


class Accel:
    def __init__(self, dim, ncols, lookback=10, type1=True, regularization=1e-8, relaxation=1.0, dtype="f64"):
        self._a = None
        self._lib = capi.load("libscsamd_f32.so" if dtype in ("f32", np.float32) else "libscsamd.so")
        T = self._T = self._lib._scs_types
        self.dim, self.ncols, self.lookback = int(dim), int(ncols), int(lookback)
        if self.dim < 1 or self._lib.scs_amd_aa_multi_width(self.ncols) == 0:
            raise ValueError("dim must be >= 1 and ncols in 1 .. 16")
        self._a = self._lib.scs_amd_aa_multi_init(self.dim, self.ncols, self.lookback, max(self.lookback, 1), 1 if type1 else 0,
                                                  regularization, relaxation, SAFEGUARD_FACTOR, MAX_WEIGHT_NORM, IR_MAX_STEPS)
        if not self._a:
            raise ValueError("scs_amd_aa_multi_init failed (bad parameters or no device memory)")

    def _obj(self):
        if not self._a:
            raise RuntimeError("object was closed")
        return self._a

    def _args(self, F, X, skip):
        T = self._T
        check_block(self.dim, self.ncols, F, "F")
        check_block(self.dim, self.ncols, X, "X")
        if not (isinstance(F, np.ndarray) and F.dtype == T.np_float and F.flags.f_contiguous and F.flags.writeable):
            raise ValueError(f"F is updated in place: it must be a writeable column-major {np.dtype(T.np_float).name} array")
        s = check_skip(self.ncols, skip)
        sk = None if s is None else np.ascontiguousarray(s != 0, dtype=T.np_int)
        return sk, (None if sk is None else sk.ctypes.data_as(T.ip))

    def apply_many(self, F, X, skip=None):
        """scs_amd_aa_multi_apply: column k of F (dim, ncols) is the map's output for the iterate in column k of X.  F is
        updated in place where a step was applied.  Returns aa_norm (ncols): 0 while a column seeds or fills its memory,
        negative on a rejected solve, positive when applied; 0 for a skipped column, of which nothing is read or written."""
        a, T = self._obj(), self._T
        sk, skp = self._args(F, X, skip)
        Xc = np.asfortranarray(X, dtype=T.np_float)
        nrm = np.zeros(self.ncols, dtype=T.np_float)
        ld = max(self.dim, 1)
        if self._lib.scs_amd_aa_multi_apply(a, F.ctypes.data_as(T.fp), ld, Xc.ctypes.data_as(T.fp), ld, skp,
                                            nrm.ctypes.data_as(T.fp)) != 0:
            raise RuntimeError("scs_amd_aa_multi_apply failed")
        return nrm

    def safeguard_many(self, F, X, skip=None):
        """scs_amd_aa_multi_safeguard: F = the map applied to X, after an applied step.  Returns rejected (ncols) of 0 / -1;
        where -1, column k of F and X (both in place) are back at the last pair before the step and the column's memory is
        empty.  X must be a writeable column-major array like F."""
        a, T = self._obj(), self._T
        sk, skp = self._args(F, X, skip)
        self._args(X, F, skip)
        rej = np.zeros(self.ncols, dtype=T.np_int)
        ld = max(self.dim, 1)
        if self._lib.scs_amd_aa_multi_safeguard(a, F.ctypes.data_as(T.fp), ld, X.ctypes.data_as(T.fp), ld, skp,
                                                rej.ctypes.data_as(T.ip)) != 0:
            raise RuntimeError("scs_amd_aa_multi_safeguard failed")
        return rej

    def reset(self, col=None):
        """Empty the memory of column `col`, or of every column (None)."""
        if col is not None and not 0 <= int(col) < self.ncols:
            raise ValueError("col out of range")
        self._lib.scs_amd_aa_multi_reset(self._obj(), -1 if col is None else int(col))

    def stats(self, col):
        """The AaStats of one column as a dict."""
        if not 0 <= int(col) < self.ncols:
            raise ValueError("col out of range")
        st = self._T.AaStats()
        self._lib.scs_amd_aa_multi_get_stats(self._obj(), int(col), C.byref(st))
        return {k: getattr(st, k) for k, _ in self._T.AaStats._fields_}

    def counters(self):
        """dict(applies, apply_syncs, safeguard_syncs, launches) since the object was created."""
        out = (C.c_longlong * 4)()
        self._lib.scs_amd_aa_multi_get_counters(self._obj(), C.byref(out))
        return dict(applies=out[0], apply_syncs=out[1], safeguard_syncs=out[2], launches=out[3])

    def close(self):
        if self._a:
            self._lib.scs_amd_aa_multi_finish(self._a)
            self._a = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
