"""`Cones` -- the cone-projection workspace of the C ABI (include/scs_amd.h, B1') as a Python object.

Projects onto the DUAL cone under the r_y metric (the Moreau wrapper of reference src/cones.c:1552-1596) on the GPU, one vector
(`project`, scs_amd_cone_proj_dual) or a block of them at once (`project_many`, scs_amd_cone_proj_dual_multi: K projections
that share the cone description and r_y).  One workspace lives for the lifetime of the object (scs_amd_cone_init once,
scs_amd_cone_finish on close / garbage collection); it carries the box cone's Newton start and the PSD blocks' eigenbases from
call to call, per column position for blocks.  Host code only: every flop is in the library.

cone  : dict(z=, l=, bu=, bl=, q=[...], s=[...], cs=[...], ep=, ed=, p=[...])
D     : row scaling (m) applied to the box bounds as the reference's normalize_box_cone does, or None
dtype : "f64" (default) or "f32" (the SFLOAT library)
"""
import ctypes as C

import numpy as np

from . import capi


def check_block(m, X, r_y=None):
    """Shapes of a block projection, checked before the library is called (needs no workspace): X (m, K) with K >= 1, r_y None
    or (m,) and positive.  Returns K."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] != m or X.shape[1] < 1:
        raise ValueError(f"X must have shape ({m}, K) with K >= 1, got {X.shape}")
    if r_y is not None:
        r = np.asarray(r_y)
        if r.shape != (m,):
            raise ValueError(f"r_y must have shape ({m},), got {r.shape}")
        if not np.all(r > 0):
            raise ValueError("r_y must be positive")
    return X.shape[1]


class Cones:
    def __init__(self, cone, D=None, dtype="f64"):
        self._w = None
        self._lib = capi.load("libscsamd_f32.so" if dtype in ("f32", np.float32) else "libscsamd.so")
        T = self._T = self._lib._scs_types
        self.cone = dict(cone)
        self.m = capi.cone_rows(self.cone)
        self._k = capi.make_cone(self.cone, T)  # owns the arrays behind the pointers
        Dv = None
        if D is not None:
            Dv = np.ascontiguousarray(D, dtype=T.np_float)
            if Dv.shape != (self.m,):
                raise ValueError("D has the wrong length")
        self._w = self._lib.scs_amd_cone_init(C.byref(self._k), self.m, Dv.ctypes.data_as(T.fp) if Dv is not None else None)
        if not self._w:
            raise ValueError("ScsAmdConeWork allocation error!")

    def _work(self):
        if not self._w:
            raise RuntimeError("workspace was closed")
        return self._w

    def _ry(self, r_y):
        if r_y is None:
            return None, None
        r = np.ascontiguousarray(r_y, dtype=self._T.np_float)
        return r, r.ctypes.data_as(self._T.fp)

    def project(self, x, r_y=None):
        """scs_amd_cone_proj_dual: x (m) -> its projection onto the dual cone under the r_y metric (r_y None: Euclidean)."""
        w, T = self._work(), self._T
        if np.asarray(x).shape != (self.m,):
            raise ValueError("x has the wrong length")
        check_block(self.m, np.asarray(x).reshape(self.m, 1), r_y)
        out = np.array(x, dtype=T.np_float, order="C", copy=True)
        r, rp = self._ry(r_y)
        if self._lib.scs_amd_cone_proj_dual(w, out.ctypes.data_as(T.fp), rp) < 0:
            raise RuntimeError("scs_amd_cone_proj_dual failed")
        return out

    def project_many(self, X, r_y=None):
        """scs_amd_cone_proj_dual_multi: column k of X (m, K), in any memory order -> the projection of that column, as `project`
        would give it.  Returns (m, K); X and r_y are not modified."""
        w, T = self._work(), self._T
        K = check_block(self.m, X, r_y)
        out = np.array(X, dtype=T.np_float, order="F", copy=True)
        r, rp = self._ry(r_y)
        if self._lib.scs_amd_cone_proj_dual_multi(w, K, out.ctypes.data_as(T.fp), max(self.m, 1), rp) < 0:
            raise RuntimeError("scs_amd_cone_proj_dual_multi failed")
        return out

    def close(self):
        if self._w:
            self._lib.scs_amd_cone_finish(self._w)
            self._w = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
