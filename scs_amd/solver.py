"""`SCS` -- the object scs-python users hold, over this library's C ABI.

Mirrors the reference project's Python interface (docs/src/api/python.rst in the
reference tree: `scs.SCS(data, cone, **settings)`, `.solve(warm_start=True, x=None, y=None,
s=None)`, `.update(b=None, c=None)` (here also `A=`, `P=`: new matrix values), result dict with 'x', 'y', 's', 'info') so that code
written against `import scs` switches with `from scs_amd.solver import SCS`.  One ScsWork
lives for the lifetime of the object (scs_init once, scs_solve / scs_update many times,
scs_finish on close / garbage collection), exactly the workspace reuse the C API offers
(include/scs.h:271-324).  Host code only: every flop is in libscsamd.so.

data : dict with 'A' (scipy sparse, m x n), 'b' (m), 'c' (n), optional 'P' (n x n, symmetric;
       the upper triangle is used, as the C API requires)
cone : dict with any of 'z' (or legacy 'f'), 'l', 'bu', 'bl', 'q', 's', 'cs', 'ep', 'ed', 'p'
settings : the fields of ScsSettings (eps_abs, max_iters, acceleration_lookback, ...);
       `use_indirect` / `gpu` / `mkl` are accepted and ignored (there is one backend);
       `dtype="f32"` selects the SFLOAT library.
"""
import ctypes as C

import numpy as np

from . import capi


class SCS:
    def __init__(self, data, cone, dtype="f64", **settings):
        self._lib = capi.load("libscsamd_f32.so" if dtype in ("f32", np.float32) else "libscsamd.so")
        self._T = self._lib._scs_types
        self._w = None
        if any(k not in data for k in ("A", "b", "c")):
            raise ValueError("data must contain 'A', 'b' and 'c'")
        cone, kw = capi.cone_and_settings(cone, settings)
        self._prob = capi.Problem(data["A"], data["b"], data["c"], cone, P=data.get("P"), T=self._T)
        self._settings = capi.default_settings(self._lib, **kw)
        self._w = self._lib.scs_init(C.byref(self._prob.data), C.byref(self._prob.k), C.byref(self._settings))
        if not self._w:
            raise ValueError("ScsWork allocation error!")  # scs-python's message for a failed scs_init
        f = self._T.np_float
        self._x = np.zeros(self._prob.n, dtype=f)
        self._y = np.zeros(self._prob.m, dtype=f)
        self._s = np.zeros(self._prob.m, dtype=f)
        self._solved_once = False

    def solve(self, warm_start=True, x=None, y=None, s=None):
        """scs_solve.  With warm_start the previous solution (or the x / y / s given) seeds the
        iteration, as in scs-python; the first solve of an object without x / y / s is cold."""
        if not self._w:
            raise RuntimeError("solver was closed")
        T = self._T
        given = [v is not None for v in (x, y, s)]
        for dst, src in ((self._x, x), (self._y, y), (self._s, s)):
            if src is not None:
                src = np.asarray(src, dtype=dst.dtype)
                if src.shape != dst.shape:
                    raise ValueError("warm-start vector has the wrong length")
                dst[:] = src
        warm = bool(warm_start) and (self._solved_once or any(given))
        sol = T.ScsSolution(self._x.ctypes.data_as(T.fp), self._y.ctypes.data_as(T.fp), self._s.ctypes.data_as(T.fp))
        info = T.ScsInfo()
        self._lib.scs_solve(self._w, C.byref(sol), C.byref(info), 1 if warm else 0)
        self._solved_once = True
        return {"x": self._x.copy(), "y": self._y.copy(), "s": self._s.copy(), "info": capi.info_dict(info)}

    def update(self, b=None, c=None, A=None, P=None):
        """scs_update: new right-hand side and / or cost on the same workspace.  A / P (an extension, scs_amd_update_matrix): new VALUES
        of the matrices on the pattern given at construction -- a scipy sparse matrix with exactly that pattern, or a 1-D array of the
        values in its CSC order (P: upper triangle); the workspace is then what a new object on those matrices would hold, without the
        pattern-dependent setup.  A different pattern or a non-finite value raises ValueError before the library is called."""
        if not self._w:
            raise RuntimeError("solver was closed")
        T = self._T
        f = T.np_float
        ax = None if A is None else self._prob.values_of(A, "A")
        px = None if P is None else self._prob.values_of(P, "P")
        for v in (ax, px):
            if v is not None and not np.all(np.isfinite(v)):
                raise ValueError("matrix values must be finite")
        bp = cp = None
        if b is not None:
            self._b_new = np.ascontiguousarray(b, dtype=f)
            if self._b_new.shape != (self._prob.m,):
                raise ValueError("b has the wrong length")
            bp = self._b_new.ctypes.data_as(T.fp)
        if c is not None:
            self._c_new = np.ascontiguousarray(c, dtype=f)
            if self._c_new.shape != (self._prob.n,):
                raise ValueError("c has the wrong length")
            cp = self._c_new.ctypes.data_as(T.fp)
        if (bp is not None or cp is not None or (ax is None and px is None)) and self._lib.scs_update(self._w, bp, cp) != 0:
            raise RuntimeError("scs_update failed")
        if ax is not None or px is not None:
            if self._lib.scs_amd_update_matrix(self._w, ax.ctypes.data_as(T.fp) if ax is not None else None,
                                               px.ctypes.data_as(T.fp) if px is not None else None) != 0:
                raise RuntimeError("scs_amd_update_matrix failed")

    def _values_blocks(self, A, P):
        """A / P of set_family_values as the nnz x K blocks of the library: lists of K matrices on the construction pattern (or of K
        value arrays in its CSC order), or nnz x K arrays.  The checks of update(A=, P=) per column; ValueError before any library call."""
        has_P = self._prob.matP is not None
        if A is None:
            raise ValueError("A must be given: the values of every problem's A")
        if (P is not None) != has_P:
            raise ValueError("P must be given exactly when the object was built with a P")

        def cols(V, which):
            if isinstance(V, (list, tuple)):
                if not V:
                    raise ValueError(f"{which} must hold at least one problem's values")
                V = np.column_stack([self._prob.values_of(M, which) for M in V])
            nnz = len(self._prob.Ax) if which == "A" else len(self._prob.Px)
            return capi.values_block(V, nnz, which, self._T.np_float)
        AX = cols(A, "A")
        PX = cols(P, "P") if has_P else None
        if PX is not None and PX.shape[1] != AX.shape[1]:
            raise ValueError("A and P must hold the same number of problems")
        return AX, PX

    def set_family_values(self, A, P=None):
        """scs_amd_family_set_values: the values of K <= 16 problems' A (and P) on the pattern given at construction, stored for any
        number of solve_family(B, C, own_values=True) calls.  A / P: lists of K scipy matrices with exactly that pattern, or nnz x K
        arrays in its CSC order (P: upper triangle).  A different pattern or a non-finite value raises ValueError before the library
        is called; a refusal of the library raises ValueError with its message.  The object's own problem is not touched."""
        if not self._w:
            raise RuntimeError("solver was closed")
        AX, PX = self._values_blocks(A, P)
        if capi.family_set_values(self._lib, self._w, AX, PX) != 0:
            why = self._lib.scs_amd_solve_family_values_refusal(self._w)
            raise ValueError(why.decode() if why else "scs_amd_family_set_values failed")
        return AX.shape[1]

    def free_family_values(self):
        """scs_amd_family_free_values: releases what set_family_values holds on the device"""
        if self._w:
            capi.family_free_values(self._lib, self._w)

    def solve_family(self, B, C, warm_start=False, x=None, y=None, s=None, scale=None, own_scale=False, stream=False, width=None,
                     A=None, P=None, own_values=False):
        """scs_amd_solve_family: K problems that share A, P and the cones of this object and differ in (b, c), in one
        device-resident loop.  B: m x K, C: n x K, as arrays or as lists of K vectors.  With warm_start, x (n x K), y and
        s (m x K) seed the columns.  Returns a list of K dicts in the shape `solve` returns.  The object's own problem and
        its last solution are not touched.  Needs adaptive_scale=0, acceleration_lookback=0 and no log_csv_filename:
        otherwise ValueError with the library's message.
        own_scale=True (scs_amd_solve_family_scaled): every problem runs under its own scale and the object's adaptive_scale is
        honoured, problem by problem; info["scale"] and info["scale_updates"] are the problem's own.  scale: K initial scales
        (implies own_scale); without it every problem starts at the object's scale.
        stream=True (scs_amd_solve_family_stream): the K problems are a queue through one block of `width` columns (2, 4, 8 or
        16; None: chosen from K), a finished column's slot going to the next problem, instead of chunks of 16 that each wait
        for their slowest column; every problem has the bits the call without stream gives it at that width.  Cones with PSD
        blocks are refused (ValueError with the library's message); a width that is none of those raises ValueError.
        A= (and P= when the object has a P; scs_amd_solve_family_values): problem k has its own matrix values as well, given as
        for set_family_values, K <= 16; it runs under its own scale as with own_scale, and is what update(A=A[k], P=P[k], b=, c=)
        and solve() would give.  own_values=True: the values of the last set_family_values instead (set once, solve many).
        Neither goes with stream=True (ValueError)."""
        if not self._w:
            raise RuntimeError("solver was closed")
        m, n = self._prob.m, self._prob.n
        values = A is not None or P is not None or bool(own_values)
        if values and stream:
            raise ValueError("A / P / own_values do not go with stream=True: the stream entry shares the values of A and P")
        if own_values and (A is not None or P is not None):
            raise ValueError("own_values=True uses the values of set_family_values: give no A / P")
        vblocks = self._values_blocks(A, P) if values and not own_values else None

        def block(v, rows, what):
            if isinstance(v, (list, tuple)):
                v = np.column_stack([np.asarray(c, dtype=float).reshape(-1) for c in v]) if len(v) else np.zeros((rows, 0))
            v = np.asarray(v, dtype=float)
            if v.ndim == 1:
                v = v.reshape(-1, 1)
            if v.ndim != 2 or v.shape[0] != rows:
                raise ValueError(f"{what} must have {rows} rows")
            return v
        B, C_ = block(B, m, "B"), block(C, n, "C")
        K = B.shape[1]
        if K < 1 or C_.shape[1] != K:
            raise ValueError("B and C must have the same number K >= 1 of columns")
        scaled = bool(own_scale) or scale is not None
        if width is not None and not stream:
            raise ValueError("width belongs to stream=True")
        if stream:
            if width is not None and (isinstance(width, bool) or not isinstance(width, (int, np.integer))
                                      or int(width) not in capi.STREAM_WIDTHS[1:]):
                raise ValueError("width must be None, 2, 4, 8 or 16")
            width = 0 if width is None else int(width)
        if scale is not None:
            scale = np.asarray(scale, dtype=float).reshape(-1)
            if scale.shape[0] != K:
                raise ValueError("scale must hold one initial scale per problem")
        if vblocks is not None and vblocks[0].shape[1] != K:
            raise ValueError("A must hold one matrix per column of B")
        if not stream and not values:
            why = (self._lib.scs_amd_solve_family_scaled_refusal if scaled else self._lib.scs_amd_solve_family_refusal)(self._w)
            if why:
                raise ValueError(why.decode())
        warm = None
        if warm_start:
            if x is None or y is None or s is None:
                raise ValueError("warm_start needs x, y and s")
            warm = (block(x, n, "x"), block(y, m, "y"), block(s, m, "s"))
            if any(v.shape[1] != K for v in warm):
                raise ValueError("warm-start blocks must have K columns")
        if values:
            # the refusal function of these two entries reports the last call's arguments too: asked after a call that failed
            rc = capi.family_set_values(self._lib, self._w, *vblocks) if vblocks is not None else 0
            out = None
            if rc == 0:
                rc, out = capi.solve_family_values(self._lib, self._w, B, C_, scales=scale, warm=warm)
            if rc != 0:
                why = self._lib.scs_amd_solve_family_values_refusal(self._w)
                if why:
                    raise ValueError(why.decode())
                raise RuntimeError("scs_amd_solve_family_values failed")
            return out
        if stream:
            rc, out = capi.solve_family_stream(self._lib, self._w, B, C_, width=int(width), own_scale=scaled, scales=scale, warm=warm)
        elif scaled:
            rc, out = capi.solve_family_scaled(self._lib, self._w, B, C_, scales=scale, warm=warm)
        else:
            rc, out = capi.solve_family(self._lib, self._w, B, C_, warm=warm)
        if rc != 0 and stream:
            # The stream entry's refusal function also reports the arguments the LAST call was refused for (a scale that is not
            # positive, say), until a call is accepted: asked before the call it would hold a refusal that no longer applies, so
            # it is asked after a call that failed, where it speaks of that call.  The library refuses before any device work.
            why = self._lib.scs_amd_solve_family_stream_refusal(self._w, 1 if scaled else 0)
            if why:
                raise ValueError(why.decode())
        if rc != 0:
            raise RuntimeError("scs_amd_solve_family_stream failed" if stream else
                               "scs_amd_solve_family_scaled failed" if scaled else "scs_amd_solve_family failed")
        return out

    def close(self):
        if getattr(self, "_w", None):
            self._lib.scs_finish(self._w)
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


def solve(data, cone, **settings):
    """One-shot form (scs-python 2.x `scs.solve`)."""
    with SCS(data, cone, **settings) as solver:
        return solver.solve()
