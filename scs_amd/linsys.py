"""`LinSys` -- the linear-system workspace of the plugin ABI (include/scs_amd.h, B1) as a Python object.

Solves the reduced KKT system of SCS on the GPU,

    (R_x + P + A' R_y^-1 A) x = r_x + A' R_y^-1 r_y ,   y = R_y^-1 (A x - r_y)

for one right-hand side (`solve`, scs_solve_lin_sys) or for a block of them at once (`solve_many`,
scs_amd_solve_lin_sys_multi: K independent PCG solves in lock step that share A, P and diag_r; with `diag_r=` every column
runs under its own diag_r, scs_amd_solve_lin_sys_multi_r -- a sweep over rho, scale or regularisation as one block; after
`set_values_many`, `own_values=True` gives every column its own values of A and P on the shared pattern,
scs_amd_solve_lin_sys_multi_v -- time-varying or scenario-dependent coefficients as one block).  One workspace lives for the
lifetime of the object (scs_init_lin_sys_work once, scs_free_lin_sys_work on close / garbage collection).  Host code only: every
flop is in the library.

A      : scipy sparse, m x n
diag_r : [R_x (n); R_y (m)], positive
P      : n x n symmetric or None; the upper triangle is used, as the C API requires
dtype  : "f64" (default) or "f32" (the SFLOAT library)
"""
import ctypes as C

import numpy as np

from . import capi


def check_block(n, m, B, S=None, tol=1e-9, DR=None):
    """Shapes of a block solve, checked before the library is called (needs no workspace): B (n + m, K), S None or (n, K),
    tol a positive scalar or K of them, DR None or (n + m, K) with every entry finite and positive (column k = the diag_r of
    column k).  Returns K."""
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != n + m or B.shape[1] < 1:
        raise ValueError(f"B must have shape ({n + m}, K) with K >= 1, got {B.shape}")
    K = B.shape[1]
    if S is not None:
        S = np.asarray(S)
        if S.ndim != 2 or S.shape != (n, K):
            raise ValueError(f"S must have shape ({n}, {K}), got {S.shape}")
    t = np.asarray(tol, dtype=np.float64)
    if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != K):
        raise ValueError(f"tol must be a scalar or have length {K}, got shape {t.shape}")
    if not np.all(t > 0):
        raise ValueError("tol must be positive")
    if DR is not None:
        DR = np.asarray(DR)
        if DR.ndim != 2 or DR.shape != (n + m, K):
            raise ValueError(f"diag_r must have shape ({n + m}, {K}), got {DR.shape}")
        if not (np.all(np.isfinite(DR)) and np.all(DR > 0)):
            raise ValueError("diag_r must be finite and positive")
    return K


def check_values_block(nnz_a, nnz_p, A_values, P_values):
    """Shapes of a block of matrix values, checked before the library is called (needs no workspace): A_values (nnz_a, K) with
    1 <= K <= 16, P_values (nnz_p, K) exactly when the workspace has a P (nnz_p is None without one), every entry finite.
    Returns K."""
    A_values = np.asarray(A_values)
    if A_values.ndim != 2 or A_values.shape[0] != nnz_a or not 1 <= A_values.shape[1] <= 16:
        raise ValueError(f"A_values must have shape ({nnz_a}, K) with 1 <= K <= 16, got {A_values.shape}")
    K = A_values.shape[1]
    if (P_values is None) != (nnz_p is None):
        raise ValueError("P_values must be given exactly when the workspace has a P")
    if P_values is not None:
        P_values = np.asarray(P_values)
        if P_values.ndim != 2 or P_values.shape != (nnz_p, K):
            raise ValueError(f"P_values must have shape ({nnz_p}, {K}), got {P_values.shape}")
    for v in (A_values, P_values):
        if v is not None and not np.all(np.isfinite(v)):
            raise ValueError("matrix values must be finite")
    return K


class LinSys:
    def __init__(self, A, diag_r, P=None, dtype="f64"):
        self._w = None
        self._vcols = 0  # columns of the set_values_many in force
        self._lib = capi.load("libscsamd_f32.so" if dtype in ("f32", np.float32) else "libscsamd.so")
        T = self._T = self._lib._scs_types
        import scipy.sparse as sp
        A = sp.csc_matrix(A)
        self.m, self.n = A.shape
        diag_r = np.ascontiguousarray(diag_r, dtype=T.np_float)
        if diag_r.shape != (self.n + self.m,):
            raise ValueError("diag_r has the wrong length")
        if P is not None and sp.csc_matrix(P).shape != (self.n, self.n):
            raise ValueError("P has the wrong shape")
        self._prob = capi.Problem(A, np.zeros(self.m), np.zeros(self.n), dict(l=self.m), P=P, T=T)  # owns the arrays behind the pointers
        self._w = self._lib.scs_init_lin_sys_work(C.byref(self._prob.matA), C.byref(self._prob.matP) if self._prob.matP is not None else None,
                                                  diag_r.ctypes.data_as(T.fp))
        if not self._w:
            raise ValueError("ScsLinSysWork allocation error!")

    def _work(self):
        if not self._w:
            raise RuntimeError("workspace was closed")
        return self._w

    def solve(self, b, s=None, tol=1e-9):
        """scs_solve_lin_sys: b = [r_x; r_y] -> [x; y]; s = warm start for x (n) or None."""
        w, T = self._work(), self._T
        b = np.asarray(b)
        if b.shape != (self.n + self.m,):
            raise ValueError("b has the wrong length")
        if s is not None and np.asarray(s).shape != (self.n,):
            raise ValueError("s has the wrong length")
        if not tol > 0:
            raise ValueError("tol must be positive")
        out = np.array(b, dtype=T.np_float, order="C", copy=True)
        sv = None if s is None else np.ascontiguousarray(s, dtype=T.np_float)
        if self._lib.scs_solve_lin_sys(w, out.ctypes.data_as(T.fp), sv.ctypes.data_as(T.fp) if sv is not None else None, float(tol)) != 0:
            raise RuntimeError("scs_solve_lin_sys failed")
        return out

    def set_values_many(self, A_values, P_values=None):
        """scs_amd_linsys_set_values_multi: the values of K (1 .. 16) systems on the pattern given at construction, for
        `solve_many(..., own_values=True)`.  A_values (nnz(A), K): column k = the values of A_k in the CSC order of A; P_values
        (nnz(upper P), K), exactly when the workspace has a P.  The workspace's own matrices, `solve` and the other forms of
        `solve_many` are not affected.  ValueError for bad shapes, a non-finite value or a refusal of the library."""
        w, T = self._work(), self._T
        nnz_p = None if self._prob.matP is None else len(self._prob.Pi)
        K = check_values_block(len(self._prob.Ai), nnz_p, A_values, P_values)
        ax = np.asfortranarray(A_values, dtype=T.np_float)
        px = None if P_values is None else np.asfortranarray(P_values, dtype=T.np_float)
        for v in (ax, px):
            if v is not None and not np.all(np.isfinite(v)):  # an entry that overflows in the library's precision
                raise ValueError("matrix values must be finite in the library's precision")
        rc = self._lib.scs_amd_linsys_set_values_multi(w, K, ax.ctypes.data_as(T.fp), max(1, ax.shape[0]),
                                                       px.ctypes.data_as(T.fp) if px is not None else None,
                                                       max(1, px.shape[0]) if px is not None else 0)
        if rc != 0:
            raise ValueError("scs_amd_linsys_set_values_multi refused the values")
        self._vcols = K

    def free_values_many(self):
        """scs_amd_linsys_free_values_multi: releases the device memory of `set_values_many`; a later set call allocates again."""
        self._lib.scs_amd_linsys_free_values_multi(self._work())
        self._vcols = 0

    def solve_many(self, B, S=None, tol=1e-9, diag_r=None, own_values=False):
        """scs_amd_solve_lin_sys_multi: column k of B (n + m, K) -> [x; y] of that column, as `solve` would give it; S (n, K) warm
        starts or None; tol a scalar or one per column.  Returns (XY, iters): the solutions (n + m, K) and the PCG iteration count
        of every column.  diag_r (n + m, K): column k is solved under its own diag_r = diag_r[:, k], as `update_diag_r` followed by
        `solve` would give it (scs_amd_solve_lin_sys_multi_r); the workspace's own diag_r is neither used nor changed.
        own_values: column k is solved with the values of A and P given to `set_values_many` as column k, as `update_values`
        followed by the above would give it (scs_amd_solve_lin_sys_multi_v); K must equal the set call's; diag_r None = the
        workspace's diag_r in every column.  The workspace's own matrices are neither used nor changed.
        B, S, tol and diag_r are not modified."""
        w, T = self._work(), self._T
        K = check_block(self.n, self.m, B, S, tol, diag_r)
        if own_values and K != self._vcols:
            raise ValueError(f"own_values needs a set_values_many of {K} columns first (in force: {self._vcols})")
        out = np.array(B, dtype=T.np_float, order="F", copy=True)
        Sv = None if S is None else np.asfortranarray(S, dtype=T.np_float)
        tv = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=T.np_float), (K,)))
        iters = np.zeros(K, dtype=T.np_int)
        Dv = None
        if diag_r is not None:
            Dv = np.asfortranarray(diag_r, dtype=T.np_float)
            if not np.all(Dv > 0):  # an entry that underflows in the library's precision
                raise ValueError("diag_r must be positive in the library's precision")
        fp = lambda v: None if v is None else v.ctypes.data_as(T.fp)
        lead = (fp(Dv), self.n + self.m)  # the DR pair that the two per-column entries take in front of B
        if own_values:
            entry, failure = self._lib.scs_amd_solve_lin_sys_multi_v, ValueError("scs_amd_solve_lin_sys_multi_v refused the call")
        elif diag_r is not None:
            entry, failure = self._lib.scs_amd_solve_lin_sys_multi_r, RuntimeError("scs_amd_solve_lin_sys_multi_r failed")
        else:
            entry, lead, failure = self._lib.scs_amd_solve_lin_sys_multi, (), RuntimeError("scs_amd_solve_lin_sys_multi failed")
        if entry(w, K, *lead, fp(out), self.n + self.m, fp(Sv), self.n, fp(tv), iters.ctypes.data_as(T.ip)) != 0:
            raise failure
        return out, iters.astype(np.int64)

    def update_diag_r(self, d):
        """scs_update_lin_sys_diag_r: new [R_x; R_y]; applies to single and block solves alike."""
        w, T = self._work(), self._T
        d = np.ascontiguousarray(d, dtype=T.np_float)
        if d.shape != (self.n + self.m,):
            raise ValueError("diag_r has the wrong length")
        if self._lib.scs_update_lin_sys_diag_r(w, d.ctypes.data_as(T.fp)) != 0:
            raise RuntimeError("scs_update_lin_sys_diag_r failed")

    def update_values(self, A_values=None, P_values=None):
        """scs_amd_linsys_update_values: new values of A and / or P on the pattern given at construction (a scipy sparse matrix with
        that pattern, or the values in its CSC order; P: upper triangle).  diag_r stays; single and block solves alike see the new
        matrices.  ValueError for a different pattern or a non-finite value, before the library is called."""
        w, T = self._work(), self._T
        ax = None if A_values is None else self._prob.values_of(A_values, "A")
        px = None if P_values is None else self._prob.values_of(P_values, "P")
        for v in (ax, px):
            if v is not None and not np.all(np.isfinite(v)):
                raise ValueError("matrix values must be finite")
        if self._lib.scs_amd_linsys_update_values(w, ax.ctypes.data_as(T.fp) if ax is not None else None,
                                                  px.ctypes.data_as(T.fp) if px is not None else None) != 0:
            raise RuntimeError("scs_amd_linsys_update_values failed")

    def stats(self):
        """ScsAmdStats of the workspace as a dict (cg_iters, lin_sys_solves, mat_vecs, ...)."""
        st = self._T.ScsAmdStats()
        self._lib.scs_amd_linsys_get_stats(self._work(), C.byref(st))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def close(self):
        if self._w:
            self._lib.scs_free_lin_sys_work(self._w)
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
