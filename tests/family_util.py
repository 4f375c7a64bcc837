"""Helpers of the family tests (tests/test_family_gpu.py): families of (b, c) on a shared A by the generator's law, and a
workspace that is driven column after column with scs_update + scs_solve -- the thing scs_amd_solve_family is measured against,
on the reference's libraries and on the project's own."""
import ctypes as C

import numpy as np

from scs_amd import capi, problems


def family_data(A, cone, K, seed, proj=problems.proj_dual_cone_np, b_scale=None):
    """K columns (b_k, c_k) by the law of scs_amd/problems.py on the shared A: z_k, x_k fresh draws, y_k = Proj_K*(z_k),
    s_k = y_k - z_k, b_k = A x_k + s_k, c_k = -A' y_k.  b_scale (K factors, optional) scales b_k: still feasible and bounded
    (the cone is a cone), a different problem with a different iteration count.  Returns B (m x K), Cc (n x K)."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    B, Cc = np.zeros((m, K), order="F"), np.zeros((n, K), order="F")
    for k in range(K):
        z = rng.uniform(-1, 1, m)
        y = proj(z, cone)
        s = y - z
        x = rng.uniform(-1, 1, n)
        B[:, k] = (A @ x + s) * (1.0 if b_scale is None else b_scale[k])
        Cc[:, k] = -(A.T @ y)
    return B, Cc


class Work:
    """One workspace of `lib` (the HIP library or a reference build) on prob, reused for a sequence of (b, c)."""

    def __init__(self, lib, prob, cg_tol_override=None, **over):
        self.lib, self.prob, self.T = lib, prob, lib._scs_types
        self.st = capi.default_settings(lib, **over)
        self.w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(self.st))
        if not self.w:
            raise RuntimeError("scs_init returned NULL")
        if cg_tol_override is not None:
            lib.scs_amd_set_cg_tol_override(self.w, float(cg_tol_override))

    def solve(self, b=None, c=None, warm=None):
        """scs_update(b, c) when given, then scs_solve; dict(x, y, s, info)."""
        T, f = self.T, self.T.np_float
        if b is not None or c is not None:
            bb = None if b is None else np.ascontiguousarray(b, dtype=f)
            cc = None if c is None else np.ascontiguousarray(c, dtype=f)
            rc = self.lib.scs_update(self.w, None if bb is None else bb.ctypes.data_as(T.fp), None if cc is None else cc.ctypes.data_as(T.fp))
            assert rc == 0
        x, y, s = np.zeros(self.prob.n, dtype=f), np.zeros(self.prob.m, dtype=f), np.zeros(self.prob.m, dtype=f)
        if warm is not None:
            x[:], y[:], s[:] = warm
        sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
        info = T.ScsInfo()
        self.lib.scs_solve(self.w, C.byref(sol), C.byref(info), 1 if warm is not None else 0)
        return dict(x=x, y=y, s=s, info=capi.info_dict(info))

    def solve_columns(self, B, Cc, warm=None):
        return [self.solve(B[:, k], Cc[:, k], None if warm is None else tuple(v[:, k] for v in warm)) for k in range(B.shape[1])]

    def family(self, B, Cc, warm=None, warm_start=None):
        return capi.solve_family(self.lib, self.w, B, Cc, warm=warm, warm_start=warm_start)

    def close(self):
        if self.w:
            self.lib.scs_finish(self.w)
            self.w = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
