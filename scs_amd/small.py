"""`SmallBatch` -- any number of SMALL problems that share A, P, the cone and the settings and differ in (b, c), every problem
solved from its first iteration to its convergence test by one workgroup inside one kernel (scs_amd_small_* in include/scs_amd.h).
Problems that bring their own values of A and P on the object's pattern: `set_values` / `solve(..., own_values=True)`, or
`solve(B, C, A=[...], P=[...])`; every problem is then equilibrated and factored by itself (scs_amd_small_set_values).

    with SmallBatch(data, cone, eps_abs=1e-4, eps_rel=1e-4) as sb:
        results = sb.solve(B, C)            # B: m x K, C: n x K  ->  K dicts with 'x', 'y', 's', 'info'
        results = sb.solve(B, C, A=[A_0, ...], P=[P_0, ...])   # every problem its own values on the object's pattern
        sb.set_values([A_0, ...], [P_0, ...]); sb.solve(B2, C2, own_values=True)   # ... set once, solved again

data, cone, settings: the construction arguments of `scs_amd.solver.SCS`.  adaptive_scale and acceleration_lookback default to 0
here (the batch serves nothing else); what the library does not serve -- box, PSD, exponential and power cones, a size over
`.limits`, adaptive scale, acceleration, a time limit, the two file names -- raises ValueError with the library's message.
Host code only: every flop is in libscsamd.so.
"""
import ctypes as ct

import numpy as np

from . import capi


def limits(lib=None):
    """(largest n, largest n + m + 1) the library serves"""
    lib = lib or capi.load("libscsamd.so")
    out = (lib._scs_types.scs_int * 2)()
    lib.scs_amd_small_limits(ct.byref(out))
    return int(out[0]), int(out[1])


class SmallBatch:
    def __init__(self, data, cone, dtype="f64", **settings):
        self._lib = capi.load("libscsamd_f32.so" if dtype in ("f32", np.float32) else "libscsamd.so")
        self._T = self._lib._scs_types
        self._h = None
        self._nvalues = 0  # problems of the last set_values
        if any(k not in data for k in ("A", "b", "c")):
            raise ValueError("data must contain 'A', 'b' and 'c'")
        cone, kw = capi.cone_and_settings(cone, settings, adaptive_scale=0, acceleration_lookback=0)
        self._prob = capi.Problem(data["A"], data["b"], data["c"], cone, P=data.get("P"), T=self._T)
        self._settings = capi.default_settings(self._lib, **kw)
        self.limits = limits(self._lib)
        self._h = self._lib.scs_amd_small_init(ct.byref(self._prob.data), ct.byref(self._prob.k), ct.byref(self._settings))
        if not self._h:
            self._fail("scs_amd_small_init", ValueError("scs_amd_small_init: failed (no HIP device, or a HIP error: see stderr)"))

    def _fail(self, entry, otherwise):
        """a call of `entry` that did not return 0: ValueError with the library's message where it refused, else `otherwise`"""
        why = self._lib.scs_amd_small_refusal()
        raise ValueError(f"{entry}: {why.decode()}") if why else otherwise

    @property
    def n(self):
        return self._prob.n

    @property
    def m(self):
        return self._prob.m

    def _values(self, M, which):
        """K matrices on the object's pattern, or an nnz x K array (a 1-D array is one problem) -> nnz x K, column-major"""
        f = self._T.np_float
        if isinstance(M, (list, tuple)):
            if len(M) < 1:
                raise ValueError(f"{which}: an empty list of matrices")
            cols = [self._prob.values_of(Mk, which) for Mk in M]
            return np.asfortranarray(np.column_stack(cols))
        try:
            V = np.asarray(M, dtype=f)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{which}: a list of matrices or an nnz x K array of values: {e}") from None
        if V.ndim == 1:
            V = V[:, None]
        nnz = len(self._prob.Ax if which == "A" else self._prob.Px)
        if V.ndim != 2 or V.shape[0] != nnz or V.shape[1] < 1:
            raise ValueError(f"{which} values must be nnz x K = {nnz} x K with K >= 1, in the CSC order of the object's pattern")
        return np.asfortranarray(V)

    def set_values(self, A, P=None):
        """Own values of A (and P) for K problems on the pattern the object was built with: lists of K scipy matrices (checked
        against the pattern, explicit zeros included), or nnz x K arrays of values in CSC order.  P exactly when the object has
        one.  Replaces the values of an earlier call.  ValueError on a pattern mismatch, a wrong K, or whatever the library
        refuses; RuntimeError when the call failed on the device."""
        if not self._h:
            raise RuntimeError("batch was closed")
        T = self._T
        if (P is not None) != (self._prob.matP is not None):
            raise ValueError("P must be given exactly when the batch was built with a P")
        AX = self._values(A, "A")
        PX = self._values(P, "P") if P is not None else None
        K = AX.shape[1]
        if PX is not None and PX.shape[1] != K:
            raise ValueError(f"A holds {K} problems and P {PX.shape[1]}")
        rc = self._lib.scs_amd_small_set_values(self._h, K, AX.ctypes.data_as(T.fp), max(1, AX.shape[0]),
                                                PX.ctypes.data_as(T.fp) if PX is not None else None,
                                                max(1, PX.shape[0]) if PX is not None else 0)
        if rc != 0:
            self._nvalues = 0
            self._fail("scs_amd_small_set_values", RuntimeError("scs_amd_small_set_values failed on the device (see stderr)"))
        self._nvalues = K

    def free_values(self):
        """release the own values; the shared `solve` is not affected"""
        if self._h:
            self._lib.scs_amd_small_free_values(self._h)
        self._nvalues = 0

    def solve(self, B, C, warm=None, own_values=False, A=None, P=None):
        """B: m x K, C: n x K (anything numpy turns into 2-D arrays of finite numbers; a 1-D array is one problem).  warm: (X, Y, S)
        of shapes n x K, m x K, m x K, the warm start of every problem, or None.  own_values: problem k under the k-th values of
        the last `set_values` (K must be that call's); A=, P=: `set_values(A, P)` once B, C and warm have passed their checks (a bad
        B leaves the values of an earlier set_values in place), then that solve.  Returns K dicts(x, y, s, info).  ValueError on a wrong shape, a non-numeric dtype, non-finite values, or whatever the library refuses (with its
        message); RuntimeError when the call failed on the device."""
        if not self._h:
            raise RuntimeError("batch was closed")
        if A is None and P is not None:
            raise ValueError("P= needs A=: the values of both are per problem")
        T, f = self._T, self._T.np_float
        n, m = self._prob.n, self._prob.m
        try:
            B = np.asarray(B, dtype=f)
            Cc = np.asarray(C, dtype=f)
        except (TypeError, ValueError) as e:
            raise ValueError(f"B and C must be numeric arrays: {e}") from None
        if B.ndim == 1 and Cc.ndim == 1:
            B, Cc = B[:, None], Cc[:, None]
        if B.ndim != 2 or Cc.ndim != 2 or B.shape[0] != m or Cc.shape[0] != n or B.shape[1] != Cc.shape[1] or B.shape[1] < 1:
            raise ValueError(f"B must be m x K = {m} x K and C n x K = {n} x K with the same K >= 1")
        if not (np.all(np.isfinite(B)) and np.all(np.isfinite(Cc))):
            raise ValueError("B and C must be finite")
        B, Cc = np.asfortranarray(B), np.asfortranarray(Cc)
        K = B.shape[1]
        if warm is not None:
            if len(warm) != 3:
                raise ValueError("warm must be (X, Y, S)")
            blocks = []
            for src, nm, rows in zip(warm, "XYS", (n, m, m)):
                src = np.asarray(src, dtype=f)
                src = src[:, None] if src.ndim == 1 else src
                if src.shape != (rows, K):
                    raise ValueError(f"warm {nm} must have shape {(rows, K)}")
                blocks.append(src)
            warm = blocks
        blk = capi.SolutionBlock(T, n, m, K, warm)
        if A is not None:  # after B, C and warm have passed: a refused call leaves the values of an earlier set_values in place
            self.set_values(A, P)
            own_values = True
        if own_values and self._nvalues and K != self._nvalues:
            raise ValueError(f"B and C hold {K} problems, but the values were set for {self._nvalues}")
        entry = self._lib.scs_amd_small_solve_values if own_values else self._lib.scs_amd_small_solve
        rc = entry(self._h, K, B.ctypes.data_as(T.fp), m, Cc.ctypes.data_as(T.fp), n, blk.sols, blk.infos,
                   1 if warm is not None else 0)
        if rc != 0:
            name = "scs_amd_small_solve_values" if own_values else "scs_amd_small_solve"
            self._fail(name, RuntimeError(f"{name} failed on the device (see stderr)"))
        return blk.results()

    def set_grid(self, workgroups):
        """the number of workgroups of the following launches; 0: the default (what the chip holds at once)"""
        if not self._h:
            raise RuntimeError("batch was closed")
        if isinstance(workgroups, bool) or not isinstance(workgroups, (int, np.integer)) or \
                self._lib.scs_amd_small_set_grid(self._h, int(workgroups)) != 0:
            raise ValueError("workgroups must be an integer in 0 .. 1048576")

    def counters(self):
        """summed over the object's life: launches, workgroups, problems, iterations"""
        out = (ct.c_longlong * 4)()
        if self._h:
            self._lib.scs_amd_small_get_counters(self._h, ct.byref(out))
        return dict(zip(("launches", "workgroups", "problems", "iterations"), (int(v) for v in out)))

    def occupancy(self):
        """workgroups per CU, LDS bytes per workgroup (both 0 before the first solve) and the default grid, the setup time in seconds,
        and the instantiation chosen at init: block_threads 256 / 1024, kernel 'narrow' / 'wide'"""
        out = (ct.c_longlong * 5)()
        if self._h:
            self._lib.scs_amd_small_get_occupancy(self._h, ct.byref(out))
        return dict(wg_per_cu=int(out[0]), lds_bytes=int(out[1]), default_grid=int(out[2]), setup_s=int(out[3]) / 1e6,
                    block_threads=int(out[4]), kernel={256: "narrow", 1024: "wide"}.get(int(out[4])))

    def close(self):
        if self._h:
            self._lib.scs_amd_small_finish(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
