"""The paced PCG enqueue loop (option cg_pace, scs_amd/csrc/linsys.hip: solve_dev): the host keeps the queue
at most `cg_lead` quanta ahead of the iteration count the device publishes in a host-visible word, instead of enqueuing a guessed
batch and blocking on a read-back.  The same kernels run in the same order on the same data, so everything below is compared
with cg_pace=0 (the batch loop) for EQUALITY: solutions bit for bit, iteration counts, cg_iters, mat_vecs.

The counter conditions are caps that follow from the loop's rule, not measurements: with cg_pace=1 nothing inside a linear solve
blocks, and a solve enqueues at most `lead` quanta more than the device executes -- `lead` iterations on the launch path,
lead * 8 + 7 on the graph path (whole graphs of 8), one more where the stop test of an iteration runs in the next iteration's
first launch (the two- and three-launch iterations)."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

from scs_amd import capi, problems
from tests import probgen

pytestmark = pytest.mark.gpu

GRAPH_ITERS = 8  # CG_GRAPH_ITERS of linsys.hip
LEAD_DEFAULT = 4


@contextlib.contextmanager
def _options(**kv):
    """Options are process-wide and read when a workspace is created: set, create and use the workspaces, restore."""
    try:
        for k, v in kv.items():
            capi.set_option(k, v)
        yield
    finally:
        for k in kv:
            capi.set_option(k, None)


def _pacing(lib, w, linsys=False):
    out = (C.c_longlong * 4)()
    (lib.scs_amd_linsys_get_cg_pacing if linsys else lib.scs_amd_get_cg_pacing)(w, C.byref(out))
    return dict(enq=out[0], done=out[1], syncs=out[2], solves=out[3])


def _slack(lead, graph, extra=0):
    """most iterations a solve may enqueue beyond the ones the device executes"""
    return (lead * GRAPH_ITERS + GRAPH_ITERS - 1 if graph else lead) + extra


# ---- whole solves -------------------------------------------------------------------------------------------------------------------
def _scs(lib, prob, profiling=False, resolve_warm=False, cg_tol_override=None, **over):
    """scs_init, scs_solve (and optionally a warm-started second scs_solve on the same workspace), counters, scs_finish"""
    T = lib._scs_types
    st = capi.default_settings(lib, **over)
    x, y, s = (np.zeros(k, dtype=T.np_float) for k in (prob.n, prob.m, prob.m))
    sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
    info = T.ScsInfo()
    w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    assert w
    try:
        if profiling:
            lib.scs_amd_set_profiling(w, 1)
        if cg_tol_override is not None:
            lib.scs_amd_set_cg_tol_override(w, float(cg_tol_override))
        lib.scs_solve(w, C.byref(sol), C.byref(info), 0)
        runs = [dict(x=x.copy(), y=y.copy(), s=s.copy(), iter=info.iter, status=info.status_val)]
        if resolve_warm:
            lib.scs_solve(w, C.byref(sol), C.byref(info), 1)
            runs.append(dict(x=x.copy(), y=y.copy(), s=s.copy(), iter=info.iter, status=info.status_val))
        stt = T.ScsAmdStats()
        lib.scs_amd_get_stats(w, C.byref(stt))
        return dict(runs=runs, cg_iters=stt.cg_iters, mat_vecs=stt.mat_vecs, solves=stt.lin_sys_solves, pace=_pacing(lib, w))
    finally:
        lib.scs_finish(w)


def _bits(a, b):
    """bit for bit (np.array_equal would call two runs that both ended in the same NaNs different)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same(a, b):
    assert len(a["runs"]) == len(b["runs"])
    for ra, rb in zip(a["runs"], b["runs"]):
        assert ra["iter"] == rb["iter"] and ra["status"] == rb["status"]
        for k in ("x", "y", "s"):
            assert _bits(ra[k], rb[k]), k
    assert a["cg_iters"] == b["cg_iters"] and a["mat_vecs"] == b["mat_vecs"] and a["solves"] == b["solves"]


@pytest.fixture(scope="module")
def small():
    """n just above the two-launch threshold (1024), below the wave layout: the four plain launches per iteration"""
    pr = problems.random_socp(1500, 3000, 4, seed=21)
    return capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])


KW = dict(verbose=0, acceleration_lookback=0, max_iters=120)


@pytest.mark.parametrize("name,opts,profiling,lead,graph", [
    ("launches", dict(graph="0"), False, LEAD_DEFAULT, False),
    ("graph", dict(), False, LEAD_DEFAULT, True),
    ("profiling", dict(), True, LEAD_DEFAULT, False),  # event-timed solves launch kernel by kernel
    ("lead1", dict(graph="0", cg_lead="1"), False, 1, False),
    ("lead16", dict(graph="0", cg_lead="16"), False, 16, False),
    ("graph_lead1", dict(cg_lead="1"), False, 1, True),
    ("graph_lead16", dict(cg_lead="16"), False, 16, True),
])
def test_paced_solve_equals_the_batch_loop_bit_for_bit(small, name, opts, profiling, lead, graph):
    amd = capi.load("libscsamd.so")
    with _options(cg_pace="0", **opts):
        ref = _scs(amd, small, profiling=profiling, **KW)
    with _options(cg_pace="1", **opts):
        got = _scs(amd, small, profiling=profiling, **KW)
    _same(ref, got)
    assert ref["pace"]["syncs"] >= ref["solves"] > 0  # the batch loop blocks at least once per linear solve
    p = got["pace"]
    print(name, "batch loop:", ref["pace"], "paced:", p)
    assert p["syncs"] == 0
    assert p["solves"] == got["solves"] and p["done"] == got["cg_iters"]
    assert 0 <= p["enq"] - p["done"] <= p["solves"] * _slack(lead, graph)


def test_a_warm_started_second_solve_does_not_read_the_first_ones_last_word(small):
    amd = capi.load("libscsamd.so")
    with _options(cg_pace="0"):
        ref = _scs(amd, small, resolve_warm=True, **KW)
    with _options(cg_pace="1"):
        got = _scs(amd, small, resolve_warm=True, **KW)
    assert len(got["runs"]) == 2
    _same(ref, got)
    assert got["pace"]["syncs"] == 0


def test_a_tolerance_only_the_iteration_cap_ends():
    """cg_tol_override far below what fp64 reaches on a tiny system: every linear solve runs into the cap of 10 n iterations
    (private.c:307), which the device enforces and publishes; forced off the one-workgroup kernel so that the enqueue loop is what runs"""
    amd = capi.load("libscsamd.so")
    pr = problems.random_socp(24, 48, 3, seed=5)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    kw = dict(verbose=0, acceleration_lookback=0, max_iters=4, cg_tol_override=1e-300)
    for opts in (dict(fused="0", cg2="0"), dict(fused="0"), dict()):
        with _options(cg_pace="0", **opts):
            ref = _scs(amd, prob, **kw)
        with _options(cg_pace="1", **opts):
            got = _scs(amd, prob, **kw)
        _same(ref, got)
        assert got["cg_iters"] > 0 and got["pace"]["syncs"] == 0


def test_two_workspaces_on_two_host_threads(small):
    """as batch_workload runs them: each thread paces its own workspace by its own word on its own stream"""
    amd = capi.load("libscsamd.so")
    pr = problems.random_socp(1700, 3300, 4, seed=22)
    other = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    probs = [small, other]
    with _options(cg_pace="1"):
        serial = [_scs(amd, p, **KW) for p in probs]
        par = [None, None]

        def run(i):
            par[i] = _scs(amd, probs[i], **KW)
        ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    for a, b in zip(serial, par):
        assert b is not None
        _same(a, b)
        assert b["pace"]["syncs"] == 0


# ---- direct linear solves ---------------------------------------------------------------------------------------------------------
def _linsys_cases(lib, n, m, col_nnz, lead, graph, extra, paced):
    """one workspace; the three solves whose `done` comes from another kernel than the iteration's, and an ordinary one.
    Returns the solutions and iteration counts; with `paced`, checks the counters of every single solve."""
    T = lib._scs_types
    A = probgen.random_csc(m, n, col_nnz, seed=3)
    prob = capi.Problem(A, np.zeros(m), np.zeros(n), dict(l=m))
    dr = probgen.diag_r(n, m, z=m // 10)
    rng = np.random.default_rng(n)
    b = rng.uniform(-1, 1, n + m)
    w = lib.scs_init_lin_sys_work(C.byref(prob.matA), None, dr.ctypes.data_as(T.fp))
    assert w
    res = []

    def solve(rhs, s, tol):
        before = _pacing(lib, w, linsys=True)
        out = rhs.copy()
        assert lib.scs_solve_lin_sys(w, out.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp) if s is not None else None, tol) == 0
        after = _pacing(lib, w, linsys=True)
        its = after["done"] - before["done"]
        assert after["solves"] - before["solves"] == 1
        if paced:
            assert after["syncs"] == 0
            over = (after["enq"] - before["enq"]) - its
            assert over <= _slack(lead, graph, extra), (over, its)
        res.append((out, its))
        return out, its

    try:
        x, its = solve(b, None, 1e-12)                    # ordinary: done published by the iteration's own kernel
        assert its > 1
        _, its0 = solve(np.full(n + m, 1e-13), None, 1e-9)  # zero right-hand side: k_rhs_prep, 0 iterations (private.c:296-299)
        assert its0 == 0
        _, itw = solve(b, x[:n].copy(), 1e-6)              # warm start equal to the solution: k_cg_start (private.c:163)
        assert itw == 0
        if n <= 64:
            _, itc = solve(b, None, 1e-300)                # nothing but the cap of 10 n iterations (or an exact breakdown) ends this
            assert itc <= 10 * n
        solve(b, None, 1e-5)                               # and an ordinary solve after all of them, on the same word
    finally:
        lib.scs_free_lin_sys_work(w)
    return res


@pytest.mark.parametrize("name,n,m,col_nnz,opts,graph,extra", [
    ("fused", 20, 60, 3, dict(), False, 0),                              # one workgroup: the device's own loop, one word at its end
    ("two_launch", 20, 60, 3, dict(fused="0"), True, 1),
    ("two_launch_no_graph", 600, 1500, 4, dict(fused="0", graph="0"), False, 1),
    ("four_launch_tiny", 20, 60, 3, dict(fused="0", cg2="0", graph="0"), False, 0),
    ("four_launch", 1500, 3000, 4, dict(graph="0"), False, 0),
    ("four_launch_graph", 1500, 3000, 4, dict(), True, 0),
    ("four_launch_strided", 1500, 3000, 4, dict(graph="0", vec_max_grid="2"), False, 0),
    ("wave_rows", 30000, 70001, 7, dict(waverows="1", graph="0"), False, 0),
    ("three_launch", 30000, 70001, 7, dict(waverows="1", cg3="1"), False, 1),
])
@pytest.mark.parametrize("lead", [1, LEAD_DEFAULT])
def test_linear_solves_equal_the_batch_loop(name, n, m, col_nnz, opts, graph, extra, lead):
    amd = capi.load("libscsamd_linsys.so")
    with _options(cg_pace="0", **opts):
        ref = _linsys_cases(amd, n, m, col_nnz, lead, graph, extra, paced=False)
    with _options(cg_pace="1", cg_lead=str(lead), **opts):
        got = _linsys_cases(amd, n, m, col_nnz, lead, graph, extra, paced=True)
    assert len(ref) == len(got)
    for (xa, ia), (xb, ib) in zip(ref, got):
        assert ia == ib
        assert _bits(xa, xb)
