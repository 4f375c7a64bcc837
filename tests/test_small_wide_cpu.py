"""The wide instantiation of the small batch: what needs no GPU.  The limits, the sizes init accepts beyond the narrow limits
(refused before the wide kernel existed), the refusals over the new limits, the field of scs_amd_small_get_occupancy that names
the instantiation (chosen at init, so known without a device), and the exports.
test_the_reference_alone_is_stable_on_the_seeds runs no code of the library: it checks the seeds of tests/small_wide_util.py where
oracle/_ref is built."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, small
from scs_amd.small import SmallBatch
from tests import small_wide_util as W

OK = dict(verbose=0, adaptive_scale=0, acceleration_lookback=0)
SMALL_ENTRIES = {"scs_amd_small_init", "scs_amd_small_refusal", "scs_amd_small_limits", "scs_amd_small_solve", "scs_amd_small_set_grid",
                 "scs_amd_small_get_counters", "scs_amd_small_get_occupancy", "scs_amd_small_finish", "scs_amd_small_set_values",
                 "scs_amd_small_solve_values", "scs_amd_small_free_values"}


def _lib():
    return capi.load("libscsamd.so")


def _prob(n, m, seed=0):
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(rng.uniform(-1, 1, (m, n)) * (rng.uniform(0, 1, (m, n)) < 0.2) + np.eye(m, n))
    return capi.Problem(A, rng.uniform(-1, 1, m), rng.uniform(-1, 1, n), dict(z=2, l=m - 2))


def _init(prob):
    lib = _lib()
    st = capi.default_settings(lib, **OK)
    h = lib.scs_amd_small_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    why = lib.scs_amd_small_refusal()
    return h, (why.decode() if why else None)


def _occupancy(h):
    out = (C.c_longlong * 5)()
    _lib().scs_amd_small_get_occupancy(h, C.byref(out))
    return list(out)


def test_the_limits_are_512_and_2304():
    """at (n, m) = (512, 1791) the wide kernel's LDS is 6 l + 2 m + 3 n + 1024 + 16 = 19982 values, 159 856 B of a CU's 163 840"""
    assert small.limits() == (512, 2304)
    for lib in ("libscsamd_f32.so", "libscsamd_dlong.so"):
        assert small.limits(capi.load(lib)) == (512, 2304)


@pytest.mark.parametrize("n,m", [(129, 258), (8, 1016)])
def test_init_accepts_the_first_sizes_over_the_narrow_limits(n, m):
    """n = 129, and n + m + 1 = 1025 with a small n: both run the wide instantiation, which init says without a device"""
    h, why = _init(_prob(n, m))
    assert h and why is None, why
    occ = _occupancy(h)
    assert occ[:2] == [0, 0] and occ[4] == 1024  # nothing of the device before a solve; the choice is made
    _lib().scs_amd_small_finish(h)


def test_init_refuses_sizes_over_the_new_limits():
    for prob, words in ((_prob(513, 520), ("n =", "513", "512")), (_prob(8, 2296), ("n + m + 1 =", "2305", "2304"))):
        h, why = _init(prob)
        assert not h and why and all(w in why for w in words), why
    h, why = _init(_prob(8, 2295))  # exactly at the limit: served
    assert h and why is None
    _lib().scs_amd_small_finish(h)


@pytest.mark.parametrize("n,m,block,kernel", [(4, 8, 256, "narrow"), (128, 895, 256, "narrow"), (128, 896, 1024, "wide"),
                                              (129, 130, 1024, "wide")])
def test_the_occupancy_names_the_instantiation(n, m, block, kernel):
    """n <= 128 and n + m + 1 <= 1024: narrow; anything else: wide.  No device is needed and no solve has run."""
    h, why = _init(_prob(n, m))
    assert h, why
    assert _occupancy(h)[4] == block
    _lib().scs_amd_small_finish(h)
    pr = _prob(n, m)
    A = sp.csc_matrix((pr.Ax, pr.Ai, pr.Ap), shape=(m, n))
    with SmallBatch(dict(A=A, b=np.zeros(m), c=np.zeros(n)), dict(z=2, l=m - 2)) as sb:
        occ = sb.occupancy()
        assert occ["block_threads"] == block and occ["kernel"] == kernel
        assert occ["wg_per_cu"] == occ["lds_bytes"] == 0
    assert sb.occupancy()["kernel"] is None  # closed: nothing to report


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path(lib)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_exports_are_unchanged():
    """the wide kernel adds no entry: the small batch exports what it exported, and the two partial libraries none of it"""
    for lib in ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so"):
        assert {s for s in _exported(lib) if s.startswith("scs_amd_small")} == SMALL_ENTRIES, lib
    for lib in ("libscsamd_linsys.so", "libscsamd_cones.so"):
        assert not {s for s in _exported(lib) if s.startswith("scs_amd_small")}, lib


def _refs():
    from oracle import pyoracle
    for lib in ("libscsindir_ref_exactcg.so", "libscsindir_ref_exactcg_omp.so"):
        if not pyoracle.ref_available(lib):
            pytest.skip(f"oracle/_ref/{lib} not built")
    return pyoracle.load_ref("libscsindir_ref_exactcg.so"), pyoracle.load_ref("libscsindir_ref_exactcg_omp.so")


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_the_reference_alone_is_stable_on_the_seeds(name):
    """the serial and the OpenMP build of the exact-solve reference agree on iter and status_val in every column of every GPU case,
    with the K and the max_iters the GPU tests use"""
    from tests import small_batch_util as U
    ref, omp = _refs()
    a, b = W.reference_case(ref, name), U.reference_columns(omp, *W.case(name))
    its = [(r["info"]["iter"], r["info"]["status_val"]) for r in a]
    print(name, its)
    assert W.agree(a, b), (name, its, [(r["info"]["iter"], r["info"]["status_val"]) for r in b])
    if "max_iters" not in W.CASES[name][7]:
        assert all(r["info"]["status_val"] == 1 for r in a), (name, its)


def test_the_reference_alone_is_stable_on_the_mixed_statuses():
    """the wide mixed-status list: infeasible, unbounded, solved, solved in both builds, with the same iteration counts"""
    from tests import small_batch_util as U
    ref, omp = _refs()
    A, cone, B, Cc = W.mixed_statuses_wide()
    a, b = (U.reference_columns(lib, A, None, cone, B, Cc, U.SETTINGS) for lib in (ref, omp))
    assert [r["info"]["status_val"] for r in a] == [-2, -1, 1, 1] and W.agree(a, b)


@pytest.mark.parametrize("name", ["w_n129"])
def test_the_reference_alone_is_stable_on_the_derived_seeds(name):
    """the same with a fresh scs_init per problem on the problems' own values (the derived case the GPU tests hold to the reference)"""
    from tests import small_values_util as V
    ref, omp = _refs()
    a, b = W.reference_derived(ref, name), V.fresh_columns(omp, *W.derived(name))
    its = [(r["info"]["iter"], r["info"]["status_val"]) for r in a]
    print(name, its)
    assert W.agree(a, b), (name, its)
