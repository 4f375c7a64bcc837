"""The host side of "new values on the same pattern" (scs_amd_update_matrix, scs_amd_linsys_update_values; include/scs_amd.h): what
each library exports, the refusals that need no device, and the entry permutation that goes with the renumbering of reorder.h --
against scipy's own permutation of the matrix, for both ways scs_init comes by the renumbered matrix, and under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scs_amd import capi, problems

FULL = ("scs_amd_update_matrix", "scs_amd_linsys_update_values", "scs_amd_plan_reorder_entries")
CONE_NINE = {"_scs_init_cone", "_scs_proj_dual_cone", "_scs_finish_cone", "_scs_set_r_y", "_scs_enforce_cone_boundaries",
             "_scs_validate_cones", "_scs_get_cone_header", "_scs_deep_copy_cone", "_scs_free_cone"}


def _exported(name):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path(name)], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.mark.parametrize("name", ["libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so"])
def test_full_libraries_export_the_update_entries(name):
    L = capi.load(name)
    for fn in FULL:
        assert hasattr(L, fn), (name, fn)


def test_linsys_library_exports_the_linsys_level_entry_only_and_the_cones_library_keeps_its_nine():
    if not shutil.which("nm"):
        pytest.skip("nm not on PATH")
    lin = _exported("libscsamd_linsys.so")
    assert "scs_amd_linsys_update_values" in lin
    assert "scs_amd_update_matrix" not in lin and "scs_amd_plan_reorder_entries" not in lin
    cones = _exported("libscsamd_cones.so")
    assert {s for s in cones if s.startswith("_scs_")} == CONE_NINE
    assert not any("update" in s for s in cones)


def test_null_workspaces_are_refused_without_a_device():
    v = np.ones(3)
    p = v.ctypes.data_as(capi.T64.fp)
    assert capi.load("libscsamd.so").scs_amd_update_matrix(None, p, None) == -1
    assert capi.load("libscsamd.so").scs_amd_update_matrix(None, None, None) == -1
    for name in ("libscsamd.so", "libscsamd_linsys.so"):
        assert capi.load(name).scs_amd_linsys_update_values(None, p, None) == -1
    v32 = np.ones(3, np.float32)
    assert capi.load("libscsamd_f32.so").scs_amd_update_matrix(None, v32.ctypes.data_as(capi.T32.fp), None) == -1
    assert capi.load("libscsamd_dlong.so").scs_amd_update_matrix(None, p, None) == -1


def _entries(lib, A, cone):
    T = lib._scs_types
    prob = capi.Problem(A, np.zeros(A.shape[0]), np.zeros(A.shape[1]), cone, T=T)
    cp, rp = np.zeros(prob.n, dtype=T.np_int), np.zeros(prob.m, dtype=T.np_int)
    ent = np.full(len(prob.Ax), -1, dtype=T.np_int)
    info = (C.c_double * 7)()
    rc = lib.scs_amd_plan_reorder_entries(C.byref(prob.matA), C.byref(prob.k), cp.ctypes.data_as(T.ip), rp.ctypes.data_as(T.ip),
                                          ent.ctypes.data_as(T.ip), info)
    return rc, list(info), cp, rp, ent, prob


def _check_against_scipy(prob, cp, rp, ent):
    """A.data[entry_new2old] is the data of A[row_new2old][:, col_new2old] with sorted indices"""
    A = prob.sparse()
    A.data = np.arange(1, A.nnz + 1, dtype=np.float64)  # every entry its own value: a wrong source cannot hide
    want = sp.csc_matrix(A[rp][:, cp])
    want.sort_indices()
    assert sorted(ent) == list(range(A.nnz))
    assert np.array_equal(A.data[ent], want.data)


@pytest.mark.parametrize("lib_name", ["libscsamd.so", "libscsamd_dlong.so"])
@pytest.mark.parametrize("pattern", ["banded", "random"])
def test_entry_permutation_equals_scipys_for_both_ways_the_renumbered_matrix_is_built(monkeypatch, pattern, lib_name):
    """a scrambled banded pattern keeps an anchored numbering and apply_reorder builds the matrix afterwards; a uniformly random one gets
    the chain + home numbering, whose matrix is built beside the measurement (info[6]); an empty column and an empty row in both"""
    monkeypatch.setenv("SCS_AMD_REORDER", "1")
    lib = capi.load(lib_name)
    n, m = 6000, 12000
    pr = problems.random_socp(n, m, 8, seed=5, band=256, scramble=9) if pattern == "banded" else problems.random_socp(n, m, 8, seed=5)
    A = pr["A"].tolil()
    A[:, 17] = 0      # an empty column
    A[5, :] = 0       # an empty row (zero cone)
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    assert A.indptr[18] == A.indptr[17] and A.tocsr().indptr[6] == A.tocsr().indptr[5]
    rc, info, cp, rp, ent, prob = _entries(lib, A, pr["cone"])
    assert rc == 1 and info[0] == 1.0
    assert info[6] == (0.0 if pattern == "banded" else 1.0), info  # which of the two ways ran
    assert sorted(cp) == list(range(n)) and sorted(rp) == list(range(m))
    _check_against_scipy(prob, cp, rp, ent)


def test_identity_when_nothing_is_kept(monkeypatch):
    monkeypatch.setenv("SCS_AMD_REORDER", "0")
    lib = capi.load("libscsamd.so")
    pr = problems.random_socp(500, 1200, 6, seed=3, band=64, scramble=2)
    rc, info, cp, rp, ent, prob = _entries(lib, pr["A"], pr["cone"])
    assert rc == 0 and info[0] == 0.0
    assert np.array_equal(ent, np.arange(len(ent))) and np.array_equal(cp, np.arange(prob.n)) and np.array_equal(rp, np.arange(prob.m))


def test_values_of_checks_the_pattern_after_the_constructors_canonicalisation():
    pr = problems.random_socp(50, 120, 4, seed=1)
    prob = capi.Problem(pr["A"], pr["b"], pr["c"], pr["cone"])
    A = pr["A"]
    shuffled = sp.coo_matrix(A)
    order = np.random.default_rng(0).permutation(A.nnz)
    shuffled = sp.coo_matrix((shuffled.data[order] * 2.0, (shuffled.row[order], shuffled.col[order])), shape=A.shape)
    got = prob.values_of(shuffled)  # another storage order of the same pattern: canonicalised like the constructor's input
    assert np.array_equal(got, prob.Ax * 2.0)
    assert np.array_equal(prob.values_of(np.arange(A.nnz)), np.arange(A.nnz, dtype=np.float64))
    other = A.tolil(copy=True)
    i, j = [(i, j) for i in range(6) for j in range(6) if A[i, j] == 0][0]
    other[i, j] = 3.0
    for bad in (other.tocsc(), A[:, :-1], np.ones(A.nnz - 1), np.ones((A.nnz, 1))):
        with pytest.raises(ValueError):
            prob.values_of(bad)
    with pytest.raises(ValueError):
        prob.values_of(np.ones(3), "P")  # no P


def test_host_half_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/native/host_sanitize_update.cpp: the entry permutation, the finiteness check and the value permutation, compiled for the HOST
    alone (--cuda-host-only, the sanitizers passed as host options) with AddressSanitizer + UBSan, on random mixed-cone patterns with
    empty columns, a matrix without entries and entry positions at the top of their type's range"""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "drv")
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", os.path.join(here, "native", "host_sanitize_update.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    env = {k: v for k, v in os.environ.items() if k != "SCS_AMD_REORDER"}
    env["SCS_AMD_REORDER"] = "1"
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "sanitizer driver ok" in out.stdout, out.stdout[-3000:]
    assert "ERROR: " not in out.stdout and "runtime error" not in out.stdout, out.stdout[-3000:]
    kept, ready = [int(t) for t in out.stdout.split("kept ")[1].split() if t.isdigit()][:2]
    assert kept > 5 and 0 < ready < kept, out.stdout[-500:]  # both ways of building the renumbered matrix were exercised
