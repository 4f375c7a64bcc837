"""Device equilibration (scs_amd/csrc/equilibrate_dev.hip, `where = 1` of scs_amd_equilibrate) against the host code
(`where = 0`) on the edge shapes of tests/equilibrate_cases.py, for the fp64, the fp32 and the 64-bit-index library.  Bit identity
is the device file's stated contract, so every comparison is np.array_equal.  The host code itself is held to the reference on the
same cases by tests/test_equilibrate_edges_cpu.py; profiles/equilibrate_edges.md says which kernel or branch each case reaches."""
import numpy as np
import pytest

from scs_amd import capi
from tests import equilibrate_cases as ec
from tests.test_equilibrate import _equilibrate_raw

pytestmark = pytest.mark.gpu

LIBS = ("libscsamd.so", "libscsamd_f32.so", "libscsamd_dlong.so")


def _run(lib, case, where):
    return _equilibrate_raw(lib, case.m, case.n, (case.Ap, case.Ai, case.Ax), case.P, case.cone, where)


def _assert_same_bits(a, b, what):
    for x, y, name in zip(a, b, ("A.x", "P.x", "D", "E")):
        if x is None:
            assert y is None
            continue
        assert x.dtype == y.dtype and np.array_equal(x, y), what + (name, int((x != y).sum()), np.abs(x - y).max())


@pytest.mark.parametrize("name", ec.NAMES)
@pytest.mark.parametrize("libname", LIBS)
def test_device_equilibration_is_bit_identical_to_host_on_edge_shapes(libname, name):
    lib = capi.load(libname)
    case = ec.build(name)
    assert lib._scs_types.np_int == (np.int64 if libname.endswith("_dlong.so") else np.int32)
    _assert_same_bits(_run(lib, case, 0), _run(lib, case, 1), (libname, name))


@pytest.mark.parametrize("libname", LIBS)
def test_row_lengths_with_the_transpose_verified_against_the_host_loop(monkeypatch, libname):
    """SCS_AMD_TRANSPOSE=verify: the device-built pattern (one-lane sort up to 32 entries, bitonic sort in LDS at 33, 64, 65, 1000
    and 4096) is compared with the host's counting sort inside the library, which refuses the call when they differ"""
    lib = capi.load(libname)
    case = ec.build("row_lengths")
    host = _run(lib, case, 0)
    monkeypatch.setenv("SCS_AMD_TRANSPOSE", "verify")
    _assert_same_bits(host, _run(lib, case, 1), (libname, "row_lengths", "verify"))


@pytest.mark.parametrize("name", ["row_lengths", "segments"])
@pytest.mark.parametrize("libname", LIBS)
def test_two_device_runs_agree_bit_for_bit(libname, name):
    """the transpose hands out a row's slots by atomics, in whatever order the lanes arrive; only the sort makes the result order-free"""
    lib = capi.load(libname)
    case = ec.build(name)
    _assert_same_bits(_run(lib, case, 1), _run(lib, case, 1), (libname, name, "run 1 against run 2"))
