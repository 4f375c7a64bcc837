"""scs_amd_small_solve / scs_amd_small_solve_values with more problems than one launch takes (SB_CHUNK = 32768 in
scs_amd/csrc/small_batch.h): the second pass of the chunk loop, whose problem p of the chunk is problem done + p of the call -- its
columns of B and Cc, its ScsSolution and ScsInfo and, with own values, its blocks of A, A', P, D and E.

The yardstick is exact: a problem's bits depend neither on its index nor on its neighbours, so problem p of a call
that repeats the six problems of a case 32768 + 2 times over (problem p = problem p mod 6) must hold the bits of problem p mod 6 of
the six-problem call.  32768 + 2 is the smallest count whose second chunk holds more than one problem; the case is the smallest of
tests/small_batch_util.py (n = 10, m = 25)."""
import numpy as np
import pytest

from scs_amd.small import SmallBatch
from tests import small_batch_util as U
from tests import small_values_util as V

pytestmark = pytest.mark.gpu

CHUNK = 32768  # SB_CHUNK
COUNT = CHUNK + 2


def _batch(A, P, cone, B, Cc, settings):
    data = dict(A=A, b=B[:, 0], c=Cc[:, 0])
    if P is not None:
        data["P"] = P
    return SmallBatch(data, cone, **settings)


def _tile(M):
    """column p of the result is column p mod K of M (K columns), COUNT columns, column-major"""
    return np.asfortranarray(M[:, np.arange(COUNT) % M.shape[1]])


def _assert_two_launches(before, after):
    assert after["launches"] - before["launches"] == 2
    assert after["problems"] - before["problems"] == COUNT


def test_shared_values_past_one_chunk():
    A, P, cone, B, Cc, st = U.case("a_zl")
    with _batch(A, P, cone, B, Cc, st) as sb:
        six = sb.solve(B, Cc)
        c0 = sb.counters()
        many = sb.solve(_tile(B), _tile(Cc))
        _assert_two_launches(c0, sb.counters())
    assert len(six) == 6 and len(many) == COUNT
    assert all(r["info"]["status_val"] == 1 for r in six)
    bad = [p for p in range(COUNT) if not U.same_bits(many[p], six[p % 6])]
    assert not bad, (len(bad), bad[:8])


def test_own_values_past_one_chunk():
    As, Ps, cone, B, Cc, st = V.derived("a_zl")
    assert Ps is None
    with _batch(As[0], None, cone, B, Cc, st) as sb:
        AX = np.asfortranarray(np.column_stack([sb._prob.values_of(Ap, "A") for Ap in As]))  # nnz x 6
        six = sb.solve(B, Cc, A=AX)
        c0 = sb.counters()
        many = sb.solve(_tile(B), _tile(Cc), A=_tile(AX))
        _assert_two_launches(c0, sb.counters())
    assert len(six) == 6 and len(many) == COUNT
    assert all(r["info"]["status_val"] == 1 for r in six)
    bad = [p for p in range(COUNT) if not U.same_bits(many[p], six[p % 6])]
    assert not bad, (len(bad), bad[:8])
