"""The time-limit end of the family loops (scs_amd_solve_family, scs_amd_solve_family_scaled, scs_amd_solve_family_stream).

With time_limit_secs = 1e-9 every clock has run out at the first check, so the reference (src/scs.c:1404-1413), the chunk loop and
the stream loop all stop there, deterministically: one iteration is run, iter = 0, and the status carries the time-limit suffix.
The reference is driven column by column with the same settings; the stream's yardstick is, as everywhere, the chunk entry at the
stream's width (tests/test_family_stream_gpu.py)."""
import numpy as np
import pytest

from scs_amd import capi
from tests.family_util import Work, family_data
from tests.test_family_gpu import _assert_same_as_reference, _ref, _socp
from tests.test_family_stream_gpu import _expected, _same, _shared, counters, stream

pytestmark = pytest.mark.gpu
SUFFIX = "(inaccurate - reached time_limit_secs)"
KW = dict(verbose=0, acceleration_lookback=0, time_limit_secs=1e-9)


@pytest.fixture(scope="module")
def small():
    pr, prob = _socp(60, 150, 5, 3)
    B, Cc = family_data(pr["A"], pr["cone"], 5, seed=8)
    return prob, B, Cc


@pytest.fixture(scope="module")
def ref_cols(small):
    """the reference on the five problems, one after the other, per adaptive_scale (no scale update happens before the first check)"""
    prob, B, Cc = small
    out = {}
    for adaptive in (0, 1):
        with Work(_ref(), prob, adaptive_scale=adaptive, **KW) as wr:
            out[adaptive] = wr.solve_columns(B, Cc)
    return out


def _assert_stopped_at_the_first_check(rc, got, ref):
    assert rc == 0
    print([(r["info"]["iter"], r["info"]["status"]) for r in got])
    assert all(r["info"]["iter"] == 0 for r in got)
    assert all(r["info"]["status"].endswith(SUFFIX) for r in got)
    _assert_same_as_reference(got, ref)


@pytest.mark.parametrize("scaled", [False, True])
def test_a_chunk_stops_at_its_first_check(small, ref_cols, scaled):
    """K = 3: width 4, one padding column; the scaled entry with adaptive_scale = 1 (a timed-out chunk runs no scale update)"""
    amd = capi.load("libscsamd.so")
    prob, B, Cc = small
    B, Cc = np.asfortranarray(B[:, :3]), np.asfortranarray(Cc[:, :3])
    with Work(amd, prob, cg_tol_override=1e-12, adaptive_scale=1 if scaled else 0, **KW) as w:
        rc, got = capi.solve_family_scaled(amd, w.w, B, Cc) if scaled else w.family(B, Cc)
    _assert_stopped_at_the_first_check(rc, got, ref_cols[1 if scaled else 0][:3])
    assert all(r["info"]["scale_updates"] == 0 for r in got)


def test_every_problem_of_a_stream_stops_at_its_own_first_check(small, ref_cols):
    """5 problems through 2 slots, shared scale: every slot is refilled, and a refilled problem's clock starts with its column"""
    amd = capi.load("libscsamd.so")
    prob, B, Cc = small
    with Work(amd, prob, cg_tol_override=1e-12, adaptive_scale=0, **KW) as w:
        want = _expected(B, Cc, 2, _shared(w, B, Cc))
        rc, got = stream(w, B, Cc, width=2)
        cnt = counters(w)
    print(cnt)
    assert cnt["refills"] == 3
    _assert_stopped_at_the_first_check(rc, got, ref_cols[0])
    for p in range(5):
        assert _same(got[p], want[p]), p
