"""
The host-side pieces of the lock-step sibk that need no device (eigd_amd/adjoint.py): the projection period of the short
recurrence, its frozen / not-converging rules, the round state shared by the four lock-step loops, and the helper that
runs a round on column chunks.
"""
import numpy as np
import pytest

from eigd_amd import tuning
from eigd_amd.adjoint import _by_column_chunks, _cg_frozen, _cg_not_converging, _cg_projection_period, _Modes


# ---- _cg_projection_period: clamp(floor(ln 1e6 / ln max(4 g, 1 + 1e-12)), 1, 4), g = max |1 - (lam_c - s) / (lam_defl - s)|
def _spectrum_with(g):
    """lam_c, lam_defl, sigma with g exactly: sigma = 0, deflated eigenvalues {1, 1 + g}, the column's own 1 + g"""
    return np.array([1.0 + g]), np.array([1.0, 1.0 + g]), 0.0


@pytest.mark.parametrize("g, period", [(0.5, 4), (10.0, 3), (100.0, 2), (1e4, 1)])
def test_projection_period_follows_the_growth_per_step(monkeypatch, g, period):
    monkeypatch.setattr(tuning, "cg_projection_period", 0)
    lam_c, lam_defl, sigma = _spectrum_with(g)
    assert abs(1.0 - (lam_c[0] - sigma) / (lam_defl[0] - sigma)) == g
    assert _cg_projection_period(lam_c, lam_defl, sigma) == period
    monkeypatch.setattr(tuning, "cg_projection_period", 3)
    assert _cg_projection_period(lam_c, lam_defl, sigma) == 3


def test_projection_period_with_a_deflated_eigenvalue_at_the_shift(monkeypatch):
    monkeypatch.setattr(tuning, "cg_projection_period", 0)
    lam = np.array([0.25, 1.0, 2.0])
    assert _cg_projection_period(lam, lam, 0.25) == 1          # g infinite (and 0 / 0 on the diagonal, ignored)
    assert _cg_projection_period(lam[1:], lam, 0.25) == 1
    monkeypatch.setattr(tuning, "cg_projection_period", 3)
    assert _cg_projection_period(lam, lam, 0.25) == 3


# ---- frozen: len >= 3, h[-1] > 0, the last two differences <= 1e-14 relative; not converging: len > 12 and not h[-1] < h[-11] / 2
def test_frozen_needs_three_entries_that_agree_to_1e_minus_14():
    assert not _cg_frozen([1.0, 1.0])                          # length 2
    assert _cg_frozen([1.0, 1.0, 1.0])                         # length 3
    assert _cg_frozen([3.0, 2.0] + [1.0] * 10)                 # length 12
    assert _cg_frozen([3.0, 2.0] + [1.0] * 11)                 # length 13
    assert _cg_frozen([5.0, 1.0 + 2e-15, 1.0 - 1e-15, 1.0])    # frozen to 1e-15
    assert not _cg_frozen([5.0, 1.0 + 2e-13, 1.0 + 1e-13, 1.0])   # moving by 1e-13
    assert not _cg_frozen([5.0, 1.0, 1.0 + 1e-13, 1.0 + 1e-13])   # only the last difference is small
    assert not _cg_frozen([0.0, 0.0, 0.0])                     # a zero residual is not a frozen one
    assert not _cg_frozen([1.0, 1.0, float("nan")])


def test_not_converging_needs_thirteen_entries_and_a_residual_that_has_not_halved():
    flat = [1.0] * 13
    assert not _cg_not_converging(flat[:2]) and not _cg_not_converging(flat[:3])
    assert not _cg_not_converging(flat[:12])                   # length 12: too short to judge
    assert _cg_not_converging(flat)                            # length 13
    halving = [2.0 ** -(i / 10.0) for i in range(13)]
    halving[-1] = 0.5 * halving[-11]                           # exactly halved over ten steps: the rule is "not <"
    assert _cg_not_converging(halving)
    halving[-1] = np.nextafter(halving[-1], 0.0)
    assert not _cg_not_converging(halving)
    assert _cg_not_converging([10.0 ** -i for i in range(12)] + [float("nan")])   # a NaN tail
    assert not _cg_not_converging([10.0 ** -i for i in range(13)])


# ---- _Modes
def test_modes_start_and_judge_apply_the_reference_test_with_strict_less():
    rnorm0, rtol, atol = 4.0, 0.25, 1e-3                       # rtol * rnorm0 = 1.0
    hist = [[] for _ in range(4)]
    m = _Modes(hist, rtol * rnorm0, atol)
    assert m.k == 4 and m.hist is hist and m.tol == 1.0
    assert not m.start([0.5, 1.0, 2.0, 3.0])                   # below rtol * rnorm0; exactly at it; two above
    assert hist == [[0.5], [1.0], [2.0], [3.0]]
    assert m.info == [0, None, None, None]
    assert m.done.tolist() == m.converged.tolist() == [True, False, False, False]
    assert m.judge(1, 1, 0.999) and not m.judge(2, 1, 1.0) and not m.judge(3, 1, 1.5)
    assert m.judge(2, 2, 0.25) and not m.judge(3, 2, float("nan"))
    assert hist == [[0.5], [1.0, 0.999], [2.0, 1.0, 0.25], [3.0, 1.5, hist[3][2]]]
    assert m.info == [0, 1, 2, None]
    assert m.done.tolist() == m.converged.tolist() == [True, True, True, False]
    # below atol only (rtol * rnorm0 smaller than atol), and exactly at atol
    m = _Modes([[], []], 1e-9, 1e-3)
    assert not m.start([5e-4, 1e-3])
    assert m.info == [0, None] and m.converged.tolist() == [True, False]
    # every mode below the tolerance at the start: nothing left to do
    m = _Modes([[], []], 1.0, 0.0)
    assert m.start(np.array([0.5, 0.25])) and m.info == [0, 0]


def test_modes_take_the_callers_verdict_where_it_compares_in_another_form():
    m = _Modes([[], []], 1.0, 0.0)
    assert not m.start([0.5, 2.0], met=[False, False])         # (the short recurrence compares squares, as the device does)
    assert m.info == [None, None] and m.hist == [[0.5], [2.0]]
    assert m.judge(1, 3, 2.0, met=True) and m.info == [None, 3] and m.converged.tolist() == [False, True]


# ---- _by_column_chunks with a made-up round
class _Block:
    def __init__(self, a):
        self.a, (self.n, self.k) = a, a.shape

    def cols(self, c0, c1):
        return _Block(self.a[:, c0:c1])

    def copy_from(self, other):
        self.a[...] = other.a
        return self


class _Ctx:
    def zeros(self, n, k):
        return _Block(np.zeros((n, k)))


def _round(calls, fail_at=None):
    def run(a, b, blk):
        calls.append((a, b, blk))
        assert blk.k == b - a
        return _Block(blk.a + 1.0), blk.a[0] > 0.0, [int(v) for v in blk.a[1]], a != fail_at
    return run


@pytest.mark.parametrize("k, width, chunks", [(31, 32, None), (32, 32, None), (33, 32, [(0, 32), (32, 33)]),
                                               (64, 64, None), (65, 64, [(0, 64), (64, 65)]),
                                               (70, 32, [(0, 32), (32, 64), (64, 70)])])
def test_chunks_are_run_in_order_and_stitched_and_a_block_that_fits_is_handed_through(k, width, chunks):
    R = _Block(np.random.default_rng(k).integers(-5, 6, size=(3, k)).astype(float))
    calls = []
    upd, conv, info, ok = _by_column_chunks(_round(calls), _Ctx(), R, width)
    assert ok
    if chunks is None:
        assert len(calls) == 1 and calls[0][:2] == (0, k) and calls[0][2] is R      # the caller's block itself ...
    else:
        assert [c[:2] for c in calls] == chunks
    assert np.array_equal(upd.a, R.a + 1.0) and upd.a is not R.a
    assert np.array_equal(conv, R.a[0] > 0.0) and info == [int(v) for v in R.a[1]]


def test_a_block_that_fits_gets_the_rounds_own_update_back():
    out = (_Block(np.ones((2, 5))), np.ones(5, dtype=bool), [1] * 5, False)
    got = _by_column_chunks(lambda a, b, blk: out, _Ctx(), _Block(np.zeros((2, 5))), 32)
    assert got is out and got[0] is out[0]                                            # ... and no copy of the update


def test_chunks_stop_behind_the_first_one_that_failed():
    R = _Block(np.arange(3 * 100, dtype=float).reshape(3, 100))
    calls = []
    upd, conv, info, ok = _by_column_chunks(_round(calls, fail_at=32), _Ctx(), R, 32)
    assert not ok and [c[:2] for c in calls] == [(0, 32), (32, 64)]                  # chunks 3 and 4 were never run
    assert np.array_equal(upd.a[:, :64], R.a[:, :64] + 1.0) and not upd.a[:, 64:].any()
    assert info[64:] == [None] * 36 and not conv[64:].any()
