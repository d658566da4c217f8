"""The float64 restatement of the scoring rule (tests/score_ref.py) against what the rule implies."""
import numpy as np
import pytest

from tests import score_ref as R


def test_probabilities_sum_to_one():
    rng = np.random.default_rng(0)
    for V, sigma in ((17, 1.0), (1000, 8.0)):
        l = np.clip(rng.normal(0, sigma, V), -30, 30).astype(np.float32)
        lps = np.array([R.score_row(l, t)[0] for t in range(V)])
        assert abs(np.exp(lps).sum() - 1.0) < 1e-12
        lp, top, tlp = R.score_row(l, 3)
        assert top == int(np.argmax(l)) and tlp == lps[top] and tlp == lps.max()


@pytest.mark.parametrize("row", [
    [1.0, 5.0, 5.0, 2.0],            # a tie: the first
    [5.0, 1.0, 5.0],
    [-1.0, -0.0, 0.0, -2.0],         # -0 equals +0: the earlier one
    [-1.0, 0.0, -0.0, -2.0],
    [np.nan, 7.0, 9.0],              # a NaN at index 0 is never displaced
    [1.0, np.nan, 0.5],              # a NaN elsewhere never displaces
    [1.0, np.nan, 3.0, np.nan, 3.0],
    [-np.inf, np.nan, -np.inf],
    [-np.inf, -np.inf, 2.0, -np.inf],
])
def test_first_max_is_the_scan(row):
    l = np.array(row, np.float32)
    assert R.first_max(l) == R.first_max_scan(l)


def test_first_max_random_ties():
    rng = np.random.default_rng(1)
    for _ in range(200):
        l = rng.integers(-3, 4, 12).astype(np.float32)
        l[rng.integers(0, 12)] = np.float32(-0.0)
        if rng.random() < 0.3:
            l[rng.integers(0, 12)] = np.nan
        assert R.first_max(l) == R.first_max_scan(l)


def test_minus_inf_entries_contribute_nothing():
    l = np.array([0.5, -np.inf, 1.5, -np.inf, -2.0], np.float32)
    kept = l[np.isfinite(l)]
    assert R.lse(l) == pytest.approx(R.lse(kept), abs=1e-15)
    lp, top, tlp = R.score_row(l, 1)
    assert lp == -np.inf and top == 2
    assert R.score_row(l, 2)[0] == pytest.approx(R.score_row(kept, 1)[0], abs=1e-15)


@pytest.mark.parametrize("V", [1, 16, 1000, 128256])
def test_all_equal_row(V):
    for c in (0.0, -7.25, 30.0):
        lp, top, tlp = R.score_row(np.full(V, c, np.float32), V - 1)
        assert top == 0
        assert lp == pytest.approx(-np.log(V), abs=1e-12) and tlp == pytest.approx(-np.log(V), abs=1e-12)


def test_target_out_of_range_and_nan_rows():
    l = np.array([1.0, 2.0, 3.0], np.float32)
    assert np.isnan(R.score_row(l, 3)[0]) and np.isnan(R.score_row(l, -1)[0])
    assert R.score_row(l, 3)[1] == 2 and np.isfinite(R.score_row(l, 3)[2])
    lp, top, tlp = R.score_row(np.array([1.0, np.nan, 3.0], np.float32), 0)
    assert np.isnan(lp) and np.isnan(tlp) and top == 2


def test_rows_and_gap():
    rng = np.random.default_rng(2)
    L = rng.normal(0, 1, (5, 33)).astype(np.float32)
    t = rng.integers(0, 33, 5)
    lp, top, tlp = R.score_rows(L, t)
    for m in range(5):
        assert (lp[m], top[m], tlp[m]) == R.score_row(L[m], int(t[m]))
    assert R.top2_gap([1.0, 4.0, 2.5]) == 1.5 and R.top2_gap([2.0, 2.0, 1.0]) == 0.0
