"""CPU: tests/logprob_ref.py, the numpy restatement of the log-probability rule the GPU tests hold the
device to, checked against closed forms and an exact rational evaluation."""
import math
from fractions import Fraction

import numpy as np
import pytest

import logprob_ref as R


@pytest.mark.parametrize("V", [1, 2, 255, 4096, 256000])
def test_all_equal_row_is_minus_log_v(V):
    for c in (0.0, -7.25, 3e38):
        row = np.full(V, c, dtype=np.float32)
        for t in {0, V // 2, V - 1}:
            assert abs(R.logprob(row, t) + math.log(V)) <= 1e-12


def test_one_hot_row():
    row = np.full(4096, -1000.0, dtype=np.float32)
    row[17] = 0.0
    lp = R.all_tokens(row)
    assert lp[17] == 0.0  # exp(-1000) is 0 in f64: S = 1 exactly
    assert np.all(np.delete(lp, 17) == -1000.0)


def test_minus_inf_entries_contribute_nothing():
    rng = np.random.default_rng(1)
    row = rng.standard_normal(300).astype(np.float32)
    masked = row.copy()
    dead = rng.permutation(300)[:100]
    masked[dead] = -np.inf
    live = np.setdiff1d(np.arange(300), dead)
    lp = R.all_tokens(masked)
    assert np.all(np.isneginf(lp[dead]))
    assert np.abs(lp[live] - R.all_tokens(row[live])).max() <= 1e-13  # the row without them
    assert not np.isnan(lp).any()


@pytest.mark.parametrize("seed,V,sd", [(0, 7, 1.0), (1, 1000, 3.0), (2, 4096, 10.0), (3, 4096, 0.01)])
def test_probabilities_sum_to_one(seed, V, sd):
    row = (np.random.default_rng(seed).standard_normal(V) * sd).astype(np.float32)
    assert abs(math.fsum(np.exp(R.all_tokens(row))) - 1.0) <= 1e-12


def _exact(row, t):
    """the rule with S summed exactly: every exp is the f64 libm value taken as a rational, their sum
    has no rounding at all; math.fsum gives the same sum correctly rounded"""
    l = [float(np.float32(v)) for v in row]
    M = max(l)
    terms = [math.exp(v - M) for v in l]
    S = sum(Fraction(x) for x in terms)
    assert float(S) == math.fsum(terms)
    return (l[t] - M) - math.log(float(S))


@pytest.mark.parametrize("V", range(1, 9))
def test_small_rows_against_the_exact_sum(V):
    rng = np.random.default_rng(100 + V)
    for _ in range(20):
        row = (rng.standard_normal(V) * 4.0).astype(np.float32)
        for t in range(V):
            # a sum of <= 8 terms in [0, 1] differs from the exact one by < 8 * 2^-53 relative
            assert abs(R.logprob(row, t) - _exact(row, t)) <= 1e-15 * 8


def test_shift_invariance():
    rng = np.random.default_rng(5)
    row = np.round(rng.standard_normal(2000) * 4.0 * 1024.0) / 1024.0  # multiples of 2^-10 below 2^6
    row = row.astype(np.float32)
    for c in (64.0, -128.0, 0.5):  # row + c is exact in f32: the differences l - M are unchanged
        shifted = (row + np.float32(c)).astype(np.float32)
        assert np.array_equal(shifted.astype(np.float64), row.astype(np.float64) + c)
        assert np.array_equal(R.all_tokens(shifted), R.all_tokens(row))


def test_zero_signs_tie_and_close_treats_minus_inf_as_equal():
    a = np.array([-0.0, 0.0, -1.0], dtype=np.float32)
    b = np.array([0.0, -0.0, -1.0], dtype=np.float32)
    assert np.array_equal(R.all_tokens(a), R.all_tokens(b))
    assert R.close([-np.inf, -1.0, -1.0], [-np.inf, -1.0 + 5e-10, -1.0 + 5e-9]).tolist() == [True, True, False]
    assert R.close([np.nan, -np.inf], [np.nan, 0.0]).tolist() == [False, False]


@pytest.mark.parametrize("kind", sorted(R.ROW_KINDS))
@pytest.mark.parametrize("V", [1, 255, R.CHUNK + 1, 4096])
def test_row_kinds_stay_inside_the_contract(kind, V):
    rows, toks = R.ROW_KINDS[kind](np.random.default_rng(9), 5, V)
    assert rows.dtype == np.float32 and rows.shape == (5, V) and toks.dtype == np.int32
    assert not np.isnan(rows).any() and np.all(np.isfinite(rows.max(axis=1)))
    assert toks.min() >= 0 and toks.max() < V
    lp = R.logprobs(rows, toks)
    assert not np.isnan(lp).any() and np.all(lp <= 0.0)
