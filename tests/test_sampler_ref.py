"""The sampling rule's numpy restatement (tests/sampler_ref.py) checked on the CPU: the splitmix64
known answers, the reductions to argmax, a chi-square of its draws against its own probabilities,
and that none of the draws the GPU tests compare is one the reference itself flags as ambiguous."""
import math

import numpy as np
import pytest

import sampler_ref as R


def test_splitmix64_known_answers():
    got = [R.mix((0 + (p + 1) * R.GOLDEN) & R.M64) for p in range(3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_uniform_in_unit_interval():
    u = np.array([R.uniform(seed, p) for seed in (0, 1, 2 ** 64 - 1) for p in range(2000)])
    assert (u >= 0.0).all() and (u < 1.0).all()
    assert 0.45 < u.mean() < 0.55
    assert R.uniform(7, 3) != R.uniform(7, 4) and R.uniform(7, 3) == R.uniform(7, 3)


def _tied_row():
    row = np.random.default_rng(3).standard_normal(500).astype(np.float32)
    row[[77, 130, 402]] = row.max() + np.float32(1.0)  # three tied maxima: the first wins
    return row


def test_top_k_1_is_first_max_argmax():
    row = _tied_row()
    for p in range(50):
        tok, m, amb, cand = R.sample(row, 1.5, 1, 1.0, seed=9, p=p)
        assert (tok, m, list(cand)) == (77, 1, [77]) and not amb
    assert int(np.argmax(row)) == 77


def test_top_p_to_zero_is_first_max_argmax():
    row = _tied_row()
    for p in range(50):
        tok, m, _, cand = R.sample(row, 1.0, 40, 1e-6, seed=9, p=p)
        assert (tok, m) == (77, 1)
        assert list(cand[:3]) == [77, 130, 402]


def test_signed_zeros_and_minus_inf_order():
    row = np.zeros(10, dtype=np.float32)
    row[::2] = -0.0
    row[7] = 1.0
    assert list(R.candidates(row, 4)) == [7, 0, 1, 2]
    row = np.full(8, -np.inf, dtype=np.float32)
    row[[5, 2]] = [1.0, 3.0]
    t = R.Table(row, 1.0, 6, 1.0)
    assert list(t.cand) == [2, 5, 0, 1, 3, 4]
    assert all(t.draw(1, p)[0] in (2, 5) for p in range(200))


def _chi2_q999(df):
    """99.9 % quantile of chi-square (Wilson-Hilferty; within 0.3 % for df >= 10)"""
    z = 3.090232306167813
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


@pytest.mark.parametrize("seed", [12345, 99])
def test_draws_follow_the_reference_probabilities(seed):
    V, K, T, top_p, N = 4096, 40, 0.8, 0.95, 4096
    t = R.Table(R.make_row(1, V, 1.0), T, K, top_p)
    toks = np.array([t.draw(seed, p)[0] for p in range(N)])
    expect = t.probs * N
    keep = expect >= 5.0
    assert keep.sum() >= 10
    counts = np.array([(toks == c).sum() for c in t.cand[:t.m]])
    assert counts.sum() == N  # every draw is one of the m kept candidates
    stat = (((counts - expect) ** 2) / expect)[keep].sum()
    df = int(keep.sum()) - (1 if keep.all() else 0)
    print(f"chi-square {stat:.1f} on {df} degrees of freedom, bound {_chi2_q999(df):.1f}")
    assert stat < _chi2_q999(df)


@pytest.mark.parametrize("case", R.DRAW_CASES, ids=lambda c: f"V{c[0]}-K{c[1]}")
def test_gpu_draw_cases_have_no_ambiguous_draw(case):
    """the GPU tests exclude flagged draws; with these inputs there is none to hide behind"""
    V, K, T, top_p, sd, n_pos = case
    t = R.Table(R.make_row(R.DRAW_SEED, V, sd), T, K, top_p)
    flagged = sum(t.draw(R.DRAW_SEED, p)[1] for p in range(n_pos))
    assert flagged == 0
