"""Parameters per row in the sampler's launches (csrc/sample.hip, gemma_test_sample_rows): greedy and
sampling rows, each with its own temperature, top_k, top_p and seed, through ONE set of launches,
against the numpy restatement of the rule (tests/sampler_ref.py) and np.argmax for the greedy rows.

The rows are those of tests/test_gpu_sample_rows.py (V = 5000: no multiple of the 2048-logit workgroup
pass, three workgroups per row; row 4 all equal: the radix-select path).  A row -> parameters mapping
that slipped by one row, a greedy row that touched its workspace or its neighbour's key slot, or a
sampling row whose key did not overwrite the row argmax's partial keys would change a token, K or m."""
import numpy as np
import pytest

import gemma_hip as G
import sampler_ref as R
from test_gpu_sample_rows import POS, ROWS, TIE_ROW, V, _rows

pytestmark = pytest.mark.gpu

S = R.DRAW_SEED
NINE = [(1.0, 40, 0.95, S), None, (0.7, 1, 1.0, 7), (1.5, 1024, 0.9, 99), (1.0, 40, 0.95, S + 1), None,
        (0.8, 0, 1.0, 2 ** 63 + 5), (2.0, 5, 0.5, 0), (1.0, 40, 0.95, S)]
NINE_TOKENS = [977, 4737, 1479, 2679, 21, 851, 2701, 3092, 2640]  # the reference's, computed on the CPU


def _check(rows, samplers, positions, got):
    """every row of one call against the reference: sampling rows token, candidates, K and m; greedy
    rows the argmax (unique maxima) with no candidates"""
    toks, cand, n_cand, n_kept = got
    for r, sp in enumerate(samplers):
        if sp is None:
            assert np.count_nonzero(rows[r] == rows[r].max()) == 1, r
            assert toks[r] == int(np.argmax(rows[r])), (r, toks[r])
            assert n_cand[r] == 0 and n_kept[r] == 0 and (cand[r] == -1).all(), r
            continue
        temp, top_k, top_p, seed = sp
        t = R.Table(rows[r], temp, top_k, top_p)
        tok, ambiguous = t.draw(seed, positions[r])
        assert not ambiguous, r  # these inputs give no prefix sum within 1e-9 of a threshold
        assert n_cand[r] == t.K, (r, n_cand[r], t.K)
        assert np.array_equal(cand[r, :t.K], t.cand), (r, np.nonzero(cand[r, :t.K] != t.cand)[0][:8])
        assert (cand[r, t.K:] == -1).all(), r
        assert n_kept[r] == t.m, (r, n_kept[r], t.m)
        assert toks[r] == tok, (r, toks[r], tok)


@pytest.fixture(scope="module")
def nine():
    rows = _rows()
    rows.setflags(write=False)
    return rows, [G.test_sample_rows(rows, NINE, POS) for _ in range(2)]


def test_nine_rows_nine_samplers_in_one_launch_set(nine):
    rows, (first, _) = nine
    _check(rows, NINE, POS, first)
    assert first[0].tolist() == NINE_TOKENS


def test_alone_and_among_the_nine(nine):
    """a row alone (all-greedy or all-sampling launches) gives what it gives among the nine (the mixed
    launches); a second nine-row call finds every workspace zero, the greedy rows' included"""
    rows, (first, second) = nine
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    for r in (0, 1, TIE_ROW, 5, ROWS - 1):
        one = G.test_sample_rows(rows[r], [NINE[r]], [POS[r]])
        for a, b in zip(one, first):
            assert np.array_equal(a[0], b[r]), r


def test_against_the_one_sampler_entry_and_argmax(nine):
    rows, _ = nine
    smp = (1.0, 40, 0.95, S)
    same = G.test_sample_rows(rows, [smp] * ROWS, POS)
    ref = G.test_sample(rows, dict(temperature=smp[0], top_k=smp[1], top_p=smp[2], seed=smp[3]), POS)
    for a, b in zip(same, ref):
        assert np.array_equal(a, b)
    # all greedy: the row argmax alone; the all-equal row's first maximum is index 0
    toks, cand, n_cand, n_kept = G.test_sample_rows(rows, [None] * ROWS, POS)
    assert toks.tolist() == [int(np.argmax(rows[r])) for r in range(ROWS)]
    assert not n_cand.any() and not n_kept.any() and (cand == -1).all()


def test_sixty_four_rows_four_kinds():
    n = 64
    rows = np.stack([R.make_row(100 + r, V, 1.0 + 0.25 * (r % 9)) for r in range(n)]).astype(np.float32)
    pos = [(37 * r + 5) % 2048 for r in range(n)]
    kinds = [None, (1.0, 40, 0.95), (0.8, 0, 1.0), (1.5, 200, 0.9)]
    samplers = [None if r % 4 == 0 else kinds[r % 4] + (S + r,) for r in range(n)]
    got = G.test_sample_rows(rows, samplers, pos)
    _check(rows, samplers, pos, got)
    assert len(set(got[0].tolist())) == n
