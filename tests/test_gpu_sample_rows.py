"""The sampler's row dimension (csrc/sample.hip, grid.y = row): nine different rows at nine different
positions through ONE set of three launches (gemma_test_sample with rows = 9), against the numpy
restatement of the rule (tests/sampler_ref.py), as tests/test_gpu_sample.py compares one row.

Row 4 is an all-equal row between ordinary rows: every entry lands in the boundary bin, so list B
holds the whole vocabulary (more than the tail's LDS array: the radix-select path) while its
neighbours' lists hold a few dozen entries.  A workspace that leaked into a neighbour's (histogram,
cursors, lists, key slot) would change that neighbour's candidates or K.  V = 5000 is no multiple of
the 2048-logit workgroup pass and spans three workgroups per row."""
import numpy as np
import pytest

import gemma_hip as G
import sampler_ref as R

pytestmark = pytest.mark.gpu

V, ROWS, TIE_ROW = 5000, 9, 4
POS = [0, 7, 1, 300, 12, 2047, 5, 64, 31]


def _rows():
    rows = np.stack([R.make_row(100 + r, V, 1.0 + 0.25 * r) for r in range(ROWS)]).astype(np.float32)
    rows[TIE_ROW] = np.float32(0.25)
    return rows


@pytest.mark.parametrize("top_k,top_p", [(40, 0.95), (1024, 1.0)], ids=["K40-p0.95", "K1024-p1"])
def test_nine_rows_in_one_launch_set(top_k, top_p):
    rows = _rows()
    smp = dict(temperature=1.0, top_k=top_k, top_p=top_p, seed=R.DRAW_SEED)
    toks, cand, n_cand, n_kept = G.test_sample(rows, smp, POS)
    for r in range(ROWS):
        t = R.Table(rows[r], 1.0, top_k, top_p)
        assert n_cand[r] == t.K == top_k, (r, n_cand[r])
        assert np.array_equal(cand[r, :t.K], t.cand), (r, np.nonzero(cand[r, :t.K] != t.cand)[0][:8])
        assert (cand[r, t.K:] == -1).all(), r
        tok, ambiguous = t.draw(R.DRAW_SEED, POS[r])
        assert not ambiguous, r  # these inputs give no prefix sum within 1e-9 of a threshold
        assert n_kept[r] == t.m, (r, n_kept[r], t.m)
        assert toks[r] == tok, (r, toks[r], tok)
    assert list(cand[TIE_ROW, :top_k]) == list(range(top_k))  # equal logits: the smallest indices
    assert len(set(toks.tolist())) > 3


def test_rows_do_not_depend_on_their_neighbours():
    """each row alone gives what it gives among the nine (the draw depends on the row, the parameters
    and (seed, p) only), and a second call finds every workspace left zero by the first"""
    rows = _rows()
    smp = dict(temperature=1.0, top_k=40, top_p=0.95, seed=R.DRAW_SEED)
    both = [G.test_sample(rows, smp, POS) for _ in range(2)]
    for a, b in zip(*both):
        assert np.array_equal(a, b)
    for r in (0, TIE_ROW, TIE_ROW + 1, ROWS - 1):
        one = G.test_sample(rows[r], smp, [POS[r]])
        for a, b in zip(one, both[0]):
            assert np.array_equal(a[0], b[r]), r
