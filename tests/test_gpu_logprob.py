"""The log-probability kernels on host rows (gemma_test_logprob: k_lse_parts + k_lse_finish) against
tests/logprob_ref.py at 1e-9 absolute (both -inf counts as equal; the margin is derived there).

Vocabulary sizes: 1 (one partial chunk), 255 (no row but the first is 16-byte aligned), CHUNK + 1 and
2049 (a guarded tail one past a chunk multiple), 4096 (TINY), 256000 (Gemma: every workgroup and the
whole merge).  Each case runs 1, 3 and 64 rows (grid.y) of distinct rows with distinct tokens, and
every launch twice: the two outputs must be the same bytes."""
import numpy as np
import pytest

import gemma_hip as G
import logprob_ref as R

pytestmark = pytest.mark.gpu

VOCABS = [1, 255, R.CHUNK + 1, 2049, 4096, 256000]
ROWS = (1, 3, 64)


def _case(kind, V):
    """64 rows of the kind, their tokens and the reference: made once for the case's three row counts"""
    rows, toks = R.ROW_KINDS[kind](np.random.default_rng([VOCABS.index(V), sorted(R.ROW_KINDS).index(kind)]), max(ROWS), V)
    ref = R.logprobs(rows, toks)
    for a in (rows, toks, ref):
        a.setflags(write=False)
    return rows, toks, ref


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("kind", sorted(R.ROW_KINDS))
def test_kernels_equal_the_reference(kind, V):
    rows, toks, ref = _case(kind, V)
    assert not np.isnan(ref).any()
    for n in ROWS:
        got = G.test_logprob(rows[:n], toks[:n])
        again = G.test_logprob(rows[:n], toks[:n])
        ok = R.close(got, ref[:n])
        with np.errstate(invalid="ignore"):
            print(kind, V, n, "max |gpu - numpy| =", np.nanmax(np.where(np.isfinite(ref[:n]), np.abs(got - ref[:n]), 0.0)))
        assert ok.all(), (kind, V, n, np.flatnonzero(~ok)[:8], got[~ok][:8], ref[:n][~ok][:8])
        assert got.tobytes() == again.tobytes(), (kind, V, n)
        if n > 1:  # a row's value does not depend on the rows beside it
            assert got[:1].tobytes() == G.test_logprob(rows[:1], toks[:1]).tobytes(), (kind, V, n)


def test_every_token_of_a_row():
    """one row repeated with each of its tokens: sum exp(lp) = 1, and the row kinds' special tokens"""
    row = (np.random.default_rng(3).standard_normal(R.CHUNK + 7) * 3.0).astype(np.float32)
    row[5] = -np.inf
    V = row.size
    got = G.test_logprob(np.repeat(row[None, :], V, axis=0), np.arange(V, dtype=np.int32))
    assert R.close(got, R.all_tokens(row)).all()
    assert np.isneginf(got[5]) and abs(np.exp(got).sum() - 1.0) <= 1e-9


def test_refusals():
    row = np.zeros((2, 16), dtype=np.float32)
    for toks in ([0, 16], [-1, 0]):
        with pytest.raises(RuntimeError, match="gemma_test_logprob: token id"):
            G.test_logprob(row, toks)
