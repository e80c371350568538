"""The top-n kernels on host rows (gemma_test_top_logprobs: k_lse_parts, k_topn_parts, k_topn_finish)
against tests/toplogprob_ref.py: tokens exactly, values within logprob_ref.MARGIN, padding (-1, NaN).
Vocabulary sizes: V < n, misaligned rows (255), the chunk edge, a one-entry third chunk, Gemma's."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import logprob_ref as R
import toplogprob_ref as T

pytestmark = pytest.mark.gpu

VOCABS = [1, 31, 255, 4095, 4096, 4097, 8193, 256000]
ROWS = (1, 3, 64)
NS = (1, 20, 32)
CHUNK = 4096  # logits per workgroup of k_topn_parts (csrc/kernels.h TOPN_CHUNK)


@functools.lru_cache(maxsize=2)
def _case(kind, V):
    """64 rows of the kind and their 32 alternatives (n < 32: a prefix of them), made once for the case"""
    rows, _ = R.ROW_KINDS[kind](np.random.default_rng([VOCABS.index(V), sorted(R.ROW_KINDS).index(kind)]), max(ROWS), V)
    tok, lps = T.tops(rows, max(NS))
    for a in (rows, tok, lps):
        a.setflags(write=False)
    return rows, tok, lps


def _check(got, rows, n, tok, lps, what):
    gt, gl = got
    assert gt.shape == gl.shape == (len(rows), n), what
    assert np.array_equal(gt, tok[:len(rows), :n]), (what, np.argwhere(gt != tok[:len(rows), :n])[:4])
    ok = T.close(gl, lps[:len(rows), :n])
    assert ok.all(), (what, np.argwhere(~ok)[:4], gl[~ok][:4], lps[:len(rows), :n][~ok][:4])
    assert ((gt == -1) == np.isnan(gl)).all() and (gt[:, :min(n, rows.shape[1])] >= 0).all(), what


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("kind", sorted(R.ROW_KINDS))
def test_kernels_equal_the_reference(kind, V):
    rows, tok, lps = _case(kind, V)
    if kind == "equal":
        assert (tok[:, :min(V, 32)] == np.arange(min(V, 32))).all()
    for n in NS:
        whole = None
        for r in ROWS:
            got = G.test_top_logprobs(rows[:r], n)
            _check(got, rows[:r], n, tok, lps, (kind, V, n, r))
            again = G.test_top_logprobs(rows[:r], n)
            assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes(), (kind, V, n, r)
            whole = got
        one = G.test_top_logprobs(rows[:1], n)  # a row's result does not depend on the rows beside it
        assert one[0].tobytes() == whole[0][:1].tobytes() and one[1].tobytes() == whole[1][:1].tobytes(), (kind, V, n)


@pytest.mark.parametrize("where", ["one chunk", "one per chunk"])
def test_the_merge_keeps_every_candidate_of_a_chunk_and_reads_every_chunk(where):
    """the 32 largest values all inside chunk 1, or one in each of the last 32 chunks"""
    V, n = 40 * CHUNK + 5, 32
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((2, V)).astype(np.float32)
    at = CHUNK + rng.permutation(CHUNK)[:n] if where == "one chunk" else (V - 1 - CHUNK * np.arange(n))
    rows[:, at] = (10.0 + rng.permutation(n)).astype(np.float32)
    tok, lps = T.tops(rows, n)
    assert sorted(tok[0]) == sorted(at)
    _check(G.test_top_logprobs(rows, n), rows, n, tok, lps, where)


@pytest.mark.parametrize("rows, V, n", [(1, 16, 0), (1, 16, 33), (0, 16, 4), (1, (1 << 20) + 1, 4)])
def test_refusals(rows, V, n):
    with pytest.raises(RuntimeError, match="gemma_test_top_logprobs: "):
        G.test_top_logprobs(np.zeros((rows, V), dtype=np.float32), n)
