"""GPU: the decode step at the end of Gemma's full context.  An engine of 8 query heads on one kv head at n_ctx
8192 prefills all but the last 42 positions in chunks and then steps to the end through the captured graph: the
step's split attention keeps its softmax image in windows there (k_attn_decode_win).  The reference is the exact
prefill path over the same sequence, itself held to the oracle at these lengths (tests/test_gpu_attn_mx_long.py).
With option att_win 1 the windowed form also runs where the resident one does (n_ctx 4096): no bit changes."""
import functools

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_attn_mx_long import G8, _rows_equal

pytestmark = pytest.mark.gpu
N_STEP = 41


@functools.lru_cache(maxsize=None)
def _stepped(n_ctx, att_win):
    """engine A: a prompt of n_ctx - 42 tokens in three passes, then N_STEP graph steps (positions n_ctx - 42 ..
    n_ctx - 2) -> (their logits rows, the whole sequence).  Read-only."""
    import gemma_hip as G
    n_prompt = n_ctx - N_STEP - 1
    e = G.Engine(G8, n_ctx=n_ctx, device=0)
    e.set_option("att_win", att_win)
    e.begin(O.make_prompt(n_prompt, G8["n_vocab"]))
    for n in (n_prompt // 3, n_prompt // 3, 0):
        e.prefill_next(n)
    rows = e.step(N_STEP, want_logits=True, use_graph=True)
    seq = [int(t) for t in e.tokens()]
    e.close()
    rows.setflags(write=False)
    return rows, seq


@pytest.mark.parametrize("n_ctx,att_win", [(8192, 0), (4096, 1)])
def test_steps_to_the_end_of_the_context_equal_the_prefill_pass(n_ctx, att_win):
    import gemma_hip as G
    rows, seq = _stepped(n_ctx, att_win)
    assert len(seq) == n_ctx
    e = G.Engine(G8, n_ctx=n_ctx, device=0)
    e.begin(seq[:-1])
    n_prompt = n_ctx - N_STEP - 1
    for n in (n_prompt // 3, n_prompt // 3, n_prompt - 2 * (n_prompt // 3)):
        e.prefill_next(n)
    tok, last, allv = e.prefill_next(0, want_all=True)
    e.close()
    _rows_equal(rows, allv, f"steps at n_ctx {n_ctx} att_win {att_win} against the prefill pass")
    assert seq[-N_STEP:] == allv.argmax(axis=1).tolist() and tok == seq[-1]
    if att_win:
        rows0, seq0 = _stepped(n_ctx, 0)
        _rows_equal(rows, rows0, "att_win 1 against att_win 0")
        assert seq == seq0
