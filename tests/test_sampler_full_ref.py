"""The whole-vocabulary rule's numpy restatement (tests/sampler_full_ref.py) checked on the CPU: its
nucleus sizes, that its draws range widely, and that none of the draws the GPU tests compare is one
the reference itself flags as ambiguous."""
import numpy as np
import pytest

import sampler_full_ref as F

# per case: the nucleus size (None: the whole row) and the distinct tokens among the draws
EXPECT = [(None, 510), (631, 140), (3026, 1787), (None, 712), (4740, 2723), (7, None)]


@pytest.mark.parametrize("case,expect", list(zip(F.DRAW_CASES, EXPECT)), ids=lambda c: str(c[0]))
def test_gpu_draw_cases_have_no_ambiguous_draw(case, expect):
    """the GPU tests exclude flagged draws; with these inputs there is none to hide behind"""
    V, T, top_p, sd, n_pos = case
    kept, distinct = expect
    t = F.Table(F.make_row(F.DRAW_SEED, V, sd), T, top_p)
    draws = [t.draw(F.DRAW_SEED, p) for p in range(n_pos)]
    assert sum(amb for _, amb in draws) == 0
    assert t.n_kept == (V if kept is None else kept)
    toks = {tok for tok, _ in draws}
    assert len(toks) > (8 if distinct else 0) and (distinct is None or len(toks) == distinct)
    if V == 256000 and top_p == 1.0:  # far more tokens than the truncated rule's 1,024 candidates could give
        order = np.argsort(-F.make_row(F.DRAW_SEED, V, sd), kind="stable")
        assert len(toks - set(order[:1024].tolist())) > 8


def test_all_equal_row_is_a_uniform_pick():
    V = 5000
    t = F.Table(np.full(V, 0.25, dtype=np.float32), 1.0, 1.0)
    for p in range(64):
        u = F.uniform(3, p)
        assert t.draw(3, p) == (min(int(u * V * F.ONE) // F.ONE, V - 1), False)
