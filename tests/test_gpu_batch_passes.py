"""The three kinds of batch pass alternated in one open batch: gemma_engine_batch_step_rows,
gemma_engine_batch_verify and gemma_engine_batch_step share the batch's scratch, its batch_step row
table and its row tokens, and each kind builds tables of its own.  What one kind leaves behind must
not reach the next.

The yardstick is tests/test_gpu_batch.py's: the oracle's single-sequence run per slot (Seq), every
row of every pass bit for bit (uint32 views, no tolerance), and after every pass each active slot's
position, tokens and pending token (_rows, _step, _verify).

The shape is the smallest at which the bookkeeping between passes can go wrong: slots 0, 2 and 3 of 4
are active and slot 1 never is, so a slot's rank among the active slots is not its index; slot 2 holds
given tokens from the first pass to the last (its picks are never committed), slots 0 and 3 decode;
in each verify pass another slot sits out, and a draft is rejected.  Every pass of more than 8 rows has
a slot whose rows straddle row 8, the edge between two groups."""
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_batch import Seq, _adopt, _begin, _engine
from test_gpu_batch_rows import NEVER, _rows, _step
from test_gpu_batch_verify import _verify

pytestmark = pytest.mark.gpu

N_GIVEN = 40  # slot 2's given tokens: more than the 32 positions it moves in the longest case


@pytest.fixture(scope="module")
def seqs():
    shape = dict(O.TINY)
    return {0: Seq(shape, 256, 20, seed=1, n_dec=24), 2: Seq(shape, 256, N_GIVEN, seed=2, n_dec=1),
            3: Seq(shape, 256, 9, seed=3, n_dec=24)}


# max_rows of the step_rows passes, bt_mfma_min, and the two verify passes' {slot: (k, a)}
FORMS = {
    # every pass at most 8 rows: step_rows (1, 6, 1); verify 4 + 4 = 8 rows, then 1 + 5 = 6 rows
    "skinny": (8, None, {0: (3, 1), 3: (3, 3)}, {2: (0, 0), 3: (4, 2)}),
    # step_rows (1, 14, 1): slot 2 has rows 1 .. 14; verify 5 + 7 = 12 rows, slot 3 has rows 5 .. 11;
    # then 1 + 8 = 9 rows, slot 3 has rows 1 .. 8
    "groups": (16, NEVER, {0: (4, 1), 3: (6, 6)}, {2: (0, 0), 3: (7, 2)}),
    "mfma": (16, 9, {0: (4, 1), 3: (6, 6)}, {2: (0, 0), 3: (7, 2)}),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_alternating_passes(seqs, form):
    max_rows, mfma_min, plan1, plan2 = FORMS[form]
    e = _engine(dict(O.TINY))
    e.batch_open_rows(4, 16)
    if mfma_min is not None:
        e.set_option("bt_mfma_min", mfma_min)
    _adopt(e, 0, seqs[0])
    _begin(e, 2, seqs[2])
    _adopt(e, 3, seqs[3])
    want = [1, 0, max_rows - 2, 1]
    assert _rows(e, seqs, max_rows) == want
    _verify(e, seqs, plan1)  # slot 2 sits out, slot 0's draft is rejected at its second entry
    _step(e, seqs, 2)
    assert _rows(e, seqs, max_rows) == want
    _verify(e, seqs, plan2)  # slot 0 sits out, slot 2 consumes a given token, slot 3's draft is rejected
    _step(e, seqs, 1)
    # slot 2 is still inside its given tokens: no pick of any pass was committed to its history
    assert seqs[2].pos < N_GIVEN and list(e.batch_tokens(2)) == list(seqs[2].prompt[:seqs[2].pos + 1])
    e.close()
