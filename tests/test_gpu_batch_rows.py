"""Batch passes with several rows per slot (gemma_engine_batch_open_rows / _step_rows): a slot that
still has given tokens to consume takes the pass's idle rows.

The yardstick is tests/test_gpu_batch.py's: the oracle's single-sequence run per slot (Seq, _truth,
_bits_equal).  Row (s, i) of a pass processes position pos_s + i, so its logits must be row
pos_s + i of that sequence's logits bit for bit (uint32 views, no tolerance), whatever the other rows
are and whichever form the pass takes (T <= 8 skinny, T >= bt_mfma_min one MFMA pass, else groups of up
to 8 rows).  With the sampler on the reference is a plain Engine stepping with the same sampler; the
device state and the log-probabilities are compared with a slot that took batch_step(1) passes.

The shapes are the smallest at which the row bookkeeping can go wrong: chunks on both sides of the
padded-n_kv bump at 31 / 32, a chunk that ends exactly on the prompt's end, a final chunk of one given
token, a chunk that ends mid-prompt, decoding slots beside ingesting ones, a slot whose rows straddle
group edges, rows that straddle position 256, G = 1 / 2 / 8 query heads per kv head, Q8_0, the Q6_K
head and K-quant layers."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_batch import SAMPLER, Seq, _adopt, _begin, _engine
from test_gpu_prefill_continue import G8, K2B, KSHAPE, _bits_equal, _key, _truth  # noqa: F401

pytestmark = pytest.mark.gpu

NEVER = G.BATCH_WIDE_MAX_SLOTS + 1  # bt_mfma_min: every pass of more than 8 rows in groups


def _need(slots):
    n = max(slots) + 1
    return [max(1, len(slots[s].prompt) - slots[s].pos) if s in slots else 0 for s in range(n)]


def _rows(e, slots, max_rows):
    """one step_rows pass over the active slots {slot: Seq}: the plan, every row, position, token and
    pending token against the oracle"""
    need = _need(slots)
    plan = list(G.batch_plan_rows(need, max_rows))
    rows_of, lg = e.batch_step_rows(max_rows, want_logits=True)
    assert list(rows_of[:len(plan)]) == plan and not rows_of[len(plan):].any(), (list(rows_of), plan)
    assert lg.shape[0] == sum(plan)
    last = e.batch_last_n()
    t = 0
    for s in sorted(slots):
        q, m = slots[s], plan[s]
        _bits_equal(lg[t:t + m], q.expect(m), f"slot {s}: rows {t} .. {t + m - 1} of {sum(plan)} from position {q.pos}")
        t += m
        q.pos += m
        assert e.batch_pos(s) == q.pos
        assert list(e.batch_tokens(s)) == list(q.full[:q.pos + 1]), (s, q.pos)
        assert last[s] == q.full[q.pos]
    assert all(last[s] == -1 for s in range(len(last)) if s not in slots)
    return plan


def _step(e, slots, n):
    """n batch_step passes after the row passes: every row, position and token"""
    lg = e.batch_step(n, want_logits=True)
    last = e.batch_last_n()
    for r, s in enumerate(sorted(slots)):
        q = slots[s]
        _bits_equal(lg[:, r], q.expect(n), f"batch_step: slot {s} from position {q.pos}")
        q.pos += n
        assert e.batch_pos(s) == q.pos
        assert list(e.batch_tokens(s)) == list(q.full[:q.pos + 1])
        assert last[s] == q.full[q.pos]


def test_one_slot_chunks_across_the_n_kv_bump():
    """45 tokens in chunks 8, 8, 8, 8, 8, 5: the chunk 24 .. 31 holds the bump at p = 31, the last chunk
    ends exactly on the prompt's end (the pick is appended); then one-row passes decode"""
    shape = dict(O.TINY)
    q = Seq(shape, 256, 45)
    e = _engine(shape)
    e.batch_open_rows(1, 8)
    _begin(e, 0, q)
    plans = [_rows(e, {0: q}, 8) for _ in range(6)]
    assert plans == [[8]] * 5 + [[5]]
    assert q.pos == 45 and list(e.batch_tokens(0)) == list(q.full[:46])
    for _ in range(3):
        assert _rows(e, {0: q}, 8) == [1]
    _step(e, {0: q}, 2)
    e.close()


def test_partial_final_chunk():
    """17 tokens: chunks 8, 8, 1; the final single given token is a chunk of its own and appends"""
    shape = dict(O.TINY)
    q = Seq(shape, 256, 17, seed=4)
    e = _engine(shape)
    e.batch_open_rows(1, 8)
    _begin(e, 0, q)
    assert [_rows(e, {0: q}, 8) for _ in range(3)] == [[8], [8], [1]]
    assert list(e.batch_tokens(0)) == list(q.full[:18])
    e.close()


def test_mid_prompt_chunk_appends_nothing():
    shape = dict(O.TINY)
    q = Seq(shape, 256, 20, seed=2)
    e = _engine(shape)
    e.batch_open_rows(1, 8)
    _begin(e, 0, q)
    _rows(e, {0: q}, 8)
    k, _ = e.batch_kv_read(0, 0, 0, 256)
    assert k[:8].any() and not k[8:].any()
    # the history past the prompt is untouched: the slot's sequence is the prompt's first pos + 1 tokens
    assert list(e.batch_tokens(0)) == list(q.prompt[:9])
    _rows(e, {0: q}, 5)  # 5 of the 12 that remain
    assert e.batch_pos(0) == 13 and list(e.batch_tokens(0)) == list(q.prompt[:14])
    e.close()


def test_mixed_pass_decoding_beside_ingesting():
    """slot 0 adopted at 30 and decoding, slot 2 with 20 given tokens, slot 5 with 3: (1, 6, 1) first;
    until all generate, then batch_step(3)"""
    shape = dict(O.TINY)
    a, b, c = Seq(shape, 256, 30, seed=1), Seq(shape, 256, 20, seed=2), Seq(shape, 256, 3, seed=3)
    e = _engine(shape)
    e.batch_open_rows(8, 8)
    _adopt(e, 0, a)
    _begin(e, 2, b)
    _begin(e, 5, c)
    slots = {0: a, 2: b, 5: c}
    plan = _rows(e, slots, 8)
    assert [plan[0], plan[2], plan[5]] == [1, 6, 1]
    n = 1
    while any(q.pos < len(q.prompt) for q in slots.values()):
        _rows(e, slots, 8)
        n += 1
    assert n == 4 and (a.pos, b.pos, c.pos) == (34, 20, 4)
    _step(e, slots, 3)
    e.close()


@pytest.fixture(scope="module")
def wide_seqs():
    shape = dict(O.TINY)
    return Seq(shape, 256, 62, seed=2, n_dec=8), Seq(shape, 256, 100, seed=5, n_dec=2)


@pytest.mark.parametrize("max_rows,mfma_min", [(64, 9), (64, NEVER), (20, 9)], ids=["mfma", "groups_of_64", "groups_8_8_4"])
def test_wide_forms(wide_seqs, max_rows, mfma_min):
    """slot 0 adopted at 62 (crosses key 64), slot 1 with 100 given tokens: one MFMA pass of 64 rows, the
    same as groups (slot 1 straddles every group edge), and passes of 20 rows as groups 8 + 8 + 4.  Every
    row equals the oracle's in each form, so the three forms give the same bits"""
    shape = dict(O.TINY)
    a, b = wide_seqs
    e = _engine(shape)
    e.batch_open_rows(3, 64)
    e.set_option("bt_mfma_min", mfma_min if max_rows == 64 else NEVER)
    _adopt(e, 0, a)
    _begin(e, 1, b)
    slots = {0: a, 1: b}
    plan = _rows(e, slots, max_rows)
    assert plan == [1, max_rows - 1]
    while b.pos < len(b.prompt):
        _rows(e, slots, max_rows)
    _rows(e, slots, max_rows)  # both generate
    e.close()


def test_rows_straddle_position_256():
    """n_ctx 512, 270 given tokens, step_rows(60): the chunk 240 .. 299 is cut at the prompt's end, rows
    240 .. 269 straddle position 256 (the attention's second KQ round and the long KQV loop)"""
    shape = dict(O.TINY)
    q = Seq(shape, 512, 270, seed=1, n_dec=3)
    e = _engine(shape, n_ctx=512)
    e.batch_open_rows(1, 64)
    _begin(e, 0, q)
    plans = [_rows(e, {0: q}, 60)[0] for _ in range(5)]
    assert plans == [60, 60, 60, 60, 30]
    _rows(e, {0: q}, 60)
    e.close()


@pytest.mark.parametrize("shape,n_ctx,okw,ekw", [
    (G8, 256, {}, {}),
    (K2B, 256, {}, {}),
    (dict(O.TINY), 256, dict(wtype=O.Q8_0), dict(wtype=G.GGML_TYPE_Q8_0)),
    (dict(O.TINY), 256, dict(kmix=2), dict(out_type=G.GGML_TYPE_Q6_K)),
    (KSHAPE, 128, dict(kmix=1), dict(wtype=G.GGML_TYPE_Q4_K)),
], ids=["G8", "K2B", "Q8_0", "Q6K_head", "kquant_layers"])
def test_shapes(shape, n_ctx, okw, ekw):
    """2 slots, 11 and 2 given tokens, 8 rows: (7, 1), (4, 1), (1, 1)"""
    slots = {0: Seq(shape, n_ctx, 11, seed=1, n_dec=3, **okw), 1: Seq(shape, n_ctx, 2, seed=2, n_dec=3, **okw)}
    e = _engine(shape, n_ctx=n_ctx, **ekw)
    e.batch_open_rows(2, 8)
    for s, q in slots.items():
        _begin(e, s, q)
    assert [_rows(e, slots, 8) for _ in range(3)] == [[7, 1], [4, 1], [1, 1]]
    e.close()


def test_device_state_equals_single_row_passes():
    """the same prompt by chunks in slot 0 and by batch_step passes of one row in slot 1: the tokens, the
    pending token and every layer's whole cache, positions 0 .. pos and the untouched rows beyond"""
    shape, n_ctx = dict(O.TINY), 256
    prompt = tuple(int(t) for t in O.make_prompt(37, shape["n_vocab"], seed=6))
    e = _engine(shape)
    e.batch_open_rows(2, 16)
    e.set_option("bt_mfma_min", NEVER)
    e.batch_begin(0, prompt)
    for want in (16, 16, 5, 1, 1):  # groups 8 + 8 twice, a skinny pass that appends, two picks
        rows_of, _ = e.batch_step_rows(16)
        assert list(rows_of) == [want, 0]
    pos = e.batch_pos(0)
    assert pos == 39
    toks0, last0 = list(e.batch_tokens(0)), e.batch_last_n()[0]
    kv0 = [e.batch_kv_read(0, il, 0, n_ctx) for il in range(shape["n_layer"])]
    e.batch_release(0)
    e.batch_begin(1, prompt)
    e.batch_step(pos)  # slot 1 alone: one row per pass
    assert e.batch_pos(1) == pos
    assert list(e.batch_tokens(1)) == toks0 and e.batch_last_n()[1] == last0
    for il in range(shape["n_layer"]):
        k1, v1 = e.batch_kv_read(1, il, 0, n_ctx)
        assert np.array_equal(kv0[il][0], k1) and np.array_equal(kv0[il][1], v1), il
        assert k1[:pos].any() and not k1[pos:].any() and not v1[pos:].any(), il
    e.close()


def test_sampler_on():
    """tokens equal a plain Engine stepping with the same sampler: a slot's last row draws with (seed,
    p = the slot's new position); the draws of the rows before it are not used"""
    shape = dict(O.TINY)
    prompts = [tuple(int(t) for t in O.make_prompt(n, shape["n_vocab"], seed=11 + n)) for n in (13, 3)]
    e = _engine(shape)
    e.set_sampler(**SAMPLER)
    e.batch_open_rows(2, 8)
    for s, pr in enumerate(prompts):
        e.batch_begin(s, pr)
    plans = [list(e.batch_step_rows(8)[0]) for _ in range(7)]
    assert plans[:2] == [[7, 1], [6, 2]] and plans[2:] == [[1, 1]] * 5
    p = _engine(shape)
    p.set_sampler(**SAMPLER)
    for s, pr in enumerate(prompts):
        p.begin(pr)
        p.step(e.batch_pos(s), use_graph=False)
        assert list(e.batch_tokens(s)) == list(p.tokens()), s
        assert len(set(list(p.tokens())[len(pr):])) > 1  # the sampler did draw varied tokens
    p.close()
    e.close()


def test_logprobs_on():
    """batch_logprobs bit-equal (f64 as uint64) between a slot fed by chunks and one fed by single-row
    passes, NaN at index 0"""
    shape = dict(O.TINY)
    prompt = tuple(int(t) for t in O.make_prompt(21, shape["n_vocab"], seed=8))
    out = []
    for rows in (True, False):
        e = _engine(shape)
        e.set_logprobs(1)
        e.batch_open_rows(1, 16)
        e.batch_begin(0, prompt)
        e.set_option("bt_mfma_min", 9)
        if rows:
            for want in (16, 5, 1, 1):  # an MFMA pass, a skinny pass that appends, two picks
                rows_of, _ = e.batch_step_rows(16)
                assert list(rows_of) == [want]
        else:
            e.batch_step(23)
        assert e.batch_pos(0) == 23
        out.append((e.batch_logprobs(0), list(e.batch_tokens(0))))
        e.close()
    (lp_rows, t_rows), (lp_one, t_one) = out
    assert t_rows == t_one and len(lp_rows) == 24
    assert np.isnan(lp_rows[0]) and np.isfinite(lp_rows[1:]).all() and (lp_rows[1:] <= 0).all()
    assert np.array_equal(lp_rows.view(np.uint64), lp_one.view(np.uint64))


def _refused(r, name="gemma_engine_batch_step_rows"):
    assert r == -1 and name in G.last_error(), (r, G.last_error())


def test_refusals_leave_the_state_untouched():
    shape = dict(O.TINY)
    a, b = Seq(shape, 256, 20, seed=2), Seq(shape, 256, 3, seed=3)
    e = _engine(shape)
    L, h = e.L, e.h
    _refused(L.gemma_engine_batch_step_rows(h, 8, None, None))  # no batch open
    for n_slots, max_rows in ((0, 8), (65, 64), (2, 7), (2, 65), (9, 8), (12, 11)):
        _refused(L.gemma_engine_batch_open_rows(h, n_slots, max_rows), "gemma_engine_batch_open_rows")
    e.batch_open_rows(3, 12)
    _refused(L.gemma_engine_batch_open_rows(h, 3, 12), "gemma_engine_batch_open_rows")  # already open
    _refused(L.gemma_engine_batch_step_rows(h, 8, None, None))  # no active slot
    _begin(e, 0, a)
    _begin(e, 2, b)
    slots = {0: a, 2: b}
    _rows(e, slots, 4)

    def state():
        return [e.batch_pos(s) for s in (0, 2)], [list(e.batch_tokens(s)) for s in (0, 2)], list(e.batch_last_n())

    before = state()
    rows_of = np.full(3, -7, dtype=np.int32)
    _refused(L.gemma_engine_batch_step_rows(h, 1, None, G._p(rows_of)))   # below the active count
    _refused(L.gemma_engine_batch_step_rows(h, 13, None, G._p(rows_of)))  # above the capacity
    _refused(L.gemma_engine_batch_step_rows(h, 0, None, G._p(rows_of)))
    assert state() == before and (rows_of == -7).all()
    _rows(e, slots, 12)  # and a valid pass after them is exact
    e.close()
    # a batch opened by batch_open has a row capacity of max(8, n_slots)
    e = _engine(shape)
    e.batch_open(2)
    a.pos = b.pos = 0
    _begin(e, 0, a)
    _begin(e, 1, b)
    _refused(e.L.gemma_engine_batch_step_rows(e.h, 9, None, None))
    assert (e.batch_pos(0), e.batch_pos(1)) == (0, 0)
    assert _rows(e, {0: a, 1: b}, 8) == [7, 1]
    e.close()


def test_context_full():
    """n_ctx 64, 63 given tokens: a pass of 62 rows is fine (pos 62), the chunk that would bring the slot
    to position 63 + 1 = n_ctx is refused and nothing moves"""
    shape = dict(O.TINY)
    c = Seq(shape, 64, 63, seed=4, n_dec=0)
    e = _engine(shape, n_ctx=64)
    e.batch_open_rows(1, 64)
    _begin(e, 0, c)
    assert _rows(e, {0: c}, 62) == [62]
    assert _rows(e, {0: c}, 8) == [1]  # position 63 = n_ctx - 1: the last one a slot can reach
    toks = list(e.batch_tokens(0))
    _refused(e.L.gemma_engine_batch_step_rows(e.h, 8, None, None))
    assert "context full" in G.last_error()
    assert e.batch_pos(0) == 63 and list(e.batch_tokens(0)) == toks and e.batch_last_n()[0] == toks[-1]
    e.close()


def test_the_engines_own_sequence_is_untouched():
    shape, n = dict(O.TINY), 20
    own = Seq(shape, 256, n, seed=1)
    other = Seq(shape, 256, 14, seed=5)
    dec, full = own.rows[n:], own.full
    e = _engine(shape)
    e.begin(own.prompt)
    e.prefill(n)
    _bits_equal(e.step(1, want_logits=True, use_graph=True), dec[:1], "the step before the batch")
    kernels = e.graph_kernels()
    e.batch_open_rows(2, 8)
    _begin(e, 1, other)
    _rows(e, {1: other}, 8)
    _bits_equal(e.step(1, want_logits=True, use_graph=True), dec[1:2], "a graph step between row passes")
    _rows(e, {1: other}, 8)
    _rows(e, {1: other}, 8)
    assert e.pos() == n + 2 and list(e.tokens()) == list(full[:n + 3])
    _bits_equal(e.step(2, want_logits=True, use_graph=True), dec[2:4], "graph steps after the row passes")
    assert e.graph_kernels() == kernels
    assert list(e.tokens()) == list(full[:n + 5])
    e.close()
