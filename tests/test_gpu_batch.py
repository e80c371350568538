"""Batched decode (gemma_engine_batch_*): up to 8 independent sequences, one row each per weight pass.

The yardstick is the oracle's single-sequence run per slot (_truth / _bits_equal of
tests/test_gpu_prefill_continue.py: Model.inference over the prompt, then its greedy decode steps):
the row a pass computes for a slot at position p must be row p of that sequence's logits bit for bit
(uint32 views, no tolerance), whatever the other rows of the pass are.  With the sampler on the
reference is a plain Engine stepping with the same sampler.

The shapes are the smallest at which a row -> slot mapping can go wrong: slots that are not the first
ones, ragged positions on both sides of a padded-n_kv bump (32) and of key 64, a slot still consuming
given tokens while others generate, R = 8 (the T = 8 instantiations), positions past 256 keys (the
attention's second KQ round and the long KQV loop), G = 1 / 2 / 8 query heads per kv head, Q8_0, the
Q6_K head and K-quant layers, and an active set that changes between calls."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_prefill_continue import G8, K2B, KSHAPE, _bits_equal, _key, _truth

pytestmark = pytest.mark.gpu

N_DEC = 10  # oracle decode steps kept per sequence (the longest generated run below is 9)
SAMPLER = dict(temperature=1.0, top_k=40, top_p=0.95, seed=20240607)


class Seq:
    """one sequence's truth and where its slot stands"""

    def __init__(self, shape, n_ctx, n_prompt, seed=1, wtype=O.Q4_0, kmix=0, n_dec=N_DEC, prompt=None):
        self.prompt = tuple(int(t) for t in (prompt if prompt is not None else O.make_prompt(n_prompt, shape["n_vocab"], seed=seed)))
        self.tok, all_ref, dec, self.full = _truth(_key(shape), n_ctx, wtype, kmix, self.prompt, n_dec)
        self.rows = np.concatenate([all_ref, dec])  # row p: the logits of sequence position p
        self.pos = 0

    def expect(self, n):
        assert self.pos + n <= len(self.rows), "the oracle run is too short for this case"
        return self.rows[self.pos:self.pos + n]


def _engine(shape, n_ctx=256, **kw):
    return G.Engine(shape, n_ctx=n_ctx, device=0, **kw)


def _begin(e, slot, seq):
    e.batch_begin(slot, seq.prompt)
    seq.pos = 0
    assert e.batch_pos(slot) == 0


def _adopt(e, slot, seq):
    """the prompt through the engine's own batched prefill, then device to device into the slot"""
    n = len(seq.prompt)
    e.begin(seq.prompt)
    tok, _ = e.prefill(n)
    assert tok == seq.tok
    e.batch_adopt(slot)
    seq.pos = n
    assert e.batch_pos(slot) == n


def _step(e, slots, n):
    """n passes over the active slots {slot: Seq}; every row, position and token against the oracle"""
    lg = e.batch_step(n, want_logits=True)
    order = sorted(slots)
    assert lg.shape[:2] == (n, len(order))
    last = e.batch_last()
    for r, s in enumerate(order):
        q = slots[s]
        _bits_equal(lg[:, r], q.expect(n), f"slot {s} (row {r} of {len(order)}) from position {q.pos}")
        q.pos += n
        assert e.batch_pos(s) == q.pos
        assert list(e.batch_tokens(s)) == list(q.full[:q.pos + 1]), (s, list(e.batch_tokens(s))[-4:], q.full[q.pos - 3:q.pos + 1])
        assert last[s] == q.full[q.pos]
    assert all(last[s] == -1 for s in range(G.BATCH_MAX_SLOTS) if s not in slots)
    return lg


def test_one_slot_consumes_its_prompt_then_decodes():
    shape = dict(O.TINY)
    q = Seq(shape, 256, 20)
    e = _engine(shape)
    e.batch_open(1)
    _begin(e, 0, q)
    _step(e, {0: q}, 23)  # rows 0 .. 19 the oracle's prefill rows, then 3 decode rows
    assert list(e.batch_tokens(0)) == list(q.full[:24])
    e.close()


def test_ragged_positions_in_slots_0_2_7():
    """slot 0 from 30 (the padded n_kv bumps at 32 inside the run), slot 2 from 62 (crosses key 64),
    slot 7 still consuming its 5 given tokens while the others generate (the nfix guard)"""
    shape = dict(O.TINY)
    a, b, c = Seq(shape, 256, 30, seed=1), Seq(shape, 256, 62, seed=2), Seq(shape, 256, 5, seed=3)
    e = _engine(shape)
    e.batch_open(8)
    _adopt(e, 0, a)
    _adopt(e, 2, b)
    _begin(e, 7, c)
    _step(e, {0: a, 2: b, 7: c}, 6)
    e.close()


def test_eight_slots():
    """R = 8: prompts from seeds 1 .. 8 of lengths 3 .. 10, which end on different passes"""
    shape = dict(O.TINY)
    seqs = {s: Seq(shape, 256, 3 + s, seed=1 + s) for s in range(8)}
    e = _engine(shape)
    e.batch_open(8)
    for s, q in seqs.items():
        _begin(e, s, q)
    _step(e, seqs, 12)
    e.close()


def test_past_256_keys():
    """n_ctx = 512, slots from 250 and 300: the attention's 256-position V staging and second KQ round"""
    shape = dict(O.TINY)
    a, b = Seq(shape, 512, 250, seed=1, n_dec=10), Seq(shape, 512, 300, seed=2, n_dec=10)
    e = _engine(shape, n_ctx=512)
    e.batch_open(2)
    _adopt(e, 0, a)
    _adopt(e, 1, b)
    _step(e, {0: a, 1: b}, 10)
    e.close()


@pytest.mark.parametrize("shape,n_ctx,R,adopt_at,okw,ekw", [
    (G8, 256, 3, 0, {}, {}),
    (K2B, 256, 3, 40, {}, {}),
    (dict(O.TINY), 256, 2, 0, dict(wtype=O.Q8_0), dict(wtype=G.GGML_TYPE_Q8_0)),
    (dict(O.TINY), 256, 2, 0, dict(kmix=2), dict(out_type=G.GGML_TYPE_Q6_K)),
    (KSHAPE, 128, 3, 0, dict(kmix=1), dict(wtype=G.GGML_TYPE_Q4_K)),
], ids=["G8", "K2B", "Q8_0", "Q6K_head", "kquant_layers"])
def test_shapes(shape, n_ctx, R, adopt_at, okw, ekw):
    seqs = {s: Seq(shape, n_ctx, 2 + s, seed=1 + s, n_dec=4, **okw) for s in range(R)}
    if adopt_at:
        seqs[1] = Seq(shape, n_ctx, adopt_at, seed=9, n_dec=4, **okw)
    e = _engine(shape, n_ctx=n_ctx, **ekw)
    e.batch_open(R)
    for s, q in seqs.items():
        if adopt_at and s == 1:
            _adopt(e, s, q)
        else:
            _begin(e, s, q)
    _step(e, seqs, 4)
    e.close()


def test_join_and_leave_and_the_cache_state():
    """R goes 1 -> 2 -> 1 -> 2, every row checked; then every layer's whole cache of each slot equals a
    plain engine's that ran the same sequence, and rows at and past pos are zero: the re-begun slot
    holds nothing of its previous sequence"""
    shape, n_ctx = dict(O.TINY), 256
    a, b, a2 = Seq(shape, n_ctx, 4, seed=1), Seq(shape, n_ctx, 6, seed=2), Seq(shape, n_ctx, 2, seed=3)
    e = _engine(shape)
    e.batch_open(2)
    _begin(e, 0, a)
    _step(e, {0: a}, 3)
    _begin(e, 1, b)
    _step(e, {0: a, 1: b}, 3)
    e.batch_release(0)
    assert e.batch_pos(0) == -1
    _step(e, {1: b}, 3)
    _begin(e, 0, a2)
    _step(e, {0: a2, 1: b}, 3)
    p = _engine(shape)
    for s, q in ((0, a2), (1, b)):
        p.begin(q.prompt)
        p.step(q.pos, use_graph=False)
        assert list(p.tokens()) == list(e.batch_tokens(s))
        for il in range(shape["n_layer"]):
            kb, vb = e.batch_kv_read(s, il, 0, n_ctx)
            kp, vp = p.kv_read(il, 0, n_ctx)
            assert np.array_equal(kb, kp) and np.array_equal(vb, vp), (s, il)
            assert kb[:q.pos].any() and not kb[q.pos:].any() and not vb[q.pos:].any(), (s, il)
    p.close()
    e.close()


def test_sampler_on():
    """tokens and logits equal plain engines with the same sampler; equal prompts give equal sequences"""
    shape, n = dict(O.TINY), 8
    prompts = [tuple(int(t) for t in O.make_prompt(3 + s, shape["n_vocab"], seed=11 + s)) for s in range(3)]
    prompts.append(prompts[0])
    e = _engine(shape)
    e.set_sampler(**SAMPLER)
    e.batch_open(4)
    for s, pr in enumerate(prompts):
        e.batch_begin(s, pr)
    lg = e.batch_step(n, want_logits=True)
    p = _engine(shape)
    p.set_sampler(**SAMPLER)
    for s, pr in enumerate(prompts):
        p.begin(pr)
        ref = p.step(n, want_logits=True, use_graph=False)
        _bits_equal(lg[:, s], ref, f"sampled slot {s}")
        assert list(e.batch_tokens(s)) == list(p.tokens())
    t0, t3 = list(e.batch_tokens(0)), list(e.batch_tokens(3))
    assert t0 == t3 and len(set(t0[len(prompts[0]):])) > 1, t0  # the sampler did draw varied tokens
    p.close()
    e.close()


def test_one_call_of_five_passes_equals_five_calls():
    shape = dict(O.TINY)
    out = []
    for calls in ((5,), (1, 1, 1, 1, 1)):
        a, b = Seq(shape, 256, 3, seed=1), Seq(shape, 256, 20, seed=2)
        e = _engine(shape)
        e.batch_open(2)
        _begin(e, 0, a)
        _adopt(e, 1, b)
        lg = np.concatenate([_step(e, {0: a, 1: b}, n) for n in calls])
        out.append((lg, list(e.batch_tokens(0)), list(e.batch_tokens(1))))
        e.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert out[0][1:] == out[1][1:]


def test_the_engines_own_sequence_is_untouched():
    shape, n, k = dict(O.TINY), 20, 2
    own = Seq(shape, 256, n, seed=1)
    other = Seq(shape, 256, 4, seed=5)
    dec, full = own.rows[n:], own.full
    e = _engine(shape)
    e.begin(own.prompt)
    e.prefill(n)
    _bits_equal(e.step(1, want_logits=True, use_graph=True), dec[:1], "the step before the batch")
    kernels = e.graph_kernels()
    e.batch_open(2)
    e.batch_adopt(0)
    adopted = Seq(shape, 256, n, seed=1)
    adopted.pos = n + 1
    _begin(e, 1, other)
    _step(e, {0: adopted, 1: other}, 4)
    assert e.pos() == n + 1 and list(e.tokens()) == list(full[:n + 2])
    _bits_equal(e.step(3, want_logits=True, use_graph=True), dec[1:4], "graph steps after the batch passes")
    assert e.graph_kernels() == kernels
    assert list(e.tokens()) == list(full[:n + 5])
    pos = n + 4  # one verify pass, all drafts right (tests/test_gpu_verify.py _check_pass)
    toks, rows = e.verify([int(t) for t in full[pos + 1:pos + 1 + k]], want_all=True)
    assert toks == [int(t) for t in full[pos + 1:pos + k + 2]] and e.pos() == pos + k + 1
    _bits_equal(rows, dec[4:4 + k + 1], "verify pass after the batch passes")
    e.close()


def _refused(r, fn):
    assert r == -1 and ("gemma_engine_batch_" + fn) in G.last_error(), (r, G.last_error())


def test_refusals():
    shape, n_ctx, V = dict(O.TINY), 256, O.TINY["n_vocab"]
    a, b = Seq(shape, n_ctx, 20, seed=1), Seq(shape, n_ctx, 3, seed=2)
    tok = np.ascontiguousarray(b.prompt, dtype=np.int32)
    e = _engine(shape)
    L, h, p = e.L, e.h, G._p
    # before open
    _refused(L.gemma_engine_batch_begin(h, 0, p(tok), 3), "begin")
    _refused(L.gemma_engine_batch_adopt(h, 0), "adopt")
    _refused(L.gemma_engine_batch_release(h, 0), "release")
    _refused(L.gemma_engine_batch_step(h, 1, None), "step")
    _refused(L.gemma_engine_batch_pos(h, 0), "pos")
    _refused(L.gemma_engine_batch_tokens(h, 0, p(tok), 3), "tokens")
    _refused(L.gemma_engine_batch_last(h, p(np.zeros(8, np.int32))), "last")
    _refused(L.gemma_engine_batch_close(h), "close")
    # open
    _refused(L.gemma_engine_batch_open(h, 0), "open")
    _refused(L.gemma_engine_batch_open(h, 9), "open")
    e.batch_open(2)
    _refused(L.gemma_engine_batch_open(h, 2), "open")
    _refused(L.gemma_engine_batch_step(h, 1, None), "step")  # no active slot
    _adopt(e, 0, a)
    # slots and tokens
    for slot in (-1, 2):
        _refused(L.gemma_engine_batch_begin(h, slot, p(tok), 3), "begin")
        _refused(L.gemma_engine_batch_adopt(h, slot), "adopt")
        _refused(L.gemma_engine_batch_release(h, slot), "release")
        _refused(L.gemma_engine_batch_pos(h, slot), "pos")
        _refused(L.gemma_engine_batch_kv_read(h, slot, 0, 0, 1, p(np.zeros(256, np.uint16)), p(np.zeros(256, np.uint16))), "kv_read")
    bad = np.ascontiguousarray([1, V, 2], dtype=np.int32)
    _refused(L.gemma_engine_batch_begin(h, 1, p(bad), 3), "begin")
    long = np.ones(n_ctx, dtype=np.int32)
    _refused(L.gemma_engine_batch_begin(h, 1, p(long), n_ctx), "begin")
    _refused(L.gemma_engine_batch_begin(h, 1, p(tok), 0), "begin")
    assert e.batch_pos(1) == -1
    # a step that would fill a slot's context: no slot advances
    _begin(e, 1, b)
    _refused(L.gemma_engine_batch_step(h, n_ctx - 20, None), "step")  # slot 0 at 20
    assert (e.batch_pos(0), e.batch_pos(1)) == (20, 0)
    _step(e, {0: a, 1: b}, 2)  # and a valid step after all of it is exact
    e.batch_close()
    _refused(L.gemma_engine_batch_adopt(h, 0), "adopt")
    _refused(L.gemma_engine_batch_step(h, 1, None), "step")
    e.close()
    # engines the batch does not serve
    v = _engine(shape, tp=(2, 0, None))
    _refused(v.L.gemma_engine_batch_open(v.h, 2), "open")
    v.close()
    big = _engine(shape, n_ctx=4096)
    _refused(big.L.gemma_engine_batch_open(big.h, 2), "open")
    big.close()


def test_memory_returns_to_the_baseline():
    shape = dict(O.TINY)
    q = Seq(shape, 256, 3, seed=2)
    base = G.mem_live()
    e = _engine(shape)
    before = G.mem_live()
    e.batch_open(8)
    assert G.mem_live()[0] > before[0] and G.mem_live()[1] > before[1]
    _begin(e, 5, q)
    _step(e, {5: q}, 2)
    e.batch_close()
    assert G.mem_live() == before
    e.batch_open(3)
    _begin(e, 2, q)
    _step(e, {2: q}, 2)
    e.close()  # with the batch still open
    assert G.mem_live() == base
