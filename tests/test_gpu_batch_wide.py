"""Wide batched decode (gemma_engine_batch_open_wide): up to 64 slots, passes of more than 8 rows.

The yardstick is tests/test_gpu_batch.py's: the oracle's single-sequence run per slot (Seq, _truth,
_bits_equal), uint32 equality of every logits row, every token and every position, whatever the other
rows of the pass are and whichever form the pass takes:
  R <= 8             the skinny pass (unchanged)
  R >= bt_mfma_min   one pass on the exact MFMA GEMMs (columns past R clamped)
  else               consecutive groups of up to 8 rows, each a skinny pass over its rows of the scratch
With the sampler on the reference is a plain Engine stepping with the same sampler.

The shapes are the smallest at which a wide pass can go wrong: R = 9 (one token tile, 55 clamped
columns), R = 33 (across the 32-token boundary of the 64 x 32 form, into the upper half of the
64-token tile) under every exact-GEMM form, R = 64 (nothing clamped), slots spread over [0, 64) at
ragged positions, an active set that moves the pass between the forms, groups of 8 + 4, positions
past 256 keys, G = 8 / 2 query heads per kv head, Q8_0, the Q6_K head and K-quant layers."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_batch import SAMPLER, Seq, _adopt, _begin, _engine
from test_gpu_prefill_continue import G8, K2B, KSHAPE, _bits_equal

pytestmark = pytest.mark.gpu

N_DEC = 6  # oracle decode steps kept per sequence: no slot below generates more
NEVER = G.BATCH_WIDE_MAX_SLOTS + 1  # bt_mfma_min: every pass of more than 8 rows in groups


def _seq(shape, n_ctx, n_prompt, seed, **kw):
    return Seq(shape, n_ctx, n_prompt, seed=seed, n_dec=N_DEC, **kw)


def _pool(i, shape=None, n_ctx=256):
    """sequence i of a fixed family: prompts of 2 .. 10 tokens, the oracle run shared by every test"""
    return _seq(shape or dict(O.TINY), n_ctx, 2 + i % 9, seed=1 + i)


def _step(e, slots, n):
    """n passes over the active slots {slot: Seq}; every row, position and token against the oracle"""
    lg = e.batch_step(n, want_logits=True)
    order = sorted(slots)
    assert lg.shape[:2] == (n, len(order))
    last = e.batch_last_n()
    for r, s in enumerate(order):
        q = slots[s]
        _bits_equal(lg[:, r], q.expect(n), f"slot {s} (row {r} of {len(order)}) from position {q.pos}")
        q.pos += n
        assert e.batch_pos(s) == q.pos
        assert list(e.batch_tokens(s)) == list(q.full[:q.pos + 1]), (s, list(e.batch_tokens(s))[-4:], q.full[q.pos - 3:q.pos + 1])
        assert last[s] == q.full[q.pos]
    assert all(last[s] == -1 for s in range(len(last)) if s not in slots)
    return lg


def _wide(n_slots, mfma_min=9, shape=None, n_ctx=256, **kw):
    e = _engine(shape or dict(O.TINY), n_ctx=n_ctx, **kw)
    e.batch_open_wide(n_slots)
    e.set_option("bt_mfma_min", mfma_min)
    return e


def test_nine_rows_on_the_mfma_gemms():
    """R = 9: one 64-token tile with 55 clamped columns; prompts of 2 .. 10 tokens end on different passes"""
    seqs = {s: _pool(s) for s in range(9)}
    e = _wide(9)
    for s, q in seqs.items():
        _begin(e, s, q)
    _step(e, seqs, 6)
    e.close()


def _full_width(R, passes=3):
    seqs = {s: _pool(s if s < 33 else (3 * s + 1) % 33) for s in range(R)}
    e = _wide(R)
    for s, q in seqs.items():
        _begin(e, s, q)
    _step(e, seqs, passes)
    e.close()


@pytest.mark.parametrize("x4", [3, 2, 0], ids=["x4_i8", "x4_f16", "x_w32"])
def test_33_rows_under_every_exact_gemm_form(x4):
    L = G.lib()
    try:
        L.hpc_set_gemm_x4(x4)
        _full_width(33)
    finally:
        L.hpc_set_gemm_x4(3)


def test_64_rows():
    _full_width(64)


def test_sparse_slots_and_ragged_positions():
    """slots {0, 7, 8, 9, 31, 32, 40, 62, 63} of 64: slot 8 from 30 (the padded n_kv bumps at 32 inside
    the run), slot 40 from 62 (crosses key 64), slot 63 still consuming its 10 given tokens while the
    others generate (the nfix guard)"""
    shape = dict(O.TINY)
    seqs = {s: _pool(i) for i, s in enumerate((0, 7, 9, 31, 32, 62))}  # prompts of 2 .. 7 tokens
    seqs[8], seqs[40], seqs[63] = _seq(shape, 256, 30, 41), _seq(shape, 256, 62, 42), _pool(8)
    assert len(seqs[63].prompt) == 10
    e = _wide(64)
    for s, q in seqs.items():
        (_adopt if s in (8, 40) else _begin)(e, s, q)
    _step(e, seqs, 2)
    _step(e, seqs, 3)
    e.close()


def test_the_form_follows_the_active_set_and_the_cache_state():
    """8 rows (skinny), a ninth joins (MFMA), two leave (skinny), then 12 rows with the MFMA form off
    (groups of 8 + 4): every call checked; afterwards one slot of each group holds the caches a plain
    engine has for the same sequence, zero at and past pos"""
    shape, n_ctx = dict(O.TINY), 256
    e = _wide(12)
    act = {s: _pool(s) for s in range(8)}
    for s, q in act.items():
        _begin(e, s, q)
    _step(e, act, 2)
    act[8] = _pool(8)
    _begin(e, 8, act[8])
    _step(e, act, 1)
    for s in (2, 5):
        e.batch_release(s)
        del act[s]
        assert e.batch_pos(s) == -1
    _step(e, act, 1)
    e.set_option("bt_mfma_min", NEVER)
    for s in (2, 5, 9, 10, 11):
        act[s] = _pool(s + 10)
        _begin(e, s, act[s])
    assert len(act) == 12
    _step(e, act, 2)
    p = _engine(shape)
    for s in (1, 11):  # rows 1 and 11: the first and the second group
        q = act[s]
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


def test_past_256_keys():
    """n_ctx = 512, 9 slots, two of them from 250 and 300: the attention's 256-position V staging and
    second KQ round among rows at short positions"""
    shape = dict(O.TINY)
    seqs = {s: _pool(s, n_ctx=512) for s in range(9)}
    seqs[3], seqs[7] = _seq(shape, 512, 250, 1), _seq(shape, 512, 300, 2)
    e = _wide(9, n_ctx=512)
    for s, q in seqs.items():
        (_adopt if s in (3, 7) else _begin)(e, s, q)
    _step(e, seqs, 4)
    e.close()


@pytest.mark.parametrize("shape,n_ctx,distinct,okw,ekw", [
    (G8, 256, 9, {}, {}),
    (K2B, 256, 3, {}, {}),
    (dict(O.TINY), 256, 9, dict(wtype=O.Q8_0), dict(wtype=G.GGML_TYPE_Q8_0)),
    (dict(O.TINY), 256, 9, dict(kmix=2), dict(out_type=G.GGML_TYPE_Q6_K)),
    (KSHAPE, 128, 9, dict(kmix=1), dict(wtype=G.GGML_TYPE_Q4_K)),
], ids=["G8", "K2B", "Q8_0", "Q6K_head", "kquant_layers"])
def test_shapes(shape, n_ctx, distinct, okw, ekw):
    """R = 9, 3 passes (K2B: three distinct sequences among the nine slots, the oracle's time)"""
    seqs = {s: Seq(shape, n_ctx, 2 + s % distinct % 3, seed=1 + s % distinct, n_dec=3, **okw) for s in range(9)}
    e = _wide(9, shape=shape, n_ctx=n_ctx, **ekw)
    for s, q in seqs.items():
        _begin(e, s, q)
    _step(e, seqs, 3)
    e.close()


@pytest.mark.parametrize("mfma_min", [9, NEVER], ids=["mfma", "groups"])
def test_sampler_on(mfma_min):
    """R = 10: tokens and logits equal plain engines with the same sampler (every row's draw in its own
    workspace, its position read through the row table); equal prompts give equal sequences"""
    shape, n = dict(O.TINY), 6
    prompts = [tuple(int(t) for t in O.make_prompt(2 + s, shape["n_vocab"], seed=11 + s)) for s in range(9)]
    prompts.append(prompts[0])
    e = _engine(shape)
    e.set_sampler(**SAMPLER)
    e.batch_open_wide(10)
    e.set_option("bt_mfma_min", mfma_min)
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
    t0, t9 = list(e.batch_tokens(0)), list(e.batch_tokens(9))
    assert t0 == t9 and len(set(t0[len(prompts[0]):])) > 1, t0  # the sampler did draw varied tokens
    p.close()
    e.close()


def test_one_call_of_five_passes_equals_five_calls():
    out = []
    for calls in ((5,), (1, 1, 1, 1, 1)):
        seqs = {s: _pool(s) for s in range(9)}
        e = _wide(9)
        for s, q in seqs.items():
            _begin(e, s, q)
        lg = np.concatenate([_step(e, seqs, n) for n in calls])
        out.append((lg, [list(e.batch_tokens(s)) for s in range(9)]))
        e.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert out[0][1] == out[1][1]


def test_the_engines_own_sequence_is_untouched():
    shape, n, k = dict(O.TINY), 20, 2
    own = Seq(shape, 256, n, seed=1)
    dec, full = own.rows[n:], own.full
    e = _engine(shape)
    e.begin(own.prompt)
    e.prefill(n)
    _bits_equal(e.step(1, want_logits=True, use_graph=True), dec[:1], "the step before the batch")
    kernels = e.graph_kernels()
    e.batch_open_wide(16)
    e.set_option("bt_mfma_min", 9)
    e.batch_adopt(3)
    adopted = Seq(shape, 256, n, seed=1)
    adopted.pos = n + 1
    act = {3: adopted}
    for i, s in enumerate((0, 1, 4, 8, 9, 12, 14, 15)):
        act[s] = _pool(i)
        _begin(e, s, act[s])
    _step(e, act, 4)
    assert e.pos() == n + 1 and list(e.tokens()) == list(full[:n + 2])
    _bits_equal(e.step(3, want_logits=True, use_graph=True), dec[1:4], "graph steps after the wide passes")
    assert e.graph_kernels() == kernels
    assert list(e.tokens()) == list(full[:n + 5])
    pos = n + 4  # one verify pass, all drafts right (tests/test_gpu_verify.py _check_pass)
    toks, rows = e.verify([int(t) for t in full[pos + 1:pos + 1 + k]], want_all=True)
    assert toks == [int(t) for t in full[pos + 1:pos + k + 2]] and e.pos() == pos + k + 1
    _bits_equal(rows, dec[4:4 + k + 1], "verify pass after the wide passes")
    e.close()


def _refused(r, name):
    assert r == -1 and name in G.last_error(), (r, G.last_error())


def test_refusals():
    shape = dict(O.TINY)
    e = _engine(shape)
    L, h, p = e.L, e.h, G._p
    buf = np.zeros(64, np.int32)
    _refused(L.gemma_engine_batch_open_wide(h, 0), "gemma_engine_batch_open_wide")
    _refused(L.gemma_engine_batch_open_wide(h, 65), "gemma_engine_batch_open_wide")
    _refused(L.gemma_engine_batch_last_n(h, p(buf), 64), "gemma_engine_batch_last_n")  # no batch
    _refused(L.gemma_engine_set_option(h, b"bt_mfma_min", 8), "bt_mfma_min")
    _refused(L.gemma_engine_set_option(h, b"bt_mfma_min", 66), "bt_mfma_min")
    e.batch_open_wide(9)
    _refused(L.gemma_engine_batch_open_wide(h, 9), "gemma_engine_batch_open_wide")
    _refused(L.gemma_engine_batch_open(h, 2), "gemma_engine_batch_open")
    seqs = {s: _pool(s) for s in range(9)}
    for s, q in seqs.items():
        _begin(e, s, q)
    _step(e, seqs, 1)
    _refused(L.gemma_engine_batch_last(h, p(buf)), "gemma_engine_batch_last_n")  # names the call that serves 9 slots
    _refused(L.gemma_engine_batch_last_n(h, p(buf), 8), "gemma_engine_batch_last_n")
    _refused(L.gemma_engine_batch_last_n(h, None, 64), "gemma_engine_batch_last_n")
    assert not buf.any()  # no refused call wrote
    _refused(L.gemma_engine_set_option(h, b"bt_mfma_min", 8), "bt_mfma_min")
    _refused(L.gemma_engine_set_option(h, b"bt_mfma_min", 66), "bt_mfma_min")
    _refused(L.gemma_engine_batch_begin(h, 9, p(buf), 3), "gemma_engine_batch_begin")  # slot range = n_slots
    assert L.gemma_engine_batch_last_n(h, p(buf), 9) == 9 and (buf[9:] == 0).all()
    assert [e.batch_pos(s) for s in range(9)] == [1] * 9
    _step(e, seqs, 2)  # and a valid step after all of it is exact
    e.close()
    # a narrow batch through the general call; it still refuses a ninth slot
    e = _engine(shape)
    _refused(L.gemma_engine_batch_open(e.h, 9), "gemma_engine_batch_open")
    e.batch_open(2)
    assert list(e.batch_last_n()) == [-1, -1] and list(e.batch_last()) == [-1] * 8
    e.close()
    # engines the batch does not serve
    v = _engine(shape, tp=(2, 0, None))
    _refused(v.L.gemma_engine_batch_open_wide(v.h, 16), "gemma_engine_batch_open_wide")
    v.close()
    big = _engine(shape, n_ctx=4096)
    _refused(big.L.gemma_engine_batch_open_wide(big.h, 16), "gemma_engine_batch_open_wide")
    big.close()


def test_memory_returns_to_the_baseline():
    q = _pool(1)
    base = G.mem_live()
    e = _engine(dict(O.TINY))
    before = G.mem_live()
    e.batch_open_wide(64)
    assert G.mem_live()[0] > before[0] and G.mem_live()[1] > before[1]
    _begin(e, 40, q)
    _step(e, {40: q}, 2)
    e.batch_close()
    assert G.mem_live() == before
    e.batch_open_wide(12)
    _begin(e, 11, q)
    _step(e, {11: q}, 2)
    e.close()  # with the batch still open
    assert G.mem_live() == base
