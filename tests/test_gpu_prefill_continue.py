"""Batched prefill from any position: chunked prompts, steps mixed with batches, a second turn and
rewind (gemma_engine_extend / gemma_engine_prefill_next).

The yardstick is the oracle's T-token graph over the FULL sequence (the CPU path,
src/gemma_model.cpp:665-747): a pass over positions [p0, p0+n) against the caches of [0, p0) must
give rows [p0, p0+n) of that graph's logits bit for bit (uint32 views, no tolerance), and the decode
that follows must equal the oracle's decode steps.  The shapes are the smallest at which a position
offset can go wrong: a 1-row pass, a start at p0 = 31 (the first row bumps the padded n_kv), chunk
lengths that are no multiple of the 8 / 16 positions of an attn_mx block, crossings of key 64 and of
256 keys (k_attn_rows' 128-position KQ passes and 256-step KQV groups, attn_mx's second set of key
tiles per wave), G = 1 / 2 / 8 query heads per kv head, and kq_gemm_min = 8 from both sides."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_prefill import _check_rows  # the approximate path's bounds (FLIP_TOL, median < 3e-2)

pytestmark = pytest.mark.gpu

# the K-quant shape of tests/test_gpu_engine_gguf.py (hd 128: the row form of the attention)
KSHAPE = dict(n_layer=2, n_embd=256, n_head=2, n_head_kv=1, head_dim=128, n_ff=512, n_vocab=1024)
# the G = 8 shape of test_prefill_attention_mfma_equals_rows (tests/test_gpu_prefill.py)
G8 =dict(n_layer=2, n_embd=2048, n_head=8, n_head_kv=1, head_dim=256, n_ff=2048, n_vocab=4096)
K2B = dict(O.GEMMA_2B, n_layer=2, n_vocab=8192)
N_DECODE = 3


def _key(shape):
    return tuple(sorted(shape.items()))


@functools.lru_cache(maxsize=None)
def _truth(shape_key, n_ctx, wtype, kmix, seq, n_decode=N_DECODE):
    """The oracle over the whole sequence, computed once per case and shared: (greedy token after
    the last row, logits of every row, logits of the n_decode greedy steps that follow, the
    sequence with those steps' tokens).  Read-only for the tests."""
    m = O.Model(O.make_config(dict(shape_key), n_ctx=n_ctx, wtype=wtype, kmix=kmix))
    tok, _, all_ref = m.inference(list(seq), 0, want_all=True)
    full = list(seq) + [tok]
    dec = []
    for _ in range(n_decode):
        t, lg, _ = m.inference(full, 1)
        dec.append(lg)
        full.append(t)
    m.close()
    all_ref.setflags(write=False)
    dec = np.stack(dec) if dec else np.zeros((0, all_ref.shape[1]), np.float32)
    dec.setflags(write=False)
    return tok, all_ref, dec, full


def _bits_equal(got, ref, what):
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (what, "rows", bad[:8], np.abs(got - ref).max())


def _chunks(e, all_ref, chunks, exact=True):
    """prefill_next over `chunks` (0 = all that remain) from the engine's position; every pass's
    rows and last row against the oracle's; returns the last pass's token"""
    tok = None
    for n in chunks:
        p0 = e.pos()
        tok, last, allv = e.prefill_next(n, want_all=True, exact=exact)
        rows = all_ref[p0:p0 + allv.shape[0]]
        assert n == 0 or allv.shape[0] == n
        assert e.pos() == p0 + allv.shape[0]
        if exact:
            _bits_equal(allv, rows, f"pass at p0 = {p0}, n = {n}")
            _bits_equal(last, rows[-1], f"last row of the pass at p0 = {p0}")
    return tok


def _decode(e, truth):
    """the decode that continues from the caches the passes wrote: logits and tokens"""
    tok_ref, _, dec, full = truth
    lg = e.step(len(dec), want_logits=True, use_graph=True)
    _bits_equal(lg, dec, "decode after the last pass")
    assert list(e.tokens()) == full, (list(e.tokens())[-6:], full[-6:])


def _chunked_case(shape, n_prompt, n_ctx, chunks, att_mx=None, wtype=O.Q4_0, kmix=0, engine_kw=None):
    assert sum(chunks) == n_prompt
    prompt = tuple(int(t) for t in O.make_prompt(n_prompt, shape["n_vocab"]))
    truth = _truth(_key(shape), n_ctx, wtype, kmix, prompt)
    e = G.Engine(shape, n_ctx=n_ctx, device=0, **(engine_kw or dict(wtype=wtype)))
    if att_mx is not None:
        e.set_option("att_mx", att_mx)
    e.begin(prompt)
    for n in chunks[:-1]:  # a pass that ends mid-prompt appends nothing
        _chunks(e, truth[1], [n])
        assert list(e.tokens()) == list(prompt[:e.pos() + 1])
    tok = _chunks(e, truth[1], chunks[-1:])
    assert tok == truth[0], (tok, truth[0])
    _decode(e, truth)
    e.close()


MX = pytest.mark.parametrize("att_mx", [1, 0], ids=["attn_mx", "attn_rows"])


@MX
def test_chunked_equals_one_graph(att_mx):
    _chunked_case(dict(O.TINY), 100, 256, (1, 30, 33, 36), att_mx)


@MX
def test_chunked_past_256_keys(att_mx):
    _chunked_case(dict(O.TINY), 300, 352, (130, 127, 43), att_mx)


@MX
def test_chunked_q8_0_gqa(att_mx):
    _chunked_case(dict(O.TINY, n_head=4, n_head_kv=2), 70, 256, (37, 33), att_mx, wtype=O.Q8_0)


@MX
def test_chunked_mha(att_mx):
    _chunked_case(dict(O.TINY, n_head=4, n_head_kv=4), 45, 128, (17, 28), att_mx)


@MX
def test_chunked_eight_heads_per_kv_head(att_mx):
    _chunked_case(G8, 150, 192, (70, 9, 71), att_mx)


def test_chunked_across_the_attn_mx_lds_limit():
    """attn_mx holds 16 score rows of p0 + T keys in the LDS (at most 2556 keys).  Chunks (1200,
    1300, 100) of a 2600-token prompt: the second pass is the matrix-core form at its largest size
    with p0 > 0 (2500 keys), the third reaches 2600 keys and takes the row form with p0 = 2500.
    The reference is this engine's own one-pass prefill (T = 2600: the row form, which the tests of
    tests/test_gpu_prefill.py tie to the oracle); the oracle's T^2 attention is too slow here."""
    shape, T, n_ctx = dict(O.TINY), 2600, 2688
    prompt = O.make_prompt(T, shape["n_vocab"], seed=5)
    e = G.Engine(shape, n_ctx=n_ctx, device=0)
    e.begin(prompt)
    tok_ref, _, all_ref = e.prefill(T, want_all=True)
    dec_ref = e.step(N_DECODE, want_logits=True, use_graph=True)
    full = list(e.tokens())
    e.extend(prompt, keep=0)
    for n in (1200, 1300):
        _chunks(e, all_ref, [n])
    assert _chunks(e, all_ref, [100]) == tok_ref
    _decode(e, (tok_ref, all_ref, dec_ref, full))
    e.close()


def _tiny(n_prompt, n_ctx=256):
    shape = dict(O.TINY)
    prompt = tuple(int(t) for t in O.make_prompt(n_prompt, shape["n_vocab"]))
    return shape, prompt, _truth(_key(shape), n_ctx, O.Q4_0, 0, prompt), G.Engine(shape, n_ctx=n_ctx, device=0)


def test_steps_then_batch():
    shape, prompt, truth, e = _tiny(60)
    e.begin(prompt)
    lg = e.step(13, want_logits=True, use_graph=True)
    _bits_equal(lg, truth[1][:13], "13 steps over the prompt")
    assert _chunks(e, truth[1], [0]) == truth[0] and e.pos() == 60
    _decode(e, truth)
    e.close()


@pytest.mark.parametrize("shape,kmix,engine_kw", [(dict(O.TINY), 2, dict(out_type=G.GGML_TYPE_Q6_K)),
                                                  (KSHAPE, 1, dict(wtype=G.GGML_TYPE_Q4_K))],
                         ids=["q6K_output", "kquant_layers"])
def test_steps_then_larger_batch_then_steps(shape, kmix, engine_kw):
    """The captured decode graph holds the address of the 1-row Q8_K image of the output norm (Q6_K
    head, K-quant `down` hand-off).  A 47-row pass after the capture must leave that address alone:
    graph steps, the batch, then graph steps again, every row and step against the oracle."""
    n_ctx = 128
    prompt = tuple(int(t) for t in O.make_prompt(60, shape["n_vocab"]))
    truth = _truth(_key(shape), n_ctx, O.Q4_0, kmix, prompt)
    e = G.Engine(shape, n_ctx=n_ctx, device=0, **engine_kw)
    e.begin(prompt)
    lg = e.step(13, want_logits=True, use_graph=True)
    _bits_equal(lg, truth[1][:13], "13 graph steps over the prompt")
    n_graph = e.graph_kernels()
    assert _chunks(e, truth[1], [0]) == truth[0] and e.pos() == 60  # 47 rows in one pass
    _decode(e, truth)
    assert e.graph_kernels() == n_graph  # the same captured graph ran before and after the pass
    e.close()


def test_batch_steps_batch():
    shape, prompt, truth, e = _tiny(60)
    e.begin(prompt)
    _chunks(e, truth[1], [20])
    lg = e.step(5, want_logits=True, use_graph=True)  # consume given tokens: nothing is appended
    _bits_equal(lg, truth[1][20:25], "5 steps after a 20-row pass")
    assert e.pos() == 25 and list(e.tokens()) == list(prompt[:26])
    assert _chunks(e, truth[1], [0]) == truth[0] and e.pos() == 60
    _decode(e, truth)
    e.close()


def _first_turn(e, shape):
    """begin(40) + prefill + 5 steps: 46 tokens, position 45, the last one pending"""
    p1 = [int(t) for t in O.make_prompt(40, shape["n_vocab"])]
    e.begin(p1)
    e.prefill(len(p1))
    e.step(5, use_graph=True)
    toks = [int(t) for t in e.tokens()]
    assert e.pos() == 45 and len(toks) == 46 and toks[:40] == p1
    return toks


def test_second_turn_and_rewind():
    shape = dict(O.TINY)
    e = G.Engine(shape, n_ctx=256, device=0)
    toks = _first_turn(e, shape)
    n_graph = e.graph_kernels()
    turn2 = [int(t) for t in O.make_prompt(23, shape["n_vocab"], seed=7)]
    e.extend(turn2)  # keep everything, the pending token included
    seq = tuple(toks + turn2)
    assert e.pos() == 45 and list(e.tokens()) == list(seq[:46])
    truth = _truth(_key(shape), 256, O.Q4_0, 0, seq)
    # the first turn's generated tokens are the oracle's greedy tokens of rows 39 .. 44
    assert [int(r.argmax()) for r in truth[1][39:45]] == toks[40:46]
    assert _chunks(e, truth[1], [0]) == truth[0] and e.pos() == len(seq)
    _decode(e, truth)
    assert e.graph_kernels() == n_graph  # the captured decode graph was kept
    # ---- rewind to position 42 and continue differently --------------------------------------
    other = [int(t) for t in O.make_prompt(19, shape["n_vocab"], seed=11)]
    e.extend(other, keep=42)
    seq2 = tuple(list(seq[:42]) + other)
    assert e.pos() == 42 and list(e.tokens()) == list(seq2[:43])
    truth2 = _truth(_key(shape), 256, O.Q4_0, 0, seq2)
    tok = _chunks(e, truth2[1], [0])
    assert tok == truth2[0]
    f = G.Engine(shape, n_ctx=256, device=0)  # a fresh engine given the same sequence
    f.begin(seq2)
    tok_f, last_f, all_f = f.prefill(len(seq2), want_all=True)
    _bits_equal(all_f, truth2[1], "fresh engine")
    assert tok_f == tok
    lg_f = f.step(N_DECODE, want_logits=True, use_graph=True)
    _bits_equal(lg_f, truth2[2], "fresh engine's decode")
    toks_f = list(f.tokens())
    f.close()
    _decode(e, truth2)
    assert list(e.tokens()) == toks_f
    assert e.graph_kernels() == n_graph
    e.close()


def test_extend_keep_0_is_begin():
    shape, prompt, truth, e = _tiny(60)
    _first_turn(e, shape)  # a used engine: caches, history and position hold another sequence
    e.extend(prompt, keep=0)
    assert e.pos() == 0 and list(e.tokens()) == [prompt[0]]
    tok, last, allv = e.prefill(len(prompt), want_all=True)  # "right after begin" holds
    _bits_equal(allv, truth[1], "prefill after extend(keep=0)")
    assert tok == truth[0]
    _decode(e, truth)
    e.close()


def test_extend_keep_none_needs_a_consumed_prompt():
    shape, prompt, truth, e = _tiny(60)
    e.begin(prompt)
    e.prefill_next(20)
    with pytest.raises(ValueError):
        e.extend([1, 2, 3])
    assert e.pos() == 20
    e.close()


@pytest.mark.parametrize("shape,n_ctx,n_prompt,chunks", [(KSHAPE, 128, 50, (5, 40, 5)), (K2B, 256, 40, (19, 21))],
                         ids=["hd128", "gemma2b_layers"])
def test_chunked_kquant_layers(shape, n_ctx, n_prompt, chunks):
    """K-quant layers (Q4_K_M layout): chunks on both sides of kq_gemm_min = 8 (the MFMA GEMM and
    the dot4 T-column kernel); hd 128 takes the row form of the attention"""
    _chunked_case(shape, n_prompt, n_ctx, chunks, kmix=1, engine_kw=dict(wtype=G.GGML_TYPE_Q4_K))


def test_chunked_q6K_output():
    _chunked_case(dict(O.TINY), 50, 128, (7, 30, 13), kmix=2, engine_kw=dict(out_type=G.GGML_TYPE_Q6_K))


def test_chunked_approximate_path():
    """exact=False (int8 / f16 MFMA): the rows of both passes within the bounds
    tests/test_gpu_prefill.py sets for this path (_check_rows: FLIP_TOL, median < 3e-2)"""
    shape, prompt, truth, e = _tiny(100)
    e.begin(prompt)
    rows = []
    for n in (40, 60):
        tok, last, allv = e.prefill_next(n, want_all=True, exact=False)
        rows.append(allv)
    assert e.pos() == 100 and len(e.tokens()) == 101
    _check_rows(np.concatenate(rows), truth[1])
    e.close()
    k = G.Engine(KSHAPE, n_ctx=128, wtype=G.GGML_TYPE_Q4_K)
    k.begin(O.make_prompt(20, KSHAPE["n_vocab"]))
    with pytest.raises(RuntimeError, match="K-quant"):
        k.prefill_next(10, exact=False)
    assert k.pos() == 0
    k.close()


def test_refusals_leave_the_state():
    shape = dict(O.TINY)
    n_ctx = 128
    e = G.Engine(shape, n_ctx=n_ctx, device=0)
    prompt = [int(t) for t in O.make_prompt(30, shape["n_vocab"])]
    e.begin(prompt)
    e.prefill_next(10)

    def refused(fn, *a, **kw):
        pos, toks = e.pos(), list(e.tokens())
        with pytest.raises(RuntimeError) as ei:
            fn(*a, **kw)
        assert ": gemma_engine_" in str(ei.value) and len(str(ei.value)) > 40, str(ei.value)
        assert e.pos() == pos and list(e.tokens()) == toks

    refused(e.extend, [1, 2], keep=11)                       # keep > pos
    refused(e.extend, [1, 2], keep=-1)
    refused(e.extend, [], keep=5)                            # n = 0
    refused(e.extend, [1] * (n_ctx - 5), keep=5)             # keep + n >= n_ctx
    refused(e.extend, [1, shape["n_vocab"]], keep=5)         # token id out of range
    refused(e.extend, [-1], keep=5)
    refused(e.prefill_next, 21)                              # more than the 20 that remain
    e.prefill_next(0)
    assert e.pos() == 30
    refused(e.prefill_next, 0)                               # nothing pending
    refused(e.prefill_next, 1)
    e.close()
    t = G.Engine(shape, n_ctx=n_ctx, device=0, tp=(2, 0, None))  # virtual ranks: row-split engine
    t.begin(prompt)
    with pytest.raises(RuntimeError, match="single-GPU"):
        t.prefill_next(10)
    assert t.pos() == 0 and list(t.tokens()) == prompt[:1]
    t.close()
