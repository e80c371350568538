"""Speculative decoding: the exact multi-token verify pass (gemma_engine_verify), the state it leaves,
and the lookup generate loop (gemma_engine_generate_lookup).

The yardstick is the oracle (Model.inference over the prompt, then its greedy decode steps, as in
tests/test_gpu_prefill_continue.py): a pass over [pending token, k drafts] must return the oracle's
decode logits for every accepted row bit for bit (uint32 views), accept exactly the leading drafts
that equal the oracle's tokens, and leave an engine whose following graph steps are the oracle's.

Greedy decoding of the synthetic TINY model repeats one token, so the greedy cases use crafted drafts
(the oracle's tokens with one entry replaced); the varied sequences come from the sampler, where the
reference is a plain engine stepping with the same (seed, position) rule."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_prefill_continue import K2B, KSHAPE, _bits_equal, _key, _truth

pytestmark = pytest.mark.gpu

N_AFTER = 3  # graph steps checked after a pass
SAMPLER = dict(temperature=1.0, top_k=40, top_p=0.95, seed=20240607)


def _setup(shape, n_prompt, n_ctx, k, wtype=O.Q4_0, kmix=0, engine_kw=None, seed=1):
    """an engine whose prompt is consumed by the batched prefill (pos == n_prompt, the greedy token
    pending), and the oracle's truth: k + 1 + N_AFTER decode steps after the prompt"""
    prompt = tuple(int(t) for t in O.make_prompt(n_prompt, shape["n_vocab"], seed=seed))
    truth = _truth(_key(shape), n_ctx, wtype, kmix, prompt, k + 1 + N_AFTER)
    e = G.Engine(shape, n_ctx=n_ctx, device=0, **(engine_kw or dict(wtype=wtype)))
    e.begin(prompt)
    tok, _ = e.prefill(n_prompt)
    assert tok == truth[0] and e.pos() == n_prompt
    return e, prompt, truth


def _drafts(full, n, k, a, n_vocab):
    """the oracle's next k tokens, entry a replaced by another id (a == k: all right)"""
    d = [int(t) for t in full[n + 1:n + 1 + k]]
    if a < k:
        d[a] = (d[a] + 1) % n_vocab
    return d


def _check_pass(e, truth, n, k, a, n_vocab):
    _, _, dec, full = truth
    toks, rows = e.verify(_drafts(full, n, k, a, n_vocab), want_all=True)
    assert toks == [int(t) for t in full[n + 1:n + a + 2]], (toks, full[n + 1:n + a + 2])
    assert e.pos() == n + a + 1
    assert rows.shape == (k + 1, n_vocab)
    _bits_equal(rows[:a + 1], dec[:a + 1], f"rows of the pass at pos {n}, k = {k}, a = {a}")
    assert list(e.tokens()) == list(full[:n + a + 2])
    lg = e.step(N_AFTER, want_logits=True, use_graph=True)
    _bits_equal(lg, dec[a + 1:a + 1 + N_AFTER], "graph steps after the pass")
    assert list(e.tokens()) == list(full[:n + a + 2 + N_AFTER])


def _case(shape, n_prompt, n_ctx, k, a, att_mx=None, **kw):
    e, prompt, truth = _setup(shape, n_prompt, n_ctx, k, **kw)
    if att_mx is not None:
        e.set_option("att_mx", att_mx)
    _check_pass(e, truth, n_prompt, k, a, shape["n_vocab"])
    e.close()


@pytest.mark.parametrize("k", [1, 7])
def test_all_accepted(k):
    _case(dict(O.TINY), 20, 256, k, k)


def test_none_accepted():
    _case(dict(O.TINY), 20, 256, 4, 0)


@pytest.mark.parametrize("att_mx", [1, 0], ids=["attn_mx", "attn_rows"])
@pytest.mark.parametrize("a", [1, 3])
def test_partial(a, att_mx):
    _case(dict(O.TINY), 20, 256, 4, a, att_mx)


def test_prefix_rule_stops_at_the_first_mismatch():
    """a later draft that equals its row's pick does not count once an earlier one is wrong"""
    shape = dict(O.TINY)
    e, prompt, truth = _setup(shape, 20, 256, 4)
    n, full = 20, truth[3]
    wrong = (int(full[n + 1]) + 1) % shape["n_vocab"]
    toks, rows = e.verify([wrong, 5, 6, 7], want_all=True)
    assert toks == [int(full[n + 1])]
    g1 = int(rows[1].argmax())  # row 1's greedy pick under the wrong draft (first max, as np.argmax)
    e.extend([prompt[-1]], keep=n - 1)  # rewind: the last prompt token given again, then its step
    e.step(1, use_graph=True)
    assert e.pos() == n and list(e.tokens()) == list(full[:n + 1])
    toks2, rows2 = e.verify([wrong, g1, 6, 7], want_all=True)
    assert int(rows2[1].argmax()) == g1  # the later draft does equal its row's pick
    assert toks2 == [int(full[n + 1])] and e.pos() == n + 1
    _bits_equal(e.step(N_AFTER, want_logits=True, use_graph=True), truth[2][1:1 + N_AFTER], "steps after the rerun")
    e.close()


@pytest.mark.parametrize("n_prompt,a", [(30, 4), (30, 2), (62, 4), (62, 1)],
                         ids=["pos30_all", "pos30_partial", "across_key_64_all", "across_key_64_partial"])
def test_positions(n_prompt, a):
    """pos = 30: the padded n_kv changes inside the pass (rows 30, 31 | 32 ..); pos = 62: the pass
    crosses key 64"""
    _case(dict(O.TINY), n_prompt, 256, 4, a)


@pytest.mark.parametrize("a", [0, 2], ids=["none", "partial"])
def test_cache_state_equals_plain_steps(a):
    shape, n, k, n_ctx = dict(O.TINY), 20, 4, 256
    e, prompt, truth = _setup(shape, n, n_ctx, k)
    assert len(e.verify(_drafts(truth[3], n, k, a, shape["n_vocab"]))) == a + 1
    p = G.Engine(shape, n_ctx=n_ctx, device=0)  # the same sequence by plain steps
    p.begin(prompt)
    p.prefill(n)
    p.step(a + 1, use_graph=True)
    pos = e.pos()
    assert pos == p.pos() == n + a + 1 and list(e.tokens()) == list(p.tokens())
    for il in range(shape["n_layer"]):
        ke, ve = e.kv_read(il, 0, n_ctx)
        kp, vp = p.kv_read(il, 0, n_ctx)
        assert not ke[pos:].any() and not ve[pos:].any(), f"layer {il}: rows >= pos not zero"
        assert ke[:pos].any() and ve[:pos].any()
        assert np.array_equal(ke[:pos], kp[:pos]) and np.array_equal(ve[:pos], vp[:pos]), f"layer {il}"
        assert np.array_equal(ke, kp) and np.array_equal(ve, vp)
    e.close()
    p.close()


def _chain(e, ref, n_new, corrupt_every, n_vocab):
    """verify passes with drafts from `ref` (k cycling 1 .. 7), every corrupt_every-th pass with one
    wrong entry, until n_new tokens are appended; every returned token is checked against ref"""
    start, i = e.pos(), 0
    while e.pos() - start < n_new:
        pos, k = e.pos(), 1 + i % 7
        d = [int(t) for t in ref[pos + 1:pos + 1 + k]]
        a = k
        if i % corrupt_every == corrupt_every - 1:
            a = i % k
            d[a] = (d[a] + 1) % n_vocab
        toks = e.verify(d)
        assert toks == [int(t) for t in ref[pos + 1:pos + a + 2]], (i, pos, k, a, toks)
        i += 1
    return i


def test_chain_of_passes_equals_plain_steps():
    shape, n = dict(O.TINY), 20
    prompt = [int(t) for t in O.make_prompt(n, shape["n_vocab"])]
    p = G.Engine(shape, n_ctx=256, device=0)
    p.begin(prompt)
    p.prefill(n)
    p.step(1 + 40 + 7, use_graph=True)
    ref = [int(t) for t in p.tokens()]
    e = G.Engine(shape, n_ctx=256, device=0)
    e.begin(prompt)
    e.prefill(n)
    e.step(1, use_graph=True)  # captures the decode graph
    n_graph = e.graph_kernels()
    passes = _chain(e, ref, 40, 2, shape["n_vocab"])
    assert passes >= 8
    assert e.graph_kernels() == n_graph
    p.begin(prompt)  # the plain engine again, to the same position
    p.prefill(n)
    p.step(e.pos() - n, use_graph=True)
    assert e.pos() == p.pos() and list(e.tokens()) == list(p.tokens()) == ref[:e.pos() + 1]
    _bits_equal(e.step(1, want_logits=True, use_graph=True), p.step(1, want_logits=True, use_graph=True), "next step")
    assert e.graph_kernels() == n_graph
    e.close()
    p.close()


def _sampled_pair(n_new):
    shape, n = dict(O.TINY), 20
    prompt = [int(t) for t in O.make_prompt(n, shape["n_vocab"])]
    p = G.Engine(shape, n_ctx=256, device=0)
    p.set_sampler(**SAMPLER)
    p.begin(prompt)
    p.prefill(n)
    p.step(n_new + 7, use_graph=True)
    ref = [int(t) for t in p.tokens()]
    assert len(set(ref[n:n + 1 + n_new])) > 1, "the sampled run is constant: the test would prove nothing"
    e = G.Engine(shape, n_ctx=256, device=0)
    e.set_sampler(**SAMPLER)
    e.begin(prompt)
    e.prefill(n)
    assert list(e.tokens()) == ref[:n + 1]
    return shape, n, p, e, ref


def test_sampler_on_passes_equal_plain_steps():
    shape, n, p, e, ref = _sampled_pair(32)
    _chain(e, ref, 32, 3, shape["n_vocab"])
    assert list(e.tokens()) == ref[:e.pos() + 1] and e.pos() >= n + 32
    e.close()
    p.close()


def test_sampler_on_generate_lookup_equals_plain_steps():
    shape, n, p, e, ref = _sampled_pair(32)
    out, st = e.generate_lookup(32, k=4, ngram_max=3)
    assert out == ref[n + 1:n + 33] and e.pos() == n + 32
    assert st["passes"] + st["plain_steps"] + st["accepted"] == 32
    e.close()
    p.close()


@pytest.mark.parametrize("shape,n_ctx,n_prompt,k,a,kw", [
    (dict(O.TINY, n_head=4, n_head_kv=2), 256, 20, 4, 2, dict(wtype=O.Q8_0)),
    (K2B, 128, 9, 7, 7, {}),
    (K2B, 128, 9, 7, 3, {}),
    (KSHAPE, 128, 20, 4, 2, dict(kmix=1, engine_kw=dict(wtype=G.GGML_TYPE_Q4_K))),
    (KSHAPE, 128, 20, 7, 7, dict(kmix=1, engine_kw=dict(wtype=G.GGML_TYPE_Q4_K))),
    (dict(O.TINY), 128, 20, 4, 2, dict(kmix=2, engine_kw=dict(out_type=G.GGML_TYPE_Q6_K))),
], ids=["q8_0_gqa", "gemma2b_layers_T8", "gemma2b_layers_partial", "kquant_layers", "kquant_layers_T8", "q6K_output"])
def test_other_engines(shape, n_ctx, n_prompt, k, a, kw):
    _case(dict(shape), n_prompt, n_ctx, k, a, **kw)


def _lookup_run():
    """generate_lookup(48, k=4, ngram_max=3) after a 6-token make_prompt block repeated 4 times, beside
    a plain engine's step(48)"""
    shape = dict(O.TINY)
    block = [int(t) for t in O.make_prompt(6, shape["n_vocab"])]
    prompt = block * 4
    p = G.Engine(shape, n_ctx=256, device=0)
    p.begin(prompt)
    p.prefill(len(prompt))
    p.step(48, use_graph=True)
    e = G.Engine(shape, n_ctx=256, device=0)
    e.begin(prompt)
    e.prefill(len(prompt))
    out, st = e.generate_lookup(48, k=4, ngram_max=3)
    return len(prompt), p, e, out, st


def test_generate_lookup_equals_plain_steps():
    n, p, e, out, st = _lookup_run()
    ref = [int(t) for t in p.tokens()]
    assert out == ref[n + 1:n + 49]
    assert e.pos() == p.pos() == n + 48 and list(e.tokens()) == ref
    assert st["passes"] + st["plain_steps"] + st["accepted"] == 48, st
    assert st["accepted"] <= st["drafted"] <= 4 * st["passes"], st
    assert st["passes"] >= 1 and st["accepted"] >= 1, st  # passes ran and drafts were accepted
    _bits_equal(e.step(1, want_logits=True, use_graph=True), p.step(1, want_logits=True, use_graph=True), "next step")
    e.close()
    p.close()


def test_generate_lookup_accepts_two_drafts_per_pass():
    """accepted >= 2 * passes: the loop does not pass with no draft ever accepted, nor with one-token
    drafts.  TINY's greedy continuation is one repeated token, where a single lookup (most recent
    match, truncated at the sequence end) drafts one token; the loop grows the draft by repeated
    lookups over its own guesses.  A CPU simulation of the loop on the oracle's output gives 10 passes
    and 37 / 38 / 37 accepted drafts for prompt seeds 1, 2, 3."""
    n, p, e, out, st = _lookup_run()
    e.close()
    p.close()
    print("generate_lookup stats:", st)
    assert st["accepted"] >= 2 * st["passes"], st


def test_refusals_leave_the_state():
    shape, n_ctx = dict(O.TINY), 64
    V = shape["n_vocab"]
    prompt = [int(t) for t in O.make_prompt(58, V)]
    e = G.Engine(shape, n_ctx=n_ctx, device=0)

    def refused(eng, draft):
        pos, toks = eng.pos(), list(eng.tokens())
        with pytest.raises(RuntimeError, match="gemma_engine_verify") as ei:
            eng.verify(draft)
        assert len(str(ei.value)) > 40, str(ei.value)
        assert eng.pos() == pos and list(eng.tokens()) == toks

    e.begin(prompt)
    refused(e, [1, 2])                      # nothing processed: every given token is pending
    e.prefill_next(50)
    refused(e, [1, 2])                      # 8 given tokens still pending
    e.prefill_next(0)
    assert e.pos() == 58
    refused(e, [])                          # k = 0
    refused(e, [1] * 8)                     # k = 8
    refused(e, [1, V])                      # token id out of range
    refused(e, [-1])
    refused(e, [1] * 5)                     # pos + k + 1 = 64 = n_ctx
    assert len(e.verify([1] * 4)) >= 1      # 63 < n_ctx fits
    e.close()
    t = G.Engine(shape, n_ctx=n_ctx, device=0, tp=(2, 0, None))  # virtual ranks: a row-split engine
    t.begin(prompt[:8])
    t.step(8, use_graph=True)
    assert t.pos() == 8
    refused(t, [1, 2])
    t.close()
