"""GPU: the product form of the per-head decode attention at head_dim 256: k_attn_head_hd<256, false>, the
instantiation launch_attn_decode starts when no debug tap is set (csrc/ops.hip; the body is attn_head_dev,
csrc/attn_impl.h).  tests/test_gpu_attn_decode_rows.py always sets the taps and so covers its tapped sibling;
here the same entry (gemma_test_attn_decode_rows, form 0) runs with taps=False and is compared bit for bit
against orc_attn_decode_row: out, the K row and V column of pos, every other cache word unchanged, the Q8_0
image, and at dsplit 1 the Q8_K image.

The positions are the edges of the form: the row's own position on the first lane and the last lane of a wave's
16 positions and on the next wave (0, 15, 16, 31, 32: only the wave that holds pos reads this token's k from
LDS); the padded count n_kv = 32 (pos / 32 + 1) around 223 / 224; the pass of 256 positions and the V group of
256 positions around 254 .. 257, 511 .. 513 and 2047 / 2048 (a later pass's 8 K loads, a later group's 8 V
loads, the own-position patch in a later group, a row whose last group is whole and one whose last group is
not); and ctx - 2 / ctx - 1, where n_kv is capped at ctx (320 and 2304 are no multiples of 256)."""
import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_attn_decode_rows import CASES, Batch, _assert_none, _check, _run

gpu = pytest.mark.gpu
POS = [0, 15, 16, 31, 32, 223, 224, 254, 255, 256, 257, 511, 512, 513, 2047, 2048]
HD = 256


def _batch(name, H, Hkv, ctx):
    b = Batch(H, Hkv, HD, ctx, name != "normal")
    for pos in sorted({p for p in POS + [ctx - 2, ctx - 1] if p < ctx}):
        b.add_case(name, pos)
    return b.freeze()


@gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("H,Hkv", [(2, 1), (4, 2), (8, 1)], ids=["G2", "G2x2", "G8"])
@pytest.mark.parametrize("ctx", [320, 2304])
def test_product_form(ctx, H, Hkv, name):
    b = _batch(name, H, Hkv, ctx)
    fails = []
    for ds in (1, 2, 4, 8):
        o = _run(b, 0, ds, taps=False, img=True, q8k=ds == 1)
        fails += _check(b, o, f"untapped H {H} Hkv {Hkv} ctx {ctx} dsplit {ds}")
    _assert_none(fails)


@gpu
@pytest.mark.parametrize("ctx", [320, 2304])
def test_tapped_and_untapped_agree(ctx):
    """the two instantiations on the same inputs: equal out, caches and images, word for word"""
    fails = []
    for name in ("normal", "cancel_kqv", "stale"):
        b = _batch(name, 4, 2, ctx)
        for ds in (1, 4):
            t = _run(b, 0, ds, taps=True, img=True, q8k=ds == 1)
            u = _run(b, 0, ds, taps=False, img=True, q8k=ds == 1)
            assert t["r"] == 0 and u["r"] == 0, (t["why"], u["why"])
            for k in ("out", "kc", "vc", "act", "da", "q8k"):
                if t[k] is not None and not np.array_equal(t[k].view(np.uint8), u[k].view(np.uint8)):
                    fails.append(f"{name} ctx {ctx} dsplit {ds}: {k} differs between the tapped and the untapped kernel")
    _assert_none(fails)


@gpu
def test_engine_across_position_256():
    """the 2-layer engine of test_engine_two_layers_graph_tokens (GQA, head_dim 256) with a 250-token prompt
    through the batched prefill and 16 graph-replayed decode steps, positions 250 .. 265: the decode attention
    goes from one pass and one V group to two inside the replayed graph.  Tokens and every logit against the
    oracle model, bit for bit."""
    import gemma_hip as G
    shape = dict(n_layer=2, n_embd=2048, n_head=8, n_head_kv=2, head_dim=256, n_ff=2048, n_vocab=4096)
    n_prompt, n_decode, n_ctx = 250, 16, 320
    m = O.Model(O.make_config(shape, n_ctx=n_ctx))
    prompt = O.make_prompt(n_prompt, shape["n_vocab"])
    seq_ref, lg_ref = m.generate(prompt, n_decode)
    e = G.Engine(shape, n_ctx=n_ctx)
    try:
        e.begin(prompt)
        tok, last = e.prefill(n_prompt)
        lg = e.step(n_decode, want_logits=True, use_graph=True)
        toks = list(e.tokens()[: len(seq_ref)])
    finally:
        e.close()
    assert tok == seq_ref[n_prompt]
    assert toks == list(seq_ref)
    assert np.array_equal(last.view(np.uint32), lg_ref[0].view(np.uint32)), "the prompt's last row"
    bad = np.flatnonzero((lg.view(np.uint32) != lg_ref[1:1 + n_decode].view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"decode steps {bad.tolist()} (positions {[n_prompt + int(i) for i in bad]}) differ from the oracle"
