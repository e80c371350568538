"""GPU: the context shift on engines (gemma_engine_shift, gemma_engine_batch_shift; DESIGN.md §5b′ "Context shift").

Small synthetic models.  Caches after a shift are held to the numpy rule (tests/test_gpu_kv_shift.py) applied to the
caches read before it; the steps behind it run eager and through the graph captured before the shift; a slot is held
to a single engine given the same calls.  The direction of the rotation is held to something that never saw a shift:
in a one-layer model layer-0 K depends on the token and its position only, so after shift(0, d) K row j is, up to the
f16 roundings, K row j of a fresh engine prefilled with tokens[d:].  Bound per NEOX pair: 4 * 2^-11 * hypot(x0, x1),
three f16 roundings plus one unit for the f32 angle (< 1e-4 rad at positions <= 256); the CPU check with the oracle's
rope rows at these positions reached 2.0 of those 4 units."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_kv_shift import shift_rule

pytestmark = pytest.mark.gpu
SHAPE, V = dict(O.TINY), O.TINY["n_vocab"]


def _caches(read, n_layer, n_ctx):  # every layer's images as the rule takes them: K [ctx][kvw], V [kvw][ctx]
    return [(k, np.ascontiguousarray(v.T)) for k, v in (read(il, 0, n_ctx) for il in range(n_layer))]


def _assert_rule(before, after, pos, keep, d):
    for il, ((k0, v0), (k1, v1)) in enumerate(zip(before, after)):
        k_ref, v_ref = shift_rule(k0, v0, pos, keep, d, SHAPE["n_head_kv"], SHAPE["head_dim"])
        assert np.array_equal(k1, k_ref) and np.array_equal(v1, v_ref), f"layer {il}"


@pytest.mark.parametrize("n_ctx,n_prompt,keep,d", [(256, 100, 8, 33), (4096, 2300, 32, 512)])
def test_shift_follows_the_rule_and_the_graph_survives_it(n_ctx, n_prompt, keep, d):
    # two engines, the same calls; the steps after the shift eager on one, by the graph captured before it on the other
    rows, toks = [], []
    for use_graph in (False, True):
        e = G.Engine(SHAPE, n_ctx=n_ctx, device=0)
        e.begin(O.make_prompt(n_prompt, V)), e.prefill(n_prompt)
        e.step(5, use_graph=use_graph)
        pos, seq = e.pos(), e.tokens().tolist()
        n_kern = e.graph_kernels() if use_graph else None
        before = _caches(e.kv_read, SHAPE["n_layer"], n_ctx)
        assert e.shift(keep, d) == pos - d == e.pos()
        assert e.tokens().tolist() == seq[:keep] + seq[keep + d:], "the history, the pending token included"
        _assert_rule(before, _caches(e.kv_read, SHAPE["n_layer"], n_ctx), pos, keep, d)
        rows.append(e.step(8, want_logits=True, use_graph=use_graph)), toks.append(e.tokens().tolist())
        assert n_kern is None or e.graph_kernels() == n_kern
        e.close()
    assert toks[0] == toks[1] and len(toks[0]) == n_prompt + 5 - d + 8 + 1
    assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))


def test_a_shifted_slot_equals_a_single_engine_and_leaves_its_neighbour_alone():
    n_ctx, keep, d = 256, 4, 17
    prompts = [O.make_prompt(60, V, seed=3), O.make_prompt(45, V, seed=4)]

    def batch(shift):
        e = G.Engine(SHAPE, n_ctx=n_ctx, device=0)
        e.batch_open(2)
        for s, p in enumerate(prompts):
            e.batch_begin(s, p)
        e.batch_step(64)
        if shift:
            assert e.batch_shift(0, keep, d) == 64 - d == e.batch_pos(0)
        lg = e.batch_step(6, want_logits=True)
        out = [(e.batch_tokens(s).tolist(), _caches(lambda il, p0, n: e.batch_kv_read(s, il, p0, n), SHAPE["n_layer"], n_ctx))
               for s in range(2)]
        assert e.batch_last()[:2].tolist() == [out[0][0][-1], out[1][0][-1]]
        e.batch_close(), e.close()
        return lg, out

    (lg1, with_shift), (lg0, without) = batch(True), batch(False)
    assert with_shift[1][0] == without[1][0] and np.array_equal(lg1[:, 1].view(np.uint32), lg0[:, 1].view(np.uint32))
    for (ka, va), (kb, vb) in zip(with_shift[1][1], without[1][1]):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), "the untouched slot"
    e = G.Engine(SHAPE, n_ctx=n_ctx, device=0)  # the single sequence: the same calls
    e.begin(prompts[0]), e.step(64), e.shift(keep, d)
    lg = e.step(6, want_logits=True)
    assert e.tokens().tolist() == with_shift[0][0]
    assert np.array_equal(lg.view(np.uint32), lg1[:, 0].view(np.uint32))
    for (ka, va), (kb, vb) in zip(_caches(e.kv_read, SHAPE["n_layer"], n_ctx), with_shift[0][1]):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), "the shifted slot"
    e.close()


def test_direction_k_rows_are_those_of_a_fresh_engine_on_the_kept_tokens():
    shape, n, d, n_ctx, half = dict(SHAPE, n_layer=1), 200, 57, 256, SHAPE["head_dim"] // 2
    e = G.Engine(shape, n_ctx=n_ctx, device=0)
    e.begin(O.make_prompt(n, V)), e.prefill(n), e.shift(0, d)
    seq = e.tokens().tolist()
    (k_s, v_s), _ = e.kv_read(0, 0, n - d), e.close()
    f = G.Engine(shape, n_ctx=n_ctx, device=0)
    f.begin(seq[:n - d]), f.prefill(n - d)
    (k_f, v_f), _ = f.kv_read(0, 0, n - d), f.close()
    a = k_s.view(np.float16).astype(np.float64).reshape(n - d, -1, 2, half)
    b = k_f.view(np.float16).astype(np.float64).reshape(n - d, -1, 2, half)
    units = np.abs(a - b).max(axis=2) / (np.hypot(b[:, :, 0], b[:, :, 1]) * 2.0 ** -11 + 1e-30)
    print(f"direction check: worst pair {units.max():.3f} of 4 units of 2^-11 hypot(x0, x1)")
    assert np.array_equal(v_s, v_f) and units.max() <= 4.0, units.max()


def test_refusals_leave_the_state_untouched():
    e, n_ctx = G.Engine(SHAPE, n_ctx=256, device=0), 256
    e.begin(O.make_prompt(40, V))
    e.prefill_next(30)  # 10 given tokens are still pending
    state = lambda: (e.pos(), e.tokens().tolist(), [x.tobytes() for x in e.kv_read(1, 0, n_ctx)])
    s0 = state()
    with pytest.raises(RuntimeError, match="not processed"):
        e.shift(0, 8)
    assert state() == s0
    e.prefill_next(0)
    s1 = state()
    for keep, d in ((-1, 4), (0, 0), (30, 11), (41, 1)):
        with pytest.raises(RuntimeError, match="keep"):
            e.shift(keep, d)
    assert state() == s1
    e.set_logprobs(True), e.step(4)  # the records are dropped from `keep` on, and steps after the shift score again
    assert e.shift(10, 20) == 24
    assert np.isnan(e.logprobs(0, 25)[10:]).all()
    e.step(3)
    assert np.isfinite(e.logprobs(25, 3)).all()
    e.close()
