"""Speculative decoding in the batch (gemma_engine_batch_verify, gemma_engine_batch_generate_lookup):
per-slot drafts in one exact pass, the accept rule, the advance and the clean-up per slot on the
device.

The yardsticks are tests/test_gpu_batch.py's and tests/test_gpu_verify.py's: the oracle's
single-sequence run per slot (Seq, _truth, _bits_equal: uint32 views, no tolerance), drafts that are
the oracle's tokens with one entry replaced, and with the sampler on a plain Engine stepping with the
same sampler.  Row (s, i) of a pass processes position pos_s + i, so rows 0 .. a_s of a slot must be
rows pos_s .. pos_s + a_s of that sequence's logits bit for bit, whatever the other rows are and
whichever form the pass takes; the device state afterwards is compared with a twin whose slots took
a_s + 1 batch_step(1) passes.

The shapes are the smallest at which the per-slot bookkeeping can go wrong: slots that are not the
first ones with different k and a in one pass, a slot whose rows straddle a group edge, the padded-n_kv
bump at 31 / 32 and key 64 inside a slot's rows, rows that straddle position 256, an ingesting slot and
a slot that sits out beside verifying ones, G = 2 / 8 query heads per kv head, Q8_0, the Q6_K head and
K-quant layers."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_batch import SAMPLER, Seq, _adopt, _begin, _engine
from test_gpu_batch_rows import NEVER, _step
from test_gpu_prefill_continue import G8, K2B, KSHAPE, _bits_equal

pytestmark = pytest.mark.gpu

KD = G.VERIFY_MAX_DRAFT
FN = "gemma_engine_batch_verify"


def _draft(q, k, a):
    """the oracle's next k tokens of q, entry a replaced by another id (a == k: all right)"""
    d = [int(t) for t in q.full[q.pos + 1:q.pos + 1 + k]]
    assert len(d) == k, "the oracle run is too short for this case"
    if a < k:
        d[a] = (d[a] + 1) % q.rows.shape[1]
    return d


def _verify(e, slots, plan):
    """one batch_verify pass over the active slots {slot: Seq}; plan {slot: (k, a)}, a slot missing
    from it sits out.  The returned tokens, n_out (the lists' lengths), rows 0 .. a of every slot
    against the oracle's rows, then every active slot's position, tokens and pending token"""
    drafts = {s: _draft(slots[s], k, a) for s, (k, a) in plan.items()}
    toks, lg = e.batch_verify(drafts, want_logits=True)
    assert lg.shape[0] == sum(1 + k for k, _ in plan.values())
    assert sorted(toks) == sorted(plan), (sorted(toks), sorted(plan))
    t = 0
    for s in sorted(plan):
        q, (k, a) = slots[s], plan[s]
        want = [int(x) for x in q.full[q.pos + 1:q.pos + a + 2]]
        assert toks[s] == want, (s, k, a, toks[s], want)
        _bits_equal(lg[t:t + a + 1], q.expect(a + 1), f"slot {s}: rows {t} .. {t + a} from position {q.pos}, k = {k}")
        t += 1 + k
        q.pos += a + 1
    last = e.batch_last_n()
    for s, q in slots.items():  # the slots that sat out as well
        assert e.batch_pos(s) == q.pos, (s, e.batch_pos(s), q.pos)
        assert list(e.batch_tokens(s)) == list(q.full[:q.pos + 1]), s
        assert last[s] == q.full[q.pos]
    assert all(last[s] == -1 for s in range(len(last)) if s not in slots)
    return lg


def test_mixed_pass_in_slots_1_4_6():
    """slots 1, 4, 6 of 8 in one pass of 17 rows: k = 7 all accepted, k = 3 with a = 1, k = 4 with
    a = 0; then three batch_step passes continue exactly"""
    shape = dict(O.TINY)
    a, b, c = Seq(shape, 256, 20, seed=1, n_dec=12), Seq(shape, 256, 13, seed=2, n_dec=12), Seq(shape, 256, 9, seed=3, n_dec=12)
    e = _engine(shape)
    e.batch_open_rows(8, 24)
    slots = {1: a, 4: b, 6: c}
    for s, q in slots.items():
        _adopt(e, s, q)
    _verify(e, slots, {1: (7, 7), 4: (3, 1), 6: (4, 0)})
    assert (a.pos, b.pos, c.pos) == (28, 15, 10)
    _step(e, slots, 3)
    e.close()


@pytest.mark.parametrize("form", ["skinny", "groups", "mfma"])
def test_pass_forms(form):
    """T = 8 (two slots, k = 3 each) on the skinny GEMM; T = 15 as groups 8 + 7 (slot 1's rows 5 .. 11
    straddle the group edge) and as one MFMA pass.  Every accepted row equals the oracle's in each
    form, so the forms give the same bits; a second pass and a batch_step continue from each"""
    shape = dict(O.TINY)
    seqs = [Seq(shape, 256, n, seed=s, n_dec=16) for n, s in ((20, 1), (13, 2), (9, 3))]
    e = _engine(shape)
    e.batch_open_rows(3, 16)
    if form == "skinny":
        slots, plan = {0: seqs[0], 1: seqs[1]}, {0: (3, 3), 1: (3, 1)}
    else:
        e.set_option("bt_mfma_min", NEVER if form == "groups" else 9)
        slots, plan = dict(enumerate(seqs)), {0: (4, 4), 1: (6, 3), 2: (2, 2)}
    for s, q in slots.items():
        _adopt(e, s, q)
    _verify(e, slots, plan)
    _verify(e, slots, {s: (k, max(a - 1, 0)) for s, (k, a) in plan.items()})
    _step(e, slots, 1)
    e.close()


def test_groups_and_mfma_give_the_same_rows_rejected_ones_included():
    """the T = 15 pass as groups and as one MFMA pass: all 15 rows bit-equal, also the rows computed
    under rejected drafts, which no oracle row covers"""
    shape = dict(O.TINY)
    seqs = [Seq(shape, 256, n, seed=s, n_dec=16) for n, s in ((20, 1), (13, 2), (9, 3))]
    rows = []
    for mfma_min in (NEVER, 9):
        e = _engine(shape)
        e.batch_open_rows(3, 16)
        e.set_option("bt_mfma_min", mfma_min)
        for s, q in enumerate(seqs):
            _adopt(e, s, q)
        rows.append(_verify(e, dict(enumerate(seqs)), {0: (4, 1), 1: (6, 3), 2: (2, 0)}))
        e.close()
    _bits_equal(rows[0], rows[1], "groups against one MFMA pass")


def test_prefix_rule_stops_at_the_first_mismatch():
    """a later draft that equals its row's pick does not count once an earlier one is wrong"""
    shape, n = dict(O.TINY), 20
    q = Seq(shape, 256, n, seed=1, n_dec=12)
    e = _engine(shape)
    e.batch_open(2)
    _adopt(e, 1, q)
    first = int(q.full[n + 1])
    wrong = (first + 1) % shape["n_vocab"]
    toks, rows = e.batch_verify({1: [wrong, 5, 6, 7]}, want_logits=True)
    assert toks == {1: [first]}
    g1 = int(rows[1].argmax())  # row 1's greedy pick under the wrong draft (first max, as np.argmax)
    e.batch_adopt(1)  # the engine's own sequence still stands at n: the slot again, from it
    assert e.batch_pos(1) == n and list(e.batch_tokens(1)) == list(q.full[:n + 1])
    toks2, rows2 = e.batch_verify({1: [wrong, g1, 6, 7]}, want_logits=True)
    assert int(rows2[1].argmax()) == g1  # the later draft does equal its row's pick
    assert toks2 == {1: [first]} and e.batch_pos(1) == n + 1
    q.pos = n + 1
    _step(e, {1: q}, 3)
    e.close()


@pytest.mark.parametrize("n_ctx,n_prompt,a", [(256, 30, 4), (256, 30, 2), (256, 62, 4), (256, 62, 1), (512, 254, 4), (512, 254, 2)],
                         ids=["pos30_all", "pos30_partial", "across_key_64_all", "across_key_64_partial",
                              "across_256_all", "across_256_partial"])
def test_positions(n_ctx, n_prompt, a):
    """pos = 30: the padded n_kv changes inside the slot's rows (30, 31 | 32 ..); pos = 62: they cross
    key 64; n_ctx 512 at 254: they straddle position 256"""
    shape = dict(O.TINY)
    q = Seq(shape, n_ctx, n_prompt, seed=2, n_dec=8)
    e = _engine(shape, n_ctx=n_ctx)
    e.batch_open(3)
    _adopt(e, 2, q)
    _verify(e, {2: q}, {2: (4, a)})
    _step(e, {2: q}, 2)
    e.close()


def test_ingesting_slot_beside_verifying_slots():
    """slot 2 consumes its 5 given tokens with k = 0 while slot 0 verifies drafts: its given tokens are
    not overwritten (batch_tokens is the prompt's prefix); once consumed it takes drafts too"""
    shape = dict(O.TINY)
    a, b = Seq(shape, 256, 20, seed=1, n_dec=24), Seq(shape, 256, 5, seed=3, n_dec=10)
    e = _engine(shape)
    e.batch_open(3)
    _adopt(e, 0, a)
    _begin(e, 2, b)
    slots = {0: a, 2: b}
    for k, acc in ((3, 3), (3, 1), (3, 0), (2, 2), (1, 1)):
        _verify(e, slots, {0: (k, acc), 2: (0, 0)})
        assert list(e.batch_tokens(2))[:len(b.prompt)] == list(b.prompt[:b.pos + 1])
    assert b.pos == 5
    _verify(e, slots, {0: (3, 2), 2: (2, 2)})
    _verify(e, slots, {0: (2, 2), 2: (2, 0)})
    _step(e, slots, 1)
    e.close()


def _state(e, s, n_layer, n_ctx):
    return (e.batch_pos(s), list(e.batch_tokens(s)), int(e.batch_last_n()[s]), e.batch_logprobs(s).view(np.uint64).copy(),
            [e.batch_kv_read(s, il, 0, n_ctx) for il in range(n_layer)])


def _same_state(x, y, what):
    assert x[:3] == y[:3], (what, x[:3], y[:3])
    assert np.array_equal(x[3], y[3]), (what, "log-probabilities")
    for il, ((k0, v0), (k1, v1)) in enumerate(zip(x[4], y[4])):
        assert np.array_equal(k0, k1) and np.array_equal(v0, v1), (what, "layer", il)


def test_sitting_out_changes_nothing():
    """slot 1 sits out (k = -1) of two passes: its position, tokens, pending token, whole caches and
    log-probabilities are what they were; then it continues exactly beside the others"""
    shape, n_ctx = dict(O.TINY), 256
    seqs = {0: Seq(shape, n_ctx, 20, seed=1, n_dec=16), 1: Seq(shape, n_ctx, 13, seed=2, n_dec=16), 2: Seq(shape, n_ctx, 9, seed=3, n_dec=16)}
    e = _engine(shape)
    e.set_logprobs(1)
    e.batch_open_rows(3, 16)
    for s, q in seqs.items():
        _adopt(e, s, q)
    _step(e, seqs, 1)
    before = _state(e, 1, shape["n_layer"], n_ctx)
    _verify(e, seqs, {0: (4, 2), 2: (3, 3)})
    _verify(e, seqs, {0: (0, 0), 2: (7, 0)})
    _same_state(before, _state(e, 1, shape["n_layer"], n_ctx), "the slot that sat out")
    _verify(e, seqs, {0: (2, 2), 1: (4, 1), 2: (1, 1)})
    _step(e, seqs, 2)
    e.close()


def test_state_equals_one_row_passes():
    """after a pass with a = 3 of 7, 0 of 4 and 5 of 5, each slot's state equals a twin slot's that took
    a + 1 batch_step(1) passes: every layer's whole cache over [0, n_ctx) (so the rejected rows are
    zero), tokens, position, pending token, and batch_logprobs bit for bit (uint64 views: NaN stays
    where nothing was scored)"""
    shape, n_ctx = dict(O.TINY), 256
    L = shape["n_layer"]
    seqs = {0: Seq(shape, n_ctx, 20, seed=1, n_dec=16), 1: Seq(shape, n_ctx, 13, seed=2, n_dec=16), 2: Seq(shape, n_ctx, 9, seed=3, n_dec=16)}
    plan = {0: (7, 3), 1: (4, 0), 2: (5, 5)}
    e = _engine(shape)
    e.set_logprobs(1)
    e.batch_open_rows(3, 24)
    for s, q in seqs.items():
        _adopt(e, s, q)
    _verify(e, seqs, plan)
    got = {s: _state(e, s, L, n_ctx) for s in seqs}
    p = _engine(shape)
    p.set_logprobs(1)
    p.batch_open(3)
    for s, q in seqs.items():  # one twin slot at a time: batch_step advances every active slot
        p.begin(q.prompt)
        p.prefill(len(q.prompt))
        p.batch_adopt(s)
        p.batch_step(plan[s][1] + 1)
        want = _state(p, s, L, n_ctx)
        _same_state(got[s], want, f"slot {s}")
        pos = want[0]
        assert pos == len(q.prompt) + plan[s][1] + 1
        lp = want[3].view(np.float64)
        assert np.isnan(lp[0]) and np.isfinite(lp[1:]).all()
        for k, v in got[s][4]:
            assert k[:pos].any() and not k[pos:].any() and not v[pos:].any(), s
        p.batch_release(s)
    p.close()
    # and the next pass continues from that state, log-probabilities included
    _verify(e, seqs, {0: (2, 2), 1: (3, 3), 2: (0, 0)})
    for s in seqs:
        lp = e.batch_logprobs(s)
        assert len(lp) == seqs[s].pos + 1 and np.isnan(lp[0]) and np.isfinite(lp[1:]).all() and (lp[1:] <= 0).all(), s
    e.close()


def test_sampler_on_chained_passes_equal_plain_steps():
    """varied sequences: three slots, chained passes with k cycling 1 .. 7 and every third draft
    corrupted; every returned token against a plain Engine stepping with the same sampler"""
    shape, n_new = dict(O.TINY), 24
    V = shape["n_vocab"]
    prompts = [[int(t) for t in O.make_prompt(n, V, seed=21 + n)] for n in (20, 13, 9)]
    p = _engine(shape)
    p.set_sampler(**SAMPLER)
    e = _engine(shape)
    e.set_sampler(**SAMPLER)
    e.batch_open_rows(3, 24)
    refs = []
    for s, pr in enumerate(prompts):
        p.begin(pr)
        p.prefill(len(pr))
        p.step(n_new + KD + 1, use_graph=False)
        refs.append([int(t) for t in p.tokens()])
        assert len(set(refs[s][len(pr):len(pr) + n_new])) > 1, "the sampled run is constant: the test would prove nothing"
        e.begin(pr)
        e.prefill(len(pr))
        e.batch_adopt(s)
        assert list(e.batch_tokens(s)) == refs[s][:len(pr) + 1]
    p.close()
    i = 0
    while any(e.batch_pos(s) - len(prompts[s]) < n_new for s in range(3)):
        drafts, want = {}, {}
        for s in range(3):
            pos, k = e.batch_pos(s), 1 + (i + 2 * s) % KD
            if pos - len(prompts[s]) >= n_new:
                continue  # a slot that has its tokens sits out
            d = refs[s][pos + 1:pos + 1 + k]
            a = k
            if (i + s) % 3 == 2:
                a = i % k
                d[a] = (d[a] + 1) % V
            drafts[s], want[s] = d, refs[s][pos + 1:pos + a + 2]
        assert e.batch_verify(drafts) == want, (i, drafts)
        i += 1
    for s in range(3):
        assert list(e.batch_tokens(s)) == refs[s][:e.batch_pos(s) + 1]
    e.close()


@pytest.mark.parametrize("shape,n_ctx,okw,ekw", [
    (G8, 256, {}, {}),
    (K2B, 256, {}, {}),
    (dict(O.TINY, n_head=4, n_head_kv=2), 256, dict(wtype=O.Q8_0), dict(wtype=G.GGML_TYPE_Q8_0)),
    (dict(O.TINY), 256, dict(kmix=2), dict(out_type=G.GGML_TYPE_Q6_K)),
    (KSHAPE, 128, dict(kmix=1), dict(wtype=G.GGML_TYPE_Q4_K)),
], ids=["G8", "K2B", "Q8_0_gqa", "Q6K_head", "kquant_layers"])
def test_shapes(shape, n_ctx, okw, ekw):
    """2 slots with 2 and 3 given tokens, consumed by three one-row passes; then one pass of 8 rows with
    a = 1 of 3 and 3 of 3, and a batch_step"""
    slots = {0: Seq(shape, n_ctx, 2, seed=1, n_dec=6, **okw), 1: Seq(shape, n_ctx, 3, seed=2, n_dec=6, **okw)}
    e = _engine(shape, n_ctx=n_ctx, **ekw)
    e.batch_open(2)
    for s, q in slots.items():
        _begin(e, s, q)
    _step(e, slots, 3)
    _verify(e, slots, {0: (3, 1), 1: (3, 3)})
    _step(e, slots, 1)
    e.close()


def test_refusals_leave_the_state_untouched():
    shape, n_ctx = dict(O.TINY), 64
    V = shape["n_vocab"]
    a, b = Seq(shape, n_ctx, 40, seed=2, n_dec=23), Seq(shape, n_ctx, 5, seed=3, n_dec=8)
    e = _engine(shape, n_ctx=n_ctx)
    L, h = e.L, e.h
    ns = 3
    draft = np.ones((ns, KD), dtype=np.int32)
    out, n_out = np.full((ns, KD + 1), -7, dtype=np.int32), np.full(ns, -7, dtype=np.int32)

    def refused(k_of, d=draft, null=None):
        k = np.ascontiguousarray(k_of, dtype=np.int32)
        args = [G._p(d), G._p(k), G._p(out), G._p(n_out), None]
        if null is not None:
            args[null] = None
        r = L.gemma_engine_batch_verify(h, *args)
        assert r == -1 and FN in G.last_error() and len(G.last_error()) > 40, (k_of, r, G.last_error())
        assert (out == -7).all() and (n_out == -7).all()

    refused([0, 0, 0])  # no batch open
    e.batch_open(ns)    # a row capacity of 8
    refused([0, 0, 0])  # no active slot
    _adopt(e, 0, a)
    _begin(e, 2, b)
    slots = {0: a, 2: b}
    _verify(e, slots, {0: (2, 2), 2: (0, 0)})

    def state():
        return [e.batch_pos(s) for s in (0, 2)], [list(e.batch_tokens(s)) for s in (0, 2)], list(e.batch_last_n())

    before = state()
    for i in range(4):
        refused([1, 0, 0], null=i)           # a null draft, k_of, out_tokens, n_out
    refused([-2, 0, 0])                      # k_of outside [-1, 7]
    refused([8, 0, 0])
    refused([0, 0, 9])
    refused([-1, 5, -1])                     # no slot takes part (slot 1 is inactive: its k_of is not read)
    refused([1, 0, 1])                       # slot 2 has given tokens pending (pos 1 of 5)
    bad = draft.copy()
    bad[0, 1] = V
    refused([2, 0, 0], d=bad)                # a used draft id outside [0, n_vocab)
    bad[0, 1] = -1
    refused([2, 0, 0], d=bad)
    refused([7, 0, 1])                       # T = 10 above the row capacity 8 (and slot 2 ingesting)
    refused([7, 0, 0])                       # T = 9
    assert state() == before
    # at k = 1 the out-of-range id at draft[0][1] is not used: the pass runs
    out2, n2 = np.zeros((ns, KD + 1), dtype=np.int32), np.zeros(ns, dtype=np.int32)
    k = np.ascontiguousarray([1, -1, 0], dtype=np.int32)
    assert L.gemma_engine_batch_verify(h, G._p(bad), G._p(k), G._p(out2), G._p(n2), None) == 3, G.last_error()
    assert n2[0] in (1, 2) and list(n2[1:]) == [0, 1]
    assert list(out2[0, :n2[0]]) == list(a.full[a.pos + 1:a.pos + 1 + n2[0]]) and out2[2, 0] == b.full[b.pos + 1]
    a.pos += int(n2[0])
    b.pos += 1
    _step(e, slots, 3)  # slot 2 consumes its given tokens
    assert b.pos == 5
    _verify(e, slots, {0: (4, 4), 2: (1, 1)})
    # context full: pos + k + 1 >= n_ctx
    while a.pos < 58:
        _verify(e, slots, {0: (min(4, 58 - a.pos - 1), min(4, 58 - a.pos - 1))})
    assert a.pos == 58
    before = state()
    refused([5, 0, -1])                      # 58 + 5 + 1 = 64 = n_ctx
    assert "context full" in G.last_error()
    assert state() == before
    _verify(e, slots, {0: (4, 1), 2: (0, 0)})  # 63 < n_ctx fits, and a valid pass after them is exact
    e.close()
    # a slot at position 0 takes no drafts
    e = _engine(shape, n_ctx=n_ctx)
    e.batch_open(1)
    e.batch_begin(0, [3])
    h = e.h
    L = e.L
    ns = 1
    draft = np.ones((ns, KD), dtype=np.int32)
    out, n_out = np.full((ns, KD + 1), -7, dtype=np.int32), np.full(ns, -7, dtype=np.int32)
    k = np.ones(1, dtype=np.int32)
    assert L.gemma_engine_batch_verify(h, G._p(draft), G._p(k), G._p(out), G._p(n_out), None) == -1 and FN in G.last_error()
    assert e.batch_pos(0) == 0 and (n_out == -7).all()
    e.close()


def test_memory_returns_to_the_baseline():
    shape = dict(O.TINY)
    q = Seq(shape, 256, 3, seed=2, n_dec=12)
    base = G.mem_live()
    e = _engine(shape)
    before = G.mem_live()
    e.batch_open_rows(8, 16)
    opened = G.mem_live()
    assert opened[0] > before[0] and opened[1] > before[1]
    _begin(e, 5, q)
    _step(e, {5: q}, 3)
    _verify(e, {5: q}, {5: (7, 3)})
    e.batch_generate_lookup(4, k=3)
    assert G.mem_live() == opened  # a pass allocates nothing
    e.batch_close()
    assert G.mem_live() == before
    e.batch_open(3)
    _begin(e, 2, q)
    _step(e, {2: q}, 3)
    _verify(e, {2: q}, {2: (4, 4)})
    e.close()  # with the batch still open
    assert G.mem_live() == base


# ---- the generate loop ------------------------------------------------------------------------------
def _lookup_prompts(V):
    """a 6-token block repeated 4 times, cut to different lengths"""
    blocks = [[int(t) for t in O.make_prompt(6, V, seed=s)] for s in (1, 2, 3)]
    return [(blocks[0] * 4)[:24], (blocks[1] * 4)[:21], (blocks[2] * 4)[:19]]


def _adopt_prompts(e, prompts):
    for s, pr in enumerate(prompts):
        e.begin(pr)
        e.prefill(len(pr))
        e.batch_adopt(s)


def _twin_tokens(shape, prompts, n_new, sampler, n_ctx=256):
    """the slots' sequences by batch_step(n_new) passes"""
    p = _engine(shape, n_ctx=n_ctx)
    if sampler:
        p.set_sampler(**SAMPLER)
    p.batch_open_wide(len(prompts))
    _adopt_prompts(p, prompts)
    p.batch_step(n_new)
    refs = [[int(t) for t in p.batch_tokens(s)] for s in range(len(prompts))]
    pos = [p.batch_pos(s) for s in range(len(prompts))]
    p.close()
    return refs, pos


@pytest.mark.parametrize("sampler", [False, True], ids=["greedy", "sampled"])
def test_generate_lookup_equals_batch_step(sampler):
    shape, n_new = dict(O.TINY), 40
    prompts = _lookup_prompts(shape["n_vocab"])
    refs, pos = _twin_tokens(shape, prompts, n_new, sampler)
    e = _engine(shape)
    if sampler:
        e.set_sampler(**SAMPLER)
    e.batch_open_rows(3, 16)
    _adopt_prompts(e, prompts)
    out, st = e.batch_generate_lookup(n_new, k=4, ngram_max=3)
    for s, pr in enumerate(prompts):
        assert [int(t) for t in out[s]] == refs[s][len(pr) + 1:len(pr) + 1 + n_new], s
        assert e.batch_pos(s) == pos[s] == len(pr) + n_new
        assert [int(t) for t in e.batch_tokens(s)] == refs[s]
        assert st[s]["passes"] + st[s]["accepted"] + st[s]["plain_steps"] == n_new, st[s]
    if not sampler:
        assert all(x["passes"] >= 1 and x["accepted"] >= 1 for x in st), st  # passes ran and drafts were accepted
    e.close()


def _simulate(ref, n0, n_new, k, ngram_max, n_ctx):
    """the loop over one slot's known sequence `ref`, n0 tokens of it there at the start: the draft
    grown by repeated lookups over its own guesses, capped and dropped as the header states"""
    seq, done = list(ref[:n0]), 0
    st = dict(passes=0, drafted=0, accepted=0, plain_steps=0)
    while done < n_new:
        kd_max, guess, draft = min(k, n_new - done - 1), list(seq), []
        while len(draft) < kd_max:
            m = G.lookup_draft(guess, ngram_max, kd_max - len(draft))
            if not m:
                break
            draft += m
            guess += m
        n = len(seq)
        if draft and (n - 1) + len(draft) + 1 >= n_ctx:
            draft = []
        a = 0
        while a < len(draft) and draft[a] == ref[n + a]:
            a += 1
        if draft:
            st["passes"] += 1
            st["drafted"] += len(draft)
            st["accepted"] += a
        else:
            st["plain_steps"] += 1
        seq += ref[n:n + a + 1]
        done += a + 1
    return st


def test_generate_lookup_stats_equal_the_simulated_loop():
    """3 slots, k = 4, 16 rows: the allotment does not bind (at most 15 rows), so every slot's loop is
    the single loop over its own sequence"""
    shape, n_new = dict(O.TINY), 40
    prompts = _lookup_prompts(shape["n_vocab"])
    refs, _ = _twin_tokens(shape, prompts, n_new, False)
    e = _engine(shape)
    e.batch_open_rows(3, 16)
    _adopt_prompts(e, prompts)
    out, st = e.batch_generate_lookup(n_new, k=4, ngram_max=3)
    e.close()
    for s, pr in enumerate(prompts):
        want = _simulate(refs[s], len(pr) + 1, n_new, 4, 3, 256)
        assert st[s] == want, (s, st[s], want)
        assert want["passes"] >= 1 and want["accepted"] >= 1, want


def test_generate_lookup_when_the_capacity_binds():
    """open(8), 8 slots, k = 4: 8 rows for 8 slots, the drafts are cut by the allotment (to nothing while
    all 8 are unfinished); the tokens are batch_step's"""
    shape, n_new = dict(O.TINY), 12
    V = shape["n_vocab"]
    prompts = [([int(t) for t in O.make_prompt(6, V, seed=1 + s)] * 3)[:18 - s] for s in range(8)]
    refs, pos = _twin_tokens(shape, prompts, n_new, False)
    e = _engine(shape)
    e.batch_open(8)
    _adopt_prompts(e, prompts)
    out, st = e.batch_generate_lookup(n_new, k=4, ngram_max=3)
    for s, pr in enumerate(prompts):
        assert [int(t) for t in out[s]] == refs[s][len(pr) + 1:len(pr) + 1 + n_new], s
        assert e.batch_pos(s) == pos[s]
        assert st[s]["passes"] + st[s]["accepted"] + st[s]["plain_steps"] == n_new, st[s]
    e.close()
