"""A sampler per slot (gemma_engine_batch_set_sampler, gemma_engine_batch_sampler) and forking a slot
(gemma_engine_batch_fork): greedy and sampling slots, each with its own parameters, in one pass.

Two yardsticks.  A plain Engine on the same sequence with set_sampler of the sampler in force on the
slot, changed at the same sequence index where the slot's changes: logits rows bit for bit
(_bits_equal: uint32 views, no tolerance), tokens equal.  And, for the cases marked CPU, the oracle:
its logits rows through the numpy restatement of the rule (tests/sampler_ref.py) or its greedy token,
fed back with Model.inference(seq, 1); no draw of these inputs is ambiguous.

The shapes are the smallest at which a row -> parameters mapping can go wrong: O.TINY at n_ctx 256,
slots that differ in mode and seed, equal prompts under different seeds, a slot that follows the
engine beside slots that do not, a setting that changes between passes, every pass type (step,
step_rows, verify, generate_lookup) and every pass form (skinny, groups of 8, MFMA)."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
import sampler_ref as R
from test_gpu_batch import _engine
from test_gpu_batch_rows import NEVER
from test_gpu_prefill_continue import _bits_equal

pytestmark = pytest.mark.gpu

SHAPE = dict(O.TINY)
V = SHAPE["n_vocab"]
N_CTX = 256
E = (1.0, 40, 0.95, 20240607)
GREEDY = (0.0, 0, 1.0, 0)


def A(seed):
    return (0.7, 8, 1.0, seed)


def P(s):
    return tuple(int(t) for t in O.make_prompt(3 + s, V, seed=11 + s))


def _kw(sp):
    return dict(temperature=sp[0], top_k=sp[1], top_p=sp[2], seed=sp[3])


def _in_force(plan, p):
    """plan: ((first sequence index, sampler or None = greedy), ...) ascending; the sampler at index p"""
    sp = None
    for start, s in plan:
        if start <= p:
            sp = s
    return sp


def _const(sp):
    return ((0, sp),)


@functools.lru_cache(maxsize=None)
def _cpu(prompt, n_seq, plan):
    """the oracle's sequence of n_seq tokens from `prompt`, every pick by the plan's sampler"""
    m = O.Model(O.make_config(SHAPE, n_ctx=N_CTX))
    seq = list(prompt)
    tok, last, _ = m.inference(seq, 0)
    while len(seq) < n_seq:
        sp = _in_force(plan, len(seq))
        if sp is not None and sp[0] > 0:
            tok, _, ambiguous, _ = R.sample(last, sp[0], sp[1], sp[2], sp[3], len(seq))
            assert not ambiguous, len(seq)
        seq.append(int(tok))
        tok, last, _ = m.inference(seq, 1)
    m.close()
    return tuple(seq)


class Plain:
    """a plain Engine stepping one sequence token by token, set_sampler following the plan"""

    def __init__(self, prompt, plan, logprobs=False):
        self.e, self.plan, self.cur = _engine(SHAPE, n_ctx=N_CTX), plan, None
        if logprobs:
            self.e.set_logprobs(1)
        self.e.begin(prompt)
        self.rows = []

    def to(self, pos):
        """step until `pos` positions are processed; returns the rows of the steps taken"""
        first = len(self.rows)
        while self.e.pos() < pos:
            sp = _in_force(self.plan, self.e.pos() + 1) or GREEDY
            if sp != self.cur:
                self.e.set_sampler(**_kw(sp))
                self.cur = sp
            self.rows.append(self.e.step(1, want_logits=True, use_graph=False)[0])
        return np.stack(self.rows[first:]) if len(self.rows) > first else np.zeros((0, V), np.float32)

    def tokens(self):
        return [int(t) for t in self.e.tokens()]

    def close(self):
        self.e.close()


@functools.lru_cache(maxsize=None)
def _plain(prompt, pos, plan):
    """(rows 0 .. pos - 1, tokens 0 .. pos) of the plain engine's run, computed once per case"""
    p = Plain(prompt, plan)
    rows = p.to(pos)
    toks = p.tokens()
    p.close()
    rows.setflags(write=False)
    return rows, toks


def _set(e, slot, sp):
    if sp is None:
        e.batch_set_sampler(slot, temperature=0.0)
    elif sp == "engine":
        e.batch_set_sampler(slot)
    else:
        e.batch_set_sampler(slot, **_kw(sp))


def _slot_equals_plain(e, s, prompt, plan, rows, pos0=0, what=""):
    """the slot's rows of the passes since pos0, its position and tokens against the plain engine"""
    pos = e.batch_pos(s)
    ref_rows, ref_toks = _plain(prompt, pos, plan)
    if rows is not None:
        _bits_equal(rows, ref_rows[pos0:pos], f"{what}slot {s} from position {pos0}")
    assert [int(t) for t in e.batch_tokens(s)] == ref_toks[:pos + 1], (what, s)
    return ref_toks


def test_mixed_narrow_pass():
    """(CPU) the engine's sampler E; slot 0 its own greedy, 1 its own A(5), 2 following the engine, 3
    slot 1's prompt under A(6): one pass serves all four, ten times"""
    n = 10
    prompts = [P(0), P(1), P(2), P(1)]
    plans = [_const(None), _const(A(5)), _const(E), _const(A(6))]
    e = _engine(SHAPE)
    e.set_sampler(**_kw(E))
    e.batch_open(4)
    _set(e, 0, None)
    _set(e, 1, A(5))
    _set(e, 3, A(6))
    for s, pr in enumerate(prompts):
        e.batch_begin(s, pr)
    lg = e.batch_step(n, want_logits=True)
    toks = []
    for s, pr in enumerate(prompts):
        toks.append(_slot_equals_plain(e, s, pr, plans[s], lg[:, s]))
        assert tuple(toks[s][:n + 1]) == _cpu(pr, n + 1, plans[s]), s
    assert toks[1][4:7] == [1357, 1357, 3223] and toks[3][4:7] == [4086, 513, 513], (toks[1], toks[3])
    assert toks[1] != toks[3]
    e.close()


def test_engine_greedy_and_a_slot_samples():
    """the engine's sampler was never set: the workspace the slot needs is the batch's own"""
    e = _engine(SHAPE)
    e.batch_open(2)
    _set(e, 1, A(5))
    assert e.batch_sampler(0) == (False, _kw(GREEDY), False)
    on, prm, own = e.batch_sampler(1)
    assert (on, own) == (True, True) and (prm["top_k"], prm["top_p"], prm["seed"]) == (8, 1.0, 5)
    e.batch_begin(0, P(0))
    e.batch_begin(1, P(1))
    lg = e.batch_step(8, want_logits=True)
    _slot_equals_plain(e, 0, P(0), _const(None), lg[:, 0])
    t = _slot_equals_plain(e, 1, P(1), _const(A(5)), lg[:, 1])
    assert len(set(t[4:])) > 1, t
    e.close()


def test_wide_groups_and_mfma():
    """(CPU) 12 slots, every third greedy, the others (1.0, 40, 0.95) under a seed each: as groups of
    8 and as one MFMA pass, the same bits; twelve distinct sequences"""
    n, ns = 8, 12
    prompts = [tuple(int(t) for t in O.make_prompt(3 + s % 5, V, seed=21 + s)) for s in range(ns)]
    plans = [_const(None if s % 3 == 0 else (1.0, 40, 0.95, 100 + s)) for s in range(ns)]
    out = []
    for mfma_min in (NEVER, 9):
        e = _engine(SHAPE)
        e.batch_open_wide(ns)
        e.set_option("bt_mfma_min", mfma_min)
        for s, pr in enumerate(prompts):
            _set(e, s, plans[s][0][1])
            e.batch_begin(s, pr)
        lg = e.batch_step(n, want_logits=True)
        toks = [tuple(int(t) for t in e.batch_tokens(s)) for s in range(ns)]
        for s, pr in enumerate(prompts):
            assert toks[s] == _cpu(pr, n + 1, plans[s]), (mfma_min, s)
            if mfma_min == NEVER:
                _slot_equals_plain(e, s, pr, plans[s], lg[:, s])
        out.append((lg, toks))
        e.close()
    _bits_equal(out[0][0].reshape(n * ns, V), out[1][0].reshape(n * ns, V), "groups against one MFMA pass")
    assert out[0][1] == out[1][1] and len(set(out[0][1])) == ns


def test_a_change_between_passes():
    """(CPU) slot 1: A(5) for the picks of indices 4 .. 7, its own greedy for 8 .. 11, the engine's E
    from 12; batch_sampler reports (mode, own) at each stage"""
    plan = ((0, A(5)), (8, None), (12, E))
    e = _engine(SHAPE)
    e.set_sampler(**_kw(E))
    e.batch_open(2)
    _set(e, 1, A(5))
    e.batch_begin(1, P(1))
    on, prm, own = e.batch_sampler(1)
    assert (on, own) == (True, True) and (prm["top_k"], prm["seed"]) == (8, 5)
    rows = [e.batch_step(7, want_logits=True)[:, 0]]  # pass i picks index i + 1: indices 1 .. 7
    _set(e, 1, None)
    assert e.batch_sampler(1)[0::2] == (False, True)
    rows.append(e.batch_step(4, want_logits=True)[:, 0])
    _set(e, 1, "engine")
    on, prm, own = e.batch_sampler(1)
    assert (on, own) == (True, False) and (prm["top_k"], prm["seed"]) == (E[1], E[3])
    rows.append(e.batch_step(4, want_logits=True)[:, 0])
    toks = _slot_equals_plain(e, 1, P(1), plan, np.concatenate(rows))
    assert tuple(toks) == _cpu(P(1), 16, plan)
    assert toks[4:] == [1357, 1357] + [3223] * 6 + [1032, 2141, 335, 2737], toks
    e.close()


def test_the_setting_belongs_to_the_slot():
    e = _engine(SHAPE)
    e.batch_open(2)
    _set(e, 1, A(5))  # on an inactive slot
    e.batch_begin(1, P(1))
    lg = e.batch_step(8, want_logits=True)
    _slot_equals_plain(e, 1, P(1), _const(A(5)), lg[:, 0], what="after begin: ")
    e.batch_release(1)
    e.batch_begin(1, P(2))
    assert e.batch_sampler(1)[0::2] == (True, True)
    lg = e.batch_step(8, want_logits=True)
    _slot_equals_plain(e, 1, P(2), _const(A(5)), lg[:, 0], what="after release and begin: ")
    e.batch_close()
    e.batch_open(2)
    assert e.batch_sampler(1)[0::2] == (False, False)
    e.batch_begin(1, P(1))
    lg = e.batch_step(8, want_logits=True)
    _slot_equals_plain(e, 1, P(1), _const(None), lg[:, 0], what="after close and open: ")
    e.close()


def test_step_rows():
    """slot 2 ingests a 20-token prompt, up to 6 rows a pass, beside two decoding slots; three
    samplers, one greedy; its first pick is its own sampler's at p = 20"""
    long = tuple(int(t) for t in O.make_prompt(20, V, seed=31))
    prompts, plans = [P(0), P(1), long], [_const(A(5)), _const(None), _const(A(6))]
    e = _engine(SHAPE)
    e.set_sampler(**_kw(E))
    e.batch_open_rows(3, 8)
    for s in range(3):
        _set(e, s, plans[s][0][1])
    e.batch_begin(0, prompts[0])
    e.batch_begin(1, prompts[1])
    e.batch_step(6)
    e.batch_begin(2, long)
    got = {s: [] for s in range(3)}
    plans_seen = []
    for _ in range(6):
        rows_of, lg = e.batch_step_rows(8, want_logits=True)
        plans_seen.append(list(rows_of))
        t = 0
        for s in range(3):
            got[s].append(lg[t:t + rows_of[s]])
            t += rows_of[s]
    assert plans_seen == [[1, 1, 6]] * 3 + [[1, 1, 2]] + [[1, 1, 1]] * 2
    for s in range(3):
        _slot_equals_plain(e, s, prompts[s], plans[s], np.concatenate(got[s]), pos0=6 if s < 2 else 0)
    rows, toks = _plain(long, e.batch_pos(2), plans[2])
    tok, _, ambiguous, _ = R.sample(rows[19], *A(6)[:3], A(6)[3], 20)
    assert not ambiguous and toks[20] == tok
    e.close()


def _corrupt(d, a):
    d = list(d)
    if a < len(d):
        d[a] = (d[a] + 1) % V
    return d


def test_batch_verify():
    """slots 0 .. 2 greedy, A(5), the engine's E with (k, a) = (3, 3), (4, 1), (2, 0), slot 3 (A(6)) sits
    out; two chained passes; tokens, positions, every layer's caches and the log-probabilities
    against plain engines"""
    prompts = [P(0), P(1), P(2), P(3)]
    plans = [_const(None), _const(A(5)), _const(E), _const(A(6))]
    e = _engine(SHAPE)
    e.set_sampler(**_kw(E))
    e.set_logprobs(1)
    e.batch_open_rows(4, 16)
    for s in (0, 1, 3):
        _set(e, s, plans[s][0][1])
    for s, pr in enumerate(prompts):
        e.batch_begin(s, pr)
    e.batch_step(8)
    pos = [8] * 4
    for ka in ({0: (3, 3), 1: (4, 1), 2: (2, 0)}, {0: (4, 1), 1: (2, 0), 2: (3, 3)}):
        drafts, want = {}, {}
        for s, (k, a) in ka.items():
            ref = _plain(prompts[s], pos[s] + k + 2, plans[s])[1]
            drafts[s] = _corrupt(ref[pos[s] + 1:pos[s] + 1 + k], a)
            want[s] = ref[pos[s] + 1:pos[s] + a + 2]
        toks = e.batch_verify(drafts)
        assert toks == want, (toks, want)
        for s, (k, a) in ka.items():
            pos[s] += a + 1
        assert [e.batch_pos(s) for s in range(4)] == pos
    for s, pr in enumerate(prompts):
        p = Plain(pr, plans[s], logprobs=True)
        p.to(pos[s])
        assert [int(t) for t in e.batch_tokens(s)] == p.tokens(), s
        for il in range(SHAPE["n_layer"]):
            k, v = e.batch_kv_read(s, il, 0, N_CTX)
            pk, pv = p.e.kv_read(il, 0, N_CTX)
            assert np.array_equal(k, pk) and np.array_equal(v, pv), (s, il)
        a, b = e.batch_logprobs(s), p.e.logprobs()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), s  # the sampler does not enter the score
        p.close()
    e.close()


def test_generate_lookup_equals_batch_step():
    """three slots adopted from prompts that repeat a 6-token block, samplers greedy / A(5) / the
    engine's: the lookup loop gives what batch_step gives a twin batch with the same settings"""
    n_new = 12
    blocks = [[int(t) for t in O.make_prompt(6, V, seed=s)] for s in (1, 2, 3)]
    prompts = [(blocks[0] * 4)[:24], (blocks[1] * 4)[:21], (blocks[2] * 4)[:19]]

    def batch():
        e = _engine(SHAPE)
        e.set_sampler(**_kw(E))
        e.batch_open_rows(3, 16)
        _set(e, 0, None)
        _set(e, 1, A(5))
        for s, pr in enumerate(prompts):
            e.begin(pr)
            e.prefill(len(pr))
            e.batch_adopt(s)
        return e

    twin = batch()
    twin.batch_step(n_new)
    refs = [[int(t) for t in twin.batch_tokens(s)] for s in range(3)]
    twin.close()
    e = batch()
    out, st = e.batch_generate_lookup(n_new, k=4, ngram_max=3)
    for s, pr in enumerate(prompts):
        assert [int(t) for t in out[s]] == refs[s][len(pr) + 1:len(pr) + 1 + n_new], s
        assert [int(t) for t in e.batch_tokens(s)] == refs[s], s
        assert st[s]["passes"] + st[s]["accepted"] + st[s]["plain_steps"] == n_new, st[s]
    e.close()


def _state(e, s):
    kv = [e.batch_kv_read(s, il, 0, N_CTX) for il in range(SHAPE["n_layer"])]
    return kv, [int(t) for t in e.batch_tokens(s)], e.batch_pos(s)


def _same_state(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[0], b[0])) and a[1:] == b[1:]


def test_fork():
    """(CPU) one prefill of 19 of 20 prompt tokens, three forks, a seed per slot: four continuations"""
    prompt = tuple(int(t) for t in O.make_prompt(20, V, seed=31))
    plans = [_const((1.0, 40, 0.95, 1 + s)) for s in range(4)]
    e = _engine(SHAPE)
    e.batch_open(4)
    e.begin(prompt)
    e.prefill_next(19)
    e.batch_adopt(0)
    for s in range(1, 4):
        e.batch_fork(0, s)
    for s in range(4):
        _set(e, s, plans[s][0][1])
    s0 = _state(e, 0)
    assert s0[2] == 19 and s0[1] == list(prompt)
    for s in range(1, 4):
        assert _same_state(_state(e, s), s0), s
    lg = e.batch_step(6, want_logits=True)
    toks = []
    for s in range(4):
        toks.append(_slot_equals_plain(e, s, prompt, plans[s], lg[:, s], pos0=19))
        assert tuple(toks[s]) == _cpu(prompt, 26, plans[s]), s
    assert toks[0][20:] == [711] * 6 and toks[1][20:23] == [3609, 3020, 740], (toks[0], toks[1])
    assert toks[2][20:23] == [311, 3298, 1789] and toks[3][20:23] == [2897, 2897, 3675], (toks[2], toks[3])
    assert len({tuple(t) for t in toks}) == 4
    # a slot whose prompt is consumed, forked over an active slot; both continue under one seed
    e.batch_fork(2, 1)
    _set(e, 1, plans[2][0][1])
    assert _same_state(_state(e, 1), _state(e, 2))
    lg = e.batch_step(4, want_logits=True)
    _bits_equal(lg[:, 1], lg[:, 2], "the fork against its source")
    assert list(e.batch_tokens(1)) == list(e.batch_tokens(2))
    _slot_equals_plain(e, 2, prompt, plans[2], lg[:, 2], pos0=25)
    e.close()


def _refused(call, *names):
    with pytest.raises(RuntimeError) as err:
        call()
    for name in names:
        assert name in str(err.value), (name, str(err.value))


def test_refusals_leave_the_state_untouched():
    SET, GET, FORK = "gemma_engine_batch_set_sampler", "gemma_engine_batch_sampler", "gemma_engine_batch_fork"
    e = _engine(SHAPE)
    _refused(lambda: e.batch_set_sampler(0, **_kw(A(5))), SET, "no batch")
    _refused(lambda: e.batch_sampler(0), GET, "no batch")
    _refused(lambda: e.batch_fork(0, 1), FORK, "no batch")
    e.batch_open(3)
    _set(e, 1, A(5))
    e.batch_begin(0, P(0))
    e.batch_begin(1, P(1))
    lg = [e.batch_step(4, want_logits=True)]
    for slot in (-1, 3):
        _refused(lambda: e.batch_set_sampler(slot, **_kw(A(5))), SET, "slot")
        _refused(lambda: e.batch_sampler(slot), GET, "slot")
        _refused(lambda: e.batch_fork(0, slot), FORK, "slot")
        _refused(lambda: e.batch_fork(slot, 0), FORK, "slot")
    _refused(lambda: e.batch_set_sampler(1, temperature=1.0, top_k=1025), SET, "top_k")
    _refused(lambda: e.batch_set_sampler(1, temperature=1.0, top_p=0.0), SET, "top_p")
    _refused(lambda: e.batch_set_sampler(1, temperature=1.0, top_p=1.5), SET, "top_p")
    _refused(lambda: e.batch_set_sampler(1, temperature=float("nan")), SET, "temperature")
    _refused(lambda: e.batch_fork(2, 0), FORK, "not active")
    _refused(lambda: e.batch_fork(1, 1), FORK, "src == dst")
    on, prm, own = e.batch_sampler(1)
    assert (on, own) == (True, True) and (prm["top_k"], prm["seed"]) == (8, 5)
    assert e.batch_sampler(0)[0::2] == (False, False) and e.batch_last()[2] == -1
    lg.append(e.batch_step(4, want_logits=True))
    lg = np.concatenate(lg)
    _slot_equals_plain(e, 0, P(0), _const(None), lg[:, 0])
    _slot_equals_plain(e, 1, P(1), _const(A(5)), lg[:, 1])
    e.close()


def test_memory_returns():
    """slot samplers on a narrow batch of a greedy engine (the batch allocates the workspaces): close,
    and freeing the engine with the batch open, return everything"""
    before = G.mem_live()
    e = _engine(SHAPE)
    idle = G.mem_live()
    for last in (False, True):
        e.batch_open(2)
        _set(e, 0, A(5))
        _set(e, 1, None)
        e.batch_begin(0, P(0))
        e.batch_begin(1, P(1))
        e.batch_step(5)
        assert G.mem_live() > idle
        if not last:
            e.batch_close()
            assert G.mem_live() == idle
    e.close()
    assert G.mem_live() == before
