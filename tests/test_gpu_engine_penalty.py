"""Penalties inside the engine's picks (gemma_engine_set_penalties) on the tiny synthetic shape.

The yardstick needs no oracle: every step returns its raw logits row, and the token the engine appends
must be the pick (greedy, or tests/sampler_ref.py / sampler_full_ref.py's draw) from the numpy-penalised
copy of that row over the sequence so far.  A returned row that was not raw would be penalised twice by
the check and the streams would part."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
import sampler_full_ref as F
import sampler_ref as R
from test_gpu_penalty import penalise

pytestmark = pytest.mark.gpu

N_CTX, N_PROMPT, N_GEN = 256, 12, 40
PEN = dict(repeat=1.25, presence=0.25, frequency=0.125, last_n=64)
GREEDY, K40, ALL = None, dict(temperature=1.0, top_k=40, top_p=0.95, seed=3), dict(temperature=0.9, top_k=G.TOP_K_ALL, top_p=0.9, seed=5)


def _prompt(seed=0, n=N_PROMPT):
    return [int(t) for t in np.random.default_rng(seed).integers(0, O.TINY["n_vocab"], n)]


def _engine(pen=PEN, smp=GREEDY):
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_penalties(**pen)
    if smp:
        e.set_sampler(**smp)
    return e


def _pick(row, hist, pen, smp):
    """the token for index len(hist) from the raw row that processed hist[-1]"""
    l, _ = penalise(row, hist, len(hist) - 1, pen["repeat"], pen["presence"], pen["frequency"], pen["last_n"])
    if smp is None:
        return int(np.argmax(l))  # the larger logit, then the smaller index
    if smp["top_k"] == G.TOP_K_ALL:
        tok, amb = F.Table(l, smp["temperature"], smp["top_p"]).draw(smp["seed"], len(hist))
    else:
        tok, _, amb, _ = R.sample(l, smp["temperature"], smp["top_k"], smp["top_p"], smp["seed"], len(hist))
    assert not amb
    return int(tok)


def _run(e, prompt, n_gen=N_GEN, **kw):
    e.begin(prompt)
    lg = e.step(len(prompt) - 1 + n_gen, **kw)
    return [int(t) for t in e.tokens()], lg


@pytest.mark.parametrize("smp", [GREEDY, K40, ALL], ids=["greedy", "k40", "all"])
@pytest.mark.parametrize("last_n", [8, 64])
def test_steps_pick_from_the_penalised_row(last_n, smp):
    pen, prompt = dict(PEN, last_n=last_n), _prompt()
    e = _engine(pen, smp)
    assert e.penalties() == (True, pen)
    hist, lg = _run(e, prompt, want_logits=True, use_graph=False)
    graph, _ = _run(e, prompt, use_graph=True)
    e.set_penalties(None)
    plain, _ = _run(e, prompt, use_graph=True)
    e.close()
    assert graph == hist and hist[:N_PROMPT] == prompt and plain != hist
    for i in range(N_PROMPT - 1, len(hist) - 1):  # row i processed hist[i]
        assert hist[i + 1] == _pick(lg[i], hist[:i + 1], pen, smp), i


def test_prefill_picks():
    prompt = _prompt(1)
    e = _engine()
    for exact in (True, False):
        e.begin(prompt)
        tok, last = e.prefill(N_PROMPT, exact=exact)
        assert tok == _pick(last, prompt, PEN, GREEDY) and list(e.tokens()) == prompt + [tok]
    e.begin(prompt)
    e.prefill_next(7)
    tok, last = e.prefill_next(5)
    assert tok == _pick(last, prompt, PEN, GREEDY) and list(e.tokens()) == prompt + [tok]
    e.close()


@pytest.mark.parametrize("rows", [False, True], ids=["batch_step", "batch_step_rows"])
def test_batch_slots_equal_single_sequences(rows):
    prompts = [_prompt(s, n) for s, n in ((2, 12), (3, 12), (4, 40 if rows else 12))]
    e = _engine()
    single = [_run(e, p, 64)[0] for p in prompts]
    if rows:  # 16-row passes (the batch's own save lists): slot 2 takes its prompt in chunks beside two decoding slots
        e.batch_open_rows(3, 16)
        for s in (0, 1):
            e.batch_begin(s, prompts[s])
        e.batch_step(N_PROMPT + 1)
        e.batch_begin(2, prompts[2])
        plans = [list(e.batch_step_rows(16)[0]) for _ in range(30)]
        assert plans[0] == [1, 1, 14] and plans[-1] == [1, 1, 1]
    else:
        e.batch_open(3)
        for s, p in enumerate(prompts):
            e.batch_begin(s, p)
        e.batch_step(N_PROMPT - 1 + 30)
    for s, ref in enumerate(single):
        got = [int(t) for t in e.batch_tokens(s)]
        assert len(got) > len(prompts[s]) + 10 and got == ref[:len(got)], s
    e.close()


def test_logprobs_stay_raw():
    e = _engine()
    e.set_logprobs(1)
    hist, _ = _run(e, _prompt(5))
    lp = e.logprobs()
    e.set_penalties(None)  # the same tokens as a given text, scored with penalties off
    e.extend(hist, keep=0)
    e.step(len(hist) - 1)
    raw = e.logprobs()
    e.close()
    n = len(hist)
    assert np.isfinite(lp[1:n]).all() and np.array_equal(lp[:n].view(np.uint64), raw[:n].view(np.uint64))


def test_parameter_change_keeps_the_graph():
    e, prompt = G.Engine(dict(O.TINY), n_ctx=N_CTX), _prompt()
    _run(e, prompt, 4)
    n0 = e.graph_kernels()
    e.set_penalties(**PEN)
    hist, _ = _run(e, prompt, 20)
    n_on = e.graph_kernels()
    assert n_on == n0 + 3  # apply, the row argmax of the penalised row, restore
    pen2 = dict(repeat=1.1, presence=0.0, frequency=0.5, last_n=5)
    e.set_penalties(**pen2)
    assert e.graph_kernels() == n_on
    lg = e.step(6, want_logits=True)
    assert e.graph_kernels() == n_on
    hist2 = [int(t) for t in e.tokens()]
    for i in range(len(hist) - 1, len(hist2) - 1):
        assert hist2[i + 1] == _pick(lg[i - (len(hist) - 1)], hist2[:i + 1], pen2, GREEDY), i
    e.set_penalties(1.0, 0.0, 0.0, 64)
    assert e.penalties()[0] is False
    _run(e, prompt, 4)
    assert e.graph_kernels() == n0
    e.close()


def test_refusals():
    e = _engine()
    before = e.penalties()
    for bad, word in ((dict(repeat=0.0), "repeat"), (dict(last_n=0), "last_n"), (dict(last_n=8193), "last_n"),
                      (dict(presence=float("inf")), "finite")):
        with pytest.raises(RuntimeError, match=word):
            e.set_penalties(**dict(PEN, **bad))
        assert e.penalties() == before
    hist, _ = _run(e, _prompt(), 4)
    e.batch_open(2)
    e.batch_adopt(0)
    with pytest.raises(RuntimeError, match="penalties"):
        e.verify([1, 2])
    with pytest.raises(RuntimeError, match="penalties"):
        e.batch_verify({0: [1, 2]})
    assert list(e.tokens()) == hist
    e.set_penalties(None)
    assert len(e.verify([1, 2])) >= 1 and len(e.batch_verify({0: [1, 2]})[0]) >= 1
    e.close()
