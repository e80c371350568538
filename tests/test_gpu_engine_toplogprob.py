"""The alternatives on the engine (gemma_engine_set_top_logprobs, n = 5): TINY at n_ctx 128, Q4_0, a
40-token prompt and 8 generated tokens.  The yardstick is tests/toplogprob_ref.py on the engine's own
logits rows; everything else is compared as bytes: every path leaves the same alternatives for an index."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
import toplogprob_ref as T

pytestmark = pytest.mark.gpu

N_CTX, N_PROMPT, N_GEN, TOP = 128, 40, 8, 5
N_SEQ = N_PROMPT + N_GEN
V = O.TINY["n_vocab"]
PROMPT = [int(t) for t in O.make_prompt(N_PROMPT, V, 1)]


def _alts(tok, lps):
    return tok.tobytes() + lps.tobytes()


def _steps(e, graph):
    e.begin(PROMPT)
    lg = e.step(N_SEQ - 1, want_logits=True, use_graph=graph)
    return _alts(*e.top_logprobs(0, N_SEQ)), lg


def _prefill(e, chunks):
    e.begin(PROMPT)
    for n in chunks:
        e.prefill_next(n)
    e.step(N_GEN - 1, use_graph=True)
    return _alts(*e.top_logprobs(0, N_SEQ))


def _batch(e, n_slots, slot, fork=None):
    """PROMPT in `slot` (or in slot 0, forked to `slot` after `fork` steps), other prompts beside it"""
    (e.batch_open_wide if n_slots > G.BATCH_MAX_SLOTS else e.batch_open)(n_slots)
    for s in range(n_slots):
        if fork is None or s != slot:
            e.batch_begin(s, PROMPT if s == (slot if fork is None else 0) else [int(t) for t in O.make_prompt(N_PROMPT, V, 10 + s)])
    if fork is not None:
        e.batch_step(fork)
        e.batch_fork(0, slot)
    e.batch_step(N_SEQ - 1 - (fork or 0))
    res = _alts(*e.batch_top_logprobs(slot, 0, N_SEQ))
    e.batch_close()
    return res


@functools.lru_cache(maxsize=None)
def _run():
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    assert e.set_logprobs(1) is True and e.set_top_logprobs(TOP) == TOP == e.set_top_logprobs()
    base, lg = _steps(e, True)
    hist = [int(t) for t in e.tokens()]
    out = dict(tokens=hist, logits=lg, tok=e.top_logprobs(0, N_SEQ)[0], lps=e.top_logprobs(0, N_SEQ)[1], lp=e.logprobs(0, N_SEQ))
    paths = {"graph": base, "eager": _steps(e, False)[0], "prefill": _prefill(e, (N_PROMPT,)),
             "prefill_next 16 16 8": _prefill(e, (16, 16, 8)), "batch 3": _batch(e, 3, 1), "wide 12": _batch(e, 12, 5),
             "fork": _batch(e, 3, 2, fork=N_PROMPT + 2)}
    # a verify pass: two of four drafts accepted; the rejected rows' indices stay (-1, NaN)
    e.begin(PROMPT)
    e.prefill(N_PROMPT)
    wrong = [(hist[N_PROMPT + 3] + 1) % V, (hist[N_PROMPT + 4] + 1) % V]
    assert e.verify(hist[N_PROMPT + 1:N_PROMPT + 3] + wrong) == hist[N_PROMPT + 1:N_PROMPT + 4]
    e.set_logprobs(0)  # (the alternatives go off with them) the rest of the sequence unscored, to read past the pass
    e.step(N_SEQ - 1 - e.pos(), use_graph=True)
    assert e.set_logprobs(1) is True and e.set_top_logprobs(TOP) == TOP
    out["verify"] = e.top_logprobs(0, N_SEQ)
    # extend(keep): the alternatives stay below keep and are cleared from it on
    e.extend([hist[N_PROMPT + 1]], keep=N_PROMPT + 1)
    out["extend"] = e.top_logprobs(0, N_PROMPT + 2)
    e.close()
    out["paths"] = paths
    return out


def test_alternatives_equal_numpy_on_the_engines_rows():
    r = _run()
    tok, lps = T.tops(r["logits"], TOP)
    assert (r["tok"][0] == -1).all() and np.isnan(r["lps"][0]).all()  # no row predicts index 0
    assert np.array_equal(r["tok"][1:], tok)
    assert T.close(r["lps"][1:], lps).all(), np.abs(r["lps"][1:] - lps).max()
    # alternative 0 is the greedy pick, and the scored token's value has the bytes of lp
    assert list(r["tok"][N_PROMPT:, 0]) == r["tokens"][N_PROMPT:]
    hit = r["tok"] == np.array(r["tokens"])[:, None]
    assert hit[N_PROMPT:].any(axis=1).all()
    assert r["lps"][hit].tobytes() == r["lp"][hit.any(axis=1)].tobytes()


@pytest.mark.parametrize("path", ["eager", "prefill", "prefill_next 16 16 8", "batch 3", "wide 12", "fork"])
def test_every_path_leaves_the_same_bytes(path):
    r = _run()
    assert r["paths"][path] == r["paths"]["graph"], path


def test_verify_and_extend():
    r = _run()
    for name, n_kept in (("verify", N_PROMPT + 4), ("extend", N_PROMPT + 1)):
        tok, lps = r[name]
        assert _alts(tok[:n_kept], lps[:n_kept]) == _alts(r["tok"][:n_kept], r["lps"][:n_kept]), name
        assert (tok[n_kept:] == -1).all() and np.isnan(lps[n_kept:]).all(), name


def test_graph_kernels_and_refusals():
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    with pytest.raises(RuntimeError, match="gemma_engine_set_top_logprobs.*turn those on first"):
        e.set_top_logprobs(TOP)
    e.begin(PROMPT)
    with pytest.raises(RuntimeError, match="gemma_engine_top_logprobs.*are off"):
        e.top_logprobs(0, 1)
    counts = []
    for lp, top in ((1, 0), (1, TOP), (1, 20), (0, 0)):
        e.set_logprobs(lp)
        assert e.set_top_logprobs(top if lp else -1) == top  # turning log-probabilities off turns the alternatives off
        e.begin(PROMPT)
        e.step(3, use_graph=True)
        counts.append(e.graph_kernels())
    assert counts == [counts[3] + 2, counts[3] + 4, counts[3] + 4, counts[3]]
    e.set_logprobs(1)
    with pytest.raises(RuntimeError, match="gemma_engine_set_top_logprobs: n = 33 outside"):
        e.set_top_logprobs(G.TOP_LOGPROBS_MAX + 1)
    e.batch_open(2)
    with pytest.raises(RuntimeError, match="gemma_engine_set_top_logprobs.*a batch is open"):
        e.set_top_logprobs(TOP)
    e.batch_begin(0, PROMPT)
    with pytest.raises(RuntimeError, match="gemma_engine_batch_top_logprobs.*are off"):
        e.batch_top_logprobs(0, 0, 1)
    e.batch_close()
    e.close()
    t = G.Engine(dict(O.TINY), n_ctx=N_CTX, tp=(2, 0, None))  # virtual ranks: a vocabulary shard per rank
    with pytest.raises(RuntimeError, match="gemma_engine_set_top_logprobs.*row-split"):
        t.set_top_logprobs(TOP)
    t.close()
