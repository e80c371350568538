"""Per-token log-probabilities on the engine (gemma_engine_set_logprobs): TINY at n_ctx 128, Q4_0, a
12-token prompt and 8 generated tokens, plus one case each on the Q6_K head and on K-quant layers.

The yardstick is tests/logprob_ref.py on the engine's OWN logits rows (the rows themselves are held to
the oracle by the other engine tests): lp[i] = logprob(row_{i-1}, tokens[i]) within 1e-9, the margin
derived in logprob_ref.  Everything else is compared as bytes: every path that computes a row gives the
same lp for it, and turning log-probabilities on changes no token and no logits row."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import logprob_ref as R
import oracle_ctypes as O
from test_gpu_prefill_continue import KSHAPE

pytestmark = pytest.mark.gpu

N_CTX, N_PROMPT, N_GEN = 128, 12, 8
N_SEQ = N_PROMPT + N_GEN  # sequence indices 0 .. 19; rows 0 .. 18 predict indices 1 .. 19
SMP = dict(temperature=0.8, top_k=40, top_p=0.95, seed=7)
V = O.TINY["n_vocab"]


def _prompt(shape=O.TINY, seed=1, n=N_PROMPT):
    return [int(t) for t in O.make_prompt(n, shape["n_vocab"], seed)]


def _engine(lp, sampler, shape=O.TINY, **kw):
    e = G.Engine(dict(shape), n_ctx=N_CTX, **kw)
    if sampler:
        e.set_sampler(**SMP)
    assert e.set_logprobs(1 if lp else 0) is bool(lp)
    return e


def _res(tokens, lp, logits=None, row0=0, n_lp=N_SEQ):
    """a path's result: the tokens, lp[0 .. n_lp) and the logits rows of sequence indices row0 .."""
    return dict(tokens=[int(t) for t in tokens], lp=np.array(lp[:n_lp]), logits=logits, row0=row0)


# ---- the paths: each leaves the 20-token sequence of `prompt` and returns _res(...) ----------------
def _steps(e, prompt, graph):
    e.begin(prompt)
    lg = e.step(N_SEQ - 1, want_logits=True, use_graph=graph)
    return _res(e.tokens(), e.logprobs(0, N_SEQ), lg)


def _split_steps(e, prompt, parts):
    e.begin(prompt)
    e.step(N_PROMPT - 1, use_graph=True)
    for n in parts:
        e.step(n, use_graph=True)  # graph replays, no host synchronise between them
    return _res(e.tokens(), e.logprobs(0, N_SEQ))


def _prefill(e, prompt, chunks):
    e.begin(prompt)
    if chunks is None:
        rows = [e.prefill(N_PROMPT, want_all=True)[2]]
    else:
        rows = [e.prefill_next(n, want_all=True)[2] for n in chunks]
    rows.append(e.step(N_GEN - 1, want_logits=True, use_graph=True))
    return _res(e.tokens(), e.logprobs(0, N_SEQ), np.concatenate(rows))


def _verify(e, prompt, hist):
    """a half-right draft of 4: two drafts accepted, three tokens appended; then 4 steps with
    log-probabilities off, so that the indices past the accepted prefix can be read back"""
    e.begin(prompt)
    e.prefill(N_PROMPT)
    wrong = [(hist[N_PROMPT + 3] + 1) % V, (hist[N_PROMPT + 4] + 1) % V]
    toks, rows = e.verify(hist[N_PROMPT + 1:N_PROMPT + 3] + wrong, want_all=True)
    assert toks == hist[N_PROMPT + 1:N_PROMPT + 4] and e.pos() == N_PROMPT + 3
    was = e.set_logprobs(-1)
    e.set_logprobs(0)
    e.step(N_SEQ - 1 - e.pos(), use_graph=True)
    e.set_logprobs(1 if was else 0)
    lp = e.logprobs(0, N_SEQ)
    assert np.isnan(lp[N_PROMPT + 4:]).all(), lp  # rejected rows and unscored steps wrote nothing
    return _res(e.tokens(), lp, rows[:3], row0=N_PROMPT, n_lp=N_PROMPT + 4)


def _lookup(e, prompt):
    e.begin(prompt)
    e.prefill(N_PROMPT)
    out, st = e.generate_lookup(N_GEN - 1, k=4, ngram_max=3)
    print("generate_lookup stats:", st)
    return _res(e.tokens(), e.logprobs(0, N_SEQ))


def _batch(e, prompt, n_slots, slot, mfma_min=None):
    """`prompt` in `slot`, other prompts in every other slot; the other slots are held to numpy"""
    (e.batch_open_wide if n_slots > G.BATCH_MAX_SLOTS else e.batch_open)(n_slots)
    if mfma_min is not None:
        e.set_option("bt_mfma_min", mfma_min)
    for s in range(n_slots):
        e.batch_begin(s, prompt if s == slot else _prompt(seed=10 + s))
    lg = e.batch_step(N_SEQ - 1, want_logits=True)  # [19][n_slots][V]: all slots active, row = slot
    for s in (0, n_slots - 1) if e.set_logprobs(-1) else ():
        _assert_numpy(e.batch_logprobs(s, 0, N_SEQ), lg[:, s], e.batch_tokens(s), "slot %d of %d" % (s, n_slots))
    res = _res(e.batch_tokens(slot), e.batch_logprobs(slot, 0, N_SEQ), np.ascontiguousarray(lg[:, slot]))
    e.batch_close()
    return res


def _adopt(e, prompt):
    e.begin(prompt)
    first = e.prefill(N_PROMPT, want_all=True)[2]
    e.batch_open(2)
    e.batch_adopt(1)
    lg = e.batch_step(N_GEN - 1, want_logits=True)
    res = _res(e.batch_tokens(1), e.batch_logprobs(1, 0, N_SEQ), np.concatenate([first, lg[:, 0]]))
    e.batch_close()
    return res


def _assert_numpy(lp, rows, tokens, what):
    """lp[0] is NaN and lp[i] = logprob(row_{i-1}, tokens[i]) within the margin"""
    assert len(lp) == len(rows) + 1 == len(tokens), what
    assert np.isnan(lp[0]), what
    ref = R.logprobs(rows, tokens[1:])
    print(what, "max |gpu - numpy| =", np.abs(lp[1:] - ref).max())
    ok = R.close(lp[1:], ref)
    assert ok.all(), (what, np.flatnonzero(~ok), lp[1:][~ok], ref[~ok])


@functools.lru_cache(maxsize=None)
def _results(lp, sampler):
    """every path on one engine, log-probabilities on or off, greedy or sampled"""
    e = _engine(lp, sampler)
    prompt = _prompt()
    out = {"graph": _steps(e, prompt, True)}
    hist = out["graph"]["tokens"]
    assert len(hist) == N_SEQ and hist[:N_PROMPT] == prompt
    out["eager"] = _steps(e, prompt, False)
    out["step 4 + 4"] = _split_steps(e, prompt, (4, 4))
    out["step 8"] = _split_steps(e, prompt, (8,))
    out["prefill"] = _prefill(e, prompt, None)
    out["prefill_next 5 5 2"] = _prefill(e, prompt, (5, 5, 2))
    out["verify"] = _verify(e, prompt, hist)
    out["generate_lookup"] = _lookup(e, prompt)
    out["batch 3"] = _batch(e, prompt, 3, 1)
    out["wide 12, mfma"] = _batch(e, prompt, 12, 5, 9)
    out["wide 12, groups"] = _batch(e, prompt, 12, 5, 65)
    out["adopt"] = _adopt(e, prompt)
    e.close()
    return out


@pytest.mark.parametrize("sampler", [False, True], ids=["greedy", "sampled"])
def test_lp_equals_numpy_on_the_raw_row(sampler):
    """with the sampler on too: the score is under softmax(row), not the tempered, truncated one"""
    r = _results(True, sampler)["graph"]
    _assert_numpy(r["lp"], r["logits"], r["tokens"], "steps")
    if sampler:  # and the two scales do differ here: the tempered row gives other numbers
        tempered = R.logprobs(r["logits"] / np.float32(SMP["temperature"]), r["tokens"][1:])
        assert np.abs(tempered - r["lp"][1:]).max() > 1e-3


@pytest.mark.parametrize("sampler", [False, True], ids=["greedy", "sampled"])
def test_one_value_per_row_and_token_on_every_path(sampler):
    res = _results(True, sampler)
    base = res["graph"]
    assert not np.isnan(base["lp"][1:]).any()
    for name, r in res.items():
        assert r["tokens"] == base["tokens"], name
        n = len(r["lp"])
        assert r["lp"].tobytes() == base["lp"][:n].tobytes(), (name, r["lp"], base["lp"][:n])


@pytest.mark.parametrize("sampler", [False, True], ids=["greedy", "sampled"])
def test_on_changes_no_token_and_no_logits_row(sampler):
    on, off = _results(True, sampler), _results(False, sampler)
    assert on.keys() == off.keys()
    for name in on:
        assert on[name]["tokens"] == off[name]["tokens"], name
        assert np.isnan(off[name]["lp"]).all(), name  # off: nothing is scored
        a, b = on[name]["logits"], off[name]["logits"]
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
            # and the rows are the base path's rows of the same sequence indices
            base = on["graph"]["logits"][on[name]["row0"]:on[name]["row0"] + len(a)]
            assert a.tobytes() == base.tobytes(), name


@pytest.mark.parametrize("name", ["q6k_output", "kquant_layers"])
def test_other_output_tails(name):
    if name == "q6k_output":
        shape, kw = dict(O.TINY), dict(out_type=G.GGML_TYPE_Q6_K)
    else:
        shape, kw = dict(KSHAPE), dict(wtype=G.GGML_TYPE_Q4_K)
    e = _engine(True, False, shape, **kw)
    prompt = _prompt(shape)
    a = _steps(e, prompt, True)
    _assert_numpy(a["lp"], a["logits"], a["tokens"], name)
    for r in (_steps(e, prompt, False), _prefill(e, prompt, None), _prefill(e, prompt, (5, 5, 2))):
        assert r["tokens"] == a["tokens"] and r["lp"].tobytes() == a["lp"].tobytes() and r["logits"].tobytes() == a["logits"].tobytes()
    e.close()


def test_extend_begin_and_positions_stepped_while_off():
    e = _engine(True, False)
    prompt = _prompt()
    base = _steps(e, prompt, True)
    hist, lp = base["tokens"], base["lp"]
    keep = 15
    # extend: lp[:keep] stays, NaN from keep on (row keep - 1 is not recomputed); read back through
    # steps taken with log-probabilities off
    e.extend([hist[keep]], keep=keep)
    assert e.logprobs(0, keep + 1)[:keep].tobytes() == lp[:keep].tobytes() and np.isnan(e.logprobs(keep, 1)[0])
    e.set_logprobs(0)
    e.step(N_SEQ - 1 - keep, use_graph=True)
    got = e.logprobs(0, N_SEQ)
    assert list(e.tokens()) == hist
    assert got[:keep].tobytes() == lp[:keep].tobytes() and np.isnan(got[keep:]).all(), got
    # the same rewind scored: the rows from keep on give indices keep + 1 .. as before, lp[keep] stays NaN
    e.set_logprobs(1)
    e.extend([hist[keep]], keep=keep)
    e.step(N_SEQ - 1 - keep, use_graph=True)
    got = e.logprobs(0, N_SEQ)
    assert np.isnan(got[keep]) and got[:keep].tobytes() == lp[:keep].tobytes()
    assert got[keep + 1:].tobytes() == lp[keep + 1:].tobytes()
    # begin resets all of it; positions stepped while off are NaN after turning on
    e.begin(prompt)
    e.set_logprobs(0)
    e.step(N_PROMPT + 2, use_graph=True)
    assert e.set_logprobs(1) is True
    assert np.isnan(e.logprobs(0, N_PROMPT + 3)).all()
    e.step(N_SEQ - 1 - e.pos(), use_graph=True)
    got = e.logprobs(0, N_SEQ)
    assert list(e.tokens()) == hist
    assert np.isnan(got[:N_PROMPT + 3]).all() and got[N_PROMPT + 3:].tobytes() == lp[N_PROMPT + 3:].tobytes()
    e.close()


@pytest.mark.parametrize("sampler", [False, True], ids=["greedy", "sampled"])
def test_graph_grows_by_two_kernels(sampler):
    e = _engine(False, sampler)
    prompt = _prompt()
    e.begin(prompt)
    e.step(3, use_graph=True)
    n0 = e.graph_kernels()
    assert e.set_logprobs(1) is True and e.set_logprobs(-1) is True
    e.begin(prompt)
    e.step(3, use_graph=True)
    assert e.graph_kernels() == n0 + 2
    assert e.set_logprobs(0) is False
    e.begin(prompt)
    e.step(3, use_graph=True)
    assert e.graph_kernels() == n0
    e.close()


def test_refusals_leave_the_state():
    t = G.Engine(dict(O.TINY), n_ctx=N_CTX, tp=(2, 0, None))  # virtual ranks: a vocabulary shard per rank
    with pytest.raises(RuntimeError, match="gemma_engine_set_logprobs.*row-split"):
        t.set_logprobs(1)
    assert t.set_logprobs(-1) is False and t.set_logprobs(0) is False
    t.close()
    e = _engine(True, False)
    prompt = _prompt()
    base = _steps(e, prompt, True)
    for p0, n in ((0, N_SEQ + 1), (-1, 2), (N_SEQ, 1), (3, -1)):
        with pytest.raises(RuntimeError, match="gemma_engine_logprobs"):
            e.logprobs(p0, n)
    assert len(e.logprobs(N_SEQ, 0)) == 0
    with pytest.raises(RuntimeError, match="gemma_engine_batch_logprobs: no batch is open"):
        e.batch_logprobs(0, 0, 1)
    e.batch_open(2)
    e.batch_begin(0, prompt)
    e.batch_step(2)
    for slot, p0, n, why in ((2, 0, 1, "slot 2 outside"), (1, 0, 1, "slot 1 is not active"), (0, 0, N_PROMPT + 1, "outside")):
        with pytest.raises(RuntimeError, match="gemma_engine_batch_logprobs: .*" + why):
            e.batch_logprobs(slot, p0, n)
    assert len(e.batch_logprobs(0, 0, N_PROMPT)) == N_PROMPT
    e.batch_close()
    assert e.logprobs(0, N_SEQ).tobytes() == base["lp"].tobytes() and list(e.tokens()) == base["tokens"]
    e.close()


def test_memory_returns():
    live0 = G.mem_live()
    e = _engine(True, True)
    prompt = _prompt()
    _prefill(e, prompt, None)  # a pass of more than 8 rows: the prefill scratch brings its own partials
    before = G.mem_live()
    for wide in (False, True):
        _batch(e, prompt, 12 if wide else 3, 1)
        assert G.mem_live() == before
    e.close()
    assert G.mem_live() == live0
