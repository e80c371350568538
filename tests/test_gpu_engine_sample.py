"""On-device sampling inside the decode step (gemma_engine_set_sampler): engines on the small shapes.

The yardstick is the oracle, teacher-forced on the engine's own tokens: O.Model.inference(prompt, 0),
then inference(history, 1) along the engine's history.  Every logits row a step returns must equal
the oracle's bit for bit (uint32 views), and every token must be tests/sampler_ref.py's draw from the
oracle's row at that position.  The reference flags no draw of these cases as ambiguous; the tests
assert that instead of excluding any."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
import sampler_ref as R
from test_gpu_prefill_continue import KSHAPE
from test_gpu_persist import GEMMA_2B_LAYERS

pytestmark = pytest.mark.gpu

N_CTX, N_PROMPT, N_STEPS = 256, 20, 16
SMP = dict(temperature=1.0, top_k=40, top_p=0.95)


@functools.lru_cache(maxsize=None)
def _model(shape_key=tuple(sorted(O.TINY.items())), n_ctx=N_CTX, wtype=O.Q4_0, kmix=0):
    return O.Model(O.make_config(dict(shape_key), n_ctx=n_ctx, wtype=wtype, kmix=kmix))


def _prompt(shape=O.TINY, n=N_PROMPT):
    return [int(t) for t in O.make_prompt(n, shape["n_vocab"])]


def _oracle_rows(m, hist, n_given):
    """rows[i] = the oracle's logits that predict position n_given + i of `hist`"""
    hist = [int(t) for t in hist]
    m.reset()
    rows = [m.inference(hist[:n_given], 0)[1]]
    for k in range(n_given + 1, len(hist)):
        rows.append(m.inference(hist[:k], 1)[1])
    return np.stack(rows)


def _bits_equal(got, ref, what):
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, np.abs(got - ref).max())


def _check(m, hist, n_given, smp, seed, lg=None, what=""):
    """hist[n_given:] are the reference's draws from the oracle's rows (and lg equals those rows)"""
    rows = _oracle_rows(m, hist, n_given)
    assert len(rows) == len(hist) - n_given > 0
    if lg is not None:
        _bits_equal(lg, rows, what + " logits")
    for i, row in enumerate(rows):
        tok, _, amb, _ = R.sample(row, smp["temperature"], smp["top_k"], smp["top_p"], seed, n_given + i)
        assert not amb, (what, "ambiguous draw at", n_given + i)
        assert hist[n_given + i] == tok, (what, "position", n_given + i, list(hist[n_given:]), tok)
    return rows


def _run(e, prompt, n_gen=N_STEPS, want_logits=True, use_graph=True):
    """begin + steps over the prompt and n_gen - 1 more: n_gen tokens appended; (history, their rows)"""
    e.begin(prompt)
    lg = e.step(len(prompt) - 1 + n_gen, want_logits=want_logits, use_graph=use_graph)
    hist = list(e.tokens())
    assert len(hist) == len(prompt) + n_gen and hist[:len(prompt)] == list(prompt)
    return hist, (lg[len(prompt) - 1:] if want_logits else None)


def test_greedy_is_untouched():
    m, prompt = _model(), _prompt()
    seq_ref, lg_ref = m.generate(prompt, N_STEPS - 1)
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    assert e.sampler()[0] is False
    for setup in (lambda: None, lambda: e.set_sampler(None), lambda: e.set_sampler(temperature=0.0, top_k=7, seed=3)):
        setup()
        assert e.sampler()[0] is False
        hist, lg = _run(e, prompt)
        assert hist == list(seq_ref)
        _bits_equal(lg, lg_ref, "greedy")
    n0 = e.graph_kernels()
    e.set_sampler(seed=1, **SMP)
    assert e.sampler() == (True, dict(temperature=1.0, top_k=40, top_p=np.float32(0.95), seed=1))
    _run(e, prompt, 4, want_logits=False)
    assert e.graph_kernels() == n0 + 3  # the sampler's three launches; k_advance stays
    e.set_sampler(None)
    hist, lg = _run(e, prompt)
    assert e.graph_kernels() == n0
    assert hist == list(seq_ref)
    _bits_equal(lg, lg_ref, "greedy after sampling")
    e.close()


def test_top_k_1_is_greedy():
    m, prompt = _model(), _prompt()
    seq_ref, lg_ref = m.generate(prompt, N_STEPS - 1)
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_sampler(temperature=1.5, top_k=1, seed=5)
    hist, lg = _run(e, prompt)
    e.close()
    assert hist == list(seq_ref)
    _bits_equal(lg, lg_ref, "top_k = 1")


def test_sampled_decode_graph_eager_and_seed_change():
    m, prompt = _model(), _prompt()
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_sampler(seed=1, **SMP)
    h1, lg1 = _run(e, prompt)                       # graph replays with logits; the prompt is consumed by
    _check(m, h1, N_PROMPT, SMP, 1, lg1, "seed 1")  # steps with sampling on and is never overwritten
    e.begin(prompt)                                 # no-host-sync graph replay, batched 8 + 8
    e.step(N_PROMPT - 1, use_graph=True)
    e.step(8, use_graph=True)
    e.step(8, use_graph=True)
    assert list(e.tokens()) == h1
    e.begin(prompt)
    e.step(N_PROMPT - 1, use_graph=True)
    e.step(16, use_graph=True)
    assert list(e.tokens()) == h1
    n_graph = e.graph_kernels()
    he, _ = _run(e, prompt, want_logits=False, use_graph=False)  # eager
    assert he == h1
    # only the seed changes: a stream-ordered copy, the captured graph is kept
    e.set_sampler(seed=2, **SMP)
    assert e.graph_kernels() == n_graph
    h2, lg2 = _run(e, prompt)
    assert e.graph_kernels() == n_graph
    _check(m, h2, N_PROMPT, SMP, 2, lg2, "seed 2")
    assert h1[N_PROMPT + 1:] != h2[N_PROMPT + 1:]
    e.close()


def test_prefill_samples_the_last_row():
    m, prompt = _model(), _prompt()
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_sampler(seed=1, **SMP)
    m.reset()
    row = m.inference(prompt, 0)[1]
    ref_tok, _, amb, _ = R.sample(row, SMP["temperature"], SMP["top_k"], SMP["top_p"], 1, N_PROMPT)
    assert not amb
    e.begin(prompt)
    tok, last = e.prefill(N_PROMPT)
    _bits_equal(last, row, "prefill last row")
    assert tok == ref_tok and list(e.tokens()) == prompt + [ref_tok]
    e.step(5, use_graph=True)  # and the decode goes on sampling
    _check(m, list(e.tokens()), N_PROMPT, SMP, 1, None, "prefill + steps")
    e.begin(prompt)  # chunked: the first pass ends mid-prompt and appends nothing
    e.prefill_next(13)
    assert list(e.tokens()) == prompt[:14]
    tok, last = e.prefill_next(7)
    _bits_equal(last, row, "chunked last row")
    assert tok == ref_tok and list(e.tokens()) == prompt + [ref_tok]
    e.begin(prompt)  # the tolerance path: the reference on the engine's own last row
    tok, last = e.prefill(N_PROMPT, exact=False)
    ref_fast, _, amb, _ = R.sample(last, SMP["temperature"], SMP["top_k"], SMP["top_p"], 1, N_PROMPT)
    assert not amb and tok == ref_fast and list(e.tokens()) == prompt + [ref_fast]
    e.close()


def test_rewind_regenerates():
    m, prompt = _model(), _prompt()
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_sampler(seed=1, **SMP)
    h1, _ = _run(e, prompt, 8, want_logits=False)
    e.extend([h1[22]], keep=22)  # positions 0..21 stay, position 22 is given again
    e.step(5, use_graph=True)
    assert list(e.tokens()) == h1  # the same seed from the same history: the same continuation
    e.set_sampler(seed=2, **SMP)
    e.extend([h1[22]], keep=22)
    e.step(5, use_graph=True)
    h2 = list(e.tokens())
    e.close()
    assert h2[:23] == h1[:23] and h2 != h1
    _check(m, h2, 23, SMP, 2, None, "rewind, seed 2")


@pytest.mark.parametrize("name", ["q6k_output", "kquant_layers"])
def test_other_output_tails(name):
    if name == "q6k_output":
        shape, kw, okw = dict(O.TINY), dict(out_type=G.GGML_TYPE_Q6_K), dict(kmix=2)
    else:
        shape, kw, okw = dict(KSHAPE), dict(wtype=G.GGML_TYPE_Q4_K), dict(kmix=1)
    m = _model(tuple(sorted(shape.items())), 128, O.Q4_0, okw["kmix"])
    prompt = _prompt(shape)
    e = G.Engine(shape, n_ctx=128, **kw)
    e.set_sampler(seed=1, **SMP)
    hist, lg = _run(e, prompt, 8)
    _check(m, hist, N_PROMPT, SMP, 1, lg, name)
    e.begin(prompt)
    tok, _ = e.prefill(N_PROMPT)
    assert tok == hist[N_PROMPT] and list(e.tokens()) == hist[:N_PROMPT + 1]
    e.close()


def test_att_o_launch_form():
    m, prompt = _model(), _prompt()
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    assert e.set_att_o(1)
    e.set_sampler(seed=1, **SMP)
    hist, lg = _run(e, prompt, 8)
    e.close()
    _check(m, hist, N_PROMPT, SMP, 1, lg, "att_o")


def test_persistent_launch_form():
    O.lib().orc_set_threads(16)
    shape = dict(GEMMA_2B_LAYERS)
    m = _model(tuple(sorted(shape.items())), 128)
    prompt = _prompt(shape, 6)
    e = G.Engine(shape, n_ctx=128)
    assert e.set_persist(1)
    e.persist_err(reset=True)
    e.set_sampler(seed=1, **SMP)
    hist, lg = _run(e, prompt, 6)
    err = e.persist_err()
    e.close()
    assert err[0] == 0, err
    _check(m, hist, 6, SMP, 1, lg, "persist")


def test_row_split_engines_refuse():
    shape, prompt = dict(O.TINY), _prompt()
    seq_ref, _ = _model().generate(prompt, 3)
    for tp in ((2, 0, None), (1, 0, G.tp_unique_id())):
        t = G.Engine(shape, n_ctx=N_CTX, device=0, tp=tp)
        with pytest.raises(RuntimeError, match="row-split"):
            t.set_sampler(seed=1, **SMP)
        assert t.sampler()[0] is False
        t.set_sampler(None)  # greedy is what they do
        hist, _ = _run(t, prompt, 4, want_logits=False)
        t.close()
        assert hist == list(seq_ref)


def test_bad_fields_leave_the_sampler():
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_sampler(seed=4, **SMP)
    before = e.sampler()
    for kw, field in ((dict(top_k=1025), "top_k"), (dict(top_k=-1), "top_k"), (dict(top_p=0.0), "top_p"),
                      (dict(top_p=1.5), "top_p"), (dict(temperature=float("inf")), "temperature")):
        with pytest.raises(RuntimeError, match=field):
            e.set_sampler(**dict(dict(temperature=1.0, seed=4), **kw))
        assert e.sampler() == before
    e.close()
