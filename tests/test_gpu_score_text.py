"""scripts/score_text.py on TINY: the perplexity it reports from the device's log-probabilities (chunked
prefill_next, no logits_all) equals exp(-mean(lp)) computed with tests/logprob_ref.py from the
logits_all of a one-pass prefill of the same text, to 1e-9 per token and in the perplexity's log."""
import importlib.util
import os

import numpy as np
import pytest

import gemma_hip as G
import logprob_ref as R
import oracle_ctypes as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("score_text", os.path.join(ROOT, "scripts", "score_text.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_score_text_equals_numpy_on_logits_all(tmp_path):
    S = _script()
    assert S.SHAPES["tiny"] == O.TINY
    T = 50
    text = [int(t) for t in O.make_prompt(T, O.TINY["n_vocab"], 3)]
    path = tmp_path / "ids.txt"
    path.write_text(", ".join(str(t) for t in text[:25]) + "\n" + " ".join(str(t) for t in text[25:]))
    assert S.read_tokens(str(path)) == text
    e = G.Engine(dict(O.TINY), n_ctx=128)
    e.begin(text)
    rows = e.prefill(T, want_all=True)[2]           # logits_all of the one-pass exact prefill, scoring off
    ref = R.logprobs(rows[:-1], text[1:])
    for chunk in (7, 64):
        lp, host = S.score(e, text, chunk, check=True)
        assert np.isnan(lp[0]) and R.close(lp[1:], ref).all(), np.abs(lp[1:] - ref).max()
        assert R.close(host[1:], ref).all()
        assert abs(-lp[1:].mean() + ref.mean()) <= R.MARGIN  # log perplexity: a mean of values each within the margin
        assert np.exp(-lp[1:].mean()) == pytest.approx(np.exp(-ref.mean()), rel=1e-9, abs=0.0)
    e.close()
