"""bench.py --dump-outputs: the files written for a finished timed call, checked on a stub engine."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _StubEngine:
    """the slice of gemma_hip.Engine that dump_outputs uses: a 3-token prompt, 2 warmup and 4 timed steps done"""

    def __init__(self):
        self.seq = np.array([2, 11, 12, 13, 21, 22, 31, 32, 33, 34], dtype=np.int32)
        self.calls = []

    def tokens(self):
        return self.seq.copy()

    def step(self, n, want_logits=False, use_graph=True):
        self.calls.append((n, want_logits, use_graph))
        return np.linspace(-1.0, 1.0, 7, dtype=np.float32)[None].repeat(n, 0)


def test_dump_outputs_writes_the_timed_tokens_and_the_next_logits_row(tmp_path):
    from bench import dump_outputs
    eng = _StubEngine()
    out = str(tmp_path / "nested" / "dump")
    shapes = dump_outputs(eng, 4, out)
    assert shapes == {"tokens": [4], "next_step_logits": [7]}
    assert sorted(os.listdir(out)) == ["next_step_logits.npy", "tokens.npy"]
    toks = np.load(os.path.join(out, "tokens.npy"))
    lg = np.load(os.path.join(out, "next_step_logits.npy"))
    assert toks.dtype == np.float64 and lg.dtype == np.float64
    assert toks.tolist() == [31.0, 32.0, 33.0, 34.0]  # the timed steps' tokens, the last step's last
    assert np.array_equal(lg, np.linspace(-1.0, 1.0, 7, dtype=np.float32).astype(np.float64))
    assert eng.calls == [(1, True, True)]  # one further replay of the decode graph, after reading the tokens
