"""The K / V read-back (gemma_engine_kv_read, gemma_engine_batch_kv_read) at positions other than
(0, n_ctx): one function serves the engine's own sequence and a batch slot, so both are read.

After a 40-token prompt every partial read must equal the same rows of the full read bit for bit, on
the first and on the last layer, and the rows the prompt never reached must be zero.  The ranges are a
single first row, a pair across the 32-position boundary, the last filled row alone, and a run that
starts mid-cache and ends on the last filled row."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O

pytestmark = pytest.mark.gpu

N_CTX, N_PROMPT = 256, 40
RANGES = ((0, 1), (31, 2), (39, 1), (7, 33))


@pytest.fixture(scope="module")
def engine():
    shape = dict(O.TINY)
    e = G.Engine(shape, n_ctx=N_CTX, device=0)
    e.begin(O.make_prompt(N_PROMPT, shape["n_vocab"]))
    e.prefill(N_PROMPT)
    e.batch_open(2)
    e.batch_adopt(1)
    yield e
    e.batch_close()
    e.close()


@pytest.mark.parametrize("who", ["own", "slot"])
def test_partial_reads_are_rows_of_the_full_read(engine, who):
    e = engine
    read = e.kv_read if who == "own" else (lambda layer, p0, n: e.batch_kv_read(1, layer, p0, n))
    for layer in (0, e.cfg.n_layer - 1):
        k_all, v_all = read(layer, 0, N_CTX)
        assert k_all[:N_PROMPT].any() and v_all[:N_PROMPT].any(), "the prompt's rows are empty"
        assert not k_all[N_PROMPT:].any() and not v_all[N_PROMPT:].any(), "rows past the prompt are not zero"
        for p0, n in RANGES:
            k, v = read(layer, p0, n)
            assert k.shape == v.shape == (n, k_all.shape[1])
            assert np.array_equal(k, k_all[p0:p0 + n]), (who, layer, p0, n, "K")
            assert np.array_equal(v, v_all[p0:p0 + n]), (who, layer, p0, n, "V")
