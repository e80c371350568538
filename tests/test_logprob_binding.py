"""CPU: the four log-probability calls (gemma_engine_set_logprobs, gemma_engine_logprobs,
gemma_engine_batch_logprobs, gemma_test_logprob) are declared in include/gemma_hpc.h, listed in the
Python binding's EXPORTS (tests/test_capi_symbols.py then checks the built library exports them) and
wrapped; the reference helper's chunk size equals the kernels'."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip  # noqa: E402
import logprob_ref  # noqa: E402

ENGINE_CALLS = {"gemma_engine_set_logprobs": "set_logprobs", "gemma_engine_logprobs": "logprobs",
                "gemma_engine_batch_logprobs": "batch_logprobs"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_logprob_calls_are_declared_exported_and_wrapped():
    text = _read("include", "gemma_hpc.h")
    for name, method in ENGINE_CALLS.items():
        assert re.search(r"^int " + name + r"\(gemma_engine \*e", text, flags=re.M), name
        assert name in gemma_hip.EXPORTS, name
        assert callable(getattr(gemma_hip.Engine, method)), method
    assert re.search(r"^int gemma_test_logprob\(const float \*logits, int rows, int n_vocab, const int32_t \*tokens, "
                     r"double \*out\);", text, flags=re.M)
    assert "gemma_test_logprob" in gemma_hip.EXPORTS
    assert callable(gemma_hip.test_logprob) and gemma_hip.test_logprob.__test__ is False


def test_reference_chunk_equals_the_kernels():
    m = re.search(r"^constexpr int LSE_CHUNK = (\d+);", _read("gemma.ggml_amd", "csrc", "kernels.h"), flags=re.M)
    assert m and int(m.group(1)) == logprob_ref.CHUNK
