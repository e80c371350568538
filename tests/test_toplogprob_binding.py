"""CPU: the four top-logprob calls are declared in include/gemma_hpc.h, listed in the Python binding's
EXPORTS (tests/test_capi_symbols.py then checks the built library exports them) and wrapped; the limit
is the same on every side."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip  # noqa: E402

DECLS = {
    "gemma_engine_set_top_logprobs": (r"gemma_engine \*e, int n", "set_top_logprobs"),
    "gemma_engine_top_logprobs": (r"gemma_engine \*e, int p0, int cnt, int32_t \*tokens, double \*lps", "top_logprobs"),
    "gemma_engine_batch_top_logprobs": (r"gemma_engine \*e, int slot, int p0, int cnt, int32_t \*tokens, double \*lps",
                                        "batch_top_logprobs"),
    "gemma_test_top_logprobs": (r"const float \*logits, int rows, int n_vocab, int n, int32_t \*tokens, double \*lps", None),
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_calls_are_declared_exported_and_wrapped():
    text = _read("include", "gemma_hpc.h")
    for name, (args, method) in DECLS.items():
        assert re.search(r"^int " + name + r"\(" + args + r"\);", text, flags=re.M), name
        assert name in gemma_hip.EXPORTS, name
        assert method is None or callable(getattr(gemma_hip.Engine, method)), method
    assert callable(gemma_hip.test_top_logprobs) and gemma_hip.test_top_logprobs.__test__ is False
    limit = int(re.search(r"^#define GEMMA_TOP_LOGPROBS_MAX (\d+)$", text, flags=re.M).group(1))
    kernels = _read("gemma.ggml_amd", "csrc", "kernels.h")
    assert limit == gemma_hip.TOP_LOGPROBS_MAX == int(re.search(r"^constexpr int TOPN_MAX = (\d+);", kernels, flags=re.M).group(1))
