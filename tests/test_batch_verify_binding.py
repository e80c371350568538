"""CPU: the two calls of speculative decoding in the batch (gemma_engine_batch_verify,
gemma_engine_batch_generate_lookup) are declared in include/gemma_hpc.h with the prototypes the
contract states, listed in the Python binding's EXPORTS (tests/test_capi_symbols.py then checks the
built library exports them) and wrapped by Engine."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip  # noqa: E402

VERIFY = ("int gemma_engine_batch_verify(gemma_engine *e, const int32_t *draft, const int32_t *k_of, "
          "int32_t *out_tokens, int32_t *n_out, float *logits);")
GENERATE = ("int gemma_engine_batch_generate_lookup(gemma_engine *e, int n_new, int k, int ngram_max, "
            "int32_t *out, gemma_spec_stats *stats);")


def _declarations():
    """the header without comments, one declaration per entry, white space folded"""
    text = open(os.path.join(ROOT, "include", "gemma_hpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return [re.sub(r"\s+", " ", d).strip() + ";" for d in text.split(";")]


def test_the_prototypes_are_declared_verbatim():
    decls = _declarations()
    assert VERIFY in decls
    assert GENERATE in decls


def test_the_calls_are_exported_and_wrapped():
    for name in ("gemma_engine_batch_verify", "gemma_engine_batch_generate_lookup"):
        assert name in gemma_hip.EXPORTS, name
    assert callable(gemma_hip.Engine.batch_verify) and callable(gemma_hip.Engine.batch_generate_lookup)


def test_the_library_exports_them_with_the_bound_signatures():
    L = gemma_hip.lib()
    assert len(L.gemma_engine_batch_verify.argtypes) == 6
    assert len(L.gemma_engine_batch_generate_lookup.argtypes) == 6
