"""CPU: the calls of the per-slot sampler (gemma_engine_batch_set_sampler, gemma_engine_batch_sampler,
gemma_engine_batch_fork) and the per-row test entry (gemma_test_sample_rows) are declared in
include/gemma_hpc.h with the prototypes the contract states, listed in the Python binding's EXPORTS
(tests/test_capi_symbols.py then checks the built library exports them) and wrapped: the three batch
calls by Engine, the test entry at module level."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip  # noqa: E402

PROTOTYPES = {
    "gemma_engine_batch_set_sampler": "int gemma_engine_batch_set_sampler(gemma_engine *e, int slot, const gemma_sampler *s);",
    "gemma_engine_batch_sampler": "int gemma_engine_batch_sampler(gemma_engine *e, int slot, gemma_sampler *out, int *own);",
    "gemma_engine_batch_fork": "int gemma_engine_batch_fork(gemma_engine *e, int src, int dst);",
    "gemma_test_sample_rows": ("int gemma_test_sample_rows(const float *logits, int rows, int n_vocab, const gemma_sampler *s_of, "
                               "const int32_t *positions, int32_t *tokens, int32_t *cand, int32_t *n_cand, int32_t *n_kept);"),
}
N_ARGS = {"gemma_engine_batch_set_sampler": 3, "gemma_engine_batch_sampler": 4, "gemma_engine_batch_fork": 3,
          "gemma_test_sample_rows": 9}


def _declarations():
    """the header without comments, one declaration per entry, white space folded"""
    text = open(os.path.join(ROOT, "include", "gemma_hpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return [re.sub(r"\s+", " ", d).strip() + ";" for d in text.split(";")]


def test_the_prototypes_are_declared_verbatim():
    decls = _declarations()
    for name, proto in PROTOTYPES.items():
        assert proto in decls, name


def test_the_calls_are_exported_and_wrapped():
    for name in PROTOTYPES:
        assert name in gemma_hip.EXPORTS, name
    for name in ("batch_set_sampler", "batch_sampler", "batch_fork"):
        assert callable(getattr(gemma_hip.Engine, name)), name
    assert callable(gemma_hip.test_sample_rows)
    assert gemma_hip.test_sample_rows.__test__ is False  # a library wrapper, not a pytest test


def test_the_library_exports_them_with_the_bound_signatures():
    L = gemma_hip.lib()
    for name, n in N_ARGS.items():
        assert len(getattr(L, name).argtypes) == n, name
