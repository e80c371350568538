"""CPU: the wide batch's two calls (gemma_engine_batch_open_wide, gemma_engine_batch_last_n) are declared
in include/gemma_hpc.h, listed in the Python binding's EXPORTS (tests/test_capi_symbols.py then checks
the built library exports them) and wrapped by Engine; the binding's wide slot bound equals the header's."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip  # noqa: E402

CALLS = ("open_wide", "last_n")


def _header():
    return open(os.path.join(ROOT, "include", "gemma_hpc.h")).read()


def test_the_wide_calls_are_declared_exported_and_wrapped():
    text = _header()
    for c in CALLS:
        name = "gemma_engine_batch_" + c
        assert re.search(r"^int " + name + r"\(gemma_engine \*e", text, flags=re.M), name
        assert name in gemma_hip.EXPORTS, name
        assert callable(getattr(gemma_hip.Engine, "batch_" + c)), c


def test_wide_slot_bound_equals_the_headers():
    m = re.search(r"^#define GEMMA_BATCH_WIDE_MAX_SLOTS (\d+)", _header(), flags=re.M)
    assert m and gemma_hip.BATCH_WIDE_MAX_SLOTS == int(m.group(1)) == 64
