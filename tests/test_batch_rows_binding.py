"""CPU: the three calls of a batch pass with several rows per slot (gemma_batch_plan_rows,
gemma_engine_batch_open_rows, gemma_engine_batch_step_rows) are declared in include/gemma_hpc.h,
listed in the Python binding's EXPORTS (tests/test_capi_symbols.py then checks the built library
exports them) and wrapped by Engine; and gemma_batch_plan_rows, a host function, gives the allotment
the header states, restated here in Python, on hand-made cases and with every refusal."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip  # noqa: E402


def _header():
    return open(os.path.join(ROOT, "include", "gemma_hpc.h")).read()


def test_the_calls_are_declared_exported_and_wrapped():
    text = _header()
    assert re.search(r"^int gemma_batch_plan_rows\(const int32_t \*need, int n_slots, int max_rows, int32_t \*rows_of\);",
                     text, flags=re.M)
    assert re.search(r"^int gemma_engine_batch_open_rows\(gemma_engine \*e, int n_slots, int max_rows\);", text, flags=re.M)
    assert re.search(r"^int gemma_engine_batch_step_rows\(gemma_engine \*e, int max_rows, float \*logits, int32_t \*rows_of\);",
                     text, flags=re.M)
    for name in ("gemma_batch_plan_rows", "gemma_engine_batch_open_rows", "gemma_engine_batch_step_rows"):
        assert name in gemma_hip.EXPORTS, name
    assert callable(gemma_hip.Engine.batch_open_rows) and callable(gemma_hip.Engine.batch_step_rows)
    assert callable(gemma_hip.batch_plan_rows)


def _rule(need, max_rows):
    """the header's rule: every active slot one row, the rest of the budget in ascending slot order"""
    R = sum(1 for n in need if n > 0)
    budget = max_rows - R
    out = []
    for n in need:
        extra = min(budget, n - 1) if n > 0 else 0
        budget -= extra
        out.append((1 + extra) if n > 0 else 0)
    return out


CASES = [
    ("the first hungry slot exhausts the budget", [100, 50, 1], 8, [6, 1, 1]),
    ("an inactive slot between active ones", [1, 0, 20, 0, 3], 8, [1, 0, 6, 0, 1]),
    ("need 1 everywhere: batch_step's R rows", [1, 1, 0, 1], 64, [1, 1, 0, 1]),
    ("max_rows = R", [9, 4, 7], 3, [1, 1, 1]),
    ("the budget outlasts the first slot", [3, 20, 5], 16, [3, 12, 1]),
    ("more budget than need", [3, 2, 0, 4], 64, [3, 2, 0, 4]),
    ("one slot, a whole wide pass", [128], 64, [64]),
    ("64 slots, one hungry at the end", [1] * 63 + [9], 64, [1] * 64),
]


@pytest.mark.parametrize("what,need,max_rows,want", CASES, ids=[c[0] for c in CASES])
def test_plan_rows_follows_the_rule(what, need, max_rows, want):
    assert _rule(need, max_rows) == want, "the test's own restatement"
    got = gemma_hip.batch_plan_rows(need, max_rows)
    assert list(got) == want
    out = np.full(len(need) + 1, -7, dtype=np.int32)
    a = np.ascontiguousarray(need, dtype=np.int32)
    T = gemma_hip.lib().gemma_batch_plan_rows(gemma_hip._p(a), len(a), max_rows, gemma_hip._p(out))
    assert T == sum(want) and out[-1] == -7  # returns the sum; writes n_slots entries only


def test_plan_rows_refusals():
    L, p = gemma_hip.lib(), gemma_hip._p
    out = np.zeros(80, dtype=np.int32)

    def refused(need, n, max_rows):
        a = np.ascontiguousarray(need, dtype=np.int32)
        r = L.gemma_batch_plan_rows(p(a), n, max_rows, p(out))
        assert r == -1 and "gemma_batch_plan_rows" in gemma_hip.last_error(), (need, n, max_rows, r)

    refused([1], 0, 8)             # n_slots outside [1, 64]
    refused([1] * 65, 65, 64)
    refused([1, -1, 2], 3, 8)      # a negative need
    refused([0, 0, 0], 3, 8)       # no active slot
    refused([5, 5, 5], 3, 2)       # max_rows below R
    refused([5, 5, 5], 3, 65)      # max_rows above 64
    refused([5, 5, 5], 3, 0)
    with pytest.raises(ValueError):
        gemma_hip.batch_plan_rows([0, 0], 8)
    assert list(gemma_hip.batch_plan_rows([5, 5, 5], 3)) == [1, 1, 1]  # and a valid call after them
