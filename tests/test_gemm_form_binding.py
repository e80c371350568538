"""CPU: hpc_set_gemm_x4 takes modes 0-4 only.  A mode outside them leaves the exact GEMM's form as it
was and says so in the library's last-error text; the call needs no GPU (it stores one integer), so
the text is checked here.  That the form really stayed: tests/test_gpu_gemm_x4.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip as G  # noqa: E402


@pytest.mark.parametrize("mode", [5, -1, 1 << 20])
def test_a_mode_outside_0_to_4_is_rejected_with_an_error_text(mode):
    L = G.lib()
    try:
        L.hpc_set_gemm_x4(mode)
        err = G.last_error()
        assert "hpc_set_gemm_x4" in err and str(mode) in err and "0..4" in err, err
    finally:
        L.hpc_set_gemm_x4(3)
