"""CPU: the launch front of the decode kernels is what DESIGN.md §5 says it is.  scripts/kernarg_front.py
compiles matvec_rr.hip and the attention translation unit to gfx950 assembly; the default plan's qkv,
attn-out and down matvecs and the per-head attention must get their leading scalars preloaded into
SGPRs, and must not wait for any kernarg load before their first vector memory load."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")

# k_matvec_rr<WT, PRO, EPI, NR, R, DD> of the Gemma-2B default plan (Q4_0 = 2, Q8_0 = 8): qkv PRO_NORM (1),
# attn-out PRO_IMG (4) + EPI_ADD over K 2048 (NR 1 / 2), down the same over K 16384 (NR 8 / 16)
CLASSES = {
    "qkv": r"^k_matvec_rr<(2, 1, 0, 1|8, 1, 0, 2),",
    "attn-out": r"^k_matvec_rr<(2, 4, 1, 1|8, 4, 1, 2),",
    "down": r"^k_matvec_rr<(2, 4, 1, 8|8, 4, 1, 16),",
    "attention": r"^k_attn_head\(",
}


@pytest.fixture(scope="module")
def fronts():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernarg_front
    out = {}
    for src in ("csrc/matvec_rr.hip", "csrc/ops.hip"):
        out.update(kernarg_front.fronts(src))
    return out


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_front_is_preloaded_and_waits_for_no_kernarg_load(fronts, cls):
    hits = {k: v for k, v in fronts.items() if re.match(CLASSES[cls], k)}
    assert hits, f"no kernel of class {cls} in the assembly"
    for name, f in hits.items():
        assert f["first_vload"], f"{name}: no vector load found"
        assert f["preload"] > 0, f"{name}: no kernel argument is preloaded"
        assert not f["waited"], f"{name}: waits for kernarg loads {f['waited']} before {f['first_vload']}"
