"""CPU: the weight ring of the round-pipelined matvecs waits the way csrc/matvec_rr.hip says it does.
scripts/rr_waits.py compiles matvec_rr.hip to gfx950 assembly once and walks the loader path and the carrier path
of EVERY k_matvec_rr instantiation (72):

  * no kernel has scratch;
  * loaders and carrier pass the same number of s_barrier (a mismatch hangs the workgroup), at least one per
    round and one in front of the rounds;
  * a ring that is refilled (D < NR: the down kernels of every plan) runs on split paths — no barrier sits in a
    block both kinds of wave run, which is what keeps the counts exact — and every round that is followed by a
    refill waits with the steady-state count (the loads of the D - 1 later rounds stay in flight), the last D
    rounds counting down to 0: no drain while refills are in flight;
  * a kernel that ships with E > 0 rounds in front of the activation image issues its first ring load before
    the image's first LDS store, and waits for the activation with those rounds still counted;
  * the kernels of the decode plans (the engine's default and the bench's tuned one) are among those walked."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def rr():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import rr_waits
    res = rr_waits.run(show_all=True)
    assert len(res) == 72, f"{len(res)} k_matvec_rr kernels walked, 2 types x 6 (prologue, epilogue) pairs x 6 NR expected"
    return rr_waits, res


def test_no_kernel_has_scratch(rr):
    _, res = rr
    bad = {k[:40]: a["scratch"] for k, a in res.items() if a["scratch"] != 0}
    assert not bad, f"private segment in {bad}"


def test_loaders_and_carrier_pass_the_same_barriers(rr):
    _, res = rr
    for name, a in res.items():
        assert "rounds" in a, f"{name}: the rounds' barriers were not found on the loader path"
        b = a["barriers"]
        assert b["loader"] == b["carrier"], f"{name}: {b}"
        assert b["loader"] >= a["nr"] + 1, f"{name}: {b} for {a['nr']} rounds"


def test_refilled_rings_run_split_and_wait_with_the_steady_state_counts(rr):
    mod, res = rr
    refilled = {k: a for k, a in res.items() if a["nr"] > a["d"]}
    assert len(refilled) == 12, sorted(refilled)  # (PRO_F32 | PRO_IMG) + EPI_ADD, NR 8 / 12 / 16, both types
    for name, a in refilled.items():
        assert a["split"], f"{name}: a barrier sits in a block that loaders and the carrier both run"
        assert len(a["rounds"]) == a["nr"] and a["lpr"] == 2
        assert not mod.steady(a), f"{name}: " + "; ".join(mod.steady(a))


def test_front_rounds_precede_the_image_and_stay_counted(rr):
    _, res = rr
    front = {k: a for k, a in res.items() if a["e"] > 0}
    assert front, "no kernel ships with rounds in front of the image"
    for name, a in front.items():
        assert a["nr"] > a["d"], f"{name}: rounds in front of the image outside the split form"
        assert a["ring_first"], f"{name}: E = {a['e']}, but the image's first LDS store precedes the ring"
        assert a["front"] and min(a["front"]) >= a["lpr"] * a["e"], f"{name}: the front's waits {a['front']} drain the E rounds"


def test_the_plans_kernels_are_walked(rr):
    mod, res = rr
    for cls, pat in mod.PLAN.items():
        hits = [k for k in res if re.match(pat, k)]
        assert hits, f"no kernel of class {cls} in the assembly"
        if cls.startswith("down"):
            assert all(res[k]["nr"] > res[k]["d"] for k in hits), f"{cls}: not a refilled ring"
