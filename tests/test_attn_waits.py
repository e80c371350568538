"""CPU: the product kernel of the per-head decode attention at head_dim 256 (k_attn_head_hd<256, false>,
csrc/ops.hip; the body is attn_head_dev, csrc/attn_impl.h) issues its K / V loads the way the header says it does.
scripts/attn_waits.py compiles ops.hip to gfx950 assembly once and reads the kernel in text order, cut at its
s_barrier instructions (front | KQ | softmax | softmax | KQV):

  * no scratch, at most 128 VGPRs (the 1024-thread workgroup's share);
  * KQ: the K loads of a pass are issued as one group with no s_waitcnt between them: 8 for a later pass, the
    8 - KPF steps past the prefetch for the first; the V steps past the prefetch (8 - VPF) the same way; nothing else
    is loaded there, so no step has a memory round trip of its own;
  * KQV: every group of V loads is 8 loads with no s_waitcnt between them (a whole group of the row, and its last
    group);
  * the softmax loads nothing;
  * no `s_waitcnt vmcnt(0)` lies between the first vector load and the first s_barrier: the RoPE wave and the cache
    append wait by count, with the K / V prefetch in flight;
  * no v_rcp_iflag_f32 (an integer division) anywhere in the kernel;
  * the kernel is a sibling of k_attn_head and is held to tests/test_kernarg_front.py's rule: its leading scalar
    arguments are preloaded and no kernarg load is waited for before the first vector load.
The tapped sibling (the instantiation tests/test_gpu_attn_decode_rows.py runs at head_dim 256) is held to the same
stream rules."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def aw():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import attn_waits
    res = attn_waits.run()
    prod = [a for k, a in res.items() if k.startswith(attn_waits.PRODUCT)]
    tap = [a for k, a in res.items() if k.startswith(attn_waits.TAPPED)]
    assert len(prod) == 1 and len(tap) == 1, sorted(res)
    print(attn_waits.listing(res))
    return attn_waits, prod[0], tap[0]


def test_no_scratch_and_at_most_128_vgprs(aw):
    _, prod, tap = aw
    for a in (prod, tap):
        assert a["scratch"] == 0 and a["vgprs"] <= 128, (a["scratch"], a["vgprs"])


@pytest.mark.parametrize("which", ["product", "tapped"])
def test_k_and_v_loads_come_in_groups(aw, which):
    mod, prod, tap = aw
    a = prod if which == "product" else tap
    kpf, vpf = mod.depths()
    assert a["barriers"] >= 4 and "kq_runs" in a, "the kernel's phases were not found"
    want = sorted(n for n in (8 - kpf, 8, 8 - vpf) if n)  # first pass past the prefetch, a later pass, V past the prefetch
    assert sorted(a["kq_runs"]) == want, f"KQ: load groups {a['kq_runs']}, want {want} (KPF {kpf}, VPF {vpf})"
    assert a["kqv_runs"] and all(n == 8 for n in a["kqv_runs"]), f"KQV: load groups {a['kqv_runs']}, want 8 each"
    assert a["softmax_loads"] == 0
    assert min(a["kq_runs"] + a["kqv_runs"]) > 1, "a load with a round trip of its own"


def test_front_waits_by_count_and_divides_nothing(aw):
    _, prod, tap = aw
    for a in (prod, tap):
        assert a["front_waits"] and min(a["front_waits"]) > 0, f"vmcnt waits before the first barrier: {a['front_waits']}"
        assert a["rcp_iflag"] == 0


def test_product_kernel_is_smaller_than_the_run_time_form(aw):
    """the figures DESIGN.md §5 records; the run-time form's at the parent commit were 2,974 instructions,
    231 conditional branches, 43 vmcnt(0) and 296 v_fma_mix"""
    _, prod, _ = aw
    # 64 per pass or group of 8 steps: the KQ pass, and the compiler's copies of the KQV group (whole / last)
    assert prod["fma_mix"] % 64 == 0 and prod["fma_mix"] < 296, prod["fma_mix"]
    assert prod["instructions"] < 2974 and prod["cond_branches"] < 231 and prod["vmcnt0"] < 43, prod


def test_sibling_launch_front():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import attn_waits
    import kernarg_front
    res = kernarg_front.fronts("csrc/ops.hip")
    for want in (attn_waits.PRODUCT, attn_waits.TAPPED):
        hits = {k: v for k, v in res.items() if k.startswith(want)}
        assert len(hits) == 1, (want, sorted(res))
        v = next(iter(hits.values()))
        assert v["preload"] >= 13, f"{want}: kernarg preload of {v['preload']} dwords"
        assert not v["waited"], f"{want}: waits for {v['waited']} before its first vector load ({v['first_vload']})"
