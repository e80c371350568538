"""GPU: the context shift's cache kernels alone (csrc/kv_shift.hip through gemma_test_kv_shift), bit for bit, whole images.

The reference is numpy on the input images, the rule of include/gemma_hpc.h (gemma_engine_shift) with orc_rope_cos_sin's
row of position `discard`; numpy's f16 conversion is the oracle's (one row is held to orc_fp32_to_fp16 in every case).
The K kernel walks windows of 512 rows, the V kernel windows of 2,048 elements from the 16-byte word that holds `keep`:
moved spans of 0, 1, a window +- 1 and three windows + 1 of each, beside every alignment class of `discard` (1, 7, 8, 9,
32, 33) and `keep` (0, 1, 31, 32), overlapping and disjoint moves, and pos = n_ctx - 1."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O

pytestmark = pytest.mark.gpu

# (n_ctx, pos, keep, discard); moved span = pos - keep - discard
CASES = [(256, 255, 0, 1), (256, 40, 31, 9), (256, 41, 32, 8), (256, 200, 1, 7), (256, 255, 31, 33), (256, 100, 0, 64),
         (4096, 575, 32, 32), (4096, 522, 1, 9), (4096, 520, 0, 7), (4096, 1601, 31, 33), (4096, 2048, 0, 1),
         (4096, 2088, 32, 8), (4096, 2083, 1, 33), (4096, 4095, 0, 2048)]
PARAMS = [c + s for c in CASES for s in ((1, 256), (2, 64), (4, 128))] + [(8192, 6185, 31, 9, 1, 256)]


def shift_rule(kc, vc, pos, keep, d, Hkv, hd, rope_base=10000.0):
    """gemma_engine_shift's rule on one layer's images kc [ctx][Hkv*hd], vc [Hkv*hd][ctx] (f16 bits) -> new images"""
    half, n = hd // 2, pos - d
    c, s = np.zeros(half, np.float32), np.zeros(half, np.float32)
    O.lib().orc_rope_cos_sin(d, hd, rope_base, O.ptr(c), O.ptr(s))
    k, v = kc.copy(), vc.copy()
    x = kc[keep + d:pos].view(np.float16).astype(np.float32).reshape(-1, Hkv, hd)
    x0, x1 = x[..., :half], x[..., half:]
    with np.errstate(over="ignore"):  # +-65504 rotated past the f16 range rounds to inf, as the K store rounds it
        out = np.concatenate([x0 * c + x1 * s, x1 * c - x0 * s], axis=-1).reshape(-1, Hkv * hd)
        k[keep:n] = out.astype(np.float16).view(np.uint16)
    if n > keep:
        assert np.array_equal(k[keep], O.fp32_to_fp16_bits(out[0]))
    v[:, keep:n] = vc[:, keep + d:pos]
    k[n:pos], v[:, n:pos] = 0, 0
    return k, v


def _images(ctx, pos, keep, d, kvw, seed):
    """a recognisable fill everywhere, random finite f16 with +-0, denormals and +-65504 on the moved span"""
    rng = np.random.default_rng(seed)
    kc = (0x3000 + np.arange(ctx * kvw, dtype=np.int64) % 1021).astype(np.uint16).reshape(ctx, kvw)
    vc = (0x3400 + np.arange(ctx * kvw, dtype=np.int64) % 1019).astype(np.uint16).reshape(kvw, ctx)
    m = pos - keep - d
    r = rng.integers(0, 1 << 16, size=(2, m, kvw), dtype=np.uint16)
    r[(r & 0x7C00) == 0x7C00] ^= 0x0400  # no inf / NaN
    special = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x7BFF, 0xFBFF], np.uint16)
    pick = rng.random(r.shape) < 0.05
    r[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    kc[keep + d:pos] = r[0]
    vc[:, keep + d:pos] = r[1].T
    return kc, vc


@pytest.mark.parametrize("ctx,pos,keep,d,Hkv,hd", PARAMS)
def test_shifted_images_equal_the_rule_in_every_word(ctx, pos, keep, d, Hkv, hd):
    kc, vc = _images(ctx, pos, keep, d, Hkv * hd, seed=pos * 64 + d)
    k_ref, v_ref = shift_rule(kc, vc, pos, keep, d, Hkv, hd)
    k, v = kc.copy(), vc.copy()
    G.test_kv_shift(k, v, pos, keep, d, Hkv, hd)
    for name, bad in (("K [position, element]", np.argwhere(k != k_ref)), ("V [element, position]", np.argwhere(v != v_ref))):
        assert not len(bad), (name, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("pos,keep,d", [(100, 60, 41), (100, -1, 8), (100, 0, 0), (256, 0, 8)])
def test_refusals_leave_both_images_as_given(pos, keep, d):
    kc, vc = _images(256, 100, 0, 8, 256, seed=1)
    k, v = kc.copy(), vc.copy()
    with pytest.raises(RuntimeError, match="kv_shift"):
        G.test_kv_shift(k, v, pos, keep, d, 1, 256)
    assert np.array_equal(k, kc) and np.array_equal(v, vc)
