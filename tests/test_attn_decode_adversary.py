"""CPU: the decode attention's oracle with a given RoPE row (orc_attn_decode_row) is the oracle already trusted,
the single-row inputs of attn_adversary.decode_case are what they claim, and a wrong accumulation of the kind
a one-row kernel can commit is visible where tests/test_gpu_attn_decode_rows.py looks for it.

Two wrong accumulations (attn_adversary.chain_dot): FOLD adds the four 8-wide accumulator rows (a0 + a1) +
(a2 + a3) where ggml_vec_dot_f16 adds (a0 + a2) + (a1 + a3) (a quad fold taking xor-1 before xor-2); REV runs
the steps of every chain last to first.

Measured (H 4, Hkv 2, ctx 320, seed 0, single rows at the 29 positions 3, 14, .. 311; shares of 32-bit words
that differ from the fmaf chain in K order):
                               head_dim 256                    head_dim 128
  wrong KQ, score words j <= pos (pooled over the rows)
    benign      FOLD / REV     0.523 / 0.660                   0.510 / 0.430
    cancel_kq   FOLD / REV     0.509 / 1.000                   0.499 / 0.999
    underflow   FOLD / REV     0.371 / 0.544                   0.366 / 0.341
  wrong KQ, output words (pooled)
    benign      FOLD / REV     0.0086 / 0                      0 / 0
    underflow   FOLD / REV     0.0086 / 0.0171                 0 / 0.0086
    cancel_kq   FOLD           0.0085                          0.0257
    cancel_kq   REV, each row at pos >= 31: 1.000 .. 1.000     1.000 .. 1.000
  wrong KQV on cancel_kqv, output words of each row
    REV,  pos >= 255           0.995 .. 1.000                  0.996 .. 1.000
    FOLD, pos >= 31            0.231 .. 0.471                  0.248 .. 0.510
So on N(0,1) inputs half of the scores may be wrong by an ulp with (almost) no output word changed: a 1-ulp
change in a score does not survive f16(w - max).  Only a comparison of the score words sees a wrong fold;
a wrong step order is also visible in the outputs of cancel_kq rows.  The floors asserted below sit under
the smallest measured value of their row of the table (0.25 under underflow's 0.37).  head_dim 64 has two
steps per chain, whose sum commutes: it cannot tell a step order."""
import functools

import numpy as np
import pytest

import attn_adversary as A
import oracle_ctypes as O

H, HKV, CTX = 4, 2, 320
U32 = np.uint32
POSITIONS = [0, 1, 31, 32, 63, 255, 256, 319]
ROWS = list(range(3, 320, 11))  # the 29 single rows of the discrimination claims


@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("pos", POSITIONS)
def test_decode_row_is_attn_decode(pos, hd):
    """given orc_rope_cos_sin's row and 1/sqrtf(hd), orc_attn_decode_row == orc_attn_decode bit for bit:
    output, both caches, scores and P16"""
    rng = np.random.default_rng([pos, hd])
    kvw = HKV * hd
    qkv = (rng.standard_normal((H + 2 * HKV) * hd) * 2.0).astype(np.float32)
    kc = np.zeros((CTX, kvw), np.uint16)
    vc = np.zeros((kvw, CTX), np.uint16)
    kc[:pos] = rng.standard_normal((pos, kvw)).astype(np.float16).view(np.uint16)
    vc[:, :pos] = rng.standard_normal((kvw, pos)).astype(np.float16).view(np.uint16)
    k1, v1, k2, v2 = kc.copy(), vc.copy(), kc.copy(), vc.copy()
    ref = np.zeros(H * hd, np.float32)
    w1, p1 = np.zeros((H, CTX), np.float32), np.zeros((H, CTX), np.uint16)
    O.lib().orc_attn_decode(O.ptr(qkv), O.ptr(k1), O.ptr(v1), pos, H, HKV, hd, CTX, 10000.0, O.ptr(ref), O.ptr(w1), O.ptr(p1), None)
    row = np.concatenate(A.rope_tables(pos, hd))
    q_scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    got, w2, p2 = O.attn_decode_row(qkv, k2, v2, pos, H, HKV, hd, CTX, row, q_scale)
    assert np.array_equal(got.view(U32), ref.view(U32))
    assert np.array_equal(k1, k2) and np.array_equal(v1, v2)
    assert np.array_equal(w1.view(U32), w2.view(U32)) and np.array_equal(p1, p2)
    n_kv = O.attn_n_kv(pos, CTX)
    assert np.isfinite(w2[:, :pos + 1]).all() and np.isneginf(w2[:, pos + 1:n_kv]).all() and p2[:, :n_kv].any()


@functools.lru_cache(maxsize=None)
def _row(name, pos, hd, Hh=H):
    """a decode_case, the oracle's results on it, and the case with the caches as the oracle left them"""
    cs = A.decode_case(name, pos, Hh, HKV, hd, CTX)
    ref, w, p, kc, vc = A.decode_oracle(cs)
    ref.setflags(write=False)
    return cs, ref, w, p, dict(cs, kc=kc, vc=vc)


@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("name", A.CASES)
def test_decode_case_under_the_identity_row_is_attn_rows(name, hd):
    """identity RoPE row, q_scale 1: the stored K row / V column are the row's own f16 words (not the garbage
    the cache held there), every other cache word is unchanged, and orc_attn_decode_row == orc_attn_rows at
    T = 1 on the caches it leaves; stale keeps garbage past pos, every other case zeros"""
    for pos in POSITIONS:
        cs, ref, _, _, after = _row(name, pos, hd)
        kvw = HKV * hd
        k_row, v_col = (A._bits(cs["qkv"][H * hd + i * kvw:H * hd + (i + 1) * kvw]) for i in (0, 1))
        # (a zero's sign follows x0 * 1 - x1 * 0, on the kernel's side as on the oracle's: compared as a value)
        same_k = (after["kc"][pos] == k_row) | (((after["kc"][pos] | k_row) & 0x7FFF) == 0)
        assert same_k.all() and np.array_equal(after["vc"][:, pos], v_col)
        for held in (cs["kc"][pos], cs["vc"][:, pos]):  # finite, non-zero, and not what the row stores
            assert ((held & 0x7FFF) != 0).all() and ((held & 0x7C00) != 0x7C00).all()
        assert (cs["kc"][pos] != k_row).mean() > 0.99 and (cs["vc"][:, pos] != v_col).mean() > 0.99
        other = np.arange(CTX) != pos
        assert np.array_equal(after["kc"][other], cs["kc"][other]) and np.array_equal(after["vc"][:, other], cs["vc"][:, other])
        past = cs["kc"][pos + 1:]
        assert ((past & 0x7FFF) != 0).all() if name == "stale" else not past.any()
        assert np.array_equal(A._bits(cs["qkv"][:H * hd]).reshape(1, H, hd), cs["q16"])
        got = O.attn_rows(cs["q16"], after["kc"], after["vc"], 1, pos, H, HKV, hd, CTX)
        assert np.array_equal(got.ravel().view(U32), ref.view(U32)), (name, pos)


def test_decode_case_zero_v_block_and_underflow_rows():
    """zero_v: the kv head's outputs are exactly zero on those dims (an image block with d == 0).  underflow
    with 8 heads: single rows hold subnormal and underflowed P, a single survivor and two tied maxima."""
    cs = A.decode_case("benign", 63, H, HKV, 64, CTX, zero_v=(1, 32, 32))
    out = A.decode_oracle(cs)[0].reshape(H, 64)
    assert not out[2:, 32:].any() and out[2:, :32].all() and out[:2].all()
    sub = zero = single = tie = 0
    for pos in (255, 256, 319):
        _, _, w, p, _ = _row("underflow", pos, 256, 8)
        for h in range(8):
            pv, wv = p[h, :pos + 1], w[h, :pos + 1]
            sub += bool((((pv & 0x7C00) == 0) & (pv != 0)).any())
            zero += bool((pv == 0).any())
            single += int((pv != 0).sum() == 1)
            tie += int((wv == wv.max()).sum() >= 2)
    assert sub >= 6 and zero >= 12 and single >= 3 and tie >= 12, (sub, zero, single, tie)


def _shares(name, pos, hd, kq, kqv):
    """(share of the score words j <= pos, share of the output words) that differ from the fmaf chain in K
    order; H1 must be the oracle itself"""
    _, ref, w, _, after = _row(name, pos, hd)
    out, _, W = A.attn_emulated(after, kq, kqv)
    if (kq, kqv) == ("H1", "H1"):
        assert np.array_equal(out.ravel().view(U32), ref.view(U32))
        assert all(np.array_equal(W[0, h][:pos + 1].view(U32), w[h, :pos + 1].view(U32)) for h in range(H))
    ws = np.concatenate([W[0, h][:pos + 1].view(U32) != w[h, :pos + 1].view(U32) for h in range(H)])
    return ws, out.ravel().view(U32) != ref.view(U32)


@pytest.mark.parametrize("hd", [256, 128])
@pytest.mark.parametrize("name", ["benign", "cancel_kq", "cancel_kqv", "underflow"])
def test_emulated_chain_is_the_decode_oracle(name, hd):
    for pos in ROWS[::4]:
        ws, os_ = _shares(name, pos, hd, "H1", "H1")
        assert not ws.any() and not os_.any()


@pytest.mark.parametrize("hd", [256, 128])
def test_wrong_fold_in_kq_moves_the_scores_and_not_the_outputs(hd):
    """benign single rows: FOLD changes a quarter of the score words or more and under 1 % of the output
    words: an output-only comparison cannot pin the fold, a score comparison does"""
    parts = [_shares("benign", pos, hd, "FOLD", "H1") for pos in ROWS]
    score = float(np.concatenate([p[0] for p in parts]).mean())
    outs = float(np.concatenate([p[1] for p in parts]).mean())
    print(f"benign hd {hd} FOLD in KQ: {score:.4f} of the score words, {outs:.4f} of the output words differ")
    assert score >= 0.25 and outs < 0.01


@pytest.mark.parametrize("hd", [256, 128])
def test_reversed_steps_in_kq_change_cancel_kq_outputs(hd):
    shares = [float(_shares("cancel_kq", pos, hd, "REV", "H1")[1].mean()) for pos in ROWS if pos >= 31]
    print(f"cancel_kq hd {hd} REV in KQ: {min(shares):.4f} .. {max(shares):.4f} of a row's output words differ")
    assert min(shares) >= 0.5


@pytest.mark.parametrize("hd", [256, 128])
def test_wrong_kqv_accumulation_changes_cancel_kqv_outputs(hd):
    rev = [float(_shares("cancel_kqv", pos, hd, "H1", "REV")[1].mean()) for pos in ROWS if pos >= 255]
    fold = [float(_shares("cancel_kqv", pos, hd, "H1", "FOLD")[1].mean()) for pos in ROWS if pos >= 31]
    print(f"cancel_kqv hd {hd} in KQV: REV {min(rev):.4f} .. {max(rev):.4f}, FOLD {min(fold):.4f} .. {max(fold):.4f}")
    assert min(rev) >= 0.5 and min(fold) >= 0.1
