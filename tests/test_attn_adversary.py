"""CPU: the prefill attention's adversarial inputs (tests/attn_adversary.py) are what they claim, and the
oracle's prefill functions agree with the decode one already trusted.

The floors below come from the generator's construction, not from a kernel: cancel_kq puts a big
cancelling pair in BIG_SHARE = 1/2 of the (key, pattern) pairs, underflow gives 2 of every 4 (row, head)
a gain that spreads the scores past the f16 exp table's subnormal range, 1 of 8 a single survivor and
every other group of 4 the tie multiplier."""
import functools

import numpy as np
import pytest

import attn_adversary as A
import oracle_ctypes as O

H, HKV, HD, CTX = 4, 2, 256, 320
U32 = np.uint32


@functools.lru_cache(maxsize=None)
def _case(name, p0, T, hd=HD):
    cs = A.make(name, T, p0, H, HKV, hd, CTX)
    ref = A.oracle_out(cs)
    ref.setflags(write=False)
    return cs, ref


@functools.lru_cache(maxsize=None)
def _emulated(name, p0, T, kq="H1", kqv="H1"):
    return A.attn_emulated(_case(name, p0, T)[0], kq, kqv)


def _share(a, b):
    return float((a.view(U32) != b.view(U32)).mean())


@pytest.mark.parametrize("pos", [0, 1, 30, 31, 32, 63, 64, 200, 318, 319])
def test_attn_rows_is_attn_decode_at_one_row(pos):
    """orc_rope_kv_rows + orc_attn_rows at T = 1, p0 = pos == orc_attn_decode, bit for bit: output,
    K row and V column."""
    Hh, Hk, hd, ctx = 4, 2, 256, 320
    rng = np.random.default_rng(pos)
    kvw = Hk * hd
    qkv = (rng.standard_normal((1, (Hh + 2 * Hk) * hd)) * 2.0).astype(np.float32)
    kc = np.zeros((ctx, kvw), np.uint16)
    vc = np.zeros((kvw, ctx), np.uint16)
    kc[:pos] = rng.standard_normal((pos, kvw)).astype(np.float16).view(np.uint16)
    vc[:, :pos] = rng.standard_normal((kvw, pos)).astype(np.float16).view(np.uint16)
    k1, v1, k2, v2 = kc.copy(), vc.copy(), kc.copy(), vc.copy()
    ref = np.zeros(Hh * hd, np.float32)
    O.lib().orc_attn_decode(O.ptr(qkv), O.ptr(k1), O.ptr(v1), pos, Hh, Hk, hd, ctx, 10000.0, O.ptr(ref), None, None, None)
    q16 = np.zeros((1, Hh, hd), np.uint16)
    O.rope_kv_rows(qkv, 1, pos, Hh, Hk, hd, ctx, q16, k2, v2)
    assert np.array_equal(k1, k2) and np.array_equal(v1, v2)
    got = O.attn_rows(q16, k2, v2, 1, pos, Hh, Hk, hd, ctx)
    assert np.array_equal(got.ravel().view(U32), ref.view(U32))


def test_attn_rows_leaves_padding_columns_and_later_rows_alone():
    cs, ref = _case("benign", 27, 6)
    ldo = H * HD + 24
    out = np.full((6, ldo), -7.5, np.float32)
    A.oracle_out(cs, ldo, out)
    assert np.array_equal(out[:, :H * HD].view(U32), ref.view(U32)) and (out[:, H * HD:] == -7.5).all()


GEOMS = [(0, 1), (0, 33), (5, 40), (27, 6), (250, 38), (282, 38)]


@pytest.mark.parametrize("name", A.CASES)
def test_cases_are_finite_seeded_and_causal(name):
    for p0, T in GEOMS:
        cs, ref = _case(name, p0, T)
        assert np.isfinite(ref).all(), (name, p0, T)
        again = A.make(name, T, p0, H, HKV, HD, CTX)
        assert all(np.array_equal(cs[k], again[k]) for k in ("q16", "kc", "vc"))
        n = p0 + T
        past_k, past_v = cs["kc"][n:], cs["vc"][:, n:]
        if name == "stale":  # finite, non-zero garbage at every position past the last row
            assert ((past_k & 0x7FFF) != 0).all() and ((past_k & 0x7C00) != 0x7C00).all()
            assert ((past_v & 0x7FFF) != 0).all() and ((past_v & 0x7C00) != 0x7C00).all()
            clean = dict(cs, kc=cs["kc"].copy(), vc=cs["vc"].copy())
            clean["kc"][n:] = 0
            clean["vc"][:, n:] = 0
            assert np.array_equal(A.oracle_out(clean).view(U32), ref.view(U32))  # P = 0 there: no effect
        else:
            assert not past_k.any() and not past_v.any()


@pytest.mark.parametrize("name,p0,T", [("cancel_kq", 250, 38), ("cancel_kq", 5, 40), ("cancel_kqv", 250, 38),
                                       ("underflow", 250, 38), ("benign", 27, 6), ("stale", 27, 6)])
def test_emulated_fmaf_chain_is_the_oracle(name, p0, T):
    """H1 (fmaf chains in K order, groups of 4 steps from the accumulator) == orc_attn_rows bit for bit:
    the emulator the discrimination tests vary is the oracle's arithmetic."""
    out, _, _ = _emulated(name, p0, T)
    assert np.array_equal(out.view(U32), _case(name, p0, T)[1].view(U32))


def _f32_ulp(x):
    return np.exp2(np.floor(np.log2(np.abs(x))) - 23)


@pytest.mark.parametrize("p0,T", [(250, 38), (5, 40)])
def test_cancel_kq_features(p0, T):
    cs, _ = _case("cancel_kq", p0, T)
    _, P, W = _emulated("cancel_kq", p0, T)
    q = cs["q16"].view(np.float16).astype(np.float64)
    k = cs["kc"].view(np.float16).astype(np.float64).reshape(CTX, HKV, HD)
    G = H // HKV
    big_pairs = absorbed = pairs = 0
    for t in range(T):
        n = p0 + t + 1
        for h in range(H):
            any_big = np.zeros(n, bool)
            any_abs = np.zeros(n, bool)
            for c, terms, mid in A.PATTERNS:
                prods = [q[t, h, 32 * s + c] * k[:n, h // G, 32 * s + c] for s, _ in terms]
                assert not np.any(sum(prods)), "the pattern's products cancel exactly"
                B = np.max(np.abs(prods), axis=0)  # the largest term (the -2 x of a three-term pattern)
                big = (B >= 2.0 ** 18) & (B < 2.0 ** 22)
                assert (B < 2.0 ** 22).all() and ((B >= 2.0 ** 18) | (B < 2.0 ** 13)).all()
                any_big |= big
                if mid is not None:
                    tm = np.abs(q[t, h, 32 * mid + c] * k[:n, h // G, 32 * mid + c])
                    u = _f32_ulp(B)
                    any_abs |= big & (tm >= u / 8) & (tm <= u)  # partly absorbed, or a tie, at that partial sum
            big_pairs += any_big.sum()
            absorbed += any_abs.sum()
            pairs += n
    # 8 patterns at 1/2 each: 1 - 2^-8 of the (row, key) pairs hold a big chain; 5 have a middle term
    assert big_pairs >= 0.95 * pairs and absorbed >= 0.9 * pairs, (big_pairs, absorbed, pairs)
    w = np.concatenate([x[np.isfinite(x)] for x in W.values()])
    assert np.abs(w).max() <= 14.0  # "within about +-12"
    assert np.median([len(np.unique(p)) for p in P.values()]) >= min(24, p0 + T // 2)


def test_cancel_kqv_features():
    cs, _ = _case("cancel_kqv", 250, 38)
    _, P, _ = _emulated("cancel_kqv", 250, 38)
    v = cs["vc"].view(np.float16).astype(np.float64).reshape(HKV, HD, CTX)
    kc = cs["kc"]
    n_pair = 0
    for b0, b1 in A.DUP_BLOCKS:
        j0, j1 = slice(32 * b0, 32 * b0 + 32), slice(32 * b1, 32 * b1 + 32)
        assert np.array_equal(kc[j0], kc[j1])
        for (t, _), p in P.items():
            vis = 32 * b1 + np.arange(32) <= 250 + t  # the later key of the pair is unmasked
            assert np.array_equal(p[j0][vis], p[j1][vis]) and p[j0][vis].any()  # equal P in the same chains
        s = v[:, :, j0] + v[:, :, j1]
        pair = (np.abs(v[:, :, j0]) >= 64) & (np.abs(s) <= np.abs(v[:, :, j0]) * 2.0 ** -7) & (s != 0)
        n_pair += pair.sum()
        assert np.abs(v[:, :, j0]).max() < 2.0 ** 14
    assert n_pair >= 0.45 * 3 * 32 * HKV * HD  # V_SHARE = 1/2 of the duplicated (dim, key) pairs


def test_underflow_features():
    p0, T = 250, 38
    _, P, W = _emulated("underflow", p0, T)
    rows = len(P)
    sub = zero = all3 = tie = single = 0
    for (t, h), p in P.items():
        pv = p[:p0 + t + 1]  # the unmasked keys
        s = ((pv & 0x7C00) == 0) & (pv != 0)
        z = pv == 0  # exp underflow, not the mask
        nrm = (pv & 0x7C00) != 0
        w = W[t, h][:p0 + t + 1]
        sub += s.any()
        zero += z.any()
        all3 += s.any() and z.any() and nrm.sum() >= 3
        tie += (w == w.max()).sum() >= 2
        single += (pv != 0).sum() == 1
    # per 8 (row, head): gains (0.5, 5, 8, 2048) x (no tie, tie)
    assert sub >= rows // 4 and zero >= rows // 2 and all3 >= rows // 4, (sub, zero, all3)
    assert tie >= rows // 4 and single >= rows // 16, (tie, single)


@pytest.mark.parametrize("mode", A.MODES[1:])
@pytest.mark.parametrize("name,p0,T", [("cancel_kq", 250, 38), ("cancel_kq", 5, 40), ("cancel_kqv", 250, 38)])
def test_wrong_accumulation_changes_half_of_the_outputs(name, p0, T, mode):
    """Discrimination: an accumulation other than the fmaf chain in K order, in the product the case aims
    at, changes at least half of the output words against orc_attn_rows."""
    kq, kqv = (mode, "H1") if name == "cancel_kq" else ("H1", mode)
    out, _, _ = _emulated(name, p0, T, kq, kqv)
    share = _share(out, _case(name, p0, T)[1])
    print(f"{name} p0 {p0} T {T} {mode}: {share:.4f} of the output words differ")
    assert share >= 0.5


def test_benign_inputs_do_not_discriminate():
    """What the engine tests feed: a wrong KQ accumulation changes about 2 % of the output words on N(0,1)
    inputs (a 1-ulp change in a score rarely survives f16(w - max) and the f16 rounding of P): why the
    cases exist."""
    for mode in A.MODES[1:]:
        out, _, _ = _emulated("benign", 250, 38, mode, "H1")
        assert _share(out, _case("benign", 250, 38)[1]) < 0.1


ROPE_SHAPES = [(256, 4, 2, 5, 6), (64, 2, 1, 37, 5), (256, 2, 2, 0, 4)]


@pytest.mark.parametrize("hd,Hh,Hk,p0,T", ROPE_SHAPES)
def test_rope_case_tells_a_contracted_build(hd, Hh, Hk, p0, T):
    ld = (Hh + 2 * Hk) * hd + 24
    qkv = A.rope_case(T, p0, Hh, Hk, hd, ld)
    q16 = np.zeros((T, Hh, hd), np.uint16)
    kc = np.zeros((CTX, Hk * hd), np.uint16)
    vc = np.zeros((Hk * hd, CTX), np.uint16)
    O.rope_kv_rows(qkv, T, p0, Hh, Hk, hd, CTX, q16, kc, vc)
    cq, ck = A.rope_contracted(qkv, T, p0, Hh, Hk, hd)
    dq, dk = float((cq.reshape(q16.shape) != q16).mean()), float((ck != kc[p0:p0 + T]).mean())
    print(f"rope hd {hd} p0 {p0}: contracted q16 words {dq:.3f}, K words {dk:.3f}")
    assert dq >= 0.25 and dk >= 0.25
    v = vc[:, p0:p0 + T]
    k_and_v = np.concatenate([v.ravel(), kc[p0:p0 + T].ravel()])
    assert (k_and_v == 0x8000).any()                                    # -0
    assert ((k_and_v & 0x7FFF) == 0x7C00).any()                         # past 65504: inf
    assert ((k_and_v & 0x7FFF) == 0x7BFF).any()                         # +-65504
    assert (((k_and_v & 0x7C00) == 0) & ((k_and_v & 0x3FF) != 0)).any()  # subnormals
    # the ties round to even: 1 + 2^-11 -> 1.0, 1 + 3 * 2^-11 -> 1 + 2^-9
    assert (v == 0x3C00).any() and (v == 0x3C02).any()
