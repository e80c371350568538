"""Adversarial inputs for the prefill attention kernels (k_attn_rows, k_attn_mx, k_attn_prefill,
k_rope_kv_prefill).  TEST INFRASTRUCTURE (CPU only, seeded): f16 bit patterns for q16 [T][H][hd], the K
cache [ctx][Hkv*hd] and the V cache [Hkv*hd][ctx] of one launch whose row t is sequence position
p0 + t, and f32 q | k | v rows for the RoPE / store kernel.

What a synthetic Gemma feeds these kernels (q, k, v about N(0,1), scores within a few units, caches zero
past the prompt) cannot tell an fmaf chain in K order from any other accumulation: a 1-ulp change in a
score does not survive f16(w - max) and the f16 rounding of P.  The cases here make it survive.

vec_dot_f16 keeps 32 chains per output: chain c runs over elements 32s + c, step s = 0, 1,
...; k_attn_mx carries four consecutive steps of a chain in one v_mfma_f32_16x16x4_f32, which is exact
only if that instruction is an fmaf chain in K order from its C input.

  cancel_kq   PATTERNS names chains and steps.  On a pattern's elements q holds one value Q per (row,
              head) and K holds coef * x per key with coefficients summing to 0 (+1, -1 or +1, +1, -2),
              so the products cancel exactly in the chain whatever Q and x are.  For BIG_SHARE of the
              (key, pattern) pairs |Q x| lies in 2^18 .. 2^22 (the rest below 2^13, cancelling too), so
              the chain's partial sum has an ulp of 2^-5 .. 2^-1 while the big term is in it and
              everything added meanwhile is rounded to that ulp.  Patterns with a free step between
              their terms put there a product of (0.5 +- 0.25) ulp of 2^8 * |x| (half an ulp of the
              partial sum for the smallest Q, a quarter for the largest).  Patterns sit in steps 0-3
              (inside the first MFMA of a chain), in steps 4-7 (inside the second) and across the two.
              Every other element is N(0,1) (K) and N(0,1) * 2.5 / sqrt(hd) (q): final scores stay
              within about +-12 and P keeps many distinct values.  One misplaced rounding moves a score
              by 2^-5 .. 2^-1.
  cancel_kqv  K rows of the 32-key blocks DUP_BLOCKS[i] = (b, b + 1) are equal (key j and j + 32: the
              same chain, consecutive steps, inside one group of 4 steps and across two), so their
              scores and P are equal; for V_SHARE of those (dim, key) pairs V holds +X and -X + small,
              |X| in 2^6 .. 2^14 and small 1 .. 3 f16 ulps of X: p X - p X + p small in one chain.
  underflow   Element E_SPREAD of K holds a distinct g_j in [-6, 0], of q a gain a per (row, head): 0.5
              (a mild spread), 5 or 8 (P normal, subnormal and exactly 0 by underflow in one row) or 2048
              (one survivor: the g_j are 6 / (p0 + T) apart).  K rows TIE_FIRST + TIE_STEP * i and the row
              after each are equal, with the lowest g and a bump on element E_TIE that only every
              other group of 4 (row, head) multiplies: those rows have two tied maxima.
  stale       a base case (cancel_kq unless told otherwise) with finite non-zero f16 garbage in every K
              row and V column past p0 + T - 1: what a rewind leaves.  k_attn_mx multiplies it by
              P = 0 over [n_kv(i), L) where the oracle never reads; bit equality is the expectation.
  benign      N(0,1) at two score scales, as _attn_case in test_gpu_ops.py.

`attn_emulated` restates the attention with a selectable chain accumulation in numpy: H1 the fmaf chain
(it equals orc_attn_rows bit for bit, tests/test_attn_adversary.py), and the micro-probe's other
hypotheses (tests/micro/mfma_f32_exact.hip): H2 reverse K order inside each group of 4 steps, H3 the 4
products of a group added to the accumulator with one rounding, H4 pairwise (p0+p1)+(p2+p3) then the
accumulator; SPLIT starts every group from zero and adds it to the accumulator afterwards.

Achieved shares of output words that differ from orc_attn_rows (H 4, Hkv 2, hd 256, ctx 320, seed 0;
the test asserts >= 0.5), wrong accumulation in the product the case aims at:
  cancel_kq  p0 250, T 38:  H2 1.000  H3 1.000  H4 1.000  SPLIT 1.000
  cancel_kq  p0 5, T 40:    H2 1.000  H3 1.000  H4 1.000  SPLIT 1.000
  cancel_kqv p0 250, T 38:  H2 0.990  H3 0.961  H4 0.986  SPLIT 0.986
  benign     p0 250, T 38 (wrong KQ): 0.020, 0.020, 0.020, 0.007

decode_case turns a case into ONE decode row (the f32 q | k | v whose values are the case's f16 words, the caches
with finite non-zero garbage at the row's own position) for the decode attention's kernels, which see one row
per workgroup: what they can get wrong is the quad fold of the 32 chain values (chain_dot mode FOLD) and the
step order of a chain (REV).  Shares on single rows (H 4, Hkv 2, ctx 320, 29 rows at 3, 14, .. 311; hd 256 / 128;
the whole table is in tests/test_attn_decode_adversary.py, which asserts its floors):
  benign     FOLD in KQ: 0.523 / 0.510 of the score words, 0.0086 / 0 of the output words
  cancel_kq  REV in KQ, each row at pos >= 31: 1.000 / 1.000 of the output words
  cancel_kqv REV in KQV, pos >= 255: 0.995 .. 1.000; FOLD in KQV, pos >= 31: 0.231 .. 0.510

rope_case builds q | k | v rows for which a contracted fma(x0, c, -(x1*s)) (and fma(x0, s, x1*c)) stores
other f16 words than the separate multiplies: each pair has x0*c and x1*s (or x0*s and -x1*c) agree to
2^-15 .. 2^-19, so the f32 rounding error of the first product is 2^-9 .. 2^-5 of the difference.  v, and
k at sequence position 0 (cos 1, sin 0: a pass-through), carry F16_SPECIALS: values that round to f16
ties, to subnormals, to +-65504, just past it (to inf), and -0.
Contracted q16 / K words that differ (the test asserts >= 0.25): hd 256, p0 5: 0.436 / 0.464; hd 64, p0 37:
0.463 / 0.456; hd 256, p0 0 (row 0 is a pass-through): 0.299 / 0.334.
"""
import numpy as np

import oracle_ctypes as O

F32, F16, U16 = np.float32, np.float16, np.uint16
CASES = ("cancel_kq", "cancel_kqv", "underflow", "stale", "benign")
MODES = ("H1", "H2", "H3", "H4", "SPLIT")
DECODE_MODES = ("FOLD", "REV")  # what a one-row kernel can get wrong: the quad fold, the step order of a chain

# cancel_kq: (chain, ((step, coefficient), ...), free step that carries the near-half-ulp term or None)
PATTERNS = (
    (1, ((0, 1), (2, -1)), 1),           # inside steps 0-3
    (5, ((0, 1), (1, 1), (3, -2)), 2),   # three terms inside steps 0-3
    (9, ((4, 1), (6, -1)), 5),           # inside steps 4-7
    (14, ((4, 1), (5, 1), (7, -2)), 6),  # three terms inside steps 4-7
    (18, ((2, 1), (5, -1)), 3),          # across the two MFMAs of a chain
    (22, ((3, 1), (4, -1)), None),       # across, adjacent steps
    (27, ((1, 1), (6, -1)), 4),          # across, five steps apart
    (30, ((0, 1), (1, -1)), None),       # the only one that fits head_dim 64
)
BIG_SHARE = 0.5
Q_EXP = (8, 9)          # |Q| = 2^Q_EXP * [1, 2)
X_EXP_BIG = (10, 11)    # |x| = 2^X_EXP * [1, 2): |Q x| in 2^18 .. 2^22 (one less for a coefficient of 2)
X_EXP_SMALL = (-3, 1)
Q_MID = 0.25            # q on a pattern's free step
DUP_BLOCKS = ((0, 1), (3, 4), (6, 7))  # steps (0, 1), (3, 4): across two groups of 4, (6, 7)
V_SHARE = 0.5
E_SPREAD, E_TIE = 7, 40
GAINS = (0.5, 5.0, 8.0, 2048.0)
TIE_FIRST, TIE_STEP = 1, 24

F16_SPECIALS = np.array([
    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2.0 + 2.0 ** -10),  # ties between two f16 normals
    2.0 ** -25, 3 * 2.0 ** -25, -5 * 2.0 ** -25,                     # ties between f16 subnormals (2^-25 -> 0)
    1e-6, -3.3e-7, 2.0 ** -24, 2.0 ** -26,                           # subnormal results, and one that rounds to 0
    65504.0, -65504.0, 65519.996, -65519.996,                        # the largest f16, and just below the tie
    65520.0, -65520.0, 70000.0,                                      # the tie that rounds to inf, and past it
    -0.0, -1e-9, 0.0], dtype=F32)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F32).astype(F16)).view(U16)


def _pow2_mant(rng, shape, exps):
    """+- 2^e * (1 + m / 1024), e uniform in [exps[0], exps[1]]: exact in f16"""
    e = rng.integers(exps[0], exps[1] + 1, shape)
    m = rng.integers(0, 1024, shape)
    s = rng.integers(0, 2, shape) * 2 - 1
    return (s * np.exp2(e.astype(np.float64)) * (1.0 + m / 1024.0)).astype(F32)


def _garbage(rng, shape):
    """finite non-zero f16 bit patterns, all exponents and both signs"""
    b = rng.integers(1, 0x7C00, shape).astype(U16)
    return b | (rng.integers(0, 2, shape).astype(U16) << 15)


def _base(rng, T, H, Hkv, hd, n, q_scale):
    q = (rng.standard_normal((T, H, hd)) * q_scale).astype(F32)
    k = rng.standard_normal((n, Hkv, hd)).astype(F32)
    v = rng.standard_normal((Hkv, hd, n)).astype(F32)
    return q, k, v


def _cancel_kq(rng, T, H, Hkv, hd, n):
    q, k, v = _base(rng, T, H, Hkv, hd, n, 2.5 / np.sqrt(hd))
    for c, terms, mid in PATTERNS:
        if max(s for s, _ in terms) >= hd // 32:
            continue
        two = max(abs(cf) for _, cf in terms) == 2
        Q = _pow2_mant(rng, (T, H), Q_EXP)
        big = rng.random((n, Hkv)) < BIG_SHARE
        xb = _pow2_mant(rng, (n, Hkv), (X_EXP_BIG[0] - two, X_EXP_BIG[1] - two))
        x = np.where(big, xb, _pow2_mant(rng, (n, Hkv), X_EXP_SMALL))
        for s, cf in terms:
            q[:, :, 32 * s + c] = Q
            k[:, :, 32 * s + c] = cf * x
        if mid is not None and mid < hd // 32:
            # (0.5 +- 0.25) ulp of 2^Q_EXP[0] * |x| (the f32 ulp of y is 2^(floor(log2 y) - 23))
            ulp = np.exp2(np.floor(np.log2(np.abs(x))) + Q_EXP[0] - 23)
            t = ulp * (0.5 + 0.25 * rng.uniform(-1, 1, x.shape)) * (rng.integers(0, 2, x.shape) * 2 - 1)
            q[:, :, 32 * mid + c] = Q_MID * (rng.integers(0, 2, (T, H)) * 2 - 1)
            k[:, :, 32 * mid + c] = t / Q_MID
    return q, k, v


def _cancel_kqv(rng, T, H, Hkv, hd, n):
    q, k, v = _base(rng, T, H, Hkv, hd, n, 2.0 / np.sqrt(hd))
    for b0, b1 in DUP_BLOCKS:
        m = min(32, n - 32 * b1)
        if m <= 0:
            continue
        j0, j1 = slice(32 * b0, 32 * b0 + m), slice(32 * b1, 32 * b1 + m)
        k[j1] = k[j0]
        X = _pow2_mant(rng, (Hkv, hd, m), (6, 13))  # |X| < 2^14
        ulp16 = np.exp2(np.floor(np.log2(np.abs(X))) - 10)
        small = ulp16 * rng.integers(1, 4, X.shape) * (rng.integers(0, 2, X.shape) * 2 - 1)
        on = rng.random(X.shape) < V_SHARE
        v[:, :, j0] = np.where(on, X, v[:, :, j0])
        v[:, :, j1] = np.where(on, -X + small, v[:, :, j1])
    return q, k, v


def underflow_kind(t, h, H):
    """(gain index into GAINS, tie multiplier on) of row t, head h"""
    i = t * H + h
    return i % 4, (i // 4) % 2 == 1


def tie_pairs(n):
    return [j for j in range(TIE_FIRST, n - 1, TIE_STEP)]


def _underflow(rng, T, H, Hkv, hd, n):
    q, k, v = _base(rng, T, H, Hkv, hd, n, 1.0 / np.sqrt(hd))
    g = -6.0 * rng.permutation(n) / n  # distinct after the f16 rounding: 6 / 320 > an f16 ulp of 6
    k[:, :, E_SPREAD] = g[:, None]
    k[:, :, E_TIE] = 0.0
    for i, j in enumerate(tie_pairs(n)):
        k[j, :, E_SPREAD] = -6.0 - i / 32.0
        k[j, :, E_TIE] = 1.0 + i / 32.0  # a later pair outranks every earlier one
        k[j + 1] = k[j]
    for t in range(T):
        for h in range(H):
            gi, tie = underflow_kind(t, h, H)
            a = GAINS[gi]
            q[t, h, E_SPREAD] = a
            q[t, h, E_TIE] = (8.0 * a + 16.0) if tie else 0.0  # lifts the pairs past a * 0 + noise
    return q, k, v


def _benign(rng, T, H, Hkv, hd, n):
    q, k, v = _base(rng, T, H, Hkv, hd, n, 1.0 / np.sqrt(hd))
    q[0::2] *= 0.5  # the two score scales of test_gpu_ops._attn_case, by row
    q[1::2] *= 4.0
    return q, k, v


_MAKERS = {"cancel_kq": _cancel_kq, "cancel_kqv": _cancel_kqv, "underflow": _underflow, "benign": _benign}


def make(case, T, p0, H, Hkv, hd, ctx, seed=0, base="cancel_kq"):
    """-> dict(q16 [T][H][hd], kc [ctx][Hkv*hd], vc [Hkv*hd][ctx]) of u16 (f16 bits) plus the geometry.
    Positions 0 .. p0 + T - 1 are filled; the rest is zero, or garbage for case "stale" (of `base`)."""
    assert case in CASES and p0 >= 0 and T > 0 and p0 + T <= ctx and H % Hkv == 0 and hd % 32 == 0
    stale = case == "stale"
    name = base if stale else case
    n = p0 + T
    rng = np.random.default_rng([seed, CASES.index(name), T, p0, H, Hkv, hd])
    q, k, v = _MAKERS[name](rng, T, H, Hkv, hd, n)
    kc = np.zeros((ctx, Hkv * hd), U16)
    vc = np.zeros((Hkv * hd, ctx), U16)
    if stale:
        kc[n:] = _garbage(rng, (ctx - n, Hkv * hd))
        vc[:, n:] = _garbage(rng, (Hkv * hd, ctx - n))
    kc[:n] = _bits(k).reshape(n, Hkv * hd)
    vc[:, :n] = _bits(v).reshape(Hkv * hd, n)
    return dict(case=case, base=name, q16=_bits(q).reshape(T, H, hd), kc=kc, vc=vc, T=T, p0=p0, H=H, Hkv=Hkv, hd=hd, ctx=ctx)


def decode_case(case, pos, H, Hkv, hd, ctx, seed=0, base="cancel_kq", zero_v=None):
    """One decode row at `pos`, from make(case, 1, pos, ...): -> that dict plus
      qkv  f32 q | k | v whose values are the f16 values of q16[0], K row pos and V column pos: with the identity
           RoPE row (cos 1, sin 0) and q_scale 1 a kernel's q16 / k16 / stored V are those words;
      kc, vc  with row / column pos overwritten by finite non-zero garbage in every case: a kernel that
           reads its own position from the cache instead of the row is wrong (for "stale", garbage past pos too).
    zero_v = (kv head, first dim, dims): those V rows are zero at every position and in the row's v, so the
    outputs of that kv head's query heads are zero there (a Q8_0 image block with d == 0)."""
    cs = make(case, 1, pos, H, Hkv, hd, ctx, seed, base)
    kc, vc = cs["kc"], cs["vc"]
    if zero_v is not None:
        kvh, d0, nd = zero_v
        vc[kvh * hd + d0:kvh * hd + d0 + nd] = 0
    qkv = np.concatenate([_h2f(cs["q16"][0]).ravel(), _h2f(kc[pos]), _h2f(vc[:, pos])]).astype(F32)
    rng = np.random.default_rng([seed, 77, CASES.index(case), pos, H, Hkv, hd])
    kc[pos] = _garbage(rng, kc.shape[1])
    vc[:, pos] = _garbage(rng, vc.shape[0])
    return dict(cs, qkv=qkv, pos=pos)


def identity_rope(hd):
    """cos 1 | sin 0: the RoPE row under which q16 / k16 are the row's own f16 values"""
    return np.concatenate([np.ones(hd // 2, F32), np.zeros(hd // 2, F32)])


def decode_oracle(cs, rope_row=None, q_scale=1.0, taps=True):
    """orc_attn_decode_row on copies of the case's caches -> (out, scores, P16, kc, vc)"""
    kc, vc = cs["kc"].copy(), cs["vc"].copy()
    row = identity_rope(cs["hd"]) if rope_row is None else rope_row
    out, w, p = O.attn_decode_row(cs["qkv"], kc, vc, cs["pos"], cs["H"], cs["Hkv"], cs["hd"], cs["ctx"], row, q_scale, taps)
    return out, w, p, kc, vc


def oracle_out(cs, ldo=None, out=None):
    return O.attn_rows(cs["q16"], cs["kc"], cs["vc"], cs["T"], cs["p0"], cs["H"], cs["Hkv"], cs["hd"], cs["ctx"], ldo, out)


# ---- the attention restated with a selectable chain accumulation -------------------------------

def _fold32(acc):
    """ggml_vec_dot_f16's reduction of the 32 chain values [..., 32] (f32 at every add)"""
    x0 = (acc[..., 0:8] + acc[..., 16:24]) + (acc[..., 8:16] + acc[..., 24:32])
    t0 = x0[..., 0:4] + x0[..., 4:8]
    return (t0[..., 0] + t0[..., 1]) + (t0[..., 2] + t0[..., 3])


def _fold32_rows_in_order(acc):
    """FOLD: the four 8-wide accumulator rows added (a0 + a1) + (a2 + a3) where ggml adds (a0 + a2) + (a1 + a3):
    a quad fold that takes xor-1 before xor-2"""
    x0 = (acc[..., 0:8] + acc[..., 8:16]) + (acc[..., 16:24] + acc[..., 24:32])
    t0 = x0[..., 0:4] + x0[..., 4:8]
    return (t0[..., 0] + t0[..., 1]) + (t0[..., 2] + t0[..., 3])


def chain_dot(x, y, mode="H1"):
    """vec_dot_f16 of f16-valued f32 arrays over the last axis (a multiple of 32), the chains carried in
    groups of 4 steps as k_attn_mx's MFMAs carry them, each group accumulated as `mode` says.  FOLD: H1's
    chains, the final fold over the accumulator rows in another order; REV: every chain's steps last to first."""
    p = (x.astype(F32) * y.astype(F32))  # exact: 11-bit x 11-bit significands
    S = p.shape[-1] // 32
    p = p.reshape(p.shape[:-1] + (S, 32))
    acc = np.zeros(p.shape[:-2] + (32,), F32)
    if mode in DECODE_MODES:
        for s in (range(S) if mode == "FOLD" else reversed(range(S))):
            acc = acc + p[..., s, :]
        return _fold32_rows_in_order(acc) if mode == "FOLD" else _fold32(acc)
    for g0 in range(0, S, 4):
        st = [p[..., s, :] for s in range(g0, min(g0 + 4, S))]
        if mode == "H1":
            for t in st:
                acc = acc + t
        elif mode == "H2":
            for t in reversed(st):
                acc = acc + t
        elif mode == "H3":
            s64 = acc.astype(np.float64)
            for t in st:
                s64 = s64 + t.astype(np.float64)
            acc = s64.astype(F32)
        elif mode in ("H4", "SPLIT"):
            st = st + [np.zeros_like(st[0])] * (4 - len(st))
            grp = (st[0] + st[1]) + (st[2] + st[3]) if mode == "H4" else ((st[0] + st[1]) + st[2]) + st[3]
            acc = acc + grp
        else:
            raise ValueError(mode)
    return _fold32(acc)


def _h2f(b):
    return np.asarray(b, U16).view(F16).astype(F32)


def attn_emulated(cs, kq_mode="H1", kqv_mode="H1"):
    """-> (out [T][H*hd] f32, P16 bits per (t, h): list of [n_kv(t)] u16, scores per (t, h)).  The softmax
    is the oracle's own (orc_soft_max_row); only the two dot products are restated."""
    T, p0, H, Hkv, hd, ctx = (cs[n] for n in ("T", "p0", "H", "Hkv", "hd", "ctx"))
    q = _h2f(cs["q16"])
    K = _h2f(cs["kc"]).reshape(ctx, Hkv, hd)
    V = _h2f(cs["vc"]).reshape(Hkv, hd, ctx)
    out = np.zeros((T, H * hd), F32)
    P, W = {}, {}
    L = O.lib()
    for t in range(T):
        pos = p0 + t
        n_kv = O.attn_n_kv(pos, ctx)
        mask = np.where(np.arange(n_kv) > pos, -np.inf, 0.0).astype(F32)
        for h in range(H):
            kvh = h // (H // Hkv)
            w = np.ascontiguousarray(chain_dot(q[t, h][None, :], K[:n_kv, kvh], kq_mode))
            W[t, h] = w + mask
            y = np.zeros(n_kv, F32)
            L.orc_soft_max_row(O.ptr(w), O.ptr(mask), O.ptr(y), n_kv, 1.0)
            p16 = y.astype(F16)
            P[t, h] = p16.view(U16)
            out[t, h * hd:(h + 1) * hd] = chain_dot(p16.astype(F32)[None, :], V[kvh, :, :n_kv], kqv_mode)
    return out, P, W


# ---- RoPE / store inputs ----------------------------------------------------------------------------

def rope_tables(pos, hd, base=10000.0):
    c, s = np.zeros(hd // 2, F32), np.zeros(hd // 2, F32)
    O.lib().orc_rope_cos_sin(pos, hd, base, O.ptr(c), O.ptr(s))
    return c, s


def rope_case(T, p0, H, Hkv, hd, ldqkv, seed=0, base=10000.0):
    """-> qkv [T][ldqkv] f32 (q | k | v, the padding columns NaN: never read)"""
    rng = np.random.default_rng([seed, T, p0, H, Hkv, hd])
    half, nh = hd // 2, H + Hkv
    assert ldqkv >= (H + 2 * Hkv) * hd
    qkv = np.full((T, ldqkv), np.nan, F32)
    for t in range(T):
        c, s = (a.astype(np.float64) for a in rope_tables(p0 + t, hd, base))
        sh = (nh, half)
        delta = np.exp2(-rng.uniform(15, 19, sh)) * (rng.integers(0, 2, sh) * 2 - 1)
        first = rng.random(sh) < 0.5  # which of the two outputs cancels
        # the two products that cancel are +-M; the other output is then M / (s c), kept inside f16
        M = np.minimum(rng.uniform(256, 2048, sh), 30000.0 * np.abs(s * c)) * (rng.integers(0, 2, sh) * 2 - 1)
        ok = np.broadcast_to(s * c != 0.0, sh)
        with np.errstate(divide="ignore", invalid="ignore"):
            # r0 = x0 c - x1 s cancels with x1 = x0 (c / s)(1 + d); r1 = x0 s + x1 c with x1 = -x0 (s / c)(1 + d)
            a0 = np.where(first, M / c, M / s)
            a1 = a0 * np.where(first, c / s, -s / c) * (1.0 + delta)
        x0 = np.where(ok, a0, rng.standard_normal(sh) * 64.0)
        x1 = np.where(ok, a1, rng.standard_normal(sh) * 64.0)
        rows = np.concatenate([x0, x1], axis=1).astype(F32)  # [head][hd]: pairs (e, e + half)
        v = (rng.standard_normal(Hkv * hd) * 4.0).astype(F32)
        for kh in range(Hkv):
            v[kh * hd:kh * hd + len(F16_SPECIALS)] = np.roll(F16_SPECIALS, t + kh)[:hd]
        if p0 + t == 0:  # cos 1, sin 0: k passes through
            m = min(len(F16_SPECIALS), half)
            rows[H:, :m] = F16_SPECIALS[:m]
        qkv[t, :nh * hd] = rows.ravel()
        qkv[t, nh * hd:(H + 2 * Hkv) * hd] = v
    return qkv


def rope_contracted(qkv, T, p0, H, Hkv, hd, base=10000.0):
    """q16 [T][H][hd] and the K rows [T][Hkv*hd] (u16) that a build contracting x0*c - x1*s into
    fma(x0, c, -(x1*s)) and x0*s + x1*c into fma(x0, s, x1*c) would store (float64-emulated: the product
    x0*c is exact in f64, the sum rounded once more to f32)."""
    half, nh = hd // 2, H + Hkv
    out = np.zeros((T, nh, hd), F32)
    for t in range(T):
        c, s = rope_tables(p0 + t, hd, base)
        x = qkv[t, :nh * hd].reshape(nh, hd)
        x0, x1 = x[:, :half], x[:, half:]
        p1, p3 = (x1 * s).astype(F32), (x1 * c).astype(F32)
        out[t, :, :half] = (x0.astype(np.float64) * c.astype(np.float64) - p1.astype(np.float64)).astype(F32)
        out[t, :, half:] = (x0.astype(np.float64) * s.astype(np.float64) + p3.astype(np.float64)).astype(F32)
    q = out[:, :H] * F32(1.0 / np.sqrt(F32(hd)))
    with np.errstate(over="ignore"):
        return _bits(q), _bits(out[:, H:]).reshape(T, Hkv * hd)
