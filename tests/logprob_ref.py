"""numpy restatement of the engine's log-probability rule (include/gemma_hpc.h at
gemma_engine_set_logprobs, DESIGN.md §5b⁗′): a helper for the log-probability tests, not a test.

    M = max_i l[i]                                  (float compare: exact, order-free, -0 == +0)
    S = sum_i exp(f64(l[i]) - f64(M))               (f64; an -inf entry contributes 0; S >= 1)
    logprob(l, t) = (f64(l[t]) - f64(M)) - log(S)   (-inf when l[t] is -inf)

Rows with a NaN, or whose maximum is -inf, are outside the contract.

MARGIN: each term is at most 1 and S >= 1, so reordering a sum of V <= 256,000 such terms and an f64
exp good to an ulp or two move S by less than V * 2^-53 = 2.9e-11 relative; log and the subtraction add
parts in 1e-16.  The device must agree with this file to 1e-9 absolute, about 30 x that bound."""
import numpy as np

MARGIN = 1e-9
CHUNK = 1024  # logits per workgroup of k_lse_parts (csrc/kernels.h LSE_CHUNK)


def logprob(row, t):
    """f64 log-probability of token t under softmax(row); row f32 [V]"""
    l = np.asarray(row, dtype=np.float32)
    assert l.ndim == 1 and 0 <= int(t) < l.size
    M = np.float64(l.max())
    d = l.astype(np.float64) - M        # <= 0, or -inf
    S = np.exp(d).sum()                 # exp(-inf) = 0
    return np.float64(d[int(t)] - np.log(S))


def logprobs(rows, tokens):
    """logprob(rows[r], tokens[r]) for rows [R][V]"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float32))
    return np.array([logprob(r, t) for r, t in zip(rows, tokens)], dtype=np.float64)


def all_tokens(row):
    """logprob(row, t) for every t"""
    l = np.asarray(row, dtype=np.float32)
    return np.array([logprob(l, t) for t in range(l.size)], dtype=np.float64)


def close(got, ref, margin=MARGIN):
    """elementwise: both -inf, or finite and within the margin"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    both_ninf = np.isneginf(got) & np.isneginf(ref)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(got) & np.isfinite(ref) & (np.abs(got - ref) <= margin)
    return both_ninf | near


# ---- the row kinds the GPU test runs (each returns rows [R][V] f32 and tokens [R], all rows and
# tokens distinct wherever V allows it, so that a row-stride or token mix-up shows) -----------------
def _tokens(rng, R, V):
    return rng.permutation(V)[:R].astype(np.int32) if V >= R else rng.integers(0, V, R).astype(np.int32)


def rows_normal(rng, R, V):
    return (rng.standard_normal((R, V)) * 3.0).astype(np.float32), _tokens(rng, R, V)


def rows_equal(rng, R, V):
    x = np.repeat((rng.standard_normal((R, 1)) * 3.0).astype(np.float32), V, axis=1)
    return x, _tokens(rng, R, V)


def rows_peak80(rng, R, V):
    """one peak 80 above the rest: the rest's terms exp(-80 + N(0, 1)) = 1e-35 vanish in S, and every
    other token's log-probability is near -80"""
    x = rng.standard_normal((R, V)).astype(np.float32)
    t = _tokens(rng, R, V)
    peak = rng.integers(0, V, R)
    x[np.arange(R), peak] += np.float32(80.0)
    t[::2] = peak[::2]  # every other row scores its peak
    return x, t


def rows_max_at_ends(rng, R, V):
    """the maximum in the last chunk (the last entry) on even rows, at index 0 on odd rows"""
    x = rng.standard_normal((R, V)).astype(np.float32)
    x[0::2, V - 1] = np.float32(9.0)
    x[1::2, 0] = np.float32(9.0)
    return x, _tokens(rng, R, V)


def rows_huge(rng, R, V):
    """entries of +-3e38: l - M overflows f32 and must be formed in f64"""
    x = rng.standard_normal((R, V)).astype(np.float32)
    k = rng.integers(0, V, (R, 3))
    x[np.arange(R), k[:, 0]] = np.float32(-3e38)
    x[np.arange(R), k[:, 1]] = np.float32(3e38)
    if V > 2:
        x[np.arange(R), k[:, 2]] = np.float32(3e38)
    t = _tokens(rng, R, V)
    if x[0, k[0, 0]] < 0:
        t[0] = k[0, 0]  # one row scores a -3e38 entry (finite: -6e38 - log S)
    return x, t


def rows_ninf(rng, R, V):
    """-inf entries: scattered ones, a whole chunk of them (where the row has more than one chunk),
    and on every third row the scored token itself"""
    x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
    x[rng.random((R, V)) < 0.1] = -np.inf
    live = np.arange(V)
    if V > CHUNK:
        c = int(rng.integers(0, (V - 1) // CHUNK))  # a full chunk, never the only one
        x[:, c * CHUNK:(c + 1) * CHUNK] = -np.inf
        live = live[live // CHUNK != c]
    keep = rng.choice(live, R)
    x[np.arange(R), keep] = np.float32(1.5)  # the maximum is finite
    t = _tokens(rng, R, V)
    if V > 1:
        for r in range(0, R, 3):
            if t[r] != keep[r]:
                x[r, t[r]] = -np.inf
    return x, t


def rows_zero_max(rng, R, V):
    """maxima of -0.0 and +0.0 mixed; everything else negative"""
    x = (-np.abs(rng.standard_normal((R, V))) - 0.5).astype(np.float32)
    k = rng.integers(0, V, (R, 2))
    x[np.arange(R), k[:, 0]] = np.float32(-0.0)
    x[np.arange(R), k[:, 1]] = np.float32(0.0) if V > 1 else np.float32(-0.0)
    t = _tokens(rng, R, V)
    t[::2] = k[::2, 0]
    return x, t


ROW_KINDS = dict(normal=rows_normal, equal=rows_equal, peak80=rows_peak80, max_at_ends=rows_max_at_ends,
                 huge=rows_huge, ninf=rows_ninf, zero_max=rows_zero_max)
