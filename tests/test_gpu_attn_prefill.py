"""GPU: the prefill attention's four kernels, each alone (gemma_test_rope_kv_prefill, gemma_test_attn_prefill),
against the oracle on the adversarial inputs of tests/attn_adversary.py.

k_rope_kv_prefill, k_attn_rows (form 0) and k_attn_mx (form 1) are bit-exact claims: every output word must
equal orc_rope_kv_rows / orc_attn_rows.  k_attn_prefill (form 2) is approximate by design and gets an error
bound.  The inputs make one misplaced rounding in a dot product worth 2^-5 .. 2^-1 in a score
(cancel_kq) or 2^10 ulps of an output (cancel_kqv); the CPU half (tests/test_attn_adversary.py) proves that
on emulated wrong accumulations."""
import ctypes as C
import functools

import numpy as np
import pytest

import attn_adversary as A
import oracle_ctypes as O

gpu = pytest.mark.gpu
CTX = 320
SENTINEL = np.float32(-7.5)
PAD = 24  # out columns past H * hd
U32 = np.uint32

HEADS = [(8, 1), (4, 2), (2, 2), (16, 1), (16, 16)]  # G = 8, 2, 1, 16, 1
# (p0, T, n_kv of the launch): one row; 16-row tiles across a multiple of 32; p0 off the tiles; fewer rows
# than a tile and fewer key tiles than waves; more than 8 key tiles (the prefetch path), two step groups and
# L capped at n_kv = 288 below the last row's own 320; n_kv == ctx
GEOMS = [(0, 1, 32), (0, 33, 64), (5, 40, 64), (27, 6, 64), (250, 38, 288), (282, 38, 320)]


def _lib():
    import gemma_hip as G
    L = G.lib()
    L.gemma_test_attn_prefill.restype = C.c_int
    L.gemma_test_attn_prefill.argtypes = [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_int64, C.c_int, C.c_void_p]
    L.gemma_test_rope_kv_prefill.restype = C.c_int
    L.gemma_test_rope_kv_prefill.argtypes = [C.c_void_p, C.c_int64] + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 3
    L.gemma_test_rows_rope_kv.restype = C.c_int
    L.gemma_test_rows_rope_kv.argtypes = [C.c_void_p, C.c_int64] + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 2
    return G, L


@functools.lru_cache(maxsize=40)
def _case(name, p0, T, H, Hkv, hd, base="cancel_kq"):
    """the inputs and the oracle's output [T][H*hd], computed once for the forms that share them"""
    cs = A.make(name, T, p0, H, Hkv, hd, CTX, base=base)
    ref = A.oracle_out(cs)
    ref.setflags(write=False)
    return cs, ref


def _run(form, cs, n_kv, ldo=None):
    """-> (return code, out [T][ldo] that went in as SENTINEL everywhere, message)"""
    G, L = _lib()
    ldo = cs["H"] * cs["hd"] + PAD if ldo is None else ldo
    out = np.full((cs["T"], ldo), SENTINEL, np.float32)
    r = L.gemma_test_attn_prefill(cs["q16"].ctypes.data, cs["kc"].ctypes.data, cs["vc"].ctypes.data, cs["T"], cs["p0"],
                                  cs["H"], cs["Hkv"], cs["hd"], CTX, n_kv, ldo, form, out.ctypes.data)
    return r, out, G.last_error()


def _diagnose(cs, got, ref, n_kv, form):
    """where an exact form left the oracle: row, head, dim, the row's n_kv, and what the other form says"""
    H, hd = cs["H"], cs["hd"]
    bad = np.argwhere(got.view(U32) != ref.view(U32))
    t, col = (int(x) for x in bad[0])
    msg = [f"{cs['case']} (base {cs['base']}) form {form} H {H} Hkv {cs['Hkv']} hd {hd} p0 {cs['p0']} T {cs['T']} n_kv {n_kv}: "
           f"{len(bad)} of {got.size} words differ; first at row {t} (position {cs['p0'] + t}, n_kv(i) "
           f"{min(n_kv, O.attn_n_kv(cs['p0'] + t, CTX))}) head {col // hd} dim {col % hd}: got {got[t, col]!r} want {ref[t, col]!r}; "
           f"rows hit {sorted(set(bad[:, 0].tolist()))[:12]} heads hit {sorted(set((bad[:, 1] // hd).tolist()))}"]
    other = 1 - form
    r, o2, why = _run(other, cs, n_kv)
    if r == 0:
        o2 = o2[:, :H * hd]
        msg.append(f"form {other} differs from the oracle in {int((o2.view(U32) != ref.view(U32)).sum())} words, "
                   f"from form {form} in {int((o2.view(U32) != got.view(U32)).sum())}")
    else:
        msg.append(f"form {other} does not run this shape ({why})")
    return "; ".join(msg)


def _check_exact(form, name, p0, T, n_kv, H, Hkv, hd, base="cancel_kq"):
    cs, ref = _case(name, p0, T, H, Hkv, hd, base)
    r, out, why = _run(form, cs, n_kv)
    assert r == 0, why
    assert (out[:, H * hd:] == SENTINEL).all(), "padding columns of out were written"
    got = out[:, :H * hd]
    if not np.array_equal(got.view(U32), ref.view(U32)):
        return _diagnose(cs, got, ref, n_kv, form)
    return None


@gpu
@pytest.mark.parametrize("form", [0, 1], ids=["rows", "mx"])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_attn_exact_forms_equal_the_oracle(H, Hkv, form):
    """k_attn_rows / k_attn_mx == orc_attn_rows bit for bit over the five cases and six geometries; the
    padding columns of out keep their sentinel.  k_attn_rows serves G <= 8: G = 16 must be refused."""
    if form == 0 and H // Hkv > 8:
        cs, _ = _case("benign", 27, 6, H, Hkv, 256)
        r, out, why = _run(0, cs, 64)
        assert r != 0 and "attn_rows: unsupported shape" in why, (r, why)
        assert (out == SENTINEL).all()
        return
    fails = []
    for p0, T, n_kv in GEOMS:
        for name in A.CASES:
            fails.append(_check_exact(form, name, p0, T, n_kv, H, Hkv, 256))
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails[:6])


@gpu
@pytest.mark.parametrize("form", [0, 1], ids=["rows", "mx"])
def test_attn_exact_forms_with_stale_caches_of_every_base(form):
    """finite garbage past the last row (a rewind's leftovers) under each base case: k_attn_mx multiplies it
    by P = 0 over [n_kv(i), L), k_attn_rows must not read it"""
    fails = []
    for H, Hkv in [(8, 1), (4, 2)]:
        for p0, T, n_kv in [(5, 40, 64), (250, 38, 288)]:
            for base in ("cancel_kqv", "underflow", "benign"):
                fails.append(_check_exact(form, "stale", p0, T, n_kv, H, Hkv, 256, base))
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails[:6])


@gpu
@pytest.mark.parametrize("hd", [64, 96, 160])
def test_attn_rows_other_head_dims(hd):
    """k_attn_rows at 2, 3 and 5 steps per chain (k_attn_mx is head_dim 256 only)"""
    fails = []
    for H, Hkv in [(4, 2), (8, 1)]:
        for p0, T, n_kv in [(0, 33, 64), (27, 6, 64), (250, 38, 288), (282, 38, 320)]:
            for name in A.CASES:
                fails.append(_check_exact(0, name, p0, T, n_kv, H, Hkv, hd))
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails[:6])


@gpu
def test_attn_mx_refusals_start_nothing():
    """attn_mx_unsupported: head_dim != 256, G = 3, rows past n_kv -> non-zero, the reason, out untouched"""
    for (H, Hkv, hd, p0, T, n_kv), reason in [((4, 2, 64, 27, 6, 64), "head_dim != 256"),
                                              ((3, 1, 256, 27, 6, 64), "query heads per kv head must divide 16"),
                                              ((4, 2, 256, 27, 6, 32), "context")]:
        cs = A.make("benign", T, p0, H, Hkv, hd, CTX)
        r, out, why = _run(1, cs, n_kv)
        assert r != 0 and why == "attn_mx: " + reason, (r, why)
        assert (out == SENTINEL).all()
    # the same rows past n_kv through the other two forms
    cs = A.make("benign", 6, 27, 4, 2, 256, CTX)
    for form in (0, 2):
        r, out, why = _run(form, cs, 32)
        assert r != 0 and "unsupported shape" in why and (out == SENTINEL).all(), (form, r, why)


@gpu
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_attn_prefill_f16_form_within_its_bound(H, Hkv):
    """k_attn_prefill (f16 MFMA, f32 sums in another order) on benign and underflow inputs: not bit-exact by
    design, every weight and the normaliser may move one f16 step.  Against ref64 = sum_j P_j v_j in
    float64 from the same f16 inputs and the oracle's own P:
        |got - ref64| <= 4 * 2^-10 * sum_j P_j |v_j| + n_kv * 2^-24 * max_j |v_j|
    Largest observed ratio to that bound on an MI355X: 0.26 (H 16, Hkv 1; 0.20, 0.13, 0.08 and 0.23 for
    (8, 1), (4, 2), (2, 2) and (16, 16))."""
    worst = 0.0
    for p0, T, n_kv in GEOMS:
        for name in ("benign", "underflow"):
            cs, ref = _case(name, p0, T, H, Hkv, 256)
            r, out, why = _run(2, cs, n_kv)
            assert r == 0, why
            assert (out[:, H * 256:] == SENTINEL).all()
            got = out[:, :H * 256].astype(np.float64)
            emu, P, _ = A.attn_emulated(cs)  # P16 of the oracle's pieces; its output is the oracle's
            assert np.array_equal(emu.view(U32), ref.view(U32))
            V = cs["vc"].view(np.float16).astype(np.float64).reshape(Hkv, 256, CTX)
            for t in range(T):
                nk = O.attn_n_kv(p0 + t, CTX)
                for h in range(H):
                    p = P[t, h].view(np.float16).astype(np.float64)
                    v = V[h // (H // Hkv), :, :nk]
                    ref64 = v @ p
                    bound = 4 * 2.0 ** -10 * (np.abs(v) @ p) + nk * 2.0 ** -24 * np.abs(v).max(axis=1)
                    err = np.abs(got[t, h * 256:(h + 1) * 256] - ref64)
                    ratio = float((err / bound).max())
                    worst = max(worst, ratio)
                    # on a miss, the oracle's exact form against the same reference, for scale
                    assert ratio <= 1.0, (name, p0, T, t, h, ratio,
                                          float((np.abs(ref[t, h * 256:(h + 1) * 256] - ref64) / bound).max()))
    print(f"attn_prefill form 2 H {H} Hkv {Hkv}: largest |got - ref64| / bound = {worst:.4f}")


ROPE_SHAPES = [(hd, Hkv, p0) for hd in (256, 64) for Hkv in (1, 2) for p0 in (0, 5, 37)]


@gpu
@pytest.mark.parametrize("hd,Hkv,p0", ROPE_SHAPES)
def test_rope_kv_prefill_equals_the_oracle(hd, Hkv, p0):
    """k_rope_kv_prefill (q16, K, V) and k_rows_rope_kv (K, V; batch.hip restates it) == orc_rope_kv_rows bit
    for bit on inputs where a contracted x0*c - x1*s stores other words (at least a quarter of them,
    tests/test_attn_adversary.py), with f16 ties, subnormals, +-65504, inf and -0 among the stored values;
    qkv rows padded; cache words outside rows p0 .. p0 + T - 1 unchanged."""
    G, L = _lib()
    H, T = 4, 6
    ld = (H + 2 * Hkv) * hd + 24
    qkv = A.rope_case(T, p0, H, Hkv, hd, ld)
    rng = np.random.default_rng(hd + Hkv + p0)
    kc0 = rng.integers(0, 65536, (CTX, Hkv * hd)).astype(np.uint16)
    vc0 = rng.integers(0, 65536, (Hkv * hd, CTX)).astype(np.uint16)
    q_ref, k_ref, v_ref = np.zeros((T, H, hd), np.uint16), kc0.copy(), vc0.copy()
    O.rope_kv_rows(qkv, T, p0, H, Hkv, hd, CTX, q_ref, k_ref, v_ref)
    q_got, k_got, v_got = np.full((T, H, hd), 0xDEAD, np.uint16), kc0.copy(), vc0.copy()
    r = L.gemma_test_rope_kv_prefill(qkv.ctypes.data, ld, T, p0, H, Hkv, hd, CTX, 10000.0, q_got.ctypes.data,
                                     k_got.ctypes.data, v_got.ctypes.data)
    assert r == 0, G.last_error()
    k_row, v_row = kc0.copy(), vc0.copy()  # the batch pass's restatement, one row-table entry per row
    r = L.gemma_test_rows_rope_kv(qkv.ctypes.data, ld, T, p0, H, Hkv, hd, CTX, 10000.0, k_row.ctypes.data, v_row.ctypes.data)
    assert r == 0, G.last_error()
    rows = slice(p0, p0 + T)
    outside_k = np.ones(CTX, bool)
    outside_k[rows] = False
    assert np.array_equal(k_got[outside_k], kc0[outside_k]) and np.array_equal(v_got[:, outside_k], vc0[:, outside_k]), \
        "cache words outside the launch's rows changed"
    assert np.array_equal(k_row[outside_k], kc0[outside_k]) and np.array_equal(v_row[:, outside_k], vc0[:, outside_k]), \
        "k_rows_rope_kv: cache words outside the launch's rows changed"
    for what, got, ref in (("q16", q_got, q_ref), ("K", k_got[rows], k_ref[rows]), ("V", v_got[:, rows].T, v_ref[:, rows].T),
                           ("k_rows_rope_kv K", k_row[rows], k_ref[rows]), ("k_rows_rope_kv V", v_row[:, rows].T, v_ref[:, rows].T)):
        bad = np.argwhere(got.reshape(T, -1) != ref.reshape(T, -1))
        assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} words differ; first at row {bad[0][0]} (position "
                               f"{p0 + bad[0][0]}) element {bad[0][1]} (head {bad[0][1] // hd}, dim {bad[0][1] % hd}): got "
                               f"{int(got.reshape(T, -1)[tuple(bad[0])]):#06x} want {int(ref.reshape(T, -1)[tuple(bad[0])]):#06x}")
