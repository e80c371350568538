"""GPU: the key-split matrix-core form of the exact prefill attention (attn_mx_long.hip: k_attn_mxl_scores,
k_attn_mxl_softmax, k_attn_mxl_kqv), alone through gemma_test_attn_mx_long against orc_attn_rows on the
adversarial inputs of tests/attn_adversary.py, and through the engine past the row form's last shape.  Bit
equality of u32 views throughout."""
import ctypes as C
import functools

import numpy as np
import pytest

import attn_adversary as A
import oracle_ctypes as O

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7.5)
PAD = 24  # out columns past H * hd
U32 = np.uint32
HEADS = [(8, 1), (4, 2), (2, 2), (16, 1), (16, 16)]  # G = 8, 2, 1, 16, 1
# (p0, T, ctx): one row and one key tile; row blocks across multiples of 32 with fewer key tiles than waves; the
# first 256-position key-block edge; 1024; the 2048-position P16 window edge; k_attn_mx's 2556-key limit; more
# rows than one 256-row slab; the last row at ctx - 1 with n_kv capped at ctx; k_attn_rows' G = 8 limit (4992);
# the end of an 8192 context
GEOMS = [(0, 1, 4096), (0, 70, 4096), (250, 12, 4096), (1018, 12, 4096), (2040, 20, 4096), (2550, 20, 4096),
         (2300, 300, 4096), (4070, 26, 4096), (4985, 20, 8192), (8150, 42, 8192)]


def _n_kv(p0, T, ctx):
    return min(32 * ((p0 + T) // 32 + 1), ctx)  # as the engine computes it


def _run(cs, n_kv):
    """-> (return code, out [T][H*hd + PAD] that went in as SENTINEL everywhere, message)"""
    import gemma_hip as G
    L = G.lib()
    L.gemma_test_attn_mx_long.restype = C.c_int
    L.gemma_test_attn_mx_long.argtypes = [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_int64, C.c_void_p]
    ldo = cs["H"] * cs["hd"] + PAD
    out = np.full((cs["T"], ldo), SENTINEL, np.float32)
    r = L.gemma_test_attn_mx_long(cs["q16"].ctypes.data, cs["kc"].ctypes.data, cs["vc"].ctypes.data, cs["T"], cs["p0"],
                                  cs["H"], cs["Hkv"], cs["hd"], cs["ctx"], n_kv, ldo, out.ctypes.data)
    return r, out, G.last_error()


def _check(name, p0, T, ctx, H, Hkv, base="cancel_kq"):
    cs = A.make(name, T, p0, H, Hkv, 256, ctx, base=base)
    ref = A.oracle_out(cs)
    r, out, why = _run(cs, _n_kv(p0, T, ctx))
    assert r == 0, why
    assert (out[:, H * 256:] == SENTINEL).all(), "padding columns of out were written"
    bad = np.argwhere(out[:, :H * 256].view(U32) != ref.view(U32))
    if len(bad) == 0:
        return None
    t, col = (int(x) for x in bad[0])
    return (f"{name} (base {base}) H {H} Hkv {Hkv} p0 {p0} T {T} ctx {ctx}: {len(bad)} of {ref.size} words differ; first at "
            f"row {t} (position {p0 + t}) head {col // 256} dim {col % 256}: got {out[t, col]!r} want {ref[t, col]!r}; "
            f"rows hit {sorted(set(bad[:, 0].tolist()))[:12]}")


@pytest.mark.parametrize("name", A.CASES)
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_attn_mx_long_equals_the_oracle(H, Hkv, name):
    """every case at ctx 4096; the two cancellation cases at ctx 8192 for the one-kv-head shapes"""
    wide = (H, Hkv) in ((8, 1), (16, 1)) and name in ("cancel_kq", "cancel_kqv")
    fails = [_check(name, p0, T, ctx, H, Hkv) for p0, T, ctx in GEOMS if ctx == 4096 or wide]
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails[:6])


def test_attn_mx_long_with_stale_caches_of_every_base():
    """finite garbage past the last row: the KQV multiplies it by P16 = 0 over (sp, L_blk)"""
    fails = [_check("stale", p0, T, 4096, H, Hkv, base) for H, Hkv in [(8, 1), (4, 2)]
             for p0, T in [(2550, 20), (4070, 26)] for base in ("cancel_kqv", "underflow", "benign")]
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails[:6])


@pytest.mark.parametrize("shape,reason", [
    (dict(hd=64), "head_dim != 256"),
    (dict(H=3, Hkv=1), "query heads per kv head must divide 16"),
    (dict(ctx=336), "n_ctx and n_kv must be multiples of 32"),
    (dict(n_kv=40), "n_ctx and n_kv must be multiples of 32"),
    (dict(n_kv=352), "n_kv > n_ctx"),
    (dict(ctx=8224), "n_ctx > 8192"),
    (dict(n_kv=32), "rows past n_kv")])
def test_attn_mx_long_refusals_start_nothing(shape, reason):
    g = dict(dict(H=4, Hkv=2, hd=256, ctx=320, n_kv=64), **shape)
    cs = A.make("benign", 6, 27, g["H"], g["Hkv"], g["hd"], g["ctx"])
    r, out, why = _run(cs, g["n_kv"])
    assert r != 0 and why == "attn_mx_long: " + reason, (r, why)
    assert (out == SENTINEL).all()


# ---- through the engine: a 5,100-token prompt on the G = 8 tiny shape (n_kv 5120 > the row form's 4992) ----
G8 = dict(n_layer=2, n_embd=2048, n_head=8, n_head_kv=1, head_dim=256, n_ff=2048, n_vocab=4096)
N_CTX, N_PROMPT, CHUNKS, N_DECODE, N_VERIFY = 5152, 5100, (2500, 2100, 500), 3, 3


@functools.lru_cache(maxsize=None)
def _token_by_token():
    """engine B: the prompt and the N_DECODE + N_VERIFY + 1 greedy tokens after it through step (the decode
    path's split attention and matvecs) -> (logits rows of every position, the sequence).  Read-only."""
    import gemma_hip as G
    prompt = O.make_prompt(N_PROMPT, G8["n_vocab"])
    e = G.Engine(G8, n_ctx=N_CTX, device=0)
    e.begin(prompt)
    rows = e.step(N_PROMPT + N_DECODE + N_VERIFY + 1, want_logits=True, use_graph=True)
    seq = [int(t) for t in e.tokens()]
    e.close()
    rows.setflags(write=False)
    return rows, seq


def _rows_equal(got, ref, what):
    bad = np.nonzero((np.atleast_2d(got).view(U32) != np.atleast_2d(ref).view(U32)).any(axis=1))[0]
    assert bad.size == 0, (what, "rows", bad[:8])


@pytest.mark.parametrize("att_mx", [1, 2])
def test_long_prompt_in_chunks_equals_token_by_token(att_mx):
    """att_mx 1: the passes take k_attn_mx, the key-split form, the key-split form; 2: the key-split form in all
    three and in the verify pass"""
    import gemma_hip as G
    rows, seq = _token_by_token()
    e = G.Engine(G8, n_ctx=N_CTX, device=0)
    e.set_option("att_mx", att_mx)
    e.begin(seq[:N_PROMPT])
    for i, n in enumerate(CHUNKS):
        p0 = e.pos()
        tok, last, allv = e.prefill_next(n, want_all=True)
        if i > 0:
            _rows_equal(allv, rows[p0:p0 + n], f"pass at p0 = {p0}")
    lg = e.step(N_DECODE, want_logits=True, use_graph=True)
    _rows_equal(lg, rows[N_PROMPT:N_PROMPT + N_DECODE], "decode after the passes")
    p = e.pos()
    toks, allv = e.verify(seq[p + 1:p + 1 + N_VERIFY], want_all=True)
    assert toks == seq[p + 1:p + 2 + N_VERIFY], (toks, seq[p + 1:p + 2 + N_VERIFY])
    _rows_equal(allv, rows[p:p + N_VERIFY + 1], "verify pass")
    assert [int(t) for t in e.tokens()] == seq
    e.close()
