"""The marshalling of the decode kernels' leading scalar parameters (launch front).

k_matvec, k_matvec_rr and k_attn_head take the fields their first loads are addressed with as scalar
parameters in front of the argument struct; the launchers fill them from the struct.  The parity
suite proves the arithmetic; these cases make every such argument distinguishable (gate != up, x !=
norm_w, nb != n_bt, strides that differ from the row length, H != Hkv != dsplit ...), at the smallest
shapes each form accepts, bit for bit against the oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O

gpu = pytest.mark.gpu

PRO_F32, PRO_NORM, PRO_EMBED, PRO_IMG = 0, 1, 3, 4
EPI_STORE, EPI_ADD, EPI_GELU_MUL, EPI_ARGMAX = 0, 1, 2, 3
KS_RR = 9
EPS = 1e-6


class MatvecArgs(C.Structure):
    """struct gemma_test_matvec_args (include/gemma_hpc.h)."""
    _fields_ = [("type", C.c_int), ("ks", C.c_int), ("pro", C.c_int), ("epi", C.c_int), ("ncols", C.c_int),
                ("grid", C.c_int), ("rows", C.c_int64), ("K", C.c_int64), ("W", C.c_void_p), ("W2", C.c_void_p),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("x_da", C.c_void_p), ("norm_w", C.c_void_p),
                ("eps", C.c_float), ("emb_scale", C.c_float), ("n_tok", C.c_int), ("tok_pos", C.c_int),
                ("emb", C.c_void_p), ("emb_rows", C.c_int64), ("emb_out", C.c_void_p), ("resid", C.c_void_p),
                ("y_stride", C.c_int64), ("y", C.c_void_p), ("keys", C.c_void_p)]


def _entry():
    import gemma_hip as G
    L = G.lib()
    L.gemma_test_matvec.restype = C.c_int
    L.gemma_test_matvec.argtypes = [C.POINTER(MatvecArgs)]
    return G, L


def _weights(rng, wtype, rows, K):
    w = (rng.standard_normal((rows, K)) * 0.05).astype(np.float32)
    return O.quantize(w, "q4_0_ref" if wtype == O.Q4_0 else "q8_0_ref")


def _rms_norm_mul(x, w):
    y = np.zeros_like(x)
    O.lib().orc_rms_norm(O.ptr(x), O.ptr(y), x.size, EPS)
    return y * w  # ggml_mul, f32


def _image(q8):
    """block_q8_0 row [nb][34] -> the activation image (csrc/device_util.h): dword ((b>>2)*8 + l)*4 + (b&3)
    holds int8 elements 4l..4l+3 of block b; da[b] = f32(d)."""
    nb = q8.size // 34
    blk = q8.reshape(nb, 34)
    da = blk[:, :2].copy().view(np.float16).astype(np.float32).ravel()
    qs = blk[:, 2:].copy().view(np.uint32).reshape(nb, 8)  # [b][l]
    act = np.zeros(nb * 8, dtype=np.uint32)
    b = np.arange(nb)[:, None]
    l = np.arange(8)[None, :]
    act[(((b >> 2) * 8 + l) * 4 + (b & 3)).ravel()] = qs.ravel()
    return act, da


def _gelu(v):
    tab = np.ctypeslib.as_array(C.cast(O.lib().orc_table_gelu_f16(), C.POINTER(C.c_uint16)), shape=(65536,))
    return tab[v.astype(np.float16).view(np.uint16)].view(np.float16).astype(np.float32)


def _run(wtype, ks, pro, epi, rows, K, ncols, grid, seed):
    """one launch through gemma_test_matvec and its reference from the oracle's pieces"""
    G, L = _entry()
    rng = np.random.default_rng(seed)
    W = _weights(rng, wtype, rows, K)
    W2 = _weights(rng, wtype, rows, K) if epi == EPI_GELU_MUL else None
    x_stride = K + 32 if ncols > 1 else K  # floats between columns: not the row length
    y_stride = rows + 5 if ncols > 1 else rows
    norm_w = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    t = MatvecArgs(type=wtype, ks=ks, pro=pro, epi=epi, ncols=ncols, grid=grid, rows=rows, K=K, W=W.ctypes.data,
                   x_stride=x_stride, y_stride=y_stride, eps=EPS, emb_scale=1.0)
    keep = [W, W2, norm_w]
    if W2 is not None:
        t.W2 = W2.ctypes.data
    # the activation columns the kernel should see, as f32 before the Q8_0 quantization
    if pro in (PRO_F32, PRO_NORM):
        xbuf = rng.standard_normal((ncols - 1) * x_stride + K).astype(np.float32)
        cols = [xbuf[c * x_stride: c * x_stride + K] for c in range(ncols)]
        if pro == PRO_NORM:
            cols = [_rms_norm_mul(np.ascontiguousarray(c), norm_w) for c in cols]
            t.norm_w = norm_w.ctypes.data
        q8 = [O.quantize(np.ascontiguousarray(c)[None], "q8_0")[0] for c in cols]
    elif pro == PRO_EMBED:
        emb_rows, n_tok, tok_pos = 24, 5, 3
        emb = _weights(rng, wtype, emb_rows, K)
        xbuf = rng.integers(0, emb_rows, n_tok).astype(np.int32)
        xbuf[tok_pos] = 17  # not row 0, and not what a wrong tok_pos would find
        xbuf[0] = 2
        scale = np.float32(3.5)
        row = O.dequantize(wtype, emb[17], K) * scale
        emb_out = np.zeros(K, dtype=np.float32)
        t.n_tok, t.tok_pos, t.emb, t.emb_rows, t.emb_scale = n_tok, tok_pos, emb.ctypes.data, emb_rows, float(scale)
        t.emb_out, t.norm_w = emb_out.ctypes.data, norm_w.ctypes.data
        keep += [emb, emb_out]
        q8 = [O.quantize(_rms_norm_mul(row, norm_w)[None], "q8_0")[0]] * ncols
    else:  # PRO_IMG: one image, the same column for every output column
        v = rng.standard_normal(K).astype(np.float32)
        q = O.quantize(v[None], "q8_0")[0]
        xbuf, da = _image(q)
        t.x_da = da.ctypes.data
        keep.append(da)
        q8 = [q] * ncols
    t.x = xbuf.ctypes.data
    n_y = (ncols - 1) * y_stride + rows
    y = np.zeros(n_y, dtype=np.float32)
    resid = rng.standard_normal(n_y).astype(np.float32)
    keys = np.zeros(grid * ncols, dtype=np.uint64)
    t.y = y.ctypes.data
    if epi == EPI_ADD:
        t.resid = resid.ctypes.data
    if epi == EPI_ARGMAX:
        t.keys = keys.ctypes.data
    r = L.gemma_test_matvec(C.byref(t))
    assert r == 0, G.last_error()

    wdata = np.ascontiguousarray(np.stack(q8))
    row_bytes = W.shape[1]
    ref = O.mul_mat(W, wtype, rows, row_bytes, K, wdata, wdata.shape[1], ncols)
    if epi == EPI_GELU_MUL:
        up = O.mul_mat(W2, wtype, rows, row_bytes, K, wdata, wdata.shape[1], ncols)
        ref = _gelu(ref) * up
    for c in range(ncols):
        want = ref[c] + resid[c * y_stride: c * y_stride + rows] if epi == EPI_ADD else ref[c]
        got = y[c * y_stride: c * y_stride + rows]
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"column {c}: {bad.size} of {rows} rows differ, first {bad[:5]}"
        if c + 1 < ncols:  # the gap between columns stays untouched
            assert not y[c * y_stride + rows: (c + 1) * y_stride].any()
        if epi == EPI_ARGMAX:
            best = int(keys[c * grid: (c + 1) * grid].max())
            assert 0xFFFFFFFF - (best & 0xFFFFFFFF) == int(np.argmax(ref[c])), "argmax key names another row"
    if pro == PRO_EMBED:
        assert np.array_equal(emb_out.view(np.uint32), row.view(np.uint32)), "emb_out is not the scaled embedding row"
    del keep


_RR_K = {}


def _smallest_rr_k(wtype):
    """the smallest K (K % 128 == 0, so that the image form takes it too) the round-pipelined form accepts:
    launch_matvec refuses the others before launching anything (matvec_rr_supported)"""
    if wtype not in _RR_K:
        G, L = _entry()
        rng = np.random.default_rng(1)
        for K in range(128, 4097, 128):
            W = _weights(rng, wtype, 8, K)
            x = np.zeros(K, dtype=np.float32)
            y = np.zeros(8, dtype=np.float32)
            t = MatvecArgs(type=wtype, ks=KS_RR, pro=PRO_F32, epi=EPI_STORE, ncols=1, grid=1, rows=8, K=K,
                           W=W.ctypes.data, x=x.ctypes.data, x_stride=K, y_stride=8, y=y.ctypes.data)
            if L.gemma_test_matvec(C.byref(t)) == 0:
                _RR_K[wtype] = K
                break
            assert "matvec(rr)" in G.last_error(), G.last_error()
        assert wtype in _RR_K, "no K up to 4096 takes the round-pipelined form"
    return _RR_K[wtype]


TYPES = pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])
NCOLS = pytest.mark.parametrize("ncols", [1, 2])


@gpu
@TYPES
@NCOLS
@pytest.mark.parametrize("K,grid", [(160, 2), (2048, 4)], ids=["strided", "scale_runs"])
def test_matvec_norm_gelu_mul(wtype, ncols, K, grid):
    """gate/up: 13 row tiles; 2 workgroups take them in two strided passes (rt_q 1, rt_r 5), 4 give every
    wave at most one (rt_q 0, rt_r 13) and, at K 2048, the scale-run form the decode step runs"""
    _run(wtype, 1, PRO_NORM, EPI_GELU_MUL, rows=100, K=K, ncols=ncols, grid=grid, seed=11)


@gpu
@TYPES
@NCOLS
def test_matvec_norm_argmax(wtype, ncols):
    _run(wtype, 1, PRO_NORM, EPI_ARGMAX, rows=100, K=160, ncols=ncols, grid=3, seed=12)


@gpu
@TYPES
@NCOLS
@pytest.mark.parametrize("pro,epi", [(PRO_NORM, EPI_STORE), (PRO_EMBED, EPI_STORE), (PRO_F32, EPI_ADD), (PRO_IMG, EPI_ADD)],
                         ids=["norm", "embed", "f32_add", "img_add"])
def test_matvec_rr(wtype, ncols, pro, epi):
    """the round-pipelined form at its smallest K; 20 rows = 3 workgroups, the last with 4 rows"""
    _run(wtype, KS_RR, pro, epi, rows=20, K=_smallest_rr_k(wtype), ncols=ncols, grid=1, seed=13 + pro)


# K-split carry: the smallest (ks, K) of each chunk count class.  The carrier chains (ks-1) * n_bt / ks
# chunks (a block tile: K 256 for Q4_0, 128 for Q8_0): whole ring turns of 4, then 0-3 remaining chunks.
_CARRY = {  # chunk count -> (ks, K) for (Q4_0, Q8_0)
    1: ((2, 512), (2, 256)),     # remainder only
    2: ((2, 1024), (2, 512)),
    3: ((4, 1024), (4, 512)),
    4: ((2, 2048), (2, 1024)),   # ring only
    7: ((8, 2048), (8, 1024)),   # ring + 3; the ks 8 LDS map (without the ns plane)
}


@gpu
@TYPES
@NCOLS
@pytest.mark.parametrize("chunks", sorted(_CARRY), ids=[f"chunks{c}" for c in sorted(_CARRY)])
@pytest.mark.parametrize("pro,epi", [(PRO_F32, EPI_ADD), (PRO_NORM, EPI_STORE)], ids=["f32_add", "norm_store"])
def test_matvec_ksplit_carry(wtype, ncols, chunks, pro, epi):
    """13 rows = two row tiles, the second partial; one workgroup takes both through the refilled ring"""
    ks, K = _CARRY[chunks][0 if wtype == O.Q4_0 else 1]
    _run(wtype, ks, pro, epi, rows=13, K=K, ncols=ncols, grid=1, seed=20 + chunks)


def _attn_case(rng, pos, H, Hkv, hd, ctx):
    qkv = rng.standard_normal((H + 2 * Hkv) * hd).astype(np.float32)
    kvw = Hkv * hd
    kc = np.zeros(ctx * kvw, dtype=np.uint16)
    kc[: pos * kvw] = rng.standard_normal(pos * kvw).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((kvw, ctx)).astype(np.float16).view(np.uint16)
    vc[:, pos:] = 0
    return qkv, kc, vc.ravel().copy()


@gpu
@pytest.mark.parametrize("H,Hkv,mode", [(4, 1, 2), (6, 2, 0), (6, 2, 2)], ids=["mqa_d2", "gqa_g3", "gqa_g3_d2"])
def test_attn_head_geometry(H, Hkv, mode):
    """the per-head decode attention with H, Hkv, hd, ctx and the dim split all different, at two
    positions a 32-boundary apart (the padded key count differs)"""
    import gemma_hip as G
    L = G.lib()
    L.gemma_test_attn_decode.restype = C.c_int
    L.gemma_test_attn_decode.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_float] + [C.c_void_p] * 5 + [C.c_int]
    OL = O.lib()
    OL.orc_attn_decode.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_float] + [C.c_void_p] * 4
    hd, ctx = 64, 128
    rng = np.random.default_rng(H * 10 + Hkv)
    for pos in (20, 52):
        qkv, kc, vc = _attn_case(rng, pos, H, Hkv, hd, ctx)
        k1, v1, k2, v2 = kc.copy(), vc.copy(), kc.copy(), vc.copy()
        ref = np.zeros(H * hd, dtype=np.float32)
        got = np.zeros(H * hd, dtype=np.float32)
        OL.orc_attn_decode(qkv.ctypes.data, k1.ctypes.data, v1.ctypes.data, pos, H, Hkv, hd, ctx, 10000.0,
                           ref.ctypes.data, None, None, None)
        r = L.gemma_test_attn_decode(qkv.ctypes.data, k2.ctypes.data, v2.ctypes.data, pos, H, Hkv, hd, ctx, 10000.0,
                                     got.ctypes.data, None, None, None, None, mode)
        assert r == 0, G.last_error()
        assert np.array_equal(k1, k2) and np.array_equal(v1, v2), f"cache update differs at pos {pos}"
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"attention output differs at pos {pos}"


@gpu
def test_engine_two_layers_graph_tokens():
    """a 2-layer engine whose qkv, attn-out and down take the round-pipelined form (K 2048 everywhere),
    GQA: 8 graph-replayed tokens bit-identical to the oracle"""
    import gemma_hip as G
    shape = dict(n_layer=2, n_embd=2048, n_head=8, n_head_kv=2, head_dim=256, n_ff=2048, n_vocab=4096)
    n_prompt, n_decode = 3, 8
    m = O.Model(O.make_config(shape, n_ctx=64))
    prompt = O.make_prompt(n_prompt, shape["n_vocab"])
    seq_ref, lg_ref = m.generate(prompt, n_decode)
    e = G.Engine(shape, n_ctx=64)
    e.begin(prompt)
    lg = e.step(n_prompt + n_decode, want_logits=True, use_graph=True)
    toks = list(e.tokens()[: len(seq_ref)])
    e.close()
    assert toks == list(seq_ref)
    assert np.array_equal(lg[n_prompt - 1:].view(np.uint32), lg_ref.view(np.uint32))


@gpu
def test_ablate_option_needs_the_variant_build():
    """the product kernels do not read mv_args::ablate: asking for an ablation is an error, not a
    silently unablated timing"""
    import gemma_hip as G
    e = G.Engine(O.TINY, n_ctx=64)
    try:
        e.set_option("ablate", 0)
        with pytest.raises(RuntimeError, match="built without -DGHIP_ABLATE"):
            e.set_option("ablate", 1)
    finally:
        e.close()
