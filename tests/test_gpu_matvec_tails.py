"""The launch tails of the decode matvecs (launch tail), bit for bit against the oracle.

EPI_ADD: the round-pipelined form (ks 9) and the K-split carry form (ks 8) load the residual of the row a
lane will store behind the activation loads and add it from a register at the end.  The cases make a wrong
row, column or guard visible: a residual that differs per element and per column, a column stride that is
not the row count, a ragged last row tile, one round and the deepest ring.

EPI_GELU_MUL: the scale-run form runs its row tile matrix-major and looks the GELU table up once, in the
middle of the stream, with the clamp cases as selects; the strided pair form looks it up once as well.
Gate values in the table's dense range, beyond +-10 (the clamp's cases) and past the f16 range; y and the
Q8_0 image of y.  (A block of y that holds an infinity or a NaN has no defined Q8_0 image, the conversion
of a NaN to an integer is not defined: the image is compared on the blocks whose reference values are all
finite, y on every row.)"""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_kernarg_args import (EPI_ADD, EPI_GELU_MUL, EPS, KS_RR, PRO_F32, PRO_IMG, PRO_NORM, MatvecArgs, _gelu,
                                   _image, _rms_norm_mul, _weights)

gpu = pytest.mark.gpu

TYPES = pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])


def _entry():
    import gemma_hip as G
    L = G.lib()
    L.gemma_test_matvec_tail.restype = C.c_int
    L.gemma_test_matvec_tail.argtypes = [C.POINTER(MatvecArgs), C.c_int, C.c_void_p, C.c_void_p]
    return G, L


def _bits_equal(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}"


_ADD_REF = {}


def _add_case(wtype, pro, K, rows, ncols):
    """weights, activation columns and residual of one EPI_ADD case with the oracle's result; shared by the
    two forms (ks 9, ks 8) and left unchanged"""
    key = (wtype, pro, K, rows, ncols)
    if key not in _ADD_REF:
        rng = np.random.default_rng(1000 + K + 17 * rows + 3 * ncols + pro + wtype)
        W = _weights(rng, wtype, rows, K)
        x_stride = K + 32
        y_stride = rows + 5
        if pro == PRO_F32:
            xbuf = rng.standard_normal((ncols - 1) * x_stride + K).astype(np.float32)
            q8 = [O.quantize(np.ascontiguousarray(xbuf[c * x_stride: c * x_stride + K])[None], "q8_0")[0] for c in range(ncols)]
            da = None
        else:  # one image, the same column for every output column
            q = O.quantize(rng.standard_normal(K).astype(np.float32)[None], "q8_0")[0]
            xbuf, da = _image(q)
            q8 = [q] * ncols
        n_y = (ncols - 1) * y_stride + rows
        resid = rng.standard_normal(n_y).astype(np.float32)
        wdata = np.ascontiguousarray(np.stack(q8))
        ref = O.mul_mat(W, wtype, rows, W.shape[1], K, wdata, wdata.shape[1], ncols)
        want = [ref[c] + resid[c * y_stride: c * y_stride + rows] for c in range(ncols)]
        _ADD_REF[key] = (W, xbuf, da, resid, x_stride, y_stride, want)
    return _ADD_REF[key]


@gpu
@TYPES
@pytest.mark.parametrize("ks", [KS_RR, 8], ids=["rr", "ks8"])
@pytest.mark.parametrize("pro", [PRO_F32, PRO_IMG], ids=["f32", "img"])
@pytest.mark.parametrize("K", [2048, 16384])
@pytest.mark.parametrize("rows", [8, 24, 13])
@pytest.mark.parametrize("ncols", [1, 2])
def test_add_residual_from_a_register(wtype, ks, pro, K, rows, ncols):
    _add_run(wtype, ks, pro, K, rows, ncols, (rows + 7) // 8)


@gpu
@TYPES
@pytest.mark.parametrize("pro", [PRO_F32, PRO_IMG], ids=["f32", "img"])
@pytest.mark.parametrize("K", [2048, 16384])
@pytest.mark.parametrize("rows", [24, 13])
def test_add_ksplit_one_workgroup_many_row_tiles(wtype, pro, K, rows):
    """the K-split form with one workgroup for all row tiles: the residual of every row tile after the
    first is loaded when the tile before it is stored"""
    _add_run(wtype, 8, pro, K, rows, 2, 1)


def _add_run(wtype, ks, pro, K, rows, ncols, grid):
    G, L = _entry()
    W, xbuf, da, resid, x_stride, y_stride, want = _add_case(wtype, pro, K, rows, ncols)
    y = np.zeros(resid.size, dtype=np.float32)
    t = MatvecArgs(type=wtype, ks=ks, pro=pro, epi=EPI_ADD, ncols=ncols, grid=grid, rows=rows, K=K,
                   W=W.ctypes.data, x=xbuf.ctypes.data, x_stride=x_stride, y_stride=y_stride, eps=EPS, emb_scale=1.0,
                   resid=resid.ctypes.data, y=y.ctypes.data)
    if da is not None:
        t.x_da = da.ctypes.data
    r = L.gemma_test_matvec_tail(C.byref(t), 0, None, None)
    assert r == 0, G.last_error()
    for c in range(ncols):
        _bits_equal(y[c * y_stride: c * y_stride + rows], want[c], f"column {c}")
        # the gap behind a column stays untouched
        assert not y[c * y_stride + rows: (c + 1) * y_stride].any()


_GELU_REF = {}


def _gelu_case(wtype, rows, scale):
    key = (wtype, rows, scale)
    if key not in _GELU_REF:
        K = 2048
        rng = np.random.default_rng(2000 + rows + wtype)
        W, W2 = _weights(rng, wtype, rows, K), _weights(rng, wtype, rows, K)
        x = rng.standard_normal(K).astype(np.float32)
        # the norm takes the scale of x out, so the scale goes into the norm's weight
        norm_w = ((1.0 + 0.1 * rng.standard_normal(K)) * scale).astype(np.float32)
        q8 = O.quantize(_rms_norm_mul(x, norm_w)[None], "q8_0")
        gate = O.mul_mat(W, wtype, rows, W.shape[1], K, q8, q8.shape[1], 1)[0]
        up = O.mul_mat(W2, wtype, rows, W.shape[1], K, q8, q8.shape[1], 1)[0]
        _GELU_REF[key] = (W, W2, x, norm_w, gate, up)
    return _GELU_REF[key]


@gpu
@TYPES
@pytest.mark.parametrize("clamp", [0, 1], ids=["table", "clamp"])
@pytest.mark.parametrize("scale", [1.0, 8.0, 1e5], ids=["dense", "beyond10", "past_f16"])
@pytest.mark.parametrize("rows,grid", [(32, 1), (32, 2), (96, 3), (96, 1)],
                         ids=["1group", "idle_waves", "3wgs", "3groups_strided"])
def test_gelu_one_lookup(wtype, clamp, scale, rows, grid):
    """(32, 1) and (96, 3): every wave at most one row tile, the scale-run form of the decode step; (32, 2): the
    same form with a second workgroup whose waves own no row tile (they stream one tile again and must store
    nothing); (96, 1): one workgroup takes three row tiles per wave position, the strided pair form"""
    G, L = _entry()
    K = 2048
    W, W2, x, norm_w, gate, up = _gelu_case(wtype, rows, scale)
    absg = np.abs(gate)
    if scale == 1.0:
        assert (absg < 10).sum() > rows // 2
    elif scale == 8.0:
        assert (gate >= 10).any() and (gate <= -10).any() and (absg < 10).any()
    else:
        assert (absg > 65504).any()
    with np.errstate(all="ignore"):
        g = _gelu(gate)
        if clamp:
            g = np.where(gate <= -10.0, np.float32(0.0), np.where(gate >= 10.0, gate, g)).astype(np.float32)
        want = (g * up).astype(np.float32)
    y = np.zeros(rows, dtype=np.float32)
    ia = np.zeros((rows + 127) // 128 * 32, dtype=np.uint32)
    ida = np.zeros(rows // 32, dtype=np.float32)
    t = MatvecArgs(type=wtype, ks=1, pro=PRO_NORM, epi=EPI_GELU_MUL, ncols=1, grid=grid, rows=rows, K=K, W=W.ctypes.data,
                   W2=W2.ctypes.data, x=x.ctypes.data, x_stride=K, y_stride=rows, eps=EPS, emb_scale=1.0,
                   norm_w=norm_w.ctypes.data, y=y.ctypes.data)
    r = L.gemma_test_matvec_tail(C.byref(t), clamp, ia.ctypes.data, ida.ctypes.data)
    assert r == 0, G.last_error()
    _bits_equal(y, want, "y")
    finite = np.isfinite(want.reshape(-1, 32)).all(axis=1)
    # past the f16 range without the clamp every block may hold an infinity: then only y is compared
    assert finite.any() or scale == 1e5
    nb = rows // 32
    unused = np.ones(ia.size, dtype=bool)
    for b in range(nb):
        unused[((b >> 2) * 8 + np.arange(8)) * 4 + (b & 3)] = False
    assert not ia[unused].any(), "the image was written outside y's blocks"
    if finite.any():
        safe = np.where(np.repeat(finite, 32), want, np.float32(0.0)).astype(np.float32)
        qs, da = O.image_of(safe)
        for b in np.flatnonzero(finite):
            got = ia[((b >> 2) * 8 + np.arange(8)) * 4 + (b & 3)]
            assert np.array_equal(got, qs[b]), f"image block {b} differs"
            assert ida[b:b + 1].view(np.uint32) == da[b:b + 1].view(np.uint32), f"image scale of block {b} differs"


@gpu
@pytest.mark.parametrize("down_img", [0, 1], ids=["f32", "image"])
def test_engine_one_layer_gemma2b_widths(down_img):
    """one layer with Gemma-2B's widths (the shapes whose attn-out, gate/up and down take the changed forms), a
    small vocabulary: a 3-token prompt and 4 graph-replayed steps, every logit equal to the oracle's; the down
    matvec from f32 h and from gate/up's image of h"""
    import gemma_hip as G
    shape = dict(n_layer=1, n_embd=2048, n_head=8, n_head_kv=1, head_dim=256, n_ff=16384, n_vocab=256)
    n_prompt, n_decode = 3, 4
    m = O.Model(O.make_config(shape, n_ctx=64))
    prompt = O.make_prompt(n_prompt, shape["n_vocab"])
    seq_ref, lg_ref = m.generate(prompt, n_decode)
    e = G.Engine(shape, n_ctx=64)
    try:
        p = e.plan()
        p["down"] = (p["down"][0], p["down"][1], down_img)
        e.set_plan(p)
        assert e.plan()["down"][2] == down_img
        e.begin(prompt)
        lg = e.step(n_prompt + n_decode, want_logits=True, use_graph=True)
        toks = list(e.tokens()[: len(seq_ref)])
    finally:
        e.close()
    assert toks == list(seq_ref)
    assert np.array_equal(lg[n_prompt - 1:].view(np.uint32), lg_ref.view(np.uint32))
