"""The skinny exact K-quant GEMM (launch_gemm_skinny_kq through gemma_test_gemm_skinny_kq): for 1 <= T
<= 8 activation rows, Q4_K / Q6_K weights in ggml's layout and in the engine's lane-contiguous one, it
must equal the oracle's mul_mat (ggml's AVX2 lane order against the Q8_K INIT) bit for bit (uint32
views, no tolerance), with and without the residual epilogue; and an engine's skinny passes (verify,
a narrow batch pass) must leave the same bytes with the option "kq_skinny" 1 as with 0.

Shapes: one row group and one super-block (8, 256); a ragged last row group and a ragged K chunk
(37, 512); (100, 2048); (72, 4096); Gemma-2B's down projection K = 16384 (16 chunks through the double
buffer); 2056 rows = 257 row groups; and 8200 rows = 1025 row groups, past the launcher's threshold
(1021): four row groups per workgroup, a wave each, the last workgroup with three idle waves — below it
a workgroup's waves share one row group and divide the columns.  Inputs as in
test_kquant_mul_mat_bit_exact: rows scaled 0.1 .. 4, the first Q8_K block of row 0 all zero (d = 0)."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
from test_gpu_kquants import _extreme_blocks
from test_gpu_prefill_continue import KSHAPE

pytestmark = pytest.mark.gpu

SHAPES = [(8, 256), (37, 512), (100, 2048), (72, 4096), (264, 16384), (2056, 256), (8200, 256)]
T_MAX = 8
CASES = [(w, r, K, t) for w in (O.Q4_K, O.Q6_K) for r, K in SHAPES for t in (0, 1) if not (t and w == O.Q6_K and K % 2048)]


@functools.lru_cache(maxsize=None)
def _case(wtype, rows, K, extreme=False):
    """weights, 8 input rows, a residual and the oracle's product of all 8 columns, shared by the T and
    layout cases (column t of mul_mat does not depend on the other columns); read-only"""
    W = O.synth_kquant(wtype, rows * 31 + K, rows, K)
    rng = np.random.default_rng(rows + K + wtype)
    X = (rng.standard_normal((T_MAX, K)) * rng.uniform(0.1, 4.0, (T_MAX, 1))).astype(np.float32)
    X[0, :256] = 0.0
    if extreme:  # |isum| at its bound: columns of equal activations quantize to -128 everywhere
        W = _extreme_blocks(wtype, W, K)
        X[1], X[2], X[3, ::2] = 1.0, -1.0, 1.0
    R = rng.standard_normal((T_MAX, rows)).astype(np.float32)
    wdata, rs = O.mul_mat_init(wtype, X)
    ref = O.mul_mat(W, wtype, rows, W.shape[1], K, wdata, rs, T_MAX)
    for a in (W, X, R, ref):
        a.setflags(write=False)
    return W, X, R, ref


def _check(wtype, rows, K, tiled, T, extreme=False):
    W, X, R, ref = _case(wtype, rows, K, extreme)
    y = G.gemm_skinny_kq(wtype, W, rows, X[:T], tiled=tiled)
    assert np.array_equal(y.view(np.uint32), ref[:T].view(np.uint32)), np.abs(y - ref[:T]).max()
    ya = G.gemm_skinny_kq(wtype, W, rows, X[:T], resid=R[:T], tiled=tiled)
    assert np.array_equal(ya.view(np.uint32), (ref[:T] + R[:T]).view(np.uint32)), "+ resid (f32 add)"


@pytest.mark.parametrize("wtype,rows,K,tiled", CASES)
@pytest.mark.parametrize("T", [1, 2, 3, 5, 8])
def test_skinny_kq_bit_identical(wtype, rows, K, tiled, T):
    _check(wtype, rows, K, tiled, T)


@pytest.mark.parametrize("wtype", [O.Q4_K, O.Q6_K], ids=["q4_K", "q6_K"])
def test_skinny_kq_extreme_blocks(wtype):
    _check(wtype, 96, 4096, 1, 5, extreme=True)


def test_skinny_kq_refusals():
    W = O.synth_kquant(O.Q6_K, 1, 8, 512)
    for T, K, tiled, why in ((0, 512, 0, "outside"), (9, 512, 0, "outside"), (2, 200, 0, "K % 256"), (2, 512, 1, "K % 2048")):
        with pytest.raises(RuntimeError, match=why):
            G.gemm_skinny_kq(O.Q6_K, W, 8, np.zeros((T, K), np.float32), tiled=tiled)


@pytest.mark.parametrize("shape,kw", [(KSHAPE, dict(wtype=G.GGML_TYPE_Q4_K)), (dict(O.TINY), dict(out_type=G.GGML_TYPE_Q6_K))],
                         ids=["kquant_layers", "q6K_output"])
@pytest.mark.parametrize("dual", [0, 1])
def test_engine_skinny_passes_same_bytes(shape, kw, dual):
    """verify passes with k = 1, 2, 4, 7 and batch steps of 3 slots: logits rows, tokens and the KV
    caches are byte-identical between kq_skinny 0 and 1"""
    n, V = 20, shape["n_vocab"]
    prompt = [int(t) for t in O.make_prompt(n, V)]
    got = []
    for skinny in (0, 1):
        e = G.Engine(dict(shape), n_ctx=128, device=0, **kw)
        e.set_option("kq_dual", dual)
        e.set_option("kq_skinny", skinny)
        e.begin(prompt)
        e.prefill(n)
        out = []
        for k in (1, 2, 4, 7):
            toks, rows = e.verify([(3 * k + i) % V for i in range(k)], want_all=True)
            out += [np.array(toks), rows]
        out += [np.array(e.tokens())] + [x for il in range(shape["n_layer"]) for x in e.kv_read(il, 0, e.pos())]
        e.batch_open(3)
        for s in range(3):
            e.batch_begin(s, prompt[:5 + s])
        out.append(e.batch_step(9, want_logits=True))
        out += [x for s in range(3) for x in e.batch_kv_read(s, shape["n_layer"] - 1, 0, e.batch_pos(s))] + [e.batch_tokens(s) for s in range(3)]
        e.close()
        got.append(out)
    assert len(got[0]) == len(got[1])
    for i, (a, b) in enumerate(zip(*got)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), i
