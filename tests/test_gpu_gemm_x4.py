"""The exact prefill GEMM in its five forms (hpc_set_gemm_x4 modes 0-4, default 3: prefill.hip k_gemm_x, the
lane-masked W32 kernel, and k_gemm_x4, the K = 4 multi-block MFMA kernel with 32 x 64 or 64 x 32 tiles,
staged from the f16 or the int8 image): bit-identical to mul_mat's AVX2 lane order (the oracle's
restatement of src/hpc.cpp:15-41 over ggml's vec_dot_q4_0_q8_0 / q8_0_q8_0) at ragged shapes, and whole
exact prefills (every prompt row's logits, the decode that continues from the cache) equal to the oracle
and to the W32 form.  Modes outside 0-4 are rejected and leave the form as it was."""
import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_prefill import _gemm, _prefill_exact_case

gpu = pytest.mark.gpu


DEFAULT = 3  # hpc_set_gemm_x4's default form


@pytest.fixture(params=[0, 1, 2, 3, 4], ids=["w32", "x4_32x64", "x4_64x32", "x4_i8", "x4_64x32_i8"])
def x4(request):
    """every exact GEMM form: the lane-masked W32 kernel (0), the K = 4 kernel with 32 rows x 64
    tokens (1) and 64 x 32 (2), and the same two staged from the int8 image (3, the default, and 4)"""
    import gemma_hip as G
    G.lib().hpc_set_gemm_x4(request.param)
    yield request.param
    G.lib().hpc_set_gemm_x4(DEFAULT)


@gpu
@pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])
@pytest.mark.parametrize("rows,K,T", [(64, 256, 64), (100, 512, 37), (72, 2048, 130), (2560, 2048, 96),
                                      (256, 16384, 70), (40, 96, 3), (8, 32, 1), (96, 1312, 65)])
def test_gemm_x4_bit_identical(x4, wtype, rows, K, T):
    import gemma_hip as G
    L = G.lib()
    rng = np.random.default_rng(rows * 13 + K + T)
    Wf = (rng.standard_normal((rows, K)) * 0.05).astype(np.float32)
    W = O.quantize(Wf, "q4_0_ref" if wtype == O.Q4_0 else "q8_0_ref")
    X = (rng.standard_normal((T, K)) * rng.uniform(0.1, 3.0, (T, 1))).astype(np.float32)
    X[0, :min(37, K)] = 0.0
    r, Y, xq, da = _gemm(L, wtype, W, X, rows, K, T, exact=True)
    assert r == 0, G.last_error()
    wdata, rs = O.mul_mat_init(wtype, X)
    ref = O.mul_mat(W, wtype, rows, W.shape[1], K, wdata, rs, T)
    assert np.array_equal(Y.view(np.uint32), ref.view(np.uint32)), np.abs(Y - ref).max()


@gpu
def test_gemm_x4_extreme_blocks(x4):
    """the isum bounds: Q8_0 weights and activations at +-127 / -128 (4 products of 128*128 = 65,536),
    Q4_0 nibbles 0 / 15 (-8 / +7), all in one row"""
    import gemma_hip as G
    L = G.lib()
    rows, K, T = 16, 256, 17
    for wtype, q in ((O.Q8_0, "q8_0_ref"), (O.Q4_0, "q4_0_ref")):
        Wf = np.zeros((rows, K), np.float32)
        Wf[0::2] = 1.0
        Wf[1::2] = -1.0
        Wf[3, ::3] = 0.01
        W = O.quantize(Wf, q)
        X = np.zeros((T, K), np.float32)
        X[0::2] = -1.0
        X[1::2] = 1.0
        X[5, 7::5] = 0.3
        r, Y, _, _ = _gemm(L, wtype, W, X, rows, K, T, exact=True)
        assert r == 0, G.last_error()
        wdata, rs = O.mul_mat_init(wtype, X)
        ref = O.mul_mat(W, wtype, rows, W.shape[1], K, wdata, rs, T)
        assert np.array_equal(Y.view(np.uint32), ref.view(np.uint32)), (wtype, np.abs(Y - ref).max())


@gpu
def test_mode_outside_0_to_4_is_rejected_and_leaves_the_form():
    """hpc_set_gemm_x4(5) and (-1) set the last-error text, which names the value, and change nothing:
    a 16 x 256 x 17 Q8_0 product still equals the oracle bit for bit from the default form, and, from
    mode 1 (the f16 image alone is written), so does a whole exact prefill, the path on which a stored
    5 made the quantizer write the f16 image while the GEMM read the int8 one."""
    import gemma_hip as G
    L = G.lib()
    rows, K, T = 16, 256, 17
    rng = np.random.default_rng(5)
    W = O.quantize((rng.standard_normal((rows, K)) * 0.05).astype(np.float32), "q8_0_ref")
    X = rng.standard_normal((T, K)).astype(np.float32)
    wdata, rs = O.mul_mat_init(O.Q8_0, X)
    ref = O.mul_mat(W, O.Q8_0, rows, W.shape[1], K, wdata, rs, T)
    try:
        L.hpc_set_gemm_x4(DEFAULT)
        for bad in (5, -1):
            L.hpc_set_gemm_x4(bad)
            err = G.last_error()
            assert err != "" and str(bad) in err, (bad, err)
            r, Y, _, _ = _gemm(L, O.Q8_0, W, X, rows, K, T, exact=True)  # (a successful call clears the text)
            assert r == 0, G.last_error()
            assert G.last_error() == ""
            assert np.array_equal(Y.view(np.uint32), ref.view(np.uint32)), (bad, np.abs(Y - ref).max())
        # the engine's pass writes only the image its form stages from: a stored 5 would not survive this
        L.hpc_set_gemm_x4(1)
        for bad in (5, -1):
            L.hpc_set_gemm_x4(bad)
            assert str(bad) in G.last_error(), bad
        _prefill_exact_case(dict(O.TINY), 33, 128, n_decode=1)
    finally:
        L.hpc_set_gemm_x4(DEFAULT)


@gpu
def test_prefill_exact_x4_gemma2b_shapes(x4):
    _prefill_exact_case(dict(O.GEMMA_2B), 96, 256, n_decode=2)


@gpu
def test_prefill_exact_x4_q8_0_gqa(x4):
    _prefill_exact_case(dict(O.TINY, n_head=4, n_head_kv=2), 70, 256, wtype=O.Q8_0)


@gpu
def test_prefill_x4_full_size_equals_w32():
    """BASELINE config 3 at full size (Gemma-2B, T = 2048): the last row's logits and the decode that
    follows from each K = 4 form (modes 1-4) equal the lane-masked W32 form's (mode 0; all bit-exact
    restatements; a size-independent check)."""
    import gemma_hip as G
    T = 2048
    shape = dict(O.GEMMA_2B)
    prompt = O.make_prompt(T, shape["n_vocab"], seed=2)
    out = []
    try:
        for on in (0, 1, 2, 3, 4):
            G.lib().hpc_set_gemm_x4(on)
            e = G.Engine(shape, n_ctx=T + 64, device=0)
            e.begin(prompt)
            tok, last = e.prefill(T)
            out.append((tok, last, e.step(2, want_logits=True, use_graph=True)))
            e.close()
    finally:
        G.lib().hpc_set_gemm_x4(DEFAULT)
    for o in out[1:]:
        assert out[0][0] == o[0]
        assert np.array_equal(out[0][1].view(np.uint32), o[1].view(np.uint32))
        assert np.array_equal(out[0][2].view(np.uint32), o[2].view(np.uint32))
