"""Every device and pinned allocation has an owner (csrc/dev_mem.h): whatever a cycle of work
allocates is freed by the end of the cycle.

gemma_hip_mem_live() counts the live allocations of the whole library.  Each test runs one cycle of
work twice and compares the count and the bytes after the second cycle with those after the first:
process-lifetime tables and scratch (the executor's GELU and RoPE tables, the C-ABI scratch and host
stage) may come into being during the first cycle, a leak would show as growth in the second.  While
the owner is open the count must lie above the value after it closed, so a counter stuck at one
value cannot pass."""
import ctypes as C
import gc

import numpy as np
import pytest

import gemma_hip as G
import ggml_ctypes as X
import oracle_ctypes as O
from test_gpu_ggml_ops import activations, quant_weight
from test_gpu_prefill import _gemm

pytestmark = pytest.mark.gpu

N_CTX = 128
# the K-quant shape of tests/test_gpu_prefill_continue.py
KSHAPE = dict(n_layer=2, n_embd=256, n_head=2, n_head_kv=1, head_dim=128, n_ff=512, n_vocab=1024)

ENGINES = {
    "q4_0": (dict(O.TINY), dict(wtype=O.Q4_0)),
    "q8_0": (dict(O.TINY), dict(wtype=O.Q8_0)),
    "q6K_output": (dict(O.TINY), dict(out_type=G.GGML_TYPE_Q6_K)),
    "kquant_layers": (KSHAPE, dict(wtype=G.GGML_TYPE_Q4_K)),
    "virtual_tp2": (dict(O.TINY), dict(tp=(2, 0, None))),
}


def _hooks():
    """the gemma_test_* entry points, each on the smallest input it accepts"""
    L = G.lib()
    rng = np.random.default_rng(3)
    L.gemma_test_exp_f16.restype = C.c_int
    L.gemma_test_exp_f16.argtypes = [C.c_void_p]
    tab = np.zeros(65536, np.uint16)
    assert L.gemma_test_exp_f16(tab.ctypes.data) == 0, G.last_error()
    L.gemma_test_rms_norm.restype = C.c_int
    L.gemma_test_rms_norm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    x = rng.standard_normal((3, 256)).astype(np.float32)
    w = np.ones(256, np.float32)
    out = np.zeros((3, 256), np.float32)
    assert L.gemma_test_rms_norm(0, x.ctypes.data, None, 3, 256, 1e-6, out.ctypes.data) == 0, G.last_error()
    q8k = np.zeros((3, 292), np.uint8)
    assert L.gemma_test_rms_norm(1, x.ctypes.data, w.ctypes.data, 3, 256, 1e-6, q8k.ctypes.data) == 0, G.last_error()
    L.gemma_test_attn_decode.restype = C.c_int
    L.gemma_test_attn_decode.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_float] + [C.c_void_p] * 5 + [C.c_int]
    H, Hkv, hd, ctx, pos = 2, 1, 256, 512, 5
    qkv = rng.standard_normal((H + 2 * Hkv) * hd).astype(np.float32)
    kc = np.zeros(ctx * Hkv * hd, np.uint16)
    vc = np.zeros(ctx * Hkv * hd, np.uint16)
    att = np.zeros(H * hd, np.float32)
    dw = np.zeros(H * ctx, np.float32)
    dp = np.zeros(H * ctx, np.uint16)
    for mode in (0, 1):  # per head; the split form with its hand-off scratch
        r = L.gemma_test_attn_decode(qkv.ctypes.data, kc.ctypes.data, vc.ctypes.data, pos, H, Hkv, hd, ctx, 10000.0,
                                     att.ctypes.data, dw.ctypes.data, dp.ctypes.data, None, None, mode)
        assert r == 0, G.last_error()
    L.gemma_test_rope_kv_prefill.restype = C.c_int
    L.gemma_test_rope_kv_prefill.argtypes = [C.c_void_p, C.c_int64] + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 3
    L.gemma_test_attn_prefill.restype = C.c_int
    L.gemma_test_attn_prefill.argtypes = [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_int64, C.c_int, C.c_void_p]
    T, ctx = 3, 64
    rows = rng.standard_normal((T, (H + 2 * Hkv) * hd)).astype(np.float32)
    q16 = np.zeros((T, H, hd), np.uint16)
    kc, vc = np.zeros((ctx, Hkv * hd), np.uint16), np.zeros((Hkv * hd, ctx), np.uint16)
    assert L.gemma_test_rope_kv_prefill(rows.ctypes.data, rows.shape[1], T, 0, H, Hkv, hd, ctx, 10000.0, q16.ctypes.data,
                                        kc.ctypes.data, vc.ctypes.data) == 0, G.last_error()
    L.gemma_test_rows_rope_kv.restype = C.c_int
    L.gemma_test_rows_rope_kv.argtypes = [C.c_void_p, C.c_int64] + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 2
    assert L.gemma_test_rows_rope_kv(rows.ctypes.data, rows.shape[1], T, 0, H, Hkv, hd, ctx, 10000.0, kc.ctypes.data,
                                     vc.ctypes.data) == 0, G.last_error()
    rows_out = np.zeros((T, H * hd), np.float32)
    for form in (0, 1, 2):  # exact rows, exact matrix-core, f16 MFMA
        assert L.gemma_test_attn_prefill(q16.ctypes.data, kc.ctypes.data, vc.ctypes.data, T, 0, H, Hkv, hd, ctx, 32, H * hd,
                                         form, rows_out.ctypes.data) == 0, G.last_error()
    G.test_sample(rng.standard_normal((2, 300)).astype(np.float32), dict(temperature=0.9, top_k=5, seed=1), [3, 4])
    W = O.quantize((rng.standard_normal((16, 64)) * 0.05).astype(np.float32), "q4_0_ref")
    xs = rng.standard_normal((3, 64)).astype(np.float32)
    for exact in (False, True):
        assert _gemm(L, O.Q4_0, W, xs, 16, 64, 3, exact=exact)[0] == 0, G.last_error()
    G.gemm_skinny(O.Q4_0, W, 16, xs)


def _debug_step(e, shape):
    qw = shape["n_head"] * shape["head_dim"]
    per = qw + 2 * shape["n_head_kv"] * shape["head_dim"] + qw + shape["n_embd"]
    taps = np.zeros(shape["n_layer"] * per, np.float32)
    assert G.lib().gemma_engine_debug_step(e.h, taps.ctypes.data, None) == 0, G.last_error()


def _engine_cycle(shape, kw):
    """create ... close; returns the live (allocations, bytes) while the engine was open"""
    V = shape["n_vocab"]
    single = "tp" not in kw  # row-split engines decode token by token: no batch, sampler or verify
    e = G.Engine(shape, n_ctx=N_CTX, device=0, **kw)
    prompt = [int(t) for t in O.make_prompt(12, V)]
    e.begin(prompt)
    if single:
        e.prefill(len(prompt))
    e.step(3, use_graph=True)
    if single:
        e.set_sampler(temperature=0.8, top_k=8, seed=5)
        e.step(2, use_graph=True)
        e.set_sampler()  # greedy again
        e.step(1, use_graph=True)
        assert len(e.verify([1, 2, 3])) >= 1
        e.extend([int(t) for t in O.make_prompt(30, V, seed=7)])
        e.prefill_next(0)  # 30 rows > the first pass's 12: the scratch regrows
        e.step(2, use_graph=True)
    _debug_step(e, shape)
    e.step(1, use_graph=True)
    _hooks()
    live = G.mem_live()
    e.close()
    return live


def _two_cycles(cycle):
    """`cycle` twice: no growth from the first to the second, and a live owner counted"""
    gc.collect()  # the counters are process-wide: an engine an earlier test left unclosed goes now, not mid-way
    open1 = cycle()
    after1 = G.mem_live()
    open2 = cycle()
    after2 = G.mem_live()
    assert after2 == after1, ("allocations (count, bytes) left by the second cycle", after2, "by the first", after1)
    assert open1[0] > after1[0] and open1[1] > after1[1], (open1, after1)
    assert open2[0] > after2[0] and open2[1] > after2[1], (open2, after2)


@pytest.mark.parametrize("kind", list(ENGINES))
def test_engine_lifecycle_frees_what_it_allocates(kind):
    shape, kw = ENGINES[kind]
    _two_cycles(lambda: _engine_cycle(shape, kw))


def test_p2p_engine_create_free():
    """GEMMA_TP_P2P: the uncached arena and its counters (created and freed; no peer is opened)"""
    def cycle():
        e = G.Engine(dict(O.TINY), n_ctx=N_CTX, device=0, tp=(2, 0, None), tp_flags=G.TP_P2P)
        assert e.tp_flags() & G.TP_P2P
        live = G.mem_live()
        e.close()
        return live
    _two_cycles(cycle)


def test_c_abi_weight_cache():
    """hpc_init -> mul_mat on a Q4_0 and a Q4_K weight -> hpc_unregister_weight / hpc_flush_weights"""
    L = G.lib()
    L.hpc_set_error_mode(0)
    L.hpc_unregister_weight.argtypes = [C.c_void_p]
    rng = np.random.default_rng(11)
    W4 = O.quantize((rng.standard_normal((64, 512)) * 0.05).astype(np.float32), "q4_0_ref")
    WK = O.synth_kquant(O.Q4_K, 17, 40, 512)
    xs = rng.standard_normal((2, 512)).astype(np.float32)
    # the cache is keyed by host address and earlier tests leave entries of arrays since freed: W4 or
    # WK may sit at such an address, so the test starts from an empty cache
    L.hpc_flush_weights()
    assert L.hpc_weight_cache_entries() == 0

    def cycle():
        assert L.hpc_init(0) == 0, G.last_error()
        for W, wtype, rows in ((W4, O.Q4_0, 64), (WK, O.Q4_K, 40)):
            wdata, rs = O.mul_mat_init(wtype, xs)
            got = G.mul_mat(W, wtype, rows, W.shape[1], 512, wdata, rs, 2)
            ref = O.mul_mat(W, wtype, rows, W.shape[1], 512, wdata, rs, 2)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        live = G.mem_live()
        assert L.hpc_unregister_weight(W4.ctypes.data) == 1
        L.hpc_flush_weights()
        assert L.hpc_weight_cache_entries() == 0
        return live
    _two_cycles(cycle)


def test_ggml_graph_row_range_view():
    """one ggml graph whose mul_mat reads a row-range view of a quantized leaf, then ggml_free: the
    leaf mirrors and the tiled copy go with the context"""
    L = X.api()
    rows, K, cols = 24, 64, 3
    w = quant_weight(O.Q4_0, rows, K, 300)
    x = activations(np.random.default_rng(8), cols, K)

    def cycle():
        c = X.new_ctx(3 << 20)
        try:
            wt = L.ggml_view_2d(c, X.qleaf(c, O.Q4_0, K, rows, w), K, 16, w.shape[1], 1 * w.shape[1])
            X.run(c, L.ggml_mul_mat(c, wt, X.leaf(c, x)))
            return G.mem_live()
        finally:
            L.ggml_free(c)
    _two_cycles(cycle)
