"""The engine's diagnostic entry points that only scripts called so far: gemma_engine_debug_step,
gemma_engine_prefill_taps, gemma_engine_time (kernels 0-4) and the two stamp entry points in a
product build.  Each is pinned against the plain decode step of the same configuration, bit for
bit, on a 3-layer Gemma-2B-shaped engine (Q4_0, n_ctx 128, 6-token prompt)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O

gpu = pytest.mark.gpu

SHAPE = dict(O.GEMMA_2B, n_layer=3, n_vocab=8192, n_head_kv=1)
N_CTX = 128
E, F, V, NL = SHAPE["n_embd"], SHAPE["n_ff"], SHAPE["n_vocab"], SHAPE["n_layer"]
QW = SHAPE["n_head"] * SHAPE["head_dim"]
QKV_ROWS = QW + 2 * SHAPE["n_head_kv"] * SHAPE["head_dim"]
PER = QKV_ROWS + QW + E  # one layer's taps: [qkv | attention out | residual after the layer]


def _engine():
    import gemma_hip as G
    return G.Engine(SHAPE, n_ctx=N_CTX, wtype=O.Q4_0)


def _debug_step(e):
    """one eager step with taps: ([n_layer][PER] taps, logits)"""
    import gemma_hip as G
    taps = np.zeros(NL * PER, dtype=np.float32)
    lg = np.zeros(V, dtype=np.float32)
    r = G.lib().gemma_engine_debug_step(e.h, taps.ctypes.data, lg.ctypes.data)
    assert r == 0, G.last_error()
    return taps.reshape(NL, PER), lg


@pytest.fixture(scope="module")
def plain():
    """the prompt and the first plain step's logits (position 0), computed once"""
    prompt = O.make_prompt(6, V)
    e = _engine()
    e.begin(prompt)
    lg = e.step(1, want_logits=True)[0].copy()
    e.close()
    lg.setflags(write=False)
    return prompt, lg


@gpu
def test_debug_step_equals_plain_step(plain):
    prompt, lg_ref = plain
    e = _engine()
    e.begin(prompt)
    taps, lg = _debug_step(e)
    e.close()
    assert np.array_equal(lg.view(np.uint32), lg_ref.view(np.uint32))
    resid = taps[:, QKV_ROWS + QW: QKV_ROWS + QW + E]
    assert np.isfinite(resid[NL - 1]).all()
    assert not np.array_equal(resid[0].view(np.uint32), resid[1].view(np.uint32))


def _mat_bytes(rows, k):
    return rows * (k // 32) * 18  # Q4_0: 18 bytes per 32 weights


@gpu
def test_time_kernel_bytes_and_state(plain):
    """algo_bytes as gemma_engine_time states them for this shape under the default plan (attn-out
    and down read the 36-bytes-per-32 activation image: qw and n_ff are whole 4-block groups):
      0 gate/up  2 * W(F, E) + 8 E + 4 F          1 down     W(E, F) + F * 36/32 + 8 E
      2 qkv      W(qkv_rows, E) + 8 E + 4 qkv_rows 3 attn-out W(E, qw) + qw * 36/32 + 8 E
      4 logits   W(V, E) + 8 E + 4 V               with W(rows, K) = rows * K/32 * 18."""
    prompt, lg_ref = plain
    want = [2 * _mat_bytes(F, E) + 8.0 * E + 4.0 * F,
            _mat_bytes(E, F) + F * 36.0 / 32 + 8.0 * E,
            _mat_bytes(QKV_ROWS, E) + 8.0 * E + 4.0 * QKV_ROWS,
            _mat_bytes(E, QW) + QW * 36.0 / 32 + 8.0 * E,
            _mat_bytes(V, E) + 8.0 * E + 4.0 * V]
    e = _engine()
    e.begin(prompt)
    got = [e.time_kernel(k, 3) for k in range(5)]
    e.begin(prompt)
    lg = e.step(1, want_logits=True)[0]
    e.close()
    for k, (us, nbytes) in enumerate(got):
        assert us > 0, k
        assert nbytes == want[k], (k, nbytes, want[k])
    assert np.array_equal(lg.view(np.uint32), lg_ref.view(np.uint32))


@gpu
def test_prefill_taps_last_row_equals_decode_tap(plain):
    """the exact batched prefill's last-layer residual of the last prompt row = the same tap of the
    token-by-token decode at that position (batched = token by token: test_gpu_prefill.py)"""
    import gemma_hip as G
    prompt, _ = plain
    T = len(prompt)
    e = _engine()
    e.begin(prompt)
    pt = np.zeros((NL, T, E), dtype=np.float32)
    assert G.lib().gemma_engine_prefill_taps(e.h, pt.ctypes.data, 1) == 0, G.last_error()
    e.begin(prompt)
    e.step(T - 1, use_graph=False)
    taps, _ = _debug_step(e)
    e.close()
    dec = taps[NL - 1, QKV_ROWS + QW: QKV_ROWS + QW + E]
    assert np.isfinite(dec).all()
    assert np.array_equal(pt[NL - 1, T - 1].view(np.uint32), dec.view(np.uint32))


@gpu
def test_stamp_entry_points_refuse_in_product_build(plain):
    import gemma_hip as G
    prompt, lg_ref = plain
    e = _engine()
    e.begin(prompt)
    with pytest.raises(RuntimeError, match="built without -DGHIP_STAMPS"):
        e.stamp_step(0)
    assert G.lib().gemma_engine_token_stamps(C.c_void_p(e.h), None) == -1
    assert "built without -DGHIP_STAMPS" in G.last_error()
    lg = e.step(1, want_logits=True)[0]
    e.close()
    assert np.array_equal(lg.view(np.uint32), lg_ref.view(np.uint32))
