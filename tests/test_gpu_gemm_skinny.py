"""The skinny exact GEMM of the verify pass (launch_gemm_skinny through gemma_test_gemm_skinny): for
1 <= T <= 8 activation rows it must equal the oracle's mul_mat (ggml's AVX2 lane order) and the exact
prefill GEMM bit for bit (uint32 views, no tolerance), with and without the residual epilogue.

Shapes: K = 32 and 96 (fewer blocks than one weight tile), rows that are no multiple of the 8-row
tile (40, 100) or of a 4-wave workgroup (72), K = 1312 (41 blocks: a ragged last Q4_0 tile and a
ragged last K chunk), K = 2048 (exactly one Q4_0 chunk, two Q8_0 chunks), Gemma-2B's down
projection K = 16384 (8 / 16 chunks through the double-buffered staging) and 8200 rows (the other
launch form).  Inputs as in
test_gemm_exact_bit_identical: rows scaled 0.1 .. 3, a zeroed run at the start of row 0 (d = 0)."""
import ctypes as C
import functools

import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O

pytestmark = pytest.mark.gpu

# the last shape is past the launcher's threshold (1021 row tiles): four row tiles per workgroup, one
# wave each, instead of one row tile whose columns the four waves share; 1025 row tiles leave the last
# workgroup three idle waves
SHAPES = [(8, 32), (40, 96), (72, 2048), (100, 512), (96, 1312), (256, 16384), (8200, 64)]
T_MAX = 8


@functools.lru_cache(maxsize=None)
def _case(wtype, rows, K):
    """weights, 8 input rows, a residual and the oracle's product of all 8 columns, shared by the T
    cases (column t of mul_mat does not depend on the other columns); read-only"""
    rng = np.random.default_rng(rows * 13 + K + wtype)
    Wf = (rng.standard_normal((rows, K)) * 0.05).astype(np.float32)
    W = O.quantize(Wf, "q4_0_ref" if wtype == O.Q4_0 else "q8_0_ref")
    X = (rng.standard_normal((T_MAX, K)) * rng.uniform(0.1, 3.0, (T_MAX, 1))).astype(np.float32)
    X[0, :min(37, K)] = 0.0
    R = rng.standard_normal((T_MAX, rows)).astype(np.float32)
    wdata, rs = O.mul_mat_init(wtype, X)
    ref = O.mul_mat(W, wtype, rows, W.shape[1], K, wdata, rs, T_MAX)
    for a in (W, X, R, ref):
        a.setflags(write=False)
    return W, X, R, ref


def _exact(wtype, W, X, rows):
    T, K = X.shape
    L = G.lib()
    L.gemma_test_gemm_exact.restype = C.c_int
    L.gemma_test_gemm_exact.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 5
    Y = np.zeros((T, rows), np.float32)
    x = np.ascontiguousarray(X)
    assert L.gemma_test_gemm_exact(wtype, rows, K, T, W.ctypes.data, x.ctypes.data, Y.ctypes.data, None, None) == 0, G.last_error()
    return Y


def _same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, np.abs(got - ref).max())


@pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])
@pytest.mark.parametrize("rows,K", SHAPES)
@pytest.mark.parametrize("T", [1, 2, 3, 5, 8])
def test_skinny_bit_identical(wtype, rows, K, T):
    W, X, R, ref = _case(wtype, rows, K)
    x, r = X[:T], R[:T]
    y = G.gemm_skinny(wtype, W, rows, x)
    _same(y, ref[:T], "skinny vs mul_mat")
    _same(y, _exact(wtype, W, x, rows), "skinny vs the exact prefill GEMM")
    ya = G.gemm_skinny(wtype, W, rows, x, resid=r)
    _same(ya, ref[:T] + r, "skinny + resid vs mul_mat + resid (f32 add)")


@pytest.mark.parametrize("T", [0, 9])
def test_skinny_refuses_other_T(T):
    W, X, R, ref = _case(O.Q4_0, 40, 96)
    x = np.zeros((T, 96), np.float32)
    with pytest.raises(RuntimeError, match="outside"):
        G.gemm_skinny(O.Q4_0, W, 40, x)
