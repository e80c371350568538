"""CPU: the tensor / view builders of include/ggml.h (csrc/ggml_api.cpp) against NumPy.

The builders touch no device, so the library is loaded as tests/test_capi_symbols.py does and the
shape (`ne`), byte strides (`nb`), root (`view_src`) and byte offset (`data - root.data`) of every
view op are compared with NumPy's `shape` / `strides` / data offset of the same operation on an
array with the tensor's memory layout (NumPy shape = ne reversed).  NumPy's stride of a size-1
dimension is arbitrary, so there `nb` is compared with ggml's own rule (noted per test).
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_ctypes as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gemma.ggml_amd", "lib", "libgemma_hip.so")
OP = {"CPY": 10, "CONT": 11, "VIEW": 12, "RESHAPE": 13, "PERMUTE": 14, "TRANSPOSE": 15, "MUL_MAT": 6}


@pytest.fixture
def X():
    if not os.path.exists(LIB):
        pytest.skip("library not built (make -C gemma.ggml_amd)")
    import ggml_ctypes
    ggml_ctypes.api()
    return ggml_ctypes


@pytest.fixture
def ctx(X):
    c = X.new_ctx(1 << 20)
    yield c
    X.api().ggml_free(c)


def _addr(a):
    return a.__array_interface__["data"][0]


def _taddr(t):
    return C.addressof(t.contents)


def _arr4(a):
    return a.reshape((1,) * (4 - a.ndim) + a.shape)


def _check(t, root, arr, base, op=None):
    """t's ne / nb / root / offset against the NumPy view `arr` of `base` (the root's array)."""
    tc, rc = t.contents, root.contents
    arr = _arr4(arr)
    assert tuple(tc.ne) == arr.shape[::-1]
    for d in range(4):
        if tc.ne[d] > 1:
            assert tc.nb[d] == arr.strides[3 - d], (d, tuple(tc.nb), arr.strides)
    off = _addr(arr) - _addr(base)
    assert tc.data - rc.data == off and tc.view_offs == off
    assert tc.view_src == _taddr(root)
    assert tc.type == rc.type
    if op is not None:
        assert tc.op == OP[op]


def _root(X, ctx, *ne):
    t = X.tensor(ctx, X.F32, *ne)
    base = np.zeros(ne[::-1], np.float32)
    assert tuple(t.contents.ne) == tuple(ne) + (1,) * (4 - len(ne))
    assert tuple(t.contents.nb)[:len(ne)] == base.strides[::-1]
    assert not t.contents.view_src and t.contents.view_offs == 0
    return t, base


@pytest.mark.parametrize("axes", [(0, 2, 1, 3), (1, 0, 2, 3), (2, 0, 1, 3)])
def test_permute(X, ctx, axes):
    a, base = _root(X, ctx, 2, 3, 4, 5)
    p = X.api().ggml_permute(ctx, a, *axes)
    # ggml: source dim i becomes result dim axes[i]; NumPy axis j is ggml dim 3 - j
    inv = [axes.index(d) for d in range(4)]
    ref = np.transpose(base, [3 - inv[3 - j] for j in range(4)])
    _check(p, a, ref, base, "PERMUTE")
    # a permute of a view with an offset keeps the root and the offset
    v = X.api().ggml_view_3d(ctx, a, 2, 2, 3, a.contents.nb[1], a.contents.nb[2], 1 * a.contents.nb[1] + 1 * a.contents.nb[2])
    pv = X.api().ggml_permute(ctx, v, *axes)
    vb = base[0, 1:4, 1:3, :]
    _check(pv, a, np.transpose(_arr4(vb), [3 - inv[3 - j] for j in range(4)]), base, "PERMUTE")


def test_transpose(X, ctx):
    a, base = _root(X, ctx, 3, 4, 2)
    t = X.api().ggml_transpose(ctx, a)
    _check(t, a, np.swapaxes(base, -1, -2), base, "TRANSPOSE")


def test_views_of_a_view_with_an_offset(X, ctx):
    L = X.api()
    a, base = _root(X, ctx, 8, 6, 4)
    nb = a.contents.nb
    v3 = L.ggml_view_3d(ctx, a, 6, 4, 3, nb[1], nb[2], 2 * nb[0] + 1 * nb[1] + 1 * nb[2])
    r3 = base[1:4, 1:5, 2:8]
    _check(v3, a, r3, base, "VIEW")
    assert v3.contents.nb[3] == nb[2] * 3  # ggml_view_3d: nb[3] = nb[2] * ne2
    v2 = L.ggml_view_2d(ctx, v3, 4, 3, nb[1], 1 * nb[0] + 1 * nb[1])
    r2 = r3[0, 1:4, 1:5]
    _check(v2, a, r2, base, "VIEW")
    assert v2.contents.nb[2] == nb[1] * 3 and v2.contents.nb[3] == nb[1] * 3  # ggml_view_2d: nb[2] = nb[3] = nb[1] * ne1
    v1 = L.ggml_view_1d(ctx, v2, 3, 1 * nb[0])
    r1 = r2[0, 1:4]
    _check(v1, a, r1, base, "VIEW")
    # a view of a view of a view still names the root, with the offsets summed
    assert v1.contents.view_offs == (2 + 1 + 1) * nb[0] + (1 + 1) * nb[1] + 1 * nb[2]
    # a strided 2-D window (the V-cache write): every second row
    w = L.ggml_view_2d(ctx, a, 5, 3, 2 * nb[1], 3 * nb[0])
    _check(w, a, base[0, 0:6:2, 3:8], base, "VIEW")


def test_reshape(X, ctx):
    L = X.api()
    a, base = _root(X, ctx, 6, 4, 5)
    _check(L.ggml_reshape_2d(ctx, a, 24, 5), a, base.reshape(5, 24), base, "RESHAPE")
    _check(L.ggml_reshape_3d(ctx, a, 3, 8, 5), a, base.reshape(5, 8, 3), base, "RESHAPE")
    v = L.ggml_view_2d(ctx, a, 6, 4, a.contents.nb[1], 2 * a.contents.nb[2])  # one contiguous slab at an offset
    _check(L.ggml_reshape_3d(ctx, v, 2, 3, 4), a, base[2].reshape(4, 3, 2), base, "RESHAPE")


@pytest.mark.parametrize("gtype", ["F32", "F16"])
def test_cont_2d_is_a_new_contiguous_tensor(X, ctx, gtype):
    L = X.api()
    gt = getattr(X, gtype)
    a = X.tensor(ctx, gt, 4, 3, 5)
    p = L.ggml_permute(ctx, a, 0, 2, 1, 3)
    c = L.ggml_cont_2d(ctx, p, 20, 3)
    cc = c.contents
    es = 4 if gtype == "F32" else 2
    ref = np.zeros((3, 20), np.float32 if gtype == "F32" else np.uint16)
    assert tuple(cc.ne) == (20, 3, 1, 1) and tuple(cc.nb)[:2] == ref.strides[::-1]
    assert tuple(cc.nb)[2:] == (60 * es, 60 * es)  # ggml: nb[i] = nb[i-1] * ne[i-1]
    assert cc.type == gt and cc.op == OP["CONT"] and not cc.view_src and cc.view_offs == 0
    assert cc.src[0] == _taddr(p) and cc.data and cc.data != a.contents.data


def test_cpy_is_a_view_of_its_destination(X, ctx):
    L = X.api()
    src = X.tensor(ctx, X.F32, 6, 4)
    cache = X.tensor(ctx, X.F16, 16, 8)
    base = np.zeros((8, 16), np.uint16)
    nb1 = cache.contents.nb[1]
    dst = L.ggml_view_2d(ctx, cache, 6, 4, nb1, 3 * 2 + 2 * nb1)
    c = L.ggml_cpy(ctx, src, dst)
    _check(c, cache, base[2:6, 3:9], base, "CPY")
    assert c.contents.src[0] == _taddr(src) and c.contents.src[1] == _taddr(dst)
    assert c.contents.type == X.F16


def test_mul_mat_result(X, ctx):
    L = X.api()
    a = X.tensor(ctx, X.Q4_0, 64, 7)
    b = X.tensor(ctx, X.F32, 64, 3, 2, 2)
    m = L.ggml_mul_mat(ctx, a, b).contents
    ref = np.zeros((2, 2, 3, 7), np.float32)
    assert tuple(m.ne) == ref.shape[::-1] and tuple(m.nb) == ref.strides[::-1]
    assert m.type == X.F32 and m.op == OP["MUL_MAT"] and not m.view_src and m.view_offs == 0 and m.data
    assert m.src[0] == _taddr(a) and m.src[1] == _taddr(b)
    # the F16 form over a cache view: [n, T, H] from a [K, n, Hkv] view and a permuted [K, T, H]
    kc = X.tensor(ctx, X.F16, 32 * 2 * 8)
    kv = L.ggml_view_3d(ctx, kc, 32, 5, 2, 32 * 2 * 2, 32 * 2, 0)
    q = L.ggml_permute(ctx, X.tensor(ctx, X.F32, 32, 4, 3), 0, 2, 1, 3)
    m = L.ggml_mul_mat(ctx, kv, q).contents
    assert tuple(m.ne) == (5, 3, 4, 1) and tuple(m.nb) == (4, 20, 60, 240)


BLCK = {"F32": 1, "F16": 1, "Q4_0": 32, "Q8_0": 32, "Q4_K": 256, "Q6_K": 256}


@pytest.mark.parametrize("gtype", list(BLCK))
def test_sizes_match_the_oracle(X, ctx, gtype):
    L, Lo = X.api(), O.lib()
    gt = getattr(X, gtype)
    blck = BLCK[gtype]
    assert L.ggml_blck_size(gt) == blck
    assert L.ggml_type_size(gt) == Lo.orc_row_size(gt, blck)
    for K in (blck, 3 * blck, 2048, 16384):
        K = (K + blck - 1) // blck * blck
        row = Lo.orc_row_size(gt, K)
        assert L.ggml_row_size(gt, K) == row, (gtype, K)
        for rows in (1, 5):
            t = L.ggml_new_tensor_2d(ctx, gt, K, rows)
            assert L.ggml_nbytes(t) == rows * row and t.contents.nb[1] == row
    # a strided view is as long as its last element reaches (ggml_nbytes of a non-contiguous tensor)
    if blck == 1:
        a = X.tensor(ctx, gt, 8, 6)
        es = L.ggml_type_size(gt)
        v = L.ggml_view_2d(ctx, a, 3, 4, 8 * es, 2 * es)
        assert L.ggml_nbytes(v) == (3 * 8 + 3) * es
        assert L.ggml_nelements(v) == 12 and L.ggml_element_size(v) == es
