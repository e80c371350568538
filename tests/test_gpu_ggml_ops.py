"""ggml graph executor, the generic ops one node at a time (include/ggml.h via tests/ggml_ctypes.py;
csrc/ggml_api.cpp running csrc/ggml_ops.hip and, for quantized MUL_MAT, the hot-path kernels).

Every result is compared bit for bit (uint32 / uint16 views) with the oracle's restatement of the
same ggml op, at the shapes and strides the Gemma graph never has: soft-max scale / mask / odd row
lengths, partial-width RoPE and table regrowth, the K % 32 tail of the F16 dot, modulo broadcast,
every copy type into cache windows, F32 / F16 get_rows, quantized mul_mat at rows and K that are
no multiple of the tile, the leaf-mirror and tiled-weight caches, and the executor's refusals.
One fresh context per case: a context-arena leaf is uploaded once per pointer by design.
"""
import ctypes as C
import os

import numpy as np
import pytest

import gemma_hip as G
import ggml_ctypes as X
import norm_adversary
import oracle_ctypes as O

gpu = pytest.mark.gpu
F = np.float32
INF = F(np.inf)


@pytest.fixture
def ctx():
    c = X.new_ctx(16 << 20)
    yield c
    X.api().ggml_free(c)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16)


def same(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    return got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(bits(got), bits(ref))


def padded_view(ctx, a, pad=3, junk=1e30):
    """a (n2, n1, n0) again as a view_3d of a larger leaf: rows `pad` elements longer than n0 and
    starting one element in (a padded nb1, a non-zero offset), the padding filled with `junk`."""
    n2, n1, n0 = a.shape
    big = np.full((n2, n1, n0 + pad), junk, a.dtype)
    big[:, :, 1:1 + n0] = a
    t = X.leaf(ctx, big)
    es = a.dtype.itemsize
    return X.api().ggml_view_3d(ctx, t, n0, n1, n2, (n0 + pad) * es, (n0 + pad) * n1 * es, es)


# ---- SOFT_MAX ---------------------------------------------------------------------------------
def ref_soft_max(a, mask, scale):
    """orc_soft_max_row per row of a (n2, n1, n); mask (m1, n) or None, row i1 % m1."""
    L = O.lib()
    out = np.zeros_like(a)
    for i2 in range(a.shape[0]):
        for i1 in range(a.shape[1]):
            x = np.ascontiguousarray(a[i2, i1])
            m = None if mask is None else np.ascontiguousarray(mask[i1 % mask.shape[0]])
            y = np.zeros_like(x)
            L.orc_soft_max_row(O.ptr(x), None if m is None else O.ptr(m), O.ptr(y), x.size, float(scale))
            out[i2, i1] = y
    return out


def soft_max_input(n, scale, rng):
    a = (rng.standard_normal((2, 3, n)) * 3).astype(F)
    a[0, 0] = (rng.standard_normal(n) * 8000).astype(F)  # spread > 1e4 for n > a few: exp underflows to 0
    if n > 1:
        a[0, 0, 0], a[0, 0, -1] = F(12000.0), F(-12000.0)
    # x*scale steps from 0 down to -20: exp passes through the f16 subnormals (e^-9.7 .. e^-17.3) to 0
    a[0, 1] = (-np.linspace(0.0, 20.0, n) / scale).astype(F)
    a[0, 2] = F(1.7)  # an all-equal row
    return a


def soft_max_masks(n, rng):
    def fin(shape):
        m = (rng.standard_normal(shape) * 0.1).astype(F)
        m[m == 0] = F(0.05)
        return m
    causal = fin((3, n))
    for i1, lim in enumerate([n - 1, n // 2, 0]):  # row 2: every entry but one masked
        causal[i1, lim + 1:] = -INF
    one = fin((1, n))
    one[0, n // 2 + 1:] = -INF
    return {"none": None, "causal": causal, "one_row": one}


@gpu
@pytest.mark.parametrize("scale", [1.0, 0.0625, 0.3])
@pytest.mark.parametrize("n", [1, 31, 64, 65, 255, 256, 257, 1000])
def test_soft_max_scale_mask_and_row_length(ctx, n, scale):
    L = X.api()
    rng = np.random.default_rng(n * 7 + int(scale * 1000))
    a = soft_max_input(n, scale, rng)
    for name, mask in soft_max_masks(n, rng).items():
        ref = ref_soft_max(a, mask, scale)
        assert np.all(np.isfinite(ref))
        for view in (False, True):
            src = padded_view(ctx, a) if view else X.leaf(ctx, a)
            mt = None if mask is None else X.leaf(ctx, mask)
            got = X.run(ctx, L.ggml_soft_max_ext(ctx, src, mt, None, scale, 0.0))
            assert same(got[0], ref), (n, scale, name, "view" if view else "contiguous")
    if n >= 255 and scale == 1.0:  # the inputs reach what they are meant to reach
        e = ref_soft_max(a, None, 1.0)
        assert (e[0, 0] == 0).any() and ((e[0, 1] > 0) & (e[0, 1] < 6.2e-5 * e[0, 1].max())).any()


# ---- ROPE -------------------------------------------------------------------------------------
def ref_rope(x, pos, n_dims, base):
    """x (T, H, ne0): NEOX pairs (k, k + n_dims/2) rotated with orc_rope_cos_sin(pos[t]) (SURVEY
    A.8), products rounded separately; columns >= n_dims copied."""
    y, half = x.copy(), n_dims // 2
    for t, p in enumerate(pos):
        c, s = np.zeros(half, F), np.zeros(half, F)
        O.lib().orc_rope_cos_sin(int(p), n_dims, float(base), O.ptr(c), O.ptr(s))
        x0, x1 = x[t, :, :half], x[t, :, half:n_dims]
        y[t, :, :half] = x0 * c - x1 * s
        y[t, :, half:n_dims] = x0 * s + x1 * c
    return y


def rope_node(ctx, xt, pos, n_dims, base, mode=2):
    pt = X.leaf(ctx, np.asarray(pos, np.int32))
    return X.api().ggml_rope_custom(ctx, xt, pt, n_dims, mode, 0, 0, base, 1.0, 0.0, 1.0, 0.0, 0.0)


def rope_check(ctx, rng, ne0, n_dims, pos, base=10000.0, view=False):
    x = rng.standard_normal((len(pos), 3, ne0)).astype(F)
    xt = padded_view(ctx, x) if view else X.leaf(ctx, x)
    got = X.run(ctx, rope_node(ctx, xt, pos, n_dims, base))
    assert same(got[0], ref_rope(x, pos, n_dims, base)), (ne0, n_dims, list(pos), base, view)


@gpu
@pytest.mark.parametrize("ne0,n_dims", [(64, 64), (64, 32), (256, 256), (8, 2)])
def test_rope_partial_width_and_positions(ctx, ne0, n_dims):
    rng = np.random.default_rng(ne0 + n_dims)
    rope_check(ctx, rng, ne0, n_dims, [3, 0, 511, 3, 1])
    rope_check(ctx, rng, ne0, n_dims, [3, 0, 511, 3, 1], view=True)


@gpu
def test_rope_table_grows_and_rebuilds(ctx):
    rng = np.random.default_rng(5)
    first = [3, 0, 511, 3, 1]
    rope_check(ctx, rng, 64, 64, first)
    rope_check(ctx, rng, 64, 64, [512, 700, 2, 700, 2047])  # past the 512 positions first built
    rope_check(ctx, rng, 64, 32, first)                      # another n_dims: rebuilt (and shrunk)
    rope_check(ctx, rng, 64, 32, [512, 700, 2, 700, 1500])   # grown again at that n_dims
    rope_check(ctx, rng, 64, 32, first, base=1e6)            # another base: rebuilt
    rope_check(ctx, rng, 64, 64, first)                      # back to the first configuration
    rope_check(ctx, rng, 64, 64, [700, 512, 0, 1, 2])


@gpu
def test_rope_two_nodes_with_different_n_dims_in_one_graph(ctx):
    L = X.api()
    rng = np.random.default_rng(6)
    pos = [3, 0, 511, 3, 1]
    x = rng.standard_normal((5, 3, 64)).astype(F)
    z = rng.standard_normal((5, 3, 64)).astype(F)
    r0 = rope_node(ctx, X.leaf(ctx, x), pos, 64, 10000.0)
    r1 = rope_node(ctx, X.leaf(ctx, z), [600, 1, 0, 2, 7], 32, 10000.0)
    got = X.run(ctx, L.ggml_add(ctx, r0, r1))
    ref = ref_rope(x, pos, 64, 10000.0) + ref_rope(z, [600, 1, 0, 2, 7], 32, 10000.0)
    assert same(got[0], ref)


@gpu
def test_rope_positions_set_between_computes_of_one_graph():
    """the reference's loop: positions live in a backend buffer and are set before every compute of
    the graph; the table is sized from the values the device is about to read"""
    L = X.api()
    rng = np.random.default_rng(7)
    wctx, cctx, buf = X.new_ctx(1 << 16, no_alloc=True), X.new_ctx(1 << 20), None
    try:
        pt, xt = X.tensor(wctx, X.I32, 2), X.tensor(wctx, X.F32, 64, 3, 2)
        buf = L.ggml_backend_alloc_ctx_tensors_from_buft(wctx, L.ggml_backend_cpu_buffer_type())
        out = L.ggml_rope_custom(cctx, xt, pt, 64, 2, 0, 0, 10000.0, 1.0, 0.0, 1.0, 0.0, 0.0)
        g = X.graph(cctx, out)
        for pos in ([1, 2], [1300, 900], [0, 2047], [5, 5]):
            x = rng.standard_normal((2, 3, 64)).astype(F)
            p = np.array(pos, np.int32)
            L.ggml_backend_tensor_set(xt, O.ptr(x), 0, x.nbytes)
            L.ggml_backend_tensor_set(pt, O.ptr(p), 0, p.nbytes)
            assert X.compute_status(cctx, g) == 0, G.last_error()
            assert same(X.get_array(out)[0], ref_rope(x, pos, 64, 10000.0)), pos
    finally:
        L.ggml_free(cctx)
        if buf:
            L.ggml_backend_buffer_free(buf)
        L.ggml_free(wctx)


# ---- RMS_NORM ---------------------------------------------------------------------------------
def ref_rms_norm(a, eps):
    out = np.zeros_like(a)
    for idx in np.ndindex(a.shape[:-1]):
        x, y = np.ascontiguousarray(a[idx]), np.zeros(a.shape[-1], F)
        O.lib().orc_rms_norm(O.ptr(x), O.ptr(y), x.size, float(eps))
        out[idx] = y
    return out


@gpu
@pytest.mark.parametrize("eps", [1e-6, 0.0])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 255, 256, 257, 1000])
def test_rms_norm_rows(ctx, n, eps):
    L = X.api()
    rng = np.random.default_rng(n + (1 if eps else 0))
    a = rng.standard_normal((2, 3, n)).astype(F)
    a[0, 1] *= F(1e-3)
    a[1, 0] *= F(3e4)
    a[1, 2] = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(F)  # mixed magnitudes
    if eps:
        a[0, 2] = 0.0  # an all-zero row: 0 * 1/sqrtf(eps)
    ref = ref_rms_norm(a, eps)
    assert np.all(np.isfinite(ref))
    for view in (False, True):
        src = padded_view(ctx, a) if view else X.leaf(ctx, a)
        got = X.run(ctx, L.ggml_rms_norm(ctx, src, eps))
        assert same(got[0], ref), (n, eps, view)


@gpu
@pytest.mark.parametrize("n", [300, 517, 1000, 1001, 1004])
def test_rms_norm_sequential_fallback(ctx, n):
    """rows on which a tree sum and ggml's sequential sum give different means
    (norm_adversary.build_row, checked by its `verify`), so the kernel leaves its tree for the
    sequential sum.  At n % 8 != 0 the last group of 8 goes through the fallback's `i0 + j < n`
    tail: a read past the row would take in the next row or the view's padding.  (build_row packs
    n // 32 blocks, the rest of the row is zero; it finds no such row at 255 or 257 and none can
    exist below one block, so those n of test_rms_norm_rows stay on random rows.)"""
    L = X.api()
    eps = 1e-6
    a = np.random.default_rng(n).standard_normal((2, 3, n)).astype(F) * F(100)
    for row, seed in (((0, 0), 0), ((1, 1), 1)):
        _, x, info = norm_adversary.build_row("q8_0", n, eps=eps, seed=seed)
        assert x.size == n and info["scale_seq"] != info["scale_tree"]
        a[row] = x
    ref = ref_rms_norm(a, eps)
    assert np.all(np.isfinite(ref))
    for view in (False, True):
        src = padded_view(ctx, a) if view else X.leaf(ctx, a)
        got = X.run(ctx, L.ggml_rms_norm(ctx, src, eps))
        assert same(got[0], ref), (n, view)


# ---- SCALE / MUL / ADD ------------------------------------------------------------------------
def ew_sources(ctx, a):
    """a (2, 2, 3, 5) = ggml [5, 3, 2, 2]: contiguous, and as permute(0,2,1,3) of a [5, 2, 3, 2] leaf."""
    yield "contiguous", X.leaf(ctx, a)
    yield "permuted", X.api().ggml_permute(ctx, X.leaf(ctx, a.transpose(0, 2, 1, 3)), 0, 2, 1, 3)


@gpu
@pytest.mark.parametrize("s", [float(np.sqrt(F(2048))), 1.0 / 16, -3.0])
def test_scale(ctx, s):
    a = np.random.default_rng(1).standard_normal((2, 2, 3, 5)).astype(F)
    for name, src in ew_sources(ctx, a):
        assert tuple(src.contents.ne) == (5, 3, 2, 2)
        assert same(X.run(ctx, X.api().ggml_scale(ctx, src, s)), a * F(s)), (s, name)


@gpu
@pytest.mark.parametrize("op", ["mul", "add"])
@pytest.mark.parametrize("bne", [(5, 3, 2, 2), (5, 1, 1, 1), (5, 3, 1, 1), (5, 1, 2, 1), (1, 1, 1, 1)])
def test_mul_add_broadcast(ctx, op, bne):
    rng = np.random.default_rng(sum(bne))
    a = rng.standard_normal((2, 2, 3, 5)).astype(F)
    b = rng.standard_normal(bne[::-1]).astype(F)
    rep = np.tile(b, [a.shape[i] // b.shape[i] for i in range(4)])  # ggml's broadcast: repetition
    ref = a * rep if op == "mul" else a + rep
    fn = X.api().ggml_mul if op == "mul" else X.api().ggml_add
    for name, src in ew_sources(ctx, a):
        assert same(X.run(ctx, fn(ctx, src, X.leaf(ctx, b))), ref), (op, bne, name)


# ---- GELU -------------------------------------------------------------------------------------
def ref_gelu(x, clamp):
    L = O.lib()
    y = np.zeros_like(x)
    L.orc_init_tables(clamp)  # the oracle's clamp flag is process-global
    try:
        L.orc_gelu(O.ptr(x), O.ptr(y), x.size)
    finally:
        L.orc_init_tables(0)
    return y


@gpu
@pytest.mark.parametrize("clamp", [0, 1])
def test_gelu_every_finite_f16(ctx, clamp):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = h[(h & 0x7C00) != 0x7C00]
    assert h.size == 63488
    x = h.view(np.float16).astype(F)
    if clamp:
        ten = F(10.0)
        edge = [ten, -ten, np.nextafter(ten, F(0)), np.nextafter(-ten, F(0)), 70000.0, -70000.0, 1e5, -1e5]
        x = np.concatenate([x, np.array(edge, F)])
    old = os.environ.pop("GEMMA_HIP_GELU_CLAMP", None)
    try:
        if clamp:
            os.environ["GEMMA_HIP_GELU_CLAMP"] = "1"  # read when the node is built
        node = X.api().ggml_gelu(ctx, X.leaf(ctx, x))
    finally:
        os.environ.pop("GEMMA_HIP_GELU_CLAMP", None)
        if old is not None:
            os.environ["GEMMA_HIP_GELU_CLAMP"] = old
    assert node.contents.op_params[0] == clamp
    got = X.run(ctx, node)
    assert same(got.ravel(), ref_gelu(x, clamp))


# ---- CPY / CONT -------------------------------------------------------------------------------
F16_SPECIAL = np.array([
    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20, 2048 + 1, 2048 + 3,  # RNE ties
    65504, 65519.996, 65520, -65520, 65536, 1e9,                          # around and above the f16 maximum
    2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 6.0e-5, -2.0 ** -14 * 0.9995,  # f16 subnormals
    -0.0, 0.0, 1e-30, -1e-30, 0.1, -3.14159], dtype=F)


def cpy_source(kind, dtype, rng):
    """(values in logical order [ne0 fastest] as (2, 3, 4) ne = [4, 3, 2], builder of the source tensor)"""
    if dtype == np.float32:
        v = F16_SPECIAL[rng.permutation(24)].reshape(2, 3, 4).copy()
    else:
        v = rng.integers(0, 0x7C00, 24).astype(np.uint16).reshape(2, 3, 4)
        v[0, 0, :4] = [0x8000, 0x0001, 0x83FF, 0x7BFF]  # -0, the smallest subnormal, a negative one, the maximum
        v[1] |= 0x8000

    def build(ctx):
        L = X.api()
        if kind == "contiguous":
            return X.leaf(ctx, v)
        if kind == "permuted":  # ne [4, 3, 2] as permute(0,2,1,3) of a [4, 2, 3] leaf
            return L.ggml_permute(ctx, X.leaf(ctx, v.transpose(1, 0, 2)), 0, 2, 1, 3)
        return L.ggml_transpose(ctx, X.leaf(ctx, v.transpose(0, 2, 1)))  # of a [3, 4, 2] leaf
    return v, build


def convert(v, dst_dtype):
    if v.dtype == dst_dtype:
        return v.copy()
    if dst_dtype == np.uint16:
        return O.fp32_to_fp16_bits(v).reshape(v.shape)
    return v.view(np.float16).astype(F)


def sentinel(dtype, rng):
    if dtype == np.float32:
        return rng.standard_normal((8, 16)).astype(F)
    return rng.integers(0, 0x7C00, (8, 16)).astype(np.uint16)


def read_back(ctx, cache):
    """the whole [16, 8] cache leaf through a node: cont_2d of a full view"""
    L = X.api()
    return L.ggml_cont_2d(ctx, L.ggml_view_2d(ctx, cache, 16, 8, cache.contents.nb[1], 0), 16, 8)


@gpu
@pytest.mark.parametrize("kind", ["contiguous", "permuted", "transposed"])
@pytest.mark.parametrize("dst_dtype", [np.float32, np.uint16], ids=["to_f32", "to_f16"])
@pytest.mark.parametrize("src_dtype", [np.float32, np.uint16], ids=["f32", "f16"])
def test_cpy_into_cache_windows(ctx, src_dtype, dst_dtype, kind):
    L = X.api()
    rng = np.random.default_rng(11)
    es = np.dtype(dst_dtype).itemsize
    model = sentinel(dst_dtype, rng)
    cache = X.leaf(ctx, model)
    # compute 1: a [6, 4] window at row 2, column 3, rows 16 wide (the V-cache write)
    v, build = cpy_source(kind, src_dtype, rng)
    win = L.ggml_view_2d(ctx, cache, 6, 4, 16 * es, (2 * 16 + 3) * es)
    got = X.run(ctx, L.ggml_cpy(ctx, build(ctx), win), read_back(ctx, cache))
    model[2:6, 3:9] = convert(v, dst_dtype).reshape(4, 6)
    assert same(got[0, 0], model), "window copy (bytes outside the window included)"
    # compute 2, same context: a 1-D run of another shape than the source (the K-cache write)
    v2, build2 = cpy_source(kind, src_dtype, rng)
    run1d = L.ggml_view_1d(ctx, cache, 24, 100 * es)
    got = X.run(ctx, L.ggml_cpy(ctx, build2(ctx), run1d), read_back(ctx, cache))
    model.reshape(-1)[100:124] = convert(v2, dst_dtype).reshape(-1)
    assert same(got[0, 0], model), "the leaf holds both windows after the second compute"


@gpu
def test_cache_in_a_backend_buffer():
    L = X.api()
    rng = np.random.default_rng(12)
    wctx = X.new_ctx(1 << 16, no_alloc=True)
    cctx = X.new_ctx(1 << 20)
    buf = None
    try:
        cache = X.tensor(wctx, X.F16, 16, 8)
        inp = X.tensor(wctx, X.F32, 24)
        buf = L.ggml_backend_alloc_ctx_tensors_from_buft(wctx, L.ggml_backend_cpu_buffer_type())
        assert cache.contents.data and inp.contents.data
        L.ggml_backend_buffer_clear(buf, 0)
        zeros = np.zeros((8, 16), np.uint16)
        assert same(X.run(cctx, read_back(cctx, cache))[0, 0], zeros)
        node = L.ggml_cpy(cctx, inp, L.ggml_view_1d(cctx, cache, 24, 40 * 2))
        out = read_back(cctx, cache)
        g = X.graph(cctx, node, out)
        model = zeros.copy()
        for k in range(2):  # the same graph twice, the input set in between
            x = rng.standard_normal(24).astype(F)
            L.ggml_backend_tensor_set(inp, O.ptr(x), 0, x.nbytes)
            assert X.compute_status(cctx, g) == 0, G.last_error()
            model.reshape(-1)[40:64] = O.fp32_to_fp16_bits(x)
            assert same(X.get_array(out)[0, 0], model), k
        # a second window through another graph: the device copy is the authority, both windows stay
        x = rng.standard_normal(24).astype(F)
        L.ggml_backend_tensor_set(inp, O.ptr(x), 0, x.nbytes)
        win = L.ggml_view_2d(cctx, cache, 6, 4, 32, (4 * 16 + 9) * 2)
        got = X.run(cctx, L.ggml_cpy(cctx, inp, win), read_back(cctx, cache))
        model[4:8, 9:15] = O.fp32_to_fp16_bits(x).reshape(4, 6)
        assert same(got[0, 0], model)
        L.ggml_backend_buffer_clear(buf, 0)
        assert same(X.run(cctx, read_back(cctx, cache))[0, 0], zeros)
    finally:
        L.ggml_free(cctx)
        if buf:
            L.ggml_backend_buffer_free(buf)
        L.ggml_free(wctx)


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=["f32", "f16"])
def test_cont_2d_of_a_permuted_tensor(ctx, dtype):
    L = X.api()
    rng = np.random.default_rng(13)
    a = rng.standard_normal((5, 3, 4)).astype(F)  # ggml [4, 3, 5], merged as kqv_merged is
    if dtype == np.uint16:
        a = a.astype(np.float16).view(np.uint16)
    got = X.run(ctx, L.ggml_cont_2d(ctx, L.ggml_permute(ctx, X.leaf(ctx, a), 0, 2, 1, 3), 20, 3))
    assert same(got[0, 0], a.transpose(1, 0, 2).reshape(3, 20))


# ---- GET_ROWS ---------------------------------------------------------------------------------
IDX_LEAF = np.array([2, 4, 6, 0, 3, 3, 5, 1, 4, 2], np.int32)  # the view takes [6, 0, 3, 3, 5, 1]


def rows_index(ctx):
    return X.api().ggml_view_1d(ctx, X.leaf(ctx, IDX_LEAF), 6, 2 * 4), IDX_LEAF[2:8]


@gpu
@pytest.mark.parametrize("K", [1, 33])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=["f32", "f16"])
def test_get_rows_f32_f16(ctx, dtype, K):
    rng = np.random.default_rng(K)
    a = rng.standard_normal((7, K)).astype(F)
    if dtype == np.uint16:
        a = a.astype(np.float16).view(np.uint16)
        a[0, 0], a[6, -1] = 0x0001, 0x83FF  # f16 subnormals
    it, idx = rows_index(ctx)
    got = X.run(ctx, X.api().ggml_get_rows(ctx, X.leaf(ctx, a), it))
    assert same(got[0, 0], convert(a, np.float32)[idx])


@gpu
@pytest.mark.parametrize("wtype,K", [(O.Q4_0, 32), (O.Q4_0, 288), (O.Q8_0, 32), (O.Q8_0, 288), (O.Q4_K, 256), (O.Q6_K, 256)])
def test_get_rows_quantized(ctx, wtype, K):
    w = quant_weight(wtype, 7, K, K + wtype)
    it, idx = rows_index(ctx)
    got = X.run(ctx, X.api().ggml_get_rows(ctx, X.qleaf(ctx, wtype, K, 7, w), it))
    ref = np.stack([O.dequantize(wtype, w[i], K) for i in idx])
    assert same(got[0, 0], ref)


def quant_weight(wtype, rows, K, seed):
    if wtype in (O.Q4_K, O.Q6_K):
        return O.synth_kquant(wtype, seed, rows, K)
    x = np.random.default_rng(seed).standard_normal((rows, K)).astype(F)
    return O.quantize(x, "q4_0_ref" if wtype == O.Q4_0 else "q8_0_ref")


# ---- MUL_MAT, F16 src0 ------------------------------------------------------------------------
def ref_mul_mat_f16(a, b):
    """a (Hkv, n, K) f16 bits, b (ne13, H, T, K) f32 -> (ne13, H, T, n): ggml's INIT (b rows to f16)
    then orc_vec_dot_f16 per (row, column); head i12 reads a[i12 // (H / Hkv)]."""
    L = O.lib()
    b16 = O.fp32_to_fp16_bits(b).reshape(b.shape)
    n13, H, T, K = b.shape
    Hkv, n = a.shape[:2]
    out = np.zeros((n13, H, T, n), F)
    s = C.c_float()
    for i13 in range(n13):
        for h in range(H):
            for t in range(T):
                y = np.ascontiguousarray(b16[i13, h, t])
                for r in range(n):
                    x = np.ascontiguousarray(a[h // (H // Hkv), r])
                    L.orc_vec_dot_f16(K, C.byref(s), O.ptr(x), O.ptr(y))
                    out[i13, h, t, r] = s.value
    return out


def cache_views(ctx, a):
    """a (Hkv, n, K) as the K cache is viewed ([K, n, Hkv], nb1 = K*Hkv*2: token-major rows) and as
    the V cache is ([K, n, Hkv], nb1 = ctx*2, nb2 = ctx*n*2: rows of a longer context)."""
    L = X.api()
    Hkv, n, K = a.shape
    kc = np.full((n + 2, Hkv, K), 0x7BFF, np.uint16)  # rows past n: f16 max, never read
    kc[:n] = a.transpose(1, 0, 2)
    yield "k_cache", L.ggml_view_3d(ctx, X.leaf(ctx, kc.reshape(-1)), K, n, Hkv, K * Hkv * 2, K * 2, 0)
    nctx = K + 3
    vc = np.full((Hkv, n, nctx), 0x7BFF, np.uint16)
    vc[:, :, :K] = a
    yield "v_cache", L.ggml_view_3d(ctx, X.leaf(ctx, vc.reshape(-1)), K, n, Hkv, nctx * 2, nctx * n * 2, 0)


@gpu
@pytest.mark.parametrize("K", [1, 31, 32, 33, 95, 256, 257])
def test_mul_mat_f16_cache_views(ctx, K):
    L = X.api()
    n, T = 5, 3
    rng = np.random.default_rng(K)
    shapes = [(2, 2, 1), (4, 2, 1), (8, 1, 1)] + ([(4, 2, 2)] if K == 33 else [])
    for H, Hkv, n13 in shapes:
        a = rng.standard_normal((Hkv, n, K)).astype(np.float16).view(np.uint16)
        b = rng.standard_normal((n13, H, T, K)).astype(F)  # rounds when converted to f16
        assert not np.array_equal(b.astype(np.float16).astype(F), b) or K < 4
        ref = ref_mul_mat_f16(a, b)
        for name, av in cache_views(ctx, a):
            # b [K, T, H, ne13] as permute(0,2,1,3) of a contiguous [K, H, T, ne13]
            bt = L.ggml_permute(ctx, X.leaf(ctx, b.transpose(0, 2, 1, 3)), 0, 2, 1, 3)
            assert tuple(bt.contents.ne) == (K, T, H, n13)
            got = X.run(ctx, L.ggml_mul_mat(ctx, av, bt))
            assert same(got, ref), (K, H, Hkv, n13, name)


# ---- MUL_MAT, Q4_0 / Q8_0 src0 ----------------------------------------------------------------
def activations(rng, cols, K):
    x = rng.standard_normal((cols, K)).astype(F)
    x[0, :32] = 0.0  # an all-zero block: Q8_0 d = 0
    if cols > 1:
        x[1, 7] = -50.0  # a negative maximum
    return x


def ref_mul_mat_q(w, wtype, rows, K, x):
    wd, rs = O.mul_mat_init(wtype, x)
    return O.mul_mat(w, wtype, rows, w.size // rows, K, wd, rs, x.shape[0])


@gpu
@pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])
@pytest.mark.parametrize("rows,K,cols", [(40, 96, 3), (33, 512, 5), (100, 2048, 37), (8, 32, 4), (8, 32, 5)])
def test_mul_mat_quantized_in_graph(ctx, wtype, rows, K, cols):
    rng = np.random.default_rng(rows + K + cols)
    w = quant_weight(wtype, rows, K, rows * 3 + K)
    x = activations(rng, cols, K)
    got = X.run(ctx, X.api().ggml_mul_mat(ctx, X.qleaf(ctx, wtype, K, rows, w), X.leaf(ctx, x)))
    assert same(got[0, 0], ref_mul_mat_q(w, wtype, rows, K, x))


@gpu
@pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])
def test_mul_mat_quantized_3d_src1(ctx, wtype):
    rows, K = 40, 96
    rng = np.random.default_rng(21)
    w = quant_weight(wtype, rows, K, 22)
    x = activations(rng, 6, K)
    bt = X.leaf(ctx, x.reshape(2, 3, K))  # [K, 3, 2]: six columns
    got = X.run(ctx, X.api().ggml_mul_mat(ctx, X.qleaf(ctx, wtype, K, rows, w), bt))
    assert got.shape == (1, 2, 3, rows)
    assert same(got.reshape(6, rows), ref_mul_mat_q(w, wtype, rows, K, x))


@gpu
@pytest.mark.parametrize("wtype", [O.Q4_0, O.Q8_0], ids=["q4_0", "q8_0"])
@pytest.mark.parametrize("cols", [3, 6])
def test_mul_mat_quantized_row_range_views(ctx, wtype, cols):
    """src0 as contiguous row ranges of a larger weight: rows 24..39, rows 1..16 (a start that is no
    multiple of 4 bytes for Q4_0's 54-byte and Q8_0's 102-byte rows), then the whole weight, then
    rows 0..15 and a [K/2, 2*rows] reshape, which share the whole weight's data pointer (the tiled
    copy is cached per (pointer, type, shape))."""
    L = X.api()
    rows, K = 48, 96
    rng = np.random.default_rng(23 + cols)
    w = quant_weight(wtype, rows, K, 24)
    rb = w.shape[1]
    big = X.qleaf(ctx, wtype, K, rows, w)
    x = activations(rng, cols, K)
    xt = X.leaf(ctx, x)
    part = L.ggml_view_2d(ctx, big, K, 16, rb, 24 * rb)
    assert same(X.run(ctx, L.ggml_mul_mat(ctx, part, xt))[0, 0], ref_mul_mat_q(w[24:40], wtype, 16, K, x))
    odd = L.ggml_view_2d(ctx, big, K, 16, rb, 1 * rb)
    assert same(X.run(ctx, L.ggml_mul_mat(ctx, odd, xt))[0, 0], ref_mul_mat_q(w[1:17], wtype, 16, K, x))
    assert same(X.run(ctx, L.ggml_mul_mat(ctx, big, xt))[0, 0], ref_mul_mat_q(w, wtype, rows, K, x))
    head = L.ggml_view_2d(ctx, big, K, 16, rb, 0)
    assert same(X.run(ctx, L.ggml_mul_mat(ctx, head, xt))[0, 0], ref_mul_mat_q(w[:16], wtype, 16, K, x))
    # the same bytes as [32, 3 * rows]: three rows of 32 per row of 96
    x32 = activations(rng, cols, 32)
    flat = L.ggml_view_2d(ctx, big, 32, 3 * rows, rb // 3, 0)
    got = X.run(ctx, L.ggml_mul_mat(ctx, flat, X.leaf(ctx, x32)))
    assert same(got[0, 0], ref_mul_mat_q(w.reshape(3 * rows, rb // 3), wtype, 3 * rows, 32, x32))


# ---- the leaf-mirror and tiled-weight caches ---------------------------------------------------
@gpu
@pytest.mark.parametrize("view", [False, True], ids=["leaf", "row_range_view"])
@pytest.mark.parametrize("cols", [2, 7])
def test_caches_do_not_outlive_their_context(cols, view):
    """two contexts of one size back to back (ggml_init hands the freed arena out again, so every
    host pointer repeats): same graph, other data; the second result must be the second data's"""
    L = X.api()
    rows, K = 24, 64
    results = []
    for k in range(2):
        c = X.new_ctx(3 << 20)
        try:
            rng = np.random.default_rng(100 + k)
            w = quant_weight(O.Q4_0, rows, K, 200 + k)
            x = activations(rng, cols, K)
            wt = X.qleaf(c, O.Q4_0, K, rows, w)
            if view:
                wt = L.ggml_view_2d(c, wt, K, 16, w.shape[1], 1 * w.shape[1])
                w = w[1:17]
            got = X.run(c, L.ggml_mul_mat(c, wt, X.leaf(c, x)))
            results.append((wt.contents.data, got[0, 0], ref_mul_mat_q(w, O.Q4_0, w.shape[0], K, x)))
        finally:
            L.ggml_free(c)
    assert results[0][0] == results[1][0], "the arena was not reused: the test does not reach the caches"
    assert not same(results[0][2], results[1][2])
    for _, got, ref in results:
        assert same(got, ref)


@gpu
@pytest.mark.parametrize("cols", [2, 7])
def test_weight_rewritten_in_a_backend_buffer(cols):
    """a quantized weight in a backend buffer, rewritten by ggml_backend_tensor_set and by
    ggml_backend_buffer_clear between computes of one graph (whole weight and a row-range view): the
    tiled copy of the old bytes must not be served"""
    L = X.api()
    rows, K = 24, 64
    rng = np.random.default_rng(300 + cols)
    wctx, cctx, buf = X.new_ctx(1 << 16, no_alloc=True), X.new_ctx(1 << 20), None
    try:
        wt = L.ggml_new_tensor_2d(wctx, O.Q4_0, K, rows)
        buf = L.ggml_backend_alloc_ctx_tensors_from_buft(wctx, L.ggml_backend_cpu_buffer_type())
        rb = K // 32 * 18
        x = activations(rng, cols, K)
        xt = X.leaf(cctx, x)
        full = L.ggml_mul_mat(cctx, wt, xt)
        part = L.ggml_mul_mat(cctx, L.ggml_view_2d(cctx, wt, K, 16, rb, 1 * rb), xt)
        gf, gp = X.graph(cctx, full), X.graph(cctx, part)
        refs = []
        for k in range(2):
            w = quant_weight(O.Q4_0, rows, K, 400 + k)
            L.ggml_backend_tensor_set(wt, O.ptr(w), 0, w.nbytes)
            for g, out, ws in ((gf, full, w), (gp, part, w[1:17])):
                assert X.compute_status(cctx, g) == 0, G.last_error()
                refs.append(ref_mul_mat_q(ws, O.Q4_0, ws.shape[0], K, x))
                assert same(X.get_array(out)[0, 0], refs[-1]), k
        assert not same(refs[0], refs[2])
        L.ggml_backend_buffer_clear(buf, 0)  # all-zero blocks: d = 0
        for g, out in ((gf, full), (gp, part)):
            assert X.compute_status(cctx, g) == 0, G.last_error()
            got = X.get_array(out)[0, 0]
            assert same(got, np.zeros_like(got))
    finally:
        L.ggml_free(cctx)
        if buf:
            L.ggml_backend_buffer_free(buf)
        L.ggml_free(wctx)


# ---- refusals ---------------------------------------------------------------------------------
def refused(ctx, node, word):
    assert X.compute_status(ctx, X.graph(ctx, node)) != 0
    assert word in G.last_error(), G.last_error()
    # the next valid compute in the process is exact
    a = np.arange(12, dtype=F).reshape(3, 4) / 7
    assert same(X.run(ctx, X.api().ggml_scale(ctx, X.leaf(ctx, a), 0.3))[0, 0], a * F(0.3))


@gpu
def test_refuses_a_non_contiguous_last_node(ctx):
    L = X.api()
    a = X.leaf(ctx, np.ones((3, 4), F))
    refused(ctx, L.ggml_transpose(ctx, L.ggml_scale(ctx, a, 2.0)), "not contiguous")


@gpu
def test_refuses_f16_src1(ctx):
    L = X.api()
    a = X.leaf(ctx, np.zeros((2, 32), np.uint16))
    b = X.leaf(ctx, np.zeros((3, 32), np.uint16))
    refused(ctx, L.ggml_mul_mat(ctx, a, b), "src1 must be f32")


@gpu
def test_refuses_strided_src1_rows_for_a_quantized_src0(ctx):
    L = X.api()
    a = X.qleaf(ctx, O.Q4_0, 32, 8, quant_weight(O.Q4_0, 8, 32, 1))
    b = L.ggml_view_2d(ctx, X.leaf(ctx, np.ones((3, 40), F)), 32, 3, 40 * 4, 0)
    refused(ctx, L.ggml_mul_mat(ctx, a, b), "contiguous src1 rows")


@gpu
@pytest.mark.parametrize("wtype", [O.Q4_K, O.Q6_K])
def test_refuses_a_kquant_k_not_multiple_of_256(ctx, wtype):
    L = X.api()
    a = L.ggml_new_tensor_2d(ctx, wtype, 384, 2)
    C.memset(a.contents.data, 0, L.ggml_nbytes(a))
    refused(ctx, L.ggml_mul_mat(ctx, a, X.leaf(ctx, np.ones((1, 384), F))), "K % 256")


@gpu
@pytest.mark.parametrize("n_dims,mode", [(64, 0), (64, 4), (63, 2)])
def test_refuses_other_rope_forms(ctx, n_dims, mode):
    x = X.leaf(ctx, np.ones((2, 3, 64), F))
    refused(ctx, rope_node(ctx, x, [0, 1], n_dims, 10000.0, mode=mode), "only NEOX")


@gpu
def test_refuses_soft_max_max_bias(ctx):
    a = X.leaf(ctx, np.ones((2, 3, 8), F))
    refused(ctx, X.api().ggml_soft_max_ext(ctx, a, None, None, 1.0, 8.0), "ALiBi")
