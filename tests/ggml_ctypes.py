"""ctypes binding of the ggml surface of include/ggml.h (libgemma_hip.so, csrc/ggml_api.cpp).

TEST INFRASTRUCTURE ONLY.  The builders touch no device, so `api()` works on a CPU-only machine;
`compute` / `run` need the GPU.  Shapes follow ggml: ne = [ne0, ne1, ne2, ne3] is the NumPy shape
reversed, so a NumPy array of shape (ne3, ne2, ne1, ne0) has the memory layout of the tensor.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import gemma_hip as G

F32, F16, Q4_0, Q8_0, Q4_K, Q6_K, I32 = 0, 1, 2, 8, 12, 14, 26
NP_OF = {F32: np.float32, F16: np.uint16, I32: np.int32}
T = C.POINTER(G.GgmlTensor)
PKG = os.path.dirname(os.path.dirname(os.path.abspath(G.__file__)))
DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ggml_driver", "gemma_graph_driver")


def build_driver():
    """The graph driver (tests/ggml_driver/gemma_graph_driver) is a product of the default
    `make -C gemma.ggml_amd`, kept next to its source.  Where it is missing while the library is
    built and up to date, run that default make again: all it then does is link the driver.  A stale
    or missing library is left alone (no compile from inside a test run)."""
    mk = ["make", "-s", "-C", PKG]
    if not os.path.exists(DRIVER) and subprocess.run(mk + ["-q", "lib/libgemma_hip.so"]).returncode == 0:
        subprocess.run(mk)
    return DRIVER


class InitParams(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


_bound = False


def _api():
    global _bound
    L = G.lib()
    if _bound:
        return L
    vp, i64, sz, f32, i = C.c_void_p, C.c_int64, C.c_size_t, C.c_float, C.c_int
    sigs = {
        "ggml_init": (vp, [InitParams]),
        "ggml_free": (None, [vp]),
        "ggml_type_size": (sz, [i]),
        "ggml_blck_size": (i64, [i]),
        "ggml_row_size": (sz, [i, i64]),
        "ggml_element_size": (sz, [T]),
        "ggml_nelements": (i64, [T]),
        "ggml_nbytes": (sz, [T]),
        "ggml_new_tensor": (T, [vp, i, i, C.POINTER(i64)]),
        "ggml_new_tensor_1d": (T, [vp, i, i64]),
        "ggml_new_tensor_2d": (T, [vp, i, i64, i64]),
        "ggml_new_tensor_3d": (T, [vp, i, i64, i64, i64]),
        "ggml_view_1d": (T, [vp, T, i64, sz]),
        "ggml_view_2d": (T, [vp, T, i64, i64, sz, sz]),
        "ggml_view_3d": (T, [vp, T, i64, i64, i64, sz, sz, sz]),
        "ggml_reshape_2d": (T, [vp, T, i64, i64]),
        "ggml_reshape_3d": (T, [vp, T, i64, i64, i64]),
        "ggml_permute": (T, [vp, T, i, i, i, i]),
        "ggml_transpose": (T, [vp, T]),
        "ggml_cont_2d": (T, [vp, T, i64, i64]),
        "ggml_get_rows": (T, [vp, T, T]),
        "ggml_scale": (T, [vp, T, f32]),
        "ggml_rms_norm": (T, [vp, T, f32]),
        "ggml_mul": (T, [vp, T, T]),
        "ggml_add": (T, [vp, T, T]),
        "ggml_mul_mat": (T, [vp, T, T]),
        "ggml_rope_custom": (T, [vp, T, T, i, i, i, i, f32, f32, f32, f32, f32, f32]),
        "ggml_soft_max_ext": (T, [vp, T, T, T, f32, f32]),
        "ggml_gelu": (T, [vp, T]),
        "ggml_cpy": (T, [vp, T, T]),
        "ggml_new_graph": (vp, [vp]),
        "ggml_build_forward_expand": (None, [vp, T]),
        "ggml_graph_compute_with_ctx": (i, [vp, vp, i]),
        "ggml_backend_cpu_buffer_type": (vp, []),
        "ggml_backend_alloc_ctx_tensors_from_buft": (vp, [vp, vp]),
        "ggml_backend_buffer_clear": (None, [vp, C.c_uint8]),
        "ggml_backend_buffer_name": (C.c_char_p, [vp]),
        "ggml_backend_buffer_get_size": (sz, [vp]),
        "ggml_backend_buffer_free": (None, [vp]),
        "ggml_backend_tensor_set": (None, [T, vp, sz, sz]),
        "ggml_backend_tensor_get": (None, [T, vp, sz, sz]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _bound = True
    return L


api = _api


def new_ctx(mem_size=16 << 20, no_alloc=False):
    return _api().ggml_init(InitParams(mem_size, None, no_alloc))


def tensor(ctx, gtype, *ne):
    """A new tensor of ggml type `gtype` and ggml shape ne (1 to 4 dims)."""
    return _api().ggml_new_tensor(ctx, gtype, len(ne), (C.c_int64 * len(ne))(*ne))


def _put(t, arr):
    b = np.ascontiguousarray(arr).view(np.uint8).ravel()
    C.memmove(t.contents.data, b.ctypes.data, b.size)


put = _put


def leaf(ctx, arr):
    """A contiguous F32 / F16 (uint16 bits) / I32 leaf holding `arr` (ggml shape = arr.shape reversed)."""
    arr = np.ascontiguousarray(arr)
    gtype = {np.dtype(np.float32): F32, np.dtype(np.uint16): F16, np.dtype(np.int32): I32}[arr.dtype]
    t = tensor(ctx, gtype, *arr.shape[::-1])
    _put(t, arr)
    return t


def qleaf(ctx, gtype, K, rows, data):
    """A quantized [K, rows] leaf holding the row bytes `data`."""
    t = _api().ggml_new_tensor_2d(ctx, gtype, K, rows)
    assert _api().ggml_nbytes(t) == np.asarray(data).size, (_api().ggml_nbytes(t), np.asarray(data).size)
    _put(t, data)
    return t


def _get(t, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(t.contents.data)).copy()


def get_array(t):
    """The host data of a contiguous F32 / F16 / I32 tensor as an array of shape (ne3, ne2, ne1, ne0)."""
    tc = t.contents
    dt = NP_OF[tc.type]
    n = int(np.prod(list(tc.ne)))
    raw = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(tc.data)
    return np.frombuffer(raw, dtype=dt).copy().reshape(tuple(tc.ne)[::-1])


def _compute(L, ctx, out):
    g = L.ggml_new_graph(ctx)
    L.ggml_build_forward_expand(g, out)
    assert L.ggml_graph_compute_with_ctx(ctx, g, 1) == 0, G.last_error()


def graph(ctx, *outs):
    L = _api()
    g = L.ggml_new_graph(ctx)
    for o in outs:
        L.ggml_build_forward_expand(g, o)
    return g


def compute_status(ctx, g):
    return _api().ggml_graph_compute_with_ctx(ctx, g, 1)


def run(ctx, *outs):
    """Expand `outs` in order, compute, and return the last node (the only one the executor copies
    back; it must be contiguous) as an array of shape (ne3, ne2, ne1, ne0)."""
    g = graph(ctx, *outs)
    assert compute_status(ctx, g) == 0, G.last_error()
    return get_array(outs[-1])
