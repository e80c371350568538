"""ctypes binding of libgemma_hip.so — the MI355X hot path behind the C-ABI in include/gemma_hpc.h.

Product-side host mirror: it only forwards to the HIP library and never falls back to CPU code.
Loading fails loudly if the library is missing or was not built for gfx950.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libgemma_hip.so")
# GHIP_LIB: an alternative build of the same library, for A/B timing of two builds on one box
# (scripts/lib_ab.sh).  Honoured only with GHIP_ALLOW_ALT_LIB=1, so a stray variable can never make
# a test, smoke() or bench.py load anything but the in-tree build.
if os.environ.get("GHIP_LIB"):
    if os.environ.get("GHIP_ALLOW_ALT_LIB") != "1":
        raise RuntimeError("GHIP_LIB is set but GHIP_ALLOW_ALT_LIB=1 is not: refusing to load a non-tree library")
    LIB_PATH = os.environ["GHIP_LIB"]

GGML_TYPE_F32, GGML_TYPE_F16, GGML_TYPE_Q4_0, GGML_TYPE_Q8_0 = 0, 1, 2, 8
GGML_TYPE_Q4_K, GGML_TYPE_Q6_K, GGML_TYPE_Q8_K = 12, 14, 15

# exported symbols (checked against include/gemma_hpc.h by tests/test_capi_symbols.py)
EXPORTS = ["mul_mat", "hpc_init", "hpc_shutdown", "hpc_register_weight", "hpc_last_error", "hpc_set_error_mode",
           "hpc_weight_cache_entries", "hpc_set_matvec_ks", "hpc_set_gemm_x4", "gemma_engine_debug_step", "gemma_engine_stamp_step", "gemma_engine_create", "gemma_engine_free", "gemma_engine_begin",
           "gemma_engine_step", "gemma_engine_tokens", "gemma_engine_pos", "gemma_engine_prefill",
           "gemma_engine_prefill_fast", "gemma_engine_prefill_taps", "gemma_engine_extend", "gemma_engine_prefill_next", "gemma_test_gemm", "gemma_test_gemm_exact", "gemma_kq_time", "hpc_graph_compute",
           "ggml_init", "ggml_free", "ggml_new_tensor_2d", "ggml_mul_mat", "ggml_graph_compute_with_ctx",
           "gemma_engine_tensor", "gemma_engine_time", "gemma_engine_sync", "gemma_engine_tune",
           "gemma_engine_plan", "gemma_engine_set_plan", "gemma_engine_set_fuse", "gemma_engine_set_att_o", "gemma_engine_set_option", "gemma_engine_set_persist", "gemma_engine_persist_err", "gemma_engine_graph_kernels", "gemma_hbm_read_gbs", "gemma_hbm_read_probe",
           "gemma_tp_unique_id", "gemma_engine_create_tp", "gemma_engine_create_tp2", "gemma_engine_tp_flags", "gemma_engine_p2p_handle", "gemma_engine_p2p_open", "gemma_engine_p2p_err", "gemma_engine_tp_info", "gemma_engine_set_persist_timeout",
           "gguf_init_from_file", "gguf_free", "gguf_get_n_kv", "gguf_get_key", "gguf_get_kv_type",
           "gguf_get_arr_type", "gguf_get_arr_n", "gguf_get_arr_data", "gguf_get_arr_str", "gguf_get_val_str",
           "gguf_get_val_data", "gguf_get_n_tensors", "gguf_get_tensor_name", "gguf_get_tensor_type",
           "gguf_get_tensor_offset", "gguf_get_version", "gguf_get_alignment", "gguf_get_data_offset",
           "gguf_find_key", "gguf_find_tensor", "ggml_get_tensor", "ggml_nbytes",
           "gemma_engine_create_from_gguf", "gemma_engine_config",
           "gemma_engine_set_sampler", "gemma_engine_sampler", "gemma_test_sample",
           "gemma_engine_verify", "gemma_engine_kv_read", "gemma_lookup_draft", "gemma_engine_generate_lookup",
           "gemma_test_gemm_skinny", "gemma_test_gemm_skinny_kq", "gemma_test_matvec", "gemma_hip_mem_live",
           "gemma_engine_batch_open", "gemma_engine_batch_close", "gemma_engine_batch_begin", "gemma_engine_batch_adopt",
           "gemma_engine_batch_release", "gemma_engine_batch_step", "gemma_engine_batch_pos", "gemma_engine_batch_tokens",
           "gemma_engine_batch_last", "gemma_engine_batch_kv_read", "gemma_engine_batch_open_wide",
           "gemma_engine_batch_last_n", "gemma_batch_plan_rows", "gemma_engine_batch_open_rows",
           "gemma_engine_batch_step_rows", "gemma_engine_batch_verify", "gemma_engine_batch_generate_lookup",
           "gemma_engine_set_logprobs", "gemma_engine_logprobs", "gemma_engine_batch_logprobs", "gemma_test_logprob",
           "gemma_engine_set_top_logprobs", "gemma_engine_top_logprobs", "gemma_engine_batch_top_logprobs", "gemma_test_top_logprobs",
           "gemma_engine_batch_set_sampler", "gemma_engine_batch_sampler", "gemma_engine_batch_fork",
           "gemma_test_sample_rows", "gemma_test_rope_kv_prefill", "gemma_test_rows_rope_kv",
           "gemma_test_attn_prefill", "gemma_test_attn_decode_rows", "gemma_test_attn_long_rows",
           "gemma_test_attn_mx_long",
           "gemma_engine_set_penalties", "gemma_engine_penalties", "gemma_test_penalize",
           "gemma_engine_shift", "gemma_engine_batch_shift", "gemma_test_kv_shift"]


def build():
    subprocess.run(["make", "-s", "-j8", "-C", PKG_DIR], check=True)


TP_REP_ATTN = 1  # include/gemma_hpc.h GEMMA_TP_REP_ATTN
TP_P2P = 2       # include/gemma_hpc.h GEMMA_TP_P2P: peer-to-peer gathers instead of RCCL (tp id None)


class GemmaConfig(C.Structure):
    _fields_ = [("n_layer", C.c_int), ("n_embd", C.c_int), ("n_head", C.c_int), ("n_head_kv", C.c_int),
                ("head_dim", C.c_int), ("n_ff", C.c_int), ("n_vocab", C.c_int), ("n_ctx", C.c_int),
                ("wtype", C.c_int), ("eps", C.c_float), ("rope_base", C.c_float), ("seed", C.c_uint64),
                ("gelu_clamp", C.c_int), ("out_type", C.c_int), ("out_gain", C.c_float)]


class GemmaSampler(C.Structure):
    """struct gemma_sampler (include/gemma_hpc.h): temperature <= 0 is greedy."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("seed", C.c_uint64)]


class GemmaPenalties(C.Structure):
    """struct gemma_penalties (include/gemma_hpc.h): repeat 1, presence 0, frequency 0 is off."""
    _fields_ = [("repeat", C.c_float), ("presence", C.c_float), ("frequency", C.c_float), ("last_n", C.c_int)]


PENALTY_MAX_LAST_N = 8192  # include/gemma_hpc.h GEMMA_PENALTY_MAX_LAST_N
SAMPLE_MAX_K = 1024  # candidates at most (top_k == 0 means this many)
TOP_K_ALL = 0x7FFFFFFF  # top_k of the whole-vocabulary sampler (GEMMA_TOP_K_ALL): every entry a candidate, nothing sorted
VERIFY_MAX_DRAFT = 7  # include/gemma_hpc.h GEMMA_VERIFY_MAX_DRAFT
BATCH_MAX_SLOTS = 8   # include/gemma_hpc.h GEMMA_BATCH_MAX_SLOTS
BATCH_WIDE_MAX_SLOTS = 64  # include/gemma_hpc.h GEMMA_BATCH_WIDE_MAX_SLOTS


class SpecStats(C.Structure):
    """struct gemma_spec_stats (include/gemma_hpc.h)."""
    _fields_ = [("passes", C.c_int), ("drafted", C.c_int), ("accepted", C.c_int), ("plain_steps", C.c_int)]


class GgmlTensor(C.Structure):
    """struct ggml_tensor as declared in include/ggml.h (only `data` is read by mul_mat)."""
    _fields_ = [("type", C.c_int), ("backend", C.c_int), ("buffer", C.c_void_p), ("ne", C.c_int64 * 4),
                ("nb", C.c_size_t * 4), ("op", C.c_int32), ("op_params", C.c_int32 * 16), ("flags", C.c_int32),
                ("grad", C.c_void_p), ("src", C.c_void_p * 10), ("perf_runs", C.c_int), ("perf_cycles", C.c_int64),
                ("perf_time_us", C.c_int64), ("view_src", C.c_void_p), ("view_offs", C.c_size_t),
                ("data", C.c_void_p), ("name", C.c_char * 64), ("extra", C.c_void_p), ("padding", C.c_char * 8)]


class GGUFInitParams(C.Structure):
    _fields_ = [("no_alloc", C.c_bool), ("ctx", C.POINTER(C.c_void_p))]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libgemma_hip.so not built ({LIB_PATH}); run `make -C {PKG_DIR}` or "
                           "__graft_entry__.build() — there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i64 = C.c_void_p, C.c_int64
    L.mul_mat.restype = None
    L.mul_mat.argtypes = [i64, i64, i64, i64, i64, i64, i64, C.c_size_t, i64, vp, vp, vp, vp, C.c_int, vp]
    L.hpc_init.restype = C.c_int
    L.hpc_init.argtypes = [C.c_int]
    L.hpc_register_weight.restype = C.c_int
    L.hpc_register_weight.argtypes = [vp, C.c_int, i64, i64, C.c_size_t]
    L.hpc_last_error.restype = C.c_int
    L.hpc_last_error.argtypes = [C.c_char_p, C.c_size_t]
    L.hpc_set_error_mode.argtypes = [C.c_int]
    L.hpc_weight_cache_entries.restype = C.c_int
    L.gemma_hip_mem_live.argtypes = [C.POINTER(i64), C.POINTER(i64)]
    L.hpc_set_matvec_ks.argtypes = [C.c_int]
    L.hpc_set_gemm_x4.argtypes = [C.c_int]
    L.hpc_set_gemm_x4.restype = None
    L.gemma_engine_debug_step.restype = C.c_int
    L.gemma_engine_debug_step.argtypes = [vp, vp, vp]
    L.gemma_engine_stamp_step.restype = C.c_int
    L.gemma_engine_stamp_step.argtypes = [vp, C.c_int, vp]
    L.gemma_tp_unique_id.restype = C.c_int
    L.gemma_tp_unique_id.argtypes = [vp, C.c_int]
    L.gemma_engine_create_tp.restype = vp
    L.gemma_engine_create_tp.argtypes = [C.POINTER(GemmaConfig), C.c_int, C.c_int, C.c_int, vp]
    L.gemma_engine_create_tp2.restype = vp
    L.gemma_engine_create_tp2.argtypes = [C.POINTER(GemmaConfig), C.c_int, C.c_int, C.c_int, vp, C.c_int]
    L.gemma_engine_tp_flags.restype = C.c_int
    L.gemma_engine_tp_flags.argtypes = [vp]
    L.gemma_engine_p2p_handle.restype = C.c_int
    L.gemma_engine_p2p_handle.argtypes = [vp, vp, C.c_int]
    L.gemma_engine_p2p_open.restype = C.c_int
    L.gemma_engine_p2p_open.argtypes = [vp, vp, C.c_int]
    L.gemma_engine_p2p_err.restype = C.c_int
    L.gemma_engine_p2p_err.argtypes = [vp, C.c_int]
    L.gemma_engine_create.restype = vp
    L.gemma_engine_create.argtypes = [C.POINTER(GemmaConfig), C.c_int]
    L.gemma_engine_free.argtypes = [vp]
    L.gemma_engine_begin.restype = C.c_int
    L.gemma_engine_begin.argtypes = [vp, vp, C.c_int]
    L.gemma_engine_step.restype = C.c_int
    L.gemma_engine_step.argtypes = [vp, C.c_int, vp, C.c_int]
    L.gemma_engine_tokens.restype = C.c_int
    L.gemma_engine_tokens.argtypes = [vp, vp, C.c_int]
    L.gemma_engine_pos.restype = C.c_int
    L.gemma_engine_pos.argtypes = [vp]
    L.gemma_engine_prefill.restype = C.c_int
    L.gemma_engine_prefill.argtypes = [vp, vp, vp]
    L.gemma_engine_prefill_fast.restype = C.c_int
    L.gemma_engine_prefill_fast.argtypes = [vp, vp, vp]
    L.gemma_engine_prefill_taps.restype = C.c_int
    L.gemma_engine_prefill_taps.argtypes = [vp, vp, C.c_int]
    L.gemma_engine_extend.restype = C.c_int
    L.gemma_engine_extend.argtypes = [vp, C.c_int, vp, C.c_int]
    L.gemma_engine_prefill_next.restype = C.c_int
    L.gemma_engine_prefill_next.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.gemma_engine_tensor.restype = C.c_int64
    L.gemma_engine_tensor.argtypes = [vp, C.c_int, vp, i64]
    L.gemma_engine_tune.argtypes = [vp, C.c_int]
    L.gemma_engine_plan.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.gemma_engine_set_plan.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.gemma_engine_set_fuse.argtypes = [vp, C.c_int]
    L.gemma_engine_set_att_o.argtypes = [vp, C.c_int]
    L.gemma_engine_set_option.restype = C.c_int
    L.gemma_engine_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.gemma_engine_set_persist.argtypes = [vp, C.c_int]
    L.gemma_engine_persist_err.argtypes = [vp, vp, C.c_int]
    L.gemma_engine_set_persist_timeout.argtypes = [vp, C.c_uint]
    L.gemma_engine_tp_info.argtypes = [vp, vp]
    L.gemma_engine_graph_kernels.argtypes = [vp]
    L.gemma_engine_time.restype = C.c_double
    L.gemma_engine_time.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.gemma_kq_time.restype = C.c_double
    L.gemma_kq_time.argtypes = [C.c_int, i64, i64, C.c_int, C.POINTER(C.c_double)]
    L.gemma_hbm_read_gbs.restype = C.c_double
    L.gemma_hbm_read_gbs.argtypes = [C.c_int, C.c_size_t, C.c_int]
    L.gemma_hbm_read_probe.restype = C.c_double
    L.gemma_hbm_read_probe.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_int]
    L.gemma_engine_sync.restype = C.c_int
    L.gemma_engine_sync.argtypes = [vp]
    L.gemma_engine_create_from_gguf.restype = vp
    L.gemma_engine_create_from_gguf.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.gemma_engine_config.restype = C.c_int
    L.gemma_engine_config.argtypes = [vp, C.POINTER(GemmaConfig)]
    L.gemma_engine_set_sampler.restype = C.c_int
    L.gemma_engine_set_sampler.argtypes = [vp, C.POINTER(GemmaSampler)]
    L.gemma_engine_sampler.restype = C.c_int
    L.gemma_engine_sampler.argtypes = [vp, C.POINTER(GemmaSampler)]
    L.gemma_test_sample.restype = C.c_int
    L.gemma_test_sample.argtypes = [vp, C.c_int, C.c_int, C.POINTER(GemmaSampler), vp, vp, vp, vp, vp]
    L.gemma_test_sample_rows.restype = C.c_int
    L.gemma_test_sample_rows.argtypes = [vp, C.c_int, C.c_int, C.POINTER(GemmaSampler), vp, vp, vp, vp, vp]
    L.gemma_engine_set_penalties.restype = C.c_int
    L.gemma_engine_set_penalties.argtypes = [vp, C.POINTER(GemmaPenalties)]
    L.gemma_engine_penalties.restype = C.c_int
    L.gemma_engine_penalties.argtypes = [vp, C.POINTER(GemmaPenalties)]
    L.gemma_test_penalize.restype = C.c_int
    L.gemma_test_penalize.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.POINTER(GemmaPenalties), vp, vp, vp]
    L.gemma_engine_shift.restype = C.c_int
    L.gemma_engine_shift.argtypes = [vp, C.c_int, C.c_int]
    L.gemma_engine_batch_shift.restype = C.c_int
    L.gemma_engine_batch_shift.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.gemma_test_kv_shift.restype = C.c_int
    L.gemma_test_kv_shift.argtypes = [vp, vp] + [C.c_int] * 6 + [C.c_float]
    L.gemma_engine_verify.restype = C.c_int
    L.gemma_engine_verify.argtypes = [vp, vp, C.c_int, vp, vp]
    L.gemma_engine_kv_read.restype = C.c_int
    L.gemma_engine_kv_read.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.gemma_lookup_draft.restype = C.c_int
    L.gemma_lookup_draft.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.gemma_engine_generate_lookup.restype = C.c_int
    L.gemma_engine_generate_lookup.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(SpecStats)]
    L.gemma_test_gemm_skinny.restype = C.c_int
    L.gemma_test_gemm_skinny.argtypes = [C.c_int, i64, i64, i64, vp, vp, vp, vp]
    L.gemma_test_gemm_skinny_kq.restype = C.c_int
    L.gemma_test_gemm_skinny_kq.argtypes = [C.c_int, i64, i64, i64, C.c_int, vp, vp, vp, vp]
    for fn, at in (("open", [C.c_int]), ("close", []), ("begin", [C.c_int, vp, C.c_int]), ("adopt", [C.c_int]),
                   ("release", [C.c_int]), ("step", [C.c_int, vp]), ("pos", [C.c_int]), ("tokens", [C.c_int, vp, C.c_int]),
                   ("last", [vp]), ("kv_read", [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
                   ("open_wide", [C.c_int]), ("last_n", [vp, C.c_int]), ("open_rows", [C.c_int, C.c_int]),
                   ("step_rows", [C.c_int, vp, vp]), ("verify", [vp, vp, vp, vp, vp]),
                   ("generate_lookup", [C.c_int, C.c_int, C.c_int, vp, C.POINTER(SpecStats)]),
                   ("set_sampler", [C.c_int, C.POINTER(GemmaSampler)]),
                   ("sampler", [C.c_int, C.POINTER(GemmaSampler), C.POINTER(C.c_int)]), ("fork", [C.c_int, C.c_int])):
        getattr(L, "gemma_engine_batch_" + fn).restype = C.c_int
        getattr(L, "gemma_engine_batch_" + fn).argtypes = [vp] + at
    L.gemma_batch_plan_rows.restype = C.c_int
    L.gemma_batch_plan_rows.argtypes = [vp, C.c_int, C.c_int, vp]
    L.gemma_engine_set_logprobs.restype = C.c_int
    L.gemma_engine_set_logprobs.argtypes = [vp, C.c_int]
    L.gemma_engine_logprobs.restype = C.c_int
    L.gemma_engine_logprobs.argtypes = [vp, C.c_int, C.c_int, vp]
    L.gemma_engine_batch_logprobs.restype = C.c_int
    L.gemma_engine_batch_logprobs.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.gemma_test_logprob.restype = C.c_int
    L.gemma_test_logprob.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.gemma_engine_set_top_logprobs.restype = C.c_int
    L.gemma_engine_set_top_logprobs.argtypes = [vp, C.c_int]
    L.gemma_engine_top_logprobs.restype = C.c_int
    L.gemma_engine_top_logprobs.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.gemma_engine_batch_top_logprobs.restype = C.c_int
    L.gemma_engine_batch_top_logprobs.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.gemma_test_top_logprobs.restype = C.c_int
    L.gemma_test_top_logprobs.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    # GGUF reader (include/ggml.h)
    L.gguf_init_from_file.restype = vp
    L.gguf_init_from_file.argtypes = [C.c_char_p, GGUFInitParams]
    L.gguf_free.argtypes = [vp]
    for fn in ("gguf_get_n_kv", "gguf_get_n_tensors", "gguf_get_version"):
        getattr(L, fn).restype = C.c_int
        getattr(L, fn).argtypes = [vp]
    for fn in ("gguf_get_alignment", "gguf_get_data_offset"):
        getattr(L, fn).restype = C.c_size_t
        getattr(L, fn).argtypes = [vp]
    for fn, rt in (("gguf_get_key", C.c_char_p), ("gguf_get_kv_type", C.c_int), ("gguf_get_arr_type", C.c_int),
                   ("gguf_get_arr_n", C.c_int), ("gguf_get_arr_data", vp), ("gguf_get_val_str", C.c_char_p),
                   ("gguf_get_val_data", vp), ("gguf_get_tensor_name", C.c_char_p),
                   ("gguf_get_tensor_type", C.c_int), ("gguf_get_tensor_offset", C.c_size_t)):
        getattr(L, fn).restype = rt
        getattr(L, fn).argtypes = [vp, C.c_int]
    L.gguf_get_arr_str.restype = C.c_char_p
    L.gguf_get_arr_str.argtypes = [vp, C.c_int, C.c_int]
    L.gguf_find_key.restype = C.c_int
    L.gguf_find_key.argtypes = [vp, C.c_char_p]
    L.gguf_find_tensor.restype = C.c_int
    L.gguf_find_tensor.argtypes = [vp, C.c_char_p]
    L.ggml_get_tensor.restype = C.POINTER(GgmlTensor)
    L.ggml_get_tensor.argtypes = [vp, C.c_char_p]
    L.ggml_nbytes.restype = C.c_size_t
    L.ggml_nbytes.argtypes = [C.POINTER(GgmlTensor)]
    L.ggml_free.restype = None
    L.ggml_free.argtypes = [vp]
    _lib = L
    return L


def last_error():
    buf = C.create_string_buffer(1024)
    lib().hpc_last_error(buf, 1024)
    return buf.value.decode()


def mem_live():
    """(live allocations, live bytes) of the whole library: gemma_hip_mem_live."""
    n, b = C.c_int64(), C.c_int64()
    lib().gemma_hip_mem_live(C.byref(n), C.byref(b))
    return n.value, b.value


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def mul_mat(src0_bytes, src0_type, ne01, nb01, shared_edge, wdata, row_size, ncols, ne1=None, nb1=None, nb2=None):
    """Call the drop-in `mul_mat` (src/hpc.h:22-32 signature) on host buffers; returns dst [ncols][ne01]."""
    L = lib()
    ne1 = ncols if ne1 is None else ne1
    nb1 = ne01 * 4 if nb1 is None else nb1
    nb2 = nb1 * ne1 if nb2 is None else nb2
    ne12 = ncols // ne1
    span = max((c % ne1) * nb1 + (c // ne1) * nb2 for c in range(ncols)) + ne01 * 4
    raw = np.zeros((span + 3) // 4, dtype=np.float32)
    dst = raw
    t0, t1 = GgmlTensor(), GgmlTensor()
    t0.data = src0_bytes.ctypes.data
    t0.type = src0_type
    t1.data = dst.ctypes.data
    t1.type = GGML_TYPE_F32
    L.mul_mat(ne01, ne1, ne12, nb01, ne1, nb1, nb2, row_size, shared_edge, C.byref(t0), None, C.byref(t1), None,
              src0_type, _p(wdata))
    out = np.empty((ncols, ne01), dtype=np.float32)
    for c in range(ncols):
        off = ((c % ne1) * nb1 + (c // ne1) * nb2) // 4
        out[c] = raw[off:off + ne01]
    return out


class Engine:
    def __init__(self, shape, n_ctx=512, wtype=GGML_TYPE_Q4_0, seed=0x6E6D6D61, eps=1e-6, rope_base=10000.0,
                 gelu_clamp=0, device=0, tp=None, out_type=0, out_gain=0.0, tp_flags=0):
        """tp = (n_ranks, rank, rccl_id_bytes) for the row-split engine (one process per GPU);
        rccl_id_bytes None = all ranks' shards virtual in this engine (single-GPU parity mode).
        tp_flags: TP_REP_ATTN keeps the attention block (Wq|Wk|Wv, Wo) whole on every rank."""
        self.cfg = GemmaConfig(n_ctx=n_ctx, wtype=wtype, eps=eps, rope_base=rope_base, seed=seed,
                               gelu_clamp=gelu_clamp, out_type=out_type, out_gain=out_gain, **shape)
        self.L = lib()
        if tp is not None and (tp[0] > 1 or tp[2] is not None):  # n_ranks 1 + id: a 1-rank RCCL comm
            idbuf = C.create_string_buffer(bytes(tp[2]), len(tp[2])) if tp[2] is not None else None
            self.h = self.L.gemma_engine_create_tp2(C.byref(self.cfg), device, tp[0], tp[1], idbuf, tp_flags)
        else:
            self.h = self.L.gemma_engine_create(C.byref(self.cfg), device)
        if not self.h:
            raise RuntimeError("gemma_engine_create failed: " + last_error())

    @classmethod
    def from_gguf(cls, path, n_ctx=512, device=0):
        """An engine on a Gemma GGUF file's weights (gemma_engine_create_from_gguf)."""
        self = cls.__new__(cls)
        self.L = lib()
        self.h = self.L.gemma_engine_create_from_gguf(path.encode(), n_ctx, device)
        if not self.h:
            raise RuntimeError("gemma_engine_create_from_gguf failed: " + last_error())
        self.cfg = GemmaConfig()
        self.L.gemma_engine_config(self.h, C.byref(self.cfg))
        return self

    def close(self):
        if self.h:
            self.L.gemma_engine_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r, what):
        if r != 0:
            raise RuntimeError(f"{what} failed: {last_error()}")

    def begin(self, prompt):
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        self._chk(self.L.gemma_engine_begin(self.h, _p(p), len(p)), "begin")
        self._n_seq = len(p)  # host-given tokens (positions [0, n_seq)); extend() moves it

    def pos(self):
        """number of processed positions"""
        return self.L.gemma_engine_pos(self.h)

    def extend(self, tokens, keep=None):
        """Continue or rewind: positions [0, keep) stay, `tokens` become the next given positions
        (consumed by step() or prefill_next()).  keep=None keeps everything, the pending greedy
        token included, and places `tokens` after it (the next turn of a conversation)."""
        t = [int(x) for x in tokens]
        if keep is None:
            keep = self.pos()
            if keep < getattr(self, "_n_seq", 0):
                raise ValueError(f"extend(keep=None): {self._n_seq - keep} given tokens are not processed yet")
            t = [int(self.tokens()[-1])] + t
        a = np.ascontiguousarray(t, dtype=np.int32)
        self._chk(self.L.gemma_engine_extend(self.h, int(keep), _p(a), len(a)), "extend")
        self._n_seq = int(keep) + len(a)

    def shift(self, keep, discard):
        """Context shift (gemma_engine_shift): positions [keep, keep + discard) are dropped, the rest of
        the caches and of the history moves down and K is rotated back by `discard`; returns the new pos."""
        n = self.L.gemma_engine_shift(self.h, int(keep), int(discard))
        if n < 0:
            raise RuntimeError("shift failed: " + last_error())
        g = getattr(self, "_n_seq", 0)  # given tokens behind the dropped span move with it
        self._n_seq = g if g <= keep else max(int(keep), g - int(discard))
        return n

    def prefill_next(self, n=0, want_all=False, exact=True):
        """One batched pass over the next n given tokens (0: all that remain) from the current
        position; returns (token, last-row logits[, the pass's rows]) like prefill().  The token is
        appended only when the pass reaches the end of the given tokens."""
        rows = n if n > 0 else max(getattr(self, "_n_seq", 0) - self.pos(), 0)
        last = np.zeros(self.cfg.n_vocab, dtype=np.float32)
        allv = np.zeros((rows, self.cfg.n_vocab), dtype=np.float32) if want_all else None
        tok = self.L.gemma_engine_prefill_next(self.h, int(n), 1 if exact else 0, _p(last), _p(allv) if want_all else None)
        if tok < 0:
            raise RuntimeError("prefill_next failed: " + last_error())
        return (tok, last, allv) if want_all else (tok, last)

    def step(self, n, want_logits=False, use_graph=True):
        lg = np.zeros((n, self.cfg.n_vocab), dtype=np.float32) if want_logits else None
        self._chk(self.L.gemma_engine_step(self.h, n, _p(lg) if want_logits else None, 1 if use_graph else 0), "step")
        return lg

    def verify(self, draft, want_all=False):
        """One exact pass over [pending token, drafts] (gemma_engine_verify): draft[i] is a guess for
        sequence index pos + 1 + i.  Returns the tokens appended (the accepted drafts plus the token
        that follows them: 1 .. len(draft) + 1 of them), with want_all also the pass's logits rows
        [len(draft) + 1][n_vocab] (rows past the accepted ones were computed under rejected drafts)."""
        d = np.ascontiguousarray([int(x) for x in draft], dtype=np.int32)
        out = np.zeros(len(d) + 1, dtype=np.int32)
        allv = np.zeros((len(d) + 1, self.cfg.n_vocab), dtype=np.float32) if want_all else None
        n = self.L.gemma_engine_verify(self.h, _p(d), len(d), _p(out), _p(allv) if want_all else None)
        if n < 0:
            raise RuntimeError("verify failed: " + last_error())
        toks = [int(t) for t in out[:n]]
        return (toks, allv) if want_all else toks

    def generate_lookup(self, n_new, k=4, ngram_max=3):
        """n_new tokens by prompt-lookup drafts and verify passes (gemma_engine_generate_lookup): the
        tokens step(n_new) appends, and dict(passes, drafted, accepted, plain_steps)."""
        out = np.zeros(max(int(n_new), 1), dtype=np.int32)
        st = SpecStats()
        r = self.L.gemma_engine_generate_lookup(self.h, int(n_new), int(k), int(ngram_max), _p(out), C.byref(st))
        self._chk(r, "generate_lookup")
        return [int(t) for t in out[:n_new]], dict(passes=st.passes, drafted=st.drafted, accepted=st.accepted,
                                                   plain_steps=st.plain_steps)

    def kv_read(self, layer, p0, n):
        """K rows and V columns p0 .. p0+n of one layer's cache as f16 bits: (k [n][kvw], v [n][kvw])"""
        kvw = self.cfg.n_head_kv * self.cfg.head_dim
        k = np.zeros((n, kvw), dtype=np.uint16)
        v = np.zeros((n, kvw), dtype=np.uint16)
        self._chk(self.L.gemma_engine_kv_read(self.h, int(layer), int(p0), int(n), _p(k), _p(v)), "kv_read")
        return k, v

    # ---- batched decode (gemma_engine_batch_*): up to BATCH_MAX_SLOTS sequences per weight pass ----
    def batch_open(self, n_slots):
        """Open the engine's batch with n_slots (1 .. BATCH_MAX_SLOTS) sequence slots."""
        self._chk(self.L.gemma_engine_batch_open(self.h, int(n_slots)), "batch_open")
        self._bt_slots = int(n_slots)

    def batch_open_wide(self, n_slots):
        """Open the engine's batch with n_slots (1 .. BATCH_WIDE_MAX_SLOTS) sequence slots: passes of
        more than 8 rows run on the exact MFMA GEMMs (option "bt_mfma_min"), the same bits."""
        self._chk(self.L.gemma_engine_batch_open_wide(self.h, int(n_slots)), "batch_open_wide")
        self._bt_slots = int(n_slots)

    def batch_open_rows(self, n_slots, max_rows):
        """batch_open_wide with the pass scratch sized for max_rows rows (max(8, n_slots) .. 64): the
        row capacity of batch_step_rows."""
        self._chk(self.L.gemma_engine_batch_open_rows(self.h, int(n_slots), int(max_rows)), "batch_open_rows")
        self._bt_slots = int(n_slots)

    def batch_step_rows(self, max_rows, want_logits=False):
        """One pass of up to max_rows rows, several per slot that still has given tokens to consume
        (batch_plan_rows states the allotment).  Returns (rows_of [n_slots], logits [T][n_vocab] in
        row order — ascending slot, then position — or None)."""
        rows_of = np.zeros(BATCH_WIDE_MAX_SLOTS, dtype=np.int32)
        lg = np.zeros((max(int(max_rows), 1), self.cfg.n_vocab), dtype=np.float32) if want_logits else None
        T = self.L.gemma_engine_batch_step_rows(self.h, int(max_rows), _p(lg) if want_logits else None, _p(rows_of))
        if T < 0:
            raise RuntimeError("batch_step_rows failed: " + last_error())
        return rows_of[:self._bt_slots].copy(), (lg[:T] if want_logits else None)

    def batch_verify(self, drafts, want_logits=False):
        """One exact pass with per-slot drafts (gemma_engine_batch_verify).  drafts: {slot: draft list}
        or a list by slot; an empty list is a plain row (k = 0), None or a missing slot sits out (-1).
        Returns {slot: tokens appended} for the participating slots, with want_logits also the pass's
        rows [T][n_vocab] in row order (ascending slot, then position)."""
        ns = self._bt_slots
        get = drafts.get if isinstance(drafts, dict) else (lambda s: drafts[s] if s < len(drafts) else None)
        d = np.zeros((ns, VERIFY_MAX_DRAFT), dtype=np.int32)
        k_of = np.full(ns, -1, dtype=np.int32)
        for s in range(ns):
            ds = get(s)
            if ds is None:
                continue
            ds = [int(x) for x in ds]
            k_of[s] = len(ds)
            d[s, :min(len(ds), VERIFY_MAX_DRAFT)] = ds[:VERIFY_MAX_DRAFT]
        out = np.zeros((ns, VERIFY_MAX_DRAFT + 1), dtype=np.int32)
        n_out = np.zeros(ns, dtype=np.int32)
        rows = int(np.clip(k_of, -1, VERIFY_MAX_DRAFT).sum()) + ns
        lg = np.zeros((max(rows, 1), self.cfg.n_vocab), dtype=np.float32) if want_logits else None
        T = self.L.gemma_engine_batch_verify(self.h, _p(d), _p(k_of), _p(out), _p(n_out), _p(lg) if want_logits else None)
        if T < 0:
            raise RuntimeError("batch_verify failed: " + last_error())
        toks = {s: [int(t) for t in out[s, :n_out[s]]] for s in range(ns) if n_out[s] > 0}
        return (toks, lg[:T]) if want_logits else toks

    def batch_generate_lookup(self, n_new, k=4, ngram_max=3):
        """n_new tokens for every active slot by prompt-lookup drafts and batch_verify passes
        (gemma_engine_batch_generate_lookup): (out [n_slots][n_new], per-slot list of dict(passes,
        drafted, accepted, plain_steps)); rows of inactive slots stay zero."""
        ns = self._bt_slots
        out = np.zeros((ns, max(int(n_new), 1)), dtype=np.int32)
        st = (SpecStats * ns)()
        r = self.L.gemma_engine_batch_generate_lookup(self.h, int(n_new), int(k), int(ngram_max), _p(out), st)
        self._chk(r, "batch_generate_lookup")
        return out[:, :n_new], [dict(passes=x.passes, drafted=x.drafted, accepted=x.accepted, plain_steps=x.plain_steps)
                                for x in st]

    def batch_set_sampler(self, slot, temperature=None, top_k=0, top_p=1.0, seed=0):
        """A sampler of the slot's own (gemma_engine_batch_set_sampler).  No parameters or temperature
        None: the slot follows the engine's sampler again.  temperature <= 0: the slot picks greedily
        whatever the engine's sampler is.  The setting stays with the slot until batch_close."""
        if temperature is None:
            r = self.L.gemma_engine_batch_set_sampler(self.h, int(slot), None)
        else:
            s = GemmaSampler(float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1))
            r = self.L.gemma_engine_batch_set_sampler(self.h, int(slot), C.byref(s))
        self._chk(r, "batch_set_sampler")

    def batch_sampler(self, slot):
        """(the slot's picks sample, {temperature, top_k, top_p, seed} in force, the setting is the
        slot's own)"""
        s = GemmaSampler()
        own = C.c_int(0)
        on = self.L.gemma_engine_batch_sampler(self.h, int(slot), C.byref(s), C.byref(own))
        if on < 0:
            raise RuntimeError("batch_sampler failed: " + last_error())
        return on == 1, dict(temperature=s.temperature, top_k=s.top_k, top_p=s.top_p, seed=s.seed), own.value == 1

    def batch_fork(self, src, dst):
        """Slot dst becomes a device-to-device copy of the active slot src's sequence (caches, history,
        position, pending and unprocessed given tokens); each slot keeps its own sampler setting."""
        self._chk(self.L.gemma_engine_batch_fork(self.h, int(src), int(dst)), "batch_fork")

    def batch_shift(self, slot, keep, discard):
        """shift() for an active slot (gemma_engine_batch_shift); returns the slot's new pos"""
        n = self.L.gemma_engine_batch_shift(self.h, int(slot), int(keep), int(discard))
        if n < 0:
            raise RuntimeError("batch_shift failed: " + last_error())
        return n

    def batch_close(self):
        self._chk(self.L.gemma_engine_batch_close(self.h), "batch_close")

    def batch_begin(self, slot, tokens):
        """begin() for a slot: caches cleared, `tokens` given, position 0, the slot active."""
        p = np.ascontiguousarray(tokens, dtype=np.int32)
        self._chk(self.L.gemma_engine_batch_begin(self.h, int(slot), _p(p), len(p)), "batch_begin")

    def batch_adopt(self, slot):
        """Copy the engine's own sequence (caches, history, position, pending token) into a slot."""
        self._chk(self.L.gemma_engine_batch_adopt(self.h, int(slot)), "batch_adopt")

    def batch_release(self, slot):
        self._chk(self.L.gemma_engine_batch_release(self.h, int(slot)), "batch_release")

    def batch_step(self, n, want_logits=False):
        """n passes, one row per active slot in ascending slot order; with want_logits the rows
        [n][R][n_vocab]."""
        lg = None
        if want_logits:
            R = sum(1 for t in self.batch_last_n() if t >= 0)
            lg = np.zeros((max(int(n), 0), R, self.cfg.n_vocab), dtype=np.float32)
        self._chk(self.L.gemma_engine_batch_step(self.h, int(n), _p(lg) if want_logits else None), "batch_step")
        return lg

    def batch_pos(self, slot):
        """processed positions of a slot; -1 for an inactive (or invalid) slot"""
        return self.L.gemma_engine_batch_pos(self.h, int(slot))

    def batch_tokens(self, slot):
        """the slot's sequence so far, the pending token included"""
        out = np.zeros(self.cfg.n_ctx + 1, dtype=np.int32)
        n = self.L.gemma_engine_batch_tokens(self.h, int(slot), _p(out), len(out))
        if n < 0:
            raise RuntimeError("batch_tokens failed: " + last_error())
        return out[:n]

    def batch_last(self):
        """the BATCH_MAX_SLOTS pending tokens in one transfer, -1 for inactive slots"""
        out = np.zeros(BATCH_MAX_SLOTS, dtype=np.int32)
        self._chk(self.L.gemma_engine_batch_last(self.h, _p(out)), "batch_last")
        return out

    def batch_last_n(self):
        """the pending tokens of the batch's slots [0, n_slots) in one transfer, -1 for inactive slots
        (any batch, up to BATCH_WIDE_MAX_SLOTS slots)"""
        out = np.zeros(BATCH_WIDE_MAX_SLOTS, dtype=np.int32)
        n = self.L.gemma_engine_batch_last_n(self.h, _p(out), len(out))
        if n < 0:
            raise RuntimeError("batch_last_n failed: " + last_error())
        return out[:n]

    def batch_kv_read(self, slot, layer, p0, n):
        """kv_read of a slot's caches: (k [n][kvw], v [n][kvw]) f16 bits"""
        kvw = self.cfg.n_head_kv * self.cfg.head_dim
        k = np.zeros((n, kvw), dtype=np.uint16)
        v = np.zeros((n, kvw), dtype=np.uint16)
        self._chk(self.L.gemma_engine_batch_kv_read(self.h, int(slot), int(layer), int(p0), int(n), _p(k), _p(v)),
                  "batch_kv_read")
        return k, v

    def sync(self):
        """wait for the engine's stream"""
        self._chk(self.L.gemma_engine_sync(self.h), "sync")

    def tokens(self):
        out = np.zeros(self.cfg.n_ctx + 1, dtype=np.int32)
        n = self.L.gemma_engine_tokens(self.h, _p(out), len(out))
        return out[:n]

    def prefill(self, n_prompt=None, want_all=False, exact=True):
        """Batched prefill of the prompt given to begin(); returns (token, last-row logits[, all rows]).
        exact=True: bit-identical to the CPU path; False: the MFMA tolerance path."""
        last = np.zeros(self.cfg.n_vocab, dtype=np.float32)
        allv = np.zeros((n_prompt, self.cfg.n_vocab), dtype=np.float32) if want_all else None
        fn = self.L.gemma_engine_prefill if exact else self.L.gemma_engine_prefill_fast
        tok = fn(self.h, _p(last), _p(allv) if want_all else None)
        if tok < 0:
            raise RuntimeError("prefill failed: " + last_error())
        return (tok, last, allv) if want_all else (tok, last)

    def tensor(self, tid, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        n = self.L.gemma_engine_tensor(self.h, tid, _p(out), nbytes)
        if n < 0:
            raise RuntimeError("tensor failed: " + last_error())
        return out[:n]

    def stamp_step(self, layer):
        """Diagnostics: one eager step; returns u64 stamps [6 regions][4096 workgroups][16 phases]."""
        out = np.zeros(6 * 4096 * 16, dtype=np.uint64)
        self._chk(self.L.gemma_engine_stamp_step(self.h, layer, _p(out)), "stamp_step")
        return out.reshape(6, 4096, 16)

    PLAN_CLASSES = ("qkv", "attn_out", "gate_up", "down", "logits")

    def tune(self, iters=8):
        """measure the launch plan (clobbers the decode state: begin() afterwards); returns it"""
        if self.L.gemma_engine_tune(self.h, iters) != 0:
            raise RuntimeError("tune failed: " + last_error())
        return self.plan()

    def plan(self):
        """{class: (k_split, rows_per_wg, image)} plus "attention": form (0 per head, 1 split)"""
        buf = (C.c_int * 16)()
        n = self.L.gemma_engine_plan(self.h, buf, 16)
        p = {k: (buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i, k in enumerate(self.PLAN_CLASSES[: n // 3])}
        if n > 15:
            p["attention"] = buf[15]
        return p

    def set_plan(self, plan):
        flat = []
        for k in self.PLAN_CLASSES:
            v = list(plan[k])
            flat += v + [0] * (3 - len(v))
        if "attention" in plan:
            flat.append(int(plan["attention"]))
        arr = (C.c_int * len(flat))(*flat)
        if self.L.gemma_engine_set_plan(self.h, arr, len(flat)) != 0:
            raise RuntimeError("set_plan failed: " + last_error())

    def set_fuse(self, front=-1):
        """fused layer front on (1) / off (0) / unchanged (-1); returns the sticky hand-off timeout
        word (0 = every in-launch hand-off completed in time)"""
        return self.L.gemma_engine_set_fuse(self.h, front)

    def set_option(self, name, value):
        """a selectable variant (include/gemma_hpc.h gemma_engine_set_option); drops the decode graph"""
        self._chk(self.L.gemma_engine_set_option(self.h, name.encode(), int(value)), f"set_option({name})")

    def set_sampler(self, temperature=0.0, top_k=0, top_p=1.0, seed=0):
        """Seeded temperature / top-k / top-p sampling inside the decode step (include/gemma_hpc.h
        has the rule).  temperature <= 0 or None: greedy, the default.  top_k 0 = 1024 candidates
        (the most the truncated rule takes), TOP_K_ALL = the whole-vocabulary sampler (temperature and
        top_p over every entry of the row).  A change of parameters keeps the captured graph; on / off drops it."""
        if temperature is None:
            r = self.L.gemma_engine_set_sampler(self.h, None)
        else:
            s = GemmaSampler(float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1))
            r = self.L.gemma_engine_set_sampler(self.h, C.byref(s))
        self._chk(r, "set_sampler")

    def sampler(self):
        """(sampling on, {temperature, top_k, top_p, seed} as last set)"""
        s = GemmaSampler()
        on = self.L.gemma_engine_sampler(self.h, C.byref(s))
        return on == 1, dict(temperature=s.temperature, top_k=s.top_k, top_p=s.top_p, seed=s.seed)

    def set_penalties(self, repeat=1.0, presence=0.0, frequency=0.0, last_n=64):
        """Repetition, presence and frequency penalties over the last last_n tokens of the sequence, applied
        on the device ahead of every pick (include/gemma_hpc.h has the rule).  repeat None, or the defaults
        (1, 0, 0): off.  A change of values or of last_n keeps the captured graph; on / off drops it.
        Raises on a refused setting, a row-split engine or the persistent launch."""
        if repeat is None:
            r = self.L.gemma_engine_set_penalties(self.h, None)
        else:
            p = GemmaPenalties(float(repeat), float(presence), float(frequency), int(last_n))
            r = self.L.gemma_engine_set_penalties(self.h, C.byref(p))
        self._chk(r, "set_penalties")

    def penalties(self):
        """(penalties on, {repeat, presence, frequency, last_n} as last set)"""
        p = GemmaPenalties()
        on = self.L.gemma_engine_penalties(self.h, C.byref(p))
        return on == 1, dict(repeat=p.repeat, presence=p.presence, frequency=p.frequency, last_n=p.last_n)

    def set_logprobs(self, on=-1):
        """Per-token log-probabilities under the raw softmax of every logits row a pass computes
        (include/gemma_hpc.h has the rule): on 1 / off 0 / keep -1; returns the setting.  On / off drops
        the captured graph; raises on a row-split engine."""
        r = self.L.gemma_engine_set_logprobs(self.h, int(on))
        if r < 0:
            raise RuntimeError("set_logprobs failed: " + last_error())
        return r == 1

    def logprobs(self, p0=0, n=None):
        """lp[p0 .. p0+n) of the engine's sequence as f64 (n=None: through the sequence's end, the
        pending pick included); NaN where no scored row predicted the index."""
        if n is None:
            n = max(self.pos() + 1, getattr(self, "_n_seq", 0)) - int(p0)
        out = np.zeros(max(int(n), 0), dtype=np.float64)
        if self.L.gemma_engine_logprobs(self.h, int(p0), int(n), _p(out)) < 0:
            raise RuntimeError("logprobs failed: " + last_error())
        return out

    def batch_logprobs(self, slot, p0=0, n=None):
        """logprobs() of an active slot of the open batch"""
        if n is None:
            n = self.batch_pos(slot) + 1 - int(p0)
        out = np.zeros(max(int(n), 0), dtype=np.float64)
        if self.L.gemma_engine_batch_logprobs(self.h, int(slot), int(p0), int(n), _p(out)) < 0:
            raise RuntimeError("batch_logprobs failed: " + last_error())
        return out

    def set_top_logprobs(self, n=-1):
        """The n most likely tokens of every scored position with their log-probabilities
        (include/gemma_hpc.h has the rule): n in [0, TOP_LOGPROBS_MAX], 0 off, -1 keep; returns the
        setting.  A change drops the captured graph; raises while log-probabilities are off, on a
        row-split engine and while a batch is open."""
        r = self.L.gemma_engine_set_top_logprobs(self.h, int(n))
        if r < 0:
            raise RuntimeError("set_top_logprobs failed: " + last_error())
        return r

    def _top_logprobs(self, call, what, p0, cnt):
        n = self.set_top_logprobs()
        tok = np.zeros((max(int(cnt), 0), n), dtype=np.int32)
        lps = np.zeros(tok.shape, dtype=np.float64)
        if call(int(p0), int(cnt), _p(tok), _p(lps)) < 0:
            raise RuntimeError(what + " failed: " + last_error())
        return tok, lps

    def top_logprobs(self, p0=0, cnt=None):
        """the alternatives of sequence indices [p0, p0+cnt) of the engine's sequence (cnt=None: through
        its end): (tokens i32 [cnt][n], lps f64 [cnt][n]) in descending order; -1 / NaN where the row has
        fewer entries or no scored row predicted the index."""
        if cnt is None:
            cnt = max(self.pos() + 1, getattr(self, "_n_seq", 0)) - int(p0)
        return self._top_logprobs(lambda *a: self.L.gemma_engine_top_logprobs(self.h, *a), "top_logprobs", p0, cnt)

    def batch_top_logprobs(self, slot, p0=0, cnt=None):
        """top_logprobs() of an active slot of the open batch"""
        if cnt is None:
            cnt = self.batch_pos(slot) + 1 - int(p0)
        return self._top_logprobs(lambda *a: self.L.gemma_engine_batch_top_logprobs(self.h, int(slot), *a),
                                  "batch_top_logprobs", p0, cnt)

    def set_att_o(self, on=-1):
        """decode attention + attn-out in one launch per layer: on 1 / off 0 / keep -1; returns the setting"""
        return self.L.gemma_engine_set_att_o(self.h, on) == 1

    def set_persist(self, on=-1):
        """The decode step's layers as one persistent launch (token.hip): on 1/0, -1 keep; returns
        True when it runs this engine's steps."""
        return self.L.gemma_engine_set_persist(self.h, on) == 1

    def set_persist_timeout(self, ticks):
        """the persistent launch's per-wait bound in 100 MHz ticks (0 = default; tests force timeouts)"""
        return self.L.gemma_engine_set_persist_timeout(self.h, ticks)

    def p2p_handle(self):
        """this rank's inbox arena as IPC handle bytes (GEMMA_TP_P2P engines)"""
        buf = C.create_string_buffer(128)
        n = self.L.gemma_engine_p2p_handle(self.h, buf, 128)
        if n <= 0:
            raise RuntimeError("gemma_engine_p2p_handle: " + last_error())
        return buf.raw[:n]

    def p2p_open(self, handles):
        """every rank's handle (rank order); then a host barrier before the first step"""
        raw = b"".join(handles)
        if self.L.gemma_engine_p2p_open(self.h, C.create_string_buffer(raw, len(raw)), len(handles)) != 0:
            raise RuntimeError("gemma_engine_p2p_open: " + last_error())

    def p2p_err(self, reset=False):
        """the sticky flag-wait timeout word of the p2p gathers"""
        return self.L.gemma_engine_p2p_err(self.h, 1 if reset else 0)

    def tp_flags(self):
        """layout flags of a row-split engine (TP_REP_ATTN)"""
        return self.L.gemma_engine_tp_flags(self.h)

    def tp_info(self):
        """[ranks, rank, RCCL communicator present, shard slots in this engine]"""
        out = (C.c_int * 4)()
        self.L.gemma_engine_tp_info(self.h, out)
        return list(out)

    def persist_err(self, reset=False):
        """Sticky hand-off timeout words [flag, site, layer] of the persistent launch."""
        out = (C.c_int * 3)()
        self.L.gemma_engine_persist_err(self.h, out, 1 if reset else 0)
        return list(out)

    def graph_kernels(self):
        """kernel launches per decode token (the captured decode graph's kernel nodes)"""
        n = self.L.gemma_engine_graph_kernels(self.h)
        if n < 0:
            raise RuntimeError("graph_kernels failed: " + last_error())
        return n

    def time_kernel(self, which, iters):
        b = C.c_double()
        us = self.L.gemma_engine_time(self.h, which, iters, C.byref(b))
        if us < 0:
            raise RuntimeError("time failed: " + last_error())
        return us, b.value


def test_sample(rows, sampler, positions):
    """The sampler's kernels on host logits rows [R][V] (gemma_test_sample): row r is drawn at sequence
    index positions[r].  sampler: dict(temperature, top_k, top_p, seed).  Returns (tokens [R],
    cand [R][1024] candidate ids in order with -1 past K, n_cand [R] = K, n_kept [R] = m; with
    top_k = TOP_K_ALL: cand all -1, n_cand = V, n_kept = the nucleus size);
    raises RuntimeError with the library's message on a refused argument."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    R, V = x.shape
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    if pos.shape != (R,):
        raise ValueError("positions: one per row")
    s = GemmaSampler(float(sampler.get("temperature", 1.0)), int(sampler.get("top_k", 0)),
                     float(sampler.get("top_p", 1.0)), int(sampler.get("seed", 0)) & (2 ** 64 - 1))
    tokens = np.zeros(R, dtype=np.int32)
    cand = np.zeros((R, SAMPLE_MAX_K), dtype=np.int32)
    n_cand = np.zeros(R, dtype=np.int32)
    n_kept = np.zeros(R, dtype=np.int32)
    r = lib().gemma_test_sample(_p(x), R, V, C.byref(s), _p(pos), _p(tokens), _p(cand), _p(n_cand), _p(n_kept))
    if r != 0:
        raise RuntimeError("gemma_test_sample failed: " + last_error())
    return tokens, cand, n_cand, n_kept


test_sample.__test__ = False  # a library wrapper, not a pytest test


def test_sample_rows(rows, samplers, positions):
    """test_sample with one sampler per row (gemma_test_sample_rows), all rows through one set of
    launches.  samplers[r]: dict(temperature, top_k, top_p, seed), a (temperature, top_k, top_p, seed)
    tuple, or None for a greedy row (then n_cand = n_kept = 0 and cand[r] is all -1)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    R, V = x.shape
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    if pos.shape != (R,) or len(samplers) != R:
        raise ValueError("positions and samplers: one per row")
    s_of = (GemmaSampler * R)()
    for r, sp in enumerate(samplers):
        if sp is None:
            sp = (0.0, 0, 1.0, 0)
        if isinstance(sp, dict):
            sp = (sp.get("temperature", 1.0), sp.get("top_k", 0), sp.get("top_p", 1.0), sp.get("seed", 0))
        s_of[r] = GemmaSampler(float(sp[0]), int(sp[1]), float(sp[2]), int(sp[3]) & (2 ** 64 - 1))
    tokens = np.zeros(R, dtype=np.int32)
    cand = np.zeros((R, SAMPLE_MAX_K), dtype=np.int32)
    n_cand = np.zeros(R, dtype=np.int32)
    n_kept = np.zeros(R, dtype=np.int32)
    r = lib().gemma_test_sample_rows(_p(x), R, V, s_of, _p(pos), _p(tokens), _p(cand), _p(n_cand), _p(n_kept))
    if r != 0:
        raise RuntimeError("gemma_test_sample_rows failed: " + last_error())
    return tokens, cand, n_cand, n_kept


test_sample_rows.__test__ = False


def _penalties(p):
    """dict(repeat, presence, frequency, last_n) or a tuple in that order -> GemmaPenalties"""
    if isinstance(p, dict):
        p = (p.get("repeat", 1.0), p.get("presence", 0.0), p.get("frequency", 0.0), p.get("last_n", 64))
    return GemmaPenalties(float(p[0]), float(p[1]), float(p[2]), int(p[3]))


def test_kv_shift(kc, vc, pos, keep, discard, Hkv, hd, rope_base=10000.0):
    """The context shift's cache kernels on one layer's images, in place (gemma_test_kv_shift): kc
    [ctx][Hkv*hd], vc [Hkv*hd][ctx], C-contiguous uint16 (f16 bits).  A refusal raises and leaves both as given."""
    for a in (kc, vc):
        if a.dtype != np.uint16 or not a.flags.c_contiguous:
            raise ValueError("test_kv_shift: C-contiguous uint16 images")
    if lib().gemma_test_kv_shift(_p(kc), _p(vc), kc.shape[0], int(Hkv), int(hd), int(pos), int(keep), int(discard), float(rope_base)) != 0:
        raise RuntimeError("gemma_test_kv_shift failed: " + last_error())


def test_penalize(rows, hist, positions, penalties, out=None):
    """The two penalty kernels on host logits rows [R][V] (gemma_test_penalize): row r processed sequence
    index positions[r] of its own history hist[r] ([R][H] int32, H > every position).  penalties:
    dict(repeat, presence, frequency, last_n), such a tuple, or None for a setting that is off.  Returns
    (penalised [R][V], restored [R][V], n_saved [R]), written into `out` when that triple is given;
    raises RuntimeError with the library's message on a refused argument (the outputs are then untouched)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    h = np.ascontiguousarray(hist, dtype=np.int32)
    R, V = x.shape
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    if pos.shape != (R,) or h.ndim != 2 or h.shape[0] != R:
        raise ValueError("positions and hist: one per row")
    pen, res, n_saved = out if out is not None else (np.zeros_like(x), np.zeros_like(x), np.zeros(R, dtype=np.int32))
    p = None if penalties is None else C.byref(_penalties(penalties))
    r = lib().gemma_test_penalize(_p(x), R, V, _p(h), h.shape[1], _p(pos), p, _p(pen), _p(res), _p(n_saved))
    if r != 0:
        raise RuntimeError("gemma_test_penalize failed: " + last_error())
    return pen, res, n_saved


test_penalize.__test__ = False


def test_logprob(rows, tokens):
    """logprob(rows[r], tokens[r]) for host logits rows [R][V] through the engine's two kernels
    (gemma_test_logprob); returns f64 [R]; raises RuntimeError with the library's message on a
    refused argument."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    R, V = x.shape
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    if t.shape != (R,):
        raise ValueError("tokens: one per row")
    out = np.zeros(R, dtype=np.float64)
    if lib().gemma_test_logprob(_p(x), R, V, _p(t), _p(out)) != 0:
        raise RuntimeError("gemma_test_logprob failed: " + last_error())
    return out


test_logprob.__test__ = False  # a library wrapper, not a pytest test


TOP_LOGPROBS_MAX = 32  # GEMMA_TOP_LOGPROBS_MAX


def test_top_logprobs(rows, n):
    """The n most likely tokens of host logits rows [R][V] with their log-probabilities through the
    engine's kernels (gemma_test_top_logprobs); returns (tokens i32 [R][n], lps f64 [R][n]); raises
    RuntimeError with the library's message on a refused argument."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    R, V = x.shape
    tok = np.zeros((R, max(int(n), 0)), dtype=np.int32)
    lps = np.zeros(tok.shape, dtype=np.float64)
    if lib().gemma_test_top_logprobs(_p(x), R, V, int(n), _p(tok), _p(lps)) != 0:
        raise RuntimeError("gemma_test_top_logprobs failed: " + last_error())
    return tok, lps


test_top_logprobs.__test__ = False  # a library wrapper, not a pytest test


def batch_plan_rows(need, max_rows):
    """The row allotment of batch_step_rows (gemma_batch_plan_rows, a host function: no GPU): need[s]
    is 0 for an inactive slot, else max(1, given - pos).  Returns rows_of [len(need)]."""
    a = np.ascontiguousarray(need, dtype=np.int32)
    out = np.zeros(max(len(a), 1), dtype=np.int32)
    if lib().gemma_batch_plan_rows(_p(a), len(a), int(max_rows), _p(out)) < 0:
        raise ValueError("gemma_batch_plan_rows: " + last_error())
    return out[:len(a)]


def lookup_draft(seq, ngram_max, k):
    """Prompt-lookup draft for `seq` (gemma_lookup_draft, a host function: no GPU): the tokens that
    followed the most recent earlier occurrence of the longest matching suffix n-gram, at most k."""
    a = np.ascontiguousarray([int(x) for x in seq], dtype=np.int32)
    out = np.zeros(VERIFY_MAX_DRAFT, dtype=np.int32)
    n = lib().gemma_lookup_draft(_p(a), len(a), int(ngram_max), int(k), _p(out))
    if n < 0:
        raise ValueError("gemma_lookup_draft: " + last_error())
    return [int(t) for t in out[:n]]


def gemm_skinny(wtype, W, rows, X, resid=None):
    """The skinny exact GEMM on host buffers (gemma_test_gemm_skinny): W ggml row-major blocks,
    X [T][K] f32, resid [T][rows] or None; returns Y [T][rows]."""
    x = np.ascontiguousarray(X, dtype=np.float32)
    T, K = x.shape
    y = np.zeros((T, rows), dtype=np.float32)
    r = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
    w = np.ascontiguousarray(W)
    rc = lib().gemma_test_gemm_skinny(int(wtype), rows, K, T, _p(w), _p(x), None if r is None else _p(r), _p(y))
    if rc != 0:
        raise RuntimeError("gemma_test_gemm_skinny failed: " + last_error())
    return y


def gemm_skinny_kq(wtype, W, rows, X, resid=None, tiled=0):
    """The skinny exact K-quant GEMM on host buffers (gemma_test_gemm_skinny_kq): W raw ggml Q4_K /
    Q6_K rows, X [T][K] f32, resid [T][rows] or None, tiled 1 = the lane-contiguous layout; returns
    Y [T][rows]."""
    x = np.ascontiguousarray(X, dtype=np.float32)
    T, K = x.shape
    y = np.zeros((T, rows), dtype=np.float32)
    r = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
    w = np.ascontiguousarray(W)
    rc = lib().gemma_test_gemm_skinny_kq(int(wtype), rows, K, T, int(tiled), _p(w), _p(x), _p(y), None if r is None else _p(r))
    if rc != 0:
        raise RuntimeError("gemma_test_gemm_skinny_kq failed: " + last_error())
    return y


def tp_unique_id():
    """RCCL unique id for gemma_engine_create_tp (call on rank 0, broadcast the bytes)."""
    buf = C.create_string_buffer(256)
    n = lib().gemma_tp_unique_id(buf, 256)
    if n <= 0:
        raise RuntimeError("gemma_tp_unique_id failed: " + last_error())
    return buf.raw[:n]


_GGUF_SCALAR = {0: C.c_uint8, 1: C.c_int8, 2: C.c_uint16, 3: C.c_int16, 4: C.c_uint32, 5: C.c_int32, 6: C.c_float,
                7: C.c_bool, 10: C.c_uint64, 11: C.c_int64, 12: C.c_double}


class GGUF:
    """A GGUF file read by the library's gguf_init_from_file (include/ggml.h): `kv` maps keys to
    values (scalars, str, lists), `tensors` maps names to (ggml type, ne, bytes) when load_tensors."""

    def __init__(self, path, load_tensors=True):
        L = lib()
        ctx = C.c_void_p()
        self.g = L.gguf_init_from_file(path.encode(), GGUFInitParams(not load_tensors, C.pointer(ctx)))
        if not self.g:
            raise ValueError(last_error())
        self.version = L.gguf_get_version(self.g)
        self.alignment = L.gguf_get_alignment(self.g)
        self.data_offset = L.gguf_get_data_offset(self.g)
        self.kv = {}
        for i in range(L.gguf_get_n_kv(self.g)):
            key = L.gguf_get_key(self.g, i).decode()
            t = L.gguf_get_kv_type(self.g, i)
            if t == 8:
                v = L.gguf_get_val_str(self.g, i).decode()
            elif t == 9:
                at, n = L.gguf_get_arr_type(self.g, i), L.gguf_get_arr_n(self.g, i)
                if at == 8:
                    v = [L.gguf_get_arr_str(self.g, i, j).decode() for j in range(n)]
                else:
                    ct = _GGUF_SCALAR[at]
                    v = list((ct * n).from_address(L.gguf_get_arr_data(self.g, i))) if n else []
            else:
                v = _GGUF_SCALAR[t].from_address(L.gguf_get_val_data(self.g, i)).value
            self.kv[key] = v
        self.tensors = {}
        for i in range(L.gguf_get_n_tensors(self.g)):
            name = L.gguf_get_tensor_name(self.g, i)
            t = L.ggml_get_tensor(ctx, name)
            data = None
            if load_tensors:
                data = C.string_at(t.contents.data, L.ggml_nbytes(t))
            self.tensors[name.decode()] = (L.gguf_get_tensor_type(self.g, i), tuple(t.contents.ne), data,
                                           L.gguf_get_tensor_offset(self.g, i))
        L.ggml_free(ctx)
        L.gguf_free(self.g)
        self.g = None
