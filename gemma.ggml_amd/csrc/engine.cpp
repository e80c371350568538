// engine.cpp — device-resident Gemma forward for MI355X (the performance path).
//
// Keeps the whole token on the GPU: weights tiled in HBM, the activation never leaves the device,
// the greedy token is fed back on the device, and one decode step (18 layers x 5 kernels + the
// logits/argmax kernel + the advance kernel) is captured once in a hipGraph and replayed.
// This file is the engine's lifecycle: create (synthetic, GGUF, external weights, row-split), free,
// begin, step, the tensor read-back and the TP / p2p set-up.  The decode step itself is
// engine_decode.cpp, the prefill engine_prefill.cpp, timing / tuning / taps engine_diag.cpp; the
// engine struct and what the units share is engine_impl.h.
#include <chrono>

#include "../../include/ggml.h"
#include "engine_impl.h"

namespace ghip {

// ---- error state ------------------------------------------------------------------------------
static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
const std::string &last_error() { return g_err; }

// ---- host-side constant tables (product code; independent of oracle/) -------------------------
static inline uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float bitsf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

uint16_t host_f32_to_f16(float f) {  // IEEE RNE, subnormals, inf/nan
    const uint32_t x = fbits(f);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000);
    const uint32_t ax = x & 0x7fffffffu;
    if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00 | (ax > 0x7f800000u ? 0x200 | ((ax >> 13) & 0x3ff) : 0));
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00);
    if (ax < 0x38800000u) {
        if (ax < 0x33000000u) return sign;
        const uint32_t e = ax >> 23, m = (ax & 0x7fffff) | 0x800000, shift = 126 - e;
        uint32_t q = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (q & 1))) q++;
        return (uint16_t)(sign | q);
    }
    uint32_t r = (ax >> 13) - (112u << 10);
    const uint32_t rem = ax & 0x1fff;
    if (rem > 0x1000 || (rem == 0x1000 && (r & 1))) r++;
    return (uint16_t)(sign | r);
}

float host_f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000) << 16, exp = (h >> 10) & 0x1f, mant = h & 0x3ff;
    if (exp == 0) {
        const float v = (float)mant * 5.9604644775390625e-08f;
        return mant == 0 ? bitsf(sign) : (sign ? -v : v);
    }
    if (exp == 31) return bitsf(sign | 0x7f800000u | (mant << 13));
    return bitsf(sign | ((exp + 112) << 23) | (mant << 13));
}

// ggml_init tables: exp and gelu over every fp16 pattern
void build_f16_tables(std::vector<uint16_t> &exp_t, std::vector<uint16_t> &gelu_t) {
    exp_t.resize(65536);
    gelu_t.resize(65536);
    for (int i = 0; i < 65536; ++i) {
        const float f = host_f16_to_f32((uint16_t)i);
        exp_t[i] = host_f32_to_f16(expf(f));
        const float inner = 1.0f + 0.044715f * f * f;
        const float t = tanhf(0.79788456080286535587989211986876f * f * inner);
        gelu_t[i] = host_f32_to_f16(0.5f * f * (1.0f + t));
    }
}

// rope NEOX cos/sin: theta = (float)p, theta *= powf(base, -2/n_dims) per pair
void build_rope(int ctx, int hd, float base, std::vector<float> &c, std::vector<float> &s) {
    const int half = hd / 2;
    c.resize((size_t)ctx * half);
    s.resize((size_t)ctx * half);
    const float theta_scale = powf(base, -2.0f / hd);
    for (int p = 0; p < ctx; ++p) {
        float theta = (float)p;
        for (int i = 0; i < half; ++i) {
            c[(size_t)p * half + i] = cosf(theta) * 1.0f;
            s[(size_t)p * half + i] = sinf(theta) * 1.0f;
            theta *= theta_scale;
        }
    }
}

// ---- synthetic weight keys (DESIGN.md §Synthetic weights; mirrors oracle/gemma_cpu.cpp) -------
static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline uint64_t tensor_key(uint64_t seed, int tid) { return splitmix64(seed ^ ((uint64_t)tid << 40)); }
static inline float synth_scale(double stdv) { return (float)(stdv * 1.7320508075688772 / 65536.0); }
enum { TID_EMBD = 0, TID_OUT_NORM = 1 };
static inline int tid_layer(int il, int k) { return 16 + il * 16 + k; }
enum { L_ATTN_NORM = 0, L_Q = 1, L_K = 2, L_V = 3, L_O = 4, L_FFN_NORM = 5, L_GATE = 6, L_UP = 7, L_DOWN = 8 };

int alloc_tiled(dev_pool &mem, tiled_mat *out, int type, int64_t rows, int64_t K, hipStream_t s) {
    tiled_mat m;
    m.type = type;
    m.rows = rows;
    m.K = K;
    m.nb = K / 32;
    m.n_rt = (rows + 7) / 8;
    const int bt = type == T_Q4_0 ? 8 : 4;
    m.n_bt = (m.nb + bt - 1) / bt;
    // zeroed on the SAME stream as the generator / repack that fills it
    if (mem.get_zeroed(&m.qs, m.qs_bytes(), s) || mem.get_zeroed(&m.sc, m.sc_bytes(), s)) {
        mem.put(m.qs);
        return -1;
    }
    *out = m;
    return 0;
}
void free_tiled(dev_pool &mem, tiled_mat &m) {
    mem.put(m.qs);
    mem.put(m.sc);
}

}  // namespace ghip

// ggml K-quant rows -> the lane-contiguous layout, in place (through a scratch copy).  Q6_K needs
// K % 2048 == 0 (else the rows stay as they are).
static int kq_retile_inplace(uint8_t *w, int type, int64_t rows, int64_t K, hipStream_t s, bool *tiled) {
    *tiled = false;
    if (type == T_Q6_K && K % 2048) return 0;
    const size_t bytes = (size_t)(K / 256 * (type == T_Q4_K ? 144 : 210) * rows);
    dev_pool tmp_mem;
    uint8_t *tmp = nullptr;
    if (tmp_mem.get(&tmp, bytes)) return -1;
    if (launch_kq_retile(type, w, tmp, rows, K, true, s)) return -1;
    GHIP_CHECK(hipMemcpyAsync(w, tmp, bytes, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipStreamSynchronize(s));
    *tiled = true;
    return 0;
}

// rows [r0, r0 + dst.rows) of a host row-major Q4_0 / Q8_0 matrix into the tiled layout; from the
// C-ABI weight cache's tiled copy (device to device) when the host weight was registered
// (hpc_register_weight at model load), else uploaded and re-tiled
static int upload_rows(const tiled_mat &dst, const void *host, int64_t r0, hipStream_t s) {
    tiled_mat reg;
    if (r0 % 8 == 0 && dst.rows % 8 == 0 && registered_tiled(host, dst.type, dst.K, &reg) && reg.n_bt == dst.n_bt &&
        r0 + dst.rows <= reg.n_rt * 8) {
        const tiled_mat src = sub_rows(reg, r0, dst.rows);
        GHIP_CHECK(hipMemcpyAsync(dst.qs, src.qs, dst.qs_bytes(), hipMemcpyDeviceToDevice, s));
        GHIP_CHECK(hipMemcpyAsync(dst.sc, src.sc, dst.sc_bytes(), hipMemcpyDeviceToDevice, s));
        return 0;  // stream-ordered; engine_create synchronises before the first use
    }
    const int64_t rb = dst.nb * (dst.type == T_Q4_0 ? 18 : 34);
    dev_pool tmp_mem;
    uint8_t *tmp = nullptr;
    if (tmp_mem.get(&tmp, (size_t)(rb * dst.rows))) return -1;
    GHIP_CHECK(hipMemcpyAsync(tmp, (const uint8_t *)host + r0 * rb, (size_t)(rb * dst.rows), hipMemcpyHostToDevice, s));
    const int rc = launch_repack(dst, tmp, rb, s);
    GHIP_CHECK(hipStreamSynchronize(s));
    return rc;
}

// ---- engine_create, phase by phase ----------------------------------------------------------------
static bool config_ok(const gemma_hip_config &c, int tp_n, const void *nccl_id) {
    const bool kq_layers = c.wtype == T_Q4_K;  // K-quant layers (Q4_K / Q6_K per matrix) + Q6_K output
    if (c.head_dim % 32 || c.n_embd % 32 || c.n_ff % 32 || c.n_ctx % 32 || c.n_head % c.n_head_kv ||
        (c.wtype != T_Q4_0 && c.wtype != T_Q8_0 && !kq_layers) ||
        (c.out_type != 0 && c.out_type != c.wtype && c.out_type != T_Q6_K)) {
        set_error("gemma_engine_create: unsupported config");
        return false;
    }
    if (kq_layers && (c.n_embd % 256 || c.n_ff % 256 || (c.n_head * c.head_dim) % 256 || c.n_embd > 4096 || tp_n > 1 ||
                      nccl_id)) {
        set_error("gemma_engine_create: K-quant layers need n_embd, n_ff, n_head*head_dim % 256 == 0, n_embd <= 4096, one rank");
        return false;
    }
    if ((c.out_type == T_Q6_K || kq_layers) && (c.n_embd % 256 || c.n_embd > 4096 || tp_n > 1 || nccl_id)) {
        set_error("gemma_engine_create: a Q6_K output needs n_embd % 256 == 0, n_embd <= 4096 and one rank");
        return false;
    }
    return true;
}

// the row split: every split matrix is cut into tp_n contiguous row ranges of whole 8-row tiles
static bool set_shards(gemma_engine *e, int tp_n, int tp_rank, const void *nccl_id, int tp_flags) {
    const gemma_hip_config &c = e->cfg;
    e->qw = c.n_head * c.head_dim;
    e->kvw = c.n_head_kv * c.head_dim;
    e->qkv_rows = e->qw + 2 * e->kvw;
    e->tp_n = tp_n;
    e->tp_rank = tp_rank;
    e->rep_attn = tp_n > 1 && (tp_flags & GEMMA_TP_REP_ATTN);
    e->p2p = tp_n > 1 && !nccl_id && (tp_flags & GEMMA_TP_P2P);
    if (tp_n < 1 || tp_rank < 0 || tp_rank >= tp_n || (!e->rep_attn && e->qkv_rows % (8 * tp_n)) ||
        c.n_embd % (8 * tp_n) || c.n_ff % (8 * tp_n) || c.n_vocab % (8 * tp_n) ||
        (tp_flags & ~(GEMMA_TP_REP_ATTN | GEMMA_TP_P2P)) || (e->p2p && tp_n > P2P_MAX_RANKS)) {
        set_error("gemma_engine_create: row split needs every matrix's rows to divide into 8-row tiles per rank");
        return false;
    }
    e->sh_qkv = e->rep_attn ? e->qkv_rows : e->qkv_rows / tp_n;
    e->sh_e = c.n_embd / tp_n;
    e->sh_o = e->rep_attn ? c.n_embd : e->sh_e;
    e->sh_ff = c.n_ff / tp_n;
    e->sh_v = c.n_vocab / tp_n;
    e->n_virtual = (tp_n > 1 && !nccl_id && !e->p2p) ? tp_n : 1;
    return true;
}

// token_embd / tied output and the output norm: uploaded, or the synthetic generator straight into
// the device layout (matches oracle/gemma_cpu.cpp); -1 when an allocation or upload failed
static int create_embeddings(gemma_engine *e, const host_weights *hw) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    const double emb_std = (c.out_gain > 0.0f ? (double)c.out_gain : 1.0) / sqrt((double)c.n_embd);
    if (e->out_type == T_Q6_K) {  // oracle make_kmat(TID_EMBD, Q6_K, out_gain/sqrt(E)) on the device
        e->embd_row_bytes = (int64_t)c.n_embd / 256 * 210;
        if (e->mem.get(&e->embd_q6k, (size_t)(e->embd_row_bytes * c.n_vocab)) ||
            e->mem.get(&e->xq8k, (size_t)c.n_embd / 256 * 292))
            return -1;
        if (!hw)
            launch_synth_kquant(T_Q6_K, e->embd_q6k, c.n_vocab, c.n_embd, tensor_key(c.seed, TID_EMBD),
                                (float)(emb_std / 0.68), s);
    } else {
        if (alloc_tiled(e->mem, &e->embd, c.wtype, c.n_vocab, c.n_embd, s)) return -1;
        if (!hw) launch_synth_tiled(e->embd, tensor_key(c.seed, TID_EMBD), synth_scale(emb_std), 0, s);
    }
    if (e->mem.get(&e->out_norm, (size_t)c.n_embd * 4)) return -1;
    if (hw) {
        if (e->out_type == T_Q6_K)
            GHIP_CHECK(hipMemcpy(e->embd_q6k, hw->embd, (size_t)(e->embd_row_bytes * c.n_vocab), hipMemcpyHostToDevice));
        else if (upload_rows(e->embd, hw->embd, 0, s))
            return -1;
        GHIP_CHECK(hipMemcpy(e->out_norm, hw->out_norm, (size_t)c.n_embd * 4, hipMemcpyHostToDevice));
    } else {
        launch_synth_norm(e->out_norm, c.n_embd, tensor_key(c.seed, TID_OUT_NORM), synth_scale(0.05), s);
    }
    if (e->out_type == T_Q6_K) return kq_retile_inplace(e->embd_q6k, T_Q6_K, c.n_vocab, c.n_embd, s, &e->embd_tiled);
    return 0;
}

// a layer's norms: replicated, the slot-0 copy serves every virtual rank
static int create_layer_norms(gemma_engine *e, int il, int vr, const host_weights *hw) {
    const gemma_hip_config &c = e->cfg;
    layer_dev &L = layer_of(e, il, vr);
    if (vr > 0) {
        L.attn_norm = layer_of(e, il, 0).attn_norm;
        L.ffn_norm = layer_of(e, il, 0).ffn_norm;
        return 0;
    }
    if (e->mem.get(&L.attn_norm, (size_t)c.n_embd * 4) || e->mem.get(&L.ffn_norm, (size_t)c.n_embd * 4)) return -1;
    if (hw) {
        GHIP_CHECK(hipMemcpy(L.attn_norm, hw->layers[il].attn_norm, (size_t)c.n_embd * 4, hipMemcpyHostToDevice));
        GHIP_CHECK(hipMemcpy(L.ffn_norm, hw->layers[il].ffn_norm, (size_t)c.n_embd * 4, hipMemcpyHostToDevice));
    } else {
        launch_synth_norm(L.attn_norm, c.n_embd, tensor_key(c.seed, tid_layer(il, L_ATTN_NORM)), synth_scale(0.05), e->stream);
        launch_synth_norm(L.ffn_norm, c.n_embd, tensor_key(c.seed, tid_layer(il, L_FFN_NORM)), synth_scale(0.05), e->stream);
    }
    return 0;
}

// layer il's K-quant matrices, raw rows: uploaded, or the oracle's make_kmat on the device; returns
// true when an allocation or upload failed
static bool create_layer_kq(gemma_engine *e, int il, const host_weights *hw) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    bool fail = false;
    if (e->kql.empty()) e->kql.resize(c.n_layer);
    kq_layer &K = e->kql[il];
    const host_weights::layer *H = hw ? &hw->layers[il] : nullptr;
    // q and k of one type share one allocation (k's rows right after q's): one launch for q|k
    const int tq = H ? H->tq : T_Q4_K, tk = H ? H->tk : T_Q4_K;
    uint8_t *qk_buf = nullptr;
    if (tq == tk) {
        const int64_t rb = c.n_embd / 256 * (tq == T_Q4_K ? 144 : 210);
        if (e->mem.get(&qk_buf, (size_t)(rb * (e->qw + e->kvw)))) return true;
    }
    auto make = [&](kq_mat &m, int type, int64_t rows, int64_t k, int tid, double stdv, const void *host) {
        m.type = type;
        m.rows = rows;
        m.K = k;
        m.rb = k / 256 * (type == T_Q4_K ? 144 : 210);
        if (fail) return;
        if (qk_buf && (&m == &K.q || &m == &K.k)) {
            m.w = qk_buf + (&m == &K.k ? m.rb * e->qw : 0);
        } else if (e->mem.get(&m.w, (size_t)(m.rb * rows))) {
            fail = true;
            return;
        }
        if (host) {
            fail |= hipMemcpy(m.w, host, (size_t)(m.rb * rows), hipMemcpyHostToDevice) != hipSuccess;
        } else {
            launch_synth_kquant(type, m.w, rows, k, tensor_key(c.seed, tid_layer(il, tid)),
                                (float)(stdv / (type == T_Q4_K ? 0.8 : 0.68)), s);
        }
        if (!fail && kq_retile_inplace(m.w, type, rows, k, s, &m.tiled)) fail = true;
    };
    const double se = 1.0 / sqrt((double)c.n_embd), sq = 1.0 / sqrt((double)e->qw), sf = 1.0 / sqrt((double)c.n_ff);
    make(K.q, H ? H->tq : T_Q4_K, e->qw, c.n_embd, L_Q, se, H ? H->q : nullptr);
    make(K.k, H ? H->tk : T_Q4_K, e->kvw, c.n_embd, L_K, se, H ? H->k : nullptr);
    K.qk_fused = qk_buf != nullptr;
    make(K.v, H ? H->tv : T_Q6_K, e->kvw, c.n_embd, L_V, se, H ? H->v : nullptr);
    make(K.o, H ? H->to : T_Q4_K, c.n_embd, e->qw, L_O, 4.0 * sq, H ? H->o : nullptr);
    make(K.gate, H ? H->tg : T_Q4_K, c.n_ff, c.n_embd, L_GATE, se, H ? H->gate : nullptr);
    make(K.up, H ? H->tu : T_Q4_K, c.n_ff, c.n_embd, L_UP, se, H ? H->up : nullptr);
    make(K.down, H ? H->td : T_Q6_K, c.n_embd, c.n_ff, L_DOWN, 4.0 * sf, H ? H->down : nullptr);
    return fail;
}

// layer il's tiled matrices for (virtual) rank slot vr: this rank's rows of each, uploaded or from
// the synthetic generator straight into the tiled layout; returns true when an allocation or upload failed
static bool create_layer_tiled(gemma_engine *e, int il, int vr, const host_weights *hw) {
    const gemma_hip_config &c = e->cfg;
    const int wt = c.wtype;
    hipStream_t s = e->stream;
    bool fail = false;
    layer_dev &L = layer_of(e, il, vr);
    const int tp_rank = rank_of(e, vr);
    const host_weights::layer *H = hw ? &hw->layers[il] : nullptr;
    const double se = 1.0 / sqrt((double)c.n_embd), sq = 1.0 / sqrt((double)e->qw), sf = 1.0 / sqrt((double)c.n_ff);
    // replicated attention block: one whole copy in slot 0 (virtual slots > 0 hold none)
    const bool att_here = !e->rep_attn || vr == 0;
    // this rank's rows [r0, r0 + n) of the fused [Wq | Wk | Wv]: the pieces of each source tensor
    const int64_t q0 = e->rep_attn ? 0 : (int64_t)tp_rank * e->sh_qkv, qn = att_here ? e->sh_qkv : 0;
    if (att_here && alloc_tiled(e->mem, &L.qkv, wt, qn, c.n_embd, s)) return true;
    const int64_t src_start[3] = {0, e->qw, e->qw + e->kvw}, src_rows[3] = {e->qw, e->kvw, e->kvw};
    const int src_tid[3] = {L_Q, L_K, L_V};
    const void *src_host[3] = {H ? H->q : nullptr, H ? H->k : nullptr, H ? H->v : nullptr};
    for (int k = 0; k < 3; ++k) {
        const int64_t a0 = std::max(q0, src_start[k]), a1 = std::min(q0 + qn, src_start[k] + src_rows[k]);
        if (a1 > a0 && hw) {
            fail |= upload_rows(sub_rows(L.qkv, a0 - q0, a1 - a0), src_host[k], a0 - src_start[k], s) != 0;
        } else if (a1 > a0) {
            launch_synth_tiled(sub_rows(L.qkv, a0 - q0, a1 - a0), tensor_key(c.seed, tid_layer(il, src_tid[k])),
                               synth_scale(se), a0 - src_start[k], s);
        }
    }
    // rows [r0, r0 + rows) of one source tensor as its own matrix
    auto make = [&](tiled_mat &m, int64_t rows, int64_t K, const void *host, int tid, double stdv, int64_t r0) {
        if (fail || alloc_tiled(e->mem, &m, wt, rows, K, s)) {
            fail = true;
            return;
        }
        if (hw) fail |= upload_rows(m, host, r0, s) != 0;
        else launch_synth_tiled(m, tensor_key(c.seed, tid_layer(il, tid)), synth_scale(stdv), r0, s);
    };
    if (att_here) make(L.o, e->sh_o, e->qw, H ? H->o : nullptr, L_O, 4.0 * sq, e->rep_attn ? 0 : (int64_t)tp_rank * e->sh_o);
    make(L.gate, e->sh_ff, c.n_embd, H ? H->gate : nullptr, L_GATE, se, (int64_t)tp_rank * e->sh_ff);
    make(L.up, e->sh_ff, c.n_embd, H ? H->up : nullptr, L_UP, se, (int64_t)tp_rank * e->sh_ff);
    make(L.down, e->sh_e, c.n_ff, H ? H->down : nullptr, L_DOWN, 4.0 * sf, (int64_t)tp_rank * e->sh_e);
    return fail;
}

// caches, tables, activations, hand-off counters and the decode state; -1 (last_error set) when
// the attention geometry is unsupported
static int create_buffers(gemma_engine *e, const std::vector<uint16_t *> *kc_ext, const std::vector<uint16_t *> *vc_ext) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    dev_pool &M = e->mem;
    if (kc_ext && vc_ext) {
        e->kc_ext = *kc_ext;
        e->vc_ext = *vc_ext;
    }
    // the own sequence: made once, here (the captured decode graph holds its addresses)
    if (seq_alloc(e, M, e->seq, e->kc_ext.empty(), nullptr)) return -1;
    std::vector<uint16_t> et, gt;
    build_f16_tables(et, gt);
    std::vector<float> rc, rs;
    build_rope(c.n_ctx, c.head_dim, c.rope_base, rc, rs);
    // attention form: one workgroup per head up to 2048 positions, the position-split form beyond
    e->att_mode = (c.head_dim <= 256 && c.n_ctx <= 2048) ? ATTN_PER_HEAD : ATTN_SPLIT;
    e->ag = attn_geometry(c.n_head, c.n_head_kv, c.head_dim, c.n_ctx);
    if (e->att_mode == ATTN_SPLIT && !e->ag.nwg) {
        set_error("gemma_engine_create: unsupported attention geometry");
        return -1;
    }
    if (M.get(&e->att_sbuf, std::max<size_t>(e->ag.sbuf_floats, 1) * 4)) return -1;
    if (M.get(&e->att_sync, (e->ag.sync_ints + 1) * 4)) return -1;
    GHIP_CHECK(hipMemsetAsync(e->att_sync, 0, (e->ag.sync_ints + 1) * 4, s));
    if (M.get(&e->exp_tab, 65536 * 2)) return -1;
    if (M.get(&e->gelu_tab, 65536 * 2)) return -1;
    if (M.get(&e->rope_cos, rc.size() * 4)) return -1;
    if (M.get(&e->rope_sin, rs.size() * 4)) return -1;
    GHIP_CHECK(hipMemcpy(e->exp_tab, et.data(), 65536 * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(e->gelu_tab, gt.data(), 65536 * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(e->rope_cos, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(e->rope_sin, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    if (M.get(&e->x, (size_t)c.n_embd * 4)) return -1;
    if (M.get(&e->qkv, (size_t)e->qkv_rows * 4)) return -1;
    if (M.get(&e->attn, (size_t)e->qw * 4)) return -1;
    if (M.get(&e->sa, (size_t)c.n_embd * 4)) return -1;
    if (M.get(&e->h, (size_t)c.n_ff * 4)) return -1;
    // launch_attn_decode needs head_dim % (32 * dsplit) == 0: the largest of 4 / 2 / 1 that divides
    // (head_dim 32 / 64 / 96 / 160 / ... take fewer workgroups per head, never a failing step)
    if (e->att_dsplit < 1) e->att_dsplit = 1;
    while (e->att_dsplit > 1 && (c.head_dim % (32 * e->att_dsplit) || (e->att_dsplit & (e->att_dsplit - 1)))) --e->att_dsplit;
    if (e->qw % 128 == 0) {  // whole 4-block groups
        if (M.get(&e->att_act, (size_t)e->qw)) return -1;
        if (M.get(&e->att_da, (size_t)e->qw / 32 * 4)) return -1;
        if (M.get_zeroed(&e->front_cnt, (size_t)c.n_layer * 16 * 32 * 4, s)) return -1;
        if (M.get_zeroed(&e->front_err, 64, s)) return -1;
        if (M.get_zeroed(&e->ao_cnt, (size_t)c.n_layer * 16 * 32 * 4, s)) return -1;
        if (M.get_zeroed(&e->ao_err, 64, s)) return -1;
    }
    if (e->sh_ff % 128 == 0) {  // every rank's shard is whole 4-block groups
        if (M.get(&e->h_act, (size_t)c.n_ff)) return -1;
        if (M.get(&e->h_da, (size_t)c.n_ff / 32 * 4)) return -1;
    }
    if (M.get(&e->logits, (size_t)c.n_vocab * 4)) return -1;
    if (e->kq) {
        const int64_t kmax = std::max<int64_t>(std::max<int64_t>(c.n_embd, e->qw), c.n_ff);
        const size_t img = (size_t)(kmax / 256 * 292 + 255) & ~(size_t)255;
        if (M.get(&e->kq_x, 4 * img)) return -1;
        e->kq_xa = e->kq_x + img;
        e->kq_xf = e->kq_x + 2 * img;
        e->kq_xh = e->kq_x + 3 * img;
        // counters: a quantize hand-off takes rows/256 (gate/up: n_ff/256), a norm hand-off rows/256 + 1
        // (down, attn-out: n_embd/256 + 1 — more than n_ff/256 when n_ff <= n_embd)
        e->kq_cnt_cap = (int)std::max<int64_t>(std::max<int64_t>(c.n_ff / 256, c.n_embd / 256 + 1), 1);
        if (M.get_zeroed(&e->kq_cnt, (size_t)e->kq_cnt_cap * 128, s)) return -1;
        if (M.get(&e->kq_g, (size_t)c.n_ff * 4)) return -1;
    }
    {  // the persistent token launch: granules, epoch, error word, argument copies
        const tok_gran_sizes g = token_gran_sizes(c.n_embd, c.n_ff, e->qkv_rows);
        const size_t n = g.gx + g.gqkv + g.gatt + g.gatt_da + g.gsa + g.gh + g.gh_da;
        if (M.get_zeroed(&e->tok_gran, n * 8, s)) return -1;
        if (M.get_zeroed(&e->epoch, 64, s)) return -1;
        static const unsigned one = 1;  // after the zeroing, on its stream
        GHIP_CHECK(hipMemcpyAsync(e->epoch, &one, 4, hipMemcpyHostToDevice, s));
        if (M.get_zeroed(&e->tok_err, 64, s)) return -1;
        if (M.get(&e->tok_dev, sizeof(tok_args))) return -1;
        if (M.get(&e->tok_tab, (size_t)c.n_layer * sizeof(tok_layer))) return -1;
    }
    if (M.get(&e->key, (size_t)e->grid_big * 8)) return -1;  // per-workgroup argmax keys
    GHIP_CHECK(hipMemsetAsync(e->key, 0, (size_t)e->grid_big * 8, s));
    if (M.get(&e->rank_keys, (size_t)e->tp_n * 8)) return -1;
    return 0;
}

// GEMMA_TP_P2P: inboxes mirroring every gathered vector, then one flag word per source rank
static int create_p2p_arena(gemma_engine *e) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    dev_pool &M = e->mem;
    size_t off = 0;
    auto take = [&](int64_t &ib, size_t bytes) { ib = (int64_t)off; off += (bytes + 255) & ~(size_t)255; };
    take(e->ib_qkv, (size_t)e->qkv_rows * 4);
    take(e->ib_sa, (size_t)c.n_embd * 4);
    take(e->ib_h, (size_t)c.n_ff * 4);
    take(e->ib_x, (size_t)c.n_embd * 4);
    take(e->ib_hact, e->h_act ? (size_t)c.n_ff : 0);
    take(e->ib_hda, e->h_act ? (size_t)c.n_ff / 32 * 4 : 0);
    take(e->ib_logits, (size_t)c.n_vocab * 4);
    take(e->ib_keys, (size_t)e->tp_n * 8);
    take(e->ib_flags, (size_t)P2P_MAX_RANKS * 4);
    if (M.get_zeroed(&e->p2p_arena, off, s, MEM_UNCACHED)) return -1;
    if (M.get_zeroed(&e->p2p_seq, 64, s)) return -1;
    if (M.get_zeroed(&e->p2p_err, 64, s)) return -1;
    e->p2p_peer[e->tp_rank] = e->p2p_arena;
    return 0;
}

static gemma_engine *engine_create(const gemma_hip_config *cfg, int device, int tp_n, int tp_rank, const void *nccl_id,
                                   const host_weights *hw = nullptr, const std::vector<uint16_t *> *kc_ext = nullptr,
                                   const std::vector<uint16_t *> *vc_ext = nullptr, int tp_flags = 0) {
    set_error("");
    const gemma_hip_config &c = *cfg;
    if (!config_ok(c, tp_n, nccl_id)) return nullptr;
    if (hipSetDevice(device) != hipSuccess) {
        set_error("gemma_engine_create: hipSetDevice failed");
        return nullptr;
    }
    constexpr bool cprof = false;  // engine-creation phase timings to stderr (diagnostics build: set true)
    auto cnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double ct0 = cprof ? cnow() : 0.0;
    auto *e = new gemma_engine();
    e->cfg = c;
    e->device = device;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("gemma_engine_create: hipStreamCreateWithFlags failed");
        delete e;
        return nullptr;
    }
    if (!set_shards(e, tp_n, tp_rank, nccl_id, tp_flags)) {  // nothing allocated yet, tp_n not validated
        (void)hipStreamDestroy(e->stream);
        delete e;
        return nullptr;
    }
    e->kq = c.wtype == T_Q4_K;
    e->out_type = (c.out_type == T_Q6_K || e->kq) ? T_Q6_K : c.wtype;
    // an allocation or a host-weight upload failed (last_error says which)
    bool up_fail = create_embeddings(e, hw) != 0;
    e->layers.resize((size_t)c.n_layer * e->n_virtual);
    for (int il = 0; il < c.n_layer && !up_fail; ++il)
        for (int vr = 0; vr < e->n_virtual && !up_fail; ++vr)
            up_fail = create_layer_norms(e, il, vr, hw) || (e->kq ? create_layer_kq(e, il, hw) : create_layer_tiled(e, il, vr, hw));
    if (up_fail) {
        gemma_engine_free(e);
        return nullptr;
    }
    if (cprof) {
        (void)hipStreamSynchronize(e->stream);
        fprintf(stderr, "[gemma_hip] engine create: weights %.2f ms\n", cnow() - ct0);
    }
    if (create_buffers(e, kc_ext, vc_ext) || (e->p2p && create_p2p_arena(e)) ||
        hipStreamSynchronize(e->stream) != hipSuccess) {
        if (last_error().empty()) set_error("gemma_engine_create: hipStreamSynchronize failed");
        gemma_engine_free(e);
        return nullptr;
    }
    // a communicator whenever an id is given, also for ONE rank: every gather, the key gather and
    // RCCL inside the captured hipGraph then run exactly as on N GPUs (a 1-rank all-gather in place)
    if (nccl_id) {
        ncclUniqueId id;
        memcpy(&id, nccl_id, sizeof(id));
        const ncclResult_t nr = ncclCommInitRank(&e->comm, tp_n, id, tp_rank);
        if (nr != ncclSuccess) set_error(std::string("ncclCommInitRank: ") + ncclGetErrorString(nr));
    }
    e->tp_n_keys = tp_n > 1 || e->comm;
    // default launch plan (the shapes of every rank's shards are equal)
    const layer_dev &L0 = e->layers[0];
    e->plan[MC_QKV] = {pick_ks(c.wtype, L0.qkv.n_bt, e->ks_small), 1, 0};
    e->plan[MC_O] = {pick_ks(c.wtype, L0.o.n_bt, e->ks_small), 1, e->att_act ? 1 : 0};  // the image feeds the fused front
    e->plan[MC_GU] = {1, 1, 0};
    e->plan[MC_DOWN] = {pick_ks(c.wtype, L0.down.n_bt, e->ks_down), 1, 0};
    e->plan[MC_LOGITS] = {1, 8, 0};  // 8 row tiles per workgroup: the round-5 bench lines' best
    if (last_error().empty()) (void)tok_prepare(e);  // K-quant engines: persist_why = "K-quant layers"
    if (!last_error().empty()) {
        gemma_engine_free(e);
        return nullptr;
    }
    if (cprof) fprintf(stderr, "[gemma_hip] engine create: total %.2f ms\n", cnow() - ct0);
    return e;
}

extern "C" gemma_engine *gemma_engine_create(const gemma_hip_config *cfg, int device) {
    return engine_create(cfg, device, 1, 0, nullptr);
}

// A Gemma GGUF file: hyper parameters as src/gemma_model.cpp:403-415 reads them (head_dim =
// gemma.attention.key_length when present, else n_embd / n_head as the reference computes it;
// rope base gemma.rope.freq_base, else 10000 as src/macro.h), tensors by the names of :145-182.
extern "C" gemma_engine *gemma_engine_create_from_gguf(const char *path, int n_ctx, int device) {
    set_error("");
    ggml_context *w = nullptr;
    gguf_init_params gp = {false, &w};
    gguf_context *g = gguf_init_from_file(path, gp);
    if (!g) return nullptr;
    std::string err;
    auto u32 = [&](const char *key, int def) -> int {
        const int i = gguf_find_key(g, key);
        if (i < 0 || gguf_get_kv_type(g, i) != GGUF_TYPE_UINT32) {
            if (def < 0 && err.empty()) err = std::string("missing u32 key ") + key;
            return def;
        }
        return (int)gguf_get_val_u32(g, i);
    };
    auto f32 = [&](const char *key, float def) -> float {
        const int i = gguf_find_key(g, key);
        return i >= 0 && gguf_get_kv_type(g, i) == GGUF_TYPE_FLOAT32 ? gguf_get_val_f32(g, i) : def;
    };
    gemma_hip_config c{};
    c.n_layer = u32("gemma.block_count", -1);
    c.n_embd = u32("gemma.embedding_length", -1);
    c.n_head = u32("gemma.attention.head_count", -1);
    c.n_head_kv = u32("gemma.attention.head_count_kv", -1);
    c.head_dim = c.n_head > 0 ? u32("gemma.attention.key_length", c.n_embd / c.n_head) : 0;
    c.eps = f32("gemma.attention.layer_norm_rms_epsilon", 1e-6f);
    c.rope_base = f32("gemma.rope.freq_base", 10000.0f);
    c.n_ctx = n_ctx;
    const int qw = c.n_head * c.head_dim, kvw = c.n_head_kv * c.head_dim;
    auto tensor = [&](const std::string &name, int type, int64_t ne0, int64_t ne1) -> const void * {
        ggml_tensor *t = err.empty() ? ggml_get_tensor(w, name.c_str()) : nullptr;
        if (!err.empty()) return nullptr;
        if (!t) {
            err = "missing tensor " + name;
            return nullptr;
        }
        if ((type >= 0 && (int)t->type != type) || t->ne[0] != ne0 || t->ne[1] != ne1 || t->ne[2] != 1) {
            err = "tensor " + name + ": type " + std::to_string(t->type) + " [" + std::to_string(t->ne[0]) + ", " +
                  std::to_string(t->ne[1]) + "] does not fit this engine";
            return nullptr;
        }
        return t->data;
    };
    host_weights hw;
    ggml_tensor *te = err.empty() ? ggml_get_tensor(w, "token_embd.weight") : nullptr;
    ggml_tensor *tq = err.empty() ? ggml_get_tensor(w, "blk.0.attn_q.weight") : nullptr;
    ggml_tensor *tg = err.empty() ? ggml_get_tensor(w, "blk.0.ffn_gate.weight") : nullptr;
    if (err.empty() && (!te || !tq || !tg)) err = "missing token_embd / blk.0 tensors";
    if (err.empty()) {
        c.n_vocab = (int)te->ne[1];
        c.n_ff = (int)tg->ne[1];
        c.wtype = (int)tq->type;
        c.out_type = te->type == GGML_TYPE_Q6_K ? T_Q6_K : 0;
        if (tq->type == GGML_TYPE_Q4_K || tq->type == GGML_TYPE_Q6_K) {  // K-quant layers (Q4_K_M files)
            c.wtype = T_Q4_K;
            if (te->type != GGML_TYPE_Q6_K) err = "K-quant layers need a Q6_K token_embd";
        } else if ((c.wtype != T_Q4_0 && c.wtype != T_Q8_0) || (te->type != tq->type && te->type != GGML_TYPE_Q6_K)) {
            err = "layer matrices must all be Q4_0 or all Q8_0 (or Q4_K / Q6_K), token_embd that type or Q6_K";
        }
    }
    const bool kqm = c.wtype == T_Q4_K;
    // a layer matrix of the layer type; K-quant layers: each Q4_K or Q6_K, the type recorded
    auto mat = [&](const std::string &name, int64_t ne0, int64_t ne1, int &type) -> const void * {
        if (!kqm) return tensor(name, c.wtype, ne0, ne1);
        const void *d = tensor(name, -1, ne0, ne1);
        if (!d) return nullptr;
        const int t = (int)ggml_get_tensor(w, name.c_str())->type;
        if (t != T_Q4_K && t != T_Q6_K) {
            err = "tensor " + name + ": K-quant layers must be Q4_K or Q6_K";
            return nullptr;
        }
        type = t;
        return d;
    };
    hw.embd = tensor("token_embd.weight", (c.out_type || kqm) ? T_Q6_K : c.wtype, c.n_embd, c.n_vocab);
    hw.out_norm = (const float *)tensor("output_norm.weight", GGML_TYPE_F32, c.n_embd, 1);
    for (int il = 0; il < c.n_layer && err.empty(); ++il) {
        const std::string b = "blk." + std::to_string(il) + ".";
        host_weights::layer L;
        L.attn_norm = (const float *)tensor(b + "attn_norm.weight", GGML_TYPE_F32, c.n_embd, 1);
        L.ffn_norm = (const float *)tensor(b + "ffn_norm.weight", GGML_TYPE_F32, c.n_embd, 1);
        L.q = mat(b + "attn_q.weight", c.n_embd, qw, L.tq);
        L.k = mat(b + "attn_k.weight", c.n_embd, kvw, L.tk);
        L.v = mat(b + "attn_v.weight", c.n_embd, kvw, L.tv);
        L.o = mat(b + "attn_output.weight", qw, c.n_embd, L.to);
        L.gate = mat(b + "ffn_gate.weight", c.n_embd, c.n_ff, L.tg);
        L.up = mat(b + "ffn_up.weight", c.n_embd, c.n_ff, L.tu);
        L.down = mat(b + "ffn_down.weight", c.n_ff, c.n_embd, L.td);
        hw.layers.push_back(L);
    }
    gemma_engine *e = nullptr;
    if (err.empty()) e = engine_create(&c, device, 1, 0, nullptr, &hw);
    else set_error("gemma_engine_create_from_gguf: " + std::string(path) + ": " + err);
    gguf_free(g);
    ggml_free(w);  // the device holds the weights now
    return e;
}

extern "C" int gemma_engine_config(const gemma_engine *e, gemma_hip_config *out) {
    if (!e || !out) return -1;
    *out = e->cfg;
    return 0;
}

// the engine's row split: [ranks, this rank, RCCL communicator present, shard slots in this engine]
extern "C" int gemma_engine_tp_info(const gemma_engine *e, int *out4) {
    if (!e || !out4) return -1;
    out4[0] = e->tp_n;
    out4[1] = e->tp_rank;
    out4[2] = e->comm ? 1 : 0;
    out4[3] = e->n_virtual;
    return 0;
}

// row-split tensor parallelism: one process per GPU; rank 0 makes the id, every rank gets a copy
extern "C" int gemma_tp_unique_id(void *out, int cap) {
    set_error("");
    if (cap < (int)sizeof(ncclUniqueId)) {
        set_error("gemma_tp_unique_id: buffer too small");
        return -1;
    }
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) {
        set_error(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
        return -1;
    }
    memcpy(out, &id, sizeof(id));
    return (int)sizeof(id);
}

// nccl_id == NULL with n_ranks > 1: every rank's shards in this one engine on one GPU (virtual
// ranks; the parity mode for boxes with a single GPU, where RCCL refuses two ranks per device)
extern "C" gemma_engine *gemma_engine_create_tp(const gemma_hip_config *cfg, int device, int n_ranks, int rank,
                                                const void *nccl_id) {
    return engine_create(cfg, device, n_ranks, nccl_id ? rank : 0, nccl_id);
}

// the same with layout flags (GEMMA_TP_REP_ATTN: the attention block whole on every rank)
extern "C" gemma_engine *gemma_engine_create_tp2(const gemma_hip_config *cfg, int device, int n_ranks, int rank,
                                                 const void *nccl_id, int flags) {
    return engine_create(cfg, device, n_ranks, (nccl_id || (flags & GEMMA_TP_P2P)) ? rank : 0, nccl_id, nullptr, nullptr,
                         nullptr, flags);
}

// GEMMA_TP_P2P: this rank's arena as an IPC handle (hipIpcMemHandle_t bytes) for the other ranks
extern "C" int gemma_engine_p2p_handle(const gemma_engine *e, void *out, int cap) {
    set_error("");
    if (!e || !e->p2p || !out || cap < (int)sizeof(hipIpcMemHandle_t)) {
        set_error("gemma_engine_p2p_handle: not a p2p engine, or buffer too small");
        return -1;
    }
    (void)hipSetDevice(e->device);
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, e->p2p_arena) != hipSuccess) {
        set_error("gemma_engine_p2p_handle: hipIpcGetMemHandle failed");
        return -1;
    }
    memcpy(out, &h, sizeof(h));
    return (int)sizeof(h);
}

// every rank's handle in rank order (n = ranks, each hipIpcMemHandle_t bytes); this rank's own entry
// is ignored.  Every rank must have opened its peers before any rank's first step (a host barrier).
extern "C" int gemma_engine_p2p_open(gemma_engine *e, const void *handles, int n) {
    set_error("");
    if (!e || !e->p2p || !handles || n != e->tp_n || e->p2p_ready) {
        set_error("gemma_engine_p2p_open: not a p2p engine, wrong rank count, or already open");
        return -1;
    }
    (void)hipSetDevice(e->device);
    for (int r = 0; r < n; ++r) {
        if (r == e->tp_rank) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, (const uint8_t *)handles + (size_t)r * sizeof(h), sizeof(h));
        void *p = nullptr;
        if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !p) {
            set_error("gemma_engine_p2p_open: hipIpcOpenMemHandle failed for rank " + std::to_string(r));
            return -1;
        }
        e->p2p_peer[r] = (uint8_t *)p;
    }
    e->p2p_ready = true;
    return 0;
}

// the sticky timeout word of the p2p gathers (reset: clear it)
extern "C" int gemma_engine_p2p_err(gemma_engine *e, int reset) {
    if (!e || !e->p2p) return -1;
    (void)hipSetDevice(e->device);
    unsigned v = 0;
    if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(&v, e->p2p_err, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (reset) (void)hipMemset(e->p2p_err, 0, 4);
    return (int)v;
}

extern "C" int gemma_engine_tp_flags(const gemma_engine *e) {
    return e ? (e->rep_attn ? GEMMA_TP_REP_ATTN : 0) | (e->p2p ? GEMMA_TP_P2P : 0) : -1;
}

extern "C" void gemma_engine_free(gemma_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    if (e->p2p)
        for (int r = 0; r < e->tp_n; ++r)
            if (r != e->tp_rank && e->p2p_peer[r]) (void)hipIpcCloseMemHandle(e->p2p_peer[r]);
    drop_graph(e);
    for (hipEvent_t &ev : e->fc_ev)
        if (ev) (void)hipEventDestroy(ev);
    e->bt_mem.clear();
    e->pf_mem.clear();
    e->mem.clear();
    (void)hipStreamDestroy(e->stream);
    delete e;
}

// ---- a sequence (seq_state, engine_impl.h) --------------------------------------------------------
// What is done to a sequence, once for the engine's own and for a batch slot: its buffers, the reset
// to a prompt, the copy, the cache and token read-backs, and the token-id check of everything the
// host hands in.
bool token_ids_ok(const gemma_engine *e, const int32_t *tokens, int n, const char *fn, bool name_id) {
    for (int i = 0; i < n; ++i)  // the embedding kernels index token_embd rows unchecked
        if (tokens[i] < 0 || tokens[i] >= e->cfg.n_vocab) {
            set_error(name_id ? std::string(fn) + ": token id " + std::to_string(tokens[i]) + " out of range [0, n_vocab)"
                              : std::string(fn) + ": token id out of range");
            return false;
        }
    return true;
}

int seq_alloc(gemma_engine *e, dev_pool &M, seq_state &S, bool caches, int *token_word) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    const size_t kv_bytes = (size_t)c.n_layer * c.n_ctx * e->kvw * 2;
    S = seq_state{};
    if (caches && (M.get_zeroed(&S.kc, kv_bytes, s) || M.get_zeroed(&S.vc, kv_bytes, s))) return -1;
    if (M.get_zeroed(&S.hist, (size_t)(c.n_ctx + 1) * 4, s) || M.get_zeroed(&S.pos, 4, s) || M.get_zeroed(&S.nfix, 4, s) ||
        M.get_zeroed(&S.rope, (size_t)(c.head_dim + 4) * 4, s) || M.get(&S.lp, (size_t)(c.n_ctx + 1) * 8))
        return -1;
    GHIP_CHECK(hipMemsetAsync(S.lp, 0xFF, (size_t)(c.n_ctx + 1) * 8, s));  // NaN: nothing is scored
    S.token = token_word;
    return token_word ? 0 : M.get_zeroed(&S.token, 4, s);
}

int seq_begin(gemma_engine *e, seq_state &S, const int32_t *tokens, int n) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    const size_t layer_bytes = (size_t)c.n_ctx * e->kvw * 2;
    if (S.kc) {  // the sequence's own allocation: all layers at once
        GHIP_CHECK(hipMemsetAsync(S.kc, 0, c.n_layer * layer_bytes, s));
        GHIP_CHECK(hipMemsetAsync(S.vc, 0, c.n_layer * layer_bytes, s));
    }
    for (int il = 0; il < (S.kc ? 0 : c.n_layer); ++il) {  // external caches: one allocation per layer
        GHIP_CHECK(hipMemsetAsync(kc_of(e, S, il), 0, layer_bytes, s));
        GHIP_CHECK(hipMemsetAsync(vc_of(e, S, il), 0, layer_bytes, s));
    }
    GHIP_CHECK(hipMemsetAsync(S.hist, 0, (size_t)(c.n_ctx + 1) * 4, s));
    GHIP_CHECK(hipMemcpyAsync(S.hist, tokens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    GHIP_CHECK(hipMemsetAsync(S.lp, 0xFF, (size_t)(c.n_ctx + 1) * 8, s));  // all-ones bytes: an f64 NaN, "not scored"
    GHIP_CHECK(hipMemsetAsync(S.pos, 0, 4, s));
    const size_t half = (size_t)c.head_dim / 2;  // RoPE row of position 0
    GHIP_CHECK(hipMemcpyAsync(S.rope, e->rope_cos, half * 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemcpyAsync(S.rope + half, e->rope_sin, half * 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemsetAsync(S.rope + 2 * half, 0, 4, s));
    GHIP_CHECK(hipMemcpyAsync(S.nfix, &n, 4, hipMemcpyHostToDevice, s));
    GHIP_CHECK(hipStreamSynchronize(s));
    S.n_given = n;
    S.host_pos = 0;
    return 0;
}

int seq_copy(gemma_engine *e, seq_state &dst, const seq_state &src) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    const size_t layer = (size_t)c.n_ctx * e->kvw;  // elements
    for (int il = 0; il < c.n_layer; ++il) {  // (an engine on external caches has one allocation per layer)
        GHIP_CHECK(hipMemcpyAsync(kc_of(e, dst, il), kc_of(e, src, il), layer * 2, hipMemcpyDeviceToDevice, s));
        GHIP_CHECK(hipMemcpyAsync(vc_of(e, dst, il), vc_of(e, src, il), layer * 2, hipMemcpyDeviceToDevice, s));
    }
    GHIP_CHECK(hipMemcpyAsync(dst.hist, src.hist, (size_t)(c.n_ctx + 1) * 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemcpyAsync(dst.lp, src.lp, (size_t)(c.n_ctx + 1) * 8, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemcpyAsync(dst.pos, src.pos, 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemcpyAsync(dst.nfix, src.nfix, 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemcpyAsync(dst.token, src.hist + src.host_pos, 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipMemcpyAsync(dst.rope, src.rope, ((size_t)c.head_dim + 1) * 4, hipMemcpyDeviceToDevice, s));
    GHIP_CHECK(hipStreamSynchronize(s));
    dst.host_pos = src.host_pos;
    dst.n_given = src.n_given;
    return 0;
}

int seq_kv_read(gemma_engine *e, const seq_state &S, int layer, int p0, int n, uint16_t *k_rows, uint16_t *v_rows, const char *fn) {
    const gemma_hip_config &c = e->cfg;
    if (layer < 0 || layer >= c.n_layer || p0 < 0 || n < 1 || (int64_t)p0 + n > c.n_ctx || !k_rows || !v_rows) {
        set_error(std::string(fn) + ": layer or positions out of range");
        return -1;
    }
    (void)hipSetDevice(e->device);
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    const size_t kvw = (size_t)e->kvw, ctx = (size_t)c.n_ctx;
    GHIP_CHECK(hipMemcpy(k_rows, kc_of(e, S, layer) + (size_t)p0 * kvw, (size_t)n * kvw * 2, hipMemcpyDeviceToHost));
    std::vector<uint16_t> vt(kvw * (size_t)n);  // V is [kvw][ctx]: columns p0 .. p0+n, then transposed
    GHIP_CHECK(hipMemcpy2D(vt.data(), (size_t)n * 2, vc_of(e, S, layer) + p0, ctx * 2, (size_t)n * 2, kvw, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < kvw; ++j)
        for (size_t r = 0; r < (size_t)n; ++r) v_rows[r * kvw + j] = vt[j * (size_t)n + r];
    return 0;
}

int seq_logprobs(gemma_engine *e, const seq_state &S, int p0, int n, double *out, const char *fn) {
    const int n_seq = std::max(S.host_pos + 1, S.n_given);  // the sequence so far: given tokens and the pending pick
    if (p0 < 0 || n < 0 || (int64_t)p0 + n > n_seq || (n > 0 && !out)) {
        set_error(std::string(fn) + ": [" + std::to_string(p0) + ", " + std::to_string((int64_t)p0 + n) + ") outside [0, n_seq = " +
                  std::to_string(n_seq) + "), or a null buffer");
        return -1;
    }
    (void)hipSetDevice(e->device);
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    if (n) GHIP_CHECK(hipMemcpy(out, S.lp + p0, (size_t)n * 8, hipMemcpyDeviceToHost));
    return n;
}

int seq_tokens(const seq_state &S, int32_t *out, int cap) {
    const int n = std::min(cap, S.host_pos + 1);  // the pending token included
    if (n) GHIP_CHECK(hipMemcpy(out, S.hist, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

extern "C" int gemma_engine_begin(gemma_engine *e, const int32_t *prompt, int n_prompt) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    if (n_prompt <= 0 || n_prompt >= c.n_ctx) {
        set_error("gemma_engine_begin: prompt length out of range");
        return -1;
    }
    if (!token_ids_ok(e, prompt, n_prompt, "gemma_engine_begin")) return -1;
    (void)hipSetDevice(e->device);
    // the decode step's argmax keys start from zero; the epoch is not bumped (gemma_engine_extend's
    // k_set_position bumps it)
    GHIP_CHECK(hipMemsetAsync(e->key, 0, (size_t)e->grid_big * 8, e->stream));
    return seq_begin(e, e->seq, prompt, n_prompt);
}

// Continue or rewind: positions [0, keep) stay, everything from `keep` on is dropped and `tokens`
// become the given-but-unprocessed positions keep .. keep+n-1.  The device state afterwards is byte
// for byte what gemma_engine_begin with the same sequence plus `keep` processed positions leaves:
// cache rows / columns >= keep and hist past the tokens zero, *pos, the RoPE row and *n_fixed
// published as k_set_position does.  Every buffer keeps its address, so the captured decode graph
// stays valid.
extern "C" int gemma_engine_extend(gemma_engine *e, int keep, const int32_t *tokens, int n) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    if (keep < 0 || keep > e->seq.host_pos) {
        set_error("gemma_engine_extend: keep = " + std::to_string(keep) + " outside [0, pos = " + std::to_string(e->seq.host_pos) + "]");
        return -1;
    }
    if (n <= 0 || !tokens || (int64_t)keep + n >= c.n_ctx) {
        set_error("gemma_engine_extend: needs n >= 1 tokens with keep + n < n_ctx");
        return -1;
    }
    if (!token_ids_ok(e, tokens, n, "gemma_engine_extend")) return -1;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    const size_t ctx = (size_t)c.n_ctx, drop = ctx - (size_t)keep;
    for (int il = 0; il < c.n_layer; ++il) {  // K [ctx][kvw]: rows >= keep; V [kvw][ctx]: columns >= keep
        GHIP_CHECK(hipMemsetAsync(kc_of(e, e->seq, il) + (size_t)keep * e->kvw, 0, drop * e->kvw * 2, s));
        GHIP_CHECK(hipMemset2DAsync(vc_of(e, e->seq, il) + keep, ctx * 2, 0, drop * 2, (size_t)e->kvw, s));
    }
    GHIP_CHECK(hipMemsetAsync(e->seq.hist + keep, 0, (ctx + 1 - (size_t)keep) * 4, s));
    GHIP_CHECK(hipMemcpyAsync(e->seq.hist + keep, tokens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    // row keep - 1 is not recomputed: lp[keep] is "not scored" with everything behind it
    GHIP_CHECK(hipMemsetAsync(e->seq.lp + keep, 0xFF, (ctx + 1 - (size_t)keep) * 8, s));
    GHIP_CHECK(hipMemsetAsync(e->key, 0, (size_t)e->grid_big * 8, s));
    // *pos = keep, its RoPE row with the position word, *n_fixed = keep + n, the epoch bump
    if (launch_set_position(tokens[0], keep, e->seq.pos, e->seq.hist, e->seq.nfix, keep + n, rope_of(e), s)) return -1;
    GHIP_CHECK(hipStreamSynchronize(s));
    e->seq.n_given = keep + n;
    e->seq.host_pos = keep;
    return 0;
}

// the decode step captured once in a hipGraph (after a first eager step has set the kernels' LDS attributes)
int ensure_graph(gemma_engine *e) {
    if (e->graph_exec) return 0;
    GHIP_CHECK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed));
    const int r = enqueue_step(e);
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->stream, &g);
    if (r != 0) return -1;
    if (ce != hipSuccess) {
        set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
        return -1;
    }
    e->graph = g;
    GHIP_CHECK(hipGraphInstantiate(&e->graph_exec, g, nullptr, nullptr, 0));
    return 0;
}

extern "C" int gemma_engine_step(gemma_engine *e, int n, float *logits, int use_graph) {
    set_error("");
    (void)hipSetDevice(e->device);
    if (e->p2p && !e->p2p_ready) {
        set_error("gemma_engine_step: p2p engine whose peers are not open (gemma_engine_p2p_open)");
        return -1;
    }
    const gemma_hip_config &c = e->cfg;
    if (e->seq.host_pos + n >= c.n_ctx) {
        set_error("gemma_engine_step: context full");
        return -1;
    }
    if (n <= 0) return 0;  // nothing to run (no warm-up step, no logits written)
    if (use_graph && !e->graph_exec) {
        // first eager step sets the kernels' LDS attributes before capture
        if (enqueue_step(e)) return -1;
        if (logits && tp_gather(e, e->logits, e->sh_v)) return -1;
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        if (logits) GHIP_CHECK(hipMemcpy(logits, e->logits, (size_t)c.n_vocab * 4, hipMemcpyDeviceToHost));
        e->seq.host_pos += 1;
        if (logits) logits += c.n_vocab;
        n -= 1;
        if (ensure_graph(e)) return -1;
    }
    // Flow control: at most FC_EVERY * FC_SLOTS decode graphs (x 92 kernels) queued ahead of the GPU,
    // so a long call never parks thousands of dispatch packets in the HW queue.  Waiting on the event
    // of the launch FC_EVERY * FC_SLOTS back never drains the queue: the GPU never idles, the host only
    // stops running ahead.  (It was added as the first lead on the rocprofv3 crash of DESIGN.md §11 and
    // did not cure it: that crash is the profiler reading past the end of the 1 MiB AQL ring when a
    // HIP 7.2 graph launch's packet batch wraps around it, whatever the queue depth.)
    constexpr int FC_EVERY = 16, FC_SLOTS = 4;
    for (int i = 0; i < n; ++i) {
        if (use_graph && !logits && i % FC_EVERY == 0) {
            hipEvent_t &ev = e->fc_ev[(i / FC_EVERY) % FC_SLOTS];
            if (!ev) GHIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            if (i >= FC_EVERY * FC_SLOTS) GHIP_CHECK(hipEventSynchronize(ev));
            GHIP_CHECK(hipEventRecord(ev, e->stream));
        }
        if (use_graph) GHIP_CHECK(hipGraphLaunch(e->graph_exec, e->stream));
        else if (enqueue_step(e)) return -1;
        if (logits) {
            if (tp_gather(e, e->logits, e->sh_v)) return -1;  // TP: the other ranks' vocab rows
            GHIP_CHECK(hipMemcpyAsync(logits + (size_t)i * c.n_vocab, e->logits, (size_t)c.n_vocab * 4,
                                      hipMemcpyDeviceToHost, e->stream));
            GHIP_CHECK(hipStreamSynchronize(e->stream));
        }
        e->seq.host_pos += 1;
    }
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    if (persist_check(e)) return -1;  // the sequence must be restarted (gemma_engine_begin)
    if (att_o_check(e)) return -1;
    return 0;
}

extern "C" int gemma_engine_sync(gemma_engine *e) {
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int gemma_engine_tokens(gemma_engine *e, int32_t *out, int cap) {
    return seq_tokens(e->seq, out, cap);
}

extern "C" int gemma_engine_pos(gemma_engine *e) { return e->seq.host_pos; }

extern "C" int gemma_engine_logprobs(gemma_engine *e, int p0, int n, double *out) {
    set_error("");
    return seq_logprobs(e, e->seq, p0, n, out, "gemma_engine_logprobs");
}

extern "C" int64_t gemma_engine_tensor(gemma_engine *e, int tid, void *dst, int64_t cap) {
    set_error("");
    (void)hipSetDevice(e->device);
    const gemma_hip_config &c = e->cfg;
    auto copy_f32 = [&](const float *p, int64_t n) -> int64_t {
        if (cap < n * 4) return -1;
        GHIP_CHECK(hipMemcpy(dst, p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return n * 4;
    };
    auto copy_mat = [&](const tiled_mat &m) -> int64_t {
        const int64_t bytes = m.rows * m.nb * (m.type == T_Q4_0 ? 18 : 34);
        if (cap < bytes) return -1;
        dev_pool tmp_mem;
        uint8_t *tmp = nullptr;
        if (tmp_mem.get(&tmp, (size_t)bytes)) return -1;
        if (launch_untile(m, tmp, e->stream)) return -1;
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        GHIP_CHECK(hipMemcpy(dst, tmp, (size_t)bytes, hipMemcpyDeviceToHost));
        return bytes;
    };
    // K-quant rows back in ggml layout
    auto copy_kq = [&](const uint8_t *w, int type, int64_t rows, int64_t K, bool tiled) -> int64_t {
        const int64_t bytes = K / 256 * (type == T_Q4_K ? 144 : 210) * rows;
        if (cap < bytes) return -1;
        if (!tiled) {
            GHIP_CHECK(hipMemcpy(dst, w, (size_t)bytes, hipMemcpyDeviceToHost));
            return bytes;
        }
        dev_pool tmp_mem;
        uint8_t *tmp = nullptr;
        if (tmp_mem.get(&tmp, (size_t)bytes)) return -1;
        if (launch_kq_retile(type, w, tmp, rows, K, false, e->stream)) return -1;
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        GHIP_CHECK(hipMemcpy(dst, tmp, (size_t)bytes, hipMemcpyDeviceToHost));
        return bytes;
    };
    if (tid == TID_EMBD && e->out_type == T_Q6_K) return copy_kq(e->embd_q6k, T_Q6_K, c.n_vocab, c.n_embd, e->embd_tiled);
    if (tid == TID_EMBD) return copy_mat(e->embd);
    if (tid == TID_OUT_NORM) return copy_f32(e->out_norm, c.n_embd);
    const int il = (tid - 16) / 16, k = (tid - 16) % 16;
    if (tid < 16 || il >= c.n_layer) return -1;
    layer_dev &L = e->layers[il];
    if (e->kq && k != L_ATTN_NORM && k != L_FFN_NORM) {  // raw K-quant rows
        const kq_layer &K = e->kql[il];
        const kq_mat *m = k == L_Q ? &K.q : k == L_K ? &K.k : k == L_V ? &K.v : k == L_O ? &K.o : k == L_GATE ? &K.gate
                        : k == L_UP ? &K.up : k == L_DOWN ? &K.down : nullptr;
        if (!m) return -1;
        return copy_kq(m->w, m->type, m->rows, m->K, m->tiled);
    }
    switch (k) {
        case L_ATTN_NORM: return copy_f32(L.attn_norm, c.n_embd);
        case L_FFN_NORM: return copy_f32(L.ffn_norm, c.n_embd);
        case L_Q: return copy_mat(sub_rows(L.qkv, 0, e->qw));
        case L_K: return copy_mat(sub_rows(L.qkv, e->qw, e->kvw));
        case L_V: return copy_mat(sub_rows(L.qkv, e->qw + e->kvw, e->kvw));
        case L_O: return copy_mat(L.o);
        case L_GATE: return copy_mat(L.gate);
        case L_UP: return copy_mat(L.up);
        case L_DOWN: return copy_mat(L.down);
    }
    return -1;
}

// the captured decode graph is stale (a plan, option or launch form changed): re-captured at the next step
void drop_graph(gemma_engine *e) {
    if (e->graph_exec) (void)hipGraphExecDestroy(e->graph_exec);
    if (e->graph) (void)hipGraphDestroy(e->graph);
    e->graph_exec = nullptr;
    e->graph = nullptr;
}
// ---- the ggml executor's fast path (engine_ext.h) ------------------------------------------------
gemma_engine *gemma_engine_create_ext(const gemma_hip_config *cfg, int device, const host_weights &hw,
                                      const std::vector<uint16_t *> &kc, const std::vector<uint16_t *> &vc) {
    if ((int)kc.size() != cfg->n_layer || (int)vc.size() != cfg->n_layer) {
        set_error("gemma_engine_create_ext: one K and one V cache per layer");
        return nullptr;
    }
    return engine_create(cfg, device, 1, 0, nullptr, &hw, &kc, &vc);
}
