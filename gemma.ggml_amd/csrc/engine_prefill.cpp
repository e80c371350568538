// engine_prefill.cpp — the batched prefill of the device-resident engine (tiled and K-quant
// layers), its taps, and the ggml executor's entry points (engine_ext.h), which drive a prefill or a
// decode step from host-supplied tokens.
#include <chrono>

#include "engine_impl.h"

// prefill buffers (lazily sized for the largest pass seen: the prompt, or a gemma_engine_prefill_next
// chunk).  A regrow drops the whole scratch and makes it anew; pf.T is set last, so a failed regrow
// leaves T = 0 and no pointer to freed memory.
// parts: the scratch also holds the log-probability partials of its rows (passes of more than 8 rows)
static int scratch_alloc(gemma_engine *e, dev_pool &M, pf_scratch &p, int T, bool parts) {
    if (p.T >= T && (!parts || p.LP)) return 0;
    T = std::max(T, p.T);
    M.clear();
    p = {};
    const gemma_hip_config &c = e->cfg;
    const int64_t E = c.n_embd, F = c.n_ff;
    p.ldq = (std::max(std::max(E, F), (int64_t)e->qw) + 255) / 256 * 256;
    p.ldd = p.ldq / 32;
    if (M.get(&p.X, (size_t)T * E * 4) || M.get(&p.SA, (size_t)T * E * 4) || M.get(&p.QKV, (size_t)T * e->qkv_rows * 4) ||
        M.get(&p.ATT, (size_t)T * e->qw * 4) || M.get(&p.G, (size_t)T * F * 4) || M.get(&p.U, (size_t)T * F * 4) ||
        M.get(&p.LG, (size_t)T * c.n_vocab * 4) ||  // all rows, as the reference computes them
        M.get(&p.DA, (size_t)T * p.ldd * 4) || M.get(&p.Q16, (size_t)T * e->qw * 2) ||
        // K-quant layers: XQ holds T Q8_K columns (292 B per 256 values) instead of the int8 image
        M.get(&p.XQ, (size_t)T * (e->kq ? p.ldq / 256 * 292 : p.ldq)) || M.get(&p.XH, (size_t)T * p.ldq * 2) ||
        M.get(&p.XM, (size_t)T * (p.ldq / 256) * 32) || M.get(&p.keys, 256 * 8) ||
        (e->out_type == T_Q6_K && M.get(&p.XQ8K, (size_t)T * (E / 256) * 292)) ||
        (parts && M.get(&p.LP, (size_t)T * lse_grid(c.n_vocab) * sizeof(lse_part)))) {
        M.clear();
        p = {};
        return -1;
    }
    p.T = T;
    return 0;
}
static int prefill_alloc(gemma_engine *e, int T) {
    return scratch_alloc(e, e->pf_mem, e->pf, T, e->logprobs && T > GEMM_SKINNY_MAX_T);
}

// What the T rows of a pass are.  Every scratch buffer is indexed by the row t; the rows description
// says where the T token ids come from and what runs at a layer's attention step:
//   batch == null   rows are positions p0 .. p0+T-1 of the engine's own sequence: RoPE + K / V store
//                   into the engine's caches, then the causal attention (prefill_attention)
//   batch           rows are a batch pass's (engine_batch.cpp): row t is the next token of its own
//                   slot (or one of several consecutive tokens of its slot: batch->src), the attention
//                   is enqueue_batch_attention and the scratch is the batch's (bt.pf)
//                   r0 > 0: the pass is rows [r0, r0 + T) of the batch's (a group of a wide pass): its
//                   tokens, its part of the row table and a view of the scratch shifted by r0 rows
struct pass_rows {
    const int *tokens = nullptr;  // device array of the T token ids
    int p0 = 0;
    const batch_pass *batch = nullptr;
    int r0 = 0;
};
static pass_rows own_rows(const gemma_engine *e, int p0) { return pass_rows{e->seq.hist + p0, p0, nullptr, 0}; }
// the scratch of a pass, by value: the engine's or the batch's, every row-indexed buffer shifted by
// the pass's first row (each by its own row stride: scratch_alloc)
static pf_scratch scratch_of(gemma_engine *e, const pass_rows &rows) {
    pf_scratch p = rows.batch ? e->bt.pf : e->pf;
    if (!rows.r0) return p;
    const gemma_hip_config &c = e->cfg;
    const size_t r = (size_t)rows.r0;
    p.T -= rows.r0;
    p.X += r * c.n_embd; p.SA += r * c.n_embd; p.QKV += r * e->qkv_rows; p.ATT += r * e->qw;
    p.G += r * c.n_ff; p.U += r * c.n_ff; p.LG += r * c.n_vocab;
    p.DA += r * p.ldd; p.Q16 += r * e->qw;
    p.XQ += r * (e->kq ? p.ldq / 256 * 292 : p.ldq); p.XH += r * p.ldq;
    p.XM += r * (p.ldq / 256) * 16;  // 32 bytes per 256 values
    if (p.XQ8K) p.XQ8K += r * (c.n_embd / 256) * 292;
    if (p.LP) p.LP += r * lse_grid(c.n_vocab);
    return p;
}

static int enqueue_prefill_kq(gemma_engine *e, int T, const pass_rows &rows);

// the K-quant prefill's MFMA GEMM (prefill_kq.hip) for T prompt rows (kq_gemm_min: default 8)
static bool kq_prefill_mfma(int T) { return T >= kq_gemm_min(); }
// T Q8_K columns of K values (ld bytes apart) -> the GEMM's f16 image in the prefill scratch
static int kq_expand(gemma_engine *e, pf_scratch &p, const uint8_t *x, int64_t ld, int64_t K, int T) {
    q8kx_args a;
    a.x = x; a.x_col_stride = ld; a.nsb = (int)(K / 256); a.T = T;
    a.xh = p.XH; a.ldh = p.ldq; a.xd = p.DA; a.ldd = p.ldd; a.xm = p.XM; a.ldm = p.ldq / 256;
    return launch_q8k_expand(a, e->stream);
}

// The exact prefill attention: on the f32 matrix cores where the shapes allow it (attn_mx.hip:
// v_mfma_f32_16x16x4_f32 is an fmaf chain over K, so vec_dot_f16's chains ride it bit for bit),
// else per row with v_fma_mix (k_attn_rows).  Option "att_mx" 0 forces the row form (tests, A/B).
// The form is resolved once per prefill (att_mx_form): the option and the shape check do not
// change between its layers.
static bool att_mx_form(const gemma_engine *e, const attnp_args &at) {
    return e->att_mx && !attn_mx_unsupported(at);
}
static int launch_attn_exact(const attnp_args &at, bool mx, hipStream_t s) {
    return mx ? launch_attn_mx(at, s) : launch_attn_rows(at, s);
}

// layer il of a T-row prefill of positions p0 .. p0+T-1, from pf.QKV: RoPE + K/V store into the
// layer caches (which hold the positions before p0), then the causal attention into pf.ATT (exact:
// the form *mx_form, resolved at the first layer; else f16 MFMA)
static int prefill_attention(gemma_engine *e, int il, int T, const pass_rows &rows, bool exact, int *mx_form) {
    if (rows.batch) return enqueue_batch_attention(e, *rows.batch, il, rows.r0, T);
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    auto &p = e->pf;
    const int p0 = rows.p0;
    ropekv_args r;
    r.qkv = p.QKV; r.ldqkv = e->qkv_rows; r.rope_cos = e->rope_cos; r.rope_sin = e->rope_sin; r.q16 = p.Q16;
    r.kc = kc_of(e, e->seq, il); r.vc = vc_of(e, e->seq, il);
    r.H = c.n_head; r.Hkv = c.n_head_kv; r.hd = c.head_dim; r.ctx = c.n_ctx; r.p0 = p0;
    r.q_scale = 1.0f / sqrtf((float)c.head_dim);
    if (launch_rope_kv_prefill(r, T, s)) return -1;
    attnp_args at;
    at.q16 = p.Q16; at.kc = r.kc; at.vc = r.vc; at.out = p.ATT; at.ldo = e->qw;
    at.T = T; at.H = c.n_head; at.Hkv = c.n_head_kv; at.hd = c.head_dim; at.ctx = c.n_ctx; at.p0 = p0;
    at.n_kv = std::min(32 * ((p0 + T) / 32 + 1), c.n_ctx);  // src/gemma_model.cpp:429 with n_total = p0 + T
    if (*mx_form < 0) *mx_form = att_mx_form(e, at);
    return exact ? launch_attn_exact(at, *mx_form == 1, s) : launch_attn_prefill(at, s);
}

// One batched pass over T rows.  Own rows (own_rows(e, p0)): hist[p0 .. p0+T), sequence positions
// p0 .. p0+T-1, the caches hold the positions before p0 (p0 = 0: the whole-prompt prefill).  Every
// scratch buffer is indexed by the row t of the pass; only the token reads, RoPE, the cache stores and
// the attention know what a row is (pass_rows).
// Two things a caller chooses apart from the rows (pass_end):
//   logits_only  the pass ends with the logits rows and the caller picks from every row (the verify
//                pass, a batch pass); else the last row's pick and the advance follow
//   skinny       T <= 8, exact: the Q4_0 / Q8_0 GEMMs go through launch_gemm_skinny (the verify pass,
//                a batch pass or group of up to 8 rows); else launch_gemm_exact / launch_gemm_q
struct pass_end {
    bool logits_only = false, skinny = false;
};
static int enqueue_prefill(gemma_engine *e, int T, const pass_rows &rows, bool exact, float *taps = nullptr, pass_end end = {}) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    int mx_form = -1;  // the exact attention's form, resolved at the first layer
    pf_scratch p = scratch_of(e, rows);
    const int wt = c.wtype;
    const int64_t E = c.n_embd, F = c.n_ff;
    const gemm_form form = gemm_form_now();  // one form for the whole pass: every image is written for the GEMM that reads it
    auto gemm = [&](const tiled_mat &m, int epi, const float *resid, float *y, int64_t ldy) {
        gemm_args g;
        set_mat(g, m);
        g.xq = p.XQ; g.xh = p.XH; g.ldq = p.ldq; g.da = p.DA; g.ldd = p.ldd; g.T = T; g.y = y; g.resid = resid; g.ldy = ldy;
        if (end.skinny) return launch_gemm_skinny(wt, epi, g, s);
        return exact ? launch_gemm_exact(wt, epi, form, g, s) : launch_gemm_q(wt, epi, g, s);
    };
    auto quant = [&](int mode, const float *x, const float *x2, int64_t K, const float *norm_w) {
        qrow_args a;
        a.x = x; a.x2 = x2; a.ldx = K; a.K = K; a.norm_w = norm_w; a.eps = c.eps;
        const bool i8img = exact && (end.skinny || form.i8);  // the int8-staged exact GEMM and the skinny GEMM read the int8 image
        a.q = (!exact || i8img) ? p.XQ : nullptr; a.qh = (exact && !i8img) ? p.XH : nullptr; a.ldq = p.ldq; a.da = p.DA; a.ldd = p.ldd;
        a.gelu_tab = e->gelu_tab; a.gelu_clamp = c.gelu_clamp;
        if (mode == QR_EMBED_NORM) {
            a.tokens = rows.tokens; a.emb_qs = e->embd.qs; a.emb_sc = e->embd.sc; a.emb_type = wt;
            a.emb_n_bt = e->embd.n_bt; a.emb_scale = sqrtf((float)E); a.emb_out = p.X; a.ldx = E;
        }
        return launch_quant_rows(mode, a, T, s);
    };
    const bool q6 = e->out_type == T_Q6_K;
    if (e->kq) {
        if (!exact) {
            set_error("gemma_engine_prefill_fast: K-quant layer engines have the exact batched prefill only");
            return -1;
        }
        if (enqueue_prefill_kq(e, T, rows)) return -1;
    } else if (q6 && launch_embed_q6K(e->embd_q6k, e->embd_row_bytes, rows.tokens, nullptr, T, (int)E, sqrtf((float)E), p.X, s, e->embd_tiled)) {
        return -1;
    }
    for (int il = 0; il < (e->kq ? 0 : c.n_layer); ++il) {
        layer_dev &L = e->layers[il];
        if (quant(il == 0 && !q6 ? QR_EMBED_NORM : QR_NORM, p.X, nullptr, E, L.attn_norm)) return -1;
        if (gemm(L.qkv, EPI_STORE, nullptr, p.QKV, e->qkv_rows)) return -1;
        if (prefill_attention(e, il, T, rows, exact, &mx_form)) return -1;
        if (quant(QR_F32, p.ATT, nullptr, e->qw, nullptr)) return -1;
        if (gemm(L.o, EPI_ADD, p.X, p.SA, E)) return -1;
        if (quant(QR_NORM, p.SA, nullptr, E, L.ffn_norm)) return -1;
        if (gemm(L.gate, EPI_STORE, nullptr, p.G, F)) return -1;
        if (gemm(L.up, EPI_STORE, nullptr, p.U, F)) return -1;
        if (quant(QR_GELU, p.G, p.U, F, nullptr)) return -1;
        if (gemm(L.down, EPI_ADD, p.SA, p.X, E)) return -1;
        if (taps) GHIP_CHECK(hipMemcpyAsync(taps + (size_t)il * T * E, p.X, (size_t)T * E * 4, hipMemcpyDeviceToDevice, s));
    }
    if (q6) {  // Q6_K tied output: Q8_K INIT of every row, then the K-quant dot per (vocab row, position)
        const int64_t ld = E / 256 * 292;
        if (launch_norm_q8K(p.X, E, e->out_norm, (int)E, c.eps, T, p.XQ8K, ld, s)) return -1;
        if (exact && kq_prefill_mfma(T) && e->embd_tiled && E % 2048 == 0) {  // the MFMA GEMM (prefill_kq.hip)
            if (kq_expand(e, p, p.XQ8K, ld, E, T)) return -1;
            kqg_args g;
            g.w = e->embd_q6k; g.row_bytes = e->embd_row_bytes; g.rows = c.n_vocab; g.nsb = (int)(E / 256); g.T = T;
            g.xh = p.XH; g.ldh = p.ldq; g.xd = p.DA; g.ldd = p.ldd; g.xm = p.XM; g.ldm = p.ldq / 256;
            g.y = p.LG; g.ldy = c.n_vocab;
            if (launch_gemm_kq(T_Q6_K, g, s)) return -1;
        } else if (enqueue_logits_q6k(e, p.XQ8K, T, p.LG)) {
            return -1;
        }
    } else {
        if (quant(QR_NORM, p.X, nullptr, E, e->out_norm)) return -1;
        if (gemm(e->embd, EPI_STORE, nullptr, p.LG, c.n_vocab)) return -1;
    }
    if (end.logits_only) return 0;
    const int p0 = rows.p0;
    // greedy token from the last row; position p0+T-1 -> p0+T, token appended at hist[p0+T] unless
    // that is still a given token (k_advance's p >= n_fixed guard: a pass that ends mid-prompt)
    // (with the sampler on: its draw at position p0+T from the same row, after *pos is in place)
    const float *last_row = p.LG + (size_t)(T - 1) * c.n_vocab;
    if (!e->sampling && launch_row_argmax(last_row, c.n_vocab, (unsigned long long *)p.keys, 256, s)) return -1;
    const int last = p0 + T - 1;
    GHIP_CHECK(hipMemcpyAsync(e->seq.pos, &last, 4, hipMemcpyHostToDevice, s));
    // (log-probabilities on: all T rows are scored, row t against hist[p0 + t + 1])
    return enqueue_pick(e, last_row, (const unsigned long long *)p.keys, 256, p.LG, T, T > GEMM_SKINNY_MAX_T ? p.LP : nullptr);
}

// Batched prefill for K-quant layers (the reference's shipped Q4_K_M model, src/app.cpp:36): the
// same T-column MUL_MATs the reference runs through mul_mat (src/hpc.cpp:216-273 with col_num = T),
// each (row, column) the decode dot (vec_dot_q{4,6}_K_q8_K in ggml's AVX2 lane order) against the
// column's Q8_K INIT — every K-quant launch covers all T columns (grid.y) — and the exact per-row
// attention of the Q4_0 prefill (k_rope_kv_prefill + k_attn_rows).  Bit-identical to the token
// loop and to the CPU path: no operation depends on the batching.
static int enqueue_prefill_kq(gemma_engine *e, int T, const pass_rows &rows) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    int mx_form = -1;  // the exact attention's form, resolved at the first layer
    pf_scratch p = scratch_of(e, rows);
    const int64_t E = c.n_embd, F = c.n_ff;
    const int64_t ldk = p.ldq / 256 * 292;  // Q8_K column stride in XQ
    uint8_t *img = (uint8_t *)p.XQ;
    // T >= kq_gemm_min() (default 8): the lane-tiled matrices go through the MFMA GEMM
    // (prefill_kq.hip) against the f16 image each Q8_K INIT is expanded to; below, or with
    // GHIP_KQ_MFMA=0, the dot4 T-column kernel.  Same bytes either way (tests/test_gpu_engine_gguf.py).
    const bool mfma = kq_prefill_mfma(T);
    auto mfma_ok = [&](const kq_mat &W) { return mfma && W.tiled && (W.type == T_Q4_K || W.K % 2048 == 0); };
    auto expand = [&](int64_t K) { return mfma ? kq_expand(e, p, img, ldk, K, T) : 0; };
    auto mv = [&](const kq_mat &W, float *y, int64_t ldy, const float *resid, const float *gate_in, const kq_mat *up) {
        if (!up && mfma_ok(W)) {
            kqg_args g;
            g.w = W.w; g.row_bytes = W.rb; g.rows = W.rows; g.nsb = (int)(W.K / 256); g.T = T;
            g.xh = p.XH; g.ldh = p.ldq; g.xd = p.DA; g.ldd = p.ldd; g.xm = p.XM; g.ldm = p.ldq / 256;
            g.y = y; g.ldy = ldy; g.resid = resid; g.gate_in = gate_in; g.gelu_tab = e->gelu_tab; g.gelu_clamp = c.gelu_clamp;
            return launch_gemm_kq(W.type, g, s);
        }
        kq_args k;
        k.w = W.w; k.row_bytes = W.rb; k.rows = W.rows; k.nsb = (int)(W.K / 256);
        k.x = img; k.x_col_stride = ldk; k.y = y; k.y_col_stride = ldy; k.ncols = T;
        k.tiled = W.tiled;
        k.resid = resid; k.gate_in = gate_in; k.gelu_tab = e->gelu_tab; k.gelu_clamp = c.gelu_clamp;
        if (up) k.w2 = up->w;
        return launch_matvec_kq(W.type, k, s);
    };
    if (launch_embed_q6K(e->embd_q6k, e->embd_row_bytes, rows.tokens, nullptr, T, (int)E, sqrtf((float)E), p.X, s, e->embd_tiled)) return -1;
    for (int il = 0; il < c.n_layer; ++il) {
        const layer_dev &L = e->layers[il];
        const kq_layer &K = e->kql[il];
        if (launch_norm_q8K(p.X, E, L.attn_norm, (int)E, c.eps, T, img, ldk, s) || expand(E)) return -1;
        const int64_t ldqkv = e->qkv_rows;
        if (K.qk_fused) {
            kq_mat qk = K.q;
            qk.rows = K.q.rows + K.k.rows;
            if (mv(qk, p.QKV, ldqkv, nullptr, nullptr, nullptr)) return -1;
        } else if (mv(K.q, p.QKV, ldqkv, nullptr, nullptr, nullptr) ||
                   mv(K.k, p.QKV + e->qw, ldqkv, nullptr, nullptr, nullptr)) {
            return -1;
        }
        if (mv(K.v, p.QKV + e->qw + e->kvw, ldqkv, nullptr, nullptr, nullptr)) return -1;
        if (prefill_attention(e, il, T, rows, true, &mx_form)) return -1;
        if (launch_quant_q8_K(p.ATT, e->qw, e->qw, T, img, ldk, s) || expand(e->qw)) return -1;
        if (mv(K.o, p.SA, E, p.X, nullptr, nullptr)) return -1;  // + inpL
        if (launch_norm_q8K(p.SA, E, L.ffn_norm, (int)E, c.eps, T, img, ldk, s) || expand(E)) return -1;
        if (K.gate.type == K.up.type && K.gate.rows == K.up.rows && K.gate.K == K.up.K && e->kq_dual &&
            !(mfma_ok(K.gate) && mfma_ok(K.up))) {
            if (mv(K.gate, p.U, F, nullptr, nullptr, &K.up)) return -1;  // gelu(gate)*up
        } else if (mv(K.gate, p.G, F, nullptr, nullptr, nullptr) || mv(K.up, p.U, F, nullptr, p.G, nullptr)) {
            return -1;
        }
        if (launch_quant_q8_K(p.U, F, F, T, img, ldk, s) || expand(F)) return -1;
        if (mv(K.down, p.X, E, p.SA, nullptr, nullptr)) return -1;  // + sa
    }
    return 0;
}

int enqueue_verify_pass(gemma_engine *e, int T, int p0) {
    if (T < 1 || T > GEMM_SKINNY_MAX_T) {
        set_error("gemma_engine_verify: a pass of " + std::to_string(T) + " rows");
        return -1;
    }
    if (prefill_alloc(e, GEMM_SKINNY_MAX_T)) return -1;  // sized once: no reallocation between passes
    return enqueue_prefill(e, T, own_rows(e, p0), true, nullptr, pass_end{true, true});
}

int batch_scratch_alloc(gemma_engine *e, int rows) {
    e->bt.pf = {};
    return scratch_alloc(e, e->bt_mem, e->bt.pf, std::max(rows, GEMM_SKINNY_MAX_T), rows > GEMM_SKINNY_MAX_T);
}

// a pass over rows [r0, r0 + T) of the batch pass bp: tokens bp.tok, the attention step by
// enqueue_batch_attention, the logits rows left in the scratch; the caller picks from every row and
// advances the slots.  skinny: the verify pass's GEMMs (T <= 8); else the exact MFMA GEMMs, any T
int enqueue_batch_pass(gemma_engine *e, const batch_pass &bp, int r0, int T, bool skinny) {
    if (T < 1 || r0 < 0 || r0 + T > e->bt.pf.T || (skinny && T > GEMM_SKINNY_MAX_T)) {
        set_error("gemma_engine_batch_step: a pass of " + std::to_string(T) + " rows from row " + std::to_string(r0) +
                  ", or no batch scratch");
        return -1;
    }
    return enqueue_prefill(e, T, pass_rows{bp.tok + r0, 0, &bp, r0}, true, nullptr, pass_end{true, skinny});
}

// one pass over rows [p0, p0+T) and its results: the last row's logits, all rows' [T][n_vocab], the
// greedy token of the last row; the engine is left at position p0 + T
static int prefill_pass(gemma_engine *e, int T, int p0, bool exact, float *logits_last, float *logits_all) {
    const gemma_hip_config &c = e->cfg;
    if (prefill_alloc(e, T)) return -1;
    if (enqueue_prefill(e, T, own_rows(e, p0), exact)) return -1;
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    if (logits_last)
        GHIP_CHECK(hipMemcpy(logits_last, e->pf.LG + (size_t)(T - 1) * c.n_vocab, (size_t)c.n_vocab * 4,
                             hipMemcpyDeviceToHost));
    if (logits_all) GHIP_CHECK(hipMemcpy(logits_all, e->pf.LG, (size_t)T * c.n_vocab * 4, hipMemcpyDeviceToHost));
    int tok = -1;
    GHIP_CHECK(hipMemcpy(&tok, e->seq.token, 4, hipMemcpyDeviceToHost));
    e->seq.host_pos = p0 + T;
    return tok;
}

// Batched prefill of the prompt given to gemma_engine_begin: all prompt
// positions in one pass, KV cache filled, logits for every row as the reference computes them
// (src/gemma_model.cpp:740); returns the greedy token and leaves the engine at position T, ready
// for gemma_engine_step.  exact: ggml-lane-order GEMMs + per-row decode-arithmetic attention,
// bit-identical to the CPU path; otherwise int8 MFMA GEMMs + f16 MFMA attention, which differ from
// it in fp32 summation order.
static int prefill_run(gemma_engine *e, bool exact, float *logits_last, float *logits_all) {
    (void)hipSetDevice(e->device);
    const int T = e->seq.n_given;
    if (T <= 0 || e->seq.host_pos != 0) {
        set_error("gemma_engine_prefill: call right after gemma_engine_begin");
        return -1;
    }
    if (e->tp_n > 1 || e->comm) {
        set_error("gemma_engine_prefill: the MFMA prefill is single-GPU (row-split engines prefill token by token)");
        return -1;
    }
    return prefill_pass(e, T, 0, exact, logits_last, logits_all);
}

extern "C" int gemma_engine_prefill(gemma_engine *e, float *logits_last, float *logits_all) {
    set_error("");
    return prefill_run(e, true, logits_last, logits_all);
}

extern "C" int gemma_engine_prefill_fast(gemma_engine *e, float *logits_last, float *logits_all) {
    set_error("");
    return prefill_run(e, false, logits_last, logits_all);
}

// One batched pass over the next n given tokens, positions [pos, pos+n), against the caches of
// [0, pos): enqueue_prefill with the row offset p0 = pos.  The given tokens are hist[.. n_prompt)
// (gemma_engine_begin / gemma_engine_extend); steps and earlier passes may have consumed some.
extern "C" int gemma_engine_prefill_next(gemma_engine *e, int n, int exact, float *logits_last, float *logits_all) {
    set_error("");
    (void)hipSetDevice(e->device);
    const int p0 = e->seq.host_pos, left = e->seq.n_given - p0;
    if (e->tp_n > 1 || e->comm) {
        set_error("gemma_engine_prefill_next: the batched prefill is single-GPU (row-split engines prefill token by token)");
        return -1;
    }
    if (left <= 0) {
        set_error("gemma_engine_prefill_next: no given token is pending (gemma_engine_begin / gemma_engine_extend supply them)");
        return -1;
    }
    if (n < 0 || n > left) {
        set_error("gemma_engine_prefill_next: n = " + std::to_string(n) + " with " + std::to_string(left) + " given tokens pending");
        return -1;
    }
    if (!exact && e->kq) {
        set_error("gemma_engine_prefill_next: K-quant layer engines have the exact batched prefill only");
        return -1;
    }
    return prefill_pass(e, n ? n : left, p0, exact != 0, logits_last, logits_all);
}

// diagnostics: the prefill (exact or MFMA) with the residual stream after every layer copied to host_taps
// [n_layer][T][n_embd] (compare with the oracle's per-layer hidden states)
extern "C" int gemma_engine_prefill_taps(gemma_engine *e, float *host_taps, int exact) {
    set_error("");
    (void)hipSetDevice(e->device);
    const gemma_hip_config &c = e->cfg;
    const int T = e->seq.n_given;
    if (T <= 0 || e->seq.host_pos != 0) {
        set_error("gemma_engine_prefill_taps: call right after gemma_engine_begin");
        return -1;
    }
    if (prefill_alloc(e, T)) return -1;
    dev_pool tmp;
    float *d = nullptr;
    const size_t n = (size_t)c.n_layer * T * c.n_embd;
    if (tmp.get(&d, n * 4)) return -1;
    int r = enqueue_prefill(e, T, own_rows(e, 0), exact != 0, d);
    if (r == 0) GHIP_CHECK(hipStreamSynchronize(e->stream));
    if (r == 0) GHIP_CHECK(hipMemcpy(host_taps, d, n * 4, hipMemcpyDeviceToHost));
    if (r == 0) e->seq.host_pos = T;
    return r;
}

// ---- the ggml executor's fast path (engine_ext.h; gemma_engine_create_ext: engine.cpp) -----------
// the device state a decode step reads: hist[pos] = token, *pos, the RoPE row of pos (k_advance
// publishes it between steps of a device-fed sequence; here the host feeds every token)
static int ext_set_position(gemma_engine *e, int token, int pos) {
    // n_fixed past the history: k_advance must not overwrite hist (the host supplies every token)
    return launch_set_position(token, pos, e->seq.pos, e->seq.hist, e->seq.nfix, e->cfg.n_ctx + 1, rope_of(e), e->stream);
}

int gemma_engine_ext_decode(gemma_engine *e, int token, int pos, float *logits) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    if (pos < 0 || pos + 1 >= c.n_ctx || token < 0 || token >= c.n_vocab) {
        set_error("gemma_engine_ext_decode: token or position out of range");
        return -1;
    }
    const bool prof = ghip_debug_level() >= 2;  // GHIP_GGML_DEBUG=2: per-step host phases to stderr
    auto us = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = prof ? us() : 0.0;
    (void)hipSetDevice(e->device);
    if (ext_set_position(e, token, pos)) return -1;
    if (!e->graph_exec) {  // first step eager (sets the kernels' LDS attributes), then capture
        if (enqueue_step(e)) return -1;
        if (ensure_graph(e)) return -1;
    } else {
        GHIP_CHECK(hipGraphLaunch(e->graph_exec, e->stream));
    }
    if (prof) GHIP_CHECK(hipStreamSynchronize(e->stream));
    const double t1 = prof ? us() : 0.0;
    // logits through a pinned staging row (a pageable device-to-host copy stages through the driver);
    // with the persistent launch its sticky timeout word rides along, so ONE sync covers both
    const size_t lb = (size_t)c.n_vocab * 4;
    const bool pchk = persist_on(e) && e->tok_err;
    auto copy_out = [&]() -> int {
        if (pchk) {
            if (!e->ext_err && e->mem.get(&e->ext_err, 16, MEM_PINNED)) return -1;
            GHIP_CHECK(hipMemcpyAsync(e->ext_err, e->tok_err, 12, hipMemcpyDeviceToHost, e->stream));
        }
        if (!e->ext_stage && e->mem.get(&e->ext_stage, lb, MEM_PINNED)) return -1;
        GHIP_CHECK(hipMemcpyAsync(e->ext_stage, e->logits, lb, hipMemcpyDeviceToHost, e->stream));
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        return 0;
    };
    if (copy_out()) return -1;
    if (pchk && persist_report(e, e->ext_err)) {  // a hand-off timeout: redo the token on the per-layer launches
        fprintf(stderr, "[gemma_hip] %s; token at position %d redone\n", last_error().c_str(), pos);
        set_error("");
        if (ext_set_position(e, token, pos) || enqueue_step(e)) return -1;
        if (copy_out()) return -1;
    }
    const double t2 = prof ? us() : 0.0;
    memcpy(logits, e->ext_stage, lb);
    if (prof) fprintf(stderr, "[gemma_hip] ext_decode: launch+run %.1f us, copy %.1f us, host copy %.1f us\n", t1 - t0, t2 - t1, us() - t2);
    e->seq.host_pos = pos + 1;
    return 0;
}

int gemma_engine_ext_prefill(gemma_engine *e, const int32_t *tokens, int T, float *logits_all) {
    if (T <= 0 || T >= e->cfg.n_ctx) {
        set_error("gemma_engine_ext_prefill: prompt length out of range");
        return -1;
    }
    if (!token_ids_ok(e, tokens, T, "gemma_engine_ext_prefill", false)) return -1;
    if (!e->graph_exec) {
        // the decode step's first launches (code-object loading, LDS attributes) and its graph
        // capture happen here, in the prompt's call, instead of in the first generated token: one
        // eager step at position 0, whose cache row the prefill below rewrites (begin clears it)
        (void)hipSetDevice(e->device);
        if (ext_set_position(e, tokens[0], 0) || enqueue_step(e) || ensure_graph(e)) return -1;
        GHIP_CHECK(hipGraphLaunch(e->graph_exec, e->stream));  // the graph's first launch uploads it
        if (!e->ext_stage && e->mem.get(&e->ext_stage, (size_t)e->cfg.n_vocab * 4, MEM_PINNED)) return -1;
        GHIP_CHECK(hipMemcpyAsync(e->ext_stage, e->logits, (size_t)e->cfg.n_vocab * 4, hipMemcpyDeviceToHost, e->stream));
        GHIP_CHECK(hipStreamSynchronize(e->stream));
    }
    if (gemma_engine_begin(e, tokens, T)) return -1;
    std::vector<float> last(e->cfg.n_vocab);
    if (gemma_engine_prefill(e, last.data(), logits_all) < 0) return -1;
    // measured: the first pinned-row copy after the prompt's large pageable copy takes ~10 ms; pay
    // it here rather than in the first generated token
    GHIP_CHECK(hipMemcpyAsync(e->ext_stage, e->logits, (size_t)e->cfg.n_vocab * 4, hipMemcpyDeviceToHost, e->stream));
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    return 0;
}
