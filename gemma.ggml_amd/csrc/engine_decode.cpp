// engine_decode.cpp — one decode token of the device-resident engine: the launches enqueue_step
// puts on the engine stream (captured once in a hipGraph and replayed), the K-quant step, the
// persistent launch's arguments and reports, and the row-split all-gathers.
// It computes exactly the graph src/gemma_model.cpp:665-747 builds, op for op (see the per-kernel
// citations in kernels.h / matvec.hip / ops.hip), with the fusions listed in DESIGN.md §Kernels.
#include "engine_impl.h"

// the inbox of a gathered working vector in every rank's p2p arena
static int64_t p2p_inbox(const gemma_engine *e, const void *work) {
    if (work == e->qkv) return e->ib_qkv;
    if (work == e->sa) return e->ib_sa;
    if (work == e->h) return e->ib_h;
    if (work == e->x) return e->ib_x;
    if (work == e->h_act) return e->ib_hact;
    if (work == e->h_da) return e->ib_hda;
    if (work == e->logits) return e->ib_logits;
    if (work == e->rank_keys) return e->ib_keys;
    return -1;
}

// one peer-to-peer gather of up to two segments (working vector, bytes per rank)
static int p2p_gather(gemma_engine *e, void *w0, int64_t b0, void *w1 = nullptr, int64_t b1 = 0, hipStream_t s = nullptr) {
    p2p_args a;
    a.nseg = w1 ? 2 : 1;
    a.seg[0].work = (uint8_t *)w0; a.seg[0].inbox = p2p_inbox(e, w0); a.seg[0].shard = b0;
    if (w1) { a.seg[1].work = (uint8_t *)w1; a.seg[1].inbox = p2p_inbox(e, w1); a.seg[1].shard = b1; }
    if (a.seg[0].inbox < 0 || (w1 && a.seg[1].inbox < 0)) {
        set_error("p2p_gather: not a gathered vector");
        return -1;
    }
    a.rank = e->tp_rank; a.n = e->tp_n;
    for (int r = 0; r < e->tp_n; ++r) a.peer[r] = e->p2p_peer[r];
    a.flags = e->ib_flags; a.seq = e->p2p_seq; a.err = e->p2p_err;
    return launch_p2p_gather(a, s ? s : e->stream);
}

// in-place all-gather of a full vector whose rank-r shard [r*cnt, (r+1)*cnt) was just written
int tp_gather(gemma_engine *e, float *full, int64_t cnt) {
    if (e->p2p) return p2p_gather(e, full, cnt * 4);
    if (!e->comm) return 0;  // one unsplit engine, or virtual ranks (shards already in place)
    const ncclResult_t r = ncclAllGather(full + (size_t)e->tp_rank * cnt, full, (size_t)cnt, ncclFloat, e->comm, e->stream);
    if (r != ncclSuccess) {
        set_error(std::string("ncclAllGather: ") + ncclGetErrorString(r));
        return -1;
    }
    return 0;
}

// in-place all-gather of the h image: per rank `act_bytes` of act (u32 groups) and `nda` scales
static int tp_gather_bytes(gemma_engine *e, uint32_t *act, int64_t act_bytes, float *da, int64_t nda) {
    if (e->p2p) return p2p_gather(e, act, act_bytes, da, nda * 4);
    if (!e->comm) return 0;
    ncclGroupStart();
    ncclResult_t r = ncclAllGather((uint8_t *)act + (size_t)e->tp_rank * act_bytes, act, (size_t)act_bytes, ncclUint8,
                                   e->comm, e->stream);
    const ncclResult_t r2 = ncclAllGather(da + (size_t)e->tp_rank * nda, da, (size_t)nda, ncclFloat, e->comm, e->stream);
    const ncclResult_t r3 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r == ncclSuccess) r = r3;
    if (r != ncclSuccess) {
        set_error(std::string("ncclAllGather(image): ") + ncclGetErrorString(r));
        return -1;
    }
    return 0;
}

// the persistent token launch's arguments and per-layer table (device copies the kernel reads);
// sets persist_why to the reason when the launch cannot run this engine
int tok_prepare(gemma_engine *e) {
    const gemma_hip_config &c = e->cfg;
    e->persist_why.clear();
    if (e->kq) e->persist_why = "K-quant layers";
    else if (e->out_type == T_Q6_K) e->persist_why = "Q6_K token_embd (the launch dequantizes the layer type)";
    else if (row_split(e)) e->persist_why = "row-split TP";
    if (!e->persist_why.empty() || !e->tok_gran) {
        if (e->persist_why.empty()) e->persist_why = "no buffers";
        return 0;
    }
    std::vector<tok_layer> tab(c.n_layer);
    for (int il = 0; il < c.n_layer; ++il) {
        const layer_dev &L = e->layers[il];
        tok_layer &T = tab[il];
        T.qkv_qs = L.qkv.qs; T.qkv_sc = L.qkv.sc; T.o_qs = L.o.qs; T.o_sc = L.o.sc;
        T.g_qs = L.gate.qs; T.g_sc = L.gate.sc; T.u_qs = L.up.qs; T.u_sc = L.up.sc; T.d_qs = L.down.qs; T.d_sc = L.down.sc;
        T.attn_norm = L.attn_norm; T.ffn_norm = L.ffn_norm;
        T.kc = kc_of(e, e->seq, il); T.vc = vc_of(e, e->seq, il);
    }
    GHIP_CHECK(hipMemcpy(e->tok_tab, tab.data(), tab.size() * sizeof(tok_layer), hipMemcpyHostToDevice));
    tok_args &a = e->tok;
    a = tok_args{};
    a.layers = e->tok_tab;
    a.n_layer = c.n_layer;
    a.E = c.n_embd; a.F = c.n_ff; a.H = c.n_head; a.Hkv = c.n_head_kv; a.hd = c.head_dim; a.ctx = c.n_ctx;
    a.qkv_rows = e->qkv_rows;
    a.att_split = e->att_dsplit;
    a.eps = c.eps; a.emb_scale = sqrtf((float)c.n_embd); a.q_scale = 1.0f / sqrtf((float)c.head_dim);
    a.emb_qs = e->embd.qs; a.emb_sc = e->embd.sc; a.emb_n_bt = e->embd.n_bt;
    a.hist = e->seq.hist; a.pos = e->seq.pos; a.rope_cur = e->seq.rope;
    a.exp_tab = e->exp_tab; a.gelu_tab = e->gelu_tab; a.gelu_clamp = c.gelu_clamp;
    const tok_gran_sizes g = token_gran_sizes(c.n_embd, c.n_ff, e->qkv_rows);
    unsigned long long *p = e->tok_gran;
    a.gx = p; p += g.gx;
    a.gqkv = p; p += g.gqkv;
    a.gatt = p; p += g.gatt;
    a.gatt_da = p; p += g.gatt_da;
    a.gsa = p; p += g.gsa;
    a.gh = p; p += g.gh;
    a.gh_da = p;
    a.epoch = e->epoch; a.x_out = e->x; a.att_out = e->attn; a.err = e->tok_err;
    a.timeout = e->persist_timeout;
    e->persist_why = token_unsupported(c.wtype, a);
    GHIP_CHECK(hipMemcpy(e->tok_dev, &a, sizeof(tok_args), hipMemcpyHostToDevice));
    return 0;
}

// After a stream sync that covers persistent-launch steps: a hand-off that timed out (a workgroup
// not co-resident, the CUs shared with another stream or process) leaves the sticky word set and the
// step's numbers wrong.  Report it, clear it and fall back to the per-layer launches for later steps
// (ADVICE r3); returns 1 when a timeout was seen.
// w = the persistent launch's sticky words [flag, site, layer] read back after the step
int persist_report(gemma_engine *e, const int *w) {
    if (!w[0]) return 0;
    (void)hipMemset(e->tok_err, 0, 64);
    e->persist = 0;
    drop_graph(e);
    set_error("persistent token launch: hand-off timeout (site " + std::to_string(w[1]) + ", layer " +
              std::to_string(w[2]) + "): the step's logits and KV rows are invalid; the engine now runs the "
              "per-layer launches");
    return 1;
}

// After a stream sync that covers k_attn_o launches: a hand-off poll that timed out leaves the sticky
// word set and the step's numbers wrong.  Report it, clear it and run the two launches from then on.
int att_o_check(gemma_engine *e) {
    if (!e->att_o || !e->ao_err) return 0;
    int w[5] = {0, 0, 0, 0, 0};
    if (hipMemcpy(w, e->ao_err, 20, hipMemcpyDeviceToHost) != hipSuccess || !w[0]) return 0;
    (void)hipMemset(e->ao_err, 0, 64);
    (void)hipMemset(e->ao_cnt, 0, (size_t)e->cfg.n_layer * 16 * 32 * 4);
    e->att_o = 0;
    drop_graph(e);
    set_error("attention + attn-out launch: hand-off timeout (counter " + std::to_string(w[2]) + " of " +
              std::to_string(w[3]) + "): the step's logits and KV rows are invalid; the engine now runs the two "
              "launches");
    return 1;
}

int persist_check(gemma_engine *e) {
    if (!persist_on(e) || !e->tok_err) return 0;
    int w[3] = {0, 0, 0};
    if (hipMemcpy(w, e->tok_err, 12, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return persist_report(e, w);
}

int enqueue_logits_q6k(gemma_engine *e, const uint8_t *x, int ncols, float *y) {
    const gemma_hip_config &c = e->cfg;
    kq_args k;
    k.w = e->embd_q6k; k.tiled = e->embd_tiled; k.row_bytes = e->embd_row_bytes; k.rows = c.n_vocab; k.nsb = c.n_embd / 256;
    k.x = x; k.x_col_stride = (c.n_embd / 256) * 292; k.y = y; k.y_col_stride = c.n_vocab; k.ncols = ncols;
    return launch_matvec_kq(T_Q6_K, k, e->stream);
}

// The one place a token is picked.  Sampling off: k_advance reduces the greedy argmax keys, launch
// for launch as before.  Sampling on: the sampler's three launches on the logits row, then the
// unchanged k_advance on its one key (the p >= n_fixed guard, the RoPE row and the epoch bump stay).
// enqueue_pick_keys is the pick without the advance (the verify pass picks every row, then advances
// once over the accepted prefix).
int enqueue_pick_keys(gemma_engine *e, const float *row, const int *pos, const unsigned long long **keys, int *n_parts) {
    if (!e->sampling) return 0;
    const sample_ws &w = e->smp_ws;
    if (launch_sample(row, 0, 1, e->cfg.n_vocab, e->smp_dev, pos, nullptr, w, sample_dbg{}, e->stream)) return -1;
    *keys = w.key;
    *n_parts = 1;
    return 0;
}

int enqueue_pick(gemma_engine *e, const float *row, const unsigned long long *keys, int n_parts, const float *rows0, int R,
                 lse_part *own) {
    if (!rows0) { rows0 = row; R = 1; }
    if (enqueue_lp_parts(e, rows0, R, own)) return -1;
    if (enqueue_pick_keys(e, row, e->seq.pos, &keys, &n_parts)) return -1;
    if (launch_advance(keys, n_parts, e->seq.token, e->seq.pos, e->seq.hist, e->cfg.n_ctx, e->seq.nfix, rope_of(e), e->stream)) return -1;
    return enqueue_lp_finish(e, rows0, R, own, &e->seq, nullptr, nullptr);
}

// The log-probabilities of a pass's rows (logprob.hip): the partials need the rows only and go right
// behind the logits launch; the finish reads the token the advance settled.  Off: nothing is launched.
static lse_part *lp_parts_of(gemma_engine *e, int R, lse_part *own) {
    if (own) return own;
    if (R <= GEMM_SKINNY_MAX_T && e->lp_parts) return e->lp_parts;
    set_error("logprobs: no partials for a pass of " + std::to_string(R) + " rows");
    return nullptr;
}

int enqueue_lp_parts(gemma_engine *e, const float *LG, int R, lse_part *own) {
    if (!e->logprobs) return 0;
    lse_part *parts = lp_parts_of(e, R, own);
    return parts ? launch_lse_parts(LG, e->cfg.n_vocab, R, e->cfg.n_vocab, parts, e->stream) : -1;
}

int enqueue_lp_finish(gemma_engine *e, const float *LG, int R, lse_part *own, const seq_state *S, const slot_row *tab,
                      const int *acc) {
    if (!e->logprobs) return 0;
    lse_finish_args a;
    a.lg = LG; a.ld = e->cfg.n_vocab; a.n = e->cfg.n_vocab; a.R = R; a.G = lse_grid(e->cfg.n_vocab); a.n_ctx = e->cfg.n_ctx;
    a.parts = lp_parts_of(e, R, own);
    if (!a.parts) return -1;
    a.tab = tab; a.acc = acc;
    if (S) { a.pos = S->pos; a.hist = S->hist; a.lp = S->lp; }
    return launch_lse_finish(a, e->stream);
}

// The picks of a pass's T rows, none advancing: the verify pass then accepts a prefix, the batch pass
// advances every row's slot.  The launch count does not depend on T: one row-argmax launch (greedy),
// the sampler's three (sampling), or both (a batch pass whose slots differ), each with the row in grid.y.
int pick_buf_alloc(dev_pool &M, pick_buf &b, hipStream_t s) {
    return M.get_zeroed(&b.keys, (size_t)(PICK_MAX_ROWS * 256 + PICK_MAX_ROWS) * 8, s);
}

// mix: which of the pass's rows sample (PICKS_*: none, all, some), decided by the caller from its host
// mirror of each participating slot's mode; -1: by the engine's sampler, the same for every row.  A
// mixed pass keeps the greedy key layout: a sampling row's tail overwrites its partial keys.
int enqueue_row_picks(gemma_engine *e, const float *LG, int T, const int *pos, const slot_row *tab, const pick_buf &b,
                      row_picks *out, int mix) {
    const int64_t V = e->cfg.n_vocab;
    if (T < 1 || T > PICK_MAX_ROWS) {
        set_error("row picks: a pass of " + std::to_string(T) + " rows");
        return -1;
    }
    if (mix < 0) mix = e->sampling ? PICKS_SAMPLE : PICKS_GREEDY;
    if (enqueue_lp_parts(e, LG, T, b.lp_parts)) return -1;  // (the caller's advance is followed by enqueue_lp_finish)
    // every sampling row in its own workspace: the buffer's own (a wide batch's, or a narrow batch's on
    // an engine that has none), else the engine's 8
    const sample_ws &w = b.ws.hist ? b.ws : e->smp_ws;
    return launch_picks(mix, LG, V, T, V, e->smp_dev, pos, tab, w, b.keys, PICK_MAX_ROWS, sample_dbg{}, e->stream, &out->keys,
                        &out->n_parts, &out->stride);
}

// the decode tail of a Q6_K tied output: rms_norm*out_norm -> Q8_K (have_img: the last down handed
// that image over) -> logits -> row argmax -> token feedback, position += 1
static int step_tail_q6k(gemma_engine *e, bool have_img) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    const int E = c.n_embd;
    if (!have_img && launch_norm_q8K(e->x, E, e->out_norm, E, c.eps, 1, e->xq8k, (E / 256) * 292, s)) return -1;
    if (enqueue_logits_q6k(e, e->xq8k, 1, e->logits)) return -1;
    if (!e->sampling && launch_row_argmax(e->logits, c.n_vocab, e->key, 256, s)) return -1;
    return enqueue_pick(e, e->logits, e->key, 256);
}

// One decode token with K-quant layer matrices (src/gemma_model.cpp:665-747 on a Q4_K_M file):
// per layer rms_norm*attn_norm -> Q8_K -> Wq, Wk, Wv (K-quant dots) -> attention (the same kernel)
// -> Q8_K(attn) -> Wo (+inpL) -> rms_norm*ffn_norm -> Q8_K -> Wgate, Wup (gelu(gate)*up epilogue)
// -> Q8_K(h) -> Wdown (+sa); then the Q6_K tied output.  ggml's INIT and vec_dot order throughout.
static int enqueue_step_kq(gemma_engine *e) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    const int E = c.n_embd;
    // Where ggml's Q8_K INIT of each matvec input runs (all write the same bytes):
    //   LAUNCH   a k_norm_q8K / k_quant_q8_K launch;
    //   PROLOGUE the consumer's prologue from f32 (KQP_NORM / KQP_F32, every workgroup);
    //   HANDOFF  the producer's tail (kq_handoff; attention: each head's super-block).
    // Images: A = attn-norm(x) -> q|k, v; B = attention out -> o; C = ffn-norm(sa) -> gate/up;
    // D = gelu(gate)*up -> down; each in its own buffer.  e->kq_fuse picks the plan:
    //   0 all LAUNCH; 1 all PROLOGUE; 2 all HANDOFF (measured: the norm tails cost more than a
    //   launch); 3 norms PROLOGUE, quantizations HANDOFF; 4 as 3 with C a LAUNCH; 5 (default) all
    //   PROLOGUE but D (the attention then keeps two workgroups per head); 6 as 5 with B a LAUNCH.
    //   Same box, Q4_K_M decode: plan 3 / 5 / 6 -> 997 / 1,017 / 980 tok/s.
    enum { LAUNCH, PROLOGUE, HANDOFF };
    static const int plan[7][4] = {{LAUNCH, LAUNCH, LAUNCH, LAUNCH},
                                   {PROLOGUE, PROLOGUE, PROLOGUE, PROLOGUE},
                                   {HANDOFF, HANDOFF, HANDOFF, HANDOFF},
                                   {PROLOGUE, HANDOFF, PROLOGUE, HANDOFF},
                                   {PROLOGUE, HANDOFF, LAUNCH, HANDOFF},
                                   {PROLOGUE, PROLOGUE, PROLOGUE, HANDOFF},
                                   {PROLOGUE, LAUNCH, PROLOGUE, HANDOFF}};
    const int mode = e->kq_fuse >= 0 && e->kq_fuse <= 6 ? e->kq_fuse : 5;
    int srcA = plan[mode][0], srcB = plan[mode][1], srcC = plan[mode][2], srcD = plan[mode][3];
    if (E > 2048) {  // the norm hand-off holds <= 2048 values in one wave
        if (srcA == HANDOFF) srcA = PROLOGUE;
        if (srcC == HANDOFF) srcC = PROLOGUE;
    }
    if (srcB == HANDOFF && !(e->att_mode == ATTN_PER_HEAD && c.head_dim == 256)) srcB = LAUNCH;
    struct img {
        int src;
        uint8_t *x;  // the Q8_K image (LAUNCH / HANDOFF)
        int pro;     // PROLOGUE: mode and f32 input
        const float *xf, *norm_w;
    };
    struct out {
        int mode = KQO_NONE;  // a HANDOFF this launch writes
        uint8_t *q8 = nullptr;
        const float *norm = nullptr;
    };
    unsigned long long *mv_dbg = nullptr;  // stamps build: the launch's phase stamps (tests/stamp_step.py KQ=1)
    auto args = [&](const kq_mat &W, float *y, const float *resid, const float *gate_in, const img &in, const out &o,
                    const kq_mat *up) {
        kq_args k;
        k.dbg_t = mv_dbg;
        k.w = W.w; k.row_bytes = W.rb; k.rows = W.rows; k.nsb = (int)(W.K / 256);
        k.x = in.x; k.x_col_stride = (W.K / 256) * 292; k.y = y; k.y_col_stride = W.rows; k.ncols = 1;
        k.tiled = W.tiled;
        k.resid = resid; k.gate_in = gate_in; k.gelu_tab = e->gelu_tab; k.gelu_clamp = c.gelu_clamp;
        k.eps = c.eps;
        if (in.src == PROLOGUE) {
            k.pro = in.pro; k.xf = in.xf; k.xf_col_stride = W.K; k.norm_w = in.norm_w;
        }
        if (o.mode != KQO_NONE) {
            k.q8_mode = o.mode; k.q8_out = o.q8; k.q8_norm = o.norm; k.q8_cnt = e->kq_cnt; k.q8_cnt_cap = e->kq_cnt_cap;
            k.q8_abl = e->kq_abl;
        }
        if (up) k.w2 = up->w;
        return k;
    };
    auto mv = [&](const kq_mat &W, float *y, const float *resid, const float *gate_in, const img &in, const out &o,
                  const kq_mat *up) { return launch_matvec_kq(W.type, args(W, y, resid, gate_in, in, o, up), s); };
    auto launch_img = [&](const img &in, int K) {
        if (in.src != LAUNCH) return 0;
        if (in.norm_w) return launch_norm_q8K(in.xf, K, in.norm_w, K, c.eps, 1, in.x, (K / 256) * 292, s);
        return launch_quant_q8_K(in.xf, K, K, 1, in.x, (K / 256) * 292, s);
    };
    if (launch_embed_q6K(e->embd_q6k, e->embd_row_bytes, e->seq.hist, e->seq.pos, 1, E, sqrtf((float)E), e->x, s, e->embd_tiled)) return -1;
    for (int il = 0; il < c.n_layer; ++il) {
        const layer_dev &L = e->layers[il];
        const kq_layer &K = e->kql[il];
        // layer 0's image A has no producing down: a launch when the plan hands it off
        const img in_a{srcA == HANDOFF && il == 0 ? LAUNCH : srcA, e->kq_x, KQP_NORM, e->x, L.attn_norm};
        if (launch_img(in_a, E)) return -1;
        const bool pair = e->kq_pair && K.qk_fused && E % 2048 == 0 && E <= 4096 && K.q.tiled == K.v.tiled &&
                          (K.q.rows + K.k.rows) % 8 == 0;
        if (pair) {  // q|k and v (their own types) in one launch
            kq_mat qk = K.q;
            qk.rows = K.q.rows + K.k.rows;
            if (launch_matvec_kq2(qk.type, args(qk, e->qkv, nullptr, nullptr, in_a, out{}, nullptr), K.v.type,
                                  args(K.v, e->qkv + e->qw + e->kvw, nullptr, nullptr, in_a, out{}, nullptr), s))
                return -1;
        } else {
            if (K.qk_fused) {  // q|k in one allocation (same type): one launch for both
                kq_mat qk = K.q;
                qk.rows = K.q.rows + K.k.rows;
                if (mv(qk, e->qkv, nullptr, nullptr, in_a, out{}, nullptr)) return -1;
            } else if (mv(K.q, e->qkv, nullptr, nullptr, in_a, out{}, nullptr) ||
                       mv(K.k, e->qkv + e->qw, nullptr, nullptr, in_a, out{}, nullptr)) {
                return -1;
            }
            if (mv(K.v, e->qkv + e->qw + e->kvw, nullptr, nullptr, in_a, out{}, nullptr)) return -1;
        }
        attn_args t = attn_of(e, il);
        if (srcB == HANDOFF) t.out_q8k = e->kq_xa;  // each head's 256 outputs are one super-block
        else if (t.mode == ATTN_PER_HEAD) t.dsplit = e->att_dsplit;
        t.dbg_t = stamp_region(e, il, 1);  // diagnostics (stamps build): the attention's phases
        if (launch_attn_decode(t, s)) return -1;
        const img in_b{srcB, e->kq_xa, KQP_F32, e->attn, nullptr};
        if (launch_img(in_b, e->qw)) return -1;
        out o_c;
        if (srcC == HANDOFF) {
            o_c.mode = KQO_NORM; o_c.q8 = e->kq_xf; o_c.norm = L.ffn_norm;
        }
        mv_dbg = stamp_region(e, il, 2);
        if (mv(K.o, e->sa, e->x, nullptr, in_b, o_c, nullptr)) return -1;  // + inpL (:723)
        mv_dbg = nullptr;
        const img in_c{srcC, e->kq_xf, KQP_NORM, e->sa, L.ffn_norm};
        if (launch_img(in_c, E)) return -1;
        out o_d;
        if (srcD == HANDOFF) {
            o_d.mode = KQO_QUANT; o_d.q8 = e->kq_xh;
        }
        if (K.gate.type == K.up.type && K.gate.rows == K.up.rows && K.gate.K == K.up.K && e->kq_dual) {
            // gate and up in one launch, gelu(gate)*up in registers (:446-449)
            mv_dbg = stamp_region(e, il, 3);
            if (mv(K.gate, e->h, nullptr, nullptr, in_c, o_d, &K.up)) return -1;
            mv_dbg = nullptr;
        } else if (mv(K.gate, e->kq_g, nullptr, nullptr, in_c, out{}, nullptr) ||
                   mv(K.up, e->h, nullptr, e->kq_g, in_c, o_d, nullptr)) {
            return -1;
        }
        const img in_d{srcD, e->kq_xh, KQP_F32, e->h, nullptr};
        if (launch_img(in_d, c.n_ff)) return -1;
        // down (+ sa, :731); under a HANDOFF plan for A it writes the next layer's image A (or the
        // output norm's)
        out o_a;
        if (srcA == HANDOFF) {
            o_a.mode = KQO_NORM;
            o_a.q8 = il + 1 < c.n_layer ? e->kq_x : e->xq8k;
            o_a.norm = il + 1 < c.n_layer ? e->layers[il + 1].attn_norm : e->out_norm;
        }
        if (mv(K.down, e->x, e->sa, nullptr, in_d, o_a, nullptr)) return -1;
    }
    // the tied output's INIT: handed over by the last down, else its own launch (256k rows over
    // thousands of workgroups would each redo the norm in a prologue)
    return step_tail_q6k(e, srcA == HANDOFF);
}

// ---- the tiled (Q4_0 / Q8_0) step, stage by stage ------------------------------------------------
// the two debug taps that follow every form of a layer's front: q|k|v and the attention output
static int tap_front(gemma_engine *e, int il) {
    if (!e->dbg) return 0;
    float *tap = e->dbg + (size_t)il * (e->qkv_rows + e->qw + e->cfg.n_embd);
    GHIP_CHECK(hipMemcpyAsync(tap, e->qkv, (size_t)e->qkv_rows * 4, hipMemcpyDeviceToDevice, e->stream));
    GHIP_CHECK(hipMemcpyAsync(tap + e->qkv_rows, e->attn, (size_t)e->qw * 4, hipMemcpyDeviceToDevice, e->stream));
    return 0;
}

// attn-out (+ residual) for the rows from r0 on: quantize(attn) -> Wo, + inpL  (:493, :723); img:
// from the Q8_0 image the attention wrote instead of its f32 output
static mv_args attn_out_of(gemma_engine *e, const layer_dev &L, size_t r0, bool img) {
    mv_args b;
    set_mat(b, L.o);
    b.x = e->attn; b.y = e->sa + r0; b.resid = e->x + r0;
    if (img) { b.x = e->att_act; b.x_da = e->att_da; }
    return b;
}
static bool att_img_on(const gemma_engine *e) { return e->att_act && att_img_ok(e) && e->plan[MC_O].img; }
static bool front_on(const gemma_engine *e) {
    return e->front_cnt && e->fuse_front && !row_split(e) && e->att_mode == ATTN_PER_HEAD && e->att_act && e->plan[MC_QKV].ks == KS_RR &&
           e->plan[MC_O].ks == KS_RR && e->plan[MC_O].img;
}

// fused front (layers > 0, or a Q6_K embedding that ran before layer 0): one launch for K1 + K2 +
// K3 below, same arithmetic (layer_front.hip).  Returns 0 done, 1 not applicable, -1 error.
static int step_front_fused(gemma_engine *e, int il) {
    if (!front_on(e) || (il == 0 && e->out_type != T_Q6_K)) return 1;
    const gemma_hip_config &c = e->cfg;
    const layer_dev &L = e->layers[il];
    front_args f;
    set_mat(f.q, L.qkv);
    f.q.norm_w = L.attn_norm; f.q.eps = c.eps; f.q.x = e->x; f.q.y = e->qkv;
    f.t = attn_of(e, il);
    f.t.out_act = e->att_act; f.t.out_da = e->att_da;
    f.o = attn_out_of(e, L, 0, true);
    f.cnt = e->front_cnt + (size_t)il * 16 * 32;  // 16 counters of 128 B
    f.err = e->front_err;
    f.dbg_t = stamp_region(e, il, 0);
    if (!layer_front_supported(c.wtype, f.q, f.t, f.o)) return 1;
    if (launch_layer_front(c.wtype, f, e->stream)) return -1;
    return tap_front(e, il);
}

// K1: [embed | rms_norm*attn_norm] + quantize -> Wq|Wk|Wv   (:677-696); each rank its rows
static int step_qkv(gemma_engine *e, int il) {
    const gemma_hip_config &c = e->cfg;
    const int wt = c.wtype;
    for (int vr = 0; vr < (e->rep_attn ? 1 : e->n_virtual); ++vr) {
        layer_dev &L = layer_of(e, il, vr);
        mv_args a;
        set_mat(a, L.qkv);
        a.norm_w = L.attn_norm; a.eps = c.eps;
        int pro = PRO_NORM;
        if (il == 0 && e->out_type != T_Q6_K) {
            pro = PRO_EMBED;
            a.x = e->seq.hist; a.tok_pos = e->seq.pos;
            a.emb_qs = e->embd.qs; a.emb_sc = e->embd.sc; a.emb_n_bt = e->embd.n_bt;
            a.emb_scale = sqrtf((float)c.n_embd);
            a.emb_out = e->x;
        } else {
            a.x = e->x;
        }
        a.dbg_t = stamp_region(e, il, 0);
        a.y = e->qkv + (e->rep_attn ? 0 : (size_t)rank_of(e, vr) * e->sh_qkv);  // this rank's rows of q|k|v
        if (launch_matvec(wt, pick_ks(wt, L.qkv.n_bt, e->plan[MC_QKV].ks), pro, EPI_STORE, a, mv_grid(e, MC_QKV, L.qkv.n_rt),
                          e->stream))
            return -1;
    }
    if (!e->rep_attn && tp_gather(e, e->qkv, e->sh_qkv)) return -1;
    return 0;
}

// K2: rope + scale + kv store + KQ + softmax + KQV  (:698-718, :454-518); replicated.  Tries
// attention + attn-out in one launch first (k_attn_o: the attention's idle workgroups run attn-out).
// Returns 1 when that ran (K3 is done), 0 when K3 is still to run, -1 on error.
static int step_attention(gemma_engine *e, int il) {
    const int wt = e->cfg.wtype;
    hipStream_t s = e->stream;
    attn_args t = attn_of(e, il);
    const bool att_img = att_img_on(e);
    if (att_img) { t.out_act = e->att_act; t.out_da = e->att_da; }
    t.dbg_t = stamp_region(e, il, 1);
    if (t.mode == ATTN_PER_HEAD) t.dsplit = e->att_dsplit;
    if (e->att_o && att_img && e->n_virtual == 1 && e->ao_cnt && e->plan[MC_O].ks == KS_RR) {
        attn_o_args f;
        f.t = t;
        f.o = attn_out_of(e, layer_of(e, il, 0), e->rep_attn ? 0 : (size_t)rank_of(e, 0) * e->sh_o, true);
        f.cnt = e->ao_cnt + (size_t)il * 16 * 32;
        f.err = e->ao_err;
        f.t.dbg_t = nullptr;  // (the fused kernel's stamps: 16 per workgroup in the attention region)
        f.dbg_t = stamp_region(e, il, 1);
        if (attn_o_supported(wt, f.t, f.o)) {
            if (launch_attn_o(wt, f, s) || tap_front(e, il)) return -1;
            if (!e->rep_attn && tp_gather(e, e->sa, e->sh_o)) return -1;
            return 1;
        }
    }
    if (launch_attn_decode(t, s) || tap_front(e, il)) return -1;
    return 0;
}

// K3: attn-out on its own launch; each rank its rows
static int step_attn_out(gemma_engine *e, int il) {
    const int wt = e->cfg.wtype;
    const bool att_img = att_img_on(e);
    for (int vr = 0; vr < (e->rep_attn ? 1 : e->n_virtual); ++vr) {
        layer_dev &L = layer_of(e, il, vr);
        mv_args b = attn_out_of(e, L, e->rep_attn ? 0 : (size_t)rank_of(e, vr) * e->sh_o, att_img);
        b.dbg_t = stamp_region(e, il, 2);
        if (launch_matvec(wt, pick_ks(wt, L.o.n_bt, e->plan[MC_O].ks), att_img ? PRO_IMG : PRO_F32, EPI_ADD, b,
                          mv_grid(e, MC_O, L.o.n_rt), e->stream))
            return -1;
    }
    if (!e->rep_attn && tp_gather(e, e->sa, e->sh_o)) return -1;
    return 0;
}

// K4: rms_norm*ffn_norm + quantize -> gate & up -> gelu(gate)*up  (:724, :446-449)
// K5: quantize(h) -> Wdown, + sa  (:450, :731)
static int step_ffn(gemma_engine *e, int il) {
    const gemma_hip_config &c = e->cfg;
    const int wt = c.wtype;
    hipStream_t s = e->stream;
    const bool h_img = e->h_act && e->plan[MC_DOWN].img;
    for (int vr = 0; vr < e->n_virtual; ++vr) {
        layer_dev &L = layer_of(e, il, vr);
        mv_args g;
        set_mat(g, L.gate);
        g.qs2 = L.up.qs; g.sc2 = L.up.sc;
        g.x = e->sa; g.norm_w = L.ffn_norm; g.eps = c.eps; g.y = e->h + (size_t)rank_of(e, vr) * e->sh_ff;
        g.gelu_tab = e->gelu_tab; g.gelu_clamp = c.gelu_clamp;
        if (h_img) {  // this rank's blocks of the image (shard offsets are whole 4-block groups)
            const size_t b0 = (size_t)rank_of(e, vr) * e->sh_ff / 32;
            g.out_act = e->h_act + b0 * 8;
            g.out_da = e->h_da + b0;
        }
        g.dbg_t = stamp_region(e, il, 3);
        if (launch_matvec(wt, e->plan[MC_GU].ks, PRO_NORM, EPI_GELU_MUL, g, mv_grid(e, MC_GU, L.gate.n_rt), s))
            return -1;
    }
    if (h_img) {
        if (tp_gather_bytes(e, e->h_act, e->sh_ff, e->h_da, e->sh_ff / 32)) return -1;
    } else if (tp_gather(e, e->h, e->sh_ff)) {
        return -1;
    }
    for (int vr = 0; vr < e->n_virtual; ++vr) {
        layer_dev &L = layer_of(e, il, vr);
        const size_t r0 = (size_t)rank_of(e, vr) * e->sh_e;
        mv_args d;
        set_mat(d, L.down);
        d.x = e->h; d.y = e->x + r0; d.resid = e->sa + r0;
        if (h_img) { d.x = e->h_act; d.x_da = e->h_da; }
        d.dbg_t = stamp_region(e, il, 4);
        if (launch_matvec(wt, pick_ks(wt, L.down.n_bt, e->plan[MC_DOWN].ks), h_img ? PRO_IMG : PRO_F32, EPI_ADD, d,
                          mv_grid(e, MC_DOWN, L.down.n_rt), s))
            return -1;
    }
    if (tp_gather(e, e->x, e->sh_e)) return -1;
    if (e->dbg)
        GHIP_CHECK(hipMemcpyAsync(e->dbg + (size_t)il * (e->qkv_rows + e->qw + c.n_embd) + e->qkv_rows + e->qw, e->x,
                                  (size_t)c.n_embd * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// K6: rms_norm*output_norm + quantize -> tied output -> logits + argmax  (:736-740, :532-546)
// K7: token feedback (greedy_sample -> input.push_back, :282-285), position += 1; the prompt is
// never overwritten: hist writes only land at positions >= n_prompt
static int step_logits(gemma_engine *e) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    if (e->out_type == T_Q6_K) return step_tail_q6k(e, false);
    const rope_row rr = rope_of(e);
    int lg_grid = 0;
    for (int vr = 0; vr < e->n_virtual; ++vr) {
        const int rk = rank_of(e, vr);
        const tiled_mat out_rows = sub_rows(e->embd, (int64_t)rk * e->sh_v, e->sh_v);  // tied output, this rank's vocab
        mv_args o;
        set_mat(o, out_rows);
        o.x = e->x; o.norm_w = e->out_norm; o.eps = c.eps; o.y = e->logits + (size_t)rk * e->sh_v;
        o.argmax_key = e->key;
        lg_grid = mv_grid(e, MC_LOGITS, out_rows.n_rt);
        o.dbg_t = e->stamp ? e->stamp + 5 * kStampRegion : nullptr;
        if (launch_matvec(c.wtype, 1, PRO_NORM, EPI_ARGMAX, o, lg_grid, s)) return -1;
        // TP: one key per rank, its index made global
        if (e->tp_n_keys && launch_reduce_keys(e->key, lg_grid, (int64_t)rk * e->sh_v, e->rank_keys + rk, s)) return -1;
    }
    if (!e->tp_n_keys) return enqueue_pick(e, e->logits, e->key, lg_grid);
    if (e->p2p && p2p_gather(e, e->rank_keys, 8, nullptr, 0, s)) return -1;
    if (e->comm) {
        const ncclResult_t nr = ncclAllGather(e->rank_keys + e->tp_rank, e->rank_keys, 1, ncclUint64, e->comm, s);
        if (nr != ncclSuccess) {
            set_error(std::string("ncclAllGather(keys): ") + ncclGetErrorString(nr));
            return -1;
        }
    }
    return launch_advance(e->rank_keys, e->tp_n, e->seq.token, e->seq.pos, e->seq.hist, c.n_ctx, e->seq.nfix, rr, s);
}

// One decode token: the embedding (a Q6_K token_embd; else layer 0's qkv prologue), the layers as
// one persistent launch (token.hip) or stage by stage, then the logits, argmax and token feedback.
int enqueue_step(gemma_engine *e) {
    const gemma_hip_config &c = e->cfg;
    hipStream_t s = e->stream;
    if (e->kq) return enqueue_step_kq(e);
    if (e->out_type == T_Q6_K &&
        launch_embed_q6K(e->embd_q6k, e->embd_row_bytes, e->seq.hist, e->seq.pos, 1, c.n_embd, sqrtf((float)c.n_embd), e->x, s,
                         e->embd_tiled))
        return -1;
    if (persist_on(e)) {
        if (launch_token(c.wtype, e->tok, e->tok_dev, s)) return -1;
        return step_logits(e);
    }
    if (front_on(e)) GHIP_CHECK(hipMemsetAsync(e->front_cnt, 0, (size_t)c.n_layer * 16 * 32 * 4, s));
    for (int il = 0; il < c.n_layer; ++il) {
        const int front = step_front_fused(e, il);
        if (front < 0) return -1;
        if (front == 1) {  // its own launches: K1, K2 (+ K3 inside it when k_attn_o runs), K3
            if (step_qkv(e, il)) return -1;
            const int att = step_attention(e, il);
            if (att < 0 || (att == 0 && step_attn_out(e, il))) return -1;
        }
        if (step_ffn(e, il)) return -1;
    }
    return step_logits(e);
}
