// engine_spec.cpp — speculative decoding on the device-resident engine (DESIGN.md §5b‴): the exact
// multi-token verify pass, the cache read-back its tests use, prompt-lookup drafts and the generate
// loop that alternates verify passes and plain graph steps.
#include "engine_impl.h"

// the verify buffers: made at the first call and kept for the engine's lifetime (never regrown)
static int verify_alloc(gemma_engine *e) {
    auto &v = e->vf;
    dev_pool &M = e->mem;
    if ((!v.picks.keys && pick_buf_alloc(M, v.picks, e->stream)) ||
        (!v.ints && M.get(&v.ints, (size_t)(GEMM_SKINNY_MAX_T + GEMM_SKINNY_MAX_T + 1) * 4)) ||
        (!v.host && M.get(&v.host, (size_t)(3 * GEMM_SKINNY_MAX_T + 1) * 4, MEM_PINNED)))
        return -1;
    return 0;
}

// One batched exact pass over [pending token, k drafts] at p0 = pos, a pick from every row, the
// accept rule and the advance over the accepted prefix on the device, the rejected rows' K / V
// cleared: afterwards the device state is what a + 1 calls of gemma_engine_step leave.
extern "C" int gemma_engine_verify(gemma_engine *e, const int32_t *draft, int k, int32_t *out_tokens, float *logits_all) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    const int p0 = e->seq.host_pos;
    if (row_split(e)) {
        set_error("gemma_engine_verify: single-GPU engines only (row-split engines decode token by token)");
        return -1;
    }
    if (p0 < e->seq.n_given || p0 < 1) {
        set_error("gemma_engine_verify: " + std::to_string(std::max(e->seq.n_given - p0, 0)) +
                  " given tokens are still pending (the drafts follow the pending picked token)");
        return -1;
    }
    if (k < 1 || k > GEMMA_VERIFY_MAX_DRAFT || !draft || !out_tokens) {
        set_error("gemma_engine_verify: k = " + std::to_string(k) + " outside [1, " + std::to_string(GEMMA_VERIFY_MAX_DRAFT) +
                  "], or a null draft / out_tokens");
        return -1;
    }
    if (!token_ids_ok(e, draft, k, "gemma_engine_verify")) return -1;
    if ((int64_t)p0 + k + 1 >= c.n_ctx) {
        set_error("gemma_engine_verify: pos + k + 1 = " + std::to_string((int64_t)p0 + k + 1) + " does not fit n_ctx = " +
                  std::to_string(c.n_ctx));
        return -1;
    }
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    if (verify_alloc(e)) return -1;
    const int T = k + 1;
    int *h_draft = e->vf.host, *h_pos = e->vf.host + GEMM_SKINNY_MAX_T, *h_out = e->vf.host + 2 * GEMM_SKINNY_MAX_T;
    int *d_pos = e->vf.ints, *d_out = e->vf.ints + GEMM_SKINNY_MAX_T;
    for (int i = 0; i < k; ++i) h_draft[i] = draft[i];
    for (int i = 0; i < T; ++i) h_pos[i] = p0 + i;
    // 1. stage: the drafts become hist[pos+1 .. pos+k], the tokens of the pass's rows 1 .. k
    GHIP_CHECK(hipMemcpyAsync(e->seq.hist + p0 + 1, h_draft, (size_t)k * 4, hipMemcpyHostToDevice, s));
    // 2. the pass
    if (enqueue_verify_pass(e, T, p0)) return -1;
    // 3. a pick from every row, none advances: row i gives the token of sequence index pos + i + 1
    // (the sampler reads each row's position from the device: p0 + i)
    if (e->sampling) GHIP_CHECK(hipMemcpyAsync(d_pos, h_pos, (size_t)T * 4, hipMemcpyHostToDevice, s));
    row_picks pk;
    if (enqueue_row_picks(e, e->pf.LG, T, d_pos, nullptr, e->vf.picks, &pk)) return -1;
    // 4. accept + advance
    verify_args v;
    v.keys = pk.keys; v.n_parts = pk.n_parts; v.key_stride = pk.stride;
    v.k = k; v.p0 = p0; v.token = e->seq.token; v.pos = e->seq.pos; v.hist = e->seq.hist; v.r = rope_of(e);
    v.zero_keys = e->key; v.n_zero = e->grid_big; v.out = d_out;
    if (launch_verify_accept(v, s)) return -1;
    // (log-probabilities on: rows 0 .. a against the tokens the accept settled; rejected rows write nothing)
    if (enqueue_lp_finish(e, e->pf.LG, T, nullptr, &e->seq, nullptr, d_out)) return -1;
    // 5. the rejected rows leave the caches
    if (e->kc_ext.empty()) {
        if (launch_verify_clean(e->seq.kc, e->seq.vc, c.n_layer, (int64_t)c.n_ctx * e->kvw, c.n_ctx, e->kvw, p0, k, d_out, s)) return -1;
    } else {
        for (int il = 0; il < c.n_layer; ++il)
            if (launch_verify_clean(kc_of(e, e->seq, il), vc_of(e, e->seq, il), 1, 0, c.n_ctx, e->kvw, p0, k, d_out, s)) return -1;
    }
    // 6. results: one synchronise
    GHIP_CHECK(hipMemcpyAsync(h_out, d_out, (size_t)(T + 1) * 4, hipMemcpyDeviceToHost, s));
    if (logits_all) GHIP_CHECK(hipMemcpyAsync(logits_all, e->pf.LG, (size_t)T * c.n_vocab * 4, hipMemcpyDeviceToHost, s));
    GHIP_CHECK(hipStreamSynchronize(s));
    const int a = h_out[0];
    if (a < 0 || a > k) {
        set_error("gemma_engine_verify: the accept kernel reported " + std::to_string(a) + " accepted drafts");
        return -1;
    }
    for (int i = 0; i <= a; ++i) out_tokens[i] = h_out[1 + i];
    e->seq.host_pos = p0 + a + 1;
    return a + 1;
}

extern "C" int gemma_engine_kv_read(gemma_engine *e, int layer, int p0, int n, uint16_t *k_rows, uint16_t *v_rows) {
    set_error("");
    return seq_kv_read(e, e->seq, layer, p0, n, k_rows, v_rows, "gemma_engine_kv_read");
}

// Prompt-lookup draft: for g = min(ngram_max, n - 1) .. 1, the most recent earlier occurrence of the
// sequence's last g tokens (largest s < n - g with seq[s .. s+g) == seq[n-g .. n)); the first g with a
// match wins and the draft is what followed it, seq[s+g .. min(s+g+k, n)).  No GPU.
extern "C" int gemma_lookup_draft(const int32_t *seq, int n, int ngram_max, int k, int32_t *out) {
    if (!seq || !out || n < 1 || ngram_max < 1 || k < 1 || k > GEMMA_VERIFY_MAX_DRAFT) {
        set_error("gemma_lookup_draft: needs n >= 1, ngram_max >= 1 and 1 <= k <= " + std::to_string(GEMMA_VERIFY_MAX_DRAFT));
        return -1;
    }
    for (int g = std::min(ngram_max, n - 1); g >= 1; --g)
        for (int s = n - g - 1; s >= 0; --s)
            if (memcmp(seq + s, seq + n - g, (size_t)g * 4) == 0) {
                const int len = std::min(s + g + k, n) - (s + g);
                for (int i = 0; i < len; ++i) out[i] = seq[s + g + i];
                return len;
            }
    return 0;
}

// The draft of a generate loop, grown by repeated lookups: one lookup stops at the sequence end (in a
// repeating run the most recent match sits right before it and yields a single token), so what it
// drafted is appended to the mirror as a guess and the rule applied again, until kd_max tokens or no
// match.  seq: the mirror, n tokens of it the sequence (room for kd_max more); the guesses past n are
// overwritten by what the pass accepts.  Returns the draft's length.
static int grow_lookup_draft(int32_t *seq, int n, int ngram_max, int kd_max, int32_t *draft) {
    int kd = 0;
    while (kd < kd_max) {
        const int m = gemma_lookup_draft(seq, n + kd, ngram_max, kd_max - kd, draft + kd);
        if (m <= 0) break;
        for (int i = 0; i < m; ++i) seq[n + kd + i] = draft[kd + i];
        kd += m;
    }
    return kd;
}

extern "C" int gemma_engine_generate_lookup(gemma_engine *e, int n_new, int k, int ngram_max, int32_t *out,
                                            gemma_spec_stats *stats) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    gemma_spec_stats st{0, 0, 0, 0};
    if (n_new < 0 || (n_new > 0 && !out) || k < 1 || k > GEMMA_VERIFY_MAX_DRAFT || ngram_max < 1) {
        set_error("gemma_engine_generate_lookup: needs n_new >= 0, 1 <= k <= " + std::to_string(GEMMA_VERIFY_MAX_DRAFT) +
                  " and ngram_max >= 1");
        return -1;
    }
    if (e->seq.host_pos < e->seq.n_given || e->seq.host_pos < 1) {
        set_error("gemma_engine_generate_lookup: given tokens are still pending (consume the prompt first)");
        return -1;
    }
    if ((int64_t)e->seq.host_pos + n_new >= c.n_ctx) {
        set_error("gemma_engine_generate_lookup: context full");
        return -1;
    }
    std::vector<int32_t> seq((size_t)c.n_ctx + 1);
    int n = gemma_engine_tokens(e, seq.data(), c.n_ctx + 1);  // the sequence so far, the pending token included
    if (n != e->seq.host_pos + 1) return -1;
    int done = 0;
    int32_t draft[GEMMA_VERIFY_MAX_DRAFT], got[GEMMA_VERIFY_MAX_DRAFT + 1];
    while (done < n_new) {
        // a pass over kd drafts appends up to kd + 1 tokens: never more than remain
        const int kd_max = std::min(k, n_new - done - 1);
        int kd = grow_lookup_draft(seq.data(), n, ngram_max, kd_max, draft);
        if (kd > 0 && (int64_t)e->seq.host_pos + kd + 1 >= c.n_ctx) kd = 0;
        if (kd > 0) {
            const int m = gemma_engine_verify(e, draft, kd, got, nullptr);
            if (m < 0) return -1;
            st.passes += 1; st.drafted += kd; st.accepted += m - 1;
            for (int i = 0; i < m; ++i) seq[n++] = out[done++] = got[i];
        } else {
            if (gemma_engine_step(e, 1, nullptr, 1)) return -1;
            int32_t tok = 0;
            GHIP_CHECK(hipMemcpy(&tok, e->seq.token, 4, hipMemcpyDeviceToHost));
            st.plain_steps += 1;
            seq[n++] = out[done++] = tok;
        }
    }
    if (stats) *stats = st;
    return 0;
}

// The same loop over the open batch's slots: per pass every unfinished slot drafts from its own mirror,
// one gemma_engine_batch_verify pass serves them all, finished slots sit out.
extern "C" int gemma_engine_batch_generate_lookup(gemma_engine *e, int n_new, int k, int ngram_max, int32_t *out,
                                                  gemma_spec_stats *stats) {
    set_error("");
    const std::string fn = "gemma_engine_batch_generate_lookup";
    const gemma_hip_config &c = e->cfg;
    batch_state &b = e->bt;
    constexpr int KD = GEMMA_VERIFY_MAX_DRAFT, NS = GEMMA_BATCH_WIDE_MAX_SLOTS;
    if (!b.open) {
        set_error(fn + ": no batch is open (gemma_engine_batch_open)");
        return -1;
    }
    if (n_new < 0 || (n_new > 0 && !out) || k < 1 || k > KD || ngram_max < 1) {
        set_error(fn + ": needs n_new >= 0, 1 <= k <= " + std::to_string(KD) + " and ngram_max >= 1");
        return -1;
    }
    int R = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        const seq_state &S = b.slot[i];
        if (!S.active) continue;
        ++R;
        if (S.host_pos < S.n_given || S.host_pos < 1) {
            set_error(fn + ": slot " + std::to_string(i) + " has given tokens still pending (consume the prompts first)");
            return -1;
        }
        if ((int64_t)S.host_pos + n_new >= c.n_ctx) {
            set_error(fn + ": context full (slot " + std::to_string(i) + ")");
            return -1;
        }
    }
    if (R == 0) {
        set_error(fn + ": no slot is active (gemma_engine_batch_begin / _adopt)");
        return -1;
    }
    // per active slot the sequence so far, the pending token included, and what it has appended
    const size_t ld = (size_t)c.n_ctx + 1;
    std::vector<int32_t> seq((size_t)b.n_slots * ld), draft((size_t)b.n_slots * KD), got((size_t)b.n_slots * (KD + 1));
    std::vector<gemma_spec_stats> st((size_t)b.n_slots, gemma_spec_stats{0, 0, 0, 0});
    int32_t n_of[NS] = {}, done[NS] = {}, k_of[NS], need[NS], rows_of[NS], n_out[NS];
    int left = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        if (!b.slot[i].active) continue;
        n_of[i] = gemma_engine_batch_tokens(e, i, seq.data() + i * ld, (int)ld);
        if (n_of[i] != b.slot[i].host_pos + 1) return -1;
        left += n_new > 0;
    }
    while (left > 0) {
        int T = 0;
        for (int i = 0; i < b.n_slots; ++i) {
            need[i] = 0;
            k_of[i] = -1;  // inactive and finished slots sit out
            if (!b.slot[i].active || done[i] >= n_new) continue;
            // a pass over kd drafts appends up to kd + 1 tokens: never more than remain
            int kd = grow_lookup_draft(seq.data() + i * ld, n_of[i], ngram_max, std::min(k, n_new - done[i] - 1),
                                       draft.data() + (size_t)i * KD);
            if (kd > 0 && (int64_t)b.slot[i].host_pos + kd + 1 >= c.n_ctx) kd = 0;
            k_of[i] = kd;
            need[i] = 1 + kd;
            T += need[i];
        }
        if (T > b.pf.T) {  // more rows than the batch holds: the drafts are cut by the one allotment rule
            if (gemma_batch_plan_rows(need, b.n_slots, b.pf.T, rows_of) < 0) {
                set_error(fn + ": " + last_error());
                return -1;
            }
            for (int i = 0; i < b.n_slots; ++i)
                if (need[i] > 0) k_of[i] = rows_of[i] - 1;
        }
        if (gemma_engine_batch_verify(e, draft.data(), k_of, got.data(), n_out, nullptr) < 0) {
            set_error(fn + ": " + last_error());
            return -1;
        }
        for (int i = 0; i < b.n_slots; ++i) {
            if (k_of[i] < 0) continue;
            const int m = n_out[i];
            if (k_of[i] > 0) {
                st[i].passes += 1; st[i].drafted += k_of[i]; st[i].accepted += m - 1;
            } else {
                st[i].plain_steps += 1;
            }
            for (int j = 0; j < m; ++j)
                seq[i * ld + n_of[i]++] = out[(size_t)i * n_new + done[i]++] = got[(size_t)i * (KD + 1) + j];
            left -= done[i] >= n_new;
        }
    }
    if (stats)
        for (int i = 0; i < b.n_slots; ++i) stats[i] = st[i];
    return 0;
}
