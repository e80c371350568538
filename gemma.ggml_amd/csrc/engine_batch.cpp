// engine_batch.cpp — batched decode on the device-resident engine (DESIGN.md §5b⁗): up to 8
// (batch_open) or 64 (batch_open_wide) independent sequences (slots), each with its own caches,
// history and position, advanced one token per weight pass.  A pass has one row per active slot:
// tokens from the batch's row-token array, the attention by k_attn_slots, the picks followed by
// k_batch_advance.  Up to 8 rows it is the verify pass (engine_prefill.cpp, the skinny GEMMs); more
// rows run as one pass on the exact MFMA GEMMs of the batched prefill (R >= bt_mfma_min), else as
// groups of up to 8 rows on the skinny GEMM.  Every slot's logits and tokens are what
// gemma_engine_step gives that sequence alone, bit for bit, in every form.  All slot state lives in
// bt_mem and advances on the device; the engine's own sequence, its captured decode graph and its
// buffers are not touched.
#include "engine_impl.h"

static constexpr int NS = GEMMA_BATCH_WIDE_MAX_SLOTS;  // every table's size
static constexpr int NARROW = GEMMA_BATCH_MAX_SLOTS;
static_assert(GEMMA_BATCH_MAX_SLOTS == GEMM_SKINNY_MAX_T, "a narrow pass has one skinny-GEMM column per slot");
// the batch is open and `slot` one of its slots, else the error (naming fn) is set
static bool slot_ok(const gemma_engine *e, int slot, const char *fn) {
    if (!e->bt.open) {
        set_error(std::string(fn) + ": no batch is open (gemma_engine_batch_open)");
        return false;
    }
    if (slot < 0 || slot >= e->bt.n_slots) {
        set_error(std::string(fn) + ": slot " + std::to_string(slot) + " outside [0, " + std::to_string(e->bt.n_slots) + ")");
        return false;
    }
    return true;
}

static void batch_drop(gemma_engine *e) {
    e->bt_mem.clear();
    e->bt = batch_state{};
}

// gemma_engine_batch_open (max_slots 8) and gemma_engine_batch_open_wide (64): the same open
static int batch_open(gemma_engine *e, int n_slots, int max_slots, const std::string &fn) {
    set_error("");
    if (e->bt.open) {
        set_error(fn + ": a batch is already open (gemma_engine_batch_close)");
        return -1;
    }
    if (n_slots < 1 || n_slots > max_slots) {
        set_error(fn + ": n_slots = " + std::to_string(n_slots) + " outside [1, " + std::to_string(max_slots) + "]");
        return -1;
    }
    if (row_split(e)) {
        set_error(fn + ": single-GPU engines only (row-split engines decode one sequence)");
        return -1;
    }
    if (e->att_mode != ATTN_PER_HEAD) {
        set_error(fn + ": the batch runs the per-head decode attention (n_ctx <= 2048, head_dim <= 256)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    dev_pool &M = e->bt_mem;
    batch_state &b = e->bt;
    b = batch_state{};
    bool bad = batch_scratch_alloc(e, n_slots) != 0 || M.get_zeroed(&b.last, NS * 4, s);
    for (int i = 0; i < n_slots && !bad; ++i) bad = seq_alloc(e, M, b.slot[i], true, b.last + i) != 0;
    bad = bad || M.get_zeroed(&b.rows, NS * sizeof(slot_row), s) || M.get_zeroed(&b.row_tok, NS * 4, s) ||
          pick_buf_alloc(M, b.picks, s) || M.get(&b.stage, NS * sizeof(slot_row), MEM_PINNED) ||
          // more rows than the engine's sampler has workspaces: the batch brings its own, one per slot
          (n_slots > NARROW && sample_ws_alloc(M, &b.picks.ws, e->cfg.n_vocab, s, n_slots));
    if (!bad) {  // no slot is active: every pending token reads -1
        int *h = (int *)b.stage;
        for (int i = 0; i < NS; ++i) h[i] = -1;
        bad = hipMemcpyAsync(b.last, h, NS * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
              hipStreamSynchronize(s) != hipSuccess;
        if (bad) set_error("initialising the slot state failed");
    }
    if (bad) {
        const std::string why = last_error();
        batch_drop(e);
        set_error(fn + ": " + why);
        return -1;
    }
    b.picks.lp_parts = b.pf.LP;  // more rows than the engine's partials hold: the scratch's own (else null)
    b.n_slots = n_slots;
    b.open = true;
    return 0;
}

extern "C" int gemma_engine_batch_open(gemma_engine *e, int n_slots) {
    return batch_open(e, n_slots, NARROW, "gemma_engine_batch_open");
}

extern "C" int gemma_engine_batch_open_wide(gemma_engine *e, int n_slots) {
    return batch_open(e, n_slots, NS, "gemma_engine_batch_open_wide");
}

extern "C" int gemma_engine_batch_close(gemma_engine *e) {
    set_error("");
    if (!e->bt.open) {
        set_error("gemma_engine_batch_close: no batch is open");
        return -1;
    }
    (void)hipSetDevice(e->device);
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    batch_drop(e);
    return 0;
}

extern "C" int gemma_engine_batch_begin(gemma_engine *e, int slot, const int32_t *tokens, int n) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    if (!slot_ok(e, slot, "gemma_engine_batch_begin")) return -1;
    if (n <= 0 || n >= c.n_ctx || !tokens) {
        set_error("gemma_engine_batch_begin: prompt length out of range");
        return -1;
    }
    if (!token_ids_ok(e, tokens, n, "gemma_engine_batch_begin")) return -1;
    (void)hipSetDevice(e->device);
    batch_state &b = e->bt;
    seq_state &S = b.slot[slot];
    // the slot's token word is its pending token, hist[0]; neither the decode step's argmax keys nor
    // the epoch belong to a slot
    GHIP_CHECK(hipMemcpyAsync(S.token, tokens, 4, hipMemcpyHostToDevice, e->stream));
    if (seq_begin(e, S, tokens, n)) return -1;
    S.active = true;
    b.dirty = true;
    return 0;
}

extern "C" int gemma_engine_batch_adopt(gemma_engine *e, int slot) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_adopt")) return -1;
    if (e->seq.n_given <= 0) {
        set_error("gemma_engine_batch_adopt: the engine has no sequence (gemma_engine_begin)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    batch_state &b = e->bt;
    if (seq_copy(e, b.slot[slot], e->seq)) return -1;
    b.slot[slot].active = true;
    b.dirty = true;
    return 0;
}

extern "C" int gemma_engine_batch_release(gemma_engine *e, int slot) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_release")) return -1;
    (void)hipSetDevice(e->device);
    batch_state &b = e->bt;
    static const int none = -1;
    GHIP_CHECK(hipMemcpyAsync(b.slot[slot].token, &none, 4, hipMemcpyHostToDevice, e->stream));
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    b.slot[slot].active = false;
    b.dirty = true;
    return 0;
}

// the row -> slot table of the active set (ascending slot order) and the rows' first tokens
static int batch_write_rows(gemma_engine *e) {
    batch_state &b = e->bt;
    hipStream_t s = e->stream;
    slot_row *h = (slot_row *)b.stage;
    int R = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        if (!b.slot[i].active) continue;
        slot_row r;
        r.qkv = b.pf.QKV + (size_t)R * e->qkv_rows;
        r.out = b.pf.ATT + (size_t)R * e->qw;
        const seq_state &S = b.slot[i];
        r.kc = S.kc; r.vc = S.vc; r.rope = S.rope;
        r.hist = S.hist; r.pos = S.pos; r.nfix = S.nfix; r.last = S.token; r.lp = S.lp;
        h[R] = r;
        b.row_slot[R] = i;
        GHIP_CHECK(hipMemcpyAsync(b.row_tok + R, S.token, 4, hipMemcpyDeviceToDevice, s));  // = hist[pos]
        ++R;
    }
    if (R) GHIP_CHECK(hipMemcpyAsync(b.rows, h, (size_t)R * sizeof(slot_row), hipMemcpyHostToDevice, s));
    b.n_rows = R;
    b.dirty = false;
    return 0;
}

int enqueue_batch_attention(gemma_engine *e, int il, int r0, int T) {
    attn_args t = attn_of(e, il);
    t.dsplit = e->att_dsplit;
    return launch_attn_slots(t, e->bt.rows + r0, T, (int64_t)il * e->cfg.n_ctx * e->kvw, e->stream);
}

extern "C" int gemma_engine_batch_step(gemma_engine *e, int n, float *logits) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    batch_state &b = e->bt;
    if (!b.open) {
        set_error("gemma_engine_batch_step: no batch is open (gemma_engine_batch_open)");
        return -1;
    }
    int R = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        if (!b.slot[i].active) continue;
        ++R;
        if ((int64_t)b.slot[i].host_pos + n >= c.n_ctx) {
            set_error("gemma_engine_batch_step: context full (slot " + std::to_string(i) + " at position " +
                      std::to_string(b.slot[i].host_pos) + ", n = " + std::to_string(n) + ", n_ctx = " + std::to_string(c.n_ctx) + ")");
            return -1;
        }
    }
    if (R == 0) {
        set_error("gemma_engine_batch_step: no slot is active (gemma_engine_batch_begin / _adopt)");
        return -1;
    }
    if (n <= 0) return 0;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    if (b.dirty && batch_write_rows(e)) return -1;
    // the form of the call's passes: up to 8 rows the skinny pass; more rows one pass on the MFMA
    // GEMMs from bt_mfma_min rows, else consecutive groups of up to 8 rows, each a skinny pass over its
    // own rows of the scratch.  The tokens, the row table and the pick keys are indexed by the global row
    const bool mfma = R > NARROW && R >= e->bt_mfma_min;
    for (int i = 0; i < n; ++i) {
        if (R <= NARROW || mfma) {
            if (enqueue_batch_pass(e, 0, R, !mfma)) return -1;
        } else {
            for (int r0 = 0; r0 < R; r0 += NARROW)
                if (enqueue_batch_pass(e, r0, std::min(NARROW, R - r0), true)) return -1;
        }
        // a pick from every row: row r gives the token of its slot's sequence index pos + 1 (the
        // sampler reads the slot's position word through the row table)
        row_picks pk;
        if (enqueue_row_picks(e, b.pf.LG, R, nullptr, b.rows, b.picks, &pk)) return -1;
        if (logits)
            GHIP_CHECK(hipMemcpyAsync(logits + (size_t)i * R * c.n_vocab, b.pf.LG, (size_t)R * c.n_vocab * 4, hipMemcpyDeviceToHost, s));
        if (launch_batch_advance(b.rows, R, pk.keys, pk.n_parts, pk.stride, b.row_tok, c.n_ctx, rope_of(e), s)) return -1;
        if (enqueue_lp_finish(e, b.pf.LG, R, b.picks.lp_parts, nullptr, b.rows, nullptr)) return -1;
    }
    GHIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < b.n_slots; ++i)
        if (b.slot[i].active) b.slot[i].host_pos += n;
    return 0;
}

extern "C" int gemma_engine_batch_pos(gemma_engine *e, int slot) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_pos")) return -1;
    if (!e->bt.slot[slot].active) {
        set_error("gemma_engine_batch_pos: slot " + std::to_string(slot) + " is not active");
        return -1;
    }
    return e->bt.slot[slot].host_pos;
}

extern "C" int gemma_engine_batch_tokens(gemma_engine *e, int slot, int32_t *out, int cap) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_tokens")) return -1;
    const seq_state &S = e->bt.slot[slot];
    if (!S.active || !out || cap < 0) {
        set_error("gemma_engine_batch_tokens: slot " + std::to_string(slot) + " is not active, or a null / negative buffer");
        return -1;
    }
    (void)hipSetDevice(e->device);
    return seq_tokens(S, out, cap);
}

extern "C" int gemma_engine_batch_last(gemma_engine *e, int32_t *out8) {
    set_error("");
    if (!e->bt.open || !out8) {
        set_error("gemma_engine_batch_last: no batch is open, or a null buffer");
        return -1;
    }
    if (e->bt.n_slots > NARROW) {
        set_error("gemma_engine_batch_last: the batch has " + std::to_string(e->bt.n_slots) +
                  " slots; it serves up to 8 (gemma_engine_batch_last_n)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    int *h = (int *)e->bt.stage;
    GHIP_CHECK(hipMemcpyAsync(h, e->bt.last, NARROW * 4, hipMemcpyDeviceToHost, e->stream));
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    memcpy(out8, h, NARROW * 4);
    return 0;
}

extern "C" int gemma_engine_batch_last_n(gemma_engine *e, int32_t *out, int cap) {
    set_error("");
    if (!e->bt.open || !out) {
        set_error("gemma_engine_batch_last_n: no batch is open, or a null buffer");
        return -1;
    }
    const int ns = e->bt.n_slots;
    if (cap < ns) {
        set_error("gemma_engine_batch_last_n: cap = " + std::to_string(cap) + " below the batch's " + std::to_string(ns) + " slots");
        return -1;
    }
    (void)hipSetDevice(e->device);
    int *h = (int *)e->bt.stage;
    GHIP_CHECK(hipMemcpyAsync(h, e->bt.last, (size_t)ns * 4, hipMemcpyDeviceToHost, e->stream));
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    memcpy(out, h, (size_t)ns * 4);
    return ns;
}

extern "C" int gemma_engine_batch_kv_read(gemma_engine *e, int slot, int layer, int p0, int n, uint16_t *k_rows,
                                          uint16_t *v_rows) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_kv_read")) return -1;
    return seq_kv_read(e, e->bt.slot[slot], layer, p0, n, k_rows, v_rows, "gemma_engine_batch_kv_read");
}

extern "C" int gemma_engine_batch_logprobs(gemma_engine *e, int slot, int p0, int n, double *out) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_logprobs")) return -1;
    if (!e->bt.slot[slot].active) {
        set_error("gemma_engine_batch_logprobs: slot " + std::to_string(slot) + " is not active");
        return -1;
    }
    return seq_logprobs(e, e->bt.slot[slot], p0, n, out, "gemma_engine_batch_logprobs");
}
