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
// gemma_engine_batch_step_rows gives a slot that still has given tokens to consume several rows of one
// pass (gemma_batch_plan_rows states the allotment): the same pass over a row table of its own, the
// attention step in two launches (K / V stores of all rows, then the attention from the cache), the
// advance per slot.  The slot's state afterwards is byte for byte what one-row passes leave.
// gemma_engine_batch_verify is gemma_engine_verify for the slots: such a pass whose rows past a slot's
// first process drafts, then per slot the accept rule, the advance over the accepted prefix and the
// rejected rows' K / V cleared, all on the device; a slot may sit the pass out.
// gemma_engine_batch_set_sampler gives a slot a sampler of its own (or its own greedy) beside slots that
// follow the engine's: every row reads its parameters from its row-table entry, and the picks of a pass take
// one, three or four launches by the mix of the participating slots; gemma_engine_batch_fork copies a slot.
//
// The three pass entries (batch_step, batch_step_rows, batch_verify) share everything but their per-slot
// tables and their advance.  Each describes its pass by a batch_pass {row table, row sources, tokens, T}
// and hands it to batch_run_pass, which alone decides the pass's form, enqueues it, picks from every
// row and copies the logits rows out; the descriptor travels as an argument down to
// enqueue_batch_attention, which alone chooses the attention kernels (by batch_pass::src).  A row-table
// entry is made in one place (batch_row), the tables of a pass with several rows per slot in one place
// (batch_build_rows: step_rows adds its slot_spans, batch_verify its bv_slots, both from the row0 and
// rank the builder returns).  After batch_run_pass an entry launches its own advance
// (launch_batch_advance / launch_rows_advance / launch_bverify_accept + _clean), then enqueue_lp_finish.
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

// A sampler per slot: the parameters the slot's rows carry (its own, else the engine's while that
// sampler is on, else greedy), and which launches a pass's picks take, from the host mirror of the
// participating slots' modes (n_sample of n_slots sample)
static sampler_params slot_params(const gemma_engine *e, int slot) {
    const batch_state &b = e->bt;
    sampler_params p;  // temperature 0: greedy
    if (b.smp_own[slot]) {
        const gemma_sampler &s = b.smp[slot];
        p.temperature = s.temperature; p.top_k = s.top_k; p.top_p = s.top_p; p.seed = s.seed;
    } else if (e->sampling) {
        p = e->smp_host;
    }
    return p;
}
static int picks_mix(int n_sample, int n_slots) {
    return n_sample == 0 ? PICKS_GREEDY : n_sample == n_slots ? PICKS_SAMPLE : PICKS_MIXED;
}

static void batch_drop(gemma_engine *e) {
    e->bt_mem.clear();
    e->bt = batch_state{};
}

// gemma_engine_batch_open (max_slots 8), gemma_engine_batch_open_wide (64) and
// gemma_engine_batch_open_rows (64, a row capacity of its own): the same open.  rows: what the pass
// scratch, the sampler workspaces and the log-probability partials are sized for (at least 8)
static int batch_open(gemma_engine *e, int n_slots, int max_slots, int rows, const std::string &fn) {
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
    const size_t rope_words = (size_t)e->cfg.head_dim + 4;
    const size_t mtab = NS * (sizeof(slot_row) + sizeof(row_src) + sizeof(slot_span));
    bool bad = batch_scratch_alloc(e, rows) != 0 || M.get_zeroed(&b.last, NS * 4, s);
    for (int i = 0; i < n_slots && !bad; ++i) bad = seq_alloc(e, M, b.slot[i], true, b.last + i) != 0;
    bad = bad || M.get_zeroed(&b.rows, NS * sizeof(slot_row), s) || M.get_zeroed(&b.row_tok, NS * 4, s) ||
          pick_buf_alloc(M, b.picks, s) || M.get(&b.stage, NS * sizeof(slot_row), MEM_PINNED) ||
          // more rows than the engine's sampler has workspaces: the batch brings its own, one per row
          (rows > NARROW && sample_ws_alloc(M, &b.picks.ws, e->cfg.n_vocab, s, rows)) ||
          // the tables of a pass with several rows per slot (gemma_engine_batch_step_rows)
          M.get_zeroed(&b.mrows, NS * sizeof(slot_row), s) || M.get_zeroed(&b.msrc, NS * sizeof(row_src), s) ||
          M.get_zeroed(&b.mspans, NS * sizeof(slot_span), s) || M.get_zeroed(&b.mrope, NS * rope_words * 4, s) ||
          M.get(&b.mstage, mtab, MEM_PINNED) ||
          // the tables of a pass with drafts (gemma_engine_batch_verify)
          M.get_zeroed(&b.vslots, NS * sizeof(bv_slot), s) || M.get_zeroed(&b.vout, NS * BV_OUT_WORDS * 4, s) ||
          M.get_zeroed(&b.vtok, NS * 4, s) || M.get(&b.vstage, NS * (sizeof(bv_slot) + BV_OUT_WORDS * 4), MEM_PINNED);
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
    return batch_open(e, n_slots, NARROW, n_slots, "gemma_engine_batch_open");
}

extern "C" int gemma_engine_batch_open_wide(gemma_engine *e, int n_slots) {
    return batch_open(e, n_slots, NS, n_slots, "gemma_engine_batch_open_wide");
}

extern "C" int gemma_engine_batch_open_rows(gemma_engine *e, int n_slots, int max_rows) {
    const char *fn = "gemma_engine_batch_open_rows";
    if (n_slots >= 1 && n_slots <= NS && (max_rows < std::max(NARROW, n_slots) || max_rows > NS)) {
        set_error(std::string(fn) + ": max_rows = " + std::to_string(max_rows) + " outside [" +
                  std::to_string(std::max(NARROW, n_slots)) + ", " + std::to_string(NS) + "]");
        return -1;
    }
    return batch_open(e, n_slots, NS, max_rows, fn);
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

// ---- a sampler per slot ----------------------------------------------------------------------------
// The setting belongs to the slot (active or not) and lives until batch_close: begin, adopt, release
// and fork leave it.  NULL: the slot follows the engine's sampler.  The parameters in force travel by
// value in the slot's rows of the row tables (slot_row::smp: one load in the kernels, as deep as the
// engine's one struct): a change here or of the engine's sampler marks the batch_step table dirty, and
// it is rewritten, a stream-ordered copy, ahead of the next pass; the other tables are built per pass.
extern "C" int gemma_engine_batch_set_sampler(gemma_engine *e, int slot, const gemma_sampler *sp) {
    set_error("");
    const std::string fn = "gemma_engine_batch_set_sampler";
    if (!slot_ok(e, slot, fn.c_str())) return -1;
    if (sp) {
        const std::string why = sampler_invalid(*sp);
        if (!why.empty()) {
            set_error(fn + ": " + why);
            return -1;
        }
    }
    (void)hipSetDevice(e->device);
    batch_state &b = e->bt;
    // a sampling slot needs a workspace per row of a pass: a wide batch has its own, a narrow one the
    // engine's 8 when the engine's sampler was ever on; else the batch makes its own now
    if (sp && sp->temperature > 0.0f && !b.picks.ws.hist && !e->smp_ws.hist &&
        sample_ws_alloc(e->bt_mem, &b.picks.ws, e->cfg.n_vocab, e->stream, b.pf.T)) {
        const std::string why = last_error();
        set_error(fn + ": " + why);
        return -1;
    }
    b.smp[slot] = sp ? *sp : gemma_sampler{0.0f, 0, 1.0f, 0};
    b.smp_own[slot] = sp != nullptr;
    b.dirty = true;  // the slot's rows carry other parameters
    return 0;
}

extern "C" int gemma_engine_batch_sampler(gemma_engine *e, int slot, gemma_sampler *out, int *own) {
    set_error("");
    if (!slot_ok(e, slot, "gemma_engine_batch_sampler")) return -1;
    const batch_state &b = e->bt;
    if (out) *out = b.smp_own[slot] ? b.smp[slot] : e->smp;
    if (own) *own = b.smp_own[slot] ? 1 : 0;
    return slot_samples(e, slot) ? 1 : 0;
}

// dst = a device-to-device copy of src's sequence (seq_copy: what adopt does from the engine's own);
// a copy, not a shared prefix.  The sampler settings stay with their slots.
extern "C" int gemma_engine_batch_fork(gemma_engine *e, int src, int dst) {
    set_error("");
    const std::string fn = "gemma_engine_batch_fork";
    if (!slot_ok(e, src, fn.c_str()) || !slot_ok(e, dst, fn.c_str())) return -1;
    batch_state &b = e->bt;
    if (!b.slot[src].active) {
        set_error(fn + ": slot " + std::to_string(src) + " (src) is not active");
        return -1;
    }
    if (src == dst) {
        set_error(fn + ": src == dst (slot " + std::to_string(src) + ")");
        return -1;
    }
    (void)hipSetDevice(e->device);
    if (seq_copy(e, b.slot[dst], b.slot[src])) return -1;
    b.slot[dst].active = true;
    b.dirty = true;
    return 0;
}

// ---- the row tables ----------------------------------------------------------------------------------
// Row t's entry of a row table, a row of slot `slot`: its part of the scratch, the slot's caches,
// history, words and sampler parameters.  own: the row has a RoPE row and a position word of its own,
// row t's of mrope (a pass with several rows per slot; k_rows_prepare fills them); else the slot's
static slot_row batch_row(const gemma_engine *e, int slot, int t, bool own) {
    const batch_state &b = e->bt;
    const seq_state &S = b.slot[slot];
    slot_row r;
    r.qkv = b.pf.QKV + (size_t)t * e->qkv_rows;
    r.out = b.pf.ATT + (size_t)t * e->qw;
    r.kc = S.kc; r.vc = S.vc;
    r.rope = own ? b.mrope + (size_t)t * (e->cfg.head_dim + 4) : S.rope;
    r.pos = own ? (int *)(r.rope + e->cfg.head_dim) : S.pos;  // a RoPE row ends with its position word
    r.hist = S.hist; r.nfix = S.nfix; r.last = S.token; r.lp = S.lp;
    r.smp = slot_params(e, slot);
    return r;
}

// the row -> slot table of the active set (ascending slot order) and the rows' first tokens
static int batch_write_rows(gemma_engine *e) {
    batch_state &b = e->bt;
    hipStream_t s = e->stream;
    slot_row *h = (slot_row *)b.stage;
    int R = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        if (!b.slot[i].active) continue;
        h[R] = batch_row(e, i, R, false);
        GHIP_CHECK(hipMemcpyAsync(b.row_tok + R, b.slot[i].token, 4, hipMemcpyDeviceToDevice, s));  // = hist[pos]
        ++R;
    }
    if (R) GHIP_CHECK(hipMemcpyAsync(b.rows, h, (size_t)R * sizeof(slot_row), hipMemcpyHostToDevice, s));
    b.dirty = false;
    return 0;
}

// The tables of a pass with several rows per slot (mrows, msrc), from the rows each slot has in it:
// m_of[i] for an active slot, 0 when it sits the pass out (an inactive slot's entry is not read).  Rows
// by ascending slot then position; a slot's rank counts every active slot before it, sitting out or
// not: its row of the batch_step table.  row0_of[i] / rank_of[i]: slot i's first row and rank, for the
// caller's per-slot table.  Returns the pass's rows T, -1 on error.
static int batch_build_rows(gemma_engine *e, const int32_t *m_of, int *row0_of, int *rank_of) {
    batch_state &b = e->bt;
    slot_row *hr = (slot_row *)b.mstage;
    row_src *hs = (row_src *)(hr + NS);
    int T = 0, rank = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        if (!b.slot[i].active) continue;
        row0_of[i] = T;
        rank_of[i] = rank;
        for (int k = 0; k < m_of[i]; ++k, ++T) {
            hr[T] = batch_row(e, i, T, true);
            hs[T] = row_src{b.slot[i].pos, k, rank};
        }
        ++rank;
    }
    GHIP_CHECK(hipMemcpyAsync(b.mrows, hr, (size_t)T * sizeof(slot_row), hipMemcpyHostToDevice, e->stream));
    GHIP_CHECK(hipMemcpyAsync(b.msrc, hs, (size_t)T * sizeof(row_src), hipMemcpyHostToDevice, e->stream));
    return T;
}

// ---- a pass --------------------------------------------------------------------------------------------
// The attention step of rows [r0, r0 + T) of bp.  One row per slot: k_attn_slots.  Rows that share
// slots: the K / V stores, a kernel boundary, the attention from the cache
int enqueue_batch_attention(gemma_engine *e, const batch_pass &bp, int il, int r0, int T) {
    attn_args t = attn_of(e, il);
    t.dsplit = e->att_dsplit;
    const int64_t layer_off = (int64_t)il * e->cfg.n_ctx * e->kvw;
    if (bp.src) return launch_attn_slot_rows(t, bp.rows + r0, bp.src + r0, T, layer_off, e->stream);
    return launch_attn_slots(t, bp.rows + r0, T, layer_off, e->stream);
}

// One pass over bp's rows and what every kind of pass does next: a pick from every row (row t reads
// its position word and its sampler parameters through bp.rows; mix: picks_mix of the participating
// slots) and, when asked, the logits rows to the host.  The advance and enqueue_lp_finish are the
// caller's.  The form of the pass is decided here and nowhere else: up to 8 rows the skinny pass; more
// rows one pass on the MFMA GEMMs from bt_mfma_min rows, else consecutive groups of up to 8 rows, each
// a skinny pass over its own rows of the scratch (the tokens, the row table and the pick keys are
// indexed by the pass's row).  A slot's rows may straddle groups: a group runs all its layers before
// the next starts, so later rows find the earlier rows' K / V in the cache
static int batch_run_pass(gemma_engine *e, const batch_pass &bp, int mix, float *logits, row_picks *pk) {
    batch_state &b = e->bt;
    const int T = bp.T;
    if (T > NARROW && T >= e->bt_mfma_min) {
        if (enqueue_batch_pass(e, bp, 0, T, false)) return -1;
    } else {
        for (int r0 = 0; r0 < T; r0 += NARROW)
            if (enqueue_batch_pass(e, bp, r0, std::min(NARROW, T - r0), true)) return -1;
    }
    if (enqueue_row_picks(e, b.pf.LG, T, nullptr, bp.rows, b.picks, pk, mix)) return -1;
    if (logits) GHIP_CHECK(hipMemcpyAsync(logits, b.pf.LG, (size_t)T * e->cfg.n_vocab * 4, hipMemcpyDeviceToHost, e->stream));
    return 0;
}

extern "C" int gemma_engine_batch_step(gemma_engine *e, int n, float *logits) {
    set_error("");
    const gemma_hip_config &c = e->cfg;
    batch_state &b = e->bt;
    if (!b.open) {
        set_error("gemma_engine_batch_step: no batch is open (gemma_engine_batch_open)");
        return -1;
    }
    int R = 0, n_sample = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        if (!b.slot[i].active) continue;
        ++R;
        n_sample += slot_samples(e, i);
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
    // one row per active slot: row r gives the token of its slot's sequence index pos + 1
    const batch_pass bp{b.rows, nullptr, b.row_tok, R};
    for (int i = 0; i < n; ++i) {
        row_picks pk;
        if (batch_run_pass(e, bp, picks_mix(n_sample, R), logits ? logits + (size_t)i * R * c.n_vocab : nullptr, &pk)) return -1;
        if (launch_batch_advance(b.rows, R, pk.keys, pk.n_parts, pk.stride, b.row_tok, c.n_ctx, rope_of(e), s)) return -1;
        if (enqueue_lp_finish(e, b.pf.LG, R, b.picks.lp_parts, nullptr, b.rows, nullptr)) return -1;
    }
    GHIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < b.n_slots; ++i)
        if (b.slot[i].active) b.slot[i].host_pos += n;
    return 0;
}

// ---- several rows per slot ---------------------------------------------------------------------
// The one statement of the allotment (a host function, no GPU): every active slot one row, then the
// rest of the budget in ascending slot order to the slots with more given tokens to consume.
extern "C" int gemma_batch_plan_rows(const int32_t *need, int n_slots, int max_rows, int32_t *rows_of) {
    set_error("");
    const char *fn = "gemma_batch_plan_rows";
    if (!need || !rows_of || n_slots < 1 || n_slots > NS) {
        set_error(std::string(fn) + ": n_slots = " + std::to_string(n_slots) + " outside [1, " + std::to_string(NS) + "], or a null array");
        return -1;
    }
    int R = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (need[s] < 0) {
            set_error(std::string(fn) + ": need[" + std::to_string(s) + "] is negative");
            return -1;
        }
        R += need[s] > 0;
    }
    if (R == 0) {
        set_error(std::string(fn) + ": no slot is active");
        return -1;
    }
    if (max_rows < R || max_rows > NS) {
        set_error(std::string(fn) + ": max_rows = " + std::to_string(max_rows) + " outside [" + std::to_string(R) + ", " +
                  std::to_string(NS) + "]");
        return -1;
    }
    int budget = max_rows - R, T = 0;
    for (int s = 0; s < n_slots; ++s) {
        const int extra = need[s] > 0 ? std::min(budget, need[s] - 1) : 0;
        rows_of[s] = need[s] > 0 ? 1 + extra : 0;
        budget -= extra;
        T += rows_of[s];
    }
    return T;
}

extern "C" int gemma_engine_batch_step_rows(gemma_engine *e, int max_rows, float *logits, int32_t *rows_of) {
    set_error("");
    const char *fn = "gemma_engine_batch_step_rows";
    const gemma_hip_config &c = e->cfg;
    batch_state &b = e->bt;
    if (!b.open) {
        set_error(std::string(fn) + ": no batch is open (gemma_engine_batch_open_rows)");
        return -1;
    }
    int32_t need[NS], m_of[NS];
    int R = 0, n_sample = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        const seq_state &S = b.slot[i];
        need[i] = S.active ? std::max(1, S.n_given - S.host_pos) : 0;
        R += S.active;
        n_sample += S.active && slot_samples(e, i);
    }
    if (R == 0) {
        set_error(std::string(fn) + ": no slot is active (gemma_engine_batch_begin / _adopt)");
        return -1;
    }
    if (max_rows < R || max_rows > b.pf.T) {
        set_error(std::string(fn) + ": max_rows = " + std::to_string(max_rows) + " outside [" + std::to_string(R) +
                  " active slots, the batch's row capacity " + std::to_string(b.pf.T) + "]");
        return -1;
    }
    const int T = gemma_batch_plan_rows(need, b.n_slots, max_rows, m_of);
    if (T < 0) {
        set_error(std::string(fn) + ": " + last_error());
        return -1;
    }
    for (int i = 0; i < b.n_slots; ++i)
        if (b.slot[i].active && (int64_t)b.slot[i].host_pos + m_of[i] >= c.n_ctx) {
            set_error(std::string(fn) + ": context full (slot " + std::to_string(i) + " at position " +
                      std::to_string(b.slot[i].host_pos) + ", " + std::to_string(m_of[i]) + " rows, n_ctx = " +
                      std::to_string(c.n_ctx) + ")");
            return -1;
        }
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    if (b.dirty && batch_write_rows(e)) return -1;
    // the pass's tables, and every active slot's span of rows by its rank
    int row0_of[NS], rank_of[NS];
    if (batch_build_rows(e, m_of, row0_of, rank_of) < 0) return -1;  // (= T, the plan's count)
    slot_span *hp = (slot_span *)((row_src *)((slot_row *)b.mstage + NS) + NS);  // behind the builder's two tables
    for (int i = 0; i < b.n_slots; ++i)
        if (b.slot[i].active) hp[rank_of[i]] = slot_span{row0_of[i], m_of[i]};
    GHIP_CHECK(hipMemcpyAsync(b.mspans, hp, (size_t)R * sizeof(slot_span), hipMemcpyHostToDevice, s));
    if (launch_rows_prepare(b.mrows, b.msrc, T, b.row_tok, rope_of(e), s)) return -1;
    // a pick from every row (one launch whatever T; only each slot's last row's is used)
    const batch_pass bp{b.mrows, b.msrc, b.row_tok, T};
    row_picks pk;
    if (batch_run_pass(e, bp, picks_mix(n_sample, R), logits, &pk)) return -1;
    if (launch_rows_advance(b.rows, b.mrows, b.mspans, R, pk.keys, pk.n_parts, pk.stride, b.row_tok, c.n_ctx, rope_of(e), s))
        return -1;
    if (enqueue_lp_finish(e, b.pf.LG, T, b.picks.lp_parts, nullptr, b.mrows, nullptr)) return -1;
    GHIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < b.n_slots; ++i) {
        if (b.slot[i].active) b.slot[i].host_pos += m_of[i];
        if (rows_of) rows_of[i] = m_of[i];
    }
    return T;
}

// ---- drafts in the batch -------------------------------------------------------------------------
// One exact pass in which every participating slot has its pending token and k_s drafts at consecutive
// positions (a several-rows-per-slot pass over tables of its own), then per slot on the device the
// accept rule, the advance over the accepted prefix and the rejected rows' K / V cleared: afterwards
// the slot's state is what a_s + 1 one-row passes leave.  A slot that sits out is in no table.
static_assert(GEMMA_VERIFY_MAX_DRAFT + 1 == BV_MAX_ROWS, "a slot's rows: its pending token and the drafts");
extern "C" int gemma_engine_batch_verify(gemma_engine *e, const int32_t *draft, const int32_t *k_of, int32_t *out_tokens,
                                         int32_t *n_out, float *logits) {
    set_error("");
    const std::string fn = "gemma_engine_batch_verify";
    const gemma_hip_config &c = e->cfg;
    batch_state &b = e->bt;
    constexpr int KD = GEMMA_VERIFY_MAX_DRAFT;
    if (!b.open) {
        set_error(fn + ": no batch is open (gemma_engine_batch_open)");
        return -1;
    }
    if (!draft || !k_of || !out_tokens || !n_out) {
        set_error(fn + ": a null draft, k_of, out_tokens or n_out");
        return -1;
    }
    int P = 0, T = 0, n_sample = 0;
    for (int i = 0; i < b.n_slots; ++i) {
        const seq_state &S = b.slot[i];
        if (!S.active) continue;
        const int k = k_of[i];
        if (k < -1 || k > KD) {
            set_error(fn + ": k_of[" + std::to_string(i) + "] = " + std::to_string(k) + " outside [-1, " + std::to_string(KD) + "]");
            return -1;
        }
        if (k < 0) continue;
        if (k >= 1 && (S.host_pos < S.n_given || S.host_pos < 1)) {
            set_error(fn + ": slot " + std::to_string(i) + " has " + std::to_string(std::max(S.n_given - S.host_pos, 0)) +
                      " given tokens still pending (the drafts follow the pending picked token)");
            return -1;
        }
        if (k >= 1 && !token_ids_ok(e, draft + (size_t)i * KD, k, fn.c_str())) return -1;
        if ((int64_t)S.host_pos + k + 1 >= c.n_ctx) {
            set_error(fn + ": context full (slot " + std::to_string(i) + ": pos + k + 1 = " +
                      std::to_string((int64_t)S.host_pos + k + 1) + " does not fit n_ctx = " + std::to_string(c.n_ctx) + ")");
            return -1;
        }
        ++P;
        T += 1 + k;
        n_sample += slot_samples(e, i);
    }
    if (P == 0) {
        set_error(fn + ": no slot takes part (no active slot, or every k_of is -1)");
        return -1;
    }
    if (T > b.pf.T) {
        set_error(fn + ": " + std::to_string(T) + " rows exceed the batch's row capacity " + std::to_string(b.pf.T));
        return -1;
    }
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    if (b.dirty && batch_write_rows(e)) return -1;
    // the pass's tables, and the per-slot table by the slot's index among the participating slots,
    // with its rank in the batch_step table
    int32_t m_of[NS];
    int row0_of[NS], rank_of[NS], part[NS];
    for (int i = 0; i < b.n_slots; ++i) m_of[i] = b.slot[i].active && k_of[i] >= 0 ? 1 + k_of[i] : 0;
    if (batch_build_rows(e, m_of, row0_of, rank_of) < 0) return -1;  // (= T)
    bv_slot *hv = (bv_slot *)b.vstage;
    int *h_out = (int *)(hv + NS);
    for (int i = 0, p = 0; i < b.n_slots; ++i) {
        if (!m_of[i]) continue;
        bv_slot v;
        v.row0 = row0_of[i]; v.m = m_of[i]; v.rank = rank_of[i];
        for (int j = 0; j < v.m - 1; ++j) v.draft[j] = draft[(size_t)i * KD + j];
        hv[p] = v;
        part[p++] = i;
    }
    GHIP_CHECK(hipMemcpyAsync(b.vslots, hv, (size_t)P * sizeof(bv_slot), hipMemcpyHostToDevice, s));
    // 1. stage: the drafts become hist_s[pos_s + 1 ..], the tokens of the slot's rows 1 .. k_s
    if (T > P && launch_bverify_stage(b.rows, b.vslots, P, c.n_ctx, s)) return -1;
    if (launch_rows_prepare(b.mrows, b.msrc, T, b.vtok, rope_of(e), s)) return -1;
    // 2. the pass over its own tokens, and a pick from every row: none advances
    const batch_pass bp{b.mrows, b.msrc, b.vtok, T};
    row_picks pk;
    if (batch_run_pass(e, bp, picks_mix(n_sample, P), logits, &pk)) return -1;
    // 3. accept + advance per slot; (log-probabilities on) rows 0 .. a_s score what the accept settled
    if (launch_bverify_accept(b.rows, b.mrows, b.vslots, P, pk.keys, pk.n_parts, pk.stride, b.row_tok, c.n_ctx, rope_of(e),
                              b.vout, s))
        return -1;
    if (enqueue_lp_finish(e, b.pf.LG, T, b.picks.lp_parts, nullptr, b.mrows, nullptr)) return -1;
    // 4. the rejected rows leave the caches
    if (T > P && launch_bverify_clean(b.rows, b.vslots, P, b.vout, c.n_layer, (int64_t)c.n_ctx * e->kvw, c.n_ctx, e->kvw, s))
        return -1;
    // 5. results: one synchronise
    GHIP_CHECK(hipMemcpyAsync(h_out, b.vout, (size_t)P * BV_OUT_WORDS * 4, hipMemcpyDeviceToHost, s));
    GHIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < b.n_slots; ++i) n_out[i] = 0;
    int wrong = -1;
    for (int p = 0; p < P; ++p) {
        const int i = part[p], a = h_out[p * BV_OUT_WORDS];
        if (a < 0 || a > k_of[i]) {
            wrong = i;
            continue;
        }
        for (int j = 0; j <= a; ++j) out_tokens[(size_t)i * (KD + 1) + j] = h_out[p * BV_OUT_WORDS + 1 + j];
        n_out[i] = a + 1;
        b.slot[i].host_pos += a + 1;
    }
    if (wrong >= 0) {
        set_error(fn + ": the accept kernel reported a count outside [0, k] for slot " + std::to_string(wrong));
        return -1;
    }
    return T;
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
