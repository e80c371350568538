// engine_impl.h — the device-resident engine's state and what its translation units share
// (internal: included only by engine.cpp, engine_decode.cpp, engine_prefill.cpp, engine_spec.cpp,
// engine_batch.cpp, engine_diag.cpp).
//   engine.cpp          lifecycle: create / free / begin / extend / step / tensor, TP and p2p set-up;
//                       what is done to a sequence (seq_state), the engine's own or a batch slot
//   engine_decode.cpp   one decode token: enqueue_step (+ K-quant), the pick, the persistent
//                       launch's arguments, the all-gathers
//   engine_prefill.cpp  batched prefill and the ggml executor's entry points
//   engine_spec.cpp     speculative decoding: the verify pass, lookup drafts, the generate loop
//   engine_batch.cpp    batched decode: up to 64 sequences (slots), one row each per weight pass
//   engine_diag.cpp     timing, tuning, plan and option setters, stamps, taps, per-op test hooks
#pragma once

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/gemma_hpc.h"
#include "engine_ext.h"
#include "kernels.h"

using namespace ghip;
using ghip::host_weights;

struct layer_dev {
    float *attn_norm = nullptr, *ffn_norm = nullptr;
    tiled_mat qkv, o, gate, up, down;
};

// K-quant layer matrices (wtype GGML_TYPE_Q4_K: llama.cpp's Q4_K_M files): raw ggml rows, each
// matrix Q4_K or Q6_K, multiplied by the K-quant matvec against the Q8_K INIT of its input
struct kq_mat {
    uint8_t *w = nullptr;
    int type = 0;
    int64_t rows = 0, K = 0, rb = 0;
    bool tiled = false;  // lane-contiguous layout (launch_kq_retile), else ggml rows
};
struct kq_layer {
    kq_mat q, k, v, o, gate, up, down;
    bool qk_fused = false;  // q and k share one allocation (k's rows right after q's, same type)
};

// matrix classes of a decode step and their launch plan (K split, row-tile groups per workgroup)
enum { MC_QKV = 0, MC_O, MC_GU, MC_DOWN, MC_LOGITS, MC_N };
struct launch_plan {
    int ks = 1, rpw = 1;
    int img = 0;  // attn-out / down: read the producer-written Q8_0 image (PRO_IMG) instead of f32
};

// scratch of a batched pass, every buffer indexed by the row t of the pass (lazily sized for the
// largest pass seen: prefill_alloc)
struct pf_scratch {
    int T = 0;
    int64_t ldq = 0, ldd = 0;
    float *X = nullptr, *SA = nullptr, *QKV = nullptr, *ATT = nullptr, *G = nullptr, *U = nullptr, *LG = nullptr;
    float *DA = nullptr;
    uint16_t *Q16 = nullptr;
    int8_t *XQ = nullptr;
    uint16_t *XH = nullptr;  // f16 image of the quantized activations (exact GEMM operand)
    uint16_t *XM = nullptr;  // K-quant prefill: the Q4_K mins operand of the Q8_K image (k_q8k_expand)
    uint8_t *XQ8K = nullptr;  // Q6_K head: the T Q8_K rows of rms_norm(x)*out_norm
    void *keys = nullptr;
    // log-probabilities: the partials of a pass of more than 8 rows, [T][G] (the engine's scratch: made
    // while they are on; a wide batch's: always, so nothing moves while it is open); else null
    lse_part *LP = nullptr;
};

// ---- a sequence (engine.cpp) ---- ---------------------------------------------------
// One sequence's state: everything on the device and advanced there (k_advance, k_batch_advance,
// k_verify_accept), plus the host's mirrors (steps and passes are deterministic).  The engine holds
// one as its own sequence (in `mem`, made once: the captured decode graph holds these addresses); a
// batch slot is another (in `bt_mem`).
struct seq_state {
    uint16_t *kc = nullptr, *vc = nullptr;  // [L][ctx][kvw], [L][kvw][ctx] (null: the engine's own on external caches)
    int *hist = nullptr;                    // [ctx + 1] the tokens by position
    double *lp = nullptr;                   // [ctx + 1] log-probability of hist[i] under the row before it (NaN: not scored)
    int *pos = nullptr, *nfix = nullptr;    // processed positions; given tokens (hist below *nfix is never overwritten)
    // the token word.  The engine's own: always the last pick (also inside the given tokens).  A
    // slot's: the pending token hist[*pos] (-1: inactive), a word of batch_state::last
    int *token = nullptr;
    float *rope = nullptr;                  // [cos | sin | (int)pos] of *pos, head_dim + 4 words
    bool active = false;                    // slots: holds a sequence
    int host_pos = 0, n_given = 0;          // mirrors of *pos / *nfix
};

// the pick keys of a pass of up to 64 rows (enqueue_row_picks)
static constexpr int PICK_MAX_ROWS = GEMMA_BATCH_WIDE_MAX_SLOTS;
struct pick_buf {
    unsigned long long *keys = nullptr;  // device: [64][256] greedy partial keys, then [64] sampler key slots
    sample_ws ws;                        // a batch's own sampler workspaces: a wide batch's, or a narrow one's made by
                                         // batch_set_sampler on an engine that has none (else the engine's 8: smp_ws)
    lse_part *lp_parts = nullptr;        // a wide batch's own log-probability partials (else the engine's 8 rows: lp_parts)
};

// ---- batched decode (engine_batch.cpp, DESIGN.md §5b⁗) ------------------------------------------
// rows from which a pass of more than 8 rows runs as ONE pass on the exact MFMA GEMMs (option
// "bt_mfma_min", [9, 65], 65 = never); below it the rows run as groups of up to 8 on the skinny GEMM.
// The default is the smallest R from which the MFMA form is faster at every larger R: DESIGN.md §5b⁗
// "Wide passes", table 1 (profiles/batch_wide/pass_time.json, pass_time_fine.json; Gemma-2B Q4_0,
// µs per pass, groups / MFMA): R = 24 5,888 / 7,256, 28 7,293 / 7,398, 29 7,529 / 7,401,
// 32 7,848 / 7,440, 48 11,887 / 7,866, 64 16,005 / 8,282.
static constexpr int BT_MFMA_MIN_DEFAULT = 29;
// What one pass over the batch's scratch is: T rows, row t with entry rows[t] and token tok[t].  It
// travels as an argument from the entry that built it to the pass's attention step; the engine keeps
// no note of the pass being enqueued.
struct batch_pass {
    const slot_row *rows;  // device: the pass's row table (bt.rows, or bt.mrows)
    const row_src *src;    // device: null for one row per slot (k_attn_slots); else rows that share slots, which run
                           // k_rows_rope_kv and k_attn_slot_rows
    const int *tok;        // device: the rows' tokens (bt.row_tok, or bt.vtok)
    int T;
};
struct batch_state {
    bool open = false;
    int n_slots = 0;
    seq_state slot[GEMMA_BATCH_WIDE_MAX_SLOTS];
    int *last = nullptr;       // device: [64] the slots' token words (one copy reads them: batch_last_n)
    slot_row *rows = nullptr;  // device: the pass's row -> slot table, rewritten when the active set changes
    int *row_tok = nullptr;    // device: [64] the token each row of the next pass processes
    pick_buf picks;
    void *stage = nullptr;     // pinned: the row table's source, batch_last's result
    pf_scratch pf;             // the pass's scratch (pf.T rows: max(8, n_slots), or open_rows' max_rows), never reallocated while the batch is open
    bool dirty = true;         // the active set changed since the table was written
    // several rows per slot (gemma_engine_batch_step_rows, gemma_engine_batch_verify): the pass's own
    // row table and row sources, rewritten by every such pass (batch_build_rows), and each row's
    // [cos | sin | (int)p]
    slot_row *mrows = nullptr;   // device: [64], row t's `rope` / `pos` its own RoPE row / position word
    row_src *msrc = nullptr;     // device: [64]
    slot_span *mspans = nullptr; // device: [64] by the slot's rank among the active slots (step_rows)
    float *mrope = nullptr;      // device: [64][head_dim + 4]
    void *mstage = nullptr;      // pinned: the three tables' source
    // drafts in the batch (gemma_engine_batch_verify): such a pass over the participating slots only.
    // Its rows' tokens are its own, so row_tok keeps the entries of the slots that sit out
    bv_slot *vslots = nullptr;   // device: [64] by the slot's index among the participating slots
    int *vout = nullptr;         // device: [64][BV_OUT_WORDS] each slot's accepted count and picks
    int *vtok = nullptr;         // device: [64] the tokens of the pass's rows
    void *vstage = nullptr;      // pinned: vslots' source, vout's copy
    // a sampler per slot (gemma_engine_batch_set_sampler): the setting belongs to the slot, active or not
    // (the device copy travels in the slot's rows of the row tables, slot_row::smp)
    bool smp_own[GEMMA_BATCH_WIDE_MAX_SLOTS] = {};      // the slot has a setting of its own ...
    gemma_sampler smp[GEMMA_BATCH_WIDE_MAX_SLOTS] = {};  // ... and its parameters as given (mode: temperature > 0)
};

struct gemma_engine {
    gemma_hip_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    // ---- memory (DESIGN.md §Memory ownership) ----
    // Every allocation belongs to one of three pools; gemma_engine_free clears them, nothing else frees.
    //   mem     the engine's lifetime: weights, caches, tables, activations, decode state, and what is
    //           created on first use and then kept (sampler workspace, verify buffers, pinned stages)
    //   pf_mem  the batched prefill's scratch, dropped and re-made whole when a pass needs more rows
    //   bt_mem  the batched decode's slots, tables and pass scratch: made whole by batch_open, cleared by
    //           batch_close; nothing in it is reallocated while the batch is open
    // The rule: anything a captured graph can hold lives in `mem` and is never reallocated; anything
    // that is reallocated calls drop_graph.  (The decode graph holds no pf_mem address.)
    dev_pool mem, pf_mem, bt_mem;
    int qw = 0, kvw = 0, qkv_rows = 0;
    // ---- weights ----
    tiled_mat embd;
    std::vector<layer_dev> layers;
    float *out_norm = nullptr;
    // token_embd / tied output in Q6_K (llama.cpp's Q4_0 / Q8_0 Gemma files): raw ggml rows, the
    // embedding dequantized by k_embed_q6K and the logits through the K-quant matvec
    int out_type = 0;
    uint8_t *embd_q6k = nullptr;
    bool embd_tiled = false;  // embd_q6k in the lane-contiguous layout (launch_kq_retile)
    int64_t embd_row_bytes = 0;
    uint8_t *xq8k = nullptr;  // the decode step's Q8_K row of rms_norm(x)*out_norm (in the captured graph)
    // ---- K-quant layers ----
    bool kq = false;              // K-quant layers (kql) instead of the tiled Q4_0 / Q8_0 ones
    std::vector<kq_layer> kql;
    uint8_t *kq_x = nullptr;      // Q8_K INIT of the current matvec input (max(E, qw, F) / 256 blocks)
    // hand-off mode (kq_fuse == 2): the Q8_K images each producer writes for its consumer, one
    // buffer per hand-off so no launch overwrites the image it reads (kq_x = the attn-norm image,
    // kq_xa = attention output, kq_xf = ffn-norm image, kq_xh = gelu(gate)*up); counters zeroed once
    uint8_t *kq_xa = nullptr, *kq_xf = nullptr, *kq_xh = nullptr;
    unsigned *kq_cnt = nullptr;
    int kq_cnt_cap = 0;
    float *kq_g = nullptr;        // ffn gate output (n_ff), consumed by the up matvec's gelu*mul epilogue
    // K-quant step options (gemma_engine_set_option): kq_fuse = the plan for where ggml's Q8_K INIT
    // runs (enqueue_step_kq, 0..6); kq_dual: gate+up in one launch; kq_pair: q|k and v in one launch
    int kq_fuse = 5, kq_dual = 1, kq_pair = 1;
    int kq_abl = 0;  // option "kq_abl": hand-off timing ablation (kq_args::q8_abl; wrong results)
    // ---- TP + p2p ----
    // row-split tensor parallelism: this rank's contiguous row range of every
    // matrix; activations are full vectors, each matvec writes its shard in place and an in-place
    // RCCL all-gather completes them
    int tp_n = 1, tp_rank = 0;
    int n_virtual = 1;  // > 1: all tp_n ranks' shards in this one engine (single-GPU parity mode, no RCCL)
    bool tp_n_keys = false;  // logits through per-rank argmax keys (row split: virtual ranks or an RCCL comm)
    ncclComm_t comm = nullptr;
    int64_t sh_qkv = 0, sh_e = 0, sh_ff = 0, sh_v = 0;  // rows per rank (qkv, n_embd, n_ff, n_vocab)
    // GEMMA_TP_REP_ATTN: Wq|Wk|Wv and Wo whole on every rank (sh_qkv = all rows, sh_o = n_embd), so
    // a layer needs 2 all-gathers (h, x) instead of 4; the FFN and the output head stay row-split
    bool rep_attn = false;
    int64_t sh_o = 0;
    // GEMMA_TP_P2P: the all-gathers by peer-to-peer pushes (p2p.hip) instead of RCCL: an uncached
    // arena of inboxes + flags per rank, shared by IPC handles (gemma_engine_p2p_handle / _open)
    bool p2p = false, p2p_ready = false;
    uint8_t *p2p_arena = nullptr;
    uint8_t *p2p_peer[P2P_MAX_RANKS] = {};
    unsigned *p2p_seq = nullptr, *p2p_err = nullptr;
    int64_t ib_qkv = 0, ib_sa = 0, ib_h = 0, ib_x = 0, ib_hact = 0, ib_hda = 0, ib_logits = 0, ib_keys = 0, ib_flags = 0;
    unsigned long long *rank_keys = nullptr;           // [tp_n] one argmax key per rank
    // ---- attention ----
    std::vector<uint16_t *> kc_ext, vc_ext;  // external per-layer caches of the own sequence (ggml executor), else empty
    int att_mode = ATTN_PER_HEAD;
    attn_geom ag;                           // split-attention geometry and its scratch
    float *att_sbuf = nullptr;
    int *att_sync = nullptr;                // hand-off counters [Hkv][2] + sticky error word
    uint16_t *exp_tab = nullptr, *gelu_tab = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    // per-head decode attention: workgroups per head (each the KQ/softmax, 1/att_dsplit of the KQV
    // dims; option "att_dsplit"). Same box, decode tok/s: 1 / 2 / 4 -> 1,443 / 1,458 / 1,458; after the
    // batched K/V step loads 2 / 4 / 8 -> 1,470-1,482 / 1,491 / 1,355-1,369 (scripts/env_ab.sh)
    int att_dsplit = 4;
    int att_mx = 1;  // option "att_mx": exact prefill attention on the f32 matrix cores (0: the row form)
    // ---- activations ----
    float *x = nullptr, *qkv = nullptr, *attn = nullptr, *sa = nullptr, *h = nullptr, *logits = nullptr;
    // Q8_0 activation images written by their producers (attention, gate/up) for attn-out and down
    // (DESIGN.md §Activation image); null when a shape does not allow them (then PRO_F32)
    uint32_t *att_act = nullptr, *h_act = nullptr;
    float *att_da = nullptr, *h_da = nullptr;
    // ---- persistent launch ----
    // the whole token's layers as ONE persistent launch (token.hip) when the shapes
    // allow it (GHIP_PERSIST=1 or gemma_engine_set_persist(e, 1)); off by default until it beats
    // the per-layer launches on the bench
    int persist = 0;
    std::string persist_why;           // why the persistent launch cannot run ("" = it can)
    tok_args tok{};                    // its arguments (host copy; tok_dev: the copy the kernel reads)
    tok_args *tok_dev = nullptr;
    tok_layer *tok_tab = nullptr;      // per-layer pointer table
    unsigned long long *tok_gran = nullptr;  // hand-off granules (zeroed once; tags carry the epoch)
    unsigned *epoch = nullptr;         // bumped by k_advance / k_set_position once per token
    int *tok_err = nullptr;            // sticky hand-off timeout [flag, site, layer]
    unsigned persist_timeout = 2000000u;  // per-wait bound of the launch (100 MHz ticks; tests shorten it)
    // ---- fused launches ----
    // fused layer front (layer_front.hip): qkv -> attention -> attn-out in one launch per layer;
    // hand-off counters [n_layer][16] zeroed once per token (memset node), sticky timeout word
    int fuse_front = 0;  // measured: 727 vs 672 us/token (the in-launch hand-offs cost as much as the
                         // launch boundaries they replace; DESIGN.md perf log) — kept as an option
    unsigned *front_cnt = nullptr;
    int *front_err = nullptr;
    // attention + attn-out in one launch (layer_front.hip k_attn_o): on / off, its per-layer hand-off
    // counters (8 replicas + done, 128 B apart; the launch leaves them zero) and sticky error words
    int att_o = 0;
    unsigned *ao_cnt = nullptr;
    int *ao_err = nullptr;
    // ---- decode state ----
    seq_state seq;                      // the engine's own sequence (begin / extend / step / verify)
    unsigned long long *key = nullptr;  // the decode step's per-workgroup argmax keys
    // on-device sampling (gemma_engine_set_sampler; sample.hip): off = greedy, nothing below is used
    bool sampling = false;
    gemma_sampler smp{0.0f, 0, 1.0f, 0};  // the parameters as given
    sampler_params smp_host;              // their device form (source of the stream-ordered copy)
    sampler_params *smp_dev = nullptr;
    sample_ws smp_ws;                     // allocated when sampling is first turned on
    // per-token log-probabilities (gemma_engine_set_logprobs; logprob.hip): off = nothing below is used
    bool logprobs = false;
    lse_part *lp_parts = nullptr;         // [8][G] partials (step, verify, narrow batch); allocated when first turned on
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    // flow control of gemma_engine_step: an event every FC_EVERY graph launches, FC_SLOTS of them
    hipEvent_t fc_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float *ext_stage = nullptr;               // pinned logits row (ggml executor path)
    int *ext_err = nullptr;                   // pinned copy of the persistent launch's sticky word (same path)
    // ---- plan ----
    // launch geometry: one plan per matrix class (defaults below; gemma_engine_tune measures)
    int ks_small = KS_RR, ks_down = KS_RR;  // round-pipelined form where the shape allows (pick_ks falls back)
    int grid_big = 2048;
    int grid_big_cap = 2048;  // workgroups the argmax key buffer holds
    launch_plan plan[MC_N];
    // ---- prefill ----
    pf_scratch pf;  // prefill buffers (lazily sized for the prompt length)
    batch_state bt;
    int bt_mfma_min = BT_MFMA_MIN_DEFAULT;  // option "bt_mfma_min"
    // ---- verify pass (gemma_engine_verify; allocated at its first call) ----
    struct {
        pick_buf picks;
        int *ints = nullptr;                 // device: [8] row positions (sampler), [9] result {a, g_0 .. g_7}
        int *host = nullptr;                 // pinned: [8] drafts, [8] row positions, [9] result
    } vf;
    // ---- diagnostics ----
    int time_hot = 0, ablate = 0;  // gemma_engine_time diagnostics: one layer's matrix repeated; ablations
    float *dbg = nullptr;  // per-layer taps [L][qkv_rows + qw + E] (debug steps only)
    unsigned long long *stamp = nullptr;  // phase stamps of one layer's kernels (diagnostic steps only)
    int stamp_layer = -1;
};

// ---- small accessors ---------------------------------------------------------------------------
static constexpr size_t kStampRegion = 4096 * 16;  // u64 per kernel: <= 4096 workgroups x 16 stamps
static inline unsigned long long *stamp_region(gemma_engine *e, int il, int k) {
    return (e->stamp && il == e->stamp_layer) ? e->stamp + (size_t)k * kStampRegion : nullptr;
}

// layer il's shards of (virtual) rank slot vr, and the rank that slot stands for
static inline layer_dev &layer_of(gemma_engine *e, int il, int vr) { return e->layers[(size_t)il * e->n_virtual + vr]; }
static inline int rank_of(const gemma_engine *e, int vr) { return e->n_virtual > 1 ? vr : e->tp_rank; }
// layer il's caches of a sequence: K [ctx][kvw], V [kvw][ctx] (only the engine's own can be external).
// "The engine's own" is decided by address: S must be e->seq itself or a slot, never a copy of one
// (a copy of e->seq on an external-cache engine has null caches).
static inline uint16_t *kc_of(const gemma_engine *e, const seq_state &S, int il) {
    return &S == &e->seq && !e->kc_ext.empty() ? e->kc_ext[il] : S.kc + (size_t)il * e->cfg.n_ctx * e->kvw;
}
static inline uint16_t *vc_of(const gemma_engine *e, const seq_state &S, int il) {
    return &S == &e->seq && !e->vc_ext.empty() ? e->vc_ext[il] : S.vc + (size_t)il * e->cfg.n_ctx * e->kvw;
}
// all ranks' rows are not in one matrix on one GPU: a row-split engine (RCCL, p2p or virtual ranks).
// (prefill_run / prefill_next test tp_n > 1 || comm without n_virtual and are left exactly so.)
static inline bool row_split(const gemma_engine *e) { return e->tp_n > 1 || e->comm || e->n_virtual > 1; }

// a batch slot's picks sample: by its own setting, else by the engine's sampler
static inline bool slot_samples(const gemma_engine *e, int slot) {
    return e->bt.smp_own[slot] ? e->bt.smp[slot].temperature > 0.0f : e->sampling;
}

// attention can hand attn-out the Q8_0 image of its output (per-head form; split form with 32-dim slices)
static inline bool att_img_ok(const gemma_engine *e) { return e->att_mode == ATTN_PER_HEAD || e->ag.img; }

// workgroups of a matvec launch: a KS = 1 workgroup runs 4 waves on 4 row tiles at a time, a
// KS > 1 workgroup its KS waves on one row tile; each workgroup repeats for rpw row-tile groups
static inline int mv_grid(const gemma_engine *e, int cls, int64_t n_rt) {
    const launch_plan &p = e->plan[cls];
    const int64_t per = (p.ks == 1 || cls == MC_GU ? 4 : 1) * (int64_t)std::max(p.rpw, 1);  // gate/up ks 2: 4 row tiles
    int64_t g = (n_rt + per - 1) / per;
    if (cls == MC_LOGITS || cls == MC_GU) g = std::min<int64_t>(g, e->grid_big);  // key slots
    return (int)std::max<int64_t>(g, 1);
}

// largest power-of-two K split <= target that divides the block-tile count and whose LDS image
// (activation + carry stash) fits the 160 KiB of a CU (Gemma-7B's down, K = 24576, steps to KS 1)
static inline int pick_ks(int wtype, int64_t n_bt, int target) {
    if (target == KS_RR) return matvec_rr_supported(wtype, n_bt) ? KS_RR : pick_ks(wtype, n_bt, 8);
    int ks = target;
    while (ks > 1 && (n_bt % ks || matvec_lds_bytes(wtype, ks, n_bt, n_bt / ks) > 160 * 1024)) ks >>= 1;
    return ks;
}

// the persistent token launch runs this engine's decode steps
static inline bool persist_on(const gemma_engine *e) {
    return e->persist && e->persist_why.empty() && !e->dbg && !e->stamp && e->att_mode == ATTN_PER_HEAD &&
           !e->fuse_front;
}

// rows [r0, r0+n) of a tiled matrix (r0, n multiples of 8) as its own tiled_mat view
static inline tiled_mat sub_rows(const tiled_mat &m, int64_t r0, int64_t n) {
    tiled_mat v = m;
    const int sb = m.type == T_Q4_0 ? 16 : 8;
    v.rows = n;
    v.n_rt = (n + 7) / 8;
    v.qs = m.qs + (r0 / 8) * m.n_bt * 1024;
    v.sc = m.sc + (r0 / 8) * m.n_bt * 8 * sb;
    return v;
}

// ---- argument builders -------------------------------------------------------------------------
// the decode attention of layer il: everything but the output images, dsplit and the stamps
static inline attn_args attn_of(gemma_engine *e, int il) {
    const gemma_hip_config &c = e->cfg;
    attn_args t;
    t.qkv = e->qkv;
    t.kc = kc_of(e, e->seq, il);
    t.vc = vc_of(e, e->seq, il);
    t.rope_cos = e->rope_cos; t.rope_sin = e->rope_sin; t.rope_cur = e->seq.rope; t.exp_tab = e->exp_tab;
    t.pos = e->seq.pos; t.out = e->attn;
    t.H = c.n_head; t.Hkv = c.n_head_kv; t.hd = c.head_dim; t.ctx = c.n_ctx;
    t.q_scale = 1.0f / sqrtf((float)c.head_dim);
    t.mode = e->att_mode;
    t.nwg = e->ag.nwg; t.sbuf = e->att_sbuf; t.sync = e->att_sync; t.err = e->att_sync + e->ag.sync_ints;
    return t;
}

// the RoPE tables and the current-position row k_advance / k_set_position publish
static inline rope_row rope_of(const gemma_engine *e) {
    rope_row rr;
    rr.cos = e->rope_cos; rr.sin = e->rope_sin; rr.cur = e->seq.rope; rr.half = e->cfg.head_dim / 2; rr.ctx = e->cfg.n_ctx;
    rr.epoch = e->epoch;
    return rr;
}

// what is wrong with a sampler's fields ("" = valid); the message names the field
static inline std::string sampler_invalid(const gemma_sampler &s) {
    if (!std::isfinite(s.temperature)) return "temperature is not finite";
    if (s.top_k < 0 || s.top_k > SAMPLE_MAX_K) return "top_k outside [0, " + std::to_string(SAMPLE_MAX_K) + "]";
    if (!std::isfinite(s.top_p) || !(s.top_p > 0.0f) || s.top_p > 1.0f) return "top_p outside (0, 1]";
    return "";
}

// ---- functions that cross translation units (internal: not part of the library's surface) -------
#pragma GCC visibility push(hidden)
// engine.cpp
int ensure_graph(gemma_engine *e);
void drop_graph(gemma_engine *e);
// engine.cpp: one function per thing done to a sequence, the engine's own or a slot
// every id in [0, n_vocab), else the error "<fn>: token id <id> out of range [0, n_vocab)" (name_id
// false: "<fn>: token id out of range")
bool token_ids_ok(const gemma_engine *e, const int32_t *tokens, int n, const char *fn, bool name_id = true);
// S's buffers from pool M, zeroed (caches false: none, the engine's own on external ones; token_word:
// the word to use instead of one of its own)
int seq_alloc(gemma_engine *e, dev_pool &M, seq_state &S, bool caches, int *token_word);
// S = the n given tokens at position 0: caches and history cleared, *pos = 0 with its RoPE row,
// *nfix = n; synchronises.  The token word is the caller's (its meaning differs, seq_state)
int seq_begin(gemma_engine *e, seq_state &S, const int32_t *tokens, int n);
// dst = src (caches, history, position, RoPE row with its position word), dst's token word the
// pending token hist[host_pos]: what a slot's word means; synchronises
int seq_copy(gemma_engine *e, seq_state &dst, const seq_state &src);
// K rows / V columns p0 .. p0+n of one layer as [n][kvw] each; fn names the caller in the range error
int seq_kv_read(gemma_engine *e, const seq_state &S, int layer, int p0, int n, uint16_t *k_rows, uint16_t *v_rows,
                const char *fn);
// hist[0 .. min(cap, host_pos + 1)): the pending token included; returns the count
int seq_tokens(const seq_state &S, int32_t *out, int cap);
// engine_decode.cpp
int enqueue_step(gemma_engine *e);
// the token of position *pos + 1 and the advance: the sampler on `row` when sampling is on, else
// the greedy argmax keys (n_parts of them) exactly as before
// rows0 / R: the pass's R rows that end with `row` (a prefill), all scored when log-probabilities are on
int enqueue_pick(gemma_engine *e, const float *row, const unsigned long long *keys, int n_parts, const float *rows0 = nullptr,
                 int R = 1, lse_part *own = nullptr);
// the pick alone, no advance: with sampling on, the sampler's draw for sequence index *pos + 1 from
// `row` into the sampler's own key slot, *keys / *n_parts set to that one key; sampling off: nothing
// is launched and the caller's greedy keys stand
int enqueue_pick_keys(gemma_engine *e, const float *row, const int *pos, const unsigned long long **keys, int *n_parts);
// The pick of every row of a pass: LG [T][n_vocab], T <= 64; the device position word of row t is
// tab[t].pos when the pass has a row table, else pos + t (its token is that sequence's index *pos_t + 1).
// Enqueues the sampler's draws (sampling on: three launches) or the row argmaxes (one launch) into b
// and returns what the advance kernel takes: row t's n_parts keys at keys + t * stride
struct row_picks {
    const unsigned long long *keys = nullptr;
    int n_parts = 0, stride = 0;
};
int pick_buf_alloc(dev_pool &M, pick_buf &b, hipStream_t s);  // zeroed on s
// Log-probabilities of a pass's R rows LG [R][n_vocab] (nothing is launched while they are off).
// enqueue_lp_parts: the rows' partials, right after the logits (enqueue_pick and enqueue_row_picks
// issue it); own: partials of the pass's own, else the engine's 8 rows.  enqueue_lp_finish: after the
// advance, lp[q] of every row; the rows are a row table's (tab), or consecutive positions of S ending
// at *S.pos (acc: the device word of a verify pass's accepted count, rows past it are not scored)
int enqueue_lp_parts(gemma_engine *e, const float *LG, int R, lse_part *own);
int enqueue_lp_finish(gemma_engine *e, const float *LG, int R, lse_part *own, const seq_state *S, const slot_row *tab,
                      const int *acc);
// lp[p0 .. p0 + n) of S into out after one synchronise; fn names the caller in the range error
int seq_logprobs(gemma_engine *e, const seq_state &S, int p0, int n, double *out, const char *fn);
// mix: PICKS_GREEDY / _SAMPLE / _MIXED from the caller's mirror of its rows' modes (a batch pass: each row
// reads its parameters from tab[t].smp); -1: the engine's sampler for every row
int enqueue_row_picks(gemma_engine *e, const float *LG, int T, const int *pos, const slot_row *tab, const pick_buf &b,
                      row_picks *out, int mix = -1);
int tok_prepare(gemma_engine *e);
int persist_report(gemma_engine *e, const int *w);
int persist_check(gemma_engine *e);
int att_o_check(gemma_engine *e);
int tp_gather(gemma_engine *e, float *full, int64_t cnt);
// ncols Q8_K columns x ((n_embd / 256) * 292 bytes apart) through the Q6_K tied output -> y [ncols][n_vocab]
int enqueue_logits_q6k(gemma_engine *e, const uint8_t *x, int ncols, float *y);
// engine_prefill.cpp: the exact batched pass over hist[p0 .. p0+T), T <= 8, with the Q4_0 / Q8_0
// GEMMs on launch_gemm_skinny and no pick: the logits rows are left in pf.LG [T][n_vocab]
int enqueue_verify_pass(gemma_engine *e, int T, int p0);
// the batch's scratch (bt.pf, `rows` >= 8 rows, from bt_mem), and one batched-decode pass over rows
// [r0, r0 + T) of bp (tokens bp.tok, attention by enqueue_batch_attention), their logits left in
// bt.pf.LG.  skinny: T <= 8 on the skinny GEMM (the verify pass's form); else the exact MFMA GEMMs
int batch_scratch_alloc(gemma_engine *e, int rows);
int enqueue_batch_pass(gemma_engine *e, const batch_pass &bp, int r0, int T, bool skinny);
// engine_batch.cpp: layer il's attention step for rows [r0, r0 + T) of bp: the one place that chooses
// a batch pass's attention (k_attn_slots, or k_rows_rope_kv + k_attn_slot_rows when bp.src is set)
int enqueue_batch_attention(gemma_engine *e, const batch_pass &bp, int il, int r0, int T);
#pragma GCC visibility pop
