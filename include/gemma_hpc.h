/*
 * gemma_hpc.h — the C-ABI drop-in boundary of the MI355X hot path (libgemma_hip.so).
 *
 * Plain C types and pointers only; no torch types.  Every entry point names the reference
 * interface it replaces.  Host side: the reference's forked ggml calls `mul_mat` from
 * ggml_compute_forward_mul_mat's COMPUTE phase; the performance path keeps the
 * whole Gemma token on the device (gemma_engine_*, the `hpc_graph_compute` role of SURVEY §8(b)).
 */
#ifndef GEMMA_HPC_H
#define GEMMA_HPC_H

#include <stddef.h>
#include <stdint.h>

#include "ggml.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- narrow drop-in: replaces src/hpc.h:22-32 / src/hpc.cpp:216-390 ------------------------
 * Same signature and argument meaning.  dst[(c % ne1)*nb1 + (c / ne1)*nb2 + r*4] =
 * vec_dot(shared_edge, src0 + r*nb01, wdata + c*row_size) for r < ne01, c < ne11*ne12, with the
 * dot computed on the GPU in ggml's AVX2 lane order (bit-identical to the CPU path).
 * src0_type: GGML_TYPE_Q4_0, GGML_TYPE_Q8_0 (wdata = block_q8_0 rows), GGML_TYPE_Q4_K /
 * GGML_TYPE_Q6_K (wdata = block_q8_K rows; ggml's AVX2 K-quant lane order) or GGML_TYPE_F16
 * (wdata = fp16 rows).  `vec_dot` is accepted for link compatibility and not called.
 * Quantized src0 is uploaded + re-tiled once and cached by (src0->data, shape) — weights are
 * immutable for the program's lifetime (src/gemma_model.cpp:24-27).  CONTRACT: a caller that
 * frees or rewrites a quantized src0 buffer calls hpc_unregister_weight(ptr) (or
 * hpc_flush_weights()) first; otherwise a later buffer at the same address gets the stale copy.
 * F16 src0 (KV-cache views) is uploaded on every call.  Errors: no return value (as the reference); the message is kept
 * for hpc_last_error() and, unless hpc_set_error_mode(0), the process exits(1) like
 * src/hpc.cpp:163-166 / src/opencl.cpp:13-17.                                                   */
void mul_mat(int64_t ne01, int64_t ne11, int64_t ne12, int64_t nb01, int64_t ne1, int64_t nb1, int64_t nb2,
             size_t row_size, int64_t shared_edge, struct ggml_tensor *src0, struct ggml_tensor *src1,
             struct ggml_tensor *dst, ggml_vec_dot_t vec_dot, enum ggml_type src0_type, const char *wdata);

/* ---- device-dispatch lifecycle: replaces src/opencl.h:22-38 (init_opencl, get_kernel,
 * create_buffer, enqueue_kernel, wait_queue_finish, release_buffer_in_set) -------------------- */
int hpc_init(int device);                 /* init_opencl (src/opencl.cpp:350-356); 0 = ok        */
void hpc_shutdown(void);                  /* frees the weight cache and the device scratch        */
int hpc_register_weight(const void *host, int type, int64_t ne00, int64_t ne01, size_t nb01);
int hpc_last_error(char *buf, size_t len);/* length of the last error message (0 = none)          */
void hpc_set_error_mode(int exit_on_error);
int hpc_weight_cache_entries(void);
int hpc_unregister_weight(const void *host); /* drop the cached device copies of `host`; returns the count */
void hpc_flush_weights(void);                /* drop every cached device weight                          */
void hpc_set_matvec_ks(int ks);          /* K-split of the quantized matvec (1/2/4/8; tests) */
/* live device + pinned allocations of the whole library (engines, caches, executor, temporaries):
   how many and their bytes; either pointer may be NULL.  Always returns 0. */
int gemma_hip_mem_live(int64_t *allocs, int64_t *bytes);
/* columns from which K-quant mul_mats (and the K-quant engine prefill) run the MFMA GEMM
 * (prefill_kq.hip) instead of the dot4 kernels; -1 = GHIP_KQ_MFMA_MIN or 8 (tests: same bytes) */
void hpc_set_kq_gemm_min(int min_cols);
/* the exact Q4_0 / Q8_0 prefill GEMM's form, modes 0-4: 1 = K = 4 multi-block MFMA (k_gemm_x4, dense
   lane fragments, 32 rows x 64 tokens per workgroup), 2 = the same with 64 x 32, 3 (default) and 4 =
   1 and 2 with the activation staged from the int8 image instead of the f16 one, 0 = the lane-masked
   32x32x16 form (k_gemm_x); bit-identical every way.  Process-wide; a pass reads it once, at its
   start.  Any other value leaves the form as it was and sets the last-error text (hpc_last_error) */
void hpc_set_gemm_x4(int mode);

/* ---- graph executor (SURVEY §8(b) `hpc_graph_compute(ggml_cgraph*)`): runs a graph built with the
 * ggml surface of include/ggml.h on the GPU; 0 = ok, else hpc_last_error() tells */
int hpc_graph_compute(struct ggml_cgraph *graph);

/* ---- device-resident Gemma engine (performance path: the Gemma graph encoded as one hipGraph) ---- */
typedef struct gemma_hip_config {
    int n_layer, n_embd, n_head, n_head_kv, head_dim, n_ff, n_vocab, n_ctx;
    int wtype; /* GGML_TYPE_Q4_0 or GGML_TYPE_Q8_0 (the layer matrices) */
    float eps, rope_base;
    uint64_t seed;
    int gelu_clamp;
    int out_type; /* token_embd / tied output: 0 = wtype, or GGML_TYPE_Q6_K (llama.cpp's Q4_0 / Q8_0 files) */
    float out_gain; /* synthetic weights: token_embd / output std x out_gain (0 = 1; SURVEY §8(d) uses 4 for
                       peaked logits in the Gemma-7B TP leg); ignored for GGUF weights */
} gemma_hip_config;

typedef struct gemma_engine gemma_engine;

gemma_engine *gemma_engine_create(const gemma_hip_config *cfg, int device);
/* real weights from a Gemma GGUF file (src/gemma_model.cpp:19-229 loads the same tensors and keys):
 * layer matrices all Q4_0 or all Q8_0, token_embd that type or Q6_K (llama.cpp's layout); NULL with
 * hpc_last_error on anything else.  gemma_engine_config returns the configuration read. */
gemma_engine *gemma_engine_create_from_gguf(const char *path, int n_ctx, int device);
int gemma_engine_config(const gemma_engine *e, gemma_hip_config *out);
/* row-split tensor parallelism: one process per GPU; rank r holds rows
 * [r*rows/n, (r+1)*rows/n) of every matrix and RCCL all-gathers complete each activation vector
 * (4 per layer + one argmax key per rank), so logits are bit-identical to one GPU.
 * gemma_tp_unique_id fills `out` (>= 128 B) on rank 0; every rank passes a copy to create_tp.
 * nccl_id == NULL: all n_ranks shards in one engine on one GPU ("virtual ranks", same shards and
 * key merge, shards written in place instead of gathered) for single-GPU parity tests. */
int gemma_tp_unique_id(void *out, int cap);
gemma_engine *gemma_engine_create_tp(const gemma_hip_config *cfg, int device, int n_ranks, int rank,
                                     const void *nccl_id);
/* n_ranks == 1 with an id: a 1-rank RCCL communicator; every all-gather and the key gather then run
 * through RCCL (captured in the decode hipGraph) exactly as on N GPUs.  tp_info: [ranks, rank,
 * communicator present, shard slots in this engine] */
int gemma_engine_tp_info(const gemma_engine *e, int *out4);
/* layout flags for create_tp2: GEMMA_TP_REP_ATTN keeps Wq|Wk|Wv and Wo whole on every rank (the
 * attention block replicated, 2 all-gathers per layer instead of 4; the FFN and the output head
 * stay row-split; the same bits either way).  tp_flags returns the engine's flags. */
#define GEMMA_TP_REP_ATTN 1
/* GEMMA_TP_P2P (nccl_id NULL, n_ranks > 1, one process per GPU): the all-gathers by peer-to-peer
 * pushes into each peer's uncached inbox arena (p2p.hip) instead of RCCL.  Each rank publishes its
 * arena with gemma_engine_p2p_handle (an IPC handle, <= 64 B), every rank passes all handles in
 * rank order to gemma_engine_p2p_open, then a host barrier, then steps.  p2p_err: a flag wait timed
 * out (sticky; reset clears). */
#define GEMMA_TP_P2P 2
int gemma_engine_p2p_handle(const gemma_engine *e, void *out, int cap);
int gemma_engine_p2p_open(gemma_engine *e, const void *handles, int n);
int gemma_engine_p2p_err(gemma_engine *e, int reset);
gemma_engine *gemma_engine_create_tp2(const gemma_hip_config *cfg, int device, int n_ranks, int rank,
                                      const void *nccl_id, int flags);
int gemma_engine_tp_flags(const gemma_engine *e);
void gemma_engine_free(gemma_engine *e);
/* start a sequence: KV cache cleared, prompt stored on the device */
int gemma_engine_begin(gemma_engine *e, const int32_t *prompt, int n_prompt);
/* run n steps of the ordered (bit-exact) per-token pass starting at the current position;
 * step i processes sequence[pos] and appends the greedy token once the prompt is consumed.
 * logits (n_vocab floats per step) are copied out when logits != NULL. use_graph: replay a
 * captured hipGraph per step (no host sync between steps when logits == NULL). */
int gemma_engine_step(gemma_engine *e, int n, float *logits, int use_graph);
int gemma_engine_tokens(gemma_engine *e, int32_t *out, int cap); /* sequence so far; returns len */
int gemma_engine_pos(gemma_engine *e);
/* batched prefill (the reference's T-token graph, src/gemma_model.cpp:665-747): processes the
 * whole prompt in one pass, writes the last row's logits (and all rows if logits_all), returns
 * the greedy token.  Bit-identical to the CPU path (ggml lane order). */
int gemma_engine_prefill(gemma_engine *e, float *logits_last, float *logits_all);
/* the same on int8/f16 MFMA: fp32 summation order differs from the CPU path (tolerance path) */
int gemma_engine_prefill_fast(gemma_engine *e, float *logits_last, float *logits_all);
/* Continue or rewind the sequence.  Positions [0, keep) stay (0 <= keep <= pos: their K/V rows are in
 * the caches); everything from `keep` on is dropped, the pending greedy token included; `tokens`
 * become positions keep .. keep+n-1, given but not yet processed (n >= 1, keep + n < n_ctx, ids in
 * [0, n_vocab)).  keep == 0 is gemma_engine_begin.  Afterwards pos == keep and either
 * gemma_engine_step consumes the tokens one by one or gemma_engine_prefill_next in batches.
 * -1 with hpc_last_error and the state untouched on a bad argument. */
int gemma_engine_extend(gemma_engine *e, int keep, const int32_t *tokens, int n);
/* One batched pass over the next `n` given-but-unprocessed tokens, positions [pos, pos+n)
 * (n == 0: all that remain; 1 <= n <= n_seq - pos), against the caches of [0, pos).  exact != 0:
 * bit-identical to the CPU path and to the token-by-token steps; 0: the MFMA tolerance path.
 * logits_last: the last row; logits_all: [n][n_vocab].  Returns the last row's greedy token; when
 * the pass reaches the end of the given tokens that token is appended (as gemma_engine_prefill
 * does) and the engine is ready for gemma_engine_step, otherwise nothing is appended and the
 * next call continues the prompt.  Scratch is sized by the largest n seen, not by n_seq.
 * Single-GPU engines only; K-quant layers have the exact form only. */
int gemma_engine_prefill_next(gemma_engine *e, int n, int exact, float *logits_last, float *logits_all);
/* Seeded temperature / top-k / top-p sampling inside the decode step (no host round trip; DESIGN.md
 * §5b″ has the rule in full).  With the sampler on, the token at sequence index p comes from its logits
 * row l[0..V): K = min(top_k, V) (top_k == 0: min(1024, V); more than 1024 candidates are not sampled:
 * the distribution is truncated there); candidates c_0..c_{K-1} = the first K entries under "larger
 * logit, then smaller index" (-0 == +0); f64 weights w_i = exp((l[c_i] - l[c_0]) / temperature) with
 * prefix sums C_i, W = C_{K-1}; m = K when top_p == 1, else the smallest i + 1 with C_i >= top_p * W;
 * u = (splitmix64_mix(seed + (p + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53, r = u * C_{m-1}; the token
 * is c_j for the smallest j < m with C_j > r (else j = m - 1).  The draw depends on (seed, p) only:
 * not on call count, graph or eager, batching, or a rewind.  Steps, prefill and prefill_next all pick
 * through it; given (prompt) positions are never overwritten.
 * Changing the parameters of a running sampler is a stream-ordered copy and keeps the captured decode
 * graph (the launch geometry does not depend on top_k); turning sampling on or off drops it. */
typedef struct gemma_sampler { float temperature; int top_k; float top_p; uint64_t seed; } gemma_sampler;
/* NULL or temperature <= 0: greedy (the default).  -1 + hpc_last_error, state untouched, on
 * top_k outside [0, 1024], top_p outside (0, 1], a non-finite field, or a row-split engine. */
int gemma_engine_set_sampler(gemma_engine *e, const gemma_sampler *s);
int gemma_engine_sampler(const gemma_engine *e, gemma_sampler *out);   /* 1 = sampling on, 0 = greedy */
/* per-op test entry: the sampler on host rows.  positions[r] = the p of row r.  Outputs (any may be
 * NULL): tokens[rows]; cand[rows][1024] candidate ids in order, -1 past K; n_cand[rows] = K;
 * n_kept[rows] = m */
int gemma_test_sample(const float *logits, int rows, int n_vocab, const gemma_sampler *s,
                      const int32_t *positions, int32_t *tokens, int32_t *cand, int32_t *n_cand, int32_t *n_kept);
/* the same with one sampler per row, s_of[rows], all rows through one set of launches (those of a batch
 * pass with this mix of rows).  A row with temperature <= 0 returns the greedy pick (the row-argmax key,
 * the launch the engine uses) with n_cand = n_kept = 0 and cand[r][*] = -1 */
int gemma_test_sample_rows(const float *logits, int rows, int n_vocab, const gemma_sampler *s_of,
                           const int32_t *positions, int32_t *tokens, int32_t *cand, int32_t *n_cand, int32_t *n_kept);
/* Per-token log-probabilities on the device (DESIGN.md §5b⁗′).  For a logits row l[0..V) (f32) and a
 * token t: M = max_i l[i] compared as floats (-0 == +0); S = sum_i exp((double)l[i] - (double)M) in
 * f64 (an -inf entry contributes 0; S >= 1); logprob(l, t) = ((double)l[t] - (double)M) - log(S), -inf
 * when l[t] is -inf.  This is the raw distribution softmax(l): the sampler's temperature, top-k and
 * top-p do not enter.  Rows with a NaN or whose maximum is -inf are outside the contract.
 * With log-probabilities on, every logits row a pass computes is scored against the token that ends up
 * behind it: the row that processed sequence index p gives lp[p + 1] = logprob(row_p, hist[p + 1]) once
 * the pick or advance has settled hist[p + 1], a given token or the pick alike.  Steps, prefill,
 * prefill_fast, prefill_next (all rows of the pass), verify (the accepted rows) and batch_step (every
 * slot) all score; a prefill of a T-token text scores its tokens 1 .. T-1 plus the appended pick, and
 * the text's perplexity is exp(-mean(lp[1..T))).  lp[i] is NaN where no scored row predicted index i:
 * index 0, indices processed while off, and everything from `keep` on after gemma_engine_extend(keep)
 * (row keep - 1 is not recomputed).  The value depends on the row and the token only, bit for bit: it
 * is the same from eager and graph steps, any split of the steps, a prefill pass or chunk, a verify
 * pass and a batch slot.  Off (the default) nothing is launched; turning it on or off drops the
 * captured decode graph, which then has exactly two more kernels per token.
 * 1 = on, 0 = off, -1 = keep; returns the setting.  -1 + hpc_last_error on a row-split engine (a
 * vocabulary shard per rank, as for the sampler). */
int gemma_engine_set_logprobs(gemma_engine *e, int on);
/* lp of sequence indices [p0, p0+n) of the engine's sequence into out (f64; NaN = not scored);
 * 0 <= p0, p0 + n <= n_seq (the sequence so far: the given tokens, or through the pending pick);
 * returns n; -1 + hpc_last_error, state untouched, on a bad range.  One synchronise. */
int gemma_engine_logprobs(gemma_engine *e, int p0, int n, double *out);
/* the same for an active slot of the open batch */
int gemma_engine_batch_logprobs(gemma_engine *e, int slot, int p0, int n, double *out);
/* per-op test entry: out[r] = logprob(rows[r], tokens[r]) on host rows [rows][n_vocab] through the two
 * kernels of the engine (rows <= 65535, n_vocab <= 2^20, ids in [0, n_vocab)) */
int gemma_test_logprob(const float *logits, int rows, int n_vocab, const int32_t *tokens, double *out);
/* Speculative decoding without a quality trade-off (DESIGN.md §5b‴).  A batched exact pass over
 * [pending token, k drafted tokens] computes the logits rows k + 1 single steps would compute, bit for
 * bit, and a pick depends on its row and position alone (greedy, or the sampler's (seed, p) rule), so
 * accepting the longest correct prefix yields exactly the sequence gemma_engine_step yields.
 * Precondition: the prompt is consumed (pos == n_seq, so hist[pos] is the pending picked token).
 * draft[0..k) are guesses for sequence indices pos+1 .. pos+k (1 <= k <= GEMMA_VERIFY_MAX_DRAFT, ids in
 * [0, n_vocab), pos + k + 1 < n_ctx).  One pass of k + 1 rows at p0 = pos (the Q4_0 / Q8_0 GEMMs on the
 * skinny exact GEMM, weights streamed once), a pick g_i from every row i for index pos + i + 1, then on
 * the device: a = the number of leading i < k with draft[i] == g_i (it stops at the first mismatch,
 * whatever later drafts say); hist[pos+1 .. pos+a+1] = g_0 .. g_a; pos += a + 1; the K / V rows the
 * pass stored for rejected drafts are cleared.  The device state afterwards is byte for byte what
 * a + 1 calls of gemma_engine_step leave, and the captured decode graph is kept.
 * Returns a + 1 (>= 1) with out_tokens[0..a] = g_0 .. g_a (room for k + 1).  logits_all (may be NULL):
 * [k + 1][n_vocab]; rows 0..a are the sequence's own rows, rows past a are returned as computed under
 * the rejected drafts (they belong to no sequence position).  One host synchronise, at the end.
 * -1 with hpc_last_error naming gemma_engine_verify and the state untouched: given tokens still
 * pending, bad k, a bad token id, pos + k + 1 >= n_ctx, a row-split engine (tp_n > 1, a communicator,
 * virtual ranks). */
#define GEMMA_VERIFY_MAX_DRAFT 7
int gemma_engine_verify(gemma_engine *e, const int32_t *draft, int k, int32_t *out_tokens, float *logits_all);
/* test entry: K rows and V columns p0 .. p0+n of one layer's cache, f16 bits; k_rows [n][kvw], v_rows
 * [n][kvw] (V transposed), kvw = n_head_kv * head_dim */
int gemma_engine_kv_read(gemma_engine *e, int layer, int p0, int n, uint16_t *k_rows, uint16_t *v_rows);
/* Batched decode (DESIGN.md §5b⁗): one batch per engine, owned by the engine, of up to
 * GEMMA_BATCH_MAX_SLOTS independent sequences (slots).  Each slot has its own KV caches, history and
 * position; one weight pass (the verify pass's skinny GEMMs, weights streamed once) advances every
 * active slot by one token.  Every slot's logits and tokens are bit for bit what gemma_engine_step gives
 * that sequence alone, and a pick needs its row and position only (greedy, or the sampler in force on
 * the slot with (seed, p): the engine's, or the slot's own, "A sampler per slot" below).  The engine's own
 * sequence, its captured decode graph and its buffers are not touched.
 * Every call returns 0 or a count; -1 with hpc_last_error naming the function and the state untouched
 * on a bad argument.
 *   open     n_slots in [1, 8]: allocates the slots, the pass's tables and its scratch.  Refused: a
 *            batch already open, row-split engines (tp_n > 1, a communicator, virtual ranks), engines
 *            whose decode attention is the position-split form (n_ctx > 2048 or head_dim > 256).
 *   close    frees everything open allocated (gemma_engine_free does so too).
 *   begin    what gemma_engine_begin does, for the slot: caches and history cleared, tokens given,
 *            pos = 0, the slot active (an active slot is restarted).  Same argument checks.
 *   adopt    copies the engine's own sequence into the slot, device to device: caches, history,
 *            position, given-token count, RoPE row — the pending picked token and any
 *            given-but-unprocessed tokens included.  The engine's sequence stays as it is.  (A long
 *            prompt enters a slot at prefill speed: begin, prefill, batch_adopt.)
 *   release  the slot becomes inactive; its memory stays for the next begin / adopt.
 *   step     n passes, each one row per active slot in ascending slot order (R rows, constant within
 *            the call).  Row r processes hist_s[pos_s] of its slot s against that slot's caches and
 *            stores that position's K / V there; if pos_s + 1 >= the slot's given-token count the
 *            row's pick becomes hist_s[pos_s + 1]; pos_s += 1.  All on the device, one host synchronise
 *            at the end.  logits: NULL or [n][R][n_vocab].  Refused: no batch, no active slot, any
 *            active slot with pos + n >= n_ctx (then no slot advances).
 *   pos      processed positions of the slot (-1: inactive).   tokens: the slot's sequence so far, the
 *            pending token included (returns the count).   last: the 8 slots' pending tokens in one
 *            transfer, -1 for inactive slots.   kv_read: gemma_engine_kv_read of the slot's caches.
 * Wide batches: up to GEMMA_BATCH_WIDE_MAX_SLOTS slots.
 *   open_wide  open with n_slots in [1, 64] and the same refusals; every other call works unchanged on
 *            a wide batch (the slot range is [0, n_slots)).  A pass of R <= 8 rows is the pass above; a
 *            pass of more rows runs as one pass on the exact MFMA GEMMs of the batched prefill when
 *            R >= bt_mfma_min (gemma_engine_set_option(e, "bt_mfma_min", v), v in [9, 65], 65 = never),
 *            else as consecutive groups of up to 8 rows.  The same bits in every form.
 *   last_n   the pending tokens of slots [0, n_slots) into out[0 .. n_slots), -1 for inactive slots;
 *            returns n_slots, -1 when cap < n_slots.  gemma_engine_batch_last serves batches of up to 8
 *            slots only (it returns -1 on a wider one).
 * Several rows per slot: a slot that still has given tokens to consume takes the pass's idle rows, so a
 * prompt enters a slot beside the decoding slots instead of one token per pass.
 *   plan_rows  gemma_batch_plan_rows, a pure host function (no GPU), the one statement of the allotment.
 *            need[s] is 0 for an inactive slot, else max(1, given - pos): the slot's given-but-unprocessed
 *            tokens, or 1 when its pending token is a pick.  Every active slot (R of them) gets one row;
 *            the remaining budget max_rows - R is dealt in ascending slot order, extra_s = min(budget,
 *            need[s] - 1).  Writes rows_of[0 .. n_slots) and returns their sum T; -1 on n_slots outside
 *            [1, 64], a negative need, no active slot, or max_rows outside [R, 64].
 *   open_rows  open with n_slots in [1, 64] and the pass scratch, pick keys, sampler workspaces and
 *            log-probability partials sized for max_rows rows, max(8, n_slots) <= max_rows <= 64; the
 *            same refusals as open.  A batch opened by open / open_wide has a row capacity of
 *            max(8, n_slots).
 *   step_rows  one pass of T = plan_rows(need from the slots' positions and given counts, max_rows)
 *            rows, ordered by ascending slot, then ascending position.  Row (s, i), i < m_s, processes
 *            hist_s[pos_s + i], stores that position's K / V in the slot's caches and attends positions
 *            0 .. pos_s + i; then pos_s += m_s, and if the new pos_s >= the slot's given-token count the
 *            last row's pick (greedy, or the sampler with (seed, p = new pos_s)) becomes hist_s[pos_s].
 *            Given tokens are never overwritten; picks of other rows are not used.  With
 *            log-probabilities on, row (s, i) scores hist_s[pos_s + i + 1].  Afterwards every slot's
 *            device state (caches, history, position, given count, RoPE row, token word, lp) is byte for
 *            byte what m_s calls of step(e, 1, ...) leave on it, and every row's logits are the row
 *            those passes compute.  The pass form goes by T as step's goes by R (T <= 8 skinny, T >=
 *            bt_mfma_min one MFMA pass, else groups of up to 8 rows; a slot's rows may straddle groups).
 *            logits: NULL or [T][n_vocab] in row order; rows_of: NULL or [n_slots] (the plan).  Returns
 *            T; one host synchronise at the end.  Refused (-1, no slot advanced): no batch, no active
 *            slot, max_rows below the active count or above the batch's row capacity, any slot with
 *            pos_s + m_s >= n_ctx.
 * A sampler per slot (DESIGN.md §5b⁗ "A sampler per slot"): greedy and sampling slots, each with its own
 * temperature, top_k, top_p and seed, share one pass.
 *   set_sampler  slot in [0, n_slots), active or not.  s == NULL: the slot follows the engine's sampler
 *            (the state after open; later gemma_engine_set_sampler calls included).  s->temperature <= 0:
 *            the slot picks greedily whatever the engine's sampler is.  Else the slot samples with its
 *            own parameters by the rule at gemma_engine_set_sampler, p the sequence index of the pick.
 *            The parameters reach the device by a stream-ordered copy into memory the batch owns (the
 *            slot's rows of the pass tables), ahead of the next pass: they govern every pick enqueued
 *            after the call.  The setting belongs to the slot: it survives begin, adopt, release and fork and
 *            ends with close.  The checks are gemma_engine_set_sampler's; a sampler workspace the batch
 *            needs and lacks (a narrow batch on an engine whose sampler was never on) is allocated now
 *            and freed by close.  Refused (-1, naming the function and the field, the state untouched):
 *            no batch, a slot outside the range, a bad field, a failed allocation.
 *   sampler  returns 1 when the slot's picks sample, 0 when they are greedy; *out = the parameters in
 *            force, *own = 1 for a setting of the slot's own, 0 when it follows the engine (either may
 *            be NULL).  -1: no batch, a bad slot.
 *   fork     dst becomes a device-to-device copy of the active slot src's sequence: caches, history,
 *            log-probabilities, position, given-token count, RoPE row, the pending token and any
 *            given-but-unprocessed tokens; dst is active afterwards, src unchanged.  The sampler settings
 *            are not copied: each slot keeps its own, so n samples of a prompt cost one prefill (begin,
 *            prefill, adopt, fork n - 1 times, a seed per slot).  A copy, not a shared prefix.  Refused
 *            (-1, nothing changed): no batch, a slot outside the range, src inactive, src == dst.
 * The guarantee: whatever the other slots do, a slot's logits rows, tokens, caches, history and
 * log-probabilities are bit for bit what a plain engine gives that sequence through gemma_engine_step
 * with gemma_engine_set_sampler set to the sampler in force on the slot at each pick.  It holds for
 * step, step_rows, gemma_engine_batch_verify (row (s, i) picks with slot s's sampler at p = pos_s + i + 1)
 * and gemma_engine_batch_generate_lookup, in every pass form (skinny, groups of 8, MFMA).  A greedy
 * slot's pick is the engine's greedy pick as it stands, not the sampler with top_k = 1: the two orders
 * differ on a signed-zero tie (the sampler's key folds -0 into +0, the argmax key does not).
 * The pick launches of a pass depend on the mix alone, decided on the host: no participating slot
 * samples, the one row-argmax launch; all sample, the sampler's three; else both, four. */
#define GEMMA_BATCH_MAX_SLOTS 8
#define GEMMA_BATCH_WIDE_MAX_SLOTS 64
int gemma_engine_batch_open(gemma_engine *e, int n_slots);
int gemma_engine_batch_close(gemma_engine *e);
int gemma_engine_batch_begin(gemma_engine *e, int slot, const int32_t *tokens, int n);
int gemma_engine_batch_adopt(gemma_engine *e, int slot);
int gemma_engine_batch_release(gemma_engine *e, int slot);
int gemma_engine_batch_step(gemma_engine *e, int n, float *logits);
int gemma_engine_batch_pos(gemma_engine *e, int slot);
int gemma_engine_batch_tokens(gemma_engine *e, int slot, int32_t *out, int cap);
int gemma_engine_batch_last(gemma_engine *e, int32_t *out8);
int gemma_engine_batch_kv_read(gemma_engine *e, int slot, int layer, int p0, int n, uint16_t *k_rows, uint16_t *v_rows);
int gemma_engine_batch_open_wide(gemma_engine *e, int n_slots);
int gemma_engine_batch_last_n(gemma_engine *e, int32_t *out, int cap);
int gemma_batch_plan_rows(const int32_t *need, int n_slots, int max_rows, int32_t *rows_of);
int gemma_engine_batch_open_rows(gemma_engine *e, int n_slots, int max_rows);
int gemma_engine_batch_step_rows(gemma_engine *e, int max_rows, float *logits, int32_t *rows_of);
int gemma_engine_batch_set_sampler(gemma_engine *e, int slot, const gemma_sampler *s);
int gemma_engine_batch_sampler(gemma_engine *e, int slot, gemma_sampler *out, int *own);
int gemma_engine_batch_fork(gemma_engine *e, int src, int dst);
/* Drafts in the batch (DESIGN.md §5b⁗ "Drafts in the batch"): gemma_engine_verify for the slots of the
 * open batch, all in one exact pass.  draft is [n_slots][GEMMA_VERIFY_MAX_DRAFT], k_of [n_slots]; k_of[s]
 * is read for active slots only:
 *   -1      the slot sits this pass out: it takes no row and not a byte of its state changes.
 *   0       one row, exactly batch_step's row for that slot (it may still be consuming given tokens:
 *           a given token is never overwritten).
 *   1 .. 7  the slot's given tokens must be consumed (pos_s >= given_s, pos_s >= 1); draft[s][0 .. k_s)
 *           are guesses for sequence indices pos_s + 1 .. pos_s + k_s.
 * The pass has T = sum (1 + k_s) rows over the participating slots, ordered by ascending slot, then
 * ascending position.  Row (s, i) processes hist_s[pos_s] for i = 0, else draft[s][i - 1], at position
 * pos_s + i: it stores that position's K / V in the slot's caches and attends positions 0 .. pos_s + i.
 * Every row gives a pick g_{s,i} for index pos_s + i + 1 (greedy, or slot s's sampler with (seed,
 * p = pos_s + i + 1)).  Then on the device, per slot: a_s = the number of leading i < k_s with
 * draft[s][i] == g_{s,i} (it stops at the first mismatch); hist_s[pos_s + 1 .. pos_s + a_s + 1] =
 * g_{s,0 .. a_s} (a given token stands); the rejected drafts behind them are zeroed in hist; pos_s +=
 * a_s + 1; the slot's token word, pending-token entry and RoPE row follow; K rows and V columns of the
 * rejected rows go back to zero in every layer.  With log-probabilities on, rows 0 .. a_s score
 * hist_s[pos_s + i + 1]; rejected rows write nothing.  Afterwards each participating slot's device state
 * (caches, history, position, given count, RoPE row, token word, lp) is byte for byte what a_s + 1 calls
 * of batch_step(e, 1, ...) leave on it, and a following batch_step, batch_step_rows or batch_verify
 * continues from it.  The pass form goes by T exactly as step_rows' does, the same bits in each.
 * out_tokens is [n_slots][GEMMA_VERIFY_MAX_DRAFT + 1]: out_tokens[s][0 .. a_s] = g_{s,0 .. a_s};
 * n_out[s] = a_s + 1 for a participating slot, 0 otherwise.  logits: NULL or [T][n_vocab] in row order;
 * rows past a_s are returned as computed under the rejected drafts.  Returns T; one host synchronise, at
 * the end.  Refused (-1, hpc_last_error naming gemma_engine_batch_verify, no slot advanced, the state
 * untouched): no batch open; a null draft, k_of, out_tokens or n_out; k_of[s] outside [-1, 7]; no
 * participating slot; k_s >= 1 on a slot with given tokens pending or at pos 0; a used draft id outside
 * [0, n_vocab); pos_s + k_s + 1 >= n_ctx; T above the batch's row capacity (max(8, n_slots), or
 * open_rows' max_rows). */
int gemma_engine_batch_verify(gemma_engine *e, const int32_t *draft, const int32_t *k_of,
                              int32_t *out_tokens, int32_t *n_out, float *logits);
/* Prompt-lookup draft for the sequence seq[0..n) (pure host function, no GPU): for g = min(ngram_max,
 * n - 1) down to 1, the largest s < n - g with seq[s..s+g) == seq[n-g..n); the first g with a match
 * wins and the draft is seq[s+g .. min(s+g+k, n)).  Returns its length (0: no g matches), -1 on
 * ngram_max < 1 or k outside [1, GEMMA_VERIFY_MAX_DRAFT]. */
int gemma_lookup_draft(const int32_t *seq, int n, int ngram_max, int k, int32_t *out);
/* passes: verify calls; drafted / accepted: draft tokens sent / accepted; plain_steps: graph steps taken
 * when no draft existed.  Tokens appended = passes + accepted + plain_steps. */
typedef struct gemma_spec_stats { int passes, drafted, accepted, plain_steps; } gemma_spec_stats;
/* n_new tokens by lookup drafts: the sequence (the pending token included) is mirrored on the host,
 * drafted from with gemma_lookup_draft, and a draft is verified (else one graph step runs).  A draft is
 * grown to k tokens by repeated lookups (what a lookup drafted is appended as a guess and the rule
 * applied again: one lookup stops at the sequence end) and shortened so that never more than n_new
 * tokens are appended.  out[0..n_new) and the final pos equal
 * gemma_engine_step(n_new) token for token, sampler on or off.  0, or -1 with hpc_last_error. */
int gemma_engine_generate_lookup(gemma_engine *e, int n_new, int k, int ngram_max, int32_t *out, gemma_spec_stats *stats);
/* The same loop for every active slot of the open batch, the passes gemma_engine_batch_verify's.  out is
 * [n_slots][n_new] (rows of inactive slots are not written), stats [n_slots] or NULL.  Every active slot
 * must have its prompt consumed, and every active slot gets exactly n_new tokens.  Per pass and per
 * unfinished slot the draft is grown from the slot's host mirror by the rule above, capped at min(k,
 * n_new - done_s - 1) and dropped when it would not fit n_ctx; when the pass's rows exceed the batch's row
 * capacity the drafts are cut by gemma_batch_plan_rows(need = 1 + draft length, capacity); finished
 * slots sit out (-1).  out[s] and each slot's final position equal what batch_step gives that slot, token
 * for token, sampler on or off.  Per slot: passes = passes in which it carried a draft, plain_steps =
 * passes in which it carried none; tokens appended = passes + accepted + plain_steps = n_new.  0, or -1
 * with hpc_last_error naming gemma_engine_batch_generate_lookup: no batch, no active slot, bad n_new / k /
 * ngram_max, a slot with given tokens pending, or pos_s + n_new >= n_ctx for a slot. */
int gemma_engine_batch_generate_lookup(gemma_engine *e, int n_new, int k, int ngram_max,
                                       int32_t *out, gemma_spec_stats *stats);
/* weights back in ggml row-major layout (tests); tid as in DESIGN.md §Synthetic weights */
int64_t gemma_engine_tensor(gemma_engine *e, int tid, void *dst, int64_t cap);
/* time `iters` launches of one hot kernel with hipEvents on the engine stream; returns avg µs and
 * the algorithmic bytes (or int-ops) per launch.  which: 0 = ffn gate/up matvec, 1 = ffn down,
 * 2 = qkv, 3 = attn out, 4 = output/logits, 5 = whole decode step (graph) */
double gemma_engine_time(gemma_engine *e, int which, int iters, double *algo_bytes);
int gemma_engine_sync(gemma_engine *e);
/* launch plan per matrix class (0 qkv, 1 attn-out, 2 gate/up, 3 down, 4 logits): K split and
 * row-tile groups per workgroup.  tune: coordinate descent over whole decode steps (hipGraph
 * replays of `iters` tokens per candidate); bit-identical results for every plan; clobbers the
 * decode state (call gemma_engine_begin afterwards).  plan/set_plan: 2 ints per class. */
int gemma_engine_tune(gemma_engine *e, int iters);
int gemma_engine_plan(gemma_engine *e, int *out, int cap);
int gemma_engine_set_plan(gemma_engine *e, const int *in, int n);
int gemma_engine_set_fuse(gemma_engine *e, int fuse_front); /* fused layer front on/off (-1 = keep); returns the hand-off timeout word */
/* the decode attention and attn-out (+ residual) in ONE launch per layer (k_attn_o: the attention
   launch's idle workgroups run attn-out's row tiles after an in-launch hand-off; same bits): on 1 /
   off 0 / keep -1; returns the setting.  A hand-off timeout is reported by gemma_engine_step (-1) and
   turns it off. */
int gemma_engine_set_att_o(gemma_engine *e, int on);
/* The measured variants that stay selectable (tests, A/B), set through the API rather than the
   environment: "kq_fuse" (K-quant Q8_K INIT plan 0..6), "kq_dual" (gate+up one launch), "kq_pair"
   (q|k and v one launch), "kq_abl" (timing ablation, wrong results), "att_mx" (exact prefill attention
   on the f32 matrix cores; 0 = the row form), "att_dsplit" (decode attention workgroups per head:
   1/2/4/8), "ks_small" / "ks_down" (launch-plan K split defaults), "grid_big", "bt_mfma_min" (rows
   from which a wide batch pass runs as one MFMA pass, [9, 65], 65 = never; default 29, measured), and the
   gemma_engine_time diagnostics "time_hot" / "ablate" (a non-zero "ablate" needs the -DGHIP_ABLATE=1
   build of the library: the product kernels do not read it).  Returns 0, -1 (unknown name or bad value). */
int gemma_engine_set_option(gemma_engine *e, const char *name, int value);
int gemma_engine_graph_kernels(gemma_engine *e);            /* kernel launches per decode token (captured graph) */
/* the decode step's layers as ONE persistent launch (opt-in: off by default, GHIP_PERSIST=1 or this
 * call; -1 = keep): returns 1 when it runs this engine's steps, 0 when not (hpc_last_error says why:
 * K-quant layers, row-split TP, shapes).  A hand-off timeout inside the launch (a workgroup not
 * co-resident) is reported: gemma_engine_step returns -1 (restart the sequence), the ggml executor's
 * decode redoes the token on the per-layer launches; either way the engine leaves the launch off. */
int gemma_engine_set_persist(gemma_engine *e, int on);
/* its sticky hand-off timeout words [flag, site, layer]; returns the flag (0 = none); reset clears */
int gemma_engine_persist_err(gemma_engine *e, int *out3, int reset);
/* tests: the launch's per-wait bound in 100 MHz ticks (0 = default 20 ms) */
int gemma_engine_set_persist_timeout(gemma_engine *e, unsigned ticks);
/* debugging: one eager step with per-layer taps [n_layer][qkv | attn_out | layer_out] */
int gemma_engine_debug_step(gemma_engine *e, float *host_taps, float *logits);
/* diagnostics: prefill (exact != 0: the exact path) with the residual stream after each layer
 * -> [n_layer][T][n_embd] */
int gemma_engine_prefill_taps(gemma_engine *e, float *host_taps, int exact);
/* diagnostics: one eager step with s_memrealtime phase stamps (100 MHz) of layer `layer`'s five
 * kernels (regions 0..4: qkv, attention, attn-out, gate/up, down) and the logits kernel (region 5);
 * out = 6 * 4096 * 16 u64, slot [region][workgroup][phase], unused slots 0 */
int gemma_engine_stamp_step(gemma_engine *e, int layer, unsigned long long *out);
/* diagnostics: one eager step through the persistent launch with its phase stamps
 * -> out [n_embd / 8][n_layer][16] u64 + 256 per-pop probes (GHIP_STAMPS build) */
int gemma_engine_token_stamps(gemma_engine *e, unsigned long long *out);
/* per-op test entry: one decode-attention block on host buffers (caches updated in place);
 * mode 0 = one workgroup per head, 1 = position-split form with the in-kernel hand-off */
int gemma_test_attn_decode(const float *qkv, uint16_t *kc, uint16_t *vc, int pos, int H, int Hkv, int hd, int ctx,
                           float rope_base, float *out, float *dbg_w, uint16_t *dbg_p, float *dbg_inv,
                           unsigned long long *dbg_t, int mode);
/* per-op test entry: the prefill's RoPE / q scale / KV store kernel on host buffers.  qkv [T][ldqkv] f32 rows
 * q | k | v (pre-RoPE) of positions p0 .. p0 + T - 1; q16_out [T][H][hd] f16 (q x 1/sqrt(hd)); kc_inout
 * [ctx][Hkv*hd] and vc_inout [Hkv*hd][ctx] f16, copied in, rows / columns p0 .. p0 + T - 1 written, copied back */
int gemma_test_rope_kv_prefill(const float *qkv, int64_t ldqkv, int T, int p0, int H, int Hkv, int hd, int ctx,
                               float rope_base, uint16_t *q16_out, uint16_t *kc_inout, uint16_t *vc_inout);
/* the same K / V store through the batch pass's restatement of that kernel (k_rows_rope_kv): one row-table entry
 * per row, 1 <= T <= 64, every row on the same caches; q is not touched by that kernel */
int gemma_test_rows_rope_kv(const float *qkv, int64_t ldqkv, int T, int p0, int H, int Hkv, int hd, int ctx,
                            float rope_base, uint16_t *kc_inout, uint16_t *vc_inout);
/* per-op test entry: one causal prefill attention launch on host buffers.  q16 [T][H][hd], kc [ctx][Hkv*hd],
 * vc [Hkv*hd][ctx] f16; row t is position p0 + t; n_kv = the padded key count of the last row (<= ctx).
 * form 0 = the exact rows kernel, 1 = the exact f32 matrix-core kernel, 2 = the approximate f16 MFMA kernel.
 * out [T][ldo] f32 is copied to the device before the launch and back after it, so columns [H*hd, ldo) keep
 * the caller's values.  A shape the form refuses: non-zero with the launcher's message, out untouched */
int gemma_test_attn_prefill(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, int T, int p0, int H, int Hkv,
                            int hd, int ctx, int n_kv, int64_t ldo, int form, float *out);
/* per-op test entry: R decode-attention rows through ONE launch form on host buffers.
 * form 0 the per-head kernel (with dsplit), 1 the position-split kernel, 2 the batch pass's one-row-per-slot
 *      kernel, 3 the several-rows-per-slot pair (the K / V store launch, then the attention on cached K / V).
 * Row r: q | k | v at qkv + r * ldqkv (pre-RoPE), position pos[r] in [0, ctx), caches of slot[r] in [0, n_slots).
 * Forms 0 and 1 run the rows as R successive launches (form 1 on one scratch allocation: sync_out receives the
 * hand-off counters' 2 * Hkv words after the last launch, err_out the sticky timeout word).  Form 2 is one
 * launch and needs distinct slots.  Form 3 is one pair of launches: rows of a slot adjacent, at consecutive
 * positions.  RoPE: rope_identity != 0 publishes cos 1 / sin 0 rows (and tables), else rope_base's.
 * kc / vc [n_slots][ctx * Hkv * hd] f16 and out [R][H * hd] are copied in before and back after the launches;
 * dbg_w f32 / dbg_p f16 [R][H][ctx] (optional; forms 2 and 3: R == 1 only); img_act u32 [R][ceil(H * hd / 128)
 * * 32] + img_da f32 [R][H * hd / 32] (optional, both or neither: the Q8_0 image of out) and img_q8k u8
 * [R][H * 292] (optional: its Q8_K image) are copied in and back too.  nwg: form 1's workgroups per kv head, 0 =
 * the geometry's own.  Bad arguments: -1 with a message; a shape the launcher refuses: non-zero with the
 * launcher's message; in both cases nothing is copied back */
typedef struct gemma_test_attn_rows_args {
    int form, R, n_slots, H, Hkv, hd, ctx, dsplit, nwg;
    int rope_identity;
    float rope_base, q_scale;
    const float *qkv;
    int64_t ldqkv;
    const int *pos, *slot;
    uint16_t *kc, *vc;
    float *out;
    float *dbg_w;
    uint16_t *dbg_p;
    uint32_t *img_act;
    float *img_da;
    uint8_t *img_q8k;
    int *sync_out;
    int err_out;
} gemma_test_attn_rows_args;
int gemma_test_attn_decode_rows(gemma_test_attn_rows_args *a);
/* per-op test entry: R rows through the long form of the batch pass's attention (attn_long.hip: k_rows_rope_kv, then
 * the scores, softmax and KQV launches; n_ctx up to 8192) as ONE call of its launcher, on the struct above.  form must be 0;
 * dsplit, nwg, img_*, sync_out are not used (the images must be NULL).  Rows may share a slot at distinct
 * positions (the K / V stores of all rows precede every read).  dbg_w f32 and dbg_p f16 [R][H][ctx] are required
 * and receive the form's scratch, by head: before the launches the entry fills the scores scratch with
 * GEMMA_TEST_ATTN_LONG_W_FILL and the P16 scratch with GEMMA_TEST_ATTN_LONG_P_FILL (large finite values: a stale
 * word that is read wins the max and changes every output), so what the kernels did not write reads back as
 * the fill.  kc / vc / out are copied in and back as above.  Bad arguments: -1 with a message; a shape or a pass
 * the launcher refuses: non-zero with its message; in both cases nothing is copied back */
#define GEMMA_TEST_ATTN_LONG_W_FILL 3.0e38f
#define GEMMA_TEST_ATTN_LONG_P_FILL 0x7BFF
int gemma_test_attn_long_rows(gemma_test_attn_rows_args *a);

/* per-op test entry: the prefill path's Q8_0 row quantization + int8 MFMA GEMM on host buffers */
int gemma_test_gemm(int type, int64_t rows, int64_t K, int64_t T, const void *W, const float *X, float *Y,
                    int8_t *xq_out, float *da_out);
/* the same with the exact (ggml AVX2 lane order) GEMM of the exact prefill */
int gemma_test_gemm_exact(int type, int64_t rows, int64_t K, int64_t T, const void *W, const float *X, float *Y,
                          int8_t *xq_out, float *da_out);
/* the same product for 1 <= T <= 8 rows through the skinny exact GEMM of the verify pass (each weight
 * tile loaded once for all T columns): Y[T][rows] = W x Q8_0(X) (+ resid [T][rows], may be NULL);
 * bit-identical to gemma_test_gemm_exact and mul_mat.  T outside [1, 8]: -1 with hpc_last_error */
int gemma_test_gemm_skinny(int type, int64_t rows, int64_t K, int64_t T, const void *W, const float *X,
                           const float *resid, float *Y);
/* per-op test entry: ONE decode matvec launch (either form) on host buffers, every argument of the
 * launch set by the caller, so that a test can make each of them distinguishable.
 * pro: 0 x = ncols columns of K floats (x_stride floats apart), 1 the same through rms_norm * norm_w,
 *      2 x = ncols rows of ggml block_q8_0 [K/32] (x_stride bytes apart),
 *      3 x = int32 tokens[n_tok], the row tokens[tok_pos] of emb (ggml rows [emb_rows][K/32] of `type`)
 *      * emb_scale through rms_norm * norm_w, 4 x = the Q8_0 activation image u32 [K/4] + x_da f32 [K/32]
 * epi: 0 y = dot, 1 y = dot + resid, 2 y = gelu(W . x) * (W2 . x), 3 y = dot and keys[ncols][grid]
 * ks:  1 / 2 / 4 / 8 waves per row tile over `grid` workgroups, 9 the round-pipelined form */
typedef struct gemma_test_matvec_args {
    int type, ks, pro, epi, ncols, grid;
    int64_t rows, K;
    const void *W, *W2;          /* ggml row-major blocks [rows][K/32] */
    const void *x;
    int64_t x_stride;
    const float *x_da, *norm_w;
    float eps, emb_scale;
    int n_tok, tok_pos;
    const void *emb;
    int64_t emb_rows;
    float *emb_out;              /* pro 3, optional: the scaled embedding row [K] */
    const float *resid;          /* epi 1: ncols columns y_stride floats apart */
    int64_t y_stride;
    float *y;                    /* ncols columns y_stride floats apart ((ncols - 1) * y_stride + rows floats) */
    unsigned long long *keys;    /* epi 3 */
} gemma_test_matvec_args;
int gemma_test_matvec(const gemma_test_matvec_args *a);
/* the same launch with the GELU clamp (epi 2) selectable and, when img_act / img_da are given (epi 2, ks 1,
 * ncols 1, rows % 32 == 0), the Q8_0 image of y the launch also writes: img_act u32 [ceil(rows / 128) * 32] in
 * the activation image's layout (whole groups of 4 blocks), img_da f32 [rows / 32] */
int gemma_test_matvec_tail(const gemma_test_matvec_args *a, int gelu_clamp, uint32_t *img_act, float *img_da);
/* K-quant matvec (Q4_K / Q6_K x Q8_K) timed alone: avg µs per launch over
 * `iters` launches rotating over cold weight copies; *algo_bytes = weights + Q8_K column + y */
double gemma_kq_time(int type, int64_t rows, int64_t K, int iters, double *algo_bytes);
/* measured HBM read roofline: streaming read of `bytes` on `device`, `iters` passes; GB/s — the
   faster of the two probes below */
double gemma_hbm_read_gbs(int device, size_t bytes, int iters);
/* one probe: variant 0 = 16-B nontemporal loads into registers, 1 = LDS-DMA (global_load_lds nt) */
double gemma_hbm_read_probe(int device, size_t bytes, int iters, int variant);
/* per-op test entry: the softmax's exp(f16) for all 65536 codes (compared with ggml's table) */
int gemma_test_exp_f16(uint16_t *out);
/* per-op test entry: one rms_norm kernel on host rows (ggml rms_norm):
 * kind 0 the ggml executor's RMS_NORM (out f32 rows), kind 1 k_norm_q8K (rms_norm * w, then
 * quantize_row_q8_K; out Q8_K rows) */
int gemma_test_rms_norm(int kind, const float *x, const float *w, int rows, int n, float eps, void *out);

#ifdef __cplusplus
}
#endif
#endif
