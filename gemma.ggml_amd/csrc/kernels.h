// kernels.h — launch wrappers for the gfx950 kernels (host-callable, no torch types).
#pragma once

#include <vector>

#include "common.h"

namespace ghip {

// the tiled weight matrix (tiled_mat, common.h) of a launch: the six fields an mv_args, a gemm_args
// or any other argument struct names it by
template <typename A> inline void set_mat(A &a, const tiled_mat &m) {
    a.qs = m.qs; a.sc = m.sc; a.rows = m.rows; a.n_rt = m.n_rt; a.n_bt = m.n_bt; a.nb = m.nb;
}

// ---- decode matvec (matvec.hip) ----------------------------------------------------------------
// Prologue: how the activation column is turned into the LDS Q8_0 image.
enum mv_pro : int {
    PRO_F32 = 0,    // x: f32[K] -> quantize_row_q8_0 (AVX2 semantics)
    PRO_NORM = 1,   // x: f32[K] -> rms_norm(x)*norm_w (A.5) -> quantize
    PRO_Q8 = 2,     // x: ggml block_q8_0[K/32] (the C-ABI `wdata`, already converted by ggml INIT)
    PRO_EMBED = 3,  // x: int32 sequence, token = x[*tok_pos]; embedding row (tiled) * emb_scale -> norm
    PRO_IMG = 4,    // x: the Q8_0 activation image its producer already wrote (act u32 [nb/4][8][4]
                    //    + x_da f32 [nb]; DESIGN.md §Activation image): a copy into LDS
};
enum mv_epi : int {
    EPI_STORE = 0,     // y[r] = dot
    EPI_ADD = 1,       // y[r] = dot + resid[r]          (ggml_add, src/gemma_model.cpp:723,731)
    EPI_GELU_MUL = 2,  // y[r] = gelu(dotA) * dotB       (src/gemma_model.cpp:446-449)
    EPI_ARGMAX = 3,    // y[r] = dot and argmax key      (greedy_sample, :532-546)
};

struct mv_args {
    const uint8_t *qs = nullptr, *sc = nullptr;    // weights (tiled)
    const uint8_t *qs2 = nullptr, *sc2 = nullptr;  // second matrix for EPI_GELU_MUL (ffn_up)
    int64_t rows = 0, n_rt = 0, n_bt = 0, nb = 0;  // nb = K/32
    const void *x = nullptr;                       // activation (see mv_pro)
    const float *x_da = nullptr;                   // PRO_IMG: the image's block scales
    int64_t x_col_stride = 0;                      // bytes between columns (multi-column launch)
    const float *norm_w = nullptr;
    float eps = 0.f;
    // PRO_EMBED: embedding source
    const int *tok_pos = nullptr;
    const uint8_t *emb_qs = nullptr, *emb_sc = nullptr;
    int64_t emb_n_bt = 0;
    float emb_scale = 1.f;
    float *emb_out = nullptr;                      // if set, block 0 writes the scaled embedding row
    // epilogue
    float *y = nullptr;
    int64_t y_col_stride = 0;                      // floats between columns
    const float *resid = nullptr;
    const uint16_t *gelu_tab = nullptr;
    int gelu_clamp = 0;
    unsigned long long *argmax_key = nullptr;      // EPI_ARGMAX: one partial key per workgroup [grid]
    uint32_t *out_act = nullptr;                   // EPI_GELU_MUL: also write y's Q8_0 image (the
    float *out_da = nullptr;                       //   next matvec's PRO_IMG input), blocks of y
    int ncols = 1;
    int ablate = 0;  // timing-only ablations (bench): 1 = no prologue, 4 = no carry, 8 = no gate/up dots
    unsigned long long *dbg_t = nullptr;  // diagnostics: 8 s_memrealtime stamps per workgroup
    // launch geometry precomputed by launch_t (no 64-bit divisions in the kernel prologue):
    // a wave's row-tile count is rt_q + (rt0 < rt_r); ygroups = EPI_GELU_MUL image groups per WG
    int64_t rt_q = 0, rt_r = 0, ygroups = 0;
};

// ks: waves that split one row tile's K range (ordered carry hand-off); 1 = one wave per tile.
// ks = KS_RR: the round-pipelined form (matvec_rr.hip): 8 loader waves interleaved over K + a carrier
// wave that runs the chains one round behind the loads; one workgroup per row tile (grid_x ignored).
constexpr int KS_RR = 9;
int launch_matvec(int wtype, int ks, int pro, int epi, const mv_args &a, int grid_x, hipStream_t s);
bool matvec_rr_supported(int wtype, int64_t n_bt);
size_t matvec_lds_bytes(int wtype, int ks, int64_t n_bt, int64_t segment_tiles);

// ---- ggml graph executor kernels (ggml_ops.hip) ----------------------------------------------------
struct gt_desc {  // a device view of a ggml tensor: data, ne, nb (bytes), type
    char *data = nullptr;
    int64_t ne[4] = {1, 1, 1, 1};
    int64_t nb[4] = {0, 0, 0, 0};
    int type = T_F32;
};
int launch_g_get_rows(const gt_desc &src, const gt_desc &idx, const gt_desc &dst, hipStream_t s);
int launch_g_elementwise(int op, const gt_desc &a, const gt_desc &b, const gt_desc &dst, float scale,
                         const uint16_t *gelu_tab, int gelu_clamp, hipStream_t s);
int launch_g_rms_norm(const gt_desc &a, const gt_desc &dst, float eps, hipStream_t s);
int launch_g_rope_neox(const gt_desc &a, const gt_desc &pos, const gt_desc &dst, int n_dims, const float *cs,
                       const float *sn, hipStream_t s);
int launch_g_soft_max(const gt_desc &a, const gt_desc &mask, int has_mask, const gt_desc &dst, float scale, hipStream_t s);
int launch_g_copy(const gt_desc &src, const gt_desc &dst, hipStream_t s);
int launch_g_mul_mat_f16(const gt_desc &a, const uint16_t *b16, int64_t ne10, const gt_desc &dst, int64_t ne11,
                         int64_t ne12, int64_t ne13, hipStream_t s);
// host tables and tiled weights shared with the engine (engine.cpp)
void build_f16_tables(std::vector<uint16_t> &exp_t, std::vector<uint16_t> &gelu_t);
void build_rope(int ctx, int hd, float base, std::vector<float> &c, std::vector<float> &s);
// both planes from `mem`, zeroed on s; -1 (error set, nothing kept) when an allocation fails
int alloc_tiled(dev_pool &mem, tiled_mat *out, int type, int64_t rows, int64_t K, hipStream_t s);
// for the cache owners that drop single entries (an engine's matrices go with its pool)
void free_tiled(dev_pool &mem, tiled_mat &m);
// capi.cpp: the C-ABI weight cache's tiled copy of a host weight (hpc_register_weight / mul_mat)
bool registered_tiled(const void *host, int type, int64_t K, tiled_mat *out);

// ---- K-quant matvec (kquant.hip) -----------------------------------------------------------------
struct kq_args {  // y[c][r] = vec_dot_{q4_K,q6_K}_q8_K(row r of w, column c of x), ggml AVX2 lane order
    const uint8_t *w = nullptr;   // ggml row-major super-blocks, row_bytes per row
    int64_t row_bytes = 0, rows = 0;
    int nsb = 0;                  // super-blocks per row (K / 256)
    const uint8_t *x = nullptr;   // Q8_K columns (292 B per super-block), x_col_stride bytes apart
    int64_t x_col_stride = 0;
    float *y = nullptr;
    int64_t y_col_stride = 0;     // floats between output columns
    int ncols = 1;
    // epilogue (engine K-quant layers): y = v + resid (ggml_add), or y = gelu(gate_in) * v (ffn_up)
    const float *resid = nullptr, *gate_in = nullptr;
    const uint16_t *gelu_tab = nullptr;
    int gelu_clamp = 0;
    // fused INIT (no separate Q8_K launch): pro = KQP_F32 quantizes f32 columns xf, KQP_NORM
    // quantizes rms_norm(xf)*norm_w (k_norm_q8K's bytes); KQP_COPY reads the Q8_K columns x
    int pro = 0;
    const float *xf = nullptr;
    int64_t xf_col_stride = 0;    // floats
    const float *norm_w = nullptr;
    float eps = 0.f;
    // fused ffn gate/up: w = gate, w2 = up (same type and shape), y = gelu(gate) * up
    const uint8_t *w2 = nullptr;
    // producer-side INIT of the NEXT matvec (y stored write-through, then a per-wave count):
    // q8_mode = KQO_QUANT: each 256-row super-block of y quantized to Q8_K by the wave completing it;
    // KQO_NORM: rms_norm(y)*q8_norm (eps) quantized by the wave completing the whole column.
    // q8_out: Q8_K columns ((rows/256)*292 B apart); q8_cnt: zero-initialised counters, 32 u32 apart,
    // q8_cnt_cap of them per launch (left zero)
    int q8_mode = 0;
    uint8_t *q8_out = nullptr;
    unsigned *q8_cnt = nullptr;
    int q8_cnt_cap = 0;
    const float *q8_norm = nullptr;
    int q8_abl = 0;  // timing ablation only (wrong bytes): 1 no tail work, 2 no counting, 4 plain stores
    int tiled = 0;   // w (and w2) in the lane-contiguous layout of launch_kq_retile
    unsigned long long *dbg_t = nullptr;  // stamps build: 16 s_memrealtime per workgroup (k_matvec_kq)
};
// ggml K-quant rows <-> the lane-contiguous device layout the matvec reads with one vector load per
// lane (Q4_K any K % 256 == 0, Q6_K K % 2048 == 0); src != dst
int launch_kq_retile(int wtype, const uint8_t *src, uint8_t *dst, int64_t rows, int64_t K, bool to_tiled, hipStream_t s);
enum kq_prologue_mode { KQP_COPY = 0, KQP_F32 = 1, KQP_NORM = 2 };
enum kq_handoff_mode { KQO_NONE = 0, KQO_QUANT = 1, KQO_NORM = 2 };
int launch_matvec_kq(int wtype, const kq_args &a, hipStream_t s);
// two K-split matvecs over one input column in one launch (e.g. q|k and v; types may differ)
int launch_matvec_kq2(int t1, const kq_args &a, int t2, const kq_args &b, hipStream_t s);
// ggml quantize_row_q8_K of ncols rows of K floats (row stride ldx floats) -> Q8_K rows ld_out bytes apart
int launch_quant_q8_K(const float *x, int64_t ldx, int64_t K, int ncols, uint8_t *out, int64_t ld_out,
                      hipStream_t s);
// rows of rms_norm(x)*w quantized to Q8_K (the tied output's INIT when token_embd is Q6_K)
int launch_norm_q8K(const float *x, int64_t ldx, const float *w, int E, float eps, int rows, uint8_t *out,
                    int64_t ld_out, hipStream_t s);
// T rows of get_rows(Q6_K token_embd, tokens)*scale; token of row t: tokens[*pos] if pos else tokens[t]
int launch_embed_q6K(const uint8_t *embd, int64_t row_bytes, const int *tokens, const int *pos, int T, int E,
                     float scale, float *out, hipStream_t s, bool tiled = false);
// synthetic Q4_K / Q6_K rows: oracle orc_synth_kquant(seed) with d (and dmin) rescaled by f
int launch_synth_kquant(int wtype, uint8_t *out, int64_t rows, int64_t K, uint64_t seed, float f, hipStream_t s);

// ---- K-quant prefill GEMM (prefill_kq.hip) -------------------------------------------------------
// T Q8_K columns -> the operand image of k_gemm_kq: xh f16 [T][ldh] with each super-block's 256
// values in AVX2-lane-major order (position 32l + 4c + k holds value 32c + 4l + k), xd f32 [T][ldd]
// (the super-block's d), xm [T][ldm][16] f16 (Q4_K mins operand: per k = 0..3 the pair sums
// S0 = bs[4k]+bs[4k+1], S1 = bs[4k+2]+bs[4k+3] as S & 63, S1 & 63, S0 >> 6, S1 >> 6)
struct q8kx_args {
    const uint8_t *x = nullptr;
    int64_t x_col_stride = 0;
    int nsb = 0, T = 0;
    uint16_t *xh = nullptr;
    int64_t ldh = 0;
    float *xd = nullptr;
    int64_t ldd = 0;
    uint16_t *xm = nullptr;
    int64_t ldm = 0;
};
int launch_q8k_expand(const q8kx_args &a, hipStream_t s);
// y[t][r] = vec_dot_{q4_K,q6_K}_q8_K(row r, column t) for all T columns, ggml AVX2 lane order, on
// v_mfma_f32_32x32x16_f16
struct kqg_args {
    const uint8_t *w = nullptr;
    int64_t row_bytes = 0, rows = 0;
    int nsb = 0, T = 0;
    int tiled = 1;  // w in launch_kq_retile's layout (Q6_K: K % 2048 == 0), else ggml's row-major blocks
    const uint16_t *xh = nullptr;
    int64_t ldh = 0;
    const float *xd = nullptr;
    int64_t ldd = 0;
    const uint16_t *xm = nullptr;
    int64_t ldm = 0;
    float *y = nullptr;
    int64_t ldy = 0;
    // epilogue as kq_args: y = v + resid, or y = gelu(gate_in) * v
    const float *resid = nullptr, *gate_in = nullptr;
    const uint16_t *gelu_tab = nullptr;
    int gelu_clamp = 0;
};
int launch_gemm_kq(int wtype, const kqg_args &a, hipStream_t s);
// the column count from which K-quant mul_mats (C-ABI, graph executor, engine prefill) take
// launch_gemm_kq: GHIP_KQ_MFMA_MIN (default 8; GHIP_KQ_MFMA=0 disables), or hpc_set_kq_gemm_min
int kq_gemm_min();
void set_kq_gemm_min(int v);

// ---- prefill (prefill.hip) ----------------------------------------------------------------------
enum qrow_mode { QR_F32 = 0, QR_NORM = 1, QR_EMBED_NORM = 2, QR_GELU = 3 };
struct qrow_args {  // T rows of K floats -> Q8_0 image q [T][ldq] int8 + da [T][ldd] (f32 of fp16 d)
    const float *x = nullptr, *x2 = nullptr;  // rows (stride ldx); x2 = `up` for QR_GELU (x = gate)
    int64_t ldx = 0, K = 0;
    const float *norm_w = nullptr;
    float eps = 0.f;
    const int *tokens = nullptr;              // QR_EMBED_NORM: token ids; embedding table (tiled)
    const uint8_t *emb_qs = nullptr, *emb_sc = nullptr;
    int emb_type = 0;
    int64_t emb_n_bt = 0;
    float emb_scale = 1.f;
    float *emb_out = nullptr;                 // scaled embedding rows (the residual stream), stride ldx
    const uint16_t *gelu_tab = nullptr;
    int gelu_clamp = 0;
    int8_t *q = nullptr;                      // int8 image (nullptr: not written)
    uint16_t *qh = nullptr;                   // optional f16 image of the same values (exact GEMM)
    int64_t ldq = 0;                          // multiple of 256 (zero padded)
    float *da = nullptr;
    int64_t ldd = 0;                          // >= ldq / 32
};
int launch_quant_rows(int mode, const qrow_args &a, int T, hipStream_t s);
struct gemm_args {  // Y[t][r] (stride ldy) = W (tiled) x Xq[t] (+ resid), t < T, r < rows
    const uint8_t *qs = nullptr, *sc = nullptr;
    int64_t rows = 0, n_rt = 0, n_bt = 0, nb = 0;
    const int8_t *xq = nullptr;
    const uint16_t *xh = nullptr;  // f16 image of xq (the exact GEMM's MFMA operand), same stride
    int64_t ldq = 0;
    const float *da = nullptr;
    int64_t ldd = 0;
    int64_t T = 0;
    float *y = nullptr;
    const float *resid = nullptr;
    int64_t ldy = 0;
};
int launch_gemm_q(int wtype, int epi, const gemm_args &g, hipStream_t s);
// The exact GEMM's form, one process-wide choice (hpc_set_gemm_x4(mode), modes 0-4, default 3) decoded
// once.  A pass reads it once (gemm_form_now) and hands the same value to the quantizer step, which
// writes the image the form stages from, and to every launch_gemm_exact of the pass.
struct gemm_form {
    bool x4 = true;  // k_gemm_x4 (the K = 4 multi-block MFMA); false: k_gemm_x (lane-masked W32)
    int rgs = 2;     // k_gemm_x4: 16-row groups per workgroup, 2 (32 rows x 64 tokens) or 4 (64 x 32)
    bool i8 = true;  // the activation is staged from the int8 image (xq); false: from the f16 image (xh)
};
gemm_form gemm_form_now();
void set_gemm_x4(int mode);  // outside 0-4: the form stays as it was, set_error says so
// the same product in ggml's AVX2 lane order (bit-identical to mul_mat)
int launch_gemm_exact(int wtype, int epi, const gemm_form &form, const gemm_args &g, hipStream_t s);
// the same product for 1 <= T <= 8 rows (gemm_skinny.hip): every weight tile loaded once and applied
// to all T columns, one thread per (row, AVX2 lane) as the decode matvec; reads the int8 image
// (xq, da); EPI_STORE / EPI_ADD.  T outside [1, 8]: -1 with set_error
constexpr int GEMM_SKINNY_MAX_T = 8;
int launch_gemm_skinny(int wtype, int epi, const gemm_args &g, hipStream_t s);

struct ropekv_args {  // RoPE q (-> f16, x q_scale) and k, store k/v of positions p0.. in the layer caches
    const float *qkv = nullptr;  // [T][ldqkv] = q | k | v
    int64_t ldqkv = 0;
    const float *rope_cos = nullptr, *rope_sin = nullptr;
    uint16_t *q16 = nullptr;     // [T][H][hd]
    uint16_t *kc = nullptr, *vc = nullptr;
    int H = 0, Hkv = 0, hd = 0, ctx = 0, p0 = 0;
    float q_scale = 1.f;
};
int launch_rope_kv_prefill(const ropekv_args &a, int T, hipStream_t s);
struct attnp_args {  // causal attention of T prompt tokens against the layer caches
    const uint16_t *q16 = nullptr;  // [T][H][hd], row t of the launch
    const uint16_t *kc = nullptr, *vc = nullptr;
    float *out = nullptr;        // [T][ldo], head h at h*hd
    int64_t ldo = 0;
    int T = 0, H = 0, Hkv = 0, hd = 0, ctx = 0, n_kv = 0;
    // row t is sequence position p0 + t and attends keys 0 .. p0 + t; the caches already hold the
    // positions < p0 (a prefill continued mid-sequence); n_kv is the padded key count of row T - 1
    int p0 = 0;
};
int launch_attn_prefill(const attnp_args &a, hipStream_t s);
// exact rows: each prompt row with the decode attention's arithmetic (ops.hip)
int launch_attn_rows(const attnp_args &a, hipStream_t s);
// the same rows on the f32 matrix cores (attn_mx.hip): v_mfma_f32_16x16x4_f32 is an fmaf chain over K,
// so vec_dot_f16's 32 chains ride K four steps at a time; "" when it runs the shapes
const char *attn_mx_unsupported(const attnp_args &a);  // nullptr: the matrix-core form runs these shapes
int launch_attn_mx(const attnp_args &a, hipStream_t s);
// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel raised to the CU's whole LDS, once per
// (slot, device), thread-safe: slots LDS_SLOT_*
enum { LDS_SLOT_ATTN_MX = 0, LDS_SLOT_GELU_LDS = 1, LDS_SLOTS = 2 };
int allow_full_lds(const void *fn, int slot);
// the `parts` partial argmax keys of each of `rows` rows (ld floats apart) in ONE launch, grid (parts,
// rows): row r's keys at keys + r * parts
int launch_row_argmax(const float *row, int64_t n, unsigned long long *keys, int parts, hipStream_t s, int rows = 1,
                      int64_t ld = 0);

// ---- weights (ops.hip) ------------------------------------------------------------------------
// ggml row-major blocks (host layout) already on device -> tiled layout
int launch_repack(const tiled_mat &m, const uint8_t *src_rowmajor, int64_t row_bytes, hipStream_t s);
// synthetic generator: same integer stream + reference quantizer as oracle/gemma_cpu.cpp
int launch_synth_tiled(const tiled_mat &m, uint64_t key, float scale, int64_t row_offset, hipStream_t s);
int launch_synth_norm(float *dst, int64_t n, uint64_t key, float scale, hipStream_t s);
int launch_untile(const tiled_mat &m, uint8_t *dst_rowmajor, hipStream_t s);

// ---- small decode ops (ops.hip) -----------------------------------------------------------------
enum attn_mode { ATTN_PER_HEAD = 0, ATTN_SPLIT = 1 };
struct attn_args {
    const float *qkv;       // [q(H*hd) | k(Hkv*hd) | v(Hkv*hd)] for one token
    uint16_t *kc, *vc;      // layer caches: K [ctx][Hkv*hd], V [Hkv*hd][ctx] (f16 bits)
    const float *rope_cos, *rope_sin;  // [ctx][hd/2]
    const float *rope_cur = nullptr;   // [cos | sin | (int)pos] of *pos (k_advance keeps it current)
    const uint16_t *exp_tab;
    const int *pos;         // device scalar (position of this token)
    float *out;             // [H*hd]
    uint32_t *out_act = nullptr;  // per-head mode: also out's Q8_0 image (attn-out's PRO_IMG input)
    float *out_da = nullptr;
    uint8_t *out_q8k = nullptr;   // per-head mode, hd == 256: out's Q8_K image (one super-block per head)
    int dsplit = 1;               // per-head mode: workgroups per head, each the KQV of hd/dsplit dims
    int H, Hkv, hd, ctx;
    float q_scale;
    float *dbg_w = nullptr;      // optional debug taps: [H][ctx] scores, [H][ctx] fp16 P, [H] inv
    uint16_t *dbg_p = nullptr;
    float *dbg_inv = nullptr;
    unsigned long long *dbg_t = nullptr;  // diagnostic phase stamps (s_memrealtime), [grid][8]
    int mode = 0;  // ATTN_PER_HEAD (one workgroup per head) or ATTN_SPLIT (long contexts)
    // split form: workgroups per kv head, scores scratch [Hkv][ctx][G], hand-off counters [Hkv][2]
    // (zero before the first launch; each launch leaves them zero), sticky error word
    int nwg = 0;
    float *sbuf = nullptr;
    int *sync = nullptr;
    int *err = nullptr;
    // per-head mode inside the persistent token launch: the output's Q8_0 image published as
    // {payload, tag} granules (act dwords in the image's dword order, block scales) instead of stores
    unsigned long long *out_gran = nullptr, *out_gran_da = nullptr;
    uint32_t gran_tag = 0;
};
// the front half of a decode layer in one launch (layer_front.hip): qkv (rr, PRO_NORM, EPI_STORE)
// -> per-head attention -> attn-out (rr, PRO_IMG from the attention's image, EPI_ADD)
struct front_args {
    mv_args q;
    attn_args t;
    mv_args o;
    unsigned *cnt = nullptr;  // this layer's hand-off counters [16], zero before the launch
    int *err = nullptr;       // sticky: a hand-off poll timed out
    unsigned long long *dbg_t = nullptr;  // diagnostics (stamps build): 16 s_memrealtime per workgroup
};
bool layer_front_supported(int wtype, const mv_args &q, const attn_args &t, const mv_args &o);
int launch_layer_front(int wtype, const front_args &f, hipStream_t s);
// the decode attention (per-head form) and attn-out (+ residual) in ONE launch (layer_front.hip
// k_attn_o): the attention launch's idle workgroups run attn-out's row tiles, weights in flight
// before the in-launch hand-off of the attention's Q8_0 image
struct attn_o_args {
    attn_args t;              // per-head attention, out_act / out_da set (the handed-off image)
    mv_args o;                // attn-out: PRO_IMG from t.out_act / t.out_da, EPI_ADD
    unsigned *cnt = nullptr;  // this layer's counters: 8 replicas + the consumers' done count, 128 B apart;
                              // zero before the launch, and the launch leaves them zero
    int *err = nullptr;       // sticky: a hand-off poll timed out (err[0]; err[1..4] diagnostics)
    unsigned long long *dbg_t = nullptr;  // stamps build: 16 s_memrealtime per workgroup
};
bool attn_o_supported(int wtype, const attn_args &t, const mv_args &o);
int launch_attn_o(int wtype, const attn_o_args &f, hipStream_t s);

// peer-to-peer all-gather (p2p.hip, GEMMA_TP_P2P): each rank pushes [rank*shard, +shard) of every
// segment's working vector into every peer's inbox (arena offset `inbox`), flags it, and copies
// the peers' shards out of its own inbox; peer[r] = rank r's arena in this process's address space
constexpr int P2P_MAX_RANKS = 8;
struct p2p_seg {
    uint8_t *work = nullptr;  // the full working vector (this rank's shard written by the producer)
    int64_t inbox = 0;        // its inbox's offset in every rank's arena (16-byte aligned)
    int64_t shard = 0;        // bytes per rank (multiple of 4)
};
struct p2p_args {
    p2p_seg seg[2];
    int nseg = 1;
    int rank = 0, n = 1;
    uint8_t *peer[P2P_MAX_RANKS] = {};
    int64_t flags = 0;        // arena offset of the u32 flag words, one per source rank
    unsigned *seq = nullptr;  // [0] gathers done, [1] workgroups finished in the current one (local)
    unsigned *err = nullptr;  // sticky: a flag wait timed out
};
int launch_p2p_gather(const p2p_args &a, hipStream_t s);

// ---- the whole decode token's layers as ONE persistent launch (token.hip) ----------
// per layer: device pointers of the tiled matrices, norms and KV caches (a table in device memory,
// read through the scalar cache: immutable for the launch)
struct tok_layer {
    const uint8_t *qkv_qs = nullptr, *qkv_sc = nullptr, *o_qs = nullptr, *o_sc = nullptr;
    const uint8_t *g_qs = nullptr, *g_sc = nullptr, *u_qs = nullptr, *u_sc = nullptr, *d_qs = nullptr, *d_sc = nullptr;
    const float *attn_norm = nullptr, *ffn_norm = nullptr;
    uint16_t *kc = nullptr, *vc = nullptr;
};
struct tok_args {
    const tok_layer *layers = nullptr;
    int n_layer = 0;
    int E = 0, F = 0, H = 0, Hkv = 0, hd = 0, ctx = 0, qkv_rows = 0;
    int att_split = 0;  // workgroups per query head (each the KQ / softmax and hd / att_split KQV dims)
    float eps = 0.f, emb_scale = 1.f, q_scale = 1.f;
    const uint8_t *emb_qs = nullptr, *emb_sc = nullptr;  // tied embedding (tiled, layer type)
    int64_t emb_n_bt = 0;
    const int *hist = nullptr, *pos = nullptr;
    const float *rope_cur = nullptr;
    const uint16_t *exp_tab = nullptr, *gelu_tab = nullptr;
    int gelu_clamp = 0;
    // in-launch hand-offs: 8-byte {payload, tag} granules (MI355X_MICROARCH handoff-1to1 / allgather)
    unsigned long long *gx = nullptr, *gqkv = nullptr, *gatt = nullptr, *gatt_da = nullptr, *gsa = nullptr,
                       *gh = nullptr, *gh_da = nullptr;
    const unsigned *epoch = nullptr;  // bumped by k_advance / k_set_position: tags are unique per token
    float *x_out = nullptr;           // the last layer's output x (the logits launch's input)
    float *att_out = nullptr;         // attention output scratch (written, unused)
    int *err = nullptr;               // [0] sticky hand-off timeout, [1] site, [2] layer
    unsigned timeout = 2000000u;      // per-wait bound in s_memrealtime ticks (100 MHz): 20 ms
    unsigned long long *dbg_t = nullptr;  // stamps build: [grid][n_layer][16] s_memrealtime
};
// granules each buffer holds for shapes (E, F, qkv_rows)
struct tok_gran_sizes {
    size_t gx, gqkv, gatt, gatt_da, gsa, gh, gh_da;
};
tok_gran_sizes token_gran_sizes(int E, int F, int qkv_rows);
// "" if the shapes / device allow the persistent token launch, else the reason
std::string token_unsupported(int wtype, const tok_args &a);
// a: the args on the host (checked), ap: the same args in device memory (what the kernel reads)
int launch_token(int wtype, const tok_args &a, const tok_args *ap, hipStream_t s);

struct attn_geom {
    int nwg = 0, grid = 0;
    int img = 0;  // the split form can write the output's Q8_0 image (32-dim KQV slices)
    size_t lds = 0, sbuf_floats = 0, sync_ints = 0;
};
attn_geom attn_geometry(int H, int Hkv, int hd, int ctx);
int launch_attn_decode(const attn_args &a, hipStream_t s);
int launch_embed(const uint8_t *qs, const uint8_t *sc, int wtype, int64_t n_bt, const int *token, float scale,
                 float *out, int64_t E, hipStream_t s);
// reduces the n_parts per-workgroup argmax keys, appends the token, advances the position
int launch_exp_f16_all(uint16_t *out, hipStream_t s);
int launch_stream_read(const void *buf, size_t bytes, unsigned *sink, hipStream_t s, int variant = 0);  // roofline probe  // the softmax's exp for all 65536 f16 codes (tests)
int launch_reduce_keys(const unsigned long long *keys, int n, int64_t row_base, unsigned long long *out, hipStream_t s);
struct rope_row {  // k_advance also publishes the new position's RoPE row: cur = [cos | sin | (int)pos]
    const float *cos = nullptr, *sin = nullptr;
    float *cur = nullptr;
    int half = 0, ctx = 0;
    unsigned *epoch = nullptr;  // if set, incremented (the persistent token launch's granule tags)
};
// read `n` weight regions with allocating loads (MALL warm-up for a later kernel), `grid` workgroups
int launch_advance(const unsigned long long *keys, int n_parts, int *token, int *pos, int *hist, int hist_cap,
                   const int *n_fixed, const rope_row &r, hipStream_t s);
int launch_set_position(int token, int p, int *pos, int *hist, int *n_fixed, int fixed, const rope_row &r, hipStream_t s);

// ---- speculative verify pass (verify.hip; gemma_engine_verify, DESIGN.md §5b‴) --------------------
struct verify_args {
    const unsigned long long *keys = nullptr;  // row i's pick: n_parts partial argmax keys at keys + i * key_stride
    int n_parts = 0, key_stride = 0;
    int k = 0, p0 = 0;                         // drafts at hist[p0 + 1 .. p0 + k], the pass's rows p0 .. p0 + k
    int *token = nullptr, *pos = nullptr, *hist = nullptr;
    rope_row r;                                // the accepted position's RoPE row, the epoch bump
    unsigned long long *zero_keys = nullptr;   // the decode step's argmax keys, zeroed as gemma_engine_extend does
    int n_zero = 0;
    int *out = nullptr;                        // [0] = a (accepted drafts), [1 + i] = g_i for i <= k
};
int launch_verify_accept(const verify_args &v, hipStream_t s);
// K rows / V columns p0 + *accepted + 1 .. p0 + k of n_layer caches (layer_stride elements apart) zeroed
int launch_verify_clean(uint16_t *kc, uint16_t *vc, int n_layer, int64_t layer_stride, int ctx, int kvw, int p0, int k,
                        const int *accepted, hipStream_t s);

// ---- batched decode (batch.hip; gemma_engine_batch_*, DESIGN.md §5b⁗) ---------------------------
// One row of a batch pass: the next token of its own sequence (slot).  The table lives in device
// memory and is rewritten when the set of active slots changes; no entry depends on a position.
struct sampler_params {  // a sampler's parameters as the kernels of sample.hip read them (device memory)
    float temperature = 0.0f;
    int top_k = 0;
    float top_p = 1.0f;
    int pad = 0;
    unsigned long long seed = 0;
};
struct slot_row {
    const float *qkv = nullptr;  // the row's q | k | v in the pass's scratch
    float *out = nullptr;        // the row's attention output [H*hd]
    uint16_t *kc = nullptr, *vc = nullptr;  // the slot's caches, layer 0 (layers a fixed stride apart)
    float *rope = nullptr;       // the slot's [cos | sin | (int)pos]: the position is read on the device
    int *hist = nullptr, *pos = nullptr, *last = nullptr;
    const int *nfix = nullptr;
    double *lp = nullptr;        // the slot's log-probabilities by sequence index (k_lse_finish)
    // the sampler in force on the row's slot, by value (the slot's own, else the engine's; temperature
    // <= 0: greedy): the sampler's kernels of a pass with a row table read it with the entry, one load
    sampler_params smp;
};
// k_attn_slots: the decode attention (attn_head_dev, per-head form) for R rows, each against its own
// slot's caches at its own position.  a: the shared fields (geometry, tables, dsplit); qkv, kc, vc,
// rope_cur and out come from rows[r], the caches offset by layer_off elements.  R <= 64.
constexpr int ATTN_SLOTS_MAX_R = 64;
int launch_attn_slots(const attn_args &a, const slot_row *rows, int R, int64_t layer_off, hipStream_t s);
// k_batch_advance: per row, reduce the n_parts pick keys at keys + r * key_stride, then k_advance for
// the row's slot: p = pos + 1, hist[p] = pick if p >= nfix, pos = p, the RoPE row of p, and the next
// pass's token hist[p] into row_tok[r] and the slot's `last`
int launch_batch_advance(const slot_row *rows, int R, const unsigned long long *keys, int n_parts, int key_stride,
                         int *row_tok, int hist_cap, const rope_row &r, hipStream_t s);
// Several rows per slot (gemma_engine_batch_step_rows): a pass of T rows ordered by slot, then by
// position.  Row t has a slot_row of its own whose `rope` is the row's own [cos | sin | (int)p] and
// whose `pos` is that row's position word, so the sampler and k_lse_finish read the row's position,
// not the slot's.  row_src says where the row comes from; slot_span which rows are a slot's.
struct row_src {
    const int *spos = nullptr;  // the slot's device position word
    int off = 0;                // the row processes hist[*spos + off]
    int rank = 0;               // the slot's index among the active slots (its row of a batch_step pass)
};
struct slot_span {
    int row0 = 0, m = 0;  // the slot's rows [row0, row0 + m) of the pass
};
// before the first layer, one workgroup per row: p = *spos + off, the row's RoPE row with its
// position word, and the row's token hist[p] into row_tok[t]
int launch_rows_prepare(const slot_row *mrows, const row_src *src, int T, int *row_tok, const rope_row &r, hipStream_t s);
// a layer's attention step for T such rows, two launches with a kernel boundary between them:
// k_rows_rope_kv (RoPE of k from the full tables at the row's position, K row p and V column p of the
// slot's caches), then k_attn_slot_rows (attn_head_dev with every K / V operand read from the cache,
// the row's own position included; it stores nothing to a cache)
int launch_attn_slot_rows(const attn_args &a, const slot_row *mrows, const row_src *src, int T, int64_t layer_off,
                          hipStream_t s);
// the first of those two launches alone (gemma_test_rows_rope_kv)
int launch_rows_rope_kv(const attn_args &a, const slot_row *mrows, int T, int64_t layer_off, hipStream_t s);
// The long form (attn_long.hip; DESIGN.md §5b⁗ "Long contexts"): a layer's attention step for T rows of any
// of the batch's row tables at n_ctx up to ATTN_LONG_MAX_CTX, four launches with kernel boundaries the
// only ordering: k_rows_rope_kv, the scores of every (row, kv head, position block) into sbuf
// [T][Hkv][ctx][G] f32, the softmax per (row, head) into pbuf [T][H][ctx] f16, the KQV per (row, kv
// head, dim slice).  Every K / V operand comes from the cache; nothing of sbuf / pbuf outlives the call.
constexpr int ATTN_LONG_MAX_CTX = 8192;
int launch_attn_long_rows(const attn_args &a, const slot_row *rows, int T, int64_t layer_off, float *sbuf, uint16_t *pbuf,
                          hipStream_t s);
// per active slot (rows: the batch_step table, by rank): the key reduction of the slot's last row,
// pos += m, the guarded hist write, the slot's RoPE row, `last` and row_tok[rank]; every row's
// position word becomes the sequence index it predicts (k_lse_finish)
int launch_rows_advance(const slot_row *rows, const slot_row *mrows, const slot_span *spans, int R,
                        const unsigned long long *keys, int n_parts, int key_stride, int *row_tok, int hist_cap,
                        const rope_row &r, hipStream_t s);
// Drafts in the batch (gemma_engine_batch_verify): a pass of such rows in which a participating slot
// has its pending token and up to 7 drafts.  The per-slot table is the pass's own, by the slot's index
// among the participating slots; slots that sit out appear in no table of the pass.
constexpr int BV_MAX_ROWS = 8;                // rows of one slot: 1 + GEMMA_VERIFY_MAX_DRAFT
constexpr int BV_OUT_WORDS = 1 + BV_MAX_ROWS; // per slot: [0] = a (accepted drafts), [1 + i] = g_i for i < m
struct bv_slot {
    int row0 = 0, m = 0;  // the slot's rows [row0, row0 + m) of the pass; m - 1 drafts
    int rank = 0;         // the slot's index in the batch_step table (rows, row_tok)
    int pad = 0;
    int draft[BV_MAX_ROWS] = {};  // draft[i], i < m - 1: the guess for sequence index pos + 1 + i
};
// before k_rows_prepare, one workgroup per participating slot: hist[pos + 1 + i] = draft[i], i < m - 1
int launch_bverify_stage(const slot_row *rows, const bv_slot *vs, int P, int hist_cap, hipStream_t s);
// per participating slot: the key reduction of each of its m rows, a = the leading drafts that equal
// their row's pick, then what a + 1 calls of k_batch_advance leave (hist under the nfix guard, pos, the
// RoPE row, `last`, row_tok[rank]); the rejected drafts behind them zeroed in hist; row (s, i)'s
// position word the index it predicts (i <= a) or -1 (k_lse_finish writes nothing); out[s] = a, g_0 ..
int launch_bverify_accept(const slot_row *rows, const slot_row *mrows, const bv_slot *vs, int P,
                          const unsigned long long *keys, int n_parts, int key_stride, int *row_tok, int hist_cap,
                          const rope_row &r, int *out, hipStream_t s);
// grid (layer, slot): K rows and V columns pos .. pos + (m - 1 - a) - 1 of the slot's caches back to
// zero, pos the slot's position after the accept and a = out[s][0] read on the device
int launch_bverify_clean(const slot_row *rows, const bv_slot *vs, int P, const int *out, int n_layer, int64_t layer_stride,
                         int ctx, int kvw, hipStream_t s);

// ---- on-device sampling (sample.hip; the rule: include/gemma_hpc.h, DESIGN.md §5b″) ------------
constexpr int SAMPLE_MAX_K = 1024;  // candidates at most (top_k == 0 means this many)
// (sampler_params, above slot_row: the engine's lives in device memory, a change is a stream-ordered copy)
constexpr int SAMPLE_WS_HIST = 4096 + 16;  // words of one row's histogram and list cursors
struct sample_ws {  // scratch of `rows` samplers, one per row of a launch (sample_ws_alloc); the tail
                    // launch leaves every row's hist and cur zero
    int rows = 0;
    unsigned *hist = nullptr, *cur = nullptr;  // [rows][SAMPLE_WS_HIST]: key histogram [4096], list cursors [2] (cur = hist + 4096)
    unsigned long long *list_a = nullptr, *list_b = nullptr;  // [rows][SAMPLE_MAX_K], [rows][cap_b] (key << 32 | ~index)
    int64_t cap_b = 0;                                        // = n_vocab
    unsigned long long *key = nullptr;  // [rows] the drawn tokens, each one argmax key (launch_advance(key, 1, ...))
};
struct sample_dbg {  // optional outputs (tests), per row: token [rows], cand [rows][SAMPLE_MAX_K] (-1 past K), K, m [rows]
    int *token = nullptr, *cand = nullptr, *n_cand = nullptr, *n_kept = nullptr;
};
int sample_ws_alloc(dev_pool &mem, sample_ws *w, int64_t n_vocab, hipStream_t s, int rows = 1);  // all four buffers, or none
void sample_ws_free(dev_pool &mem, sample_ws *w);
// The rows of a pass, three launches in all (grid.y = row): row r's token for sequence index
// *pos_r + 1 from lg[r * ld .. + n) into w.key[r], in row r's own workspace.  pos_r is tab[r].pos when
// a row table is given, else pos + r.  prm, pos and tab are device pointers read by the kernels; the
// geometry depends on n and rows only.
// Parameters per row: with a row table row r's parameters are tab[r].smp (prm is not read); a row
// whose temperature is <= 0 is greedy: it leaves all three kernels before its first
// atomic, its workspace stays zero and its key slot is not written.  key_parts > 1: row r's key slot
// is w.key + r * key_parts and the tail fills it [pick, 0, 0, ...]: the layout of the row-argmax
// partial keys, so an advance kernel reduces greedy and sampling rows of one pass alike.
int launch_sample(const float *lg, int64_t ld, int rows, int64_t n, const sampler_params *prm, const int *pos,
                  const slot_row *tab, const sample_ws &w, const sample_dbg &dbg, hipStream_t s, int key_parts = 1);
// The picks of a pass's rows, one key layout per pass, the launch count by `mix` alone:
//   PICKS_GREEDY  no row samples: the one row-argmax launch, 256 partial keys per row at keys
//   PICKS_SAMPLE  every row samples: the sampler's three launches, one key per row at keys + rows_cap * 256
//   PICKS_MIXED   both, four launches: the row argmax over every row, then the sampler, whose tail
//                 overwrites a sampling row's 256 partial keys with [pick, 0 ...]
// keys: [rows_cap * 256 + rows_cap] u64.  out_*: what the advance kernel takes
enum { PICKS_GREEDY = 0, PICKS_SAMPLE = 1, PICKS_MIXED = 2 };
int launch_picks(int mix, const float *lg, int64_t ld, int rows, int64_t n, const sampler_params *prm, const int *pos,
                 const slot_row *tab, const sample_ws &w, unsigned long long *keys, int rows_cap, const sample_dbg &dbg,
                 hipStream_t s, const unsigned long long **out_keys, int *out_parts, int *out_stride);

// ---- per-token log-probabilities (logprob.hip; the rule: include/gemma_hpc.h, DESIGN.md §5b⁗′) ----
constexpr int LSE_CHUNK = 1024;  // logits per workgroup of k_lse_parts: G = ceil(n_vocab / LSE_CHUNK), n_vocab alone
constexpr int LSE_MAX_G = 1024;  // partials k_lse_finish merges (n_vocab <= 2^20)
struct lse_part {                // one chunk of one row: its float max and sum exp((double)l - (double)m)
    double s;
    float m, pad;
};
int lse_grid(int64_t n_vocab);
// parts[r][g] for the `rows` rows lg + r * ld of n logits, grid (G, rows); needs no token and no position
int launch_lse_parts(const float *lg, int64_t ld, int rows, int64_t n, lse_part *parts, hipStream_t s);
struct lse_finish_args {  // grid (1, R): lp[q_r] = logprob(row r, hist[q_r]) once the advance has settled hist[q_r]
    const float *lg = nullptr;
    int64_t ld = 0;
    int n = 0, R = 0, G = 0, n_ctx = 0;
    const lse_part *parts = nullptr;
    // the sequence index q_r row r predicts, its history and its lp array: tab[r]'s (*pos after the
    // slot's advance) when the pass has a row table; else one sequence whose rows are consecutive
    // positions ending at *pos: q_r = *pos - (last - r), last = R - 1, or *acc when acc is set (a verify
    // pass: rows past the accepted count write nothing).  q outside [1, n_ctx] or a token outside
    // [0, n): nothing is written
    const slot_row *tab = nullptr;
    const int *pos = nullptr, *hist = nullptr, *acc = nullptr;
    double *lp = nullptr;
};
int launch_lse_finish(const lse_finish_args &a, hipStream_t s);

// ---- generic ggml-op kernels used by the C-ABI and the ggml-compatible executor ----------------
int launch_mul_mat_f16(const uint16_t *src0, int64_t nb01_elems, int64_t ne01, const uint16_t *src1,
                       int64_t row_size_elems, int64_t ncols, int64_t K, float *dst, hipStream_t s);

}  // namespace ghip
