// batch.hip — batched decode (gemma_engine_batch_*, DESIGN.md §5b⁗): the kernels that let one
// weight pass serve up to 64 independent sequences (8 on the skinny GEMM, more on the MFMA GEMMs).
//
//  * k_attn_slots: the decode attention for R rows, row r against the caches of its own slot at its
//    own position.  It is k_attn_head's body (attn_head_dev, attn_impl.h) instantiated per row: RoPE
//    NEOX, the K / V store of this position, vec_dot_f16 lane order by v_fma_mix, the fp16 exp table,
//    the exact integer sum, KQV per output dim.  The row's pointers come from a device table
//    (slot_row); the position is the word published with the slot's RoPE row.  No workgroup waits on
//    another.
//  * k_batch_advance: k_advance per row — the pick-key reduction and the slot's token feedback.
//  * several rows per slot (gemma_engine_batch_step_rows, "Several rows per slot" in §5b⁗):
//    k_rows_prepare (the rows' positions, RoPE rows and tokens), per layer k_rows_rope_kv (the K / V
//    stores of all rows) then k_attn_slot_rows (attn_head_dev with every K / V operand read from the
//    cache), and k_rows_advance (k_batch_advance per slot, pos += m).
//  * drafts in the batch (gemma_engine_batch_verify, "Drafts in the batch" in §5b⁗): such a pass over the
//    participating slots, with k_bverify_stage in front (the drafts into hist) and, instead of
//    k_rows_advance, k_bverify_accept (the accept rule and the advance over the accepted prefix per
//    slot) and k_bverify_clean (the rejected rows' K / V back to zero).
#include "attn_impl.h"
#include "pick.h"

namespace ghip {
namespace {

// grid (8 * H * dsplit, R): as k_attn_head, the G * dsplit workgroups of a kv head share an XCD (they
// read the same K rows through its L2); the rows of a pass are spread over the XCDs
__global__ void __launch_bounds__(AH_THREADS) k_attn_slots(attn_args a, const slot_row *rows, int64_t layer_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int S = a.dsplit, G = a.H / a.Hkv;
    const int row = blockIdx.y, hs = blockIdx.x >> 3, h = hs / S, sp = hs % S;
    if ((int)(blockIdx.x & 7) != ((h / G + row) & 7)) return;
    const slot_row r = rows[row];
    a.qkv = r.qkv;
    a.kc = r.kc + layer_off;
    a.vc = r.vc + layer_off;
    a.rope_cur = r.rope;
    a.out = r.out;
    attn_head_dev<AH_THREADS, false, AH_KPF, AH_VPF, false>(a, h, smem, nullptr, sp);
}

// What a pass leaves on a slot (sr: its entry of the batch_step table) that had m rows in it, the last
// of which picks from `keys`: the position m further with its RoPE row, the pick committed there, the
// pending token in *sr.last and *tok_out (what the slot's row processes in a following batch_step
// pass).  own: the m rows' entries when they have position words of their own, else null.
__device__ __forceinline__ void slot_advance_dev(const slot_row &sr, int m, const slot_row *own, const unsigned long long *keys,
                                                 int n_parts, int *tok_out, int hist_cap, const rope_row &r,
                                                 unsigned long long *red) {
    // every thread reads the position before the barrier; thread 0 writes it after (as k_advance)
    const int p = *sr.pos + m;
    const int fixed = *sr.nfix;
    if (p < r.ctx) publish_rope_row(sr.rope, r.cos, r.sin, r.half, p);  // the next position's, with its position word
    // row (s, i) predicts sequence index pos + i + 1: what k_lse_finish reads as its position
    if (own && (int)threadIdx.x < m) *own[threadIdx.x].pos += 1;
    const unsigned long long best = block_max_key(keys, n_parts, red);
    if (threadIdx.x == 0) {
        const int tok = commit_pick(sr.hist, p, fixed, hist_cap, key_index(best));
        *sr.pos = p;
        *sr.last = tok;
        *tok_out = tok;
    }
}

__global__ void __launch_bounds__(256) k_batch_advance(const slot_row *rows, const unsigned long long *keys, int n_parts,
                                                       int key_stride, int *row_tok, int hist_cap, rope_row r) {
    __shared__ unsigned long long red[4];
    const slot_row sr = rows[blockIdx.x];
    slot_advance_dev(sr, 1, nullptr, keys + (int64_t)blockIdx.x * key_stride, n_parts, row_tok + blockIdx.x, hist_cap, r, red);
}

// ---- several rows per slot (gemma_engine_batch_step_rows) -----------------------------------------
// k_attn_slots stores its own position's K / V and patches its own row from LDS: right only while no
// other row of the launch reads that position.  Rows that share a slot at consecutive positions do,
// so their pass runs two launches per layer, the kernel boundary between them the only ordering.

// one workgroup per row, before the first layer: the row's position, RoPE row and token
__global__ void __launch_bounds__(256) k_rows_prepare(const slot_row *mrows, const row_src *src, int *row_tok, rope_row r) {
    const slot_row sr = mrows[blockIdx.x];
    const row_src rs = src[blockIdx.x];
    int p = *rs.spos + rs.off;
    if (p >= r.ctx) p = r.ctx - 1;  // (the host refused such a pass: its mirror of *spos is exact)
    publish_rope_row(sr.rope, r.cos, r.sin, r.half, p);
    if (threadIdx.x == 0) row_tok[blockIdx.x] = sr.hist[p];
}

// step 1 of a layer, one workgroup per row: k_rope_kv_prefill's arithmetic (the decode attention's)
// for the row's k and v at the row's position p, into K row p and V column p of its slot's caches
__global__ void __launch_bounds__(256) k_rows_rope_kv(attn_args a, const slot_row *mrows, int64_t layer_off) {
    const slot_row r = mrows[blockIdx.x];
    const int tid = threadIdx.x, hd = a.hd, half = hd / 2, kvw = a.Hkv * hd;
    const int p = ((const int *)r.rope)[hd];
    const float *cs = a.rope_cos + (int64_t)p * half, *sn = a.rope_sin + (int64_t)p * half;
    const float *kr = r.qkv + (int64_t)a.H * hd, *vr = kr + kvw;
    uint16_t *kc = r.kc + layer_off, *vc = r.vc + layer_off;
    for (int i = tid; i < a.Hkv * half; i += 256) {
        const int kh = i / half, e = i % half;
        const float x0 = kr[kh * hd + e], x1 = kr[kh * hd + e + half], c = cs[e], s = sn[e];
        const float p0 = x0 * c, p1 = x1 * s, p2 = x0 * s, p3 = x1 * c;
        kc[(int64_t)p * kvw + kh * hd + e] = (uint16_t)f2h(p0 - p1);
        kc[(int64_t)p * kvw + kh * hd + e + half] = (uint16_t)f2h(p2 + p3);
    }
    for (int d = tid; d < kvw; d += 256) vc[(int64_t)d * a.ctx + p] = (uint16_t)f2h(vr[d]);
}

// step 2, grid (8 * H * dsplit, T): attn_head_dev per (row, head, dsplit part) with every K / V
// operand from the cache.  Placement as k_attn_slots: the G * dsplit workgroups of a (row, kv head)
// share an XCD; so do 8 consecutive rows of one slot, which read the same K rows through its L2 (a
// slot with many rows is spread over the XCDs in runs of 8, not piled onto one)
__global__ void __launch_bounds__(AH_THREADS) k_attn_slot_rows(attn_args a, const slot_row *mrows, const row_src *src,
                                                               int64_t layer_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int S = a.dsplit, G = a.H / a.Hkv;
    const int row = blockIdx.y, hs = blockIdx.x >> 3, h = hs / S, sp = hs % S;
    const row_src rs = src[row];
    if ((int)(blockIdx.x & 7) != ((h / G + rs.rank + (rs.off >> 3)) & 7)) return;
    const slot_row r = mrows[row];
    a.qkv = r.qkv;
    a.kc = r.kc + layer_off;
    a.vc = r.vc + layer_off;
    a.rope_cur = r.rope;
    a.out = r.out;
    attn_head_dev<AH_THREADS, false, AH_KPF, AH_VPF, false, false, true>(a, h, smem, nullptr, sp);
}

// k_batch_advance per slot, for a slot that had m rows in the pass
__global__ void __launch_bounds__(256) k_rows_advance(const slot_row *rows, const slot_row *mrows, const slot_span *spans,
                                                      const unsigned long long *keys, int n_parts, int key_stride,
                                                      int *row_tok, int hist_cap, rope_row r) {
    __shared__ unsigned long long red[4];
    const slot_row sr = rows[blockIdx.x];
    const slot_span sp = spans[blockIdx.x];
    // the slot's last row picks
    slot_advance_dev(sr, sp.m, mrows + sp.row0, keys + (int64_t)(sp.row0 + sp.m - 1) * key_stride, n_parts,
                     row_tok + blockIdx.x, hist_cap, r, red);
}

// ---- drafts in the batch (gemma_engine_batch_verify) ------------------------------------------------
// The pass is a several-rows-per-slot pass (k_rows_prepare, k_rows_rope_kv, k_attn_slot_rows) whose
// rows past a slot's first process drafts.  Three kernels of its own, each over the participating
// slots (vs[blockIdx]; rows[vs.rank] is the slot's entry of the batch_step table).

// before k_rows_prepare reads the rows' tokens: the drafts become hist[pos + 1 .. pos + m)
__global__ void __launch_bounds__(64) k_bverify_stage(const slot_row *rows, const bv_slot *vs, int hist_cap) {
    const bv_slot *v = vs + blockIdx.x;
    const slot_row sr = rows[v->rank];
    const int i = threadIdx.x, q = *sr.pos + 1 + i;
    if (i < v->m - 1 && i < BV_MAX_ROWS - 1 && q < hist_cap) sr.hist[q] = v->draft[i];
}

// k_verify_accept per slot, the advance k_batch_advance's: row (s, i) picked g_i for sequence index
// p0 + i + 1, hist[p0 + 1 + i] holds draft[i] (i < k = m - 1); a = the leading drafts that equal their
// row's pick.  Then what a + 1 one-row passes leave on the slot.
__global__ void __launch_bounds__(256) k_bverify_accept(const slot_row *rows, const slot_row *mrows, const bv_slot *vs,
                                                        const unsigned long long *keys, int n_parts, int key_stride,
                                                        int *row_tok, int hist_cap, rope_row r, int *out) {
    __shared__ unsigned long long red[4];
    __shared__ int gs[BV_MAX_ROWS], a_sh;
    const int tid = threadIdx.x;
    const bv_slot *v = vs + blockIdx.x;
    const int row0 = v->row0, m = min(v->m, BV_MAX_ROWS), rank = v->rank;
    const slot_row sr = rows[rank];
    // every thread reads the position before the first barrier; thread 0 writes it after (as k_advance)
    const int p0 = *sr.pos;
    const int fixed = *sr.nfix;
    for (int i = 0; i < m; ++i) {
        const unsigned long long best = block_max_key(keys + (int64_t)(row0 + i) * key_stride, n_parts, red);
        if (tid == 0) gs[i] = key_index(best);
        __syncthreads();  // red[] is reused by the next row: thread 0 has read it
    }
    if (tid == 0) {
        const int k = m - 1;
        int a = 0;
        while (a < k && sr.hist[p0 + 1 + a] == gs[a]) ++a;  // stops at the first mismatch
        // (a k = 0 slot may still be ingesting given tokens)
        for (int i = 0; i <= a; ++i) gs[i] = commit_pick(sr.hist, p0 + 1 + i, fixed, hist_cap, gs[i]);
        for (int i = a + 1; i < k; ++i) sr.hist[p0 + 1 + i] = 0;  // the rejected drafts behind them
        *sr.pos = p0 + a + 1;
        *sr.last = gs[a];
        row_tok[rank] = gs[a];  // what the slot's row processes in a following batch_step pass
        int *o = out + blockIdx.x * BV_OUT_WORDS;
        o[0] = a;
        for (int i = 0; i < m; ++i) o[1 + i] = gs[i];
        a_sh = a;
    }
    __syncthreads();
    const int a = a_sh, p = p0 + a + 1;
    if (p < r.ctx) publish_rope_row(sr.rope, r.cos, r.sin, r.half, p);
    // an accepted row's position word becomes the sequence index it predicts (what k_lse_finish reads);
    // a rejected row's -1: outside [1, n_ctx], nothing is scored
    if (tid < m) *mrows[row0 + tid].pos = tid <= a ? p0 + tid + 1 : -1;
}

// grid (layer, slot): the K rows and V columns the pass stored under the slot's rejected drafts, p0 + a
// + 1 .. p0 + k = pos .. pos + (k - a) - 1 with pos the position the accept left, back to zero
__global__ void __launch_bounds__(256) k_bverify_clean(const slot_row *rows, const bv_slot *vs, const int *out,
                                                       int64_t layer_stride, int ctx, int kvw) {
    const bv_slot *v = vs + blockIdx.y;
    const int k = v->m - 1, a = out[blockIdx.y * BV_OUT_WORDS];
    if (a < 0 || a >= k) return;
    const slot_row sr = rows[v->rank];
    const int r0 = *sr.pos, n = k - a;
    if (r0 < 0 || r0 + n > ctx) return;
    uint16_t *K = sr.kc + (int64_t)blockIdx.x * layer_stride, *V = sr.vc + (int64_t)blockIdx.x * layer_stride;
    for (int idx = threadIdx.x; idx < n * kvw; idx += 256) {
        const int rr = r0 + idx / kvw, j = idx % kvw;
        K[(int64_t)rr * kvw + j] = 0;
        V[(int64_t)j * ctx + rr] = 0;
    }
}

}  // namespace

// the shapes and rows k_attn_slots and k_attn_slot_rows serve, and the LDS image they share (*lds);
// what: the error's prefix
static bool attn_slots_shape_ok(const attn_args &a, const slot_row *rows, int R, const char *what, size_t *lds) {
    if (a.mode != ATTN_PER_HEAD || a.hd % 32 != 0 || a.hd > 256 || a.ctx % 32 != 0 || a.Hkv <= 0 || a.H % a.Hkv != 0 ||
        a.dsplit < 1 || a.hd % (32 * a.dsplit) || 4 * (a.hd / a.dsplit) > AH_THREADS || a.out_act || a.out_q8k ||
        a.out_gran || !rows || R < 1 || R > ATTN_SLOTS_MAX_R) {
        set_error(std::string(what) + ": unsupported shape for the per-head form, or a pass outside [1, 64] rows");
        return false;
    }
    *lds = ((2 * (size_t)a.hd * 2 + 15) & ~(size_t)15) + (size_t)a.ctx * 4 + (size_t)a.ctx * 2 + 16;
    if (*lds > 64 * 1024) {  // n_ctx <= 2048 keeps it near 13 KiB
        set_error(std::string(what) + ": context too long for the LDS image");
        return false;
    }
    return true;
}

int launch_attn_slots(const attn_args &a, const slot_row *rows, int R, int64_t layer_off, hipStream_t s) {
    size_t lds;
    if (!attn_slots_shape_ok(a, rows, R, "attn_slots", &lds)) return -1;
    hipLaunchKernelGGL(k_attn_slots, dim3(8 * a.H * a.dsplit, R), dim3(AH_THREADS), lds, s, a, rows, layer_off);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_batch_advance(const slot_row *rows, int R, const unsigned long long *keys, int n_parts, int key_stride,
                         int *row_tok, int hist_cap, const rope_row &r, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_advance, dim3(R), dim3(256), 0, s, rows, keys, n_parts, key_stride, row_tok, hist_cap, r);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_rows_prepare(const slot_row *mrows, const row_src *src, int T, int *row_tok, const rope_row &r, hipStream_t s) {
    if (!mrows || !src || !row_tok || T < 1 || T > ATTN_SLOTS_MAX_R) {
        set_error("rows_prepare: a pass outside [1, 64] rows, or no row table");
        return -1;
    }
    hipLaunchKernelGGL(k_rows_prepare, dim3(T), dim3(256), 0, s, mrows, src, row_tok, r);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

// k_rows_rope_kv alone, the first of launch_attn_slot_rows' two launches (the per-op test entry)
int launch_rows_rope_kv(const attn_args &a, const slot_row *mrows, int T, int64_t layer_off, hipStream_t s) {
    if (!mrows || T < 1 || T > ATTN_SLOTS_MAX_R || a.Hkv <= 0 || a.hd <= 0 || a.hd % 2) {
        set_error("rows_rope_kv: a pass outside [1, 64] rows, no row table, or an odd head_dim");
        return -1;
    }
    hipLaunchKernelGGL(k_rows_rope_kv, dim3(T), dim3(256), 0, s, a, mrows, layer_off);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_attn_slot_rows(const attn_args &a, const slot_row *mrows, const row_src *src, int T, int64_t layer_off,
                          hipStream_t s) {
    if (!src) {
        set_error("attn_slot_rows: no row sources");
        return -1;
    }
    size_t lds;
    if (!attn_slots_shape_ok(a, mrows, T, "attn_slot_rows", &lds)) return -1;
    hipLaunchKernelGGL(k_rows_rope_kv, dim3(T), dim3(256), 0, s, a, mrows, layer_off);
    GHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_attn_slot_rows, dim3(8 * a.H * a.dsplit, T), dim3(AH_THREADS), lds, s, a, mrows, src, layer_off);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_rows_advance(const slot_row *rows, const slot_row *mrows, const slot_span *spans, int R,
                        const unsigned long long *keys, int n_parts, int key_stride, int *row_tok, int hist_cap,
                        const rope_row &r, hipStream_t s) {
    hipLaunchKernelGGL(k_rows_advance, dim3(R), dim3(256), 0, s, rows, mrows, spans, keys, n_parts, key_stride, row_tok,
                       hist_cap, r);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

static bool bverify_tables_ok(const slot_row *rows, const bv_slot *vs, int P, const char *what) {
    if (rows && vs && P >= 1 && P <= ATTN_SLOTS_MAX_R) return true;
    set_error(std::string(what) + ": a pass outside [1, 64] slots, or no table");
    return false;
}

int launch_bverify_stage(const slot_row *rows, const bv_slot *vs, int P, int hist_cap, hipStream_t s) {
    if (!bverify_tables_ok(rows, vs, P, "bverify_stage")) return -1;
    hipLaunchKernelGGL(k_bverify_stage, dim3(P), dim3(64), 0, s, rows, vs, hist_cap);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_bverify_accept(const slot_row *rows, const slot_row *mrows, const bv_slot *vs, int P,
                          const unsigned long long *keys, int n_parts, int key_stride, int *row_tok, int hist_cap,
                          const rope_row &r, int *out, hipStream_t s) {
    if (!bverify_tables_ok(rows, vs, P, "bverify_accept")) return -1;
    if (!mrows || !keys || !row_tok || !out || n_parts < 1) {
        set_error("bverify_accept: no row table, keys or result buffer");
        return -1;
    }
    hipLaunchKernelGGL(k_bverify_accept, dim3(P), dim3(256), 0, s, rows, mrows, vs, keys, n_parts, key_stride, row_tok,
                       hist_cap, r, out);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_bverify_clean(const slot_row *rows, const bv_slot *vs, int P, const int *out, int n_layer, int64_t layer_stride,
                         int ctx, int kvw, hipStream_t s) {
    if (!bverify_tables_ok(rows, vs, P, "bverify_clean")) return -1;
    if (!out || n_layer < 1 || ctx < 1 || kvw < 1) {
        set_error("bverify_clean: no accepted counts, or an empty cache");
        return -1;
    }
    hipLaunchKernelGGL(k_bverify_clean, dim3(n_layer, P), dim3(256), 0, s, rows, vs, out, layer_stride, ctx, kvw);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
