// batch.hip — batched decode (gemma_engine_batch_*, DESIGN.md §5b⁗): the two kernels that let one
// weight pass serve up to 64 independent sequences (8 on the skinny GEMM, more on the MFMA GEMMs).
//
//  * k_attn_slots: the decode attention for R rows, row r against the caches of its own slot at its
//    own position.  It is k_attn_head's body (attn_head_dev, attn_impl.h) instantiated per row: RoPE
//    NEOX, the K / V store of this position, vec_dot_f16 lane order by v_fma_mix, the fp16 exp table,
//    the exact integer sum, KQV per output dim.  The row's pointers come from a device table
//    (slot_row); the position is the word published with the slot's RoPE row.  No workgroup waits on
//    another.
//  * k_batch_advance: k_advance per row — the pick-key reduction and the slot's token feedback.
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

__global__ void __launch_bounds__(256) k_batch_advance(const slot_row *rows, const unsigned long long *keys, int n_parts,
                                                       int key_stride, int *row_tok, int hist_cap, rope_row r) {
    __shared__ unsigned long long red[4];
    const slot_row sr = rows[blockIdx.x];
    keys += (int64_t)blockIdx.x * key_stride;
    // every thread reads the position before the barrier; thread 0 writes it after (as k_advance)
    const int p = *sr.pos + 1;
    const int fixed = *sr.nfix;
    if (p < r.ctx) publish_rope_row(sr.rope, r.cos, r.sin, r.half, p);  // the next position's, with its position word
    const unsigned long long best = block_max_key(keys, n_parts, red);
    if (threadIdx.x == 0) {
        int tok = key_index(best);
        if (p < hist_cap) {
            if (p >= fixed) sr.hist[p] = tok;  // never overwrite a given token
            else tok = sr.hist[p];
        }
        *sr.pos = p;
        *sr.last = tok;
        row_tok[blockIdx.x] = tok;  // what the row processes in the next pass
    }
}

}  // namespace

int launch_attn_slots(const attn_args &a, const slot_row *rows, int R, int64_t layer_off, hipStream_t s) {
    if (a.mode != ATTN_PER_HEAD || a.hd % 32 != 0 || a.hd > 256 || a.ctx % 32 != 0 || a.Hkv <= 0 || a.H % a.Hkv != 0 ||
        a.dsplit < 1 || a.hd % (32 * a.dsplit) || 4 * (a.hd / a.dsplit) > AH_THREADS || a.out_act || a.out_q8k ||
        a.out_gran || !rows || R < 1 || R > ATTN_SLOTS_MAX_R) {
        set_error("attn_slots: unsupported shape for the per-head form, or a pass outside [1, 64] rows");
        return -1;
    }
    const size_t lds = ((2 * (size_t)a.hd * 2 + 15) & ~(size_t)15) + (size_t)a.ctx * 4 + (size_t)a.ctx * 2 + 16;
    if (lds > 64 * 1024) {  // n_ctx <= 2048 keeps it near 13 KiB
        set_error("attn_slots: context too long for the LDS image");
        return -1;
    }
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

}  // namespace ghip
