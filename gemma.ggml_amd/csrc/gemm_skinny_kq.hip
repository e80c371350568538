// gemm_skinny_kq.hip — the exact Q4_K / Q6_K GEMM for 1 <= T <= 8 Q8_K activation columns (the verify
// pass, a narrow batch pass and the 8-row groups of a mid-sized one on K-quant layers and the Q6_K
// output head): Y[t][r] = vec_dot_q{4,6}_K_q8_K(W row r, X column t), with kq_store's
// epilogues (plain, + resid, gelu(gate_in) * v).
//
// Order: kquant.hip's, unchanged.  One thread is one (row, AVX2 lane l) of an 8-row group; per
// super-block, in super-block order, acc_t = fmaf(y_t.d * f16(x.d), (float)isum_t, acc_t) for each of
// its columns t (Q4_K: the mins chain in lanes 0..3 beside it), then kq_store's fold.  isum_t is an
// exact integer, so how it is formed is free; the float chain per (row, column) is one thread walking K
// in order.  Every (row, column) therefore equals k_matvec_kq, k_matmul_kq and the MFMA GEMM bit for bit.
//
// What the T-column kernel (k_matmul_kq) does per column is done here once per super-block:
//   weights     a super-block's bytes are loaded once (kq_load) and applied to all T columns; a ring of
//               SKQ_CS super-blocks per wave is in flight ahead of its arithmetic, slot i refilled
//               right after its use.  No load sits in a branch: past the last super-block the index
//               is clamped and the slot is never used.
//   decode      Q4_K: the eight masked nibble dwords, the six-bit scales and the lane's two mins.
//               Q6_K: the eight 6-bit dwords already re-biased to signed int8 (q - 32 bytewise without
//               carries: y = q ^ 0x20, then bit 5 of y copied into bits 6 and 7), so a chunk and column
//               cost one signed v_dot4 instead of two; isum is the same integer.
//   activations the T Q8_K columns are staged in K chunks of SKQ_CS super-blocks (T = 8: 9.1 KiB),
//               double buffered: chunk c + 2 is loaded to registers and chunk c + 1 stored to the
//               other buffer in front of chunk c's compute, one barrier per chunk (gemm_skinny.hip's
//               scheme).  The blocks keep ggml's layout (d, 256 int8, 16 bsums: 73 dwords), so the
//               mins term reads the chunk's bsums; a lane's dwords of a chunk are consecutive over
//               l and shared by the 8 rows (LDS broadcast): no bank conflicts.
// Two forms, chosen by row-group count: four row groups per workgroup, a wave each; or (SPLIT, narrow
// matrices) one row group per workgroup whose waves divide the columns (wave w: columns w, w + NW),
// each streaming the group through its own ring (the re-reads hit L2).
#include "kquant_impl.h"

namespace ghip {
namespace {

constexpr int SKQ_CS = 4;  // super-blocks per K chunk = depth of the weight ring

// a super-block's weights for one AVX2 lane, decoded once for all columns
template <int WT> struct skq_dec;
template <> struct skq_dec<T_Q4_K> {
    uint32_t q[8];   // chunk 2j: low nibbles of quant dword j, chunk 2j + 1: high nibbles
    int sc[8];       // the chunks' six-bit scales
    int mn0, mn1;    // mins 2k, 2k + 1 of the lane's pair k = l & 3
    float d, dmin;   // f16(x.d), f16(x.dmin)
};
template <> struct skq_dec<T_Q6_K> {
    uint32_t q[8];   // chunk 4j + i: q6 - 32 as int8
    int sc[8];       // the lane's int8 scale of each chunk
    float d;
};

template <int WT>
__device__ __forceinline__ skq_dec<WT> skq_decode(const kq_raw<WT> &r, int l) {
    skq_dec<WT> w;
    if constexpr (WT == T_Q4_K) {
        const uint32_t u0 = r.h.y, u1 = r.h.z, u2 = r.h.w;  // kq_terms' unpack
        const uint32_t s03 = u0 & 0x3f3f3f3fu;
        const uint32_t s47 = (u2 & 0x0f0f0f0fu) | (((u0 >> 6) & 0x03030303u) << 4);
        const uint32_t m03 = u1 & 0x3f3f3f3fu;
        const uint32_t m47 = ((u2 >> 4) & 0x0f0f0f0fu) | (((u1 >> 6) & 0x03030303u) << 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t scw = j < 2 ? s03 : s47;
            w.sc[2 * j] = (scw >> (16 * (j & 1))) & 0xFF;
            w.sc[2 * j + 1] = (scw >> (16 * (j & 1) + 8)) & 0xFF;
            w.q[2 * j] = r.q[j] & 0x0F0F0F0Fu;
            w.q[2 * j + 1] = (r.q[j] >> 4) & 0x0F0F0F0Fu;
        }
        const int k = l & 3;
        const uint32_t mw = k < 2 ? m03 : m47;
        w.mn0 = (mw >> (16 * (k & 1))) & 0xFF;
        w.mn1 = (mw >> (16 * (k & 1) + 8)) & 0xFF;
        w.d = pin(h2f(r.h.x));
        w.dmin = pin(h2f(r.h.x >> 16));
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t qla = r.qla[j], qlb = r.qlb[j], qh = r.qh[j];
            const uint32_t q6[4] = {(qla & 0x0F0F0F0Fu) | ((qh & 0x03030303u) << 4),
                                    (qlb & 0x0F0F0F0Fu) | (((qh >> 2) & 0x03030303u) << 4),
                                    ((qla >> 4) & 0x0F0F0F0Fu) | (((qh >> 4) & 0x03030303u) << 4),
                                    ((qlb >> 4) & 0x0F0F0F0Fu) | (((qh >> 6) & 0x03030303u) << 4)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t y = q6[i] ^ 0x20202020u;  // q >= 32: q - 32; else q + 32, bit 5 set: - 64 = bits 6, 7
                w.q[4 * j + i] = y | ((y & 0x20202020u) << 1) | ((y & 0x20202020u) << 2);
                const int bi = 8 * j + 2 * i + (l >> 2);
                w.sc[4 * j + i] = (int)(int8_t)(uint8_t)(r.sc[bi >> 2] >> (8 * (bi & 3)));
            }
        }
        w.d = pin(h2f(r.d));
    }
    return w;
}

// NW waves; SPLIT: they share row group blockIdx.x and take TW columns each, else a row group each
template <int WT, int T, bool TL, bool SPLIT>
__global__ void __launch_bounds__(SPLIT ? 64 * (T < 4 ? T : 4) : 256) k_gemm_skinny_kq(kq_args a) {
    constexpr int NW = SPLIT ? (T < 4 ? T : 4) : 4, NTH = 64 * NW, TW = SPLIT ? (T + NW - 1) / NW : T;
    constexpr int CS = SKQ_CS, CW = CS * 73;       // dwords of one column's chunk
    constexpr int N_IT = T * CW, RA = (N_IT + NTH - 1) / NTH;
    __shared__ __attribute__((aligned(16))) uint32_t smem[2 * N_IT];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane >> 3, l = lane & 7, nsb = a.nsb;
    const int64_t n_groups = (a.rows + 7) / 8;
    const int64_t g_raw = SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * NW + wave;
    const int64_t g = g_raw < n_groups ? g_raw : n_groups - 1;  // idle waves re-read the last group, store nothing
    const int64_t row_raw = g * 8 + rr;
    const int64_t row = row_raw < a.rows ? row_raw : a.rows - 1;  // all lanes stay active for the folds
    const uint8_t *wrow = a.w + row * a.row_bytes;
    const int nch = (nsb + CS - 1) / CS;
    int tc[TW];  // this wave's columns (SPLIT: past T clamped to a duplicate that is not stored)
#pragma unroll
    for (int j = 0; j < TW; ++j) tc[j] = SPLIT ? (wave + NW * j < T ? wave + NW * j : T - 1) : j;

    // ---- activation staging: chunk c of every column -> registers -> the LDS buffer ---------------
    uint32_t sa[RA];
    auto stage_load = [&](int c) {
        const int w0 = c * CW, wn = nsb * 73;  // the chunk's first dword of a column, the column's dwords
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int it = tid + j * NTH, t = it / CW, k = it % CW;
            sa[j] = 0u;
            if (it < N_IT && w0 + k < wn) sa[j] = *(const uint32_t *)(a.x + (int64_t)t * a.x_col_stride + (int64_t)(w0 + k) * 4);
        }
    };
    auto stage_store = [&](uint32_t *buf) {
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int it = tid + j * NTH;
            if (it < N_IT) buf[it] = sa[j];  // [column][block of the chunk][73]
        }
    };

    stage_load(0);  // older than the ring: its LDS stores below do not wait for the weights
    kq_raw<WT> ring[CS];
#pragma unroll
    for (int i = 0; i < CS; ++i) ring[i] = kq_load<WT, TL>(wrow, i < nsb ? i : nsb - 1, l);
    stage_store(smem);
    stage_load(1);  // past the last chunk every load is predicated off

    float acc[TW], accm[TW];
#pragma unroll
    for (int j = 0; j < TW; ++j) acc[j] = accm[j] = 0.0f;

    for (int c = 0; c < nch; ++c) {
        const uint32_t *buf = smem + (c & 1) * N_IT;
        __syncthreads();  // chunk c is staged; every wave is done reading the other buffer
        stage_store(smem + ((c + 1) & 1) * N_IT);
        stage_load(c + 2);
#pragma unroll
        for (int i = 0; i < CS; ++i) {
            const int s = c * CS + i;
            const skq_dec<WT> w = skq_decode<WT>(ring[i], l);
            const int sn = s + CS;
            ring[i] = kq_load<WT, TL>(wrow, sn < nsb ? sn : nsb - 1, l);
            if (s >= nsb) continue;  // wave-uniform: the ragged last chunk
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                const uint32_t *xb = buf + (tc[j] * CS + i) * 73;  // the column's Q8_K block: d, q8[256], bsums[16]
                const float yd = __builtin_bit_cast(float, xb[0]);
                const uint32_t *q8 = xb + 1 + l;  // chunk m of lane l: dword 8m + l
                int sumi = 0;
#pragma unroll
                for (int m = 0; m < 8; ++m) sumi += w.sc[m] * sdot4k(w.q[m], q8[8 * m]);
                acc[j] = __builtin_fmaf(yd * w.d, (float)sumi, acc[j]);
                if constexpr (WT == T_Q4_K) {
                    // bsums 4k .. 4k + 3 of the lane's pair k = l & 3 (dwords 65 + 2k, 66 + 2k)
                    const uint32_t b0 = xb[65 + 2 * (l & 3)], b1 = xb[66 + 2 * (l & 3)];
                    const int S0 = (int)(int16_t)b0 + (int)(int16_t)(b0 >> 16), S1 = (int)(int16_t)b1 + (int)(int16_t)(b1 >> 16);
                    const int prod = w.mn0 * S0 + w.mn1 * S1;
                    if (l < 4) accm[j] = __builtin_fmaf(-yd * w.dmin, (float)prod, accm[j]);
                }
                // the chain's value pinned here: the column's dots and FMA stay in this slot
                asm volatile("" : "+v"(acc[j]));
            }
        }
    }

#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const bool own = (!SPLIT || wave + NW * j < T) && g_raw < n_groups;  // wave-uniform
        kq_store<WT>(a, tc[j], own ? row_raw : a.rows, l, acc[j], accm[j]);
    }
}

template <int WT, bool TL, bool SPLIT>
void skinny_kq_go(const kq_args &a, unsigned grid, hipStream_t s) {
    switch (a.ncols) {
#define SKQ_CASE(N)                                                                                                  \
    case N:                                                                                                          \
        hipLaunchKernelGGL((k_gemm_skinny_kq<WT, N, TL, SPLIT>), dim3(grid), dim3(SPLIT ? 64 * (N < 4 ? N : 4) : 256), 0, s, a); \
        break;
        SKQ_CASE(1) SKQ_CASE(2) SKQ_CASE(3) SKQ_CASE(4) SKQ_CASE(5) SKQ_CASE(6) SKQ_CASE(7) SKQ_CASE(8)
#undef SKQ_CASE
    }
}

}  // namespace

int launch_gemm_skinny_kq(int wtype, const kq_args &a, hipStream_t s) {
    if (a.ncols < 1 || a.ncols > GEMM_SKINNY_MAX_T) {
        set_error("gemm_skinny_kq: T = " + std::to_string(a.ncols) + " outside [1, " + std::to_string(GEMM_SKINNY_MAX_T) + "]");
        return -1;
    }
    if ((wtype != T_Q4_K && wtype != T_Q6_K) || a.nsb <= 0 || a.rows <= 0 || !a.w || !a.x || !a.y || a.x_col_stride % 4 ||
        ((uintptr_t)a.x & 3) || a.x_col_stride < (int64_t)a.nsb * 292) {
        set_error("gemm_skinny_kq: Q4_K / Q6_K rows of K = 256 * nsb against 4-byte aligned Q8_K columns");
        return -1;
    }
    if (a.pro != KQP_COPY || a.q8_mode != KQO_NONE || a.w2 || (a.gate_in && !a.gelu_tab)) {
        set_error("gemm_skinny_kq: takes a precomputed Q8_K image, one matrix and no hand-off");
        return -1;
    }
    if (a.tiled && wtype == T_Q6_K && a.nsb % 8) {
        set_error("gemm_skinny_kq: the lane-contiguous Q6_K layout needs K % 2048 == 0");
        return -1;
    }
    // a wave per row group, four groups per workgroup, where that still leaves a workgroup per CU;
    // narrower matrices put one row group on every workgroup and split its columns over the waves
    const int64_t groups = (a.rows + 7) / 8;
    const bool wide = (groups + 3) / 4 >= 256;
    const unsigned grid = (unsigned)(wide ? (groups + 3) / 4 : groups);
#define SKQ_GO(WT)                                            \
    do {                                                      \
        if (a.tiled && wide) skinny_kq_go<WT, true, false>(a, grid, s);  \
        else if (a.tiled) skinny_kq_go<WT, true, true>(a, grid, s);      \
        else if (wide) skinny_kq_go<WT, false, false>(a, grid, s);       \
        else skinny_kq_go<WT, false, true>(a, grid, s);                  \
    } while (0)
    if (wtype == T_Q4_K) SKQ_GO(T_Q4_K);
    else SKQ_GO(T_Q6_K);
#undef SKQ_GO
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
