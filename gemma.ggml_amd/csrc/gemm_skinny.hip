// gemm_skinny.hip — the exact Q4_0 / Q8_0 GEMM for 1 <= T <= 8 activation rows (the verify pass of
// speculative decoding, DESIGN.md §5b‴): Y[t][r] = vec_dot(W row r, Xq row t) (+ resid[t][r]).
//
// Order: matvec_impl.h's, unchanged.  One thread is one (row, AVX2 lane) of an 8-row tile; it walks
// the row's blocks in order with one fmaf(d_w*d_a, (float)isum, acc) per block and the 8 lanes are
// folded by fold8, so every (row, column) equals ggml's vec_dot, launch_gemm_exact and k_matvec bit
// for bit.  What is new is that a weight tile is loaded from HBM once and applied to all T columns:
// T independent accumulator chains per thread.
//
// Activations: the Q8_0 image of 8 columns at K = 16384 is 144 KiB, so it is staged in K chunks of
// CT = 8 weight tiles (Q4_0: 64 blocks, Q8_0: 32), double buffered in LDS (T = 8, Q4_0: 2 x 18 KiB
// per workgroup).  The chain order only needs a thread to walk its own blocks in order, which
// chunking keeps.  Reading the image from L2 per use instead would cost 16 global loads per column
// and tile against one weight load, and splitting the columns over two launches would stream the
// weights twice.  Chunk c + 2 is loaded into registers and chunk c + 1 stored to the other buffer in
// front of chunk c's compute: the loads are older than the compute's weight reloads and have a whole
// chunk to land, so the stores never wait for HBM.  The stores transpose into the lane-major layout
// of matvec_impl.h (uint4 [block / 4][lane] = 4 blocks of one lane), so the compute reads two
// ds_read_b128 of int8 and two of scales per Q4_0 tile and column.  One barrier per chunk.
//
// Q4_0 without an ns table: the nibbles are moved to the top of their bytes and biased,
// ((x << 4) ^ 0x80) = 16 * (x - 8) as int8, so v_dot4 gives 16 * isum exactly (|16 * isum| <=
// 16 * 4 * 8 * 127 < 2^24), and the staged activation scale is d_a / 16 (exact: a power of two, and
// d_a >= 2^-24).  fmaf((d_w * d_a / 16), (float)(16 * isum), acc) has the same real product as
// fmaf(d_w * d_a, (float)isum, acc) and one rounding: the same bits, with no per-column bias term
// and no second LDS table.  The weight transform is done once per tile, not per column.
//
// Weights: a CT-deep register ring per wave (8 KiB in flight), slot i refilled with the next
// chunk's tile right after its use; loads are never inside a branch (past the last tile the index
// is clamped and the re-read tile meets zeroed activations: d = 0, an exact no-op).  No K split:
// a (row tile, column) chain belongs to one wave for the whole K.  The 4 waves of a workgroup share
// a staged chunk and own 4 row tiles, or (SPLIT, narrow matrices) one row tile and a share of its
// columns each.
#include "matvec_impl.h"

namespace ghip {
namespace {

constexpr int SK_CT = 8;  // weight tiles per K chunk = depth of the register ring

// SPLIT (matrices with too few row tiles to fill the CUs four waves at a time, e.g. n_embd rows): the
// workgroup's 4 waves share ONE row tile and divide the columns (wave w: columns w, w + 4), each
// streaming the tile through its own ring (the re-reads hit L2).  A row tile's chains then run on
// all 4 SIMDs of its CU instead of one; a (row, column) chain is still one thread walking K in order.
template <int WT, int T, bool SPLIT>
__global__ void __launch_bounds__(256) k_gemm_skinny(gemm_args g) {
    constexpr int NW = 4, TW = SPLIT ? (T + 3) / 4 : T;  // waves per workgroup, columns per wave
    constexpr int BT = wfmt<WT>::BT, SB = wfmt<WT>::SCALE_BYTES;
    constexpr int CT = SK_CT, CB = CT * BT, NTH = 64 * NW;
    constexpr int ACT_COL = CB * 32;                  // bytes of one column's chunk of int8
    constexpr int BUF = T * (ACT_COL + CB * 4);       // + its block scales
    constexpr int N_ACT = T * CB * 2, N_DA = T * CB;  // 16-B activation items, scales per chunk
    constexpr int RA = (N_ACT + NTH - 1) / NTH, RD = (N_DA + NTH - 1) / NTH;
    constexpr float DSC = WT == T_Q4_0 ? 0.0625f : 1.0f;
    __shared__ __attribute__((aligned(16))) uint8_t smem[2 * BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane >> 3, l = lane & 7;
    const int64_t rt_raw = SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * NW + wave;
    int tc[TW];  // this wave's columns (SPLIT: past T clamped to a duplicate that is not stored)
#pragma unroll
    for (int j = 0; j < TW; ++j) tc[j] = SPLIT ? (wave + 4 * j < T ? wave + 4 * j : T - 1) : j;
    const int64_t rt = rt_raw < g.n_rt ? rt_raw : g.n_rt - 1;  // idle waves re-read the last tile, store nothing
    const int n_bt = (int)g.n_bt, nb = (int)g.nb;
    const int nch = (n_bt + CT - 1) / CT;

    // ---- the weight ring -----------------------------------------------------------------------
    uint4 wq[CT], ws[CT];
    const uint8_t *qrow = g.qs + rt * n_bt * 1024 + (uint32_t)lane * 16u;
    const uint8_t *srow = g.sc + rt * n_bt * 8 * SB + (uint32_t)rr * SB;
    auto wload = [&](int i, int bt) {
        bt = bt < n_bt ? bt : n_bt - 1;
        wq[i] = ld_nt16(qrow + (int64_t)bt * 1024);
        ws[i] = ld_scale<WT>(srow + (int64_t)bt * 8 * SB);
    };

    // ---- activation staging: chunk c -> registers -> LDS buffer (transposed) ---------------------
    uint4 sa[RA];
    float sd[RD];
    auto stage_load = [&](int c) {
        const int b0 = c * CB;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int it = tid + j * NTH;  // (column, block, half)
            const int t = it / (CB * 2), r = it % (CB * 2), b = b0 + (r >> 1);
            sa[j] = make_uint4(0, 0, 0, 0);
            if (it < N_ACT && b < nb) sa[j] = *(const uint4 *)(g.xq + (int64_t)t * g.ldq + (int64_t)b * 32 + (r & 1) * 16);
        }
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int it = tid + j * NTH;  // (column, block)
            const int t = it / CB, b = b0 + it % CB;
            sd[j] = 0.0f;
            if (it < N_DA && b < nb) sd[j] = g.da[(int64_t)t * g.ldd + b];
        }
    };
    auto stage_store = [&](uint8_t *buf) {
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int it = tid + j * NTH;
            if (it >= N_ACT) continue;
            const int t = it / (CB * 2), r = it % (CB * 2), b = r >> 1, l0 = (r & 1) * 4;
            uint32_t *dst = (uint32_t *)(buf + t * ACT_COL) + ((b >> 2) * 8 + l0) * 4 + (b & 3);
            dst[0] = sa[j].x; dst[4] = sa[j].y; dst[8] = sa[j].z; dst[12] = sa[j].w;
        }
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int it = tid + j * NTH;
            if (it < N_DA) ((float *)(buf + T * ACT_COL))[it] = sd[j] * DSC;  // [column][block]
        }
    };

    stage_load(0);  // older than the ring: its LDS stores below do not wait for the weights
#pragma unroll
    for (int i = 0; i < CT; ++i) wload(i, i);
    stage_store(smem);
    stage_load(1);  // past the last chunk every load is predicated off (b >= nb): zeros

    float acc[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) acc[t] = 0.0f;

    // one (tile, column) pair's LDS operands: Q4_0 two uint4 of int8 + 8 scales, Q8_0 one + 4
    struct opnd {
        uint4 a0, a1;
        float4 d0, d1;
    };
    for (int c = 0; c < nch; ++c) {
        const uint8_t *buf = smem + (c & 1) * BUF;
        __syncthreads();  // chunk c is staged; every wave is done reading the other buffer
        // chunk c + 1 (loaded a whole chunk ago) into the other buffer, chunk c + 2 into the registers.
        // Both sit in front of the compute: behind it, their predicated blocks let the compiler sink
        // every dot and FMA of the chunk below them, with all operands live (spills)
        stage_store(smem + ((c + 1) & 1) * BUF);
        stage_load(c + 2);
        auto ld = [&](int i, int j) {
            const int t = tc[j];
            const uint4 *at = (const uint4 *)(buf + t * ACT_COL);
            const float *dt = (const float *)(buf + T * ACT_COL) + t * CB + i * BT;
            opnd o;
            if constexpr (WT == T_Q4_0) {
                o.a0 = at[(2 * i) * 8 + l]; o.a1 = at[(2 * i + 1) * 8 + l];
                o.d0 = *(const float4 *)dt; o.d1 = *(const float4 *)(dt + 4);
            } else {
                o.a0 = at[i * 8 + l]; o.a1 = o.a0;
                o.d0 = *(const float4 *)dt; o.d1 = o.d0;
            }
            return o;
        };
        // The (tile, column) pairs in order, each pair's operands read one pair ahead of its FMAs.
        // The fences keep that shape: left alone, the scheduler hoists the reads of all CT x T pairs
        // above the first FMA and spills.
        opnd cur = ld(0, 0);
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const uint4 q = wq[i], scv = ws[i];
            wload(i, (c + 1) * CT + i);
            const uint32_t qv[4] = {q.x, q.y, q.z, q.w};
            const uint32_t sv[4] = {scv.x, scv.y, scv.z, scv.w};
            uint32_t lo[4], hi[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {  // Q4_0: 16 * (nibble - 8) as int8, once per tile
                lo[p] = WT == T_Q4_0 ? ((qv[p] << 4) & 0xF0F0F0F0u) ^ 0x80808080u : qv[p];
                hi[p] = WT == T_Q4_0 ? (qv[p] & 0xF0F0F0F0u) ^ 0x80808080u : 0u;
            }
#pragma unroll
            for (int t = 0; t < TW; ++t) {
                opnd nxt = cur;
                if (t + 1 < TW) nxt = ld(i, t + 1);
                else if (i + 1 < CT) nxt = ld(i + 1, 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (WT == T_Q4_0) {
                    const uint32_t av[8] = {cur.a0.x, cur.a0.y, cur.a0.z, cur.a0.w, cur.a1.x, cur.a1.y, cur.a1.z, cur.a1.w};
                    const float dav[8] = {cur.d0.x, cur.d0.y, cur.d0.z, cur.d0.w, cur.d1.x, cur.d1.y, cur.d1.z, cur.d1.w};
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int s0 = sdot4(lo[p], av[2 * p], 0);
                        const int s1 = sdot4(hi[p], av[2 * p + 1], 0);
                        const float d0 = mix_lo(sv[p], dav[2 * p]);
                        const float d1 = mix_hi(sv[p], dav[2 * p + 1]);
                        acc[t] = __builtin_fmaf(d0, (float)s0, acc[t]);
                        acc[t] = __builtin_fmaf(d1, (float)s1, acc[t]);
                    }
                } else {
                    const uint32_t av[4] = {cur.a0.x, cur.a0.y, cur.a0.z, cur.a0.w};
                    const float dav[4] = {cur.d0.x, cur.d0.y, cur.d0.z, cur.d0.w};
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int s = sdot4(lo[p], av[p], 0);
                        const float d = (p & 1) ? mix_hi(sv[p >> 1], dav[p]) : mix_lo(sv[p >> 1], dav[p]);
                        acc[t] = __builtin_fmaf(d, (float)s, acc[t]);
                    }
                }
                // the chain's value pinned here: keeps the pair's dots and FMAs in this slot (IR passes
                // otherwise pack the columns' chains into vectors or sink them, and spill)
                asm volatile("" : "+v"(acc[t]));
                __builtin_amdgcn_sched_barrier(0);
                cur = nxt;
            }
        }
    }

    const int64_t row = rt_raw * 8 + rr;
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const float v = fold8(acc[j]);
        const bool own = !SPLIT || wave + 4 * j < T;
        if (l == 0 && own && rt_raw < g.n_rt && row < g.rows) {
            const int64_t o = (int64_t)tc[j] * g.ldy + row;
            g.y[o] = g.resid ? v + g.resid[o] : v;  // ggml_add of the residual (EPI_ADD)
        }
    }
}

template <int WT, bool SPLIT>
void skinny_go(const gemm_args &g, unsigned grid, hipStream_t s) {
    switch (g.T) {
#define SK_CASE(N) case N: hipLaunchKernelGGL((k_gemm_skinny<WT, N, SPLIT>), dim3(grid), dim3(256), 0, s, g); break;
        SK_CASE(1) SK_CASE(2) SK_CASE(3) SK_CASE(4) SK_CASE(5) SK_CASE(6) SK_CASE(7) SK_CASE(8)
#undef SK_CASE
    }
}

}  // namespace

int launch_gemm_skinny(int wtype, int epi, const gemm_args &g, hipStream_t s) {
    if (g.T < 1 || g.T > GEMM_SKINNY_MAX_T) {
        set_error("gemm_skinny: T = " + std::to_string(g.T) + " outside [1, " + std::to_string(GEMM_SKINNY_MAX_T) + "]");
        return -1;
    }
    if ((wtype != T_Q4_0 && wtype != T_Q8_0) || (epi != EPI_STORE && epi != EPI_ADD) || (epi == EPI_ADD && !g.resid)) {
        set_error("gemm_skinny: unsupported (type, epilogue)");
        return -1;
    }
    if (!g.xq || !g.da || !g.y || g.rows <= 0 || g.nb <= 0 || g.nb * 32 > g.ldq || g.ldd < g.nb || g.ldq % 16 ||
        g.n_rt != (g.rows + 7) / 8 || g.n_bt * (wtype == T_Q4_0 ? 8 : 4) < g.nb) {
        set_error("gemm_skinny: needs the int8 activation image (xq, da) and a tiled matrix of K = 32 * nb");
        return -1;
    }
    gemm_args a = g;
    if (epi == EPI_STORE) a.resid = nullptr;
    // a wave per row tile, 4 row tiles per workgroup, where that still leaves a workgroup per CU;
    // narrow matrices (n_embd rows) put one row tile on every CU and split its columns over the waves
    const bool wide = (g.n_rt + 3) / 4 >= 256;
    const unsigned grid = (unsigned)(wide ? (g.n_rt + 3) / 4 : g.n_rt);
    if (wtype == T_Q4_0 && wide) skinny_go<T_Q4_0, false>(a, grid, s);
    else if (wtype == T_Q4_0) skinny_go<T_Q4_0, true>(a, grid, s);
    else if (wide) skinny_go<T_Q8_0, false>(a, grid, s);
    else skinny_go<T_Q8_0, true>(a, grid, s);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
