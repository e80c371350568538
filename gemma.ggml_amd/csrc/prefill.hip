// prefill.hip — the batched-prompt (prefill) path for gfx950: every MUL_MAT of the Gemma graph
// with col_num = T tokens becomes an int8 MFMA GEMM.
//
// Numerics: activations are quantized to Q8_0 exactly as ggml's INIT does
// (AVX2 quantize_row_q8_0, SURVEY A.2, bit-identical to the decode prologue), and the int32 dot of
// every 32-element block is exact (v_mfma_i32_16x16x32_i8 = one block).  Only the fp32 accumulation
// across blocks differs from ggml's AVX2 lane order (one chain acc = fmaf(d_w*d_a, isum, acc) in
// block order instead of 8 lane chains + fold), so prefill logits match the CPU path to ~1e-6
// relative (tests: 1e-3), while the per-token decode path stays bit-exact.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>

#include "device_util.h"
#include "kernels.h"
#include "pick.h"

namespace ghip {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

// quantize_row_q8_0 (AVX2) of one 32-element block held by a quad (8 values per lane):
// amax, d = amax/127 (fp16 RNE), id = 127/amax, rint; the int8 image and/or the same integers as f16
// (the exact GEMM's MFMA operand), and the block scale
__device__ __forceinline__ void quant_block_q8(const qrow_args &a, int64_t t, int64_t b, int q, const float v[8]) {
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    amax = fmaxf(amax, dpp_f<0xB1>(amax));
    amax = fmaxf(amax, dpp_f<0x4E>(amax));
    const uint32_t d16 = f2h(amax / 127.f);
    const float id = (amax != 0.0f) ? 127.f / amax : 0.0f;
    uint32_t pk[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int qi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) qi[k] = (int)__builtin_rintf(v[4 * h + k] * id);
        pk[h] = (uint32_t)(qi[0] & 0xFF) | ((uint32_t)(qi[1] & 0xFF) << 8) | ((uint32_t)(qi[2] & 0xFF) << 16) |
                ((uint32_t)(qi[3] & 0xFF) << 24);
    }
    if (a.q) *(uint2 *)(a.q + t * a.ldq + b * 32 + q * 8) = make_uint2(pk[0], pk[1]);
    if (a.qh) {
        uint32_t hv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q0 = (int8_t)(pk[k >> 1] >> (16 * (k & 1))), q1 = (int8_t)(pk[k >> 1] >> (16 * (k & 1) + 8));
            hv[k] = f2h((float)q0) | (f2h((float)q1) << 16);
        }
        *(uint4 *)(a.qh + t * a.ldq + b * 32 + q * 8) = make_uint4(hv[0], hv[1], hv[2], hv[3]);
    }
    if (q == 0) a.da[t * a.ldd + b] = h2f(d16);
}

// zero the K padding of row t's images (the GEMMs stage whole 256-element chunks)
__device__ __forceinline__ void quant_pad(const qrow_args &a, int64_t t, int tid, int nth) {
    const int64_t K = a.K, nb = K / 32;
    if (a.q)
        for (int64_t i = K + tid * 4; i < a.ldq; i += nth * 4) *(uint32_t *)(a.q + t * a.ldq + i) = 0;
    if (a.qh)
        for (int64_t i = K + tid * 2; i < a.ldq; i += nth * 2) *(uint32_t *)(a.qh + t * a.ldq + i) = 0;
    for (int64_t b = nb + tid; b < a.ldd; b += nth) a.da[t * a.ldd + b] = 0.0f;
}

// ---- rows -> Q8_0 (int8 image + f32 of the fp16 block scale) --------------------------------
// One 256-thread workgroup per token row; a quad of threads owns a block (8 elements each).
template <int MODE>
__global__ void __launch_bounds__(256) k_quant_rows(qrow_args a) {
    const int t = blockIdx.x, tid = threadIdx.x, q = tid & 3;
    const int64_t K = a.K, nb = K / 32;
    const float *x = a.x + (int64_t)t * a.ldx;
    const float *x2 = a.x2 ? a.x2 + (int64_t)t * a.ldx : nullptr;
    int64_t tok = 0;
    if (MODE == QR_EMBED_NORM) tok = a.tokens[t];
    auto load = [&](int64_t i0, float v[8]) {
        if (MODE == QR_EMBED_NORM) {
            // ggml_get_rows (dequantize_row_*) then ggml_scale by sqrt(E) (src/gemma_model.cpp:677-679)
            const int64_t rt = tok >> 3, rr = tok & 7;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t i = i0 + j, b = i >> 5;
                const int e = (int)(i & 31), l = e >> 2, k = e & 3;
                float w;
                if (a.emb_type == T_Q4_0) {
                    const int64_t tile = rt * a.emb_n_bt + (b >> 3), bi = b & 7;
                    const uint16_t d16 = ((const uint16_t *)(a.emb_sc + (tile * 8 + rr) * 16))[bi];
                    const uint8_t byte = a.emb_qs[tile * 1024 + (rr * 8 + l) * 16 + (bi >> 1) * 4 + k];
                    const int qv = (int)((bi & 1) ? (byte >> 4) : (byte & 15)) - 8;
                    w = (float)qv * pin(h2f(d16));
                } else {
                    const int64_t tile = rt * a.emb_n_bt + (b >> 2), bi = b & 3;
                    const uint16_t d16 = ((const uint16_t *)(a.emb_sc + (tile * 8 + rr) * 8))[bi];
                    const int qv = (int)(int8_t)a.emb_qs[tile * 1024 + (rr * 8 + l) * 16 + bi * 4 + k];
                    w = (float)qv * pin(h2f(d16));
                }
                v[j] = w * a.emb_scale;
            }
        } else {
            const float4 u = *(const float4 *)(x + i0), w4 = *(const float4 *)(x + i0 + 4);
            v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w; v[4] = w4.x; v[5] = w4.y; v[6] = w4.z; v[7] = w4.w;
            if (MODE == QR_GELU) {  // gelu(gate) (fp16 table) then ggml_mul by up
                const float4 g0 = *(const float4 *)(x2 + i0), g1 = *(const float4 *)(x2 + i0 + 4);
                const float up[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float g;
                    if (a.gelu_clamp && v[j] <= -10.0f) g = 0.0f;
                    else if (a.gelu_clamp && v[j] >= 10.0f) g = v[j];
                    else g = h2f(a.gelu_tab[f2h(v[j])]);
                    v[j] = g * up[j];
                }
            }
        }
    };
    float scale = 1.0f;
    if (MODE == QR_NORM || MODE == QR_EMBED_NORM) {
        double part = 0.0;
        for (int64_t b = tid >> 2; b < nb; b += 64) {
            float v[8];
            load(b * 32 + q * 8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) part += (double)(v[j] * v[j]);
            if (MODE == QR_EMBED_NORM) {
                float *eo = a.emb_out + (int64_t)t * a.ldx + b * 32 + q * 8;
                *(float4 *)eo = make_float4(v[0], v[1], v[2], v[3]);
                *(float4 *)(eo + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        __shared__ double red[4];
        part = wave_sum_f64(part);  // any order: the mean is certified
        if ((tid & 63) == 0) red[tid >> 6] = part;
        __syncthreads();
        const double sum = red[0] + red[1] + red[2] + red[3];
        const double q = div_by_n(sum, K);
        float mean = (float)q;
        if (__builtin_expect(!rms_mean_certain(q, K), 0))  // workgroup-uniform; rare: ggml's own order
            mean = (float)(seq_sumsq_wave(K, [&](int64_t i0, float v[8]) { load(i0, v); }) / (double)K);
        scale = 1.0f / sqrtf(mean + a.eps);
    }
    for (int64_t b = tid >> 2; b < nb; b += 64) {
        float v[8];
        load(b * 32 + q * 8, v);
        if (MODE == QR_NORM || MODE == QR_EMBED_NORM) {
            const float4 w0 = *(const float4 *)(a.norm_w + b * 32 + q * 8);
            const float4 w1 = *(const float4 *)(a.norm_w + b * 32 + q * 8 + 4);
            const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (v[j] * scale) * wv[j];  // rms_norm, then ggml_mul
        }
        quant_block_q8(a, t, b, q, v);
    }
    quant_pad(a, t, tid, 256);
}

// QR_GELU with the fp16 gelu table in LDS (128 KiB, loaded once per workgroup; one workgroup per CU
// walks rows t = blockIdx.x, + gridDim.x, ...): the per-element table lookups are LDS reads instead
// of dependent global loads.  Same values as k_quant_rows<QR_GELU> (the table's entries, the clamp
// rule, g * up, the same block quantizer): bit-identical.
constexpr int QG_THREADS = 1024;
__global__ void __launch_bounds__(QG_THREADS) k_quant_gelu_lds(qrow_args a, int T) {
    extern __shared__ __attribute__((aligned(16))) uint16_t gtab[];  // 65536 fp16 entries
    const int tid = threadIdx.x, q = tid & 3;
    for (int i = tid; i < 65536 / 8; i += QG_THREADS) ((uint4 *)gtab)[i] = ((const uint4 *)a.gelu_tab)[i];
    __syncthreads();
    const int64_t K = a.K, nb = K / 32;
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        const float *x = a.x + t * a.ldx, *x2 = a.x2 + t * a.ldx;
        for (int64_t b = tid >> 2; b < nb; b += QG_THREADS / 4) {
            const int64_t i0 = b * 32 + q * 8;
            const float4 u0 = *(const float4 *)(x + i0), u1 = *(const float4 *)(x + i0 + 4);
            const float4 g0 = *(const float4 *)(x2 + i0), g1 = *(const float4 *)(x2 + i0 + 4);
            float v[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
            const float up[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float g;
                if (a.gelu_clamp && v[j] <= -10.0f) g = 0.0f;
                else if (a.gelu_clamp && v[j] >= 10.0f) g = v[j];
                else g = h2f(gtab[f2h(v[j])]);
                v[j] = g * up[j];
            }
            quant_block_q8(a, t, b, q, v);
        }
        quant_pad(a, t, tid, QG_THREADS);
    }
}

// ---- int8 MFMA GEMM: Y[t][r] = sum_b (d_w[r][b] * d_a[t][b]) * isum_b(W[r], Xq[t]) ------------
// Workgroup tile 64 weight rows x 64 tokens, 4 waves of 32 x 32 (2 x 2 MFMA 16x16x32 tiles).  K is
// staged 8 blocks (256 int8) at a time: weight tiles of the decode layout are unpacked to plain int8
// rows in LDS (row stride 272 B: conflict-free ds_read_b64 of the MFMA operands), the token rows are
// copied as they are.  One MFMA = one block's exact int32 dot for 16 x 16 (row, token) pairs.
constexpr int GM = 64, GN = 64, GKB = 8, GS = 272;

template <int WT, int EPI>
__global__ void __launch_bounds__(256) k_gemm_q(gemm_args g) {
    __shared__ __attribute__((aligned(16))) int8_t As[GM * GS];
    __shared__ __attribute__((aligned(16))) int8_t Bs[GN * GS];
    __shared__ float dws[GM][GKB + 1];
    __shared__ float das[GN][GKB + 1];
    constexpr int BT = wfmt<WT>::BT, SB = wfmt<WT>::SCALE_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * GM, t0 = blockIdx.y * GN;
    const int wr = (wave & 1) * 32, wt = (wave >> 1) * 32;
    const int l16 = lane & 15, kg = lane >> 4;
    float acc[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[i][j][v] = 0.0f;

    const int64_t n_rt = g.n_rt, n_bt = g.n_bt;
    for (int64_t kb0 = 0; kb0 < g.nb; kb0 += GKB) {
        // stage weights: 8 row tiles x (8 / BT) block tiles, 64 lane records of 16 B each
        constexpr int TPR = GKB / BT;  // block tiles per row tile in one stage
        for (int rec = tid; rec < 8 * TPR * 64; rec += 256) {
            const int tile_i = rec >> 6, ln = rec & 63, rr = ln >> 3, l = ln & 7;
            const int rti = tile_i / TPR, bti = tile_i % TPR;
            int64_t rt = r0 / 8 + rti, bt = kb0 / BT + bti;
            const bool ok = rt < n_rt && bt < n_bt;
            rt = ok ? rt : 0;
            bt = ok ? bt : 0;
            const uint4 qv = *(const uint4 *)(g.qs + (rt * n_bt + bt) * 1024 + ln * 16);
            const uint32_t qd[4] = {qv.x, qv.y, qv.z, qv.w};
            int8_t *arow = As + (rti * 8 + rr) * GS + bti * BT * 32 + l * 4;
            if (WT == T_Q4_0) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    // byte k of dword p: low nibble = block 2p elem 4l+k, high = block 2p+1
                    const uint32_t lo = qd[p] & 0x0F0F0F0Fu, hi = (qd[p] >> 4) & 0x0F0F0F0Fu;
                    // nibble n -> int8 n - 8 per byte, no cross-byte borrow: v = n ^ 8 is n - 8 as a
                    // 4-bit two's complement; sign-extend it (bit 3 set -> high nibble 0xF)
                    const uint32_t vlo = lo ^ 0x08080808u, vhi = hi ^ 0x08080808u;
                    const uint32_t slo = vlo | ((vlo & 0x08080808u) * 0x1Eu);
                    const uint32_t shi = vhi | ((vhi & 0x08080808u) * 0x1Eu);
                    *(uint32_t *)(arow + (2 * p) * 32) = ok ? slo : 0u;
                    *(uint32_t *)(arow + (2 * p + 1) * 32) = ok ? shi : 0u;
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) *(uint32_t *)(arow + p * 32) = ok ? qd[p] : 0u;
            }
            if (l == 0) {
                const uint16_t *sp = (const uint16_t *)(g.sc + ((rt * n_bt + bt) * 8 + rr) * SB);
#pragma unroll
                for (int b = 0; b < BT; ++b) dws[rti * 8 + rr][bti * BT + b] = ok ? h2f(sp[b]) : 0.0f;
            }
        }
        // stage tokens: 64 rows x 256 int8 + their block scales
        for (int c = tid; c < GN * 16; c += 256) {
            const int row = c >> 4, seg = c & 15;
            const int64_t t = t0 + row < g.T ? t0 + row : 0;
            const uint4 v = *(const uint4 *)(g.xq + t * g.ldq + kb0 * 32 + seg * 16);
            *(uint4 *)(Bs + row * GS + seg * 16) = v;
        }
        for (int c = tid; c < GN * GKB; c += 256) {
            const int row = c >> 3, b = c & 7;
            const int64_t t = t0 + row < g.T ? t0 + row : 0;
            das[row][b] = (kb0 + b < g.nb) ? g.da[t * g.ldd + kb0 + b] : 0.0f;
        }
        __syncthreads();
#pragma unroll 2
        for (int b = 0; b < GKB; ++b) {
            long av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *(const long *)(As + (wr + i * 16 + l16) * GS + b * 32 + kg * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *(const long *)(Bs + (wt + j * 16 + l16) * GS + b * 32 + kg * 8);
            float dw[2][4], dt[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int v = 0; v < 4; ++v) dw[i][v] = dws[wr + i * 16 + kg * 4 + v][b];
#pragma unroll
            for (int j = 0; j < 2; ++j) dt[j] = das[wt + j * 16 + l16][b];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const v4i z = {0, 0, 0, 0};
                    const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(av[i], bv[j], z, 0, 0, 0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[i][j][v] = __builtin_fmaf(dw[i][v] * dt[j], (float)c[v], acc[i][j][v]);
                }
        }
        __syncthreads();
    }
    // epilogue: lane holds rows r0+wr+i*16+kg*4+v (4 consecutive) of token t0+wt+j*16+l16
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t t = t0 + wt + j * 16 + l16;
        if (t >= g.T) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t r = r0 + wr + i * 16 + kg * 4;
            float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            float *y = g.y + t * g.ldy + r;
            if (EPI == EPI_ADD) {
                const float *rs = g.resid + t * g.ldy + r;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (r + v < g.rows) o[v] = o[v] + rs[v];
            }
            if (r + 3 < g.rows && (g.ldy & 3) == 0) {
                *(float4 *)y = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (r + v < g.rows) y[v] = o[v];
            }
        }
    }
}

// ---- exact GEMM: ggml's AVX2 lane order for every (row, token) pair ------------------------------
// The reference computes each prompt row's MUL_MAT with the same vec_dot as decode:
// eight fp32 lane chains acc_l = fmaf(d_w*d_a, isum_l, acc_l) in block order, isum_l = the exact
// int32 dot of elements 4l..4l+3, then hsum ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)).
// The lane sums come from f16 MFMA with the lane structure in the M dimension: an MFMA row is one
// (weight row, AVX2 lane l), its A row holds only elements 4l..4l+3 of the block (zeros elsewhere),
// so D[m][token] = isum_l exactly (products and sums of small integers are exact in f32) and
// arrives as f32 — no conversion.  A lane's D registers hold the lanes of one (row, token), so one
// d = d_w*d_a (exact: two fp16 significands) serves their fmaf; the chain continues block after
// block in the same register: the identical operation sequence, so Y is bit-identical to mul_mat.
// Two kernels, five forms (gemm_form): k_gemm_x (the lane-masked 32x32x16 form, "W32") and
// k_gemm_x4 (the K = 4 multi-block form, the default).  Both: K is staged XKB = 8 blocks at a time,
// weights converted to f16 (Q4_0 nibbles / Q8_0 int8 by the 0x6400 exponent trick) on the way to
// LDS, tokens as f16 rows; blockIdx.x walks tokens so the token tiles of one weight tile run
// together and the weights leave HBM about once per XCD.
typedef _Float16 xh8 __attribute__((ext_vector_type(8)));
typedef float xf16v __attribute__((ext_vector_type(16)));

// four small integers (bytes of v, biased so they are in [0, 1024)) -> 2 dwords of f16 pairs
// f16(1024 + u) has bits 0x6400 | u; subtracting the bias (1024 + b) in f16 is exact
__device__ __forceinline__ uint2 bytes_to_f16x4(uint32_t v, uint32_t bias_pair) {
    const uint32_t lo = __builtin_amdgcn_perm(0u, v, 0x0c010c00u) | 0x64006400u;  // bytes 0,1
    const uint32_t hi = __builtin_amdgcn_perm(0u, v, 0x0c030c02u) | 0x64006400u;  // bytes 2,3
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 b = __builtin_bit_cast(h2, bias_pair);
    const h2 l2 = __builtin_bit_cast(h2, lo) - b, h2v = __builtin_bit_cast(h2, hi) - b;
    return make_uint2(__builtin_bit_cast(uint32_t, l2), __builtin_bit_cast(uint32_t, h2v));
}

constexpr int XCT = 2;                    // 16-token MFMA column tiles per wave
constexpr int XRT = 8;                    // 2-row MFMA row tiles per wave, i.e. XRT/4 8-row groups (8 measured best)
constexpr int XW = 4;                     // waves per workgroup: XWR row groups x XWC token groups
constexpr int XNT = 64 * XW;
constexpr int XM = 32, XWR = XM / (2 * XRT), XWC = XW / XWR, XN = XWC * 16 * XCT, XKB = 8;
static_assert(XWR * XWC == XW && XWR * 2 * XRT == XM, "wave grid");
static_assert(XRT % 4 == 0 && XCT == 2, "waves of 8*RG rows x 32 tokens");
constexpr int XS_ROW = XKB * 32 * 2 + 16;  // bytes per staged token row (f16, padded)
constexpr int XREC = XN * XKB * 64 / 16 / XNT;  // 16-B token records per thread per stage
static_assert(XN * XKB * 64 / 16 % XNT == 0, "token records");

typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// The W32 form (hpc_set_gemm_x4(0)): the lane sums from v_mfma_f32_32x32x16_f16.  K = 16 covers half
// a block, and only the four AVX2 lanes 4h..4h+3 have elements in half h, so MFMA row m = 4*row + i
// (i = lane & 3 of half h) wastes 3/4 of each A row: a wave's 8 rows x 32 tokens per block take two
// 32x32x16 MFMAs (h = 0, 1) and four 16-B LDS fragment reads.  D row m = (reg & 3) + 8*(reg >> 2) +
// 4*(lane >> 5) puts the four lanes of one (row, token) in consecutive registers and both halves in
// the same lane, so the hsum needs no lane exchange.  Same operands, same products, same fmaf chains
// as the 16x16x32 restatement it replaced: bit-identical.
// Workgroup tile XM = 32 rows x XN = 64 tokens, 4 waves of 16 rows x 32 tokens; weights staged as
// pre-masked 16-B A fragments per (block, row, lane), tokens from the quantizer's f16 image.
template <int WT, int EPI>
__global__ void __launch_bounds__(XNT) k_gemm_x(gemm_args g) {
    constexpr int RG = XRT / 4;  // 8-row groups per wave
    // A fragments: [b][row][lane] 16 B (lane l's 4 f16 in half l&1 of the fragment) + a zero region
    // the inactive lanes read at the same strides (no per-lane select).  The fragment rows are padded
    // to WFR = 9 x 16 B: the 8 active lanes of a ds_read_b128 lane group then hit distinct banks
    // (rows 2 apart would share them at 8 x 16 B)
    constexpr int WFR = 9;
    __shared__ __attribute__((aligned(16))) uint4 Wf[XKB * XM * WFR + 7 * 16 + 1];
    __shared__ __attribute__((aligned(16))) uint8_t Xs[XN * XS_ROW];
    __shared__ __attribute__((aligned(16))) float dws[XKB][2][XM / 2];  // [b][row & 1][row >> 1]
    __shared__ __attribute__((aligned(16))) float das[XKB][XN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave % XWR) * 2 * XRT, wt = (wave / XWR) * 16 * XCT;  // wave tile: rows wr.., tokens wt..
    const int64_t t0 = (int64_t)blockIdx.x * XN, r0 = (int64_t)blockIdx.y * XM;
    const int64_t n_rt = g.n_rt, n_bt = g.n_bt, nb = g.nb;
    // this lane's A fragment: MFMA row (lane & 31) = 4 * row + (lane & 3); the lane's k group
    // 8*(lane >> 5) .. holds the elements of AVX2 lane 4h + (lane & 3) iff (lane >> 5) == (lane & 3) >> 1
    const bool a_act = (lane >> 5) == ((lane & 3) >> 1);
    // inactive lanes read zeros from the slot of a 256-B zero row that none of the active lanes of
    // their ds_read_b128 lane group uses (MI355X_MICROARCH §LDS: b128 lane groups {0-3,12-15,
    // 20-27}, {4-11,16-19,28-31} and the same + 32; bank (a/4) mod 64): with one shared zero slot
    // the group read it as one more distinct 16-B address on busy banks (A reads 7 / 6 LDS cycles
    // instead of 4; scripts/lds_banks.py gemm_x_zero_search).  Table for WFR = 9: [group][half].
    constexpr int ZC[4][2] = {{2, 3}, {1, 0}, {1, 0}, {0, 1}};
    const int x32 = lane & 31;
    const int zg = 2 * (lane >> 5) + ((x32 >= 4 && x32 < 12) || (x32 >= 16 && x32 < 20) || x32 >= 28 ? 1 : 0);
    const uint4 *a_ptr = !a_act ? &Wf[XKB * XM * WFR + ZC[zg][0]] : &Wf[(wr + ((lane & 31) >> 2)) * WFR + (lane & 3)];
    const int a_bstride = a_act ? XM * WFR : 0;
    // the half-1 lanes' fragments (lane 4 + (lane & 3)); the next 8-row group (8 * WFR, i.e. the
    // active slots move by 8 of 16: the zero slot moves with them)
    const int a_hoff = a_act ? 4 : ZC[zg][1] - ZC[zg][0];
    const int a_rgoff = a_act ? 8 * WFR : 8;
    for (int i = tid; i < 7 * 16 + 1; i += XNT) Wf[XKB * XM * WFR + i] = make_uint4(0u, 0u, 0u, 0u);

    // one stage's global loads, in registers: the next stage's are in flight during the current stage's MFMAs
    constexpr int BT = wfmt<WT>::BT;
    constexpr int WRECS = (WT == T_Q4_0) ? 256 : 512;  // 16-B weight records per stage
    constexpr int WREC = (WRECS + XNT - 1) / XNT;      // per thread
    constexpr int XDA = (XN * XKB + XNT - 1) / XNT;    // token scales per thread per stage
    u4v wq[WREC], ws[WREC], xr[XREC];
    float xd[XDA];
    auto gload = [&](int64_t kb0) {
#pragma unroll
        for (int k = 0; k < WREC; ++k) {
            const int rec = tid + XNT * k, tile_i = (rec >> 6) & 7, ln = rec & 63, rr = ln >> 3;
            if (rec >= WRECS) break;  // wave-uniform
            const int rti = (WT == T_Q4_0) ? (tile_i & 3) : (tile_i >> 1), bti = (WT == T_Q4_0) ? 0 : (tile_i & 1);
            int64_t rt = r0 / 8 + rti, bt = kb0 / BT + bti;
            const bool ok = rt < n_rt && bt < n_bt;
            rt = ok ? rt : 0;
            bt = ok ? bt : 0;
            wq[k] = *(const u4v *)(g.qs + (rt * n_bt + bt) * 1024 + ln * 16);
            const uint8_t *sp = g.sc + ((rt * n_bt + bt) * 8 + rr) * wfmt<WT>::SCALE_BYTES;
            if (WT == T_Q4_0) ws[k] = *(const u4v *)sp;
            else { const uint2 s2 = *(const uint2 *)sp; ws[k] = u4v{s2.x, s2.y, 0u, 0u}; }
            if (!ok) { wq[k] = u4v{0u, 0u, 0u, 0u}; ws[k] = u4v{0u, 0u, 0u, 0u}; }
        }
#pragma unroll
        for (int k = 0; k < XREC; ++k) {  // XN tokens x 512 B in 16-B records
            const int rec = tid + XNT * k, tok = rec >> 5, seg = rec & 31;
            const int64_t t = t0 + tok < g.T ? t0 + tok : 0;
            xr[k] = *(const u4v *)(g.xh + t * g.ldq + kb0 * 32 + seg * 8);
        }
#pragma unroll
        for (int k = 0; k < XDA; ++k) {
            const int c = (tid + XNT * k) % (XN * 8), tok = c >> 3, b = c & 7;
            const int64_t t = t0 + tok < g.T ? t0 + tok : 0;
            xd[k] = (kb0 + b < nb) ? g.da[t * g.ldd + kb0 + b] : 0.0f;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int k = 0; k < WREC; ++k) {
            const int rec = tid + XNT * k, tile_i = (rec >> 6) & 7, ln = rec & 63, rr = ln >> 3, l = ln & 7;
            if (rec >= WRECS) break;  // wave-uniform
            const int rti = (WT == T_Q4_0) ? (tile_i & 3) : (tile_i >> 1), bti = (WT == T_Q4_0) ? 0 : (tile_i & 1);
            const int row = rti * 8 + rr;
            const uint32_t qd[4] = {wq[k].x, wq[k].y, wq[k].z, wq[k].w};
            const uint32_t sd[4] = {ws[k].x, ws[k].y, ws[k].z, ws[k].w};
            auto put = [&](int b, uint2 f) {
                Wf[(b * XM + row) * WFR + l] = (l & 1) ? make_uint4(0u, 0u, f.x, f.y) : make_uint4(f.x, f.y, 0u, 0u);
            };
            if (WT == T_Q4_0) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {  // nibble n -> f16(n - 8): bias 1032
                    put(2 * p, bytes_to_f16x4(qd[p] & 0x0F0F0F0Fu, 0x64086408u));
                    put(2 * p + 1, bytes_to_f16x4((qd[p] >> 4) & 0x0F0F0F0Fu, 0x64086408u));
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)  // int8 q -> f16(q): byte q ^ 0x80 = q + 128, bias 1152
                    put(bti * 4 + p, bytes_to_f16x4(qd[p] ^ 0x80808080u, 0x64806480u));
            }
            if (l == 0) {
#pragma unroll
                for (int b = 0; b < BT; ++b) dws[(WT == T_Q4_0 ? 0 : bti * 4) + b][row & 1][row >> 1] = h2f(sd[b >> 1] >> (16 * (b & 1)));
            }
        }
#pragma unroll
        for (int k = 0; k < XREC; ++k) {
            const int rec = tid + XNT * k, tok = rec >> 5, seg = rec & 31;
            *(u4v *)(Xs + tok * XS_ROW + seg * 16) = xr[k];
        }
#pragma unroll
        for (int k = 0; k < XDA; ++k) {
            const int c = tid + XNT * k;
            if (c < XN * 8) das[c & 7][c >> 3] = xd[k];
        }
    };

    // one block's operands from LDS and its step: all MFMAs of the block first (back-to-back on the
    // matrix pipe), then the lane-chain fmafs
    const int n32 = lane & 31, g32 = lane >> 5;
    float acc[RG][4][8];
#pragma unroll
    for (int q = 0; q < RG; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int l = 0; l < 8; ++l) acc[q][j][l] = 0.0f;
    struct frag { xh8 a[RG][2]; xh8 b[2]; float dw[RG][4]; float da; };
    auto ldfrag = [&](int b, frag &f) {
#pragma unroll
        for (int q = 0; q < RG; ++q) {
            const uint4 *ab = a_ptr + b * a_bstride + q * a_rgoff;
            f.a[q][0] = *(const xh8 *)ab;
            f.a[q][1] = *(const xh8 *)(ab + a_hoff);
            const float4 dwq = *(const float4 *)&dws[b][g32][wr / 2 + 4 * q];
            f.dw[q][0] = dwq.x; f.dw[q][1] = dwq.y; f.dw[q][2] = dwq.z; f.dw[q][3] = dwq.w;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) f.b[h] = *(const xh8 *)(Xs + (wt + n32) * XS_ROW + b * 64 + h * 32 + g32 * 16);
        f.da = das[b][wt + n32];
    };
    auto block = [&](const frag &f) {
        const xf16v z = {};
        xf16v d[RG][2];
#pragma unroll
        for (int q = 0; q < RG; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h) d[q][h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[q][h], f.b[h], z, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < RG; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float dd = f.dw[q][j] * f.da;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[q][j][i] = __builtin_fmaf(dd, d[q][0][4 * j + i], acc[q][j][i]);
                    acc[q][j][4 + i] = __builtin_fmaf(dd, d[q][1][4 * j + i], acc[q][j][4 + i]);
                }
            }
    };

    gload(0);
    for (int64_t kb0 = 0; kb0 < nb; kb0 += XKB) {
        lstore();
        __syncthreads();
        if (kb0 + XKB < nb) gload(kb0 + XKB);
        const int nbs = (int)(nb - kb0 < XKB ? nb - kb0 : XKB);
        for (int b = 0; b < nbs; ++b) {
            frag cur;
            ldfrag(b, cur);
            block(cur);
        }
        __syncthreads();
    }
    // hsum in registers: ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7))
    const int64_t t = t0 + wt + n32;
#pragma unroll
    for (int q = 0; q < RG; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *a = acc[q][j];
            float o = ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
            const int64_t r = r0 + wr + 8 * q + 2 * j + g32;
            if (t >= g.T || r >= g.rows) continue;
            if (EPI == EPI_ADD) o = o + g.resid[t * g.ldy + r];
            g.y[t * g.ldy + r] = o;
        }
}

// ---- exact GEMM on the K = 4 multi-block MFMA ------------------------------------
// v_mfma_f32_16x16x4_4b_f16 = FOUR independent 16x16x4 products, one per block of 16 lanes: block
// b of the instruction is ONE AVX2 lane l of ggml's vec_dot_q4_0_q8_0 — A = the 4 weights 4l..4l+3
// of 16 rows, B = the same 4 activations of 16 tokens — so D[b][row][token] = isum_l exactly (4
// products of small integers, f32 accumulate; tests/micro/mfma_k4.hip: every output integral and
// equal) and EVERY product is useful: the W32 form's A fragments are 3/4 zeros (8x the Q4_0 bytes
// in LDS), here they are the 8 dense bytes of (row, lane).  Two instructions cover a block's 8
// lanes.  Layout (probed, tests/micro/mfma_k4.hip): A lane L = (block L/16, row L%16), B lane L =
// (block L/16, token L%16), D register r of lane L = (block r/4, row 4*(L/16) + r%4, token L%16):
// each lane holds 4 rows x 8 lanes of one token per token group, so the fmaf chains and the final
// hsum ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)) stay in the lane's registers.  Same operands, same
// d = d_w*d_a, same fmaf sequence in block order as k_gemm_x: bit-identical.
// Tile: 4 waves = 2 row groups (16 rows) x 2 token groups (32 tokens); XKB = 8 blocks per stage.
// LDS: A as [block][row group][lane][16 rows] x 8 B (a 32-lane half of a b64 read = 256 contiguous
// bytes: conflict-free), tokens as k_gemm_x's padded f16 rows.
typedef _Float16 xh4 __attribute__((ext_vector_type(4)));
constexpr int X4_ACOL = 16 * 8;                          // bytes per (block, row group, lane) column
// RGS: row groups (16 rows) per workgroup — 2: 32 rows x 64 tokens, 4: 64 rows x 32 tokens (the token
// image, re-read by every row tile, is the bulk of the staging: 64 rows halve it)
// XI: the activation staged from the int8 Q8_0 image (g.xq, 32 B per block and token: half the
// global / L2 bytes of the f16 image) and converted to f16 while it is written to LDS (q ^ 0x80
// over bias 1152: exact), instead of read as the f16 image g.xh
// 3 waves per SIMD: what the register budget must allow (LDS: 53 KB per workgroup fits 3 per CU)
template <int WT, int EPI, int RGS, int XI = 0>
__global__ void __launch_bounds__(XNT) __attribute__((amdgpu_waves_per_eu(3, 3))) k_gemm_x4(gemm_args g) {
    static_assert(XNT == 256 && (RGS == 2 || RGS == 4), "4 waves: RGS row groups x 4/RGS token groups");
    constexpr int M4 = 16 * RGS, N4 = 32 * (4 / RGS), X4_ABLK = RGS * 8 * X4_ACOL;
    constexpr int XREC4 = N4 * XKB * (XI ? 32 : 64) / 16 / XNT;
    constexpr int XSEG = XKB * (XI ? 32 : 64) / 16;  // 16-B global records per token and stage
    __shared__ __attribute__((aligned(16))) uint8_t Wa[XKB * X4_ABLK];
    __shared__ __attribute__((aligned(16))) uint8_t Xs[N4 * XS_ROW];
    __shared__ __attribute__((aligned(16))) float dws[XKB][M4];
    __shared__ __attribute__((aligned(16))) float das[XKB][N4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave % RGS, tg = wave / RGS;        // this wave: rows 16*rg.., tokens 32*tg..
    const int q = lane >> 4, l16 = lane & 15;
    const int64_t t0 = (int64_t)blockIdx.x * N4, r0 = (int64_t)blockIdx.y * M4;
    const int64_t n_rt = g.n_rt, n_bt = g.n_bt, nb = g.nb;

    // [token group][AVX2 lane][row pair]: rows (2p, 2p+1) of one lane chain pair as one float2, as
    // their D registers sit side by side, so each v_pk_fma_f32 takes them with no register moves
    // (two independent fmaf chains per instruction: the same roundings as two v_fma_f32)
    typedef float xf2 __attribute__((ext_vector_type(2)));
    xf2 acc[2][8][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int l = 0; l < 8; ++l)
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2) acc[c][l][p2] = xf2{0.0f, 0.0f};

    constexpr int BT = wfmt<WT>::BT;
    constexpr int WRECS = (M4 / 8) * 64 * (WT == T_Q4_0 ? 1 : 2);  // 16-B weight records per stage
    constexpr int WREC = (WRECS + XNT - 1) / XNT;
    constexpr int XDA4 = (N4 * XKB + XNT - 1) / XNT;
    u4v wq[WREC], ws[WREC], xr[XREC4];
    float xd[XDA4];
    auto gload = [&](int64_t kb0) {
#pragma unroll
        for (int k = 0; k < WREC; ++k) {
            const int rec = tid + XNT * k, tile_i = rec >> 6, ln = rec & 63, rr = ln >> 3;
            if (rec >= WRECS) break;  // wave-uniform
            const int rti = (WT == T_Q4_0) ? tile_i : (tile_i >> 1), bti = (WT == T_Q4_0) ? 0 : (tile_i & 1);
            int64_t rt = r0 / 8 + rti, bt = kb0 / BT + bti;
            const bool ok = rt < n_rt && bt < n_bt;
            rt = ok ? rt : 0;
            bt = ok ? bt : 0;
            wq[k] = *(const u4v *)(g.qs + (rt * n_bt + bt) * 1024 + ln * 16);
            const uint8_t *sp = g.sc + ((rt * n_bt + bt) * 8 + rr) * wfmt<WT>::SCALE_BYTES;
            if (WT == T_Q4_0) ws[k] = *(const u4v *)sp;
            else { const uint2 s2 = *(const uint2 *)sp; ws[k] = u4v{s2.x, s2.y, 0u, 0u}; }
            if (!ok) { wq[k] = u4v{0u, 0u, 0u, 0u}; ws[k] = u4v{0u, 0u, 0u, 0u}; }
        }
#pragma unroll
        for (int k = 0; k < XREC4; ++k) {
            const int rec = tid + XNT * k, tok = rec / XSEG, seg = rec % XSEG;
            const int64_t t = t0 + tok < g.T ? t0 + tok : 0;
            if (XI) xr[k] = *(const u4v *)(g.xq + t * g.ldq + kb0 * 32 + seg * 16);
            else xr[k] = *(const u4v *)(g.xh + t * g.ldq + kb0 * 32 + seg * 8);
        }
#pragma unroll
        for (int k = 0; k < XDA4; ++k) {
            const int c = (tid + XNT * k) % (N4 * 8), tok = c >> 3, b = c & 7;
            const int64_t t = t0 + tok < g.T ? t0 + tok : 0;
            xd[k] = (kb0 + b < nb) ? g.da[t * g.ldd + kb0 + b] : 0.0f;
        }
    };
    auto lstore = [&]() {
        // A: row slot swizzled by the lane: (row & 15) ^ 2l, so each 16-lane group (rr 2 values x l 0..7)
        // of a ds_write_b64 lands on 32 distinct banks (unswizzled: 8-way, 50 % of the LDS cycles
        // conflicts in the PMC; scripts/lds_banks.py); a 16-row column stays one contiguous 128 B
#pragma unroll
        for (int k = 0; k < WREC; ++k) {
            const int rec = tid + XNT * k, tile_i = rec >> 6, ln = rec & 63, rr = ln >> 3, l = ln & 7;
            if (rec >= WRECS) break;  // wave-uniform
            const int rti = (WT == T_Q4_0) ? tile_i : (tile_i >> 1), bti = (WT == T_Q4_0) ? 0 : (tile_i & 1);
            const int row = rti * 8 + rr;  // 0..M4-1
            const uint32_t qd[4] = {wq[k].x, wq[k].y, wq[k].z, wq[k].w};
            const uint32_t sd[4] = {ws[k].x, ws[k].y, ws[k].z, ws[k].w};
            // row slot swizzled by the lane: (row & 15) ^ 2l, so each 16-lane group (rr 2 values x l 0..7)
            // of a ds_write_b64 lands on 32 distinct banks (unswizzled: 8-way, 50 % of the LDS cycles
            // conflicts in the PMC; scripts/lds_banks.py); a 16-row column stays one contiguous 128 B
            uint8_t *col = Wa + ((row >> 4) * 8 + l) * X4_ACOL + (((row & 15) ^ (2 * l)) & 15) * 8;
            auto put = [&](int b, uint2 f) { *(uint2 *)(col + b * X4_ABLK) = f; };
            if (WT == T_Q4_0) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {  // nibble n -> f16(n - 8): bias 1032
                    put(2 * p, bytes_to_f16x4(qd[p] & 0x0F0F0F0Fu, 0x64086408u));
                    put(2 * p + 1, bytes_to_f16x4((qd[p] >> 4) & 0x0F0F0F0Fu, 0x64086408u));
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)  // int8 q -> f16(q): byte q ^ 0x80 = q + 128, bias 1152
                    put(bti * 4 + p, bytes_to_f16x4(qd[p] ^ 0x80808080u, 0x64806480u));
            }
            if (l == 0) {
#pragma unroll
                for (int b = 0; b < BT; ++b) dws[(WT == T_Q4_0 ? 0 : bti * 4) + b][row] = h2f(sd[b >> 1] >> (16 * (b & 1)));
            }
        }
        // token rows: the 8-B chunks of tokens 8..15 (of every 16) swapped within their 16 B, so the
        // compiler's ds_read2_b64 of B (16-lane groups, banks mod 32) sees tokens j and j + 8 on
        // different banks (pitch 528 B alone: 2-way)
#pragma unroll
        for (int k = 0; k < XREC4; ++k) {
            const int rec = tid + XNT * k, tok = rec / XSEG, seg = rec % XSEG;
            const u4v v = xr[k];
            if (XI) {  // 16 int8 -> 16 f16 = two 16-B chunks of the f16 row
                const uint2 c0 = bytes_to_f16x4(v.x ^ 0x80808080u, 0x64806480u), c1 = bytes_to_f16x4(v.y ^ 0x80808080u, 0x64806480u);
                const uint2 c2 = bytes_to_f16x4(v.z ^ 0x80808080u, 0x64806480u), c3 = bytes_to_f16x4(v.w ^ 0x80808080u, 0x64806480u);
                const u4v h0 = (tok & 8) ? u4v{c1.x, c1.y, c0.x, c0.y} : u4v{c0.x, c0.y, c1.x, c1.y};
                const u4v h1 = (tok & 8) ? u4v{c3.x, c3.y, c2.x, c2.y} : u4v{c2.x, c2.y, c3.x, c3.y};
                // a record's two f16 chunks go to the row's two halves (chunk 2s at s, 2s + 1 at 16 + s),
                // so each b128 store instruction covers consecutive 16-B slots (chunks 2s, 2s + 1 side
                // by side put a 32-B lane stride in every store: 21 % conflict cycles in the PMC)
                *(u4v *)(Xs + tok * XS_ROW + seg * 16) = h0;
                *(u4v *)(Xs + tok * XS_ROW + 256 + seg * 16) = h1;
            } else {
                *(u4v *)(Xs + tok * XS_ROW + seg * 16) = (tok & 8) ? u4v{v.z, v.w, v.x, v.y} : v;
            }
        }
#pragma unroll
        for (int k = 0; k < XDA4; ++k) {
            const int c = tid + XNT * k;
            if (c < N4 * 8) das[c & 7][c >> 3] = xd[k];
        }
    };
    // this lane's operand addresses: A column (row group rg, AVX2 lane 4*ih + q, row l16), B (token
    // 32*tg + 16*c + l16, the same lane's 4 elements)
    const uint8_t *a_base = Wa + (rg * 8 + q) * X4_ACOL + ((l16 ^ (2 * q)) & 15) * 8;              // lane q
    const uint8_t *a_base1 = Wa + (rg * 8 + 4 + q) * X4_ACOL + ((l16 ^ (8 + 2 * q)) & 15) * 8;     // lane 4 + q
    // chunk 4*ih + q, 8-B halves swapped for tokens with bit 3 set; XI: old chunk c at slot c/2 (even c)
    // or 16 + c/2 (odd c), i.e. the lane's parity bit (q ^ swap) >> 1 picks the row half, blocks 32 B apart
    const int qs_ = q ^ ((l16 >> 3) & 1);
    const uint8_t *b_base = Xs + (32 * tg + l16) * XS_ROW + (XI ? ((qs_ >> 1) & 1) * 256 + (qs_ & 1) * 8 : qs_ * 8);
    constexpr int BSTEP = XI ? 32 : 64, BHALF = XI ? 16 : 32;  // bytes per block, second AVX2 half
    // one block's operands: A: 2 lanes' fragments, B: 2 token groups x 2, d_w of the lane's 4 rows, d_a
    // of its 2 tokens
    struct x4ops {
        xh4 a0, a1, bb[2][2];
        float4 dw4;
        float da[2];
    };
    auto ldops = [&](int b, x4ops &o) {
        o.a0 = *(const xh4 *)(a_base + b * X4_ABLK);
        o.a1 = *(const xh4 *)(a_base1 + b * X4_ABLK);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            o.bb[c][0] = *(const xh4 *)(b_base + c * 16 * XS_ROW + b * BSTEP);
            o.bb[c][1] = *(const xh4 *)(b_base + c * 16 * XS_ROW + b * BSTEP + BHALF);
            o.da[c] = das[b][32 * tg + 16 * c + l16];
        }
        o.dw4 = *(const float4 *)&dws[b][16 * rg + 4 * q];
    };
    auto compute = [&](const x4ops &o) {
        const float dw[4] = {o.dw4.x, o.dw4.y, o.dw4.z, o.dw4.w};
        const xf16v z = {};
        auto group = [&](int c) {
            xf16v d[2];
            d[0] = __builtin_amdgcn_mfma_f32_16x16x4f16(o.a0, o.bb[c][0], z, 0, 0, 0);
            d[1] = __builtin_amdgcn_mfma_f32_16x16x4f16(o.a1, o.bb[c][1], z, 0, 0, 0);
            xf2 dd[2];
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2) dd[p2] = xf2{dw[2 * p2] * o.da[c], dw[2 * p2 + 1] * o.da[c]};
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int bq = 0; bq < 4; ++bq)  // D registers 4*bq .. 4*bq+3: AVX2 lane 4*h + bq, rows 0..3
#pragma unroll
                    for (int p2 = 0; p2 < 2; ++p2) {
                        const xf2 dv = {d[h][4 * bq + 2 * p2], d[h][4 * bq + 2 * p2 + 1]};
                        acc[c][4 * h + bq][p2] = __builtin_elementwise_fma(dd[p2], dv, acc[c][4 * h + bq][p2]);
                    }
        };
        // a block's two token groups one after the other (half the MFMA results live): token group
        // 1's MFMAs after group 0's chains
        group(0);
        __builtin_amdgcn_sched_barrier(0);
        group(1);
    };

    for (int64_t kb0 = 0; kb0 < nb; kb0 += XKB) {
        gload(kb0);  // (no register prefetch: the other workgroups of the CU overlap)
        lstore();
        __syncthreads();
        const int nbs = (int)(nb - kb0 < XKB ? nb - kb0 : XKB);
#pragma unroll 1
        for (int b = 0; b < nbs; ++b) {
            x4ops cur;
            ldops(b, cur);
            compute(cur);
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t t = t0 + 32 * tg + 16 * c + l16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float a[8];
#pragma unroll
            for (int l = 0; l < 8; ++l) a[l] = acc[c][l][i >> 1][i & 1];
            float o = ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
            const int64_t r = r0 + 16 * rg + 4 * q + i;
            if (t >= g.T || r >= g.rows) continue;
            if (EPI == EPI_ADD) o = o + g.resid[t * g.ldy + r];
            g.y[t * g.ldy + r] = o;
        }
    }
}

// ---- RoPE + q scale + KV store for T prompt tokens (positions p0 .. p0+T-1) --------------------
// Same per-element arithmetic as the decode attention (src/gemma_model.cpp:698-718, 499-518).
__global__ void __launch_bounds__(256) k_rope_kv_prefill(ropekv_args a) {
    const int t = blockIdx.x, tid = threadIdx.x, half = a.hd / 2, p = a.p0 + t;
    const float *row = a.qkv + (int64_t)t * a.ldqkv;
    const float *cs = a.rope_cos + (int64_t)p * half, *sn = a.rope_sin + (int64_t)p * half;
    const int kvw = a.Hkv * a.hd;
    for (int i = tid; i < a.H * half; i += 256) {
        const int h = i / half, e = i % half;
        const float x0 = row[h * a.hd + e], x1 = row[h * a.hd + e + half], c = cs[e], s = sn[e];
        const float p0 = x0 * c, p1 = x1 * s, p2 = x0 * s, p3 = x1 * c;
        const float r0 = p0 - p1, r1 = p2 + p3;
        uint16_t *qo = a.q16 + ((int64_t)t * a.H + h) * a.hd;
        qo[e] = (uint16_t)f2h(r0 * a.q_scale);
        qo[e + half] = (uint16_t)f2h(r1 * a.q_scale);
    }
    const float *kr = row + (int64_t)a.H * a.hd, *vr = kr + kvw;
    for (int i = tid; i < a.Hkv * half; i += 256) {
        const int kh = i / half, e = i % half;
        const float x0 = kr[kh * a.hd + e], x1 = kr[kh * a.hd + e + half], c = cs[e], s = sn[e];
        const float p0 = x0 * c, p1 = x1 * s, p2 = x0 * s, p3 = x1 * c;
        a.kc[(int64_t)p * kvw + kh * a.hd + e] = (uint16_t)f2h(p0 - p1);
        a.kc[(int64_t)p * kvw + kh * a.hd + e + half] = (uint16_t)f2h(p2 + p3);
    }
    for (int d = tid; d < kvw; d += 256) a.vc[(int64_t)d * a.ctx + p] = (uint16_t)f2h(vr[d]);
}

// ---- causal prefill attention on f16 MFMA ---------------------------------------------------------
// A workgroup takes 64 query rows = (query, head) pairs of one kv head: QBQ = 64/G consecutive
// queries x the G heads sharing that kv head, so each K/V block is staged once for all of them.
// Per 64-key block: S = Q K^T (v_mfma_f32_16x16x32_f16, f32 accumulate of exact f16 products).
// ggml's soft_max_ext needs the row max before any e is formed (e = f16(exp(f16(w - max)))), so
// S is formed three times: (1) max, (2) the exact integer sum of e (as the decode kernel), (3)
// P16 = f16(e * (float)(1/sum)) and O += P V.  Only the fp32 order of the S and O sums differs
// from ggml's vec_dot_f16 lane order.
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int AP_HD = 256, AP_QS = AP_HD + 8, AP_KB = 64, AP_VS = AP_KB + 8;

__device__ __forceinline__ float row16_max(float v) {  // max over the 16 lanes of a DPP row
    v = fmaxf(v, dpp_f<0xB1>(v));
    v = fmaxf(v, dpp_f<0x4E>(v));
    v = fmaxf(v, dpp_f<0x141>(v));
    v = fmaxf(v, dpp_f<0x140>(v));
    return v;
}
__device__ __forceinline__ unsigned long long row16_sum(unsigned long long v) {  // exact (integers)
    auto step = [&](auto ctrl) {
        constexpr int C = decltype(ctrl)::value;
        const unsigned long long t = ((unsigned long long)dpp_u<C>((uint32_t)(v >> 32)) << 32) | dpp_u<C>((uint32_t)v);
        v += t;
    };
    step(std::integral_constant<int, 0xB1>());
    step(std::integral_constant<int, 0x4E>());
    step(std::integral_constant<int, 0x141>());
    step(std::integral_constant<int, 0x140>());
    return v;
}

__global__ void __launch_bounds__(256) k_attn_prefill(attnp_args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *Qs = (uint16_t *)smem;           // [64][AP_QS]
    uint16_t *Ks = Qs + 64 * AP_QS;            // [AP_KB][AP_QS]
    uint16_t *Vt = Ks + AP_KB * AP_QS;         // [AP_HD][AP_VS]  (V^T block: dims x keys)
    uint16_t *Ps = Vt + AP_HD * AP_VS;         // [64][AP_VS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kg = lane >> 4;
    const int G = a.H / a.Hkv, QBQ = 64 / G, kvh = blockIdx.y;
    const int tq0 = blockIdx.x * QBQ;
    const int kvw = a.Hkv * AP_HD;
    // stage the 64 query rows (row m -> query tq0 + m / G, head kvh*G + m % G)
    for (int c = tid; c < 64 * (AP_HD / 8); c += 256) {
        const int m = c / (AP_HD / 8), seg = c % (AP_HD / 8);
        int t = tq0 + m / G;
        t = t < a.T ? t : a.T - 1;
        const int h = kvh * G + m % G;
        *(uint4 *)(Qs + m * AP_QS + seg * 8) = *(const uint4 *)(a.q16 + ((int64_t)t * a.H + h) * AP_HD + seg * 8);
    }
    // this wave's rows: 16*wave + kg*4 + v  ->  their sequence positions p0 + t (for the causal mask)
    int tr[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) tr[v] = a.p0 + tq0 + (16 * wave + kg * 4 + v) / G;
    const int t_last = a.p0 + min(tq0 + QBQ - 1, a.T - 1);
    const int n_kb = t_last / AP_KB + 1;  // key blocks reaching the last query (keys j <= t only)
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned long long isum[4] = {0, 0, 0, 0};
    float inv[4];
    v4f o[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) o[n] = (v4f){0.f, 0.f, 0.f, 0.f};

    auto stage_k = [&](int kb) {
        for (int c = tid; c < AP_KB * (AP_HD / 8); c += 256) {
            const int r = c / (AP_HD / 8), seg = c % (AP_HD / 8);
            const int j = kb * AP_KB + r;
            const int jc = j < a.ctx ? j : 0;
            *(uint4 *)(Ks + r * AP_QS + seg * 8) = *(const uint4 *)(a.kc + (int64_t)jc * kvw + kvh * AP_HD + seg * 8);
        }
    };
    auto scores = [&](v4f S[4]) {  // S[c][v]: row 16*wave + kg*4 + v, key kb*64 + c*16 + l16
#pragma unroll
        for (int c = 0; c < 4; ++c) S[c] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < AP_HD / 32; ++ks) {
            const v8h av = *(const v8h *)(Qs + (16 * wave + l16) * AP_QS + ks * 32 + kg * 8);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const v8h bv = *(const v8h *)(Ks + (c * 16 + l16) * AP_QS + ks * 32 + kg * 8);
                S[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, S[c], 0, 0, 0);
            }
        }
    };
    // the mfma output row for (c, v) is 16*wave + kg*4 + v; keys are per lane: kb*64 + c*16 + l16
    for (int pass = 0; pass < 3; ++pass) {
        for (int kb = 0; kb < n_kb; ++kb) {
            __syncthreads();
            stage_k(kb);
            if (pass == 2)
                for (int c = tid; c < AP_HD * (AP_KB / 8); c += 256) {
                    const int d = c / (AP_KB / 8), seg = c % (AP_KB / 8);
                    const int j0 = kb * AP_KB + seg * 8;
                    const int jc = j0 + 8 <= a.ctx ? j0 : 0;
                    *(uint4 *)(Vt + d * AP_VS + seg * 8) =
                        *(const uint4 *)(a.vc + ((int64_t)kvh * AP_HD + d) * a.ctx + jc);
                }
            __syncthreads();
            v4f S[4];
            scores(S);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = kb * AP_KB + c * 16 + l16;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const bool live = j <= tr[v] && j < a.n_kv;  // mask j > pos -> -inf
                    const float w = S[c][v] * 1.0f + 0.0f;
                    if (pass == 0) {
                        if (live) mx[v] = fmaxf(mx[v], w);
                    } else {
                        uint32_t e16 = 0;
                        if (live) e16 = exp_f16_of(f2h(w - mx[v]));
                        if (pass == 1) {
                            isum[v] += (unsigned long long)(uint32_t)(h2f(e16) * 16777216.0f);
                        } else {
                            Ps[(16 * wave + kg * 4 + v) * AP_VS + c * 16 + l16] = (uint16_t)f2h(h2f(e16) * inv[v]);
                        }
                    }
                }
            }
            if (pass == 2) {
                // O[rows][dims] += P[rows][keys] . V[keys][dims]  (Ps rows are this wave's own)
#pragma unroll
                for (int kk = 0; kk < AP_KB / 32; ++kk) {
                    const v8h pv = *(const v8h *)(Ps + (16 * wave + l16) * AP_VS + kk * 32 + kg * 8);
#pragma unroll
                    for (int n = 0; n < 16; ++n) {
                        const v8h vv = *(const v8h *)(Vt + (n * 16 + l16) * AP_VS + kk * 32 + kg * 8);
                        o[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pv, vv, o[n], 0, 0, 0);
                    }
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int v = 0; v < 4; ++v) mx[v] = row16_max(mx[v]);
        } else if (pass == 1) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const unsigned long long tot = row16_sum(isum[v]);
                const double sum = (double)tot * (1.0 / 16777216.0);
                inv[v] = (float)(1.0 / sum);
            }
        }
    }
    // out[t][h*hd + d]: lane holds rows 16*wave + kg*4 + v, dims n*16 + l16
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int m = 16 * wave + kg * 4 + v, t = tq0 + m / G, h = kvh * G + m % G;
        if (t >= a.T) continue;
        float *orow = a.out + (int64_t)t * a.ldo + (int64_t)h * AP_HD;
#pragma unroll
        for (int n = 0; n < 16; ++n) orow[n * 16 + l16] = o[n][v];
    }
}

// argmax over one logits row -> per-workgroup partial keys (ordered float, ~index), reduced by
// k_advance exactly as in the decode step (first max wins, src/gemma_model.cpp:538-543)
// grid (parts, rows): row blockIdx.y of lg (ld floats apart) -> its `parts` partial keys at keys + row * parts
__global__ void __launch_bounds__(256) k_row_argmax(const float *lg, int64_t ld, int64_t n, unsigned long long *keys) {
    const float *row = lg + (int64_t)blockIdx.y * ld;
    keys += (int64_t)blockIdx.y * gridDim.x;
    unsigned long long best = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = argmax_key(row[i], i);
        best = key > best ? key : best;
    }
    __shared__ unsigned long long red[4];
    best = block_max_key(best, red);
    if (threadIdx.x == 0) keys[blockIdx.x] = best;
}

}  // namespace

int launch_quant_rows(int mode, const qrow_args &a, int T, hipStream_t s) {
    if (a.K % 32 || a.ldq % 256 || a.ldq < a.K || a.ldd * 32 < a.ldq) {
        set_error("quant_rows: K must be a multiple of 32, ldq a multiple of 256");
        return -1;
    }
    switch (mode) {
        case QR_F32: hipLaunchKernelGGL(k_quant_rows<QR_F32>, dim3(T), dim3(256), 0, s, a); break;
        case QR_NORM: hipLaunchKernelGGL(k_quant_rows<QR_NORM>, dim3(T), dim3(256), 0, s, a); break;
        case QR_EMBED_NORM: hipLaunchKernelGGL(k_quant_rows<QR_EMBED_NORM>, dim3(T), dim3(256), 0, s, a); break;
        case QR_GELU: {
            // the LDS-table form (the per-row form k_quant_rows<QR_GELU>: T = 2048 exact prefill
            // 78.4 vs 77.5 ms; this kernel 109 -> ~57 us per layer)
            if (allow_full_lds((const void *)k_quant_gelu_lds, LDS_SLOT_GELU_LDS)) return -1;
            hipLaunchKernelGGL(k_quant_gelu_lds, dim3((unsigned)std::min(T, 256)), dim3(QG_THREADS), 65536 * 2, s, a, T);
            break;
        }
        default: set_error("quant_rows: bad mode"); return -1;
    }
    GHIP_CHECK(hipGetLastError());
    return 0;
}

// the run-time (weight type, epilogue) of a GEMM as compile-time constants: f(wt, ep) with
// decltype(wt)::value = T_Q4_0 / T_Q8_0 and decltype(ep)::value = EPI_STORE / EPI_ADD; false (f not
// called) for any other pair
template <class F>
static bool with_gemm_kind(int wtype, int epi, F f) {
    auto with_epi = [&](auto wt) {
        if (epi == EPI_STORE) f(wt, std::integral_constant<int, EPI_STORE>());
        else if (epi == EPI_ADD) f(wt, std::integral_constant<int, EPI_ADD>());
        else return false;
        return true;
    };
    if (wtype == T_Q4_0) return with_epi(std::integral_constant<int, T_Q4_0>());
    if (wtype == T_Q8_0) return with_epi(std::integral_constant<int, T_Q8_0>());
    return false;
}

int launch_gemm_q(int wtype, int epi, const gemm_args &g, hipStream_t s) {
    if (g.ldq % 256 || g.nb * 32 > g.ldq) {
        set_error("gemm_q: activation image must be padded to 256 elements");
        return -1;
    }
    const dim3 grid((unsigned)((g.rows + GM - 1) / GM), (unsigned)((g.T + GN - 1) / GN));
    const bool known = with_gemm_kind(wtype, epi, [&](auto wt, auto ep) {
        hipLaunchKernelGGL((k_gemm_q<decltype(wt)::value, decltype(ep)::value>), grid, dim3(256), 0, s, g);
    });
    if (!known) {
        set_error("gemm_q: unsupported (type, epilogue)");
        return -1;
    }
    GHIP_CHECK(hipGetLastError());
    return 0;
}

// which exact GEMM runs (hpc_set_gemm_x4): 0 the lane-masked W32 form (k_gemm_x), 1 the K = 4
// multi-block form (k_gemm_x4, 32 rows x 64 tokens per workgroup; T = 2048 prefill 70.9 vs 77.6 ms),
// 2 the same with 64 x 32 (72.3 ms), 3 = 1 with the activation staged from the int8 image (the
// default: 68.0 vs 70.8 ms), 4 = 2 staged from the int8 image; same bits every way
static std::atomic<int> g_gemm_x4{3};
void set_gemm_x4(int mode) {
    if (mode < 0 || mode > 4) set_error("hpc_set_gemm_x4: mode " + std::to_string(mode) + " outside 0..4 (the form is unchanged)");
    else g_gemm_x4.store(mode);
}
gemm_form gemm_form_now() {  // the only reader of the mode's numbering
    const int mode = g_gemm_x4.load();
    gemm_form f;
    f.x4 = mode != 0;
    f.rgs = (mode == 2 || mode == 4) ? 4 : 2;
    f.i8 = mode == 3 || mode == 4;
    return f;
}

int launch_gemm_exact(int wtype, int epi, const gemm_form &form, const gemm_args &g, hipStream_t s) {
    if (g.ldq % 256 || g.nb * 32 > g.ldq || g.T <= 0 || g.rows <= 0 || !(form.i8 ? (const void *)g.xq : (const void *)g.xh)) {
        set_error("gemm_exact: needs the activation image of its form (int8 or f16), padded to 256 elements");
        return -1;
    }
    // workgroup tile: k_gemm_x XM x XN, k_gemm_x4 16 * rgs rows x 32 * (4 / rgs) tokens; the row bound
    // below is the form's own grid.y (the 64-row forms take twice the rows of the 32-row ones)
    const int M = form.x4 ? 16 * form.rgs : XM, N = form.x4 ? 32 * (4 / form.rgs) : XN;
    const int64_t gy = (g.rows + M - 1) / M;
    if (gy > 65535) {
        set_error("gemm_exact: too many rows");
        return -1;
    }
    const dim3 grid((unsigned)((g.T + N - 1) / N), (unsigned)gy);
    const bool known = with_gemm_kind(wtype, epi, [&](auto wt, auto ep) {
        constexpr int W = decltype(wt)::value, E = decltype(ep)::value;
        if (!form.x4) hipLaunchKernelGGL((k_gemm_x<W, E>), grid, dim3(XNT), 0, s, g);
        else if (form.rgs == 4 && form.i8) hipLaunchKernelGGL((k_gemm_x4<W, E, 4, 1>), grid, dim3(XNT), 0, s, g);
        else if (form.rgs == 4) hipLaunchKernelGGL((k_gemm_x4<W, E, 4>), grid, dim3(XNT), 0, s, g);
        else if (form.i8) hipLaunchKernelGGL((k_gemm_x4<W, E, 2, 1>), grid, dim3(XNT), 0, s, g);
        else hipLaunchKernelGGL((k_gemm_x4<W, E, 2>), grid, dim3(XNT), 0, s, g);
    });
    if (!known) {
        set_error("gemm_exact: unsupported (type, epilogue)");
        return -1;
    }
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_row_argmax(const float *row, int64_t n, unsigned long long *keys, int parts, hipStream_t s, int rows, int64_t ld) {
    hipLaunchKernelGGL(k_row_argmax, dim3(parts, rows), dim3(256), 0, s, row, ld, n, keys);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_rope_kv_prefill(const ropekv_args &a, int T, hipStream_t s) {
    hipLaunchKernelGGL(k_rope_kv_prefill, dim3(T), dim3(256), 0, s, a);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_attn_prefill(const attnp_args &a, hipStream_t s) {
    const int G = a.H / a.Hkv;
    if (a.hd != AP_HD || a.H % a.Hkv || 64 % G || a.ctx % 8) {
        set_error("attn_prefill: unsupported shape (head_dim 256, 64 % G == 0)");
        return -1;
    }
    const size_t lds = (size_t)(64 * AP_QS + AP_KB * AP_QS + AP_HD * AP_VS + 64 * AP_VS) * 2;
    GHIP_CHECK(hipFuncSetAttribute((const void *)k_attn_prefill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int QBQ = 64 / G;
    hipLaunchKernelGGL(k_attn_prefill, dim3((a.T + QBQ - 1) / QBQ, a.Hkv), dim3(256), lds, s, a);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip

namespace ghip {
// hipFuncAttributeMaxDynamicSharedMemorySize = the CU's 160 KiB, once per (slot, device): the
// attribute only caps a launch's dynamic LDS, so the whole LDS serves every later size; std::call_once
// makes it thread-safe and the per-device flag correct for engines on several GPUs.
int allow_full_lds(const void *fn, int slot) {
    static std::once_flag once[LDS_SLOTS][64];
    static hipError_t err[LDS_SLOTS][64];
    int dev = 0;
    GHIP_CHECK(hipGetDevice(&dev));
    if (slot < 0 || slot >= LDS_SLOTS || dev < 0 || dev >= 64) {
        set_error("allow_full_lds: bad slot or device");
        return -1;
    }
    // the device's opt-in limit (160 KiB on gfx950; a smaller-LDS target keeps launching what fits
    // instead of failing on an attribute it cannot grant — ADVICE r5)
    std::call_once(once[slot][dev], [&] {
        int optin = 0;
        err[slot][dev] = hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev);
        if (err[slot][dev] == hipSuccess && optin > 64 * 1024)
            err[slot][dev] = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, optin);
    });
    GHIP_CHECK(err[slot][dev]);
    return 0;
}
}  // namespace ghip
