// kquant_impl.h — the K-quant dot shared by kquant.hip and gemm_skinny_kq.hip: a super-block's weight
// bytes for one AVX2 lane (kq_raw / kq_load), its exact terms against a Q8_K block (kq_terms), and the
// fold + epilogue + store of a (row, column) chain (kq_store).  kquant.hip's header has the numerics.
#pragma once
#include "device_util.h"
#include "kernels.h"

namespace ghip {
namespace {

__device__ __forceinline__ int sdot4k(uint32_t a, uint32_t b) { return __builtin_amdgcn_sdot4((int)a, (int)b, 0, false); }

// a dword at a 2-byte aligned address (Q6_K blocks are 210 B: odd blocks start 2 mod 4)
__device__ __forceinline__ uint32_t ld_u32_a2(const uint8_t *p) {
    const uint16_t *h = (const uint16_t *)p;
    return (uint32_t)h[0] | ((uint32_t)h[1] << 16);
}

// one super-block s of row `wrow` for AVX2 lane l: the lane's exact int32 sum and the fp32 scale
// d = y.d*f16(x.d); Q4_K also the mins lane k = l & 3 (meaningful in lanes 0..3): prod and dmin
struct kq_term { int sumi; float d; int prod; float dmin; };

// a super-block's weight bytes for AVX2 lane l, loaded ahead of the arithmetic (kq_terms)
template <int WT> struct kq_raw;
template <> struct kq_raw<T_Q4_K> { uint4 h; uint32_t q[4]; };
template <> struct kq_raw<T_Q6_K> { uint32_t qla[2], qlb[2], qh[2], sc[4]; uint32_t d; };

// Lane-contiguous device layout of K-quant rows (launch_kq_retile; the engine's weights, `TL`):
// row-major rows, row_bytes unchanged, only the bytes inside a row move so that each AVX2 lane's
// operands are one contiguous, aligned vector:
//   Q4_K, per super-block (144 B): header [d, dmin, scales] (16 B) unchanged; quant dword j of lane
//     l (ggml byte 16 + 32j + 4l) -> 16 + 16l + 4j: one 16-B load per lane instead of four.
//   Q6_K, per group of 8 super-blocks (1680 B, 16-aligned): [8 x ql 128 B][8 x qh 64 B]
//     [8 x scales 16 B][8 x d 2 B]; within super-block i: ql dword k of lane l (ggml byte 32k + 4l)
//     -> 128i + 16l + 4k, qh dword j (ggml byte 128 + 32j + 4l) -> 1024 + 64i + 8l + 4j; scales
//     -> 1536 + 16i, d -> 1664 + 2i: four loads per lane instead of ~21 two-byte-aligned ones.
// Same bytes, same arithmetic: the dots are unchanged.
// Non-temporal lane-contiguous weight loads (GHIP_KQ_NT bits: 1 Q4_K, 2 Q6_K, 4 the lane-own quant bytes only; as the Q4_0 matvecs load theirs):
// measured slower, Q4_K_M decode 1,059-1,064 (plain) vs 1,036-1,037 (Q4_K nt) / 1,019-1,028 (Q6_K nt)
// tok/s, 1,028-1,034 (lane-own quant bytes nt, headers plain) (same box, interleaved) — off
#ifndef GHIP_KQ_NT
#define GHIP_KQ_NT 0
#endif
typedef uint32_t kq_v4u __attribute__((ext_vector_type(4)));
typedef uint32_t kq_v2u __attribute__((ext_vector_type(2)));
template <int WT, bool LANE = false>  // LANE: each lane its own bytes (not a wave-shared header)
__device__ __forceinline__ uint4 kq_ld16(const uint8_t *p) {
    if constexpr ((GHIP_KQ_NT & (WT == T_Q4_K ? 1 : 2)) || (LANE && (GHIP_KQ_NT & 4))) {
        const kq_v4u v = __builtin_nontemporal_load((const kq_v4u *)p);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *(const uint4 *)p;
}
template <int WT, bool LANE = false>
__device__ __forceinline__ uint2 kq_ld8(const uint8_t *p) {
    if constexpr ((GHIP_KQ_NT & (WT == T_Q4_K ? 1 : 2)) || (LANE && (GHIP_KQ_NT & 4))) {
        const kq_v2u v = __builtin_nontemporal_load((const kq_v2u *)p);
        return make_uint2(v.x, v.y);
    }
    return *(const uint2 *)p;
}
template <int WT, bool TL = false>
__device__ __forceinline__ kq_raw<WT> kq_load(const uint8_t *wrow, int s, int l) {
    kq_raw<WT> r;
    if constexpr (TL && WT == T_Q4_K) {
        const uint8_t *blk = wrow + (int64_t)s * 144;
        r.h = kq_ld16<WT>(blk);
        const uint4 q = kq_ld16<WT, true>(blk + 16 + 16 * l);
        r.q[0] = q.x; r.q[1] = q.y; r.q[2] = q.z; r.q[3] = q.w;
        return r;
    }
    if constexpr (TL && WT == T_Q6_K) {
        const uint8_t *g = wrow + (int64_t)(s >> 3) * 1680;
        const int i = s & 7;
        const uint4 ql = kq_ld16<WT, true>(g + 128 * i + 16 * l);
        const uint2 qh = kq_ld8<WT, true>(g + 1024 + 64 * i + 8 * l);
        const uint4 sc = kq_ld16<WT>(g + 1536 + 16 * i);
        r.qla[0] = ql.x; r.qlb[0] = ql.y; r.qla[1] = ql.z; r.qlb[1] = ql.w;
        r.qh[0] = qh.x; r.qh[1] = qh.y;
        r.sc[0] = sc.x; r.sc[1] = sc.y; r.sc[2] = sc.z; r.sc[3] = sc.w;
        r.d = *(const uint16_t *)(g + 1664 + 2 * i);
        return r;
    }
    if constexpr (WT == T_Q4_K) {
        const uint8_t *blk = wrow + (int64_t)s * 144;
        r.h = *(const uint4 *)blk;  // d, dmin, scales[12]
#pragma unroll
        for (int j = 0; j < 4; ++j) r.q[j] = *(const uint32_t *)(blk + 16 + 32 * j + 4 * l);
    } else {
        const uint8_t *blk = wrow + (int64_t)s * 210;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            r.qla[j] = ld_u32_a2(blk + 64 * j + 4 * l);
            r.qlb[j] = ld_u32_a2(blk + 64 * j + 32 + 4 * l);
            r.qh[j] = ld_u32_a2(blk + 128 + 32 * j + 4 * l);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) r.sc[k] = ld_u32_a2(blk + 192 + 4 * k);
        r.d = *(const uint16_t *)(blk + 208);
    }
    return r;
}

template <int WT>
__device__ __forceinline__ kq_term kq_terms(const kq_raw<WT> &r, const uint8_t *xs, int s, int l) {
    kq_term t;
    const uint8_t *xb = xs + s * 292;
    const float yd = *(const float *)xb;
    const int8_t *q8 = (const int8_t *)(xb + 4);
    if constexpr (WT == T_Q4_K) {
        // six-bit scales / mins (src/kernals.cl:79-84)
        const uint32_t u0 = r.h.y, u1 = r.h.z, u2 = r.h.w;
        const uint32_t s03 = u0 & 0x3f3f3f3fu;                                      // sc 0..3
        const uint32_t s47 = (u2 & 0x0f0f0f0fu) | (((u0 >> 6) & 0x03030303u) << 4);  // sc 4..7
        const uint32_t m03 = u1 & 0x3f3f3f3fu;                                      // mins 0..3
        const uint32_t m47 = ((u2 >> 4) & 0x0f0f0f0fu) | (((u1 >> 6) & 0x03030303u) << 4);
        int sumi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t scw = j < 2 ? s03 : s47;
            const int sc_lo = (scw >> (16 * (j & 1))) & 0xFF, sc_hi = (scw >> (16 * (j & 1) + 8)) & 0xFF;
            const uint32_t alo = *(const uint32_t *)(q8 + 64 * j + 4 * l);
            const uint32_t ahi = *(const uint32_t *)(q8 + 64 * j + 32 + 4 * l);
            sumi += sc_lo * sdot4k(r.q[j] & 0x0F0F0F0Fu, alo) + sc_hi * sdot4k((r.q[j] >> 4) & 0x0F0F0F0Fu, ahi);
        }
        t.sumi = sumi;
        t.d = yd * pin(h2f(r.h.x));
        t.dmin = -yd * pin(h2f(r.h.x >> 16));
        const int16_t *bs = (const int16_t *)(xb + 260);
        const int k = l & 3;
        const int S0 = (int)bs[4 * k] + (int)bs[4 * k + 1], S1 = (int)bs[4 * k + 2] + (int)bs[4 * k + 3];
        const uint32_t mw = k < 2 ? m03 : m47;
        const int mn0 = (mw >> (16 * (k & 1))) & 0xFF, mn1 = (mw >> (16 * (k & 1) + 8)) & 0xFF;
        t.prod = mn0 * S0 + mn1 * S1;
    } else {
        int sumi = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t qla = r.qla[j], qlb = r.qlb[j], qh = r.qh[j];
            const uint32_t q6[4] = {(qla & 0x0F0F0F0Fu) | ((qh & 0x03030303u) << 4),
                                    (qlb & 0x0F0F0F0Fu) | (((qh >> 2) & 0x03030303u) << 4),
                                    ((qla >> 4) & 0x0F0F0F0Fu) | (((qh >> 4) & 0x03030303u) << 4),
                                    ((qlb >> 4) & 0x0F0F0F0Fu) | (((qh >> 6) & 0x03030303u) << 4)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t av = *(const uint32_t *)(q8 + 128 * j + 32 * i + 4 * l);
                const int p = sdot4k(q6[i], av) - sdot4k(0x20202020u, av);
                const int bi = 8 * j + 2 * i + (l >> 2);  // scale byte 192 + bi
                const int sc = (int)(int8_t)(uint8_t)(r.sc[bi >> 2] >> (8 * (bi & 3)));
                sumi += sc * p;
            }
        }
        t.sumi = sumi;
        t.d = yd * pin(h2f(r.d));
        t.prod = 0;
        t.dmin = 0.0f;
    }
    return t;
}

// KQ_PF super-blocks' weight loads are issued before any of their arithmetic (one memory round trip
// per group instead of one per super-block)
#ifndef GHIP_KQ_PF
#define GHIP_KQ_PF 2  // Q4_K_M decode, same box: 1 / 2 / 3 / 4 / 8 -> 1.170 / 1.132 / 1.140 / 1.155 / 1.315 ms/token
#endif
constexpr int KQ_PF = GHIP_KQ_PF;

// write-through (sc1) global accesses for the in-launch hand-off (MI355X_MICROARCH sc1 table row 1,
// the pattern attn_impl.h documents): values read back inside the launch are stored and loaded sc1
typedef __attribute__((address_space(1))) float kq_gfloat;
typedef __attribute__((address_space(1))) unsigned kq_guint;
__device__ __forceinline__ void kq_st_sc1(float *p, float v) {
    __hip_atomic_store((kq_gfloat *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void kq_put(const kq_args &a, int64_t o, float v) {
    if (a.q8_mode != KQO_NONE && !(a.q8_abl & 4)) kq_st_sc1(a.y + o, v);
    else a.y[o] = v;
}

// fold the 8 lanes (and the 4 mins lanes) of each row; lane 0 of the 8-group stores
template <int WT>
__device__ __forceinline__ void kq_store(const kq_args &a, int col, int64_t row_raw, int l, float acc, float accm) {
    float v = fold8_dpp(acc);  // ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)) in lane 0 of the 8-group
    if (WT == T_Q4_K) v = v + quad_fold_dpp(accm);  // (m0+m2)+(m1+m3) in lane 0
    if (l == 0 && row_raw < a.rows) {
        const int64_t o = (int64_t)col * a.y_col_stride + row_raw;
        if (a.gate_in) {  // gelu(gate) then ggml_mul by up (src/gemma_model.cpp:444-452)
            const float g = a.gate_in[o];
            const float gl = (a.gelu_clamp && g <= -10.0f) ? 0.0f : (a.gelu_clamp && g >= 10.0f) ? g : h2f(a.gelu_tab[f2h(g)]);
            v = gl * v;
        } else if (a.resid) {
            v = v + a.resid[o];
        }
        kq_put(a, o, v);
    }
}

}  // namespace
}  // namespace ghip
