// attn_decode_win.hip — the decode step's position-split attention with the softmax image P16 held in
// windows (DESIGN.md §5 "Windowed decode attention"): k_attn_decode's launch, grid, hand-off and arithmetic
// (ops.hip), with phase B redesigned so that its LDS no longer grows with n_ctx.  k_attn_decode keeps
// P16 [G][ctx] resident (128 KiB at G 8, n_ctx 8192: over the 160 KiB of a workgroup with the staging
// images on top); here LDS holds two windows of ATT_PW positions:
//   B1) statistics, nothing stored: all 16 waves split the n_kv x G scores (thread -> head tid % G,
//       positions tid / G + k * 1024 / G: coalesced sc1 loads, 8 in flight per lane).  Each head's max
//       (an order-preserving key, LDS max) and the integer sum of its fp16 e values in units of 2^-24
//       (u64, LDS add) are exact in any order, so the split changes no bit; every thread then holds the
//       mx and inv = (float)(1 / sum) of its own head in registers.
//   B2) per window: the 1,024 threads re-read the window's scores and store P16 = f16(f32(e) * inv),
//       e = fp16 exp(f16(w - mx)), -inf -> 0: the two roundings of the resident form.  The KQV quads
//       (dim, head) consume the window, their eight accumulators carried across windows: every output
//       is still one vec_dot_f16 over n_kv in ggml's step order.  The windows are double-buffered: the
//       score loads of window k + 1 are issued in front of the dot of window k and turned into P16
//       behind it, one barrier per window.  V comes four 32-position steps per round trip.
// LDS at G 8, head_dim 256: q16 4 KiB + k16 0.5 KiB + Ks 16 KiB + Vs 16 KiB + Pw 2 x 8 x (1024 + 8) x 2 B
// = 32.25 KiB + 96 B of reduction words = 70,496 B (68.8 KiB) at any n_ctx.  Co-residency is
// k_attn_decode's: nwg * Hkv <= ATT_MAXWG workgroups of 1,024 threads, one per CU suffices.
#include "attn_impl.h"

namespace ghip {
namespace {

#define ATT_STAMP(i)                                                                                        \
    do {                                                                                                    \
        if (GHIP_STAMPS && a.dbg_t && tid == 0) a.dbg_t[(int64_t)(kvh * a.nwg + wg) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)

constexpr int ADW_NF = 8;  // scores a lane holds in flight (one round trip per ADW_NF)

// element i (0 .. 7) of the 8 halfs of v replaced by h: selects only, no indexed register
__device__ __forceinline__ uint4 put_half(uint4 v, int i, uint32_t h) {
    const uint32_t sh = 16 * (i & 1), m = ~(0xFFFFu << sh), hv = h << sh;
    const int w = i >> 1;
    v.x = w == 0 ? (v.x & m) | hv : v.x;
    v.y = w == 1 ? (v.y & m) | hv : v.y;
    v.z = w == 2 ? (v.z & m) | hv : v.z;
    v.w = w == 3 ? (v.w & m) | hv : v.w;
    return v;
}

// the reductions over lanes of one head: lanes l, l ^ G, l ^ 2G, ... (G a power of two)
__device__ __forceinline__ float head_max(float v, int G) {
    for (int s = G; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ unsigned long long head_sum_u64(unsigned long long v, int G) {
    for (int s = G; s < 64; s <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ void __launch_bounds__(ATT_THREADS) k_attn_decode_win(attn_args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int hd = a.hd, half = hd / 2, tid = threadIdx.x, t4 = tid & 3, quad = tid >> 2;
    const int lane = tid & 63, wave = tid >> 6;
    // (placement, numbering and phase A: k_attn_decode's, ops.hip)
    const int G = a.H / a.Hkv, nwg = a.nwg;
    const int slot = blockIdx.x >> 3, kvh = (slot / nwg) * 8 + (int)(blockIdx.x & 7), wg = slot % nwg;
    if (kvh >= a.Hkv) return;
    const attn_split sp = attn_split_of(G, hd);
    const int PS = sp.ps, DS = sp.ds;
    const int nb = (hd + DS - 1) / DS;  // workgroups with KQV work
    const int kvw = a.Hkv * hd;
    ATT_STAMP(0);
    // ---- early loads (issue order = wait order): RoPE inputs, then the K and V rows to stage
    const float *qg = a.qkv + (int64_t)kvh * G * hd;
    const float *kh = a.qkv + (int64_t)a.H * hd + (int64_t)kvh * hd;
    const float *vh = a.qkv + (int64_t)a.H * hd + kvw + (int64_t)kvh * hd;
    const float *cs = a.rope_cur, *sn = a.rope_cur + half;  // row of *pos (k_advance keeps it)
    const int npair = G * half, nq4 = npair / 4;
    float4 qa[2] = {}, qb[2] = {}, ca[2] = {}, sa[2] = {};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i4 = tid + r * ATT_THREADS;
        if (i4 - lane < nq4) {
            const int i = (i4 < nq4 ? i4 : 0) * 4;
            const int h = i / half, e = i % half;
            qa[r] = *(const float4 *)(qg + h * hd + e);
            qb[r] = *(const float4 *)(qg + h * hd + e + half);
            ca[r] = *(const float4 *)(cs + e);
            sa[r] = *(const float4 *)(sn + e);
        }
    }
    const int kq4 = half / 4;  // k: 4 pairs per thread for tid < half/4
    const int ik = (tid < kq4 ? tid : 0) * 4;
    float4 ka{}, kb{}, kc4{}, ks4{};
    if (wave * 64 < kq4) {
        ka = *(const float4 *)(kh + ik); kb = *(const float4 *)(kh + ik + half);
        kc4 = *(const float4 *)(cs + ik); ks4 = *(const float4 *)(sn + ik);
    }
    // phase A, first position block of this workgroup: its PS K rows, one coalesced uint4 each
    const int kcw = hd / 8;  // uint4 per K row
    uint4 kst[ATT_STG];
#pragma unroll
    for (int r = 0; r < ATT_STG; ++r) {
        const int idx = tid + r * ATT_THREADS;
        const int row = idx / kcw, c = idx % kcw;
        int j = wg * PS + row;
        j = (idx < PS * kcw && j < a.ctx) ? j : 0;  // rows >= pos are masked; no dependency on pos
        kst[r] = *(const uint4 *)(a.kc + (int64_t)j * kvw + (int64_t)kvh * hd + c * 8);
    }
    // phase B: V rows d of [wg*DS, +DS), positions [0, ATT_VW), one coalesced uint4 each
    constexpr int vcw = ATT_VW / 8;
    uint4 vst[ATT_STG];
    float vsx[ATT_STG];
#pragma unroll
    for (int r = 0; r < ATT_STG; ++r) {
        const int idx = tid + r * ATT_THREADS;
        const int dd = idx / vcw, c = idx % vcw;
        int d = wg * DS + dd;
        d = (idx < DS * vcw && d < hd && wg < nb) ? d : 0;
        vst[r] = *(const uint4 *)(a.vc + ((int64_t)kvh * hd + d) * a.ctx + (c * 8 < a.ctx ? c * 8 : 0));
        vsx[r] = vh[d];  // this token's v of the row (patched into the staged copy)
    }
    const int pa = quad / G < PS ? quad / G : 0, ha = quad % G;
    const bool has_a = quad / G < PS;
    const int db = wg * DS + quad / G, hb = quad % G;
    const bool has_b = wg < nb && quad / G < DS && db < hd;
    const uint16_t *vrow = a.vc + ((int64_t)kvh * hd + (has_b ? db : 0)) * a.ctx;
    const float vx = has_b ? vh[db] : 0.0f;
    ATT_STAMP(6);
    // pos is published with the RoPE row (k_advance / begin): no dependent load
    const int pos = __builtin_amdgcn_readfirstlane(((const int *)a.rope_cur)[hd]);
    const int n_total = pos + 1;
    int n_kv = 32 * (n_total / 32 + 1);  // src/gemma_model.cpp:429
    if (n_kv > a.ctx) n_kv = a.ctx;
    ATT_STAMP(7);

    // LDS: q16 [G][hd], k16 [hd], Ks [PS][hd], Vs [DS][ATT_VW], Pw [2][G][ATT_PWS], e_sum [G], mx_key [G]
    uint16_t *q16 = (uint16_t *)smem;
    uint16_t *k16 = q16 + (size_t)G * hd;
    uint16_t *Ks = k16 + hd;
    uint16_t *Vs = Ks + (size_t)PS * hd;
    uint16_t *Pw = Vs + (size_t)DS * ATT_VW;
    unsigned long long *e_sum = (unsigned long long *)(Pw + (size_t)2 * G * ATT_PWS);
    uint32_t *mx_key = (uint32_t *)(e_sum + G);
    for (int h = tid; h < G; h += ATT_THREADS) {
        mx_key[h] = 0u;  // below the key of every float, -inf included
        e_sum[h] = 0ull;
    }

    // RoPE NEOX on q (then * q_scale) and on k; f32 -> f16 (ggml_cpy / MUL_MAT INIT conversions)
    auto rope4 = [&](float4 x0v, float4 x1v, float4 cv, float4 sv, float scale, bool scaled, uint16_t *lo,
                     uint16_t *hi) {
        const float x0s[4] = {x0v.x, x0v.y, x0v.z, x0v.w}, x1s[4] = {x1v.x, x1v.y, x1v.z, x1v.w};
        const float cs4[4] = {cv.x, cv.y, cv.z, cv.w}, sn4[4] = {sv.x, sv.y, sv.z, sv.w};
        uint32_t l2[2] = {0, 0}, h2[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x0 = x0s[k], x1 = x1s[k], c = cs4[k], s = sn4[k];
            const float p0 = x0 * c, p1 = x1 * s, p2 = x0 * s, p3 = x1 * c;
            const float r0 = p0 - p1, r1 = p2 + p3;
            const uint32_t a0 = scaled ? f2h(r0 * scale) : f2h(r0), a1 = scaled ? f2h(r1 * scale) : f2h(r1);
            l2[k >> 1] |= a0 << (16 * (k & 1));
            h2[k >> 1] |= a1 << (16 * (k & 1));
        }
        *(uint2 *)lo = make_uint2(l2[0], l2[1]);
        *(uint2 *)hi = make_uint2(h2[0], h2[1]);
    };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i4 = tid + r * ATT_THREADS;
        if (i4 < nq4) {
            const int i = i4 * 4, h = i / half, e = i % half;
            rope4(qa[r], qb[r], ca[r], sa[r], a.q_scale, true, q16 + h * hd + e, q16 + h * hd + e + half);
        }
    }
    for (int i4 = tid + 2 * ATT_THREADS; i4 < nq4; i4 += ATT_THREADS) {  // G * hd > 4096 (rare)
        const int i = i4 * 4, h = i / half, e = i % half;
        rope4(*(const float4 *)(qg + h * hd + e), *(const float4 *)(qg + h * hd + e + half), *(const float4 *)(cs + e),
              *(const float4 *)(sn + e), a.q_scale, true, q16 + h * hd + e, q16 + h * hd + e + half);
    }
    if (tid < kq4) rope4(ka, kb, kc4, ks4, 1.0f, false, k16 + ik, k16 + ik + half);
    // stage K and V rows (V patched at `pos`: this token's cache write is not visible in-launch)
    // (one call per staging register: an `r` loop here is not unrolled by the compiler, which then keeps kst in scratch)
    static_assert(ATT_STG == 2, "two staging registers");
    auto stage = [&](int r, uint4 kx, uint4 v, float vx_r) {
        const int idx = tid + r * ATT_THREADS;
        if (idx < PS * kcw) *(uint4 *)(Ks + (size_t)idx * 8) = kx;
        if (idx < DS * vcw) {
            const int c = idx % vcw;
            if (pos >= c * 8 && pos < c * 8 + 8) v = put_half(v, pos - c * 8, f2h(vx_r));
            *(uint4 *)(Vs + (size_t)idx * 8) = v;
        }
    };
    stage(0, kst[0], vst[0], vsx[0]);
    stage(1, kst[1], vst[1], vsx[1]);
    __syncthreads();
    ATT_STAMP(1);
    // this token's cache entries (src/gemma_model.cpp:506-517): K row by workgroup 0, V column
    // `pos` by the KQV workgroup owning each dimension
    if (wg == 0)
        for (int i = tid; i < hd; i += ATT_THREADS) a.kc[(int64_t)pos * kvw + (int64_t)kvh * hd + i] = k16[i];
    if (has_b && hb == 0 && t4 == 0) a.vc[((int64_t)kvh * hd + db) * a.ctx + pos] = f2h(vx);

    // ---- phase A: KQ (vec_dot_f16 over hd per kv position) + mask (j > pos -> -inf), scale 1.0
    float *sk_out = a.sbuf + (int64_t)kvh * a.ctx * G;  // [ctx][G]
    for (int blk = wg, pass = 0; blk * PS < n_kv; blk += nwg, ++pass) {
        const int j = blk * PS + pa;
        float acc[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) acc[y] = 0.0f;
        const uint16_t *qh16 = q16 + (size_t)ha * hd + t4 * 8;
        if (pass == 0) {  // staged rows (LDS); row `pos` from this token's k16
            const uint16_t *krow = ((j == pos) ? k16 : Ks + (size_t)pa * hd) + t4 * 8;
            for (int s = 0; s * 32 < hd; ++s)
                f16_step8(acc, *(const uint4 *)(krow + s * 32), *(const uint4 *)(qh16 + s * 32));
        } else {
            const int jc = j < pos ? j : pos;
            if (jc == pos) {
                for (int s = 0; s * 32 < hd; ++s)
                    f16_step8(acc, *(const uint4 *)(k16 + s * 32 + t4 * 8), *(const uint4 *)(qh16 + s * 32));
            } else {
                const uint16_t *krow = a.kc + (int64_t)jc * kvw + (int64_t)kvh * hd + t4 * 8;
                for (int s = 0; s * 32 < hd; ++s)
                    f16_step8(acc, *(const uint4 *)(krow + s * 32), *(const uint4 *)(qh16 + s * 32));
            }
        }
        const float kq = quad_reduce_f16(acc);
        if (t4 == 0 && has_a && j < n_kv) {
            const float w = (j > pos) ? -INFINITY : kq * 1.0f + 0.0f;
            st_sc1(sk_out + (int64_t)j * G + ha, w);
            if (a.dbg_w) a.dbg_w[(int64_t)(kvh * G + ha) * a.ctx + j] = w;
        }
    }
    // publish: every storing wave drains its stores, then one lane arrives
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ATT_STAMP(2);
    int *cnt = a.sync + kvh * 2;
    if (tid == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wg >= nb) return;  // no KQV work for this workgroup

    // ---- hand-off: wait for all nwg workgroups of this kv head (bounded spin)
    if (tid == 0) {
        int spins = 0;
        while (ld_sc1_i(cnt) < nwg) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1 << 26)) {  // never on a healthy device: flag and fall through
                if (a.err) *a.err = 1;
                break;
            }
        }
    }
    __syncthreads();
    ATT_STAMP(3);

    // ---- B1: soft_max_ext's statistics per head, all waves.  Thread -> head hs, positions
    // j0 + k * JS: a wave's load covers 64 / G whole rows of sbuf [ctx][G]
    const int hs = tid & (G - 1), JS = ATT_THREADS / G, j0 = tid / G;
    const float *sk_h = sk_out + hs;
    auto load_nf = [&](int jb, int jend, float(&w)[ADW_NF]) {  // scores hs of jb + k * JS (below jend, else -inf)
#pragma unroll
        for (int k = 0; k < ADW_NF; ++k) {
            const int j = jb + k * JS;
            w[k] = j < jend ? ld_sc1(sk_h + (int64_t)j * G) : -INFINITY;
        }
    };
    float s0[ADW_NF];  // the thread's first ADW_NF scores stay in registers for the second pass
    load_nf(j0, n_kv, s0);
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < ADW_NF; ++k) mx = fmaxf(mx, s0[k]);
    for (int jb = j0 + ADW_NF * JS; jb < n_kv; jb += ADW_NF * JS) {
        float w[ADW_NF];
        load_nf(jb, n_kv, w);
#pragma unroll
        for (int k = 0; k < ADW_NF; ++k) mx = fmaxf(mx, w[k]);
    }
    mx = head_max(mx, G);
    if (lane < G) {
        const uint32_t b = __builtin_bit_cast(uint32_t, mx);
        atomicMax(mx_key + hs, (b & 0x80000000u) ? ~b : (b | 0x80000000u));
    }
    __syncthreads();
    {
        const uint32_t key = mx_key[hs];
        mx = __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
    }
    // e = f16(exp(f16(w - mx))), 0 for -inf: fp16 in [0, 1], exact multiples of 2^-24, so the integer
    // sum is the exact sum in any order (ggml's double accumulation of them is exact too)
    auto e_of = [&](float w) -> uint32_t { return w != -INFINITY ? exp_f16_of(f2h(w - mx)) : 0u; };
    unsigned long long isum = 0;
#pragma unroll
    for (int k = 0; k < ADW_NF; ++k) isum += (unsigned long long)(uint32_t)(h2f(e_of(s0[k])) * 16777216.0f);
    for (int jb = j0 + ADW_NF * JS; jb < n_kv; jb += ADW_NF * JS) {
        float w[ADW_NF];
        load_nf(jb, n_kv, w);
#pragma unroll
        for (int k = 0; k < ADW_NF; ++k) isum += (unsigned long long)(uint32_t)(h2f(e_of(w[k])) * 16777216.0f);
    }
    isum = head_sum_u64(isum, G);
    if (lane < G && isum) atomicAdd(e_sum + hs, isum);
    __syncthreads();
    const double sum = (double)e_sum[hs] * (1.0 / 16777216.0);
    const float inv = (float)(1.0 / sum);
    if (a.dbg_inv && wg == 0 && tid < G) a.dbg_inv[kvh * G + hs] = inv;
    ATT_STAMP(4);
    // hand-off bookkeeping: the last KQV workgroup to get here resets the counters for the next
    // launch (every other workgroup of this kv head has already passed its poll)
    if (tid == 0) {
        const int done = __hip_atomic_fetch_add(cnt + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done == nb - 1) {
            __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(cnt + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- B2: P16 in windows of ATT_PW positions, and KQV: out[h][d] = vec_dot_f16(n_kv, V[kvh][d], P16[h])
    // the fill: thread -> (head hs, window positions j0 + k * JS); rows of ATT_PWS halfs (16 B of pad: the G
    // rows a wave stores to, and the quads of a wave read from, start in different banks)
    uint16_t *dbg_p = a.dbg_p && wg == 0 ? a.dbg_p + (int64_t)(kvh * G + hs) * a.ctx : nullptr;
    auto fill_put = [&](int w0, int jl0, const float(&w)[ADW_NF], uint16_t *buf) {
#pragma unroll
        for (int k = 0; k < ADW_NF; ++k) {
            const int jl = jl0 + k * JS;
            if (jl < ATT_PW && w0 + jl < n_kv) {
                const uint16_t p = (uint16_t)f2h(h2f(e_of(w[k])) * inv);
                buf[(size_t)hs * ATT_PWS + jl] = p;
                if (dbg_p) dbg_p[w0 + jl] = p;
            }
        }
    };
    // window w0's scores past the first ADW_NF per thread (G > 8)
    auto fill_rest = [&](int w0, uint16_t *buf) {
        const int wend = w0 + ATT_PW < n_kv ? w0 + ATT_PW : n_kv;
        for (int jl0 = j0 + ADW_NF * JS; jl0 < ATT_PW; jl0 += ADW_NF * JS) {
            float w[ADW_NF];
            load_nf(w0 + jl0, wend, w);
            fill_put(w0, jl0, w, buf);
        }
    };
    float acc[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) acc[y] = 0.0f;
    const uint16_t *vs = Vs + (size_t)(has_b ? db - wg * DS : 0) * ATT_VW;
    const uint32_t vx16 = f2h(vx);
    // one 32-position step's V operand: staged (patched at `pos` already) below ATT_VW, else the cache
    auto dot = [&](int w0, const uint16_t *buf) {
        const int wend = w0 + ATT_PW < n_kv ? w0 + ATT_PW : n_kv;
        const uint16_t *prow = buf + (size_t)hb * ATT_PWS + t4 * 8;
        int st = w0;
        for (; st + 128 <= wend; st += 128) {  // four steps' V loads issued together (one round trip)
            const int e0 = st + t4 * 8;
            uint4 xv[4];
            if (st < ATT_VW) {
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[k] = *(const uint4 *)(vs + e0 + 32 * k);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[k] = *(const uint4 *)(vrow + e0 + 32 * k);
                if (pos >= st && pos < st + 128) {  // this token's V: its cache write may not be visible
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = pos - e0 - 32 * k;
                        if (i >= 0 && i < 8) xv[k] = put_half(xv[k], i, vx16);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) f16_step8(acc, xv[k], *(const uint4 *)(prow + (st - w0) + 32 * k));
        }
        for (; st < wend; st += 32) {
            const int e0 = st + t4 * 8, i = pos - e0;
            uint4 xv;
            if (st < ATT_VW) {
                xv = *(const uint4 *)(vs + e0);
            } else {
                xv = *(const uint4 *)(vrow + e0);
                if (i >= 0 && i < 8) xv = put_half(xv, i, vx16);
            }
            f16_step8(acc, xv, *(const uint4 *)(prow + (st - w0)));
        }
    };
    {
        float w[ADW_NF];
        load_nf(j0, n_kv < ATT_PW ? n_kv : ATT_PW, w);
        fill_put(0, j0, w, Pw);
        fill_rest(0, Pw);
    }
    __syncthreads();
    for (int w0 = 0, k = 0; w0 < n_kv; w0 += ATT_PW, k ^= 1) {
        uint16_t *cur = Pw + (size_t)k * G * ATT_PWS, *nxt = Pw + (size_t)(k ^ 1) * G * ATT_PWS;
        const int w1 = w0 + ATT_PW;
        const bool more = w1 < n_kv;
        float w[ADW_NF];
        if (more) load_nf(w1 + j0, w1 + ATT_PW < n_kv ? w1 + ATT_PW : n_kv, w);  // in flight under the dot
        if (has_b) dot(w0, cur);
        if (more) {
            fill_put(w1, j0, w, nxt);
            fill_rest(w1, nxt);
            __syncthreads();  // window k + 1 is filled and window k consumed
        }
    }
    const float o = quad_reduce_f16(acc);
    if (has_b && t4 == 0) {
        a.out[(int64_t)(kvh * G + hb) * hd + db] = o;
        if (a.out_act) ((float *)smem)[hb * DS + (db - wg * DS)] = o;  // q16 is dead after KQ
    }
    if (a.out_act) {
        // this slice's Q8_0 blocks of each head's output (DS == 32, aligned: one block per head)
        __syncthreads();
        if (tid < G * 4) {
            const int h = tid >> 2, q = tid & 3;
            const float *op = (const float *)smem + h * DS + q * 8;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = op[j];
            image_put_quad(a.out_act, nullptr, a.out_da, (int64_t)(kvh * G + h) * (hd / 32) + wg, q, v);
        }
    }
    ATT_STAMP(5);
}

}  // namespace

// g: attn_geometry of a's shape; launch_attn_decode (ops.hip) has checked the shape, the scratch and g.lds_win
int launch_attn_decode_win(const attn_args &a, const attn_geom &g, hipStream_t s) {
    if (g.lds_win > 64 * 1024)
        GHIP_CHECK(hipFuncSetAttribute((const void *)k_attn_decode_win, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_win));
    hipLaunchKernelGGL(k_attn_decode_win, dim3(g.grid), dim3(ATT_THREADS), g.lds_win, s, a);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
