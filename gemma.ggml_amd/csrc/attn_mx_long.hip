// attn_mx_long.hip — the exact causal prefill attention on the f32 matrix cores with no LDS bound on the key
// count: k_attn_mx's arithmetic (attn_mx.hip) for passes whose 16 score rows do not fit the LDS (n_kv > 2556),
// up to n_ctx 8192.  Every KQ and KQV output is one vec_dot_f16 — 32 fmaf chains, four steps of a chain per
// v_mfma_f32_16x16x4_f32, folded by fold32 — and the softmax is soft_max_ext's (mask j > sp, fp16 exp of
// f16(w - max), the exact integer sum of e * 2^24, inv = (float)(1 / sum), P16 = f16(e * inv)): the same bits
// as k_attn_mx, k_attn_rows and orc_attn_rows.
//
// Three launches per layer and slab of at most 256 rows; kernel boundaries are the only ordering (no counter,
// no spin, no co-residency assumption).  The unit is k_attn_mx's 16-row block: P = 16 / G positions x the G
// heads of a kv head, row m = p * G + g.
//  1) k_attn_mxl_scores, grid (key block of 256 positions, row block, kv head), 4 waves: the block's q operands
//     in registers (64 f32 per lane), wave w takes the 16-position key tiles w, w + 4, .. of its key block, the
//     next tile's K loads issued before the current tile's 64 MFMAs; folded scores -> sbuf [row][head][ld] f32
//     for the keys up to the block's last position.  A workgroup whose key block starts past that position
//     returns at once; the host launches no key block past the slab's last position.
//  2) k_attn_mxl_softmax, grid (head, row): max, integer-exact sum, P16 -> pbuf [row][head][ld] f16 over
//     [0, L_blk), L_blk the padded key count of the row block's last row: zeros on (sp, L_blk), so the 16 rows
//     of a block run one common length in 3).  Keys j > sp are never read (-inf whatever the scratch holds).
//     Padding rows of the slab's last block get zeros.
//  3) k_attn_mxl_kqv, grid (row block, kv head, 4 dim splits), 4 waves: each wave owns one 16-dim tile of V for
//     the whole key range, its 32 accumulator tiles stay in registers across windows of MXL_WIN positions x 16
//     rows of P16 staged in LDS between two barriers (64 KiB + the 16 B row skew of k_attn_mx: two workgroups
//     per CU); V streams from the [d][ctx] cache one step group ahead of its MFMAs.  Each output is one chain
//     over n_kv in ggml's step order; steps past a row's n_kv multiply P = 0, steps past L_blk are zero operands.
// Stale caches: K / V words past the pass's last row are finite (gemma_engine_extend zeroes them), as for k_attn_mx.
#include "device_util.h"
#include "kernels.h"

namespace ghip {
namespace {

typedef float mx4 __attribute__((ext_vector_type(4)));
constexpr int MXL_HD = 256;
constexpr int MXL_THREADS = 256, MXL_WAVES = MXL_THREADS / 64;
constexpr int MXL_KB = 256;                // key positions per scores workgroup: 16 tiles, 4 per wave
constexpr int MXL_WIN = 2048;              // P16 positions per LDS window
constexpr int MXL_SKEW = 8;                // halfs: the 16 rows of an MFMA operand read sit 16 B apart in the banks
constexpr int MXL_DSPLIT = MXL_HD / 16 / MXL_WAVES;  // 4 workgroups share the 16 dim tiles of a row block
constexpr int MXL_SLAB = 256;              // rows per slab (a multiple of every P)

struct mxl_args {
    attnp_args a;
    float *sbuf;
    uint16_t *pbuf;
    int t0, Ts;   // the slab: rows t0 .. t0 + Ts - 1 of the pass, slab row r = t - t0
    int ld;       // positions per (row, head) of sbuf / pbuf (a.n_kv)
};

// ggml_vec_dot_f16's fold of the 32 chain values of one output (as attn_mx.hip)
__device__ __forceinline__ float fold32(const mx4 acc[32], int r) {
    float x0[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const float a = acc[l][r] + acc[16 + l][r];
        const float b = acc[8 + l][r] + acc[24 + l][r];
        x0[l] = a + b;
    }
    float t0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t0[i] = x0[i] + x0[i + 4];
    const float h0 = t0[0] + t0[1], h1 = t0[2] + t0[3];
    return h0 + h1;
}

// 32 consecutive f16 (64 B) -> 32 f32 operands (exact widening)
__device__ __forceinline__ void widen32(const uint4 v[4], float out[32]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            out[8 * q + 2 * k] = h2f(w[k]);
            out[8 * q + 2 * k + 1] = h2f(w[k] >> 16);
        }
    }
}

// the row block rb of the slab (longest first): its first slab row, the sequence position of its last real row
// and that row's padded key count
struct mxl_block {
    int r0, s_last, L;
};
__device__ __forceinline__ mxl_block mxl_block_of(const mxl_args &x, int P, int rb_rev) {
    const int nrb = (x.Ts + P - 1) / P, rb = nrb - 1 - rb_rev;
    mxl_block b;
    b.r0 = rb * P;
    b.s_last = x.a.p0 + x.t0 + min(b.r0 + P - 1, x.Ts - 1);
    b.L = min(32 * ((b.s_last + 1) / 32 + 1), x.a.n_kv);
    return b;
}

__global__ void __launch_bounds__(MXL_THREADS, 2) k_attn_mxl_scores(mxl_args x) {
    const attnp_args &a = x.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = a.H / a.Hkv, P = 16 / G, kvh = blockIdx.z;
    const mxl_block b = mxl_block_of(x, P, blockIdx.y);
    const int n_keys = b.s_last + 1;  // positions past the block's last row are masked for all its rows
    const int n_kt = min((n_keys + 15) / 16, ((int)blockIdx.x + 1) * (MXL_KB / 16));
    const int kt0 = blockIdx.x * (MXL_KB / 16) + wave;
    if (kt0 >= n_kt) return;  // wave-uniform; the whole workgroup when its key block starts past s_last
    const int kvw = a.Hkv * MXL_HD;
    const int m_l = lane & 15, kk = lane >> 4;  // MFMA A row / B column, K index of this lane
    // q operands: row m_l = (position, head), elements 32(4t + kk) + c, t = 0, 1
    float qf[2][32];
    {
        const int r = b.r0 + m_l / G, h = kvh * G + m_l % G;
        const uint16_t *qr = a.q16 + ((int64_t)(x.t0 + (r < x.Ts ? r : 0)) * a.H + h) * MXL_HD;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            uint4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = *(const uint4 *)(qr + 32 * (4 * t + kk) + 8 * q);
            widen32(v, qf[t]);
        }
    }
    // this lane's 128 B of key row kt * 16 + m_l
    auto kload = [&](int kt, uint4 kv[2][4]) {
        const int j = kt * 16 + m_l;
        const uint16_t *kr = a.kc + (int64_t)(j < n_keys ? j : 0) * kvw + (int64_t)kvh * MXL_HD;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) kv[t][q] = *(const uint4 *)(kr + 32 * (4 * t + kk) + 8 * q);
    };
    uint4 kn[2][4];
    kload(kt0, kn);
    for (int kt = kt0; kt < n_kt; kt += MXL_WAVES) {
        uint4 kv[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) kv[t][q] = kn[t][q];
        if (kt + MXL_WAVES < n_kt) kload(kt + MXL_WAVES, kn);
        mx4 acc[32];
        const mx4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        {
            float kf[32];
            widen32(kv[0], kf);
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[0][c], kf[c], z, 0, 0, 0);
            widen32(kv[1], kf);
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[1][c], kf[c], acc[c], 0, 0, 0);
        }
        // register r of this lane: row m = 4 kk + r, key position kt * 16 + m_l
        const int jn = kt * 16 + m_l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float kq = fold32(acc, r);
            const int m = 4 * kk + r, row = b.r0 + m / G, h = kvh * G + m % G;
            if (jn < n_keys && row < x.Ts) x.sbuf[((int64_t)row * a.H + h) * x.ld + jn] = kq * 1.0f + 0.0f;  // ggml: kq * scale + mask
        }
    }
}

// grid (head, slab row incl. the last block's padding rows)
__global__ void __launch_bounds__(MXL_THREADS) k_attn_mxl_softmax(mxl_args x) {
    __shared__ uint32_t mx_key;
    __shared__ unsigned long long e_sum;
    const attnp_args &a = x.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int G = a.H / a.Hkv, P = 16 / G, h = blockIdx.x, row = blockIdx.y;
    const int nrb = (x.Ts + P - 1) / P;
    const mxl_block b = mxl_block_of(x, P, nrb - 1 - row / P);
    const float *S = x.sbuf + ((int64_t)row * a.H + h) * x.ld;
    uint16_t *Pr = x.pbuf + ((int64_t)row * a.H + h) * x.ld;
    if (row >= x.Ts) {  // padding row: zero operands of the block's MFMAs (its outputs are not stored)
        for (int j = tid; j < b.L; j += MXL_THREADS) Pr[j] = 0;
        return;
    }
    const int sp = a.p0 + x.t0 + row, n = sp + 1;  // keys 0 .. sp; the rest of the row's n_kv is masked: e = 0
    if (tid == 0) {
        mx_key = 0u;  // below the key of every float, -inf included
        e_sum = 0ull;
    }
    __syncthreads();
    float lmax = -INFINITY;
    for (int j = tid; j < n; j += MXL_THREADS) lmax = fmaxf(lmax, S[j]);
    lmax = wave_max(lmax);
    if (lane == 0) {
        const uint32_t k = __builtin_bit_cast(uint32_t, lmax);
        atomicMax(&mx_key, (k & 0x80000000u) ? ~k : (k | 0x80000000u));
    }
    __syncthreads();
    const uint32_t key = mx_key;
    const float mx = __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
    // e values are fp16 in [0, 1]: exact multiples of 2^-24, so the integer sum is the exact sum in any order
    unsigned long long isum = 0;
    for (int j = tid; j < n; j += MXL_THREADS) {
        const float w = S[j];
        uint16_t e16 = 0;
        if (w != -INFINITY) e16 = (uint16_t)exp_f16_of(f2h(w - mx));
        Pr[j] = e16;  // parked: this thread reads it back below
        isum += (unsigned long long)(uint32_t)(h2f(e16) * 16777216.0f);
    }
    isum = wave_sum_u64(isum);
    if (lane == 0 && isum) atomicAdd(&e_sum, isum);
    __syncthreads();
    const double sum = (double)e_sum * (1.0 / 16777216.0);
    const float inv = (float)(1.0 / sum);
    for (int j = tid; j < b.L; j += MXL_THREADS) Pr[j] = j < n ? (uint16_t)f2h(h2f(Pr[j]) * inv) : (uint16_t)0;
}

__global__ void __launch_bounds__(MXL_THREADS, 2) k_attn_mxl_kqv(mxl_args x, int win) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const attnp_args &a = x.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = a.H / a.Hkv, P = 16 / G, kvh = blockIdx.y;
    const mxl_block b = mxl_block_of(x, P, blockIdx.x);
    const int L = b.L, WS = win + MXL_SKEW;
    uint16_t *Ps = (uint16_t *)smem;  // [16][WS]: P16 of the block's rows, positions w0 .. w0 + win
    const int m_l = lane & 15, kk = lane >> 4;
    const int dt = blockIdx.z * MXL_WAVES + wave;  // this wave's 16-dim tile
    const uint16_t *vr = a.vc + ((int64_t)kvh * MXL_HD + dt * 16 + m_l) * a.ctx;  // this lane's V row (B column)
    const uint16_t *pr = Ps + m_l * WS;                                            // A row m_l
    const uint16_t *pg = x.pbuf + ((int64_t)b.r0 * a.H + (int64_t)kvh * G) * x.ld;  // row m of the block: + m * ld
    mx4 acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = (mx4){0.0f, 0.0f, 0.0f, 0.0f};
    // this lane's V step of group u (positions 32(4u + kk) ..), one group ahead of its MFMAs
    auto vload = [&](int u, uint4 vv[4]) {
        const int e0 = 32 * (4 * u + kk);
#pragma unroll
        for (int q = 0; q < 4; ++q) vv[q] = e0 < L ? *(const uint4 *)(vr + e0 + 8 * q) : make_uint4(0u, 0u, 0u, 0u);
    };
    const int n_sg = (L / 32 + 3) / 4;  // step groups (steps past L: zero operands)
    uint4 vn[4];
    vload(0, vn);
    for (int w0 = 0; w0 < L; w0 += win) {
        const int wn = min(L - w0, win), nch = wn / 8;  // L % 32 == 0
        if (w0) __syncthreads();  // the window before is consumed
        // rows (p, g) of the block are rows r0 + p, heads kvh * G + g of pbuf: consecutive (row, head) pairs
        for (int idx = tid; idx < 16 * nch; idx += MXL_THREADS) {
            const int m = idx / nch, c = idx % nch;
            *(uint4 *)(Ps + m * WS + c * 8) =
                *(const uint4 *)(pg + ((int64_t)(m / G) * a.H + m % G) * x.ld + w0 + c * 8);
        }
        __syncthreads();
        const int u1 = w0 + win >= L ? n_sg : (w0 + win) / 128;  // a window that is not the last is MXL_WIN: whole groups
        for (int u = w0 / 128; u < u1; ++u) {
            const int e0 = 32 * (4 * u + kk);  // this lane's step: positions e0 .. e0 + 31
            uint4 pv[4], vv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q] = vn[q];
            if (u + 1 < n_sg) vload(u + 1, vn);
#pragma unroll
            for (int q = 0; q < 4; ++q) pv[q] = e0 < L ? *(const uint4 *)(pr + (e0 - w0) + 8 * q) : make_uint4(0u, 0u, 0u, 0u);
            float pf[32], vf[32];
            widen32(pv, pf);
            widen32(vv, vf);
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[c], vf[c], acc[c], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = 4 * kk + r, row = b.r0 + m / G, h = kvh * G + m % G;
        const float o = fold32(acc, r);
        if (row < x.Ts) a.out[(int64_t)(x.t0 + row) * a.ldo + (int64_t)h * MXL_HD + dt * 16 + m_l] = o;
    }
}

}  // namespace

// nullptr when the key-split matrix-core form runs these shapes, else why not
const char *attn_mx_long_unsupported(const attnp_args &a) {
    if (a.hd != MXL_HD) return "head_dim != 256";
    if (a.Hkv <= 0 || a.H <= 0 || a.H % a.Hkv) return "heads";
    const int G = a.H / a.Hkv;
    if (G > 16 || 16 % G) return "query heads per kv head must divide 16";
    if (a.ctx <= 0 || a.ctx % 32 || a.n_kv <= 0 || a.n_kv % 32) return "n_ctx and n_kv must be multiples of 32";
    if (a.n_kv > a.ctx) return "n_kv > n_ctx";
    if (a.ctx > ATTN_MX_LONG_MAX_CTX) return "n_ctx > 8192";
    if (a.T <= 0 || a.p0 < 0 || a.p0 + a.T > a.n_kv) return "rows past n_kv";
    return nullptr;
}

size_t attn_mx_long_scratch(int slab_rows, int H, int ctx, bool p16) { return (size_t)slab_rows * H * ctx * (p16 ? 2 : 4); }
int attn_mx_long_slab_rows(int T) { return std::min(MXL_SLAB, (T + 15) / 16 * 16); }

int launch_attn_mx_long(const attnp_args &a, float *sbuf, uint16_t *pbuf, int slab_rows, hipStream_t s) {
    if (const char *why = attn_mx_long_unsupported(a)) {
        set_error(std::string("attn_mx_long: ") + why);
        return -1;
    }
    if (!sbuf || !pbuf || slab_rows < 16 || slab_rows % 16 || (slab_rows < MXL_SLAB && slab_rows < a.T)) {
        set_error("attn_mx_long: scratch of min(256, T rounded up to 16) rows needed");
        return -1;
    }
    const int slab = std::min(slab_rows, MXL_SLAB), G = a.H / a.Hkv, P = 16 / G;
    if (allow_full_lds((const void *)k_attn_mxl_kqv, LDS_SLOT_ATTN_MXL)) return -1;
    for (int t0 = 0; t0 < a.T; t0 += slab) {
        mxl_args x{a, sbuf, pbuf, t0, std::min(slab, a.T - t0), a.n_kv};
        const int nrb = (x.Ts + P - 1) / P, s_last = a.p0 + t0 + x.Ts - 1;
        const int nkb = s_last / MXL_KB + 1;  // key blocks that some row block needs
        const int Lmax = std::min(32 * ((s_last + 1) / 32 + 1), a.n_kv), win = std::min(Lmax, MXL_WIN);
        hipLaunchKernelGGL(k_attn_mxl_scores, dim3(nkb, nrb, a.Hkv), dim3(MXL_THREADS), 0, s, x);
        GHIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_attn_mxl_softmax, dim3(a.H, nrb * P), dim3(MXL_THREADS), 0, s, x);
        GHIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_attn_mxl_kqv, dim3(nrb, a.Hkv, MXL_DSPLIT), dim3(MXL_THREADS),
                           (size_t)16 * (win + MXL_SKEW) * 2, s, x, win);
        GHIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace ghip
