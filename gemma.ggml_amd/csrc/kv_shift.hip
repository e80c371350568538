// kv_shift.hip — the context shift (gemma_engine_shift, DESIGN.md §5b′ "Context shift"): positions
// [keep, keep + discard) of a sequence are dropped and everything behind them moves down by `discard`,
// in place, in every layer's caches.  With n = pos - discard the new length, for x in [keep, pos):
//
//   V [kvw][ctx]:  V[j][x] = V[j][x + discard]           (bits)     x < n, else 0
//   K [ctx][kvw]:  K[x]    = rope(K[x + discard], -discard)         x < n, else 0
//
// K is stored after RoPE, so a moved row is rotated back by `discard` positions: with c | s the RoPE
// row of position `discard` and (x0, x1) the NEOX pair (i, i + hd/2), out0 = f16(x0 c + x1 s),
// out1 = f16(x1 c - x0 s), each product and sum one f32 operation (k_rows_rope_kv's forms, batch.hip).
//
// The move overlaps itself (destination x, source x + discard > x).  Both kernels are driven by the
// DESTINATION and give every word one owner: a workgroup owns a strip of the cache over all positions
// and walks it in ascending windows, so the reader and the writer of every word are the same
// workgroup.  Per window: the loads of window w + 1 are issued, the values of window w pass a barrier,
// window w is stored.  A window's sources lie above its destinations, and above every destination of
// an earlier window, so a store never reaches a word that is still to be read; the barrier orders the
// loads of a window (any thread) before its stores (any thread).  No workgroup waits for another: no
// counter, no spin, no residency assumption, no scratch image.
//
//  * k_shift_k   grid (Hkv * slices, n_layer).  A strip is 16 NEOX pairs of one kv head (8 when hd/2 is
//                an odd multiple of 8): per row two 32-byte segments, hd/2 apart.  A thread keeps 8 pairs
//                of c | s in registers for the whole walk and handles KS_ROWS rows of a window, each one
//                16-byte load and store per segment.
//  * k_shift_v   grid (kvw, n_layer): one cache row [ctx] per workgroup.  Destination and source differ
//                by 2 * discard mod 16 bytes, so a window of VS_WORDS aligned 16-byte destination words
//                is staged through the LDS: the aligned source words that cover it (one more than the
//                window when the offsets differ) are loaded into registers one window ahead, written to
//                a double-buffered LDS image, and read back at the element offset.  Whole words are
//                stored as 16 bytes; the two ragged words (around `keep`, around `pos`) element by
//                element, so nothing below `keep` or from `pos` on is written.
//  * k_shift_seq one workgroup: hist moved the same way (the pending token hist[pos] included, the
//                vacated entries zero), *pos = n with its RoPE row (publish_rope_row), *nfix, the epoch
//                bump and the decode step's argmax keys back to zero, as gemma_engine_extend leaves them.
#include "device_util.h"
#include "kernels.h"
#include "pick.h"

namespace ghip {
namespace {

constexpr int KS_ROWS = 4;       // rows of a window per thread (k_shift_k): 8 x 16 bytes in flight per thread
constexpr int VS_WORDS = 256;    // 16-byte destination words per window (k_shift_v): one per thread

// 8 f16 (a 16-byte word) <-> f32
__device__ __forceinline__ void unpack8(const uint4 &w, float *f) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = h2f(u[i] & 0xFFFFu);
        f[2 * i + 1] = h2f(u[i] >> 16);
    }
}
__device__ __forceinline__ uint4 pack8(const float *f) {
    uint32_t u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = f2h(f[2 * i]) | (f2h(f[2 * i + 1]) << 16);
    return make_uint4(u[0], u[1], u[2], u[3]);
}

// su: threads per row of the strip (1 or 2), each 8 pairs; rows of a window: (256 / su) * KS_ROWS
__global__ void __launch_bounds__(256) k_shift_k(uint16_t *kc, int64_t layer_stride, int kvw, int hd, int su, int pos, int keep,
                                                 int discard, const float *cs, const float *sn) {
    const int half = hd / 2, U = half / 8;                   // 8-pair units per head
    const int tid = threadIdx.x, rw = 256 / su;              // rows per pass of the workgroup
    const int unit = blockIdx.x * su + tid % su, r = tid / su;
    const int lo = (unit / U) * hd + (unit % U) * 8;         // the unit's first element of a row; its partners at lo + half
    uint16_t *K = kc + (int64_t)blockIdx.y * layer_stride;
    float c[8], s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c[i] = cs[(unit % U) * 8 + i];
        s[i] = sn[(unit % U) * 8 + i];
    }
    const int n = pos - discard, win = rw * KS_ROWS;
    uint4 a[KS_ROWS], b[KS_ROWS], na[KS_ROWS] = {}, nb[KS_ROWS] = {};
    // destination row x of slot j of the window at x0; its source x + discard is read while x < n
    auto load = [&](int x0, uint4 *A, uint4 *B) {
#pragma unroll
        for (int j = 0; j < KS_ROWS; ++j) {
            const int x = x0 + j * rw + r;
            A[j] = B[j] = make_uint4(0, 0, 0, 0);
            if (x < n) {
                const uint16_t *row = K + (int64_t)(x + discard) * kvw + lo;
                A[j] = *(const uint4 *)row;
                B[j] = *(const uint4 *)(row + half);
            }
        }
    };
    load(keep, a, b);
    for (int x0 = keep; x0 < pos; x0 += win) {
        if (x0 + win < pos) load(x0 + win, na, nb);  // the next window's sources lie above every row stored so far
#pragma unroll
        for (int j = 0; j < KS_ROWS; ++j) {
            if (x0 + j * rw + r >= n) continue;      // the vacated tail stays zero
            float f0[8], f1[8], o0[8], o1[8];
            unpack8(a[j], f0);
            unpack8(b[j], f1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float p0 = f0[i] * c[i], p1 = f1[i] * s[i], p2 = f0[i] * s[i], p3 = f1[i] * c[i];
                o0[i] = p0 + p1;
                o1[i] = p3 - p2;
            }
            a[j] = pack8(o0);
            b[j] = pack8(o1);
        }
        __syncthreads();  // every load of this window (and of the next) is ordered before this window's stores
#pragma unroll
        for (int j = 0; j < KS_ROWS; ++j) {
            const int x = x0 + j * rw + r;
            if (x < pos) {
                uint16_t *row = K + (int64_t)x * kvw + lo;
                *(uint4 *)row = a[j];
                *(uint4 *)(row + half) = b[j];
            }
            a[j] = na[j];
            b[j] = nb[j];
        }
    }
}

__global__ void __launch_bounds__(256) k_shift_v(uint16_t *vc, int64_t layer_stride, int ctx, int pos, int keep, int discard) {
    __shared__ __attribute__((aligned(16))) uint16_t img[2][(VS_WORDS + 2) * 8];
    const int tid = threadIdx.x;
    uint16_t *V = vc + (int64_t)blockIdx.y * layer_stride + (int64_t)blockIdx.x * ctx;
    const int n = pos - discard, dw = discard >> 3, de = discard & 7;
    const int g_end = (pos + 7) >> 3;  // destination words [keep / 8, g_end)
    // the aligned source words of the window whose first destination word is g0: g0 + dw + t, t <= VS_WORDS;
    // thread 0 also takes the one past the window.  Only words that hold an element below pos are read
    uint4 cur, cur_x, nxt = make_uint4(0, 0, 0, 0), nxt_x = make_uint4(0, 0, 0, 0);
    auto load = [&](int g0, uint4 &w, uint4 &wx) {
        const int sw = g0 + dw + tid;
        w = wx = make_uint4(0, 0, 0, 0);
        if (sw * 8 < pos) w = *(const uint4 *)(V + (int64_t)sw * 8);
        if (tid == 0 && (sw + VS_WORDS) * 8 < pos) wx = *(const uint4 *)(V + (int64_t)(sw + VS_WORDS) * 8);
    };
    int buf = 0;
    load(keep >> 3, cur, cur_x);
    for (int g0 = keep >> 3; g0 < g_end; g0 += VS_WORDS, buf ^= 1) {
        if (g0 + VS_WORDS < g_end) load(g0 + VS_WORDS, nxt, nxt_x);  // issued before this window's stores
        *(uint4 *)(img[buf] + tid * 8) = cur;
        if (tid == 0) *(uint4 *)(img[buf] + VS_WORDS * 8) = cur_x;
        __syncthreads();  // the window's sources are in the LDS: its stores cannot reach an unread word
        const int g = g0 + tid;
        if (g < g_end) {
            const uint16_t *src = img[buf] + tid * 8 + de;  // element 8 g + discard of the row
            uint16_t o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = 8 * g + i < n ? src[i] : (uint16_t)0;  // the vacated tail is zero
            if (8 * g >= keep && 8 * g + 8 <= pos) {
                *(uint4 *)(V + (int64_t)g * 8) = make_uint4(o[0] | ((uint32_t)o[1] << 16), o[2] | ((uint32_t)o[3] << 16),
                                                             o[4] | ((uint32_t)o[5] << 16), o[6] | ((uint32_t)o[7] << 16));
            } else {  // the ragged first and last words: only the elements of [keep, pos)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (8 * g + i >= keep && 8 * g + i < pos) V[(int64_t)g * 8 + i] = o[i];
            }
        }
        cur = nxt;
        cur_x = nxt_x;
    }
}

__global__ void __launch_bounds__(256) k_shift_seq(int *hist, int *pos_w, int *nfix, int fixed, int pos, int keep, int discard,
                                                   rope_row r, unsigned long long *zero_keys, int n_zero) {
    const int tid = threadIdx.x, n = pos - discard;
    // hist[x] = hist[x + discard] for x in [keep, n], the pending token at n included; then zero up to pos
    for (int x0 = keep; x0 <= pos; x0 += 256) {
        const int x = x0 + tid;
        const int v = x <= n ? hist[x + discard] : 0;
        __syncthreads();  // this window's loads before its stores; its sources lie above every earlier store
        if (x <= pos) hist[x] = v;
    }
    if (tid == 0) {
        *pos_w = n;
        *nfix = fixed;
        if (r.epoch) ++*r.epoch;
    }
    publish_rope_row(r.cur, r.cos, r.sin, r.half, n);
    for (int j = tid; j < n_zero; j += 256) zero_keys[j] = 0;
}

}  // namespace

const char *kv_shift_unsupported(int ctx, int Hkv, int hd) {
    if (Hkv < 1 || hd < 16 || hd % 16) return "head_dim must be a multiple of 16";
    if (ctx < 8 || ctx % 8) return "n_ctx must be a multiple of 8";
    return nullptr;
}

int launch_kv_shift(const kv_shift_args &a, hipStream_t s) {
    if (const char *why = kv_shift_unsupported(a.ctx, a.Hkv, a.hd)) {
        set_error(std::string("kv_shift: ") + why);
        return -1;
    }
    if (!a.kc || !a.vc || !a.cs || !a.sn || a.n_layer < 1 || a.keep < 0 || a.discard < 1 || a.pos >= a.ctx ||
        (int64_t)a.keep + a.discard > a.pos) {
        set_error("kv_shift: needs 0 <= keep, 1 <= discard, keep + discard <= pos < n_ctx");
        return -1;
    }
    const int kvw = a.Hkv * a.hd, U = a.hd / 16, su = U % 2 ? 1 : 2;
    hipLaunchKernelGGL(k_shift_k, dim3(a.Hkv * U / su, a.n_layer), dim3(256), 0, s, a.kc, a.layer_stride, kvw, a.hd, su, a.pos,
                       a.keep, a.discard, a.cs, a.sn);
    GHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_shift_v, dim3(kvw, a.n_layer), dim3(256), 0, s, a.vc, a.layer_stride, a.ctx, a.pos, a.keep, a.discard);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_seq_shift(int *hist, int *pos_word, int *nfix, int fixed, int pos, int keep, int discard, const rope_row &r,
                     unsigned long long *zero_keys, int n_zero, hipStream_t s) {
    if (keep < 0 || discard < 1 || pos >= r.ctx || (int64_t)keep + discard > pos) {
        set_error("seq_shift: needs 0 <= keep, 1 <= discard, keep + discard <= pos < n_ctx");
        return -1;
    }
    hipLaunchKernelGGL(k_shift_seq, dim3(1), dim3(256), 0, s, hist, pos_word, nfix, fixed, pos, keep, discard, r, zero_keys, n_zero);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
