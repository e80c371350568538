// toplogprob.hip — the n most likely tokens of every logits row of a pass, with their log-probabilities
// (DESIGN.md §5b⁗′ "Alternatives"; the rule is stated in include/gemma_hpc.h at
// gemma_engine_set_top_logprobs): the min(n, V) entries with the largest pick keys argmax_key(l[i], i)
// (pick.h), in descending key order, each with logprob(l, i) by k_lse_finish's rule.
//
// Two launches with a kernel boundary between them, beside the log-probability pair:
//   k_topn_parts   grid (Gt, R), right behind k_lse_parts: workgroup g reads chunk g of row r once
//                  (TOPN_CHUNK logits, four 16-byte loads per thread, all issued before the first is
//                  used), keeps its 16 keys per thread in registers and leaves the chunk's n largest,
//                  sorted descending and padded with key 0, in tparts[r][g][0 .. n).
//   k_topn_finish  grid (1, R), right behind k_lse_finish: the row's Gt * n candidates, a key per thread
//                  and round in registers, through the same selection; M and S from the lse_parts
//                  (lse_impl.h), then lane i < n of wave 0 writes alt_tok[q][i] and alt_lp[q][i].
//
// The selection (block_top_n) is exact and its result a function of the keys alone: the keys of a row
// are distinct, the histograms hold integer counts (atomics in any order give the same sums), the
// survivors are compacted in any order and then sorted by one wave.
//   1. Bound.  The n-th largest of the 256 thread maxima is at most the n-th largest key, so every
//      key below it is out.  On logits this leaves between n and a few n keys, and the hot first
//      levels of the descent below see 256 keys in place of 4,096 (LDS atomics on one address
//      serialise).
//   2. Radix descent (radix_top), 8 key bits per level from the top: the 32 value bits, then the low
//      index bits that can differ (12 inside a chunk, 20 in a row).  A level counts the digits of the
//      keys still tied with the n-th largest, scans the 256 counts from the top and finds the digit
//      of the n-th largest; keys with a larger digit are in, with a smaller one out.  It ends as soon
//      as the chosen digit's keys are all needed, at the latest at the last level: distinct keys.
//      A thread keeps what is tied and what is in as two bit masks over its register keys, so no
//      register array is indexed by a variable (0 scratch).
#include "lse_impl.h"
#include "pick.h"

namespace ghip {
namespace {

typedef unsigned long long u64;

constexpr int TOPN_TH = 256, TOPN_LOADS = 4;
static_assert(TOPN_CHUNK == TOPN_TH * TOPN_LOADS * 4, "four 16-byte loads per thread and chunk");
static_assert(TOPN_TH == LSE_TH, "k_topn_finish runs lse_merge");
constexpr int TOPN_CHUNK_BITS = 12;  // index bits that differ inside a chunk
static_assert(TOPN_CHUNK == 1 << TOPN_CHUNK_BITS, "a chunk's indices share the bits above these");
constexpr int TOPN_ROW_BITS = 20;    // ... inside a row: n_vocab <= LSE_MAX_G * LSE_CHUNK = 2^20
static_assert((int64_t)LSE_MAX_G * LSE_CHUNK == 1 << TOPN_ROW_BITS, "the log-probability code's n_vocab limit");

struct topn_lds {
    unsigned hist[256];
    unsigned wtot[TOPN_TH / 64];
    int digit, rem, stop;
    unsigned cnt;
    u64 bound;
    u64 out[TOPN_MAX];
};

// Of this thread's keys key[j] with bit j of `tied` set (all the block's such keys distinct, none 0),
// the ones among the block's n largest such keys, as a bit mask; all of them when the block has fewer
// than n.  low_bits: the key's bits 32 .. 63 and 0 .. low_bits - 1 are the only ones that differ.
template <int KPT>
__device__ __forceinline__ uint32_t radix_top(const u64 (&key)[KPT], uint32_t tied, int n, int low_bits, topn_lds &L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int low_levels = (low_bits + 7) >> 3;
    uint32_t in = 0;
    int rem = n;  // the n-th largest key is the rem-th largest tied one
    L.hist[tid] = 0;
    __syncthreads();
    for (int lvl = 0; lvl < 4 + low_levels; ++lvl) {
        const int sh = lvl < 4 ? 56 - 8 * lvl : 8 * (3 + low_levels - lvl);
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if ((tied >> j) & 1u) atomicAdd(&L.hist[(unsigned)(key[j] >> sh) & 255u], 1u);
        __syncthreads();
        // thread t owns digit 255 - t: the keys with its digit or a larger one (inclusive scan from the top)
        const unsigned c = L.hist[255 - tid];
        L.hist[255 - tid] = 0;  // for the next level
        unsigned incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == 63) L.wtot[wave] = incl;
        __syncthreads();
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < TOPN_TH / 64; ++w) {
            if (w < wave) incl += L.wtot[w];
            total += L.wtot[w];
        }
        if (total < (unsigned)rem) return in | tied;  // fewer than n keys in all (the first level only)
        const unsigned above = incl - c;
        if (incl >= (unsigned)rem && above < (unsigned)rem) {  // one thread: the n-th largest key's digit
            L.digit = 255 - tid;
            L.rem = rem - (int)above;
            L.stop = c == (unsigned)rem - above;  // every key of the digit is needed
        }
        __syncthreads();
        const unsigned digit = (unsigned)L.digit;
        rem = L.rem;
        const int stop = L.stop;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const unsigned d = (unsigned)(key[j] >> sh) & 255u;
            const uint32_t bit = ((tied >> j) & 1u) << j;
            if (d > digit) in |= bit;
            if (d != digit) tied &= ~bit;
        }
        if (stop) break;
    }
    return in | tied;
}

// The n largest of the block's keys (KPT per thread; key 0: no key; the others distinct), sorted
// descending and padded with key 0: wave 0's return value, lane i holding the i-th largest (i < 32).
// n in [1, TOPN_MAX].  256 threads.
template <int KPT>
__device__ __forceinline__ u64 block_top_n(const u64 (&key)[KPT], int n, int low_bits, topn_lds &L) {
    const int tid = threadIdx.x;
    uint32_t tied = 0;
    u64 mx = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        tied |= (uint32_t)(key[j] != 0) << j;
        mx = key[j] > mx ? key[j] : mx;
    }
    if (KPT > 1) {  // the bound: the smallest of the n largest thread maxima (none while fewer than n threads hold a key)
        if (tid == 0) {
            L.cnt = 0;
            L.bound = ~0ull;
        }
        const u64 one[1] = {mx};
        const uint32_t top = radix_top<1>(one, mx != 0, n, low_bits, L);  // (its barriers order the two words above)
        if (top) {
            atomicAdd(&L.cnt, 1u);
            atomicMin(&L.bound, mx);
        }
        __syncthreads();
        const u64 bound = L.cnt == (unsigned)n ? L.bound : 0;
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (key[j] < bound) tied &= ~(1u << j);
    }
    const uint32_t in = radix_top<KPT>(key, tied, n, low_bits, L);  // (at least two barriers before the words are rewritten)
    if (tid < TOPN_MAX) L.out[tid] = 0;
    if (tid == 0) L.cnt = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if ((in >> j) & 1u) {
            const unsigned slot = atomicAdd(&L.cnt, 1u);
            if (slot < (unsigned)TOPN_MAX) L.out[slot] = key[j];
        }
    __syncthreads();
    if (tid >= 64) return 0;
    // one key per lane, a bitonic network by shuffles over lanes 0 .. 31 (the lanes above mirror them)
    u64 v = L.out[tid & (TOPN_MAX - 1)];
#pragma unroll
    for (int k = 2; k <= TOPN_MAX; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 o = __shfl_xor(v, j);
            const bool first = (tid & j) == 0, desc = (tid & k) == 0 || k == TOPN_MAX;
            v = (first == desc) == (o > v) ? o : v;  // the pair's first lane keeps the larger key of a descending run
        }
    return v;
}

__global__ void __launch_bounds__(TOPN_TH) k_topn_parts(const float *lg, int64_t ld, int n_vocab, int n, u64 *tparts) {
    __shared__ topn_lds L;
    const int tid = threadIdx.x;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    const int base = blockIdx.x * TOPN_CHUNK + tid * 4;
    float4 q[TOPN_LOADS];
#pragma unroll
    for (int j = 0; j < TOPN_LOADS; ++j) {  // load j of the thread: 16 bytes, the wave's 1 KiB contiguous
        const int i0 = base + j * (TOPN_TH * 4);
        if (i0 + 4 <= n_vocab && ((uintptr_t)(row + i0) & 15) == 0) {
            q[j] = *(const float4 *)(row + i0);
        } else {  // a misaligned row, the row's tail: guarded scalars (past the end: no key below)
            q[j].x = i0 + 0 < n_vocab ? row[i0 + 0] : 0.0f;
            q[j].y = i0 + 1 < n_vocab ? row[i0 + 1] : 0.0f;
            q[j].z = i0 + 2 < n_vocab ? row[i0 + 2] : 0.0f;
            q[j].w = i0 + 3 < n_vocab ? row[i0 + 3] : 0.0f;
        }
    }
    u64 key[TOPN_LOADS * 4];
#pragma unroll
    for (int j = 0; j < TOPN_LOADS; ++j) {
        const int i0 = base + j * (TOPN_TH * 4);
        key[4 * j + 0] = i0 + 0 < n_vocab ? argmax_key(q[j].x, i0 + 0) : 0;
        key[4 * j + 1] = i0 + 1 < n_vocab ? argmax_key(q[j].y, i0 + 1) : 0;
        key[4 * j + 2] = i0 + 2 < n_vocab ? argmax_key(q[j].z, i0 + 2) : 0;
        key[4 * j + 3] = i0 + 3 < n_vocab ? argmax_key(q[j].w, i0 + 3) : 0;
    }
    const u64 v = block_top_n<TOPN_LOADS * 4>(key, n, TOPN_CHUNK_BITS, L);
    if (tid < n) tparts[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n + tid] = v;
}

// KPT: candidates per thread, Gt * n <= 256 * KPT
template <int KPT>
__global__ void __launch_bounds__(TOPN_TH) k_topn_finish(topn_finish_args a) {
    __shared__ topn_lds L;
    __shared__ lse_merge_lds ML;
    __shared__ double S_all;
    const int tid = threadIdx.x, r = blockIdx.y;
    const int last = lse_last_row(a.l);
    if (r > last || last >= a.l.R) return;
    const int total = a.Gt * a.top;
    const u64 *cand = a.tparts + (int64_t)r * total;
    u64 key[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) key[j] = tid + j * TOPN_TH < total ? cand[tid + j * TOPN_TH] : 0;
    const u64 v = block_top_n<KPT>(key, a.top, TOPN_ROW_BITS, L);
    const float M = lse_merge(a.l.parts + (int64_t)r * a.l.G, a.l.G, ML, &S_all);
    __syncthreads();
    if (tid >= a.top) return;
    lse_target t;
    if (!lse_target_of(a.l, r, last, &t)) return;
    const int64_t o = (int64_t)t.q * TOPN_MAX + tid;
    // past the row's entries (n > n_vocab): token -1, the all-ones NaN
    t.alt_tok[o] = v ? key_index(v) : -1;
    t.alt_lp[o] = v ? lse_value(key_value(v), M, S_all) : __builtin_bit_cast(double, ~0ull);
}

}  // namespace

int topn_grid(int64_t n_vocab) { return (int)((n_vocab + TOPN_CHUNK - 1) / TOPN_CHUNK); }

static bool topn_shape_ok(int rows, int64_t n_vocab, int n) {
    if (rows >= 1 && rows <= 65535 && n_vocab >= 1 && n_vocab <= (int64_t)LSE_MAX_G * LSE_CHUNK && n >= 1 && n <= TOPN_MAX) return true;
    set_error("top logprobs: rows outside [1, 65535], n_vocab outside [1, " + std::to_string((int64_t)LSE_MAX_G * LSE_CHUNK) +
              "] or n outside [1, " + std::to_string(TOPN_MAX) + "]");
    return false;
}

int launch_topn_parts(const float *lg, int64_t ld, int rows, int64_t n_vocab, int n, unsigned long long *tparts, hipStream_t s) {
    if (!topn_shape_ok(rows, n_vocab, n)) return -1;
    if (!lg || !tparts) {
        set_error("top logprobs: no rows or no candidate scratch");
        return -1;
    }
    hipLaunchKernelGGL(k_topn_parts, dim3(topn_grid(n_vocab), rows), dim3(TOPN_TH), 0, s, lg, ld, (int)n_vocab, n, tparts);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_topn_finish(const topn_finish_args &a, hipStream_t s) {
    if (!topn_shape_ok(a.l.R, a.l.n, a.top)) return -1;
    if (!a.tparts || !a.l.parts || a.Gt != topn_grid(a.l.n) || a.l.G != lse_grid(a.l.n) ||
        (!a.l.tab && (!a.l.pos || !a.l.alt_tok || !a.l.alt_lp))) {
        set_error("top logprobs: the finish launch's candidates, partials or sequence are not set");
        return -1;
    }
    const int per = (a.Gt * a.top + TOPN_TH - 1) / TOPN_TH;  // <= 32: Gt <= 256, n <= 32
    const dim3 grid(1, a.l.R), block(TOPN_TH);
    if (per <= 1) hipLaunchKernelGGL(k_topn_finish<1>, grid, block, 0, s, a);
    else if (per <= 2) hipLaunchKernelGGL(k_topn_finish<2>, grid, block, 0, s, a);
    else if (per <= 4) hipLaunchKernelGGL(k_topn_finish<4>, grid, block, 0, s, a);
    else if (per <= 8) hipLaunchKernelGGL(k_topn_finish<8>, grid, block, 0, s, a);
    else if (per <= 16) hipLaunchKernelGGL(k_topn_finish<16>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_topn_finish<32>, grid, block, 0, s, a);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
