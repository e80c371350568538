// sample.hip — seeded temperature / top-k / top-p sampling of one logits row on the device
// (DESIGN.md §5b″; the rule is stated in include/gemma_hpc.h at gemma_engine_set_sampler).
//
// The row is the f32 logits the launch before just wrote (L2 / Infinity Cache traffic).  Three
// launches, a kernel boundary between the phases (no in-launch cross-workgroup hand-off):
//   k_sample_hist     wide: every logit -> a monotone u32 key (larger logit = larger key, -0 = +0);
//                     an LDS histogram of the key's top 12 bits per workgroup, its non-zero bins
//                     added to one global histogram (integer atomics: the sums are order-free)
//   k_sample_compact  wide: every workgroup finds the bin b* that holds the K-th largest key from
//                     that histogram; keys in bins above b* go to list A (fewer than K), keys in
//                     b* to list B, each as the u64 (key << 32 | ~index) — the argmax-key format,
//                     unique per entry, "larger" = larger logit, then smaller index.  Ranges of the
//                     lists are reserved with one atomic per workgroup and list: the arrival order
//                     shows in the lists and is removed by the sort below
//   k_sample_tail     one workgroup: A and B into LDS (B first narrowed to its K - |A| largest by
//                     a radix select when A + B exceed the LDS array: tie-heavy rows), a bitonic
//                     sort (descending: logit desc, index asc), the first K are the candidates;
//                     f64 weights, prefix sums, the top-p cut, the splitmix64 draw keyed by
//                     (seed, p = *pos + 1); one key in the argmax format for k_advance.  It also
//                     zeroes the histogram and the list cursors for the next call.
// Parameters per row (a batch pass, "A sampler per slot" in DESIGN.md §5b⁗): with a row table row r
// reads its own sampler_params from its entry, tab[r].smp, wave-uniformly (a scalar load of the same
// depth as the one struct's, as k_attn_slots reads its table entry).  A row whose temperature is <= 0
// is greedy: its workgroups leave all three kernels on that wave-uniform branch before their first
// atomic, so its workspace stays as it was (zero) and its key slot (the row-argmax launch's partial
// keys) stands.
// The result depends on the row and the parameters only.  K <= 1024; the launch geometry does not
// depend on top_k (it is read from the device struct), so only sampling on / off changes a graph.
#include <algorithm>

#include "kernels.h"
#include "pick.h"

namespace ghip {
namespace {

constexpr int SM_BINS = 4096, SM_SHIFT = 20;  // histogram over the key's top 12 bits
constexpr int SM_TH = 256, SM_PER = 8, SM_CHUNK = SM_TH * SM_PER;  // logits per workgroup pass
constexpr int SM_GRID_MAX = 1024;
constexpr int SM_TAIL = 1024;  // the tail workgroup: one thread per candidate
constexpr int SM_CAP = 2048;   // entries the tail sorts (>= SAMPLE_MAX_K)
static_assert(SM_TAIL == SAMPLE_MAX_K && SM_CAP >= SAMPLE_MAX_K && SM_BINS == 16 * SM_TH, "sampler geometry");

// monotone key of a logit: the argmax key's high word (pick.h) with -0 made +0
__device__ __forceinline__ uint32_t logit_key(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (u == 0x80000000u) u = 0;
    return ordered_bits(u);
}
__device__ __forceinline__ int sample_k(const sampler_params &p, int64_t n) {
    const int k = p.top_k > 0 ? p.top_k : SAMPLE_MAX_K;
    return (int)(n < (int64_t)k ? n : (int64_t)k);
}

// All three kernels: grid.y = the row of the pass.  A row's logits are lg + row * ld and its
// workspace the row-th of each sample_ws array; the offsets are wave-uniform (scalar registers).
// the row's parameters: its table entry's, else the launch's one struct
__device__ __forceinline__ sampler_params row_params(const sampler_params *prm, const slot_row *tab) {
    return tab ? tab[blockIdx.y].smp : *prm;
}

__global__ void __launch_bounds__(SM_TH) k_sample_hist(const float *lg, int64_t ld, int64_t n, const slot_row *tab,
                                                       unsigned *ghist) {
    __shared__ unsigned h[SM_BINS];
    const int tid = threadIdx.x;
    // a greedy row of a mixed pass leaves here (rows without a table always sample, nothing is read)
    if (tab && !(tab[blockIdx.y].smp.temperature > 0.0f)) return;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    ghist += (int64_t)blockIdx.y * SAMPLE_WS_HIST;
    for (int i = tid; i < SM_BINS; i += SM_TH) h[i] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * SM_CHUNK; base < n; base += (int64_t)gridDim.x * SM_CHUNK) {
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            const int64_t i = base + k * SM_TH + tid;
            if (i < n) atomicAdd(&h[logit_key(row[i]) >> SM_SHIFT], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < SM_BINS; i += SM_TH) {
        const unsigned c = h[i];
        if (c) atomicAdd(&ghist[i], c);
    }
}

__global__ void __launch_bounds__(SM_TH) k_sample_compact(const float *lg, int64_t ld, int64_t n, const sampler_params *prm,
                                                          const slot_row *tab, const unsigned *ghist, unsigned *cur,
                                                          unsigned long long *list_a, unsigned long long *list_b,
                                                          int64_t cap_b) {
    __shared__ unsigned wtot[SM_TH / 64];
    __shared__ unsigned s_bin, s_cnt[2], s_base[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.y;
    const float *row = lg + r * ld;
    ghist += r * SAMPLE_WS_HIST;
    cur += r * SAMPLE_WS_HIST;
    list_a += r * SAMPLE_MAX_K;
    list_b += r * cap_b;
    const sampler_params P = row_params(prm, tab);
    if (tab && !(P.temperature > 0.0f)) return;  // a greedy row: before the first barrier and atomic
    const unsigned K = (unsigned)sample_k(P, n);
    // b*: the bin with (entries in bins above it) < K <= (those + its own); thread t owns bins 16t .. 16t+15
    unsigned loc[16], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = *(const uint4 *)(ghist + tid * 16 + q * 4);
        loc[4 * q] = v.x; loc[4 * q + 1] = v.y; loc[4 * q + 2] = v.z; loc[4 * q + 3] = v.w;
        sum += v.x + v.y + v.z + v.w;
    }
    unsigned incl = sum;  // this thread's bins and those of the wave's higher threads
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_down(incl, off);
        if (lane + off < 64) incl += v;
    }
    if (lane == 0) wtot[wave] = incl;
    if (tid == 0) s_bin = 0;
    __syncthreads();
    unsigned above = incl - sum;
    for (int w = wave + 1; w < SM_TH / 64; ++w) above += wtot[w];
    if (above < K && K <= above + sum) {  // exactly one thread
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            if (above + loc[j] >= K) {
                s_bin = (unsigned)(tid * 16 + j);
                break;
            }
            above += loc[j];
        }
    }
    __syncthreads();
    const unsigned bsel = s_bin;
    for (int64_t base = (int64_t)blockIdx.x * SM_CHUNK; base < n; base += (int64_t)gridDim.x * SM_CHUNK) {
        if (tid < 2) s_cnt[tid] = 0;
        __syncthreads();
        unsigned long long comp[SM_PER];
        int slot[SM_PER];  // -1: not kept; bit 30: list B
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            const int64_t i = base + k * SM_TH + tid;
            slot[k] = -1;
            if (i < n) {
                const uint32_t key = logit_key(row[i]);
                const unsigned bin = key >> SM_SHIFT;
                comp[k] = pack_key(key, i);
                if (bin > bsel) slot[k] = (int)atomicAdd(&s_cnt[0], 1u);
                else if (bin == bsel) slot[k] = (int)atomicAdd(&s_cnt[1], 1u) | (1 << 30);
            }
        }
        __syncthreads();
        if (tid < 2 && s_cnt[tid]) s_base[tid] = atomicAdd(&cur[tid], s_cnt[tid]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            if (slot[k] < 0) continue;
            const bool b = (slot[k] >> 30) & 1;
            const int64_t at = (int64_t)s_base[b ? 1 : 0] + (slot[k] & ((1 << 30) - 1));
            if (b) {
                if (at < cap_b) list_b[at] = comp[k];
            } else if (at < SAMPLE_MAX_K) {
                list_a[at] = comp[k];
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint64_t splitmix64_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(SM_TAIL) k_sample_tail(const sampler_params *prm, const int *pos, const slot_row *tab, int64_t n,
                                                         unsigned *ghist, unsigned *cur, const unsigned long long *list_a,
                                                         const unsigned long long *list_b, int64_t cap_b,
                                                         unsigned long long *key_out, int key_parts, sample_dbg dbg) {
    const sampler_params P = row_params(prm, tab);
    if (tab && !(P.temperature > 0.0f)) return;  // a greedy row: workspace and key slot untouched
    {  // this row's position word, workspace, key slot and debug outputs
        const int64_t r = blockIdx.y;
        pos = tab ? tab[r].pos : pos + r;
        ghist += r * SAMPLE_WS_HIST;
        cur += r * SAMPLE_WS_HIST;
        list_a += r * SAMPLE_MAX_K;
        list_b += r * cap_b;
        key_out += r * key_parts;
        if (dbg.token) dbg.token += r;
        if (dbg.n_cand) dbg.n_cand += r;
        if (dbg.n_kept) dbg.n_kept += r;
        if (dbg.cand) dbg.cand += r * SAMPLE_MAX_K;
    }
    __shared__ unsigned long long ks[SM_CAP];
    __shared__ double cs[SM_TAIL];
    __shared__ double wtot[SM_TAIL / 64];
    __shared__ unsigned hist[256];
    __shared__ unsigned s_d, s_rem, s_cnt, s_cursor;
    __shared__ int s_m, s_j;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = sample_k(P, n);
    const int p = *pos + 1;
    const unsigned ca = cur[0], cb = cur[1];
    const int n_a = (int)(ca < (unsigned)SAMPLE_MAX_K ? ca : (unsigned)SAMPLE_MAX_K);
    const int64_t n_b = (int64_t)cb < cap_b ? (int64_t)cb : cap_b;
    __syncthreads();  // every thread has read the cursors
    for (int i = tid; i < SM_BINS; i += SM_TAIL) ghist[i] = 0;  // scratch ready for the next call
    if (tid < 2) cur[tid] = 0;

    for (int i = tid; i < n_a; i += SM_TAIL) ks[i] = list_a[i];
    int n_s;
    if (n_a + n_b <= SM_CAP) {
        for (int i = tid; i < (int)n_b; i += SM_TAIL) ks[n_a + i] = list_b[i];
        n_s = n_a + (int)n_b;
    } else {
        // B narrowed to its `need` largest entries (entries are unique): MSB-first radix select of
        // the need-th largest, 8 bits a pass, until the entries that share the prefix are all kept
        unsigned need = K > n_a ? (unsigned)(K - n_a) : 0u;
        if ((int64_t)need > n_b) need = (unsigned)n_b;
        unsigned long long prefix = 0, mask = 0;
        unsigned rem = need;
        for (int shift = 56; shift >= 0 && rem > 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < n_b; i += SM_TAIL) {
                const unsigned long long v = list_b[i];
                if ((v & mask) == prefix) atomicAdd(&hist[(unsigned)(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0;
                int d = 255;
                for (; d > 0; --d) {
                    if (cum + hist[d] >= rem) break;
                    cum += hist[d];
                }
                s_d = (unsigned)d;
                s_rem = rem - cum;
                s_cnt = hist[d];
            }
            __syncthreads();
            prefix |= (unsigned long long)s_d << shift;
            mask |= 255ull << shift;
            rem = s_rem;
            const unsigned cnt = s_cnt;
            __syncthreads();
            if (cnt == rem) break;
        }
        if (tid == 0) s_cursor = 0;
        __syncthreads();
        if (need > 0) {
            for (int64_t i = tid; i < n_b; i += SM_TAIL) {
                const unsigned long long v = list_b[i];
                if ((v & mask) >= prefix) {
                    const unsigned at = atomicAdd(&s_cursor, 1u);
                    if (n_a + (int)at < SM_CAP && at < need) ks[n_a + at] = v;
                }
            }
        }
        __syncthreads();
        const unsigned got = s_cursor < need ? s_cursor : need;
        n_s = n_a + (int)got;
    }
    // the histogram and the lists agree, so n_s >= K; were the scratch ever clobbered, never hand
    // k_advance an index outside the row: fewer candidates, or token 0
    const int Ke = K < n_s ? K : n_s;
    if (Ke <= 0) {
        if (tid < key_parts) key_out[tid] = tid == 0 ? 0x80000000FFFFFFFFull : 0ull;
        return;
    }
    int P2 = 2;
    while (P2 < n_s) P2 <<= 1;
    for (int i = n_s + tid; i < P2; i += SM_TAIL) ks[i] = 0;  // below every entry (a NaN's key)
    __syncthreads();
    // bitonic sort, descending
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2 / 2; t += SM_TAIL) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = ks[i], b = ks[l];
                const bool desc = (i & k) == 0;
                if (desc ? a < b : a > b) {
                    ks[i] = b;
                    ks[l] = a;
                }
            }
            __syncthreads();
        }
    }
    // weights (f64) and their prefix sums: thread i = candidate i
    const float l0 = key_value(ks[0]);
    double w = 0.0;
    if (tid < Ke) {
        const float li = key_value(ks[tid]);
        w = exp(((double)li - (double)l0) / (double)P.temperature);
    }
    double incl = w;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    if (tid == 0) s_m = Ke;
    __syncthreads();
    double pre = 0.0;
    for (int q = 0; q < wave; ++q) pre += wtot[q];
    const double c_i = pre + incl;
    cs[tid] = c_i;
    __syncthreads();
    const double W = cs[Ke - 1];
    if (P.top_p != 1.0f && tid < Ke) {
        const double thr = (double)P.top_p * W;
        if (c_i >= thr && (tid == 0 || cs[tid - 1] < thr)) s_m = tid + 1;
    }
    __syncthreads();
    const int m = s_m;
    if (tid == 0) s_j = m - 1;
    __syncthreads();
    const uint64_t z = P.seed + (uint64_t)(int64_t)(p + 1) * 0x9E3779B97F4A7C15ull;
    const double u = (double)(splitmix64_mix(z) >> 11) * 0x1.0p-53;
    const double r = u * cs[m - 1];
    if (tid < m && c_i > r && (tid == 0 || cs[tid - 1] <= r)) s_j = tid;
    __syncthreads();
    const unsigned long long pick = ks[s_j];
    // (key_parts > 1: the rest of the row's partial keys become key 0, below every candidate)
    if (tid < key_parts) key_out[tid] = tid == 0 ? pick : 0ull;
    if (tid == 0) {
        if (dbg.token) *dbg.token = key_index(pick);
        if (dbg.n_cand) *dbg.n_cand = Ke;
        if (dbg.n_kept) *dbg.n_kept = m;
    }
    if (dbg.cand) dbg.cand[tid] = tid < Ke ? key_index(ks[tid]) : -1;
}

}  // namespace

int sample_ws_alloc(dev_pool &mem, sample_ws *w, int64_t n_vocab, hipStream_t s, int rows) {
    if (n_vocab <= 0 || n_vocab > 0x7FFFFFFFll || rows < 1) {
        set_error("sampler: n_vocab or rows out of range");
        return -1;
    }
    *w = sample_ws{};
    w->cap_b = n_vocab;
    const size_t R = (size_t)rows;
    if (mem.get_zeroed(&w->hist, R * SAMPLE_WS_HIST * 4, s) || mem.get(&w->list_a, R * SAMPLE_MAX_K * 8) ||
        mem.get(&w->list_b, R * (size_t)n_vocab * 8) || mem.get_zeroed(&w->key, R * 8, s)) {
        sample_ws_free(mem, w);
        return -1;
    }
    w->cur = w->hist + SM_BINS;
    w->rows = rows;
    return 0;
}

void sample_ws_free(dev_pool &mem, sample_ws *w) {
    mem.put(w->hist);
    mem.put(w->list_a);
    mem.put(w->list_b);
    mem.put(w->key);
    *w = sample_ws{};
}

int launch_sample(const float *lg, int64_t ld, int rows, int64_t n, const sampler_params *prm, const int *pos,
                  const slot_row *tab, const sample_ws &w, const sample_dbg &dbg, hipStream_t s, int key_parts) {
    if (!w.hist || n <= 0 || n > w.cap_b || rows < 1 || rows > w.rows || (!pos && !tab) || (!prm && !tab) || key_parts < 1 ||
        key_parts > SM_TAIL) {
        set_error("sampler: scratch not sized for these rows");
        return -1;
    }
    const int grid = (int)std::min<int64_t>((n + SM_CHUNK - 1) / SM_CHUNK, SM_GRID_MAX);
    hipLaunchKernelGGL(k_sample_hist, dim3(grid, rows), dim3(SM_TH), 0, s, lg, ld, n, tab, w.hist);
    hipLaunchKernelGGL(k_sample_compact, dim3(grid, rows), dim3(SM_TH), 0, s, lg, ld, n, prm, tab, (const unsigned *)w.hist,
                       w.cur, w.list_a, w.list_b, w.cap_b);
    hipLaunchKernelGGL(k_sample_tail, dim3(1, rows), dim3(SM_TAIL), 0, s, prm, pos, tab, n, w.hist, w.cur,
                       (const unsigned long long *)w.list_a, (const unsigned long long *)w.list_b, w.cap_b, w.key, key_parts, dbg);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_picks(int mix, const float *lg, int64_t ld, int rows, int64_t n, const sampler_params *prm, const int *pos,
                 const slot_row *tab, const sample_ws &w, unsigned long long *keys, int rows_cap, const sample_dbg &dbg,
                 hipStream_t s, const unsigned long long **out_keys, int *out_parts, int *out_stride) {
    if (!keys || rows < 1 || rows > rows_cap || mix < PICKS_GREEDY || mix > PICKS_MIXED) {
        set_error("picks: no key buffer, or a pass outside its rows");
        return -1;
    }
    constexpr int PARTS = 256;  // the row argmax's partial keys per row
    if (mix != PICKS_SAMPLE && launch_row_argmax(lg, n, keys, PARTS, s, rows, ld)) return -1;
    if (mix == PICKS_GREEDY || mix == PICKS_MIXED) {
        *out_keys = keys; *out_parts = PARTS; *out_stride = PARTS;
    }
    if (mix == PICKS_GREEDY) return 0;
    sample_ws v = w;
    v.key = mix == PICKS_MIXED ? keys : keys + (size_t)rows_cap * PARTS;
    if (launch_sample(lg, ld, rows, n, prm, pos, tab, v, dbg, s, mix == PICKS_MIXED ? PARTS : 1)) return -1;
    if (mix == PICKS_SAMPLE) {
        *out_keys = v.key; *out_parts = 1; *out_stride = 1;
    }
    return 0;
}

}  // namespace ghip
